// Host drivers of the graph-algorithm consumers (kernels: pma_consumer.h, pma_scan.h, pma_paths.h, pma_cores.h, pma_centrality.h,
// pma_scc.h, pma_msf.h, pma_intersect.h, pma_truss.h, pma_sample.h, pma_msbfs.h, pma_colour.h, pma_community.h).  Included at the end of engine.cc: part of the engine's single translation unit, in the library
// (csrc/ppcsr_hip.hip) and in the emulator (tests/hostsim/ppcsr_sim.cpp) alike.
namespace ppcsr {

// The consumers run over a table of gapped arrays (pma_consumer.h: ConsumerPart) — a PPPCSR's partitions, or one engine alone —
// on this engine's stream.  The partitions' own streams must be idle first: their last batch may still be in flight.
// *slots = slots of all arrays; the table goes to the device (one copy, into *d_tab) unless d_tab is null.  alloc_code: the status
// of a table that cannot be allocated (ConsumerScope::alloc_code).
int Engine::consumer_table(const ConsumerRef *parts, uint32_t P, uint32_t total_n, void **d_tab, uint64_t *slots, int alloc_code) {
  Impl &p = *p_;
  std::vector<ConsumerPart> tab(P + 1);
  uint64_t chunks = 0, tot = 0;
  for (uint32_t k = 0; k < P; k++) {
    const Impl &q = *parts[k].e->p_;
    if (parts[k].e != this) GCHK(gpu::sync(q.stream));
    tab[k] = ConsumerPart{q.v.items, q.v.nodes, q.v.g.N, chunks, q.v.g.n, parts[k].first, {0, 0}};
    chunks += (q.v.g.N + 63) / 64;
    tot += q.v.g.N;
  }
  tab[P] = ConsumerPart{nullptr, nullptr, 0, chunks, 0, total_n, {0, 0}};
  *slots = tot;
  if (!d_tab) return PPCSR_OK;
  const int oom = gpu::dmalloc(d_tab, (P + 1) * sizeof(ConsumerPart));
  if (oom != 0) return fail(alloc_code, std::string("device allocation of the consumer table: ") + gpu::err_str(oom));
  GCHK(gpu::h2d(*d_tab, tab.data(), (P + 1) * sizeof(ConsumerPart), p.stream));
  GCHK(gpu::sync(p.stream));
  return PPCSR_OK;
}

// Triangle counts and common-neighbour counts intersect vertex ranges as sorted lists, which holds in the regular regime
// only: a partition in the sequential regime (narrow == 0: ranges may be unsorted or overlapping until the next re-check) is
// refused rather than answered on a wrong assumption.
int Engine::intersect_regime(const ConsumerRef *parts, uint32_t P, const char *what, std::string *msg) {
  for (uint32_t k = 0; k < P; k++)
    if (parts[k].e->p_->v.g.narrow == 0u) {
      *msg = std::string(what) + ": the structure is in the sequential regime (add_node after a doubling: vertex ranges may be unsorted "
             "or overlapping, stats.narrow == 0) and sorted ranges cannot be intersected; it ends at the next range re-check";
      return PPCSR_EUNSUPPORTED;
    }
  return PPCSR_OK;
}

// One consumer call: what every *_over does before and after its own launches.  open() selects the device, refuses the
// sequential regime for a consumer that intersects, and builds the table; alloc() hands out the call's device buffers, all of
// which are freed on every exit path; stream() and the three grids are what the call's launches go out with; read_back() is a
// host read in the middle of the call; start() / stop() / done() run the timer and hand device_ms out.
struct Engine::ConsumerScope {
  Engine &eng;
  Impl &p;
  std::vector<void *> bufs;
  const ConsumerPart *tab_ = nullptr;
  uint64_t slots_ = 0;
  uint32_t n_ = 0;
  int rc = PPCSR_OK;  // the first allocation that failed (later ones are not tried)
  const int alloc_code;  // its status: PPCSR_EHIP from the earlier consumers, PPCSR_ENOMEM from edge_support / ktruss

  explicit ConsumerScope(Engine *e, int alloc_status = PPCSR_EHIP) : eng(*e), p(*e->p_), alloc_code(alloc_status) {}
  ConsumerScope(const ConsumerScope &) = delete;  // (it owns the buffers; a launch's arguments are copies of plain pointers)
  ~ConsumerScope() {
    for (void *b : bufs) gpu::dfree(b);
  }
  int fail(int code, const std::string &msg) { return eng.fail(code, msg); }
  // intersects: the consumer's name when it needs sorted, disjoint vertex ranges
  int open(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const char *intersects = nullptr, bool device_table = true) {
    GCHK(gpu::set_device(eng.device_));
    std::string msg;
    if (intersects && eng.intersect_regime(parts, P, intersects, &msg) != PPCSR_OK) return fail(PPCSR_EUNSUPPORTED, msg);
    n_ = total_n;
    void *d_tab = nullptr;
    const int e = eng.consumer_table(parts, P, total_n, device_table ? &d_tab : nullptr, &slots_, alloc_code);
    if (d_tab) bufs.push_back(d_tab);
    tab_ = static_cast<const ConsumerPart *>(d_tab);
    return e;
  }
  const ConsumerPart *table() const { return tab_; }
  uint64_t slots() const { return slots_; }  // slots of all arrays: what one streaming pass reads
  uint64_t words() const { return std::max<uint64_t>(n_, 1); }  // length of a per-vertex buffer (never an empty allocation)
  gpu::stream_t stream() const { return p.stream; }
  // a streaming pass (cp_stream: a wave per four 64-slot chunks, four waves per workgroup), a per-vertex launch (a thread per
  // vertex), a launch with a wave per entry of a list
  uint32_t pass_grid() const { return grid_for((slots_ + 255) / 256, 4, 8192); }
  uint32_t vert_grid() const { return grid_for(n_, 256, 4096); }
  uint32_t list_grid(uint64_t count) const { return grid_for(count, 4, 16384); }
  template <class T>
  T *alloc(const char *what, uint64_t count) {
    void *b = nullptr;
    if (rc != PPCSR_OK) return nullptr;
    const int e = gpu::dmalloc(&b, count * sizeof(T));
    if (e != 0) {
      rc = fail(alloc_code, std::string("device allocation of ") + what + ": " + gpu::err_str(e));
      return nullptr;
    }
    bufs.push_back(b);
    return static_cast<T *>(b);
  }
  // a host read in the middle of the call: the copy, the wait for it, and whatever error a launch before it has left
  int read_back(void *dst, const void *src, uint64_t bytes) {
    GCHK(gpu::d2h(dst, src, bytes, p.stream));
    GCHK(gpu::sync(p.stream));
    GCHK(gpu::last_error());
    return PPCSR_OK;
  }
  void start() { p.timer.start(p.stream); }
  void stop() { p.timer.stop(p.stream); }
  int done(double *device_ms) {
    GCHK(gpu::sync(p.stream));
    GCHK(gpu::last_error());
    if (device_ms) *device_ms = p.timer.ms();
    return PPCSR_OK;
  }

  // The striped counters of a call (cp_striped_add): kBfsStripes stripes, kWords words of T apart, word w of every stripe one
  // counter — behind kLead words of the call's own.  The device block (one allocation, made where the object is constructed)
  // and its host mirror: zero() clears the block, read() is ONE host read of all of it, sum(w) adds counter w up from the
  // mirror and lead(i) is word i of the leading ones.
  template <class T, uint32_t kWords, uint32_t kLead = 0>
  struct Striped {
    static constexpr uint32_t kCount = kLead + kBfsStripes * kWords;
    ConsumerScope &cs;
    T *dev;
    std::vector<T> host;
    Striped(ConsumerScope &scope, const char *what) : cs(scope), dev(scope.alloc<T>(what, kCount)), host(kCount, 0) {}
    T *stripes() const { return dev + kLead; }
    int zero() { return gpu::dset(dev, 0, kCount * sizeof(T), cs.p.stream); }
    int read() { return cs.read_back(host.data(), dev, kCount * sizeof(T)); }
    T lead(uint32_t i) const { return host[i]; }
    uint64_t sum(uint32_t w = 0) const {
      uint64_t all = 0;
      for (uint32_t k = 0; k < kBfsStripes; k++) all += host[kLead + (uint64_t)k * kWords + w];
      return all;
    }
  };
  // counter block of the hybrid loop: [0] vertices found, [1] a hub was left to the streaming pass, then the streaming pass's
  // striped count
  typedef Striped<uint32_t, kBfsStripeWords, kBfsStripeWords> HybridCounters;

  // The hybrid loop of bfs_over and sssp_over, from a frontier of one vertex (in d_f0) at step `step` until a step finds
  // nothing.  A small frontier is expanded one wave per vertex (per_vertex(cur, nfront, step, nxt): builds the next frontier
  // list); a frontier that is a sizeable share of the graph is expanded by one streaming pass over every gapped array
  // (pass(step)) — its cost does not depend on hub degrees — and the list is rebuilt from d_key (levels / stamps: the
  // frontier is { v : key[v] == step }) only when the frontier becomes small again.  One host read per step.
  // reread_list: the pass's count is an upper bound (BFS counts claims), so the exact length is read back with the list;
  // an exact count (SSSP: the stamp admits each vertex once) is not read again.  sizes (may be null): the frontier size of
  // every step is appended to it — exact where the count is.
  static uint32_t hybrid_big(uint32_t nn) { return (uint32_t)std::max<uint64_t>(64, (uint64_t)nn / 256); }
  template <class Pass, class PerVertex>
  int hybrid(uint32_t nn, const uint32_t *d_key, uint32_t step, uint32_t *d_f0, uint32_t *d_f1, HybridCounters &cnt, bool reread_list, Pass pass,
             PerVertex per_vertex, std::vector<uint32_t> *sizes = nullptr) {
    uint32_t nfront = 1;
    uint32_t *cur = d_f0, *nxt = d_f1;
    uint32_t *const d_cnt = cnt.dev;
    bool have_list = true;
    const uint32_t big = hybrid_big(nn);  // frontier size from which the pass is cheaper
    for (; nfront > 0; step++) {
      if (sizes) sizes->push_back(nfront);
      GCHK(cnt.zero());
      if (nfront >= big) {
        pass(step);
        have_list = false;
      } else {
        if (!have_list) {
          GPU_LAUNCH(p.stream, k_bfs_collect, grid_for(nn, 256), 256, d_key, nn, step, cur, d_cnt);
          if (reread_list) {
            GCHK(gpu::d2h(cnt.host.data(), d_cnt, sizeof(uint32_t), p.stream));
            GCHK(gpu::sync(p.stream));
            nfront = cnt.lead(0);
          }
          GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), p.stream));
        }
        per_vertex((const uint32_t *)cur, nfront, step, nxt);
        have_list = true;
        std::swap(cur, nxt);
      }
      int e = cnt.read();
      if (e != PPCSR_OK) return e;
      if (cnt.lead(1)) {  // hubs of this step were skipped by the per-vertex kernel: one pass finishes the step
        pass(step);
        e = cnt.read();
        if (e != PPCSR_OK) return e;
        have_list = false;
      }
      nfront = cnt.lead(0) + (uint32_t)cnt.sum();
    }
    return PPCSR_OK;
  }

  // The loop of a sweep BACK over levels whose sizes a hybrid() run recorded: from the last level but one down to level 0,
  // the same choice per level.  A level of at least hybrid_big vertices takes one streaming pass (pass(level, false)); a
  // smaller one is listed from d_key (k_bfs_collect) and handled one wave per vertex (per_vertex(list, count, level)), and if
  // that launch left hubs behind (d_cnt[1]) one pass over those alone finishes the level (pass(level, true)).  One host read
  // per small level.
  template <class Pass, class PerVertex>
  int sweep_back(uint32_t nn, const uint32_t *d_key, const std::vector<uint32_t> &sizes, uint32_t *d_list, uint32_t *d_cnt, Pass pass,
                 PerVertex per_vertex) {
    const uint32_t big = hybrid_big(nn);
    uint32_t h_cnt[2] = {0, 0};
    for (uint64_t level = sizes.size() - 1; level-- > 0;) {
      if (sizes[level] >= big) {
        pass((uint32_t)level, false);
        continue;
      }
      GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), p.stream));
      GPU_LAUNCH(p.stream, k_bfs_collect, grid_for(nn, 256), 256, d_key, nn, (uint32_t)level, d_list, d_cnt);
      per_vertex((const uint32_t *)d_list, sizes[level], (uint32_t)level);
      const int e = read_back(h_cnt, d_cnt, 2 * sizeof(uint32_t));
      if (e != PPCSR_OK) return e;
      if (h_cnt[1]) pass((uint32_t)level, true);
    }
    return PPCSR_OK;
  }

  // Stage 1 of pma_cores.h, shared by kcore_over and colouring_over: from the cleared deg[] / fill[] to the compact symmetric
  // adjacency of G.  The degree pass, the three launches of the scan (off[n] = 2 |E(G)|), the host read of that total, the
  // allocation of the lists (the call's alloc_code when it fails), the fill pass.  *adj: the lists; *entries: their length.
  int symmetric_adjacency(uint32_t P, uint32_t *d_deg, uint32_t *d_fill, unsigned long long *d_off, unsigned long long *d_tiles, uint32_t ntiles,
                          uint32_t **adj, uint64_t *entries) {
    const uint32_t nn = n_;
    GPU_LAUNCH(p.stream, k_kc_degree, pass_grid(), 256, tab_, P, nn, d_deg);
    GPU_LAUNCH(p.stream, k_kc_tile_sums, grid_for(ntiles, 1, 65536), 256, (const uint32_t *)d_deg, nn, ntiles, d_tiles);
    GPU_LAUNCH(p.stream, k_kc_scan_tiles, 1, 64, d_tiles, ntiles, d_off + nn);
    GPU_LAUNCH(p.stream, k_kc_scan_write, grid_for(ntiles, 1, 65536), 256, (const uint32_t *)d_deg, nn, ntiles, (const unsigned long long *)d_tiles, d_off);
    unsigned long long total = 0;
    const int e = read_back(&total, d_off + nn, sizeof(total));
    if (e != PPCSR_OK) return e;
    uint32_t *d_adj = alloc<uint32_t>("d_adj", std::max<uint64_t>(total, 1));
    if (rc != PPCSR_OK) return rc;
    GPU_LAUNCH(p.stream, k_kc_fill, pass_grid(), 256, tab_, P, nn, (const unsigned long long *)d_off, d_fill, d_adj);
    *adj = d_adj;
    *entries = total;
    return PPCSR_OK;
  }

  // The device side of colouring_over, shared with label_propagation_over, which needs the adjacency and the colours ON THE
  // DEVICE: the buffers (colour_alloc: eleven allocations, in this order), and from the cleared buffers to the last round
  // (colour_run; n > 0).  Afterwards d_deg, d_off, d_adj (2 |E(G)| = ctr[3] entries) and d_col hold the graph and the answer;
  // d_fill equals d_deg; d_pred, d_f0, d_f1, d_long, d_key, d_tiles and d_cnt are free.  ctr: the counters of
  // ppcsr_debug_colouring_counters.
  struct ColourStage {
    uint32_t *d_deg = nullptr, *d_col = nullptr, *d_fill = nullptr, *d_pred = nullptr, *d_f0 = nullptr, *d_f1 = nullptr, *d_long = nullptr;
    unsigned long long *d_key = nullptr, *d_off = nullptr, *d_tiles = nullptr;
    uint32_t *d_cnt = nullptr, *d_adj = nullptr;
    uint32_t ntiles = 0;
    uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  };
  void colour_alloc(ColourStage *st) {
    const uint64_t w = words();
    st->ntiles = (uint32_t)(((uint64_t)n_ + kKcTile - 1) / kKcTile);
    st->d_deg = alloc<uint32_t>("d_deg", w), st->d_col = alloc<uint32_t>("d_col", w), st->d_fill = alloc<uint32_t>("d_fill", w);
    st->d_pred = alloc<uint32_t>("d_pred", w);
    st->d_f0 = alloc<uint32_t>("d_f0", w), st->d_f1 = alloc<uint32_t>("d_f1", w);  // (a vertex enters one frontier once: no list exceeds n)
    st->d_long = alloc<uint32_t>("d_long", w);
    st->d_key = alloc<unsigned long long>("d_key", w);
    st->d_off = alloc<unsigned long long>("d_off", w + 1), st->d_tiles = alloc<unsigned long long>("d_tiles", std::max<uint64_t>(st->ntiles, 1));
    st->d_cnt = alloc<uint32_t>("d_cnt", kColCntWords);
  }
  int colour_run(uint32_t P, uint32_t order, uint64_t seed, ColourStage *st) {
    const uint32_t nn = n_;
    const uint64_t w = words();
    uint32_t *const d_deg = st->d_deg, *const d_col = st->d_col, *const d_fill = st->d_fill, *const d_pred = st->d_pred, *const d_long = st->d_long;
    uint32_t *const d_cnt = st->d_cnt;
    unsigned long long *const d_key = st->d_key, *const d_off = st->d_off;
    const uint32_t window = p.colour_window;
    uint64_t(&ctr)[8] = st->ctr;
    uint64_t &rounds = ctr[0], &launches = ctr[6], &reads = ctr[7];
    uint32_t h_cnt[4] = {0, 0, 0, 0};  // next frontier, deferred lists, extra window passes, the largest colour
    const auto read_cnt = [&](uint32_t nwords) {
      reads++;
      return read_back(h_cnt, d_cnt, nwords * sizeof(uint32_t));
    };
    // stage 1: deg[], off[] (off[nn] = 2 |E(G)|), adj[]
    GCHK(gpu::dset(d_deg, 0, w * sizeof(uint32_t), p.stream));
    GCHK(gpu::dset(d_fill, 0, w * sizeof(uint32_t), p.stream));
    GCHK(gpu::dset(d_pred, 0, w * sizeof(uint32_t), p.stream));
    GCHK(gpu::dset(d_cnt, 0, kColCntWords * sizeof(uint32_t), p.stream));
    GPU_LAUNCH(p.stream, k_kc_init, vert_grid(), 256, d_col, nn);
    uint32_t *d_adj = nullptr;
    int e = symmetric_adjacency(P, d_deg, d_fill, d_off, st->d_tiles, st->ntiles, &d_adj, &ctr[3]);
    if (e != PPCSR_OK) return e;
    st->d_adj = d_adj;
    reads++;
    // the order, pred[] and the first frontier
    GPU_LAUNCH(p.stream, k_col_keys, vert_grid(), 256, order, (unsigned long long)seed, (const uint32_t *)d_deg, nn, d_key);
    GPU_LAUNCH(p.stream, k_col_pred, pass_grid(), 256, tab_, P, nn, (const unsigned long long *)d_key, d_pred);
    uint32_t *cur = st->d_f0, *nxt = st->d_f1;
    GPU_LAUNCH(p.stream, k_col_collect, grid_for(nn, 256), 256, (const uint32_t *)d_pred, nn, cur, d_cnt);
    launches += 9;  // (k_kc_init, the five of stage 1, these three)
    e = read_cnt(1);
    if (e != PPCSR_OK) return e;
    uint64_t done = 0;
    for (uint32_t nfront = h_cnt[0]; nfront > 0; nfront = h_cnt[0]) {
      if (rounds == nn) return fail(PPCSR_EHIP, "colouring: more rounds than the graph has vertices");
      rounds++;
      done += nfront;
      ctr[1] = std::max<uint64_t>(ctr[1], nfront);
      GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), p.stream));
      GPU_LAUNCH(p.stream, k_col_round, list_grid(nfront), 256, (const unsigned long long *)d_off, (const uint32_t *)d_adj, (const uint32_t *)cur,
                 nfront, d_col, d_pred, nxt, d_long, d_cnt);
      launches++;
      e = read_cnt(4);
      if (e != PPCSR_OK) return e;
      if (h_cnt[1]) {  // lists beyond one wave's reach: a workgroup each, appending to the same frontier
        ctr[2] += h_cnt[1];
        GPU_LAUNCH(p.stream, k_col_long, grid_for(h_cnt[1], 1, 1024), 256, (const unsigned long long *)d_off, (const uint32_t *)d_adj,
                   (const uint32_t *)d_long, h_cnt[1], window, d_col, d_pred, nxt, d_cnt);
        launches++;
        e = read_cnt(4);
        if (e != PPCSR_OK) return e;
      }
      std::swap(cur, nxt);
    }
    if (done != nn) return fail(PPCSR_EHIP, "colouring: the rounds ended with vertices left uncoloured");
    ctr[4] = (uint64_t)h_cnt[3] + 1;
    ctr[5] = h_cnt[2];
    return PPCSR_OK;
  }

  // sample_over / walks_over: the hubs among d_q[0, k) (d_q == nullptr: among all vertices) and their measure prefix
  int sample_hubs(uint32_t P, const uint32_t *d_q, uint64_t k, bool weighted, SmHubs *hb);
};

// bfs.h:15-36: level of every vertex from `start` (UINT32_MAX = unreachable); one launch per level, whatever the number of arrays
int Engine::bfs_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint32_t *levels, double *device_ms) {
  const uint32_t nn = total_n;
  if (start >= nn) return fail(PPCSR_EINVAL, "bfs: start vertex out of range");  // (refused before the device is even selected)
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t bit_words = ((uint64_t)nn + 63) / 64 * 2;  // frontier / visited bitmaps of the streaming levels
  uint32_t *d_fb = cs.alloc<uint32_t>("d_fb", bit_words), *d_vb = cs.alloc<uint32_t>("d_vb", bit_words);
  uint32_t *d_lv = cs.alloc<uint32_t>("d_lv", nn), *d_f0 = cs.alloc<uint32_t>("d_f0", nn), *d_f1 = cs.alloc<uint32_t>("d_f1", nn);
  ConsumerScope::HybridCounters cnt(cs, "d_cnt");
  uint32_t *const d_cnt = cnt.dev, *const d_found = cnt.stripes();  // (a launch's arguments are plain pointers)
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  GCHK(gpu::dset(d_lv, 0xFF, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  const uint32_t zero = 0;
  GCHK(gpu::h2d(d_lv + start, &zero, sizeof(uint32_t), cs.stream()));
  GCHK(gpu::h2d(d_f0, &start, sizeof(uint32_t), cs.stream()));
  rc = cs.hybrid(
      nn, d_lv, 0, d_f0, d_f1, cnt, true,
      [&](uint32_t level) {
        GPU_LAUNCH(cs.stream(), k_bfs_bits, cs.vert_grid(), 256, (const uint32_t *)d_lv, nn, level, d_fb, d_vb);
        GPU_LAUNCH(cs.stream(), k_bfs_edges_bits, cs.pass_grid(), 256, tab, P, nn, level, (const uint32_t *)d_fb, (const uint32_t *)d_vb, d_lv,
                   d_found);
      },
      [&](const uint32_t *cur, uint32_t nfront, uint32_t level, uint32_t *nxt) {
        GPU_LAUNCH(cs.stream(), k_bfs_level, cs.list_grid(nfront), 256, tab, P, nn, cur, nfront, level, d_lv, nxt, d_cnt);
      });
  if (rc != PPCSR_OK) return rc;
  cs.stop();
  GCHK(gpu::d2h(levels, d_lv, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  return cs.done(device_ms);
}

// Shortest paths over the edge values (pma_paths.h).  The hybrid loop with rounds in place of levels: stamp[] holds the round
// for which a vertex was last made active, so the round's bitmap and list come from k_bfs_bits / k_bfs_collect.  The call
// ends when a round lowers no distance.
int Engine::sssp_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint64_t *dist, double *device_ms) {
  const uint32_t nn = total_n;
  if (start >= nn) return fail(PPCSR_EINVAL, "sssp: start vertex out of range");
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t bit_words = ((uint64_t)nn + 63) / 64 * 2;  // active bitmap of the streaming rounds (d_vb: k_bfs_bits' second output, unused)
  uint32_t *d_ab = cs.alloc<uint32_t>("d_ab", bit_words), *d_vb = cs.alloc<uint32_t>("d_vb", bit_words);
  unsigned long long *d_dist = cs.alloc<unsigned long long>("d_dist", nn);
  uint32_t *d_st = cs.alloc<uint32_t>("d_st", nn), *d_f0 = cs.alloc<uint32_t>("d_f0", nn), *d_f1 = cs.alloc<uint32_t>("d_f1", nn);
  ConsumerScope::HybridCounters cnt(cs, "d_cnt");
  uint32_t *const d_cnt = cnt.dev, *const d_found = cnt.stripes();  // (a launch's arguments are plain pointers)
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  GCHK(gpu::dset(d_dist, 0xFF, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
  GCHK(gpu::dset(d_st, 0, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  const unsigned long long zero = 0;
  const uint32_t round0 = 1;  // (stamp 0: never active)
  GCHK(gpu::h2d(d_dist + start, &zero, sizeof(zero), cs.stream()));
  GCHK(gpu::h2d(d_st + start, &round0, sizeof(uint32_t), cs.stream()));
  GCHK(gpu::h2d(d_f0, &start, sizeof(uint32_t), cs.stream()));
  rc = cs.hybrid(
      nn, d_st, round0, d_f0, d_f1, cnt, false,
      [&](uint32_t round) {
        GPU_LAUNCH(cs.stream(), k_bfs_bits, cs.vert_grid(), 256, (const uint32_t *)d_st, nn, round, d_ab, d_vb);
        GPU_LAUNCH(cs.stream(), k_sssp_edges, cs.pass_grid(), 256, tab, P, nn, round, (const uint32_t *)d_ab, d_dist, d_st, d_found);
      },
      [&](const uint32_t *cur, uint32_t nact, uint32_t round, uint32_t *nxt) {
        GPU_LAUNCH(cs.stream(), k_sssp_relax, cs.list_grid(nact), 256, tab, P, nn, cur, nact, round, d_dist, d_st, nxt, d_cnt);
      });
  if (rc != PPCSR_OK) return rc;
  cs.stop();
  GCHK(gpu::d2h(dist, d_dist, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
  return cs.done(device_ms);
}

// Weakly connected components (pma_paths.h): hook pass + pointer jumping until a hook pass finds no edge with two labels;
// one host read per round.
int Engine::components_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *labels, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  uint32_t *d_lab = cs.alloc<uint32_t>("d_lab", cs.words());
  ConsumerScope::Striped<uint32_t, kBfsStripeWords> cnt(cs, "d_cnt");
  const ConsumerPart *tab = cs.table();
  uint32_t *const d_cnt = cnt.dev;
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  if (nn) GPU_LAUNCH(cs.stream(), k_cc_init, cs.vert_grid(), 256, d_lab, nn);
  for (bool more = nn != 0; more;) {
    GCHK(cnt.zero());
    GPU_LAUNCH(cs.stream(), k_cc_hook, cs.pass_grid(), 256, tab, P, nn, d_lab, d_cnt);
    GPU_LAUNCH(cs.stream(), k_cc_jump, cs.vert_grid(), 256, d_lab, nn);
    const int e = cnt.read();
    if (e != PPCSR_OK) return e;
    more = cnt.sum() != 0;
  }
  cs.stop();
  if (nn) GCHK(gpu::d2h(labels, d_lab, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  return cs.done(device_ms);
}

// Shortest-path counts and betweenness centrality (pma_centrality.h).  Per source: the hybrid loop as in bfs_over, with the
// claims counted exactly (reread_list = false) and the size of every level kept; then, for betweenness, sweep_back over those
// levels and one launch that adds delta into bc.  The pass that finishes a per-vertex launch must not repeat what that launch
// has added: the launch stamps the hubs it skips with its own number (d_hub, never reset: numbers are not reused within a
// call) and the pass takes exactly those as its sources.  One host read per level forward, one per small level backward,
// one D2H of the results at the end.
int Engine::centrality_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, uint32_t *levels,
                            double *sigma, double *bc, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t words = cs.words();
  const uint64_t bit_words = std::max<uint64_t>(((uint64_t)nn + 63) / 64 * 2, 2);  // source / placed bitmaps of the streaming passes
  uint32_t *d_sb = cs.alloc<uint32_t>("d_sb", bit_words), *d_pb = cs.alloc<uint32_t>("d_pb", bit_words);
  uint32_t *d_lv = cs.alloc<uint32_t>("d_lv", words), *d_hub = cs.alloc<uint32_t>("d_hub", words);
  uint32_t *d_f0 = cs.alloc<uint32_t>("d_f0", words), *d_f1 = cs.alloc<uint32_t>("d_f1", words);
  double *d_sigma = cs.alloc<double>("d_sigma", words);
  double *d_delta = bc ? cs.alloc<double>("d_delta", words) : nullptr, *d_bc = bc ? cs.alloc<double>("d_bc", words) : nullptr;
  ConsumerScope::HybridCounters cnt(cs, "d_cnt");
  uint32_t *const d_cnt = cnt.dev, *const d_found = cnt.stripes();  // (a launch's arguments are plain pointers)
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  GCHK(gpu::dset(d_hub, 0xFF, words * sizeof(uint32_t), cs.stream()));  // (kBcNoStamp: no launch has this number)
  if (bc) GCHK(gpu::dset(d_bc, 0, words * sizeof(double), cs.stream()));
  uint32_t stamp = 0;  // number of the last per-vertex launch
  std::vector<uint32_t> sizes;
  const auto bits = [&](uint32_t level, bool hubs_only) {
    GPU_LAUNCH(cs.stream(), k_bc_bits, cs.vert_grid(), 256, (const uint32_t *)d_lv, (const uint32_t *)d_hub, nn, level,
               hubs_only ? stamp : kBcNoStamp, d_sb, d_pb);
  };
  for (uint64_t i = 0; i < k; i++) {
    const uint32_t s = sources[i];
    GPU_LAUNCH(cs.stream(), k_bc_init, cs.vert_grid(), 256, d_lv, d_sigma, d_delta, nn, s, d_f0);
    sizes.clear();
    uint32_t pv_level = kBcNoStamp;  // level of the last per-vertex launch: a pass for the same level finishes it
    rc = cs.hybrid(
        nn, d_lv, 0, d_f0, d_f1, cnt, false,
        [&](uint32_t level) {
          bits(level, level == pv_level);
          GPU_LAUNCH(cs.stream(), k_bc_edges_forward, cs.pass_grid(), 256, tab, P, nn, level, (const uint32_t *)d_sb,
                     (const uint32_t *)d_pb, d_lv, d_sigma, d_found);
        },
        [&](const uint32_t *cur, uint32_t nfront, uint32_t level, uint32_t *nxt) {
          pv_level = level;
          stamp++;
          GPU_LAUNCH(cs.stream(), k_bc_level, cs.list_grid(nfront), 256, tab, P, nn, cur, nfront, level, d_lv, d_sigma, d_hub, stamp, nxt,
                     d_cnt);
        },
        &sizes);
    if (rc != PPCSR_OK) return rc;
    if (!bc) continue;
    rc = cs.sweep_back(
        nn, d_lv, sizes, d_f0, d_cnt,
        [&](uint32_t level, bool hubs_only) {
          bits(level, hubs_only);
          GPU_LAUNCH(cs.stream(), k_bc_edges_backward, cs.pass_grid(), 256, tab, P, nn, level, (const uint32_t *)d_sb,
                     (const uint32_t *)d_lv, (const double *)d_sigma, d_delta);
        },
        [&](const uint32_t *list, uint32_t nlist, uint32_t level) {
          stamp++;
          GPU_LAUNCH(cs.stream(), k_bc_delta_vertex, cs.list_grid(nlist), 256, tab, P, nn, list, nlist, level, (const uint32_t *)d_lv,
                     (const double *)d_sigma, d_delta, d_hub, stamp, d_cnt);
        });
    if (rc != PPCSR_OK) return rc;
    GPU_LAUNCH(cs.stream(), k_bc_accumulate, cs.vert_grid(), 256, d_bc, (const double *)d_delta, nn, s);
  }
  cs.stop();
  if (levels && nn) GCHK(gpu::d2h(levels, d_lv, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  if (sigma && nn) GCHK(gpu::d2h(sigma, d_sigma, (uint64_t)nn * sizeof(double), cs.stream()));
  if (bc && nn) GCHK(gpu::d2h(bc, d_bc, (uint64_t)nn * sizeof(double), cs.stream()));
  return cs.done(device_ms);
}
int Engine::path_counts_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint32_t *levels, double *sigma,
                             double *device_ms) {
  if (start >= total_n) return fail(PPCSR_EINVAL, "path_counts: start vertex out of range");
  return centrality_over(parts, P, total_n, &start, 1, levels, sigma, nullptr, device_ms);
}
int Engine::betweenness_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, double *bc,
                             double *device_ms) {
  for (uint64_t i = 0; i < k; i++)
    if (sources[i] >= total_n) return fail(PPCSR_EINVAL, "betweenness: source vertex out of range");
  return centrality_over(parts, P, total_n, sources, k, nullptr, nullptr, bc, device_ms);
}

// Core numbers (pma_cores.h).  Stage 1 exports the upper-orientation graph as a compact symmetric adjacency (degree pass,
// scan, fill pass); stage 2 peels it level by level in sub-rounds.  One host read of the small counter block per level (the
// level and its first frontier) and per sub-round (the next frontier, the deferred long lists).  device_ms covers the whole
// call: besides the kernels it holds the host read of the edge total and the allocation of the lists between the scan and
// the fill pass, and every round trip of the peel.
int Engine::kcore_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *core, uint32_t *kmax, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const uint64_t words = cs.words();
  const uint32_t ntiles = (uint32_t)(((uint64_t)nn + kKcTile - 1) / kKcTile);
  uint32_t *d_deg = cs.alloc<uint32_t>("d_deg", words), *d_core = cs.alloc<uint32_t>("d_core", words), *d_fill = cs.alloc<uint32_t>("d_fill", words);
  uint32_t *d_f0 = cs.alloc<uint32_t>("d_f0", words), *d_f1 = cs.alloc<uint32_t>("d_f1", words);  // (a vertex enters one frontier once: no list exceeds n)
  uint32_t *d_long = cs.alloc<uint32_t>("d_long", words);
  unsigned long long *d_off = cs.alloc<unsigned long long>("d_off", words + 1), *d_tiles = cs.alloc<unsigned long long>("d_tiles", std::max<uint64_t>(ntiles, 1));
  uint32_t *d_cnt = cs.alloc<uint32_t>("d_cnt", kKcCntWords);
  if (cs.rc != PPCSR_OK) return cs.rc;
  uint32_t top = 0;
  cs.start();
  if (nn) {
    // stage 1: deg[], off[] (off[nn] = 2 |E(G)|), adj[]
    GCHK(gpu::dset(d_deg, 0, words * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_fill, 0, words * sizeof(uint32_t), cs.stream()));
    GPU_LAUNCH(cs.stream(), k_kc_init, cs.vert_grid(), 256, d_core, nn);
    uint32_t *d_adj = nullptr;
    uint64_t entries = 0;  // (2 |E(G)|: not needed here)
    int e = cs.symmetric_adjacency(P, d_deg, d_fill, d_off, d_tiles, ntiles, &d_adj, &entries);
    if (e != PPCSR_OK) return e;
    // stage 2
    uint32_t h_cnt[4] = {0, 0, 0, 0};  // (host copy of the three words of the counter block that are in use, padded to 16 bytes)
    uint32_t *cur = d_f0, *nxt = d_f1;
    for (;;) {
      GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), cs.stream()));
      GCHK(gpu::dset(d_cnt + 2, 0xFF, sizeof(uint32_t), cs.stream()));
      GPU_LAUNCH(cs.stream(), k_kc_min, grid_for(nn, 256, 1024), 256, (const uint32_t *)d_deg, (const uint32_t *)d_core, nn, d_cnt);
      GPU_LAUNCH(cs.stream(), k_kc_collect, grid_for(nn, 256), 256, (const uint32_t *)d_deg, d_core, nn, cur, d_cnt);
      e = cs.read_back(h_cnt, d_cnt, 3 * sizeof(uint32_t));
      if (e != PPCSR_OK) return e;
      uint32_t nfront = h_cnt[0];
      const uint32_t k = h_cnt[2];
      if (nfront == 0) break;  // (k == kMax: every vertex is assigned)
      top = k;
      while (nfront > 0) {
        GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), cs.stream()));
        GPU_LAUNCH(cs.stream(), k_kc_peel, cs.list_grid(nfront), 256, (const unsigned long long *)d_off, (const uint32_t *)d_adj, (const uint32_t *)cur,
                   nfront, k, d_deg, d_core, nxt, d_long, d_cnt);
        e = cs.read_back(h_cnt, d_cnt, 2 * sizeof(uint32_t));
        if (e != PPCSR_OK) return e;
        if (h_cnt[1]) {  // lists beyond one wave's reach: a second launch splits them over waves and appends to the same frontier
          GPU_LAUNCH(cs.stream(), k_kc_peel_long, grid_for((uint64_t)h_cnt[1] * 16, 4, 4096), 256, (const unsigned long long *)d_off, (const uint32_t *)d_adj,
                     (const uint32_t *)d_long, h_cnt[1], k, d_deg, d_core, nxt, d_cnt);
          e = cs.read_back(h_cnt, d_cnt, sizeof(uint32_t));
          if (e != PPCSR_OK) return e;
        }
        nfront = h_cnt[0];
        std::swap(cur, nxt);
      }
    }
  }
  cs.stop();
  if (core && nn) GCHK(gpu::d2h(core, d_core, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  if (kmax) *kmax = top;
  return cs.done(device_ms);
}

// Greedy colouring in a fixed vertex order (pma_colour.h).  Stage 1 is k-core's (symmetric_adjacency); then the keys of the
// order, one streaming pass for pred[], the first frontier, and one round per level of the order's DAG: a launch, one host
// read of the small counter block and, if the round deferred long lists, k_col_long and a second read.  A vertex enters one
// frontier, so more rounds than vertices is reported as an error instead of spinning, and so is a loop that ends with
// vertices left over.  device_ms covers the whole call, as kcore_over's.  A failed allocation is PPCSR_ENOMEM here.
// (The device side is ConsumerScope::colour_alloc / colour_run, which label_propagation_over runs as its first stage.)
int Engine::colouring_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint32_t *colour,
                           uint32_t *ncolours, double *device_ms) {
  const uint32_t nn = total_n;
  if (order > kColOrderId) return fail(PPCSR_EINVAL, "colouring: unknown vertex order");  // (refused before the device is even selected)
  ConsumerScope cs(this, PPCSR_ENOMEM);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  ConsumerScope::ColourStage st;
  cs.colour_alloc(&st);
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  if (nn) {
    const int e = cs.colour_run(P, order, seed, &st);
    if (e != PPCSR_OK) return e;
  }
  cs.stop();
  if (colour && nn) GCHK(gpu::d2h(colour, st.d_col, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (ncolours) *ncolours = (uint32_t)st.ctr[4];
  for (int i = 0; i < 8; i++) p_->colour_ctr[i] = st.ctr[i];
  return PPCSR_OK;
}
int Engine::colouring_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "colouring counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->colour_ctr[i];
  return PPCSR_OK;
}

// Label-propagation communities (pma_community.h; the definition: include/ppcsr.h).  The colouring's stage first — adjacency and
// colours stay on the device — then, for the weighted form, the second adjacency with the values; the counting sort of the
// vertices by (colour, tier) and ONE read of the bucket offsets; then sweeps: per class up to three launches over host-known
// ranges, per sweep one read of the striped counters.  The buffers the colouring's rounds are done with carry the labels
// (d_f0), the class lists (d_f1) and the marks of the community count (d_long).  Every change raises the weight of the edges
// whose ends agree, so the sweeps end; the bound on them (that weight plus one) is checked instead of trusted.
int Engine::label_propagation_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint32_t flags,
                                   uint32_t max_sweeps, const uint32_t *init, uint32_t *labels, uint64_t *ncommunities, uint32_t *sweeps,
                                   double *device_ms) {
  const uint32_t nn = total_n;
  // (all refused before the device is even selected)
  if (order > kColOrderId) return fail(PPCSR_EINVAL, "label propagation: unknown vertex order");
  if (flags & ~kLpWeighted) return fail(PPCSR_EINVAL, "label propagation: unknown flag bits");
  if (init)
    for (uint32_t v = 0; v < nn; v++)
      if (init[v] >= nn) return fail(PPCSR_EINVAL, "label propagation: an initial label is not a vertex id");
  const bool weighted = (flags & kLpWeighted) != 0;
  ConsumerScope cs(this, PPCSR_ENOMEM);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  ConsumerScope::ColourStage st;
  cs.colour_alloc(&st);
  ConsumerScope::Striped<unsigned long long, kLpStripeWords> cnt(cs, "d_lpcnt");
  if (cs.rc != PPCSR_OK) return cs.rc;
  unsigned long long *const d_stripes = cnt.stripes();
  uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t &nsweeps = ctr[0], &classes = ctr[1], &changes = ctr[2], &last = ctr[3], &launches = ctr[7];
  cs.start();
  if (nn) {
    int e = cs.colour_run(P, order, seed, &st);
    if (e != PPCSR_OK) return e;
    launches += st.ctr[6];
    const ConsumerPart *const tab = cs.table();  // (a launch's arguments are copies of plain pointers)
    uint32_t *const d_lab = st.d_f0, *const d_list = st.d_f1, *const d_fill = st.d_fill;
    const uint32_t *const d_col = st.d_col;
    uint8_t *const d_mark = reinterpret_cast<uint8_t *>(st.d_long);
    const unsigned long long *const d_off = st.d_off;
    const uint32_t *const d_adj = st.d_adj;
    const uint64_t entries = st.ctr[3];
    unsigned long long *d_wadj = nullptr;
    if (weighted) {
      d_wadj = cs.alloc<unsigned long long>("d_wadj", std::max<uint64_t>(entries, 1));
      if (cs.rc != PPCSR_OK) return cs.rc;
      GCHK(gpu::dset(d_fill, 0, cs.words() * sizeof(uint32_t), cs.stream()));
      GPU_LAUNCH(cs.stream(), k_lp_fill_weighted, cs.pass_grid(), 256, tab, P, nn, d_off, d_fill, d_wadj);
      launches++;
    }
    // the class lists: buckets 3 * colour + tier, their offsets read once
    const uint32_t buckets = 3u * (uint32_t)st.ctr[4];
    uint32_t *d_hist = cs.alloc<uint32_t>("d_hist", 3ull * buckets + 1);  // hist[buckets], first[buckets + 1], cursor[buckets]
    if (cs.rc != PPCSR_OK) return cs.rc;
    uint32_t *const d_first = d_hist + buckets, *const d_cursor = d_first + buckets + 1;
    GCHK(gpu::dset(d_hist, 0, (uint64_t)buckets * sizeof(uint32_t), cs.stream()));
    GPU_LAUNCH(cs.stream(), k_lp_hist, cs.vert_grid(), 256, d_col, d_off, nn, d_hist);
    GPU_LAUNCH(cs.stream(), k_lp_scan, 1, 64, (const uint32_t *)d_hist, buckets, d_first, d_cursor);
    GPU_LAUNCH(cs.stream(), k_lp_class_fill, cs.vert_grid(), 256, d_col, d_off, nn, d_cursor, d_list);
    launches += 3;
    std::vector<uint32_t> first(buckets + 1, 0);
    e = cs.read_back(first.data(), d_first, (uint64_t)(buckets + 1) * sizeof(uint32_t));
    if (e != PPCSR_OK) return e;
    for (uint32_t c = 0; 3 * c < buckets; c++) {
      if (first[3 * c + 3] > first[3 * c]) classes++;
      ctr[5] += first[3 * c + 3] - first[3 * c + 2];
    }
    // the labels
    if (init)
      GCHK(gpu::h2d(d_lab, init, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
    else
      GPU_LAUNCH(cs.stream(), k_lp_identity, cs.vert_grid(), 256, d_lab, nn);
    // the sweeps
    const uint64_t heaviest = weighted ? 0xFFFFFFFFull : 1ull;
    const uint64_t bound = entries / 2 > (~0ull - 1) / heaviest ? ~0ull : entries / 2 * heaviest + 1;  // (W(G) + 1, saturating)
    const uint32_t slots = p_->lp_table_slots;
    for (;;) {
      if (nsweeps == bound) return fail(PPCSR_EHIP, "label propagation: more sweeps than the graph has weight");
      nsweeps++;
      GCHK(cnt.zero());
      for (uint32_t b = 0; b < buckets; b++) {
        const uint32_t count = first[b + 1] - first[b];
        if (!count) continue;
        const uint32_t *const part = d_list + first[b];
        launches++;
        // (the launches differ in the kernel alone: tier = b % 3, and the weighted form reads the 8-byte entries)
#define LP_STEP(kernel, grid, ...)                                                                                      \
  do {                                                                                                                   \
    if (weighted)                                                                                                        \
      GPU_LAUNCH(cs.stream(), kernel<true>, grid, 256, d_off, d_adj, (const unsigned long long *)d_wadj, part, count, __VA_ARGS__); \
    else                                                                                                                 \
      GPU_LAUNCH(cs.stream(), kernel<false>, grid, 256, d_off, d_adj, (const unsigned long long *)d_wadj, part, count, __VA_ARGS__); \
  } while (0)
        if (b % 3 == 0)
          LP_STEP(k_lp_step_lanes, cs.list_grid(count), d_lab, d_stripes);
        else if (b % 3 == 1)
          LP_STEP(k_lp_step_wave, cs.list_grid(count), d_lab, d_stripes);
        else
          LP_STEP(k_lp_step_block, grid_for(count, 1, 1024), slots, d_lab, d_stripes);
#undef LP_STEP
      }
      e = cnt.read();
      if (e != PPCSR_OK) return e;
      if (cnt.sum(kLpCntFault)) return fail(PPCSR_EHIP, "label propagation: a list overflowed its label table in every hash split");
      last = cnt.sum(kLpCntChanges);
      changes += last;
      ctr[6] += cnt.sum(kLpCntPasses);
      if (last == 0 || nsweeps == max_sweeps) break;
    }
    // the labels in use
    GCHK(cnt.zero());
    GCHK(gpu::dset(d_mark, 0, nn, cs.stream()));
    GPU_LAUNCH(cs.stream(), k_lp_mark, cs.vert_grid(), 256, (const uint32_t *)d_lab, nn, d_mark);
    GPU_LAUNCH(cs.stream(), k_lp_count_marks, cs.vert_grid(), 256, (const uint8_t *)d_mark, nn, d_stripes);
    launches += 2;
    e = cnt.read();
    if (e != PPCSR_OK) return e;
    ctr[4] = cnt.sum(kLpCntLabels);
    cs.stop();
    if (labels) GCHK(gpu::d2h(labels, d_lab, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  } else {
    cs.stop();
  }
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (ncommunities) *ncommunities = ctr[4];
  if (sweeps) *sweeps = (uint32_t)nsweeps;
  for (int i = 0; i < 8; i++) p_->lp_ctr[i] = ctr[i];
  return PPCSR_OK;
}
int Engine::community_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "community counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->lp_ctr[i];
  return PPCSR_OK;
}

// Modularity of any labels (pma_community.h): the labels go up, one streaming pass adds the weights to tot[label] and to the
// striped counters, a vertex pass squares and sums tot[] into one 128-bit partial per workgroup; one read of the counters,
// one of the partials.  q is formed here, in doubles: out[1] / out[0] - S / out[0]^2.
int Engine::modularity_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *labels, uint32_t flags, uint64_t out[4],
                            double *q, double *device_ms) {
  const uint32_t nn = total_n;
  if (flags & ~kLpWeighted) return fail(PPCSR_EINVAL, "modularity: unknown flag bits");
  if (!labels && nn) return fail(PPCSR_EINVAL, "modularity: no labels");
  for (uint32_t v = 0; v < nn; v++)
    if (labels[v] >= nn) return fail(PPCSR_EINVAL, "modularity: a label is not below the number of vertices");
  ConsumerScope cs(this, PPCSR_ENOMEM);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const uint64_t words = cs.words();
  const uint32_t grid = cs.vert_grid();
  uint32_t *d_lab = cs.alloc<uint32_t>("d_lab", words);
  unsigned long long *d_tot = cs.alloc<unsigned long long>("d_tot", words), *d_part = cs.alloc<unsigned long long>("d_part", 2ull * grid);
  ConsumerScope::Striped<unsigned long long, kLpStripeWords> cnt(cs, "d_lpcnt");
  if (cs.rc != PPCSR_OK) return cs.rc;
  const ConsumerPart *const tab = cs.table();  // (a launch's arguments are copies of plain pointers)
  unsigned long long *const d_stripes = cnt.stripes();
  uint64_t res[4] = {0, 0, 0, 0};
  cs.start();
  if (nn) {
    GCHK(gpu::h2d(d_lab, labels, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_tot, 0, words * sizeof(unsigned long long), cs.stream()));
    GCHK(cnt.zero());
    if (flags & kLpWeighted)
      GPU_LAUNCH(cs.stream(), k_lp_mod_pass<true>, cs.pass_grid(), 256, tab, P, nn, (const uint32_t *)d_lab, d_tot, d_stripes);
    else
      GPU_LAUNCH(cs.stream(), k_lp_mod_pass<false>, cs.pass_grid(), 256, tab, P, nn, (const uint32_t *)d_lab, d_tot, d_stripes);
    GPU_LAUNCH(cs.stream(), k_lp_mod_squares, grid, 256, (const unsigned long long *)d_tot, nn, d_part);
    int e = cnt.read();
    if (e != PPCSR_OK) return e;
    std::vector<unsigned long long> part(2ull * grid, 0);
    e = cs.read_back(part.data(), d_part, part.size() * sizeof(unsigned long long));
    if (e != PPCSR_OK) return e;
    res[0] = 2 * cnt.sum(kLpCntWeight);
    res[1] = 2 * cnt.sum(kLpCntInside);
    for (uint32_t b = 0; b < grid; b++) {
      res[2] += part[2ull * b];
      res[3] += part[2ull * b + 1] + (res[2] < part[2ull * b] ? 1u : 0u);
    }
  }
  cs.stop();
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (out)
    for (int i = 0; i < 4; i++) out[i] = res[i];
  if (q) {
    const double m2 = (double)res[0], squares = (double)res[3] * 18446744073709551616.0 + (double)res[2];
    *q = res[0] ? (double)res[1] / m2 - squares / m2 / m2 : 0.0;
  }
  return PPCSR_OK;
}

// The lexicographically first maximal independent set in the same vertex orders (pma_colour.h), in place: per round one
// streaming pass, one vertex launch and one host read of the striped count (vertices left, vertices that joined).  Every round
// decides a vertex, and the bound the header documents is 2 n + 1 rounds: past it an error, not a spin.
int Engine::mis_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint8_t *in_set, uint64_t *size,
                     double *device_ms) {
  const uint32_t nn = total_n;
  if (order > kColOrderId) return fail(PPCSR_EINVAL, "mis: unknown vertex order");
  ConsumerScope cs(this, PPCSR_ENOMEM);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t words = cs.words();
  unsigned long long *d_key = cs.alloc<unsigned long long>("d_key", words);
  uint8_t *d_state = cs.alloc<uint8_t>("d_state", words), *d_out = cs.alloc<uint8_t>("d_out", words);
  uint32_t *d_blocked = cs.alloc<uint32_t>("d_blocked", words);
  uint32_t *d_deg = order == kColOrderDegree ? cs.alloc<uint32_t>("d_deg", words) : nullptr;
  ConsumerScope::Striped<unsigned long long, kMisStripeWords> cnt(cs, "d_cnt");
  unsigned long long *const d_cnt = cnt.dev;
  if (cs.rc != PPCSR_OK) return cs.rc;
  uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t &rounds = ctr[0], &passes = ctr[1], &members = ctr[4], &launches = ctr[6], &reads = ctr[7];
  cs.start();
  if (nn) {
    if (d_deg) {
      GCHK(gpu::dset(d_deg, 0, words * sizeof(uint32_t), cs.stream()));
      GPU_LAUNCH(cs.stream(), k_kc_degree, cs.pass_grid(), 256, tab, P, nn, d_deg);
      ctr[5]++;
      launches++;
    }
    GPU_LAUNCH(cs.stream(), k_col_keys, cs.vert_grid(), 256, order, (unsigned long long)seed, (const uint32_t *)d_deg, nn, d_key);
    launches++;
    GCHK(gpu::dset(d_state, kMisUndecided, words, cs.stream()));
    GCHK(gpu::dset(d_out, 0, words, cs.stream()));
    GCHK(gpu::dset(d_blocked, 0, words * sizeof(uint32_t), cs.stream()));  // (rounds count from 1)
    for (uint64_t left = nn; left > 0;) {
      if (rounds > 2 * (uint64_t)nn) return fail(PPCSR_EHIP, "mis: more than 2 n + 1 rounds");
      rounds++;
      GCHK(cnt.zero());
      GPU_LAUNCH(cs.stream(), k_mis_pass, cs.pass_grid(), 256, tab, P, nn, (uint32_t)rounds, (const unsigned long long *)d_key,
                 (const uint8_t *)d_state, d_out, d_blocked);
      GPU_LAUNCH(cs.stream(), k_mis_step, cs.vert_grid(), 256, nn, (uint32_t)rounds, d_state, (const uint8_t *)d_out, (const uint32_t *)d_blocked,
                 d_cnt);
      passes++;
      launches += 2;
      const int e = cnt.read();
      if (e != PPCSR_OK) return e;
      reads++;
      const uint64_t all = cnt.sum(), joined = all >> 32, undecided = all & 0xFFFFFFFFull;
      if (undecided >= left) return fail(PPCSR_EHIP, "mis: a round decided nothing");
      members += joined;
      left = undecided;
      if (rounds == 1) {
        ctr[2] = joined;
        ctr[3] = undecided;
      }
    }
  }
  cs.stop();
  if (in_set && nn) GCHK(gpu::d2h(in_set, d_state, (uint64_t)nn, cs.stream()));
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (size) *size = members;
  for (int i = 0; i < 8; i++) p_->mis_ctr[i] = ctr[i];
  return PPCSR_OK;
}
int Engine::mis_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "mis counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->mis_ctr[i];
  return PPCSR_OK;
}

// Strongly connected components (pma_scc.h): trim to a fixpoint, forward-backward reach from one pivot, then colouring rounds
// while anything is live, the trim again after each.  Every streaming pass costs one host read of the striped counters (the
// loop conditions); the counters of ppcsr_debug_scc_counters are kept on the host from those same reads.  Every loop is
// bounded by what it retires or marks, so a pass count beyond the vertex count is reported as an error instead of spinning.
int Engine::scc_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *labels, uint64_t *count, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t words = cs.words();
  const uint64_t bit_words = std::max<uint64_t>(((uint64_t)nn + 63) / 64 * 2, 2);
  uint32_t *d_scc = cs.alloc<uint32_t>("d_scc", words), *d_col = cs.alloc<uint32_t>("d_col", words), *d_live = cs.alloc<uint32_t>("d_live", bit_words);
  uint8_t *d_out = cs.alloc<uint8_t>("d_out", words), *d_in = cs.alloc<uint8_t>("d_in", words);  // has_out / has_in of a trim sweep
  uint8_t *d_fw = cs.alloc<uint8_t>("d_fw", words), *d_bw = cs.alloc<uint8_t>("d_bw", words);    // marks of a reach
  ConsumerScope::Striped<unsigned long long, kSccStripeWords> cnt(cs, "d_cnt");
  unsigned long long *const d_cnt = cnt.dev;
  unsigned long long *d_aux = cs.alloc<unsigned long long>("d_aux", 2);  // [0]: the pivot's key, [1]: the label of its SCC (low word)
  if (cs.rc != PPCSR_OK) return cs.rc;
  uint64_t ctr[8] = {0, 0, UINT64_MAX, 0, 0, 0, 0, 0};
  uint64_t &passes = ctr[6], &reads = ctr[7];
  uint64_t live = nn, sccs = 0;
  const uint32_t pass_grid = cs.pass_grid(), vert_grid = cs.vert_grid();
  // the striped count of the launches since zero(): its low and high halves.  (k_scc_reach_*: a pass makes fewer than 2^32
  // stores per direction — the bound the kernels' own 64-bit adds rest on — so the stripes' sum carries nothing from the low
  // half into the high one either.)
  const auto zero = [&]() { return cnt.zero(); };
  const auto read = [&](uint64_t *lo, uint64_t *hi) {
    const int e = cnt.read();
    if (e != PPCSR_OK) return e;
    reads++;
    const uint64_t all = cnt.sum();
    *lo = all & 0xFFFFFFFFull;
    *hi = all >> 32;
    return (int)PPCSR_OK;
  };
  const auto spinning = [&]() { return fail(PPCSR_EHIP, "scc: a loop made more passes than the graph has vertices"); };
  const auto trim = [&]() {
    for (uint64_t sweep = 0, got = 1, hi = 0; live > 0 && got > 0; sweep++) {
      if (sweep > (uint64_t)nn + 1) return spinning();
      GCHK(zero());
      GPU_LAUNCH(cs.stream(), k_scc_trim_edges, pass_grid, 256, tab, P, nn, (const uint32_t *)d_live, d_out, d_in);
      GPU_LAUNCH(cs.stream(), k_scc_trim_retire, vert_grid, 256, d_scc, nn, d_out, d_in, d_live, d_cnt);
      passes++;
      ctr[1]++;
      const int e = read(&got, &hi);
      if (e != PPCSR_OK) return e;
      ctr[0] += got;
      live -= got;
    }
    return (int)PPCSR_OK;
  };
  cs.start();
  if (nn) {
    GCHK(gpu::dset(d_scc, 0xFF, words * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_live, 0xFF, bit_words * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_out, 0, words, cs.stream()));
    GCHK(gpu::dset(d_in, 0, words, cs.stream()));
    int e = trim();
    if (e != PPCSR_OK) return e;
    if (live > 0) {  // forward-backward from the pivot
      unsigned long long h_aux[2] = {0, 0xFFFFFFFFull};
      GCHK(gpu::h2d(d_aux, h_aux, sizeof(h_aux), cs.stream()));
      GPU_LAUNCH(cs.stream(), k_scc_pivot, grid_for(nn, 256, 512), 256, tab, P, nn, (const uint32_t *)d_live, d_aux);
      GPU_LAUNCH(cs.stream(), k_scc_marks, vert_grid, 256, (const uint32_t *)d_scc, nn, (const uint32_t *)nullptr, d_fw, d_bw);
      e = cs.read_back(h_aux, d_aux, sizeof(unsigned long long));
      if (e != PPCSR_OK) return e;
      reads++;
      const uint32_t pivot = 0xFFFFFFFFu - (uint32_t)h_aux[0];
      if (h_aux[0] == 0 || pivot >= nn) return fail(PPCSR_EHIP, "scc: no pivot among the live vertices");
      ctr[2] = pivot;
      const uint8_t marked = kSccMarked;
      GCHK(gpu::h2d(d_fw + pivot, &marked, 1, cs.stream()));
      GCHK(gpu::h2d(d_bw + pivot, &marked, 1, cs.stream()));
      bool fw_open = true, bw_open = true;
      for (uint64_t it = 0; fw_open || bw_open; it++) {
        if (it > (uint64_t)nn + 1) return spinning();
        GCHK(zero());
        if (fw_open && bw_open)
          GPU_LAUNCH(cs.stream(), k_scc_reach_both, pass_grid, 256, tab, P, nn, d_fw, d_bw, d_cnt);
        else if (fw_open)
          GPU_LAUNCH(cs.stream(), k_scc_reach_fw, pass_grid, 256, tab, P, nn, d_fw, d_cnt);
        else
          GPU_LAUNCH(cs.stream(), k_scc_reach_bw, pass_grid, 256, tab, P, nn, d_bw, d_cnt);
        passes++;
        uint64_t f = 0, b = 0;
        e = read(&f, &b);
        if (e != PPCSR_OK) return e;
        fw_open = fw_open && f > 0;
        bw_open = bw_open && b > 0;
      }
      GCHK(zero());
      GPU_LAUNCH(cs.stream(), k_scc_min, grid_for(nn, 256, 512), 256, (const uint8_t *)d_fw, (const uint8_t *)d_bw, nn, (uint32_t *)(d_aux + 1));
      GPU_LAUNCH(cs.stream(), k_scc_assign, vert_grid, 256, (const uint8_t *)d_fw, (const uint8_t *)d_bw, nn, (const uint32_t *)nullptr,
                 (const uint32_t *)(d_aux + 1), d_scc, d_live, d_cnt);
      uint64_t got = 0, hi = 0;
      e = read(&got, &hi);
      if (e != PPCSR_OK) return e;
      if (got == 0 || got > live) return fail(PPCSR_EHIP, "scc: the pivot's component came out empty");
      ctr[3] = got;
      live -= got;
      e = trim();
      if (e != PPCSR_OK) return e;
    }
    while (live > 0) {  // one colouring round
      ctr[4]++;
      GPU_LAUNCH(cs.stream(), k_scc_colour_init, vert_grid, 256, (const uint32_t *)d_scc, nn, d_col);
      for (uint64_t it = 0, got = 1, hi = 0; got > 0; it++) {
        if (it > (uint64_t)nn + 1) return spinning();
        GCHK(zero());
        GPU_LAUNCH(cs.stream(), k_scc_colour_prop, pass_grid, 256, tab, P, nn, (const uint32_t *)d_live, d_col, d_cnt);
        passes++;
        e = read(&got, &hi);
        if (e != PPCSR_OK) return e;
      }
      GPU_LAUNCH(cs.stream(), k_scc_marks, vert_grid, 256, (const uint32_t *)d_scc, nn, (const uint32_t *)d_col, (uint8_t *)nullptr, d_bw);
      for (uint64_t it = 0, lo = 0, got = 1; got > 0; it++) {
        if (it > (uint64_t)nn + 1) return spinning();
        GCHK(zero());
        GPU_LAUNCH(cs.stream(), k_scc_reach_colour, pass_grid, 256, tab, P, nn, (const uint32_t *)d_col, d_bw, d_cnt);
        passes++;
        e = read(&lo, &got);
        if (e != PPCSR_OK) return e;
      }
      GCHK(zero());
      GPU_LAUNCH(cs.stream(), k_scc_assign, vert_grid, 256, (const uint8_t *)nullptr, (const uint8_t *)d_bw, nn, (const uint32_t *)d_col,
                 (const uint32_t *)nullptr, d_scc, d_live, d_cnt);
      uint64_t got = 0, hi = 0;
      e = read(&got, &hi);
      if (e != PPCSR_OK) return e;
      if (got == 0 || got > live) return fail(PPCSR_EHIP, "scc: a colouring round retired nothing");
      ctr[5] += got;
      live -= got;
      e = trim();
      if (e != PPCSR_OK) return e;
    }
    if (count) {
      GCHK(zero());
      GPU_LAUNCH(cs.stream(), k_scc_count, vert_grid, 256, (const uint32_t *)d_scc, nn, d_cnt);
      uint64_t hi = 0;
      e = read(&sccs, &hi);
      if (e != PPCSR_OK) return e;
    }
  }
  cs.stop();
  if (labels && nn) GCHK(gpu::d2h(labels, d_scc, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (count) *count = sccs;
  for (int i = 0; i < 8; i++) p_->scc_ctr[i] = ctr[i];
  return PPCSR_OK;
}
int Engine::scc_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "scc counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->scc_ctr[i];
  return PPCSR_OK;
}

// Minimum spanning forest (pma_msf.h): Boruvka rounds.  A round is the lightest-weight pass and one host read of its count of
// cut edges — none ends the loop — then the lightest-pair pass, the hook launch and pointer doubling, one host read per jump
// launch (the first of them brings the round's hooks along), then the reset.  So passes = 2 * rounds - 1: the last round makes
// the first pass only.  The striped counters are cleared once and read as running totals.  Every component with a cut edge
// merges, so more than floor(log2 n) + 2 rounds, a round that hooks nothing or a doubling of more than 34 launches is reported
// as an error instead of spinning.  The edge list is sorted by lo << 32 | hi on the device (sort_pairs_stable: the keys are unique).
int Engine::msf_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *weight,
                     uint32_t *labels, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t words = cs.words();
  uint32_t *d_comp = cs.alloc<uint32_t>("d_comp", words), *d_par = cs.alloc<uint32_t>("d_par", words), *d_bw = cs.alloc<uint32_t>("d_bw", words);
  unsigned long long *d_bp = cs.alloc<unsigned long long>("d_bp", words);
  unsigned long long *d_k0 = cs.alloc<unsigned long long>("d_k0", words), *d_k1 = cs.alloc<unsigned long long>("d_k1", words);  // the list: keys
  uint32_t *d_w0 = cs.alloc<uint32_t>("d_w0", words), *d_w1 = cs.alloc<uint32_t>("d_w1", words);                                  // and weights
  Edge *d_out = edges ? cs.alloc<Edge>("d_out", words) : nullptr;
  ConsumerScope::Striped<unsigned long long, kMsfStripeWords> cnt(cs, "d_cnt");
  unsigned long long *const d_cnt = cnt.dev;
  uint32_t *d_ne = cs.alloc<uint32_t>("d_ne", 2);  // the length of the list
  if (cs.rc != PPCSR_OK) return cs.rc;
  uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t &rounds = ctr[0], &passes = ctr[1], &reads = ctr[7];
  uint64_t tot[3] = {0, 0, 0};  // running totals of the three counter words, as of the last read
  uint64_t m = 0;
  const uint32_t pass_grid = cs.pass_grid(), vert_grid = cs.vert_grid();
  // the counters' growth since the last read: [0] cut edges / pointers moved, [1] hooks, [2] weight
  const auto read = [&](uint64_t grew[3]) {
    const int e = cnt.read();
    if (e != PPCSR_OK) return e;
    reads++;
    for (uint32_t w = 0; w < 3; w++) {
      const uint64_t now = cnt.sum(w);
      grew[w] = now - tot[w];
      tot[w] = now;
    }
    return (int)PPCSR_OK;
  };
  uint32_t max_rounds = 2;  // floor(log2 n) + 2
  while (((uint64_t)nn >> (max_rounds - 1)) != 0) max_rounds++;
  cs.start();
  if (nn) {
    GCHK(cnt.zero());
    GCHK(gpu::dset(d_ne, 0, 2 * sizeof(uint32_t), cs.stream()));
    GPU_LAUNCH(cs.stream(), k_cc_init, vert_grid, 256, d_par, nn);
    GPU_LAUNCH(cs.stream(), k_msf_reset, vert_grid, 256, d_comp, (const uint32_t *)d_par, d_bw, d_bp, nn);
    for (;;) {
      if (rounds >= max_rounds) return fail(PPCSR_EHIP, "msf: more rounds than halving the components allows");
      uint64_t grew[3];
      GPU_LAUNCH(cs.stream(), k_msf_weight, pass_grid, 256, tab, P, nn, (const uint32_t *)d_comp, d_bw, d_cnt);
      passes++;
      rounds++;
      int e = read(grew);
      if (e != PPCSR_OK) return e;
      if (grew[0] == 0) break;
      GPU_LAUNCH(cs.stream(), k_msf_pair, pass_grid, 256, tab, P, nn, (const uint32_t *)d_comp, d_bw, d_bp);
      passes++;
      GPU_LAUNCH(cs.stream(), k_msf_hook, vert_grid, 256, (const uint32_t *)d_comp, d_par, (const uint32_t *)d_bw, (const unsigned long long *)d_bp, nn,
                 d_k0, d_w0, d_ne, d_cnt);
      uint64_t hooks = 0, jumps = 0;
      for (uint64_t moved = 1; moved > 0;) {
        if (jumps > 34) return fail(PPCSR_EHIP, "msf: pointer doubling did not end");
        GPU_LAUNCH(cs.stream(), k_msf_jump, vert_grid, 256, d_par, nn, d_cnt);
        jumps++;
        e = read(grew);
        if (e != PPCSR_OK) return e;
        moved = grew[0];
        hooks += grew[1];
      }
      if (hooks == 0 || ctr[5] + hooks >= nn) return fail(PPCSR_EHIP, "msf: a round with cut edges hooked nothing, or too much");
      ctr[2] += jumps;
      ctr[3] = std::max(ctr[3], jumps);
      if (rounds == 1) ctr[4] = hooks;
      ctr[5] += hooks;
      GPU_LAUNCH(cs.stream(), k_msf_reset, vert_grid, 256, d_comp, (const uint32_t *)d_par, d_bw, d_bp, nn);
    }
    // finish: labels (d_bw is all kMax: the last reset, and a pass without cut edges stores nothing), the length, the sort
    GPU_LAUNCH(cs.stream(), k_msf_label_min, vert_grid, 256, (const uint32_t *)d_comp, d_bw, nn);
    GPU_LAUNCH(cs.stream(), k_msf_label_assign, vert_grid, 256, (const uint32_t *)d_comp, (const uint32_t *)d_bw, d_par, nn);
    uint32_t h_ne = 0;
    const int e = cs.read_back(&h_ne, d_ne, sizeof(uint32_t));
    if (e != PPCSR_OK) return e;
    reads++;
    m = h_ne;
    if (m != ctr[5]) return fail(PPCSR_EHIP, "msf: the edge list and the hook counts disagree");
    if (edges && m) {
      unsigned bits = 33;  // keys are below n << 32
      while (bits < 64 && ((uint64_t)nn >> (bits - 32)) != 0) bits++;
      const int sorted = sort_pairs_stable(cs.stream(), d_k0, d_k1, d_w0, d_w1, m, bits,
                                           [&](size_t bytes) { return cs.alloc<uint8_t>("d_tmp", std::max<uint64_t>(bytes, 1)); });
      if (sorted == 2) return cs.rc;
      if (sorted != 0) return fail(PPCSR_EHIP, "msf: device sort failed");
      GPU_LAUNCH(cs.stream(), k_msf_pack, grid_for(m, 256, 4096), 256, (const unsigned long long *)d_k1, (const uint32_t *)d_w1, m, d_out);
    }
  }
  cs.stop();
  if (edges && m && cap) GCHK(gpu::d2h(edges, d_out, std::min<uint64_t>(cap, m) * sizeof(Edge), cs.stream()));
  if (labels && nn) GCHK(gpu::d2h(labels, d_par, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
  const int done = cs.done(device_ms);
  if (done != PPCSR_OK) return done;
  if (count) *count = m;
  if (weight) *weight = tot[2];
  ctr[6] = (uint64_t)nn - m;
  for (int i = 0; i < 8; i++) p_->msf_ctr[i] = ctr[i];
  return (edges && cap < m) ? PPCSR_ERANGE : PPCSR_OK;
}
int Engine::msf_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "msf counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->msf_ctr[i];
  return PPCSR_OK;
}

// Edge support and truss numbers (pma_truss.h).  Stage 1: one streaming pass marks the edges of G by slot and counts
// in-degrees and edges per chunk, two scans give the offsets of the in-lists and of the output, one host read the number of
// edges (the lists are allocated then), a second pass fills the in-lists.  The support phase is one launch and, if it deferred
// edges, a second one finds them.  The peel (ktruss only) costs one host read of the small counter block per level (the threshold
// and the first frontier) and per sub-round (the next frontier, the deferred edges), as kcore_over.  device_ms covers the whole call,
// allocations and round trips included.  A failed allocation is PPCSR_ENOMEM here.
int Engine::truss_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, bool peel, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *total,
                       uint32_t *tmax, uint32_t *vtruss, double *device_ms) {
  const uint32_t nn = total_n;
  const char *const what = peel ? "ktruss" : "edge_support";
  ConsumerScope cs(this, PPCSR_ENOMEM);
  uint64_t slots = 0;
  for (uint32_t k = 0; k < P; k++) slots += (parts[k].e->N() + 63) / 64 * 64;
  if (slots >= (1ull << 32)) return fail(PPCSR_EUNSUPPORTED, std::string(what) + ": 2^32 slots or more (an edge is named by a 32-bit slot id)");
  int rc = cs.open(parts, P, nn, what);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t words = cs.words(), swords = std::max<uint64_t>(slots, 1);
  const uint32_t chunks = (uint32_t)(slots / 64);
  const uint32_t vtiles = (uint32_t)(((uint64_t)nn + kKcTile - 1) / kKcTile), ctiles = (chunks + kKcTile - 1) / kKcTile;
  uint32_t *d_stamp = cs.alloc<uint32_t>("d_stamp", swords), *d_sup = cs.alloc<uint32_t>("d_sup", swords);
  uint32_t *d_tr = peel ? cs.alloc<uint32_t>("d_tr", swords) : nullptr;
  uint32_t *d_indeg = cs.alloc<uint32_t>("d_indeg", words), *d_fill = cs.alloc<uint32_t>("d_fill", words);
  uint32_t *d_ccnt = cs.alloc<uint32_t>("d_ccnt", std::max<uint32_t>(chunks, 1));
  unsigned long long *d_inoff = cs.alloc<unsigned long long>("d_inoff", words + 1), *d_choff = cs.alloc<unsigned long long>("d_choff", (uint64_t)chunks + 1);
  unsigned long long *d_tiles = cs.alloc<unsigned long long>("d_tiles", std::max<uint32_t>(std::max(vtiles, ctiles), 1));
  uint32_t *d_vt = vtruss ? cs.alloc<uint32_t>("d_vt", words) : nullptr;
  ConsumerScope::Striped<unsigned long long, kTrStripeWords> tot(cs, "d_tot");
  uint32_t *d_cnt = cs.alloc<uint32_t>("d_cnt", kTrCntWords);
  if (cs.rc != PPCSR_OK) return cs.rc;
  uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t &reads = ctr[7];
  uint64_t m = 0;
  uint32_t top = 0;
  Edge *d_out = nullptr;
  uint32_t h_cnt[4] = {0, 0, 0, 0};
  const auto read_cnt = [&](uint32_t nwords) {
    reads++;
    return cs.read_back(h_cnt, d_cnt, nwords * sizeof(uint32_t));
  };
  cs.start();
  if (nn && chunks) {
    const uint32_t chunk_grid = grid_for(chunks, 4, 8192), slot_grid = grid_for(slots, 256, 4096);
    const uint32_t long_grid = 2048;  // the long-range kernels: at most the 8192 waves the chip holds at once
    // stage 1
    GCHK(gpu::dset(d_indeg, 0, words * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_fill, 0, words * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_sup, 0, swords * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::dset(d_cnt, 0, kTrCntWords * sizeof(uint32_t), cs.stream()));
    GCHK(tot.zero());
    GPU_LAUNCH(cs.stream(), k_tr_init, cs.pass_grid(), 256, tab, P, nn, d_stamp, d_indeg, d_ccnt);
    GPU_LAUNCH(cs.stream(), k_kc_tile_sums, grid_for(vtiles, 1, 65536), 256, (const uint32_t *)d_indeg, nn, vtiles, d_tiles);
    GPU_LAUNCH(cs.stream(), k_kc_scan_tiles, 1, 64, d_tiles, vtiles, d_inoff + nn);
    GPU_LAUNCH(cs.stream(), k_kc_scan_write, grid_for(vtiles, 1, 65536), 256, (const uint32_t *)d_indeg, nn, vtiles, (const unsigned long long *)d_tiles, d_inoff);
    GPU_LAUNCH(cs.stream(), k_kc_tile_sums, grid_for(ctiles, 1, 65536), 256, (const uint32_t *)d_ccnt, chunks, ctiles, d_tiles);
    GPU_LAUNCH(cs.stream(), k_kc_scan_tiles, 1, 64, d_tiles, ctiles, d_choff + chunks);
    GPU_LAUNCH(cs.stream(), k_kc_scan_write, grid_for(ctiles, 1, 65536), 256, (const uint32_t *)d_ccnt, chunks, ctiles, (const unsigned long long *)d_tiles, d_choff);
    unsigned long long entries = 0;
    rc = cs.read_back(&entries, d_inoff + nn, sizeof(entries));
    if (rc != PPCSR_OK) return rc;
    reads++;
    m = entries;
    const uint64_t ewords = std::max<uint64_t>(m, 1);
    uint32_t *d_inw = cs.alloc<uint32_t>("d_inw", ewords), *d_ins = cs.alloc<uint32_t>("d_ins", ewords);
    uint32_t *d_long = cs.alloc<uint32_t>("d_long", ewords);
    // (an edge enters one frontier once: no list exceeds |E|)
    uint32_t *d_f0 = peel ? cs.alloc<uint32_t>("d_f0", ewords) : nullptr, *d_f1 = peel ? cs.alloc<uint32_t>("d_f1", ewords) : nullptr;
    if (edges && cap && m) d_out = cs.alloc<Edge>("d_out", std::min<uint64_t>(cap, m));
    if (cs.rc != PPCSR_OK) return cs.rc;
    if (m && (edges || total || tmax || vtruss)) {  // (a call that only asks for *count ends here: the size query)
      const unsigned long long *inoff = d_inoff;
      const uint32_t *inw = d_inw, *ins = d_ins;
      GPU_LAUNCH(cs.stream(), k_tr_fill, cs.pass_grid(), 256, tab, P, nn, inoff, d_fill, d_inw, d_ins);
      // support
      GPU_LAUNCH(cs.stream(), k_tr_support, chunk_grid, 256, tab, P, nn, inoff, inw, ins, (const uint32_t *)d_stamp, d_sup, d_long, d_cnt, tot.stripes());
      // (the deferred edges, their number read on the device: no round trip, and a launch that finds none ends at once)
      GPU_LAUNCH(cs.stream(), k_tr_support_long, long_grid, 256, tab, P, nn, inoff, inw, ins, (const uint32_t *)d_long, (const uint32_t *)d_cnt, d_sup,
                 tot.stripes());
      // peel
      uint32_t *cur = d_f0, *nxt = d_f1;
      uint32_t r = 1;  // the sub-round about to run
      while (peel) {
        GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), cs.stream()));
        GCHK(gpu::dset(d_cnt + 2, 0xFF, sizeof(uint32_t), cs.stream()));
        GPU_LAUNCH(cs.stream(), k_tr_min, grid_for(slots, 256, 1024), 256, (const uint32_t *)d_sup, (const uint32_t *)d_stamp, slots, d_cnt);
        GPU_LAUNCH(cs.stream(), k_tr_collect, slot_grid, 256, (const uint32_t *)d_sup, d_stamp, d_tr, slots, r, cur, d_cnt);
        rc = read_cnt(3);
        if (rc != PPCSR_OK) return rc;
        uint32_t nfront = h_cnt[0];
        if (nfront == 0) break;  // (the threshold is kMax: every edge has its truss number)
        const TrPeel level{h_cnt[2], 0, d_sup, d_stamp, d_tr, nullptr, d_cnt};
        top = level.s + 2;
        ctr[2]++;
        uint64_t here = 0;
        while (nfront > 0) {
          TrPeel pl = level;
          pl.r = r;
          pl.next = nxt;
          here++;
          ctr[5] = std::max<uint64_t>(ctr[5], nfront);
          GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), cs.stream()));
          // (8192 waves are what the chip holds at once: a frontier below that gets teams of waves per edge, a wider one goes round)
          const uint32_t team = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(8192 / nfront, 1), kTrTeamMax);
          GPU_LAUNCH(cs.stream(), k_tr_peel, grid_for((uint64_t)nfront * team, 4, 2048), 256, tab, P, nn, inoff, inw, ins, (const uint32_t *)cur, nfront, team,
                     pl, d_long);
          // walks beyond kTrWaveSlots: a second launch splits them over waves and appends to the same frontier
          // (at most nfront edges are deferred: 64 waves for each, up to the chip's)
          GPU_LAUNCH(cs.stream(), k_tr_peel_long, grid_for((uint64_t)nfront * 64, 4, long_grid), 256, tab, P, nn, inoff, inw, ins, (const uint32_t *)d_long, pl);
          rc = read_cnt(2);
          if (rc != PPCSR_OK) return rc;
          ctr[6] += h_cnt[1];
          nfront = h_cnt[0];
          std::swap(cur, nxt);
          r++;
        }
        ctr[3] += here;
        ctr[4] = std::max(ctr[4], here);
      }
      // output
      if (d_vt) GCHK(gpu::dset(d_vt, 0, words * sizeof(uint32_t), cs.stream()));
      if (d_out || d_vt)
        GPU_LAUNCH(cs.stream(), k_tr_emit, chunk_grid, 256, tab, P, (const uint32_t *)d_stamp, (const uint32_t *)(peel ? d_tr : d_sup),
                   (const unsigned long long *)d_choff, d_out, cap, d_vt);
    }
  }
  cs.stop();
  GCHK(gpu::d2h(tot.host.data(), tot.dev, sizeof(unsigned long long) * tot.kCount, cs.stream()));  // (waited for by done(), with the rest)
  if (d_out) GCHK(gpu::d2h(edges, d_out, std::min<uint64_t>(cap, m) * sizeof(Edge), cs.stream()));
  if (vtruss && nn) {
    if (m) GCHK(gpu::d2h(vtruss, d_vt, (uint64_t)nn * sizeof(uint32_t), cs.stream()));  // (vtruss != null: the block above ran)
    else memset(vtruss, 0, (uint64_t)nn * sizeof(uint32_t));
  }
  rc = cs.done(device_ms);
  if (rc != PPCSR_OK) return rc;
  const uint64_t triangles = (nn && chunks && m) ? tot.sum() / 3 : 0;
  if (count) *count = m;
  if (total) *total = triangles;
  if (tmax) *tmax = top;
  ctr[0] = m;
  ctr[1] = triangles;
  for (int i = 0; i < 8; i++) p_->ktruss_ctr[i] = ctr[i];
  return (edges && cap < m) ? PPCSR_ERANGE : PPCSR_OK;
}
int Engine::edge_support_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *total,
                              double *device_ms) {
  return truss_over(parts, P, total_n, false, edges, cap, count, total, nullptr, nullptr, device_ms);
}
int Engine::ktruss_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint32_t *tmax,
                        uint32_t *vtruss, double *device_ms) {
  return truss_over(parts, P, total_n, true, edges, cap, count, nullptr, tmax, vtruss, device_ms);
}
int Engine::ktruss_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "ktruss counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->ktruss_ctr[i];
  return PPCSR_OK;
}

// Triangle counts (pma_intersect.h): one pass over every chunk, then the chunks that hold an edge with a long range again
int Engine::triangles_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint64_t *tri, uint64_t *total, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, nn, "triangles");
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  uint64_t chunks = 0;
  for (uint32_t k = 0; k < P; k++) chunks += (parts[k].e->N() + 63) / 64;
  if (chunks >= (1ull << 32)) return fail(PPCSR_EUNSUPPORTED, "triangles: more than 2^32 chunks");
  unsigned long long *d_tri = tri ? cs.alloc<unsigned long long>("d_tri", cs.words()) : nullptr;
  ConsumerScope::Striped<unsigned long long, kTriStripeWords> tot(cs, "d_tot");
  unsigned long long *const d_tot = tot.dev;
  uint32_t *d_list = cs.alloc<uint32_t>("d_list", std::max<uint64_t>(chunks, 1));  // chunks that hold an edge with a long range
  uint32_t *d_cnt = cs.alloc<uint32_t>("d_cnt", 32);
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  if (tri) GCHK(gpu::dset(d_tri, 0, cs.words() * sizeof(unsigned long long), cs.stream()));
  GCHK(tot.zero());
  GCHK(gpu::dset(d_cnt, 0, 32 * sizeof(uint32_t), cs.stream()));
  GPU_LAUNCH(cs.stream(), k_tri_edges, grid_for(chunks, 4, 8192), 256, tab, P, nn, d_tri, d_tot, d_list, d_cnt);
  uint32_t ndefer = 0;
  rc = cs.read_back(&ndefer, d_cnt, sizeof(uint32_t));
  if (rc != PPCSR_OK) return rc;
  if (ndefer) GPU_LAUNCH(cs.stream(), k_tri_long, grid_for((uint64_t)ndefer * 4, 1, 16384), 256, tab, P, nn, d_tri, d_tot, (const uint32_t *)d_list, ndefer);
  cs.stop();
  GCHK(gpu::d2h(tot.host.data(), d_tot, sizeof(unsigned long long) * tot.kCount, cs.stream()));  // (waited for by done(), with the counts)
  if (tri && nn) GCHK(gpu::d2h(tri, d_tri, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
  rc = cs.done(device_ms);
  if (rc == PPCSR_OK && total) *total = tot.sum();
  return rc;
}

// Common-neighbour counts (pma_intersect.h).  Pairs and counts: host memory (staged through the buffers of lookup_edges,
// lookup_stage pairs at a time), or this GPU's
int Engine::common_neighbours_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *a, const uint32_t *b, uint64_t nq,
                                   uint32_t *counts, bool on_device, double *device_ms) {
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, total_n, "common_neighbours");
  if (rc != PPCSR_OK) return rc;
  if (device_ms) *device_ms = 0.0;  // (a call that open() refuses leaves *device_ms alone, as every other consumer does)
  if (nq == 0) return PPCSR_OK;
  Impl &p = *p_;
  const ConsumerPart *tab = cs.table();
  if (on_device) {
    cs.start();
    GPU_LAUNCH(p.stream, k_common_neighbours, query_blocks(p, (nq + 63) / 64), 256, tab, P, total_n, a, b, nq, counts);
    cs.stop();
    return cs.done(device_ms);
  }
  const uint64_t stage = std::min(nq, p.q.lookup_stage);
  if (stage > p.q.lookup_cap) {
    uint64_t c0 = p.q.lookup_cap, c1 = p.q.lookup_cap, c2 = p.q.lookup_cap;
    if (grow_buf(&p.q.src, &c0, stage) || grow_buf(&p.q.dst, &c1, stage) || grow_buf(&p.q.val, &c2, stage)) {
      p.q.lookup_cap = 0;
      return fail(PPCSR_ENOMEM, "common_neighbours: staging");
    }
    p.q.lookup_cap = stage;
  }
  for (uint64_t i0 = 0; i0 < nq; i0 += stage) {
    const uint64_t m = std::min(stage, nq - i0);
    GCHK(gpu::h2d(p.q.src, a + i0, m * sizeof(uint32_t), p.stream));
    GCHK(gpu::h2d(p.q.dst, b + i0, m * sizeof(uint32_t), p.stream));
    cs.start();
    GPU_LAUNCH(p.stream, k_common_neighbours, query_blocks(p, (m + 63) / 64), 256, tab, P, total_n, (const uint32_t *)p.q.src,
               (const uint32_t *)p.q.dst, m, p.q.val);
    cs.stop();
    GCHK(gpu::d2h(counts + i0, p.q.val, m * sizeof(uint32_t), p.stream));
    GCHK(gpu::sync(p.stream));
    if (device_ms) *device_ms += p.timer.ms();
  }
  return cs.done(nullptr);
}

// Sampling (pma_sample.h).  A vertex whose range is beyond kBfsWaveSlots is never walked by the wave of a draw: such vertices
// are listed once per call — those among the queried vertices for sample_over, all of the graph for walks_over, whose walkers
// may reach any of them — and the measure prefix over their 64-slot chunks is built once with the gather's chunk map and
// scans.  Two host reads (the number of hubs, the number of their chunks); none when the launch meets no hub.
int Engine::ConsumerScope::sample_hubs(uint32_t P, const uint32_t *d_q, uint64_t k, bool weighted, SmHubs *hb) {
  const uint64_t cap = slots_ / kBfsWaveSlots + 1;  // (ranges are disjoint in the regular regime)
  uint32_t *d_hid = alloc<uint32_t>("d_hid", words());
  uint32_t *d_part = alloc<uint32_t>("d_part", cap), *d_lo = alloc<uint32_t>("d_lo", cap), *d_len = alloc<uint32_t>("d_len", cap);
  uint32_t *d_nch = alloc<uint32_t>("d_nch", cap), *d_cnt = alloc<uint32_t>("d_cnt", 1);
  unsigned long long *d_choff = alloc<unsigned long long>("d_choff", cap + 1);
  if (rc != PPCSR_OK) return rc;
  GCHK(gpu::dset(d_hid, 0xFF, words() * sizeof(uint32_t), p.stream));
  GCHK(gpu::dset(d_cnt, 0, sizeof(uint32_t), p.stream));
  GPU_LAUNCH(p.stream, k_sm_hubs, grid_for(k, 256, 4096), 256, tab_, P, n_, d_q, k, d_hid, d_part, d_lo, d_len, d_nch, (uint32_t)cap, d_cnt);
  uint32_t nhub = 0;
  int e = read_back(&nhub, d_cnt, sizeof(uint32_t));
  if (e != PPCSR_OK) return e;
  if (nhub > cap) return fail(PPCSR_EHIP, "sampling: more long vertex ranges than the arrays have room for");
  *hb = SmHubs{d_hid, d_part, d_lo, d_len, d_choff, nullptr};
  if (nhub == 0) return PPCSR_OK;
  e = eng.xscan(d_nch, false, nhub, d_choff, true, false, false);
  if (e != PPCSR_OK) return e;
  unsigned long long C = 0;
  e = read_back(&C, d_choff + nhub, sizeof(unsigned long long));
  if (e != PPCSR_OK) return e;
  uint32_t *d_crow = alloc<uint32_t>("d_crow", C);
  unsigned long long *d_cm = alloc<unsigned long long>("d_cm", C), *d_cpre = alloc<unsigned long long>("d_cpre", C + 1);
  if (rc != PPCSR_OK) return rc;
  GCHK(gpu::dset(d_crow, 0, C * sizeof(uint32_t), p.stream));
  GPU_LAUNCH(p.stream, k_gather_mark, grid_for(nhub, 256, 4096), 256, (const uint32_t *)d_nch, (const unsigned long long *)d_choff, (uint64_t)nhub,
             d_crow);
  e = eng.xscan(d_crow, false, C, d_crow, false, true, true);
  if (e != PPCSR_OK) return e;
  hb->cpre = d_cpre;
  GPU_LAUNCH(p.stream, k_sm_hub_count, grid_for((C + 63) / 64, 4, 8192), 256, tab_, n_, *hb, (const uint32_t *)d_crow, (uint64_t)C,
             weighted ? 1u : 0u, d_cm);
  return eng.xscan(d_cm, true, C, d_cpre, true, false, false);
}

// dests[i * fanout + j] = draw (seed, i, j) from L(vertices[i]), values beside them
int Engine::sample_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *vertices, uint64_t k, uint32_t fanout, uint64_t seed,
                        uint32_t flags, uint32_t *dests, uint32_t *values, bool on_device, double *device_ms) {
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, total_n, "sample_neighbours");
  if (rc != PPCSR_OK) return rc;
  if (device_ms) *device_ms = 0.0;
  if (k == 0) return PPCSR_OK;
  const ConsumerPart *tab = cs.table();
  const uint64_t cells = k * (uint64_t)fanout;
  const uint32_t *d_q = vertices;
  uint32_t *d_d = dests, *d_v = values;
  if (!on_device) {
    uint32_t *q = cs.alloc<uint32_t>("d_q", k);
    d_d = cs.alloc<uint32_t>("d_dests", cells);
    d_v = values ? cs.alloc<uint32_t>("d_values", cells) : nullptr;
    if (cs.rc != PPCSR_OK) return cs.rc;
    GCHK(gpu::h2d(q, vertices, k * sizeof(uint32_t), cs.stream()));
    d_q = q;
  }
  cs.start();
  SmHubs hb{};
  rc = cs.sample_hubs(P, d_q, k, (flags & kSmWeighted) != 0, &hb);
  if (rc != PPCSR_OK) return rc;
  GPU_LAUNCH(cs.stream(), k_sm_sample, cs.list_grid(k), 256, tab, P, total_n, hb, d_q, k, 0ull, fanout, (unsigned long long)seed, flags, d_d, d_v);
  cs.stop();
  if (!on_device) {
    GCHK(gpu::d2h(dests, d_d, cells * sizeof(uint32_t), cs.stream()));
    if (values) GCHK(gpu::d2h(values, d_v, cells * sizeof(uint32_t), cs.stream()));
  }
  return cs.done(device_ms);
}

// out[i][0] = starts[i], out[i][t + 1] = draw (seed, i, t) from L(out[i][t]): one launch per step over all walkers.  The hubs'
// prefix is built ONCE, for every hub of the graph, before the first step: no step recounts a hub, and no step reads back.
int Engine::walks_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *starts, uint64_t k, uint32_t length, uint64_t seed,
                       uint32_t flags, uint32_t *out, bool on_device, double *device_ms) {
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, total_n, "random_walks");
  if (rc != PPCSR_OK) return rc;
  if (device_ms) *device_ms = 0.0;
  if (k == 0) return PPCSR_OK;
  const ConsumerPart *tab = cs.table();
  const uint64_t cells = k * ((uint64_t)length + 1);
  const uint32_t *d_q = starts;
  uint32_t *d_out = out;
  if (!on_device) {
    uint32_t *q = cs.alloc<uint32_t>("d_q", k);
    d_out = cs.alloc<uint32_t>("d_out", cells);
    if (cs.rc != PPCSR_OK) return cs.rc;
    GCHK(gpu::h2d(q, starts, k * sizeof(uint32_t), cs.stream()));
    d_q = q;
  }
  cs.start();
  SmHubs hb{};
  rc = cs.sample_hubs(P, nullptr, total_n, (flags & kSmWeighted) != 0, &hb);
  if (rc != PPCSR_OK) return rc;
  GPU_LAUNCH(cs.stream(), k_sm_walk_init, grid_for(k, 256, 4096), 256, d_q, k, total_n, length, d_out);
  for (uint32_t t = 0; t < length; t++)
    GPU_LAUNCH(cs.stream(), k_sm_walk, cs.list_grid(k), 256, tab, P, total_n, hb, d_out, k, 0ull, length, t, (unsigned long long)seed, flags);
  cs.stop();
  if (!on_device) GCHK(gpu::d2h(out, d_out, cells * sizeof(uint32_t), cs.stream()));
  return cs.done(device_ms);
}

// |L(v)| and the weighted W(v) of every vertex: one streaming pass, sources from the items (either regime)
int Engine::degrees_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *deg, uint64_t *wsum, double *device_ms) {
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, total_n);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  uint32_t *d_deg = deg ? cs.alloc<uint32_t>("d_deg", cs.words()) : nullptr;
  unsigned long long *d_ws = wsum ? cs.alloc<unsigned long long>("d_wsum", cs.words()) : nullptr;
  if (cs.rc != PPCSR_OK) return cs.rc;
  cs.start();
  if (deg) GCHK(gpu::dset(d_deg, 0, cs.words() * sizeof(uint32_t), cs.stream()));
  if (wsum) GCHK(gpu::dset(d_ws, 0, cs.words() * sizeof(unsigned long long), cs.stream()));
  GPU_LAUNCH(cs.stream(), k_sm_degrees, cs.pass_grid(), 256, tab, P, total_n, d_deg, d_ws);
  cs.stop();
  if (deg && total_n) GCHK(gpu::d2h(deg, d_deg, (uint64_t)total_n * sizeof(uint32_t), cs.stream()));
  if (wsum && total_n) GCHK(gpu::d2h(wsum, d_ws, (uint64_t)total_n * sizeof(uint64_t), cs.stream()));
  return cs.done(device_ms);
}

// Multi-source BFS (pma_msbfs.h): the sources in groups of 64, a group's levels until one finds nothing.  The loop is the
// hybrid loop's — a union frontier of at least hybrid_big vertices takes one streaming pass, a smaller one is listed (from
// stamp[] by k_bfs_collect when the level before was a pass) and expanded one wave per vertex, and hubs that launch leaves
// behind are finished by one pass — with a vertex step behind every edge step.  One host read per level: the 64 counts, the
// length of the next list and the hub flag (a level whose per-vertex launch met a hub is read twice: the listed vertex step
// declines to run, and the pass and the step over all n follow).  In the sequential regime every level is a pass: node
// ranges are never walked.  device_ms adds the groups' loops up; the copy of a group's rows to the caller lies between them.
int Engine::multi_bfs_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, uint32_t *levels,
                           uint64_t *reached, uint64_t *far, uint32_t *ecc, double *harmonic, double *device_ms) {
  const uint32_t nn = total_n;
  for (uint64_t i = 0; i < k; i++)
    if (sources[i] >= nn) return fail(PPCSR_EINVAL, "multi_bfs: source vertex out of range");
  if (k == 0) return PPCSR_OK;
  bool ranges = true;  // node ranges may be walked: no partition is in the sequential regime
  for (uint32_t q = 0; q < P; q++) ranges = ranges && parts[q].e->p_->v.g.narrow != 0u;
  ConsumerScope cs(this);
  const int rc = cs.open(parts, P, nn);
  if (rc != PPCSR_OK) return rc;
  const ConsumerPart *tab = cs.table();
  const uint64_t bit_words = ((uint64_t)nn + 63) / 64 * 2;  // union-frontier bitmap of the passes (d_vb: k_bfs_bits' second output, unused)
  uint32_t *d_fb = cs.alloc<uint32_t>("d_fb", bit_words), *d_vb = cs.alloc<uint32_t>("d_vb", bit_words);
  unsigned long long *d_seen = cs.alloc<unsigned long long>("d_seen", nn), *d_front = cs.alloc<unsigned long long>("d_front", nn);
  unsigned long long *d_next = cs.alloc<unsigned long long>("d_next", nn), *d_sw = cs.alloc<unsigned long long>("d_sw", 64);
  uint32_t *d_st = cs.alloc<uint32_t>("d_st", nn), *d_f0 = cs.alloc<uint32_t>("d_f0", nn), *d_f1 = cs.alloc<uint32_t>("d_f1", nn);
  uint32_t *d_lvg = levels ? cs.alloc<uint32_t>("d_levels", std::min<uint64_t>(k, 64) * nn) : nullptr;
  ConsumerScope::Striped<uint32_t, kMsStripeWords, kMsLead> cnt(cs, "d_cnt");
  uint32_t *const d_cnt = cnt.dev, *const d_stripes = cnt.stripes();  // (a launch's arguments are plain pointers)
  if (cs.rc != PPCSR_OK) return cs.rc;
  const uint32_t big = ConsumerScope::hybrid_big(nn);
  const bool look = p_->msbfs_look != 0u;
  uint64_t ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double ms = 0;
  for (uint64_t g0 = 0; g0 < k; g0 += 64) {
    const uint32_t nbits = (uint32_t)std::min<uint64_t>(64, k - g0);
    uint32_t verts[64], nv = 0;
    unsigned long long words[64];
    for (uint32_t b = 0; b < nbits; b++) {  // repeated sources share a vertex's word
      uint32_t at = 0;
      while (at < nv && verts[at] != sources[g0 + b]) at++;
      if (at == nv) {
        verts[nv] = sources[g0 + b];
        words[nv++] = 0;
      }
      words[at] |= 1ull << b;
    }
    uint64_t g_reached[64], g_far[64];
    uint32_t g_ecc[64];
    double g_harm[64];
    for (uint32_t b = 0; b < 64; b++) g_reached[b] = 1, g_far[b] = 0, g_ecc[b] = 0, g_harm[b] = 0.0;
    ctr[0]++;
    cs.start();
    GCHK(gpu::dset(d_seen, 0, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
    GCHK(gpu::dset(d_front, 0, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
    GCHK(gpu::dset(d_next, 0, (uint64_t)nn * sizeof(unsigned long long), cs.stream()));
    GCHK(gpu::dset(d_st, 0xFF, (uint64_t)nn * sizeof(uint32_t), cs.stream()));
    if (d_lvg) GCHK(gpu::dset(d_lvg, 0xFF, (uint64_t)nbits * nn * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::h2d(d_f0, verts, nv * sizeof(uint32_t), cs.stream()));
    GCHK(gpu::h2d(d_sw, words, nv * sizeof(unsigned long long), cs.stream()));
    GPU_LAUNCH(cs.stream(), k_ms_init, 1, 64, (const uint32_t *)d_f0, (const unsigned long long *)d_sw, nv, nn, d_seen, d_front, d_st, d_lvg);
    const auto full = [&](uint32_t level) {  // the edge step as a pass, the vertex step over all n
      GPU_LAUNCH(cs.stream(), k_bfs_bits, cs.vert_grid(), 256, (const uint32_t *)d_st, nn, level, d_fb, d_vb);
      if (look)
        GPU_LAUNCH(cs.stream(), k_ms_edges<true>, cs.pass_grid(), 256, tab, P, nn, (const uint32_t *)d_fb, (const unsigned long long *)d_front,
                   (const unsigned long long *)d_seen, d_next);
      else
        GPU_LAUNCH(cs.stream(), k_ms_edges<false>, cs.pass_grid(), 256, tab, P, nn, (const uint32_t *)d_fb, (const unsigned long long *)d_front,
                   (const unsigned long long *)d_seen, d_next);
      GPU_LAUNCH(cs.stream(), k_ms_vertices, cs.vert_grid(), 256, nn, (const uint32_t *)nullptr, (const uint32_t *)d_cnt, level, nbits, d_seen,
                 d_front, d_next, d_st, d_lvg, d_stripes);
      ctr[2]++;
      ctr[6]++;
    };
    uint32_t nfront = nv;
    uint32_t *cur = d_f0, *nxt = d_f1;
    bool have_list = true;
    for (uint32_t level = 0; nfront > 0; level++) {
      ctr[1]++;
      ctr[5] = std::max<uint64_t>(ctr[5], nfront);
      GCHK(cnt.zero());
      bool listed = ranges && nfront < big;
      if (!listed) {
        full(level);
        have_list = false;
      } else {
        if (!have_list) {  // (the union count of the vertex step is exact: the list's length is not read back)
          GPU_LAUNCH(cs.stream(), k_bfs_collect, grid_for(nn, 256), 256, (const uint32_t *)d_st, nn, level, cur, d_cnt);
          GCHK(gpu::dset(d_cnt, 0, 2 * sizeof(uint32_t), cs.stream()));
        }
        GPU_LAUNCH(cs.stream(), k_ms_level, cs.list_grid(nfront), 256, tab, P, nn, (const uint32_t *)cur, nfront, d_front,
                   (const unsigned long long *)d_seen, d_next, nxt, d_cnt);
        GPU_LAUNCH(cs.stream(), k_ms_vertices, grid_for(nn, 256, 512), 256, nn, (const uint32_t *)nxt, (const uint32_t *)d_cnt, level, nbits, d_seen,
                   d_front, d_next, d_st, d_lvg, d_stripes);
        ctr[3]++;
        ctr[6]++;
      }
      int e = cnt.read();
      if (e != PPCSR_OK) return e;
      ctr[7]++;
      if (listed && cnt.lead(1)) {  // hubs were skipped, and with them the vertex step: one pass finishes the level
        GCHK(cnt.zero());
        full(level);
        ctr[4]++;
        e = cnt.read();
        if (e != PPCSR_OK) return e;
        ctr[7]++;
        listed = false;
        have_list = false;
      }
      if (listed) {
        nfront = cnt.lead(0);
        std::swap(cur, nxt);
        have_list = true;
      } else {
        nfront = (uint32_t)cnt.sum(kMsUnion);
      }
      for (uint32_t b = 0; b < nbits; b++) {
        const uint64_t c = cnt.sum(b);
        if (c == 0) continue;
        g_reached[b] += c;
        g_far[b] += (uint64_t)(level + 1u) * c;
        g_ecc[b] = level + 1u;
        g_harm[b] += (double)c / (double)(level + 1u);
      }
    }
    cs.stop();
    if (d_lvg) GCHK(gpu::d2h(levels + g0 * nn, d_lvg, (uint64_t)nbits * nn * sizeof(uint32_t), cs.stream()));
    const int done = cs.done(nullptr);
    if (done != PPCSR_OK) return done;
    ms += p_->timer.ms();
    for (uint32_t b = 0; b < nbits; b++) {
      if (reached) reached[g0 + b] = g_reached[b];
      if (far) far[g0 + b] = g_far[b];
      if (ecc) ecc[g0 + b] = g_ecc[b];
      if (harmonic) harmonic[g0 + b] = g_harm[b];
    }
  }
  if (device_ms) *device_ms = ms;
  for (int i = 0; i < 8; i++) p_->msbfs_ctr[i] = ctr[i];
  return PPCSR_OK;
}
int Engine::multi_bfs_counters(uint64_t out[8]) {
  if (!out) return fail(PPCSR_EINVAL, "multi_bfs counters: no output");
  for (int i = 0; i < 8; i++) out[i] = p_->msbfs_ctr[i];
  return PPCSR_OK;
}

int Engine::debug_mulhi(const uint64_t *a, const uint64_t *b, uint64_t k, uint64_t *out) {
  if (k == 0) return PPCSR_OK;
  ConsumerScope cs(this);
  GCHK(gpu::set_device(device_));
  unsigned long long *d_a = cs.alloc<unsigned long long>("d_a", k), *d_b = cs.alloc<unsigned long long>("d_b", k);
  unsigned long long *d_o = cs.alloc<unsigned long long>("d_o", k);
  if (cs.rc != PPCSR_OK) return cs.rc;
  GCHK(gpu::h2d(d_a, a, k * sizeof(uint64_t), cs.stream()));
  GCHK(gpu::h2d(d_b, b, k * sizeof(uint64_t), cs.stream()));
  GPU_LAUNCH(cs.stream(), k_sm_mulhi, grid_for(k, 256, 4096), 256, (const unsigned long long *)d_a, (const unsigned long long *)d_b, k, d_o);
  GCHK(gpu::d2h(out, d_o, k * sizeof(uint64_t), cs.stream()));
  return cs.done(nullptr);
}

// pagerank.h:15-29: out[d] = sum over edges (s, d), in ascending s, of node_values[s] / num_neighbors(s).  The bulk scan
// emits (dest, contribution) per edge in CSR order — array after array, in partition order, which is ascending global source
// order because the partitions hold ascending vertex ranges — a STABLE sort by dest keeps ascending source order inside every
// destination, and one thread per destination adds its run sequentially: the reference's order of fp32 additions.
int Engine::pagerank_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const float *node_values, float *out, double *device_ms) {
  const uint32_t nn = total_n;
  ConsumerScope cs(this);
  int rc = cs.open(parts, P, nn, nullptr, false);
  if (rc != PPCSR_OK) return rc;
  Impl &p = *p_;
  const uint64_t N = cs.slots();  // room for every edge
  float *d_val = cs.alloc<float>("d_val", nn), *d_out = cs.alloc<float>("d_out", nn);
  uint32_t *d_k0 = cs.alloc<uint32_t>("d_k0", N), *d_k1 = cs.alloc<uint32_t>("d_k1", N);
  float *d_c0 = cs.alloc<float>("d_c0", N), *d_c1 = cs.alloc<float>("d_c1", N);
  if (cs.rc != PPCSR_OK) return cs.rc;
  GCHK(gpu::h2d(d_val, node_values, (uint64_t)nn * sizeof(float), p.stream));
  cs.start();
  // every array's edge count first (its place in the shared key / contribution arrays), then the contribution passes; the
  // first array's pass needs no count (it starts at 0) and goes out with its counts, as the one-engine call always did
  std::vector<uint32_t> tile(P);
  std::vector<uint64_t> ntiles(P);
  for (uint32_t k = 0; k < P; k++) {
    rc = scan_count(parts[k].e, &tile[k], &ntiles[k]);
    if (rc != PPCSR_OK) return rc;
    const Impl &q = *parts[k].e->p_;
    if (k == 0)
      scan_write(parts[0].e, tile[0], ntiles[0], nullptr, reinterpret_cast<int *>(d_k0), q.v.g.N, d_val + parts[0].first, d_c0, nullptr, 0, nn);
    GCHK(gpu::d2h(q.h_total, q.d_total, sizeof(unsigned long long), p.stream));
  }
  GCHK(gpu::sync(p.stream));
  GCHK(gpu::last_error());
  uint64_t m = 0;
  for (uint32_t k = 0; k < P; k++) {
    const uint64_t mk = *parts[k].e->p_->h_total;
    if (k > 0)
      scan_write(parts[k].e, tile[k], ntiles[k], nullptr, reinterpret_cast<int *>(d_k0 + m), mk, d_val + parts[k].first, d_c0 + m, nullptr,
                 0, nn);
    m += mk;
  }
  if (m) {
    unsigned bits = 1;  // keys are clamped to [0, n]
    while (bits < 32 && ((uint64_t)nn >> bits) != 0) bits++;
    rc = sort_pairs_stable(p.stream, d_k0, d_k1, d_c0, d_c1, m, bits);
    if (rc != 0) return fail(rc == 2 ? PPCSR_ENOMEM : PPCSR_EHIP, "pagerank: device sort failed");
  }
  uint32_t *d_long = cs.alloc<uint32_t>("d_long", (uint64_t)nn + 1);  // [0]: count, [1..]: destinations with long runs
  if (cs.rc != PPCSR_OK) return cs.rc;
  GCHK(gpu::dset(d_long, 0, sizeof(uint32_t), p.stream));
  GPU_LAUNCH(p.stream, k_pr_segsum, grid_for(nn, 256), 256, (const uint32_t *)d_k1, (const float *)d_c1, m, nn, d_out, d_long + 1, d_long);
  GPU_LAUNCH(p.stream, k_pr_longruns, 2048, 256, (const uint32_t *)d_k1, (const float *)d_c1, m, (const uint32_t *)(d_long + 1),
             (const uint32_t *)d_long, d_out);
  cs.stop();
  GCHK(gpu::d2h(out, d_out, (uint64_t)nn * sizeof(float), p.stream));
  return cs.done(device_ms);
}

}  // namespace ppcsr
