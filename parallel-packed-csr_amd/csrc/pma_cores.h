// Core numbers (k-core decomposition) over the table of gapped arrays (pma_consumer.h).  The edge set is the one k_cc_hook
// streams: the live edges of cp_load_chunks — taken from each item's own src, so nothing here assumes that vertex ranges
// are sorted or disjoint (the sequential regime is answered).
// The undirected graph G is the one k_tri_edges counts in, the upper orientation: {a, b}, a < b < n, is an edge exactly when
// the pair (a, b) is stored; pairs with src > dst and self-loops play no part.  A pair is stored at most once, so G is simple.
//
// Why this consumer EXPORTS where triangles intersect in place: peeling a vertex a must lower the degree of every neighbour,
// and those are the b of stored (a, b) — a's own range — AND the c of stored (c, a), c < a: a's in-neighbours, which the array
// does not index (finding them is a pass over everything).  So stage 1 builds a compact symmetric adjacency of G, 2 |E(G)|
// uint32 entries, once; stage 2 touches each list once, in peel order, which the array's layout cannot serve.
//
// Stage 1, three streaming passes' worth of work: k_kc_degree (deg[a]++, deg[b]++ per upper edge), an exclusive scan of the
// degrees into 64-bit offsets (k_kc_tile_sums / k_kc_scan_tiles / k_kc_scan_write), k_kc_fill (per-vertex cursors; the order
// inside a list is free).  A hub's run fills whole waves with one source: its lanes are counted within the wave and one lane
// issues the atomic (kc_source_runs; the reason is that of kCcRunLanes in pma_paths.h).  The destination side is one atomic
// per edge.
//
// Stage 2, peeling in sub-rounds (ParK: Dasari, Desh, Zubair 2014; PKC: Kabir, Madduri 2017 — PAPERS.md).  deg[v] starts as
// v's degree in G and only falls; core[v] starts unassigned (kMax).  A LEVEL k is the smallest deg among the unassigned
// vertices (k_kc_min — levels that no vertex has are never run); its first frontier is every unassigned vertex with
// deg == k (k_kc_collect, which assigns core = k).  A SUB-ROUND gives every frontier vertex u a wave that walks u's list:
// for a neighbour w whose degree looks above k the wave decrements deg[w] atomically, and the one decrement that returns
// k + 1 assigns core[w] = k and appends w to the next frontier.  The plain look may be stale, and stale means too large
// (deg only falls): the atomic decides.  The level ends when a sub-round appends nothing.
// Invariants, with L(k) = "level k has ended":
//  (1) deg[w] is decremented at most once per incident edge {u, w} from u's side — when u, which enters one frontier once (3),
//      is walked — so at most deg_G(w) times in all: it never wraps below zero.
//  (2) At L(k) every unassigned vertex has deg > k.  At the start of level k that holds for k - 1 and hence the unassigned
//      have deg >= k; those with deg == k are assigned by the collect; one with deg > k that ends at or below k has passed
//      through the decrement k + 1 -> k (decrements are by one), which assigned it.
//  (3) Every vertex enters exactly one frontier, exactly once.  The values deg[w] takes are strictly falling, so during
//      level k at most one decrement returns k + 1; a vertex the collect took has deg <= k and returns less; after L(k) an
//      assigned vertex has deg <= k < k' + 1 for every later level k', so it is never appended again; and by (2) the collect
//      of a later level only sees unassigned vertices.  Every vertex is assigned at last: the level only rises while
//      unassigned vertices remain.
//  (4) The level at which v enters is its core number.  Let S be the vertices unassigned when level k starts: by (3) those
//      that enter at levels >= k.  No vertex of S has been walked and every vertex outside S has been walked to the end (a
//      level ends only when a sub-round appends nothing), so deg[v], v in S, is the number of v's neighbours inside S, and it
//      is >= k because k is the minimum.  S has minimum degree >= k: core(v) >= k for all of S.  Conversely, let H be a
//      subgraph of minimum degree >= k + 1 and v the first vertex of H to be assigned, at level j.  A vertex is walked only
//      in a launch after the one that assigned it, so until then no vertex of H has been walked and deg[v] >= k + 1
//      throughout; but v is assigned when deg[v] equals j (collect) or falls to j (decrement): j >= k + 1.  So a vertex
//      that enters at level k lies in no such H: core(v) <= k.  This is the argument of sub-round peeling; the order of
//      removals inside a level does not enter it, so neither does the schedule.
// The frontier a sub-round appends is a function of the graph (w crosses k exactly when enough of its neighbours are in
// frontiers of this level), so levels and sub-rounds equal those of a synchronous peel on the host.
#pragma once
#include "pma_consumer.h"
#include "pma_paths.h"  // kCcRunLanes

namespace ppcsr {

constexpr uint32_t kKcTile = 1024;  // degrees per workgroup of the scan: 4 waves x 4 steps x 64 lanes
// counter block of the host loop: [0] vertices appended to the next frontier, [1] frontier vertices deferred to k_kc_peel_long,
// [2] the level (smallest deg among the unassigned; kMax: none left).  Three words are used; the device block is padded to 8
// (32 bytes, a sector of its own), and the host reads the first two or three of them.
constexpr uint32_t kKcCntWords = 8;

// Lanes of a wave that hold an upper edge of ONE source: the runs of cp_end_runs, from kCcRunLanes lanes on.  Out: lead — this
// lane issues for cnt edges; rank — this lane's place among them; leader — the lane that issues for this one (itself when not
// part of a reduced run).
PMA_DEV void kc_source_runs(bool up, uint32_t src, int lane, bool &lead, uint32_t &cnt, uint32_t &rank, int &leader) {
  cnt = 1;
  rank = 0;
  leader = lane;
  lead = cp_end_runs<kCcRunLanes>(up, src, lane, [&](bool in, uint64_t grp) {
    if (in) {
      cnt = (uint32_t)wv::popc64(grp);
      rank = dev::lanemask_lt_count(grp, lane);
      leader = wv::ctz64(grp);
    }
  });
}

// ---- stage 1: the symmetric adjacency of G ---------------------------------------------------------------------------------------------
// (both passes: the streaming load, then per chunk the upper edges of G and their source runs)
PMA_KERNEL void k_kc_degree(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t *deg) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&a)[kB], bool(&up)[kB], int lane) {
#pragma unroll
    for (int b = 0; b < kB; b++) {
      bool lead;
      uint32_t cnt, rank;
      int leader;
      up[b] = up[b] && a[b] < e[b].dest;
      kc_source_runs(up[b], a[b], lane, lead, cnt, rank, leader);
      if (lead) wv::atomic_add_u32(&deg[a[b]], cnt);
      if (up[b]) wv::atomic_add_u32(&deg[e[b].dest], 1u);
    }
  });
}
// fill[v]: entries of v's list written so far (ends at deg[v]); a reduced run takes its places with one atomic
PMA_KERNEL void k_kc_fill(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ off,
                          uint32_t *fill, uint32_t *adj) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&a)[kB], bool(&up)[kB], int lane) {
#pragma unroll
    for (int b = 0; b < kB; b++) {
      bool lead;
      uint32_t cnt, rank;
      int leader;
      up[b] = up[b] && a[b] < e[b].dest;
      kc_source_runs(up[b], a[b], lane, lead, cnt, rank, leader);
      uint32_t base = 0;
      if (lead) base = wv::atomic_add_u32(&fill[a[b]], cnt);
      base = wv::shfl(base, leader);
      if (up[b]) {
        adj[off[a[b]] + base + rank] = e[b].dest;
        adj[off[e[b].dest] + wv::atomic_add_u32(&fill[e[b].dest], 1u)] = a[b];
      }
    }
  });
}

// Exclusive scan of the degrees into 64-bit offsets: tile sums, one wave over the tile sums, the tiles again.  (Not a hot
// path: n words, three launches per call.)
PMA_DEV unsigned long long kc_wave_scan(unsigned long long v, int lane) {  // inclusive
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = cp_shfl(v, lane >= d ? lane - d : lane);
    if (lane >= d) v += o;
  }
  return v;
}
PMA_KERNEL void k_kc_tile_sums(const uint32_t *__restrict__ deg, uint32_t n, uint32_t ntiles, unsigned long long *tilesum) {
  PMA_SHARED unsigned long long ws[4];
  const int lane = wv::lane(), w = wv::wave_in_block();
  for (uint64_t t = wv::block_idx(); t < ntiles; t += wv::grid_dim()) {
    const uint64_t base = t * kKcTile + (uint64_t)w * 256;
    unsigned long long sum = 0;
    for (int j = 0; j < 4; j++) {
      const uint64_t i = base + (uint64_t)j * 64 + (uint64_t)lane;
      if (i < n) sum += deg[i];
    }
    sum = cp_shfl(kc_wave_scan(sum, lane), 63);
    if (lane == 0) ws[w] = sum;
    wv::block_sync();
    if (wv::thread_idx() == 0) tilesum[t] = ws[0] + ws[1] + ws[2] + ws[3];
    wv::block_sync();
  }
}
PMA_KERNEL void k_kc_scan_tiles(unsigned long long *tilesum, uint32_t ntiles, unsigned long long *total) {  // <<<1, 64>>>
  const int lane = wv::lane();
  unsigned long long carry = 0;
  for (uint64_t base = 0; base < ntiles; base += 64) {
    const uint64_t i = base + (uint64_t)lane;
    const unsigned long long v = i < ntiles ? tilesum[i] : 0ull;
    const unsigned long long s = kc_wave_scan(v, lane);
    if (i < ntiles) tilesum[i] = carry + s - v;
    carry += cp_shfl(s, 63);
  }
  if (lane == 0) *total = carry;
}
PMA_KERNEL void k_kc_scan_write(const uint32_t *__restrict__ deg, uint32_t n, uint32_t ntiles, const unsigned long long *__restrict__ tile_excl,
                                unsigned long long *off) {
  PMA_SHARED unsigned long long ws[4];
  const int lane = wv::lane(), w = wv::wave_in_block();
  for (uint64_t t = wv::block_idx(); t < ntiles; t += wv::grid_dim()) {
    const uint64_t base = t * kKcTile + (uint64_t)w * 256;
    unsigned long long x[4], s[4], sum = 0;
    for (int j = 0; j < 4; j++) {
      const uint64_t i = base + (uint64_t)j * 64 + (uint64_t)lane;
      x[j] = i < n ? deg[i] : 0u;
      s[j] = kc_wave_scan(x[j], lane);
      sum += cp_shfl(s[j], 63);
    }
    if (lane == 0) ws[w] = sum;
    wv::block_sync();
    unsigned long long run = tile_excl[t];
    for (int q = 0; q < w; q++) run += ws[q];
    for (int j = 0; j < 4; j++) {
      const uint64_t i = base + (uint64_t)j * 64 + (uint64_t)lane;
      if (i < n) off[i] = run + s[j] - x[j];
      run += cp_shfl(s[j], 63);
    }
    wv::block_sync();
  }
}

// ---- stage 2: peeling --------------------------------------------------------------------------------------------------------------------
PMA_KERNEL void k_kc_init(uint32_t *core, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) core[v] = kMax;
}
// cnt[2] = the smallest deg among the unassigned vertices (preset to kMax): one atomic per workgroup
PMA_KERNEL void k_kc_min(const uint32_t *__restrict__ deg, const uint32_t *__restrict__ core, uint32_t n, uint32_t *cnt) {
  PMA_SHARED uint32_t red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t m = kMax;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride)
    if (core[v] == kMax && deg[v] < m) m = deg[v];
  m = cp_wave_min(m, lane);
  if (lane == 0) red[wv::wave_in_block()] = m;
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    for (uint32_t q = 1; q < (wv::block_dim() >> 6); q++) m = red[q] < m ? red[q] : m;
    if (m != kMax) wv::atomic_min_u32(&cnt[2], m);
  }
}
// first frontier of the level k = cnt[2] (written by the launch before): every unassigned vertex with deg == k is assigned
// and listed
PMA_KERNEL void k_kc_collect(const uint32_t *__restrict__ deg, uint32_t *core, uint32_t n, uint32_t *front, uint32_t *cnt) {
  const int lane = wv::lane();
  const uint32_t k = cnt[2];
  if (k == kMax) return;
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t u = base + (uint64_t)lane;
    const bool in = u < n && core[u] == kMax && deg[u] == k;
    if (in) core[u] = k;
    cp_append(in, (uint32_t)u, front, cnt, lane);
  }
}
// adj[b, e) of a frontier vertex of level k, 64 entries per step, one atomic per wave per step on the counter
PMA_DEV void kc_peel_range(const uint32_t *__restrict__ adj, uint64_t b, uint64_t e, uint32_t k, int lane, uint32_t *deg, uint32_t *core,
                           uint32_t *next, uint32_t *cnt) {
  for (uint64_t base = b; base < e; base += 64) {
    const uint64_t i = base + (uint64_t)lane;
    uint32_t w = 0;
    bool won = false;
    if (i < e) {
      w = adj[i];
      // (the look may be stale, that is: too large — the atomic decides, and is issued only for what looked above k)
      if (deg[w] > k) won = wv::atomic_add_u32(&deg[w], 0xFFFFFFFFu) == k + 1u;
      if (won) core[w] = k;
    }
    cp_append(won, w, next, cnt, lane);
  }
}
// one sub-round: a wave per frontier vertex; a list beyond kBfsWaveSlots entries is left to k_kc_peel_long (longl, cnt[1])
PMA_KERNEL void k_kc_peel(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ front,
                          uint32_t nfront, uint32_t k, uint32_t *deg, uint32_t *core, uint32_t *next, uint32_t *longl, uint32_t *cnt) {
  const int lane = wv::lane();
  const uint64_t wstride = cp_waves();
  for (uint64_t f = cp_wave(); f < nfront; f += wstride) {
    const uint32_t u = wv::uni(front[f]);
    const uint64_t b = off[u], e = off[(uint64_t)u + 1];
    if (e - b > kBfsWaveSlots) {
      if (lane == 0) longl[wv::atomic_add_u32(&cnt[1], 1u)] = u;
      continue;
    }
    kc_peel_range(adj, b, e, k, lane, deg, core, next, cnt);
  }
}
// the deferred lists of the sub-round, split over waves in segments of kBfsWaveSlots entries: the grid's waves form groups of
// `per` waves, a group takes every `groups`-th list and its waves every `per`-th segment of it
PMA_KERNEL void k_kc_peel_long(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ longl,
                               uint32_t nlong, uint32_t k, uint32_t *deg, uint32_t *core, uint32_t *next, uint32_t *cnt) {
  const int lane = wv::lane();
  const uint64_t waves = cp_waves();
  const uint64_t gw = wv::uni(cp_wave());
  const uint64_t per = waves / nlong ? waves / nlong : 1, groups = waves / per;
  if (gw >= groups * per) return;
  for (uint64_t i = gw / per; i < nlong; i += groups) {
    const uint32_t u = wv::uni(longl[i]);
    const uint64_t b = off[u], e = off[(uint64_t)u + 1];
    for (uint64_t s = b + (gw % per) * kBfsWaveSlots; s < e; s += per * kBfsWaveSlots)
      kc_peel_range(adj, s, s + kBfsWaveSlots < e ? s + kBfsWaveSlots : e, k, lane, deg, core, next, cnt);
  }
}

}  // namespace ppcsr
