// What the graph-algorithm consumers share (pma_scan.h: BFS / PageRank, pma_paths.h, pma_cores.h, pma_centrality.h, pma_scc.h,
// pma_msf.h, pma_intersect.h): the table of gapped arrays and its two searches; the streaming pass over the concatenated chunk
// space (cp_load_chunks, cp_stream); the vertex bitmaps (cp_bit, cp_store_bits); shuffles and the wave minimum (cp_shfl,
// cp_wave_min); the runs of a wave's lanes on one target word and their combiner (cp_end_runs, cp_combine_runs); the striped
// workgroup count (cp_striped_add); one wave per listed vertex (cp_frontier_vertex, cp_walk_vertices, cp_walk_slots) and the append to a vertex
// list (cp_append_at, cp_append).  Everything here is inlined into its kernel.
#pragma once
#include "pma_device.h"

namespace ppcsr {

// The consumers run over a TABLE of gapped arrays: the partitions of a PPPCSR (vertex ranges [first, first + n), edges stored
// with a partition-local src and a global dest), or one engine as a one-entry table.  Vertex ids in levels[], the frontier
// lists and bitmaps are global.  The table has P + 1 entries: entry P only closes the two searchable columns (first = the
// vertex count of the whole graph, chunk0 = the number of 64-slot chunks of all arrays).
struct ConsumerPart {
  const Edge *items;
  const Node *nodes;
  uint64_t N;       // slots
  uint64_t chunk0;  // 64-slot chunks of the arrays before this one
  uint32_t n;       // vertices
  uint32_t first;   // global id of vertex 0
  uint32_t pad[2];
};
static_assert(sizeof(ConsumerPart) == 48, "consumer table entry");
// owner of global vertex u (wave-uniform): the last entry whose first vertex is <= u — an empty partition shares its first
// vertex with the next one, which is the owner (the rule of PPPCSR.cpp:58-66)
PMA_DEV uint32_t cp_owner(const ConsumerPart *tab, uint32_t P, uint32_t u) {
  uint32_t lo = 0, hi = P - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// array that holds chunk ch of the concatenated chunk space (wave-uniform)
PMA_DEV uint32_t cp_chunk_owner(const ConsumerPart *tab, uint32_t P, uint64_t ch) {
  uint32_t lo = 0, hi = P - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tab[mid].chunk0 <= ch) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// this wave's index in the grid and the grid's number of waves: a kernel gives a wave every cp_waves()-th item of its work
PMA_DEV uint64_t cp_wave() { return (uint64_t)wv::block_idx() * (wv::block_dim() >> 6) + wv::wave_in_block(); }
PMA_DEV uint64_t cp_waves() { return (uint64_t)wv::grid_dim() * (wv::block_dim() >> 6); }

// ---- the streaming pass ------------------------------------------------------------------------------------------------------
// The chunk space is the concatenation of the table's arrays: each chunk finds its array by a wave-uniform search of the chunk
// prefix — with one array, a search of no steps: items0 / N0 / n0 are tab[0]'s, loaded once before the kernel's loop, so that
// there is no table look-up inside it — and its edges get global sources, src + first.  kB 64-slot chunks from ch0 on are in
// flight per wave.  Out, per chunk: the lane's item, its global source, and whether it is a LIVE edge: a non-null,
// non-sentinel slot other than slot N-1, with a local src < n_p and a global dest < n.  The edge set of every consumer is
// defined here and only here.
template <int kB>
PMA_DEV void cp_load_chunks(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const Edge *items0, uint64_t N0, uint32_t n0,
                            uint64_t ch0, uint64_t nchunks, int lane, Edge (&e)[kB], uint32_t (&src)[kB], bool (&live)[kB]) {
  uint32_t first[kB], pn[kB];
#pragma unroll
  for (int b = 0; b < kB; b++) {
    const Edge *items = items0;
    uint64_t s = (ch0 + b) * 64 + (uint64_t)lane, N = N0;
    first[b] = 0;
    pn[b] = n0;
    if (P > 1 && ch0 + b < nchunks) {
      const uint32_t k = cp_chunk_owner(tab, P, ch0 + b);
      items = tab[k].items;
      s -= tab[k].chunk0 * 64;
      N = tab[k].N;
      first[b] = tab[k].first;
      pn[b] = tab[k].n;
    }
    e[b] = null_edge();
    if (ch0 + b < nchunks && s + 1 < N) e[b] = items[s];  // (slot N-1 is never part of a neighbourhood)
  }
  // (a loop of its own, behind all kB loads: a predicate on e[b] inside the load loop costs the kernels their kB loads in
  // flight — k_bfs_edges_bits then compiles to 20 VGPRs instead of 26, and a BFS over 2^28 slots takes 12 % longer)
#pragma unroll
  for (int b = 0; b < kB; b++) {
    live[b] = e[b].value != 0 && !is_sentinel(e[b]) && e[b].src < pn[b] && e[b].dest < n;
    src[b] = e[b].src + first[b];
  }
}

// One streaming pass: a wave takes every cp_waves()-th group of kB chunks and hands each group's items to
// body(Edge (&e)[kB], uint32_t (&src)[kB], bool (&live)[kB], int lane).  A body is written as PHASES, each a loop over all kB
// chunks, so that the kB gathers of a phase are in flight TOGETHER: written one chunk after the other, the load of chunk b + 1
// waits for the store of chunk b whenever the two may alias (levels[] in k_bfs_edges_bits).  (k_cc_hook alone writes this
// loop out: pma_paths.h says why.)
template <int kB, class Body>
PMA_DEV void cp_stream(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, Body body) {
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  const Edge *const items0 = tab[0].items;
  const uint64_t N0 = tab[0].N;
  const uint32_t n0 = tab[0].n;
  for (uint64_t ch0 = wv::uni(cp_wave() * kB); ch0 < nchunks; ch0 += wstride * kB) {
    Edge e[kB];
    uint32_t src[kB];
    bool live[kB];
    cp_load_chunks<kB>(tab, P, n, items0, N0, n0, ch0, nchunks, lane, e, src, live);
    body(e, src, live, lane);
  }
}

// ---- vertex bitmaps: bit v of word v >> 5 -------------------------------------------------------------------------------------
PMA_DEV bool cp_bit(const uint32_t *bits, uint32_t v) { return ((bits[v >> 5] >> (v & 31u)) & 1u) != 0u; }
// the 64 vertices from `base` on (a multiple of 64), one per lane: lanes 0 and 1 store the two words of their ballot
PMA_DEV void cp_store_bits(uint32_t *bits, uint64_t base, uint64_t ballot, int lane) {
  if (lane < 2) bits[(base >> 5) + lane] = (uint32_t)(ballot >> (32 * lane));
}

// ---- shuffles, and the minimum over the wave's 64 lanes in every lane (an xor butterfly) ---------------------------------------
PMA_DEV uint32_t cp_shfl(uint32_t v, int src) { return wv::shfl(v, src); }
PMA_DEV unsigned long long cp_shfl(unsigned long long v, int src) {
  return ((unsigned long long)wv::shfl((uint32_t)(v >> 32), src) << 32) | wv::shfl((uint32_t)v, src);
}
template <class T>
PMA_DEV T cp_wave_min(T v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const T o = cp_shfl(v, lane ^ d);
    v = o < v ? o : v;
  }
  return v;
}

// ---- runs of lanes on one target word --------------------------------------------------------------------------------------------
// The lanes with `want` each have an atomic to issue on the word that `key` names.  Lanes on one word are served one after the
// other by the memory side, and a vertex's slots are contiguous: a hub's run — or one giant component — fills whole waves with
// one key.  The runs at the two ends of the wave's pending lanes (a run is "all pending lanes with this key", whatever their
// order; a run that fills the wave is both — its second visit finds the leader alone) are handed to run(in, grp) when they
// have kRun lanes or more: grp is the ballot of the run's lanes, `in` says this lane is one, and the call is made by the whole
// wave.  The run's first lane, ctz(grp), is left to issue for all of it.  Called by the whole wave; true: this lane issues —
// a lane of no such run issues its own.
template <int kRun, class Run>
PMA_DEV bool cp_end_runs(bool want, uint32_t key, int lane, Run run) {
  bool issue = want;
  const uint64_t pend = wv::ballot(want);
  if (pend) {
    const int ends[2] = {wv::ctz64(pend), 63 - wv::clz64(pend)};
    for (int t = 0; t < 2; t++) {
      const uint32_t k = wv::bcast(key, ends[t]);
      const bool in = issue && key == k;
      const uint64_t grp = wv::ballot(in);
      if (wv::popc64(grp) < kRun) continue;
      run(in, grp);
      if (in) issue = lane == wv::ctz64(grp);
    }
  }
  return issue;
}
// The same with a value v per lane, combined inside the wave: reduce(x, lane) combines over all 64 lanes (a minimum, a sum), the
// lanes outside the run giving `neutral`; every lane of the run receives the result in v.
template <int kRun, class T, class Reduce>
PMA_DEV bool cp_combine_runs(bool want, uint32_t key, T &v, T neutral, int lane, Reduce reduce) {
  return cp_end_runs<kRun>(want, key, lane, [&](bool in, uint64_t) {
    const T r = reduce(in ? v : neutral, lane);
    if (in) v = r;
  });
}

// The workgroup's count into striped counters: kBfsStripes counters on cache lines of their own (kWords words of T apart),
// one add per workgroup.  On a heavy BFS level nearly every wave has claims, and 32 K adds to ONE word are served one after
// the other by the memory side — that was 260-290 us of the 320 / 290 us the heavy levels took, whatever the per-edge work
// looked like.  mine: this wave's count (wave-uniform); red: 4 words of LDS; the host sums the stripes.
constexpr uint32_t kBfsStripes = 64, kBfsStripeWords = 32;
PMA_DEV void cp_atomic_add(uint32_t *p, uint32_t v) { wv::atomic_add_u32(p, v); }
PMA_DEV void cp_atomic_add(unsigned long long *p, unsigned long long v) { wv::atomic_add_u64(p, v); }
template <class T, uint32_t kWords>
PMA_DEV void cp_striped_add(T *stripes, T mine, T *red) {
  if (wv::lane() == 0) red[wv::wave_in_block()] = mine;
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    const T all = red[0] + red[1] + red[2] + red[3];
    if (all) cp_atomic_add(stripes + (uint64_t)(wv::block_idx() % kBfsStripes) * kWords, all);
  }
}

// ---- one wave per frontier vertex --------------------------------------------------------------------------------------------
constexpr uint64_t kBfsWaveSlots = 4096;  // longest slot range one wave walks on its own
// Array and node record of frontier vertex u (wave-uniform; items0 / nodes0 are tab[0]'s: with one array there is no search
// and no table look-up).  false: u is a hub, left to one streaming pass, which the host runs when it finds *hub_flag set.
PMA_DEV bool cp_frontier_vertex(const ConsumerPart *__restrict__ tab, uint32_t P, const Edge *items0, const Node *nodes0, uint32_t u, int lane,
                                uint32_t *hub_flag, const Edge *&items, Node &nd) {
  items = items0;
  if (P == 1) {
    nd = nodes0[u];
  } else {
    const uint32_t k = cp_owner(tab, P, u);
    items = tab[k].items;
    nd = tab[k].nodes[u - tab[k].first];
  }
  if ((uint64_t)nd.end - (uint64_t)nd.beginning <= kBfsWaveSlots) return true;
  if (lane == 0) *hub_flag = 1u;
  return false;
}
// One wave per vertex of list[0, nlist): vertex(u, items, nd) gets the vertex, its array and its node record — the slot range
// is its to walk (cp_walk_slots); hub(u) runs instead for a vertex cp_frontier_vertex leaves to the streaming pass.
template <class Hub, class Vertex>
PMA_DEV void cp_walk_vertices(const ConsumerPart *__restrict__ tab, uint32_t P, const uint32_t *list, uint32_t nlist, uint32_t *hub_flag, int lane,
                              Hub hub, Vertex vertex) {
  const uint64_t wstride = cp_waves();
  const Edge *const items0 = tab[0].items;
  const Node *const nodes0 = tab[0].nodes;
  for (uint64_t f = cp_wave(); f < nlist; f += wstride) {
    const uint32_t u = wv::uni(list[f]);
    const Edge *items;
    Node nd;
    if (cp_frontier_vertex(tab, P, items0, nodes0, u, lane, hub_flag, items, nd))
      vertex(u, items, nd);
    else
      hub(u);
  }
}
// the slots (beginning, end) of one vertex, 64 per step, by the whole wave: slot(val, dst) — val == 0 for a null slot and
// for the lanes beyond the range's end
template <class Slot>
PMA_DEV void cp_walk_slots(const Edge *items, const Node &nd, int lane, Slot slot) {
  for (uint64_t base = (uint64_t)nd.beginning + 1; base < (uint64_t)nd.end; base += 64) {
    const uint64_t s = base + (uint64_t)lane;
    uint32_t val = 0, dst = 0;
    if (s < (uint64_t)nd.end) {
      val = items[s].value;
      dst = items[s].dest;
    }
    slot(val, dst);
  }
}
// The lanes with `in` each take the next place of a list whose length is *count: one ballot, one atomic per wave, the lanes
// rank behind it.  Called by the whole wave; the place is valid in the lanes with `in`.
PMA_DEV uint32_t cp_append_at(bool in, uint32_t *count, int lane) {
  const uint64_t m = wv::ballot(in);
  if (m == 0) return 0;
  uint32_t b = 0;
  if (lane == 0) b = wv::atomic_add_u32(count, (uint32_t)wv::popc64(m));
  b = wv::shfl(b, 0);
  return b + dev::lanemask_lt_count(m, lane);
}
// the lanes with `in` append x to list[]
PMA_DEV void cp_append(bool in, uint32_t x, uint32_t *list, uint32_t *count, int lane) {
  const uint32_t at = cp_append_at(in, count, lane);
  if (in) list[at] = x;
}

}  // namespace ppcsr
