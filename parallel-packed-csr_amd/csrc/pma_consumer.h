// What the graph-algorithm consumers share (pma_scan.h: BFS / PageRank, pma_paths.h, pma_cores.h, pma_intersect.h): the table
// of gapped arrays, its two searches, the streaming load of the concatenated chunk space, the striped workgroup count, the
// look-up of a frontier vertex and the append to a vertex list.  Everything here is inlined into its kernel.
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
// the lanes with `in` append x to list[], whose length is *count: one ballot, one atomic per wave, the lanes write behind it
PMA_DEV void cp_append(bool in, uint32_t x, uint32_t *list, uint32_t *count, int lane) {
  const uint64_t m = wv::ballot(in);
  if (m == 0) return;
  uint32_t b = 0;
  if (lane == 0) b = wv::atomic_add_u32(count, (uint32_t)wv::popc64(m));
  b = wv::shfl(b, 0);
  if (in) list[b + dev::lanemask_lt_count(m, lane)] = x;
}

}  // namespace ppcsr
