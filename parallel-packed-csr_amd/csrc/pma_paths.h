// Consumers that use the edge VALUES and the edges as undirected pairs: single-source shortest paths and weakly connected
// components over the table of gapped arrays (pma_consumer.h).  The edge set is the one the BFS kernels walk: the live edges
// of cp_load_chunks.
#pragma once
#include "pma_consumer.h"

namespace ppcsr {

constexpr unsigned long long kNoPath = 0xFFFFFFFFFFFFFFFFull;

// ---- SSSP: frontier relaxation to a fixpoint -------------------------------------------------------------------------------
// dist[] only falls.  stamp[v] is the last round for which v was made active: a vertex whose distance falls in round r gets
// stamp r + 1 (an atomic max: the first writer of the round sees an older stamp and is the one that appends / counts the
// vertex, so a vertex enters a round's active set once).  The active set of round r is { v : stamp[v] == r } — stamp[] plays
// the part levels[] plays in BFS, so k_bfs_bits and k_bfs_collect build the round's bitmap and list from it unchanged.
// Every fall re-activates, so when a round lowers nothing every edge has dist[v] <= dist[u] + w: with dist[start] = 0 that
// is the shortest-path condition.  Sums cannot overflow: an active source has a finite distance, the sum of at most n - 1
// <= 2^32 - 1 values <= 2^32 - 2 (include/ppcsr.h).
PMA_DEV bool sssp_relax_edge(unsigned long long nd, uint32_t dst, uint32_t round, unsigned long long *dist, uint32_t *stamp) {
  // (the caller has had a plain look at dist[dst] — possibly stale, that is: too large — and found it above nd: the atomic
  // decides, and is issued only for what looked like a fall)
  if (wv::atomic_min_u64(&dist[dst], nd) <= nd) return false;
  if (stamp[dst] == round + 1u) return false;  // (already active for the next round; stale means one more atomic)
  return wv::atomic_max_u32(&stamp[dst], round + 1u) <= round;
}
// Small active set: one wave per active vertex walks its slot range 64 slots per step; a hub is left to the streaming pass
// through the same flag word as in BFS (next_count[1]).  dist[u] is read when the wave starts: it may already be lower than
// at the start of the round (another wave lowered it; u then is active again next round).  A newer, smaller dist[u] only
// relaxes with a tighter bound — the fixpoint, which is unique, does not depend on it.
PMA_KERNEL void k_sssp_relax(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *front, uint32_t nfront,
                             uint32_t round, unsigned long long *dist, uint32_t *stamp, uint32_t *next, uint32_t *next_count) {
  const int lane = wv::lane();
  cp_walk_vertices(
      tab, P, front, nfront, &next_count[1], lane, [](uint32_t) {},  // (a hub: k_sssp_edges)
      [&](uint32_t u, const Edge *items, const Node &nd) {
        const unsigned long long du = dist[u];
        cp_walk_slots(items, nd, lane, [&](uint32_t val, uint32_t dst) {
          bool won = false;
          if (val != 0 && dst < n && du + val < dist[dst]) won = sssp_relax_edge(du + val, dst, round, dist, stamp);
          cp_append(won, dst, next, next_count, lane);
        });
      });
}
// Large active set (or hubs left over): one streaming pass over the concatenated chunk space, four 64-slot chunks in flight
// per wave; the source is tested against the round's active bitmap (n / 8 bytes: L2-resident), dist[src] is gathered only
// for edges that pass.  `found` (kBfsStripes counters on lines of their own, one add per workgroup) counts the vertices
// this pass made active for the next round — exactly, since the stamp admits each vertex once.
PMA_KERNEL void k_sssp_edges(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t round,
                             const uint32_t *__restrict__ active_bits, unsigned long long *dist, uint32_t *stamp, uint32_t *found) {
  PMA_SHARED uint32_t red[4];
  uint32_t mine = 0;
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&hit)[kB], int) {
    unsigned long long nd[kB], dd[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && cp_bit(active_bits, src[b]);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      nd[b] = hit[b] ? dist[src[b]] + e[b].value : kNoPath;
      dd[b] = hit[b] ? dist[e[b].dest] : 0ull;
    }
#pragma unroll
    for (int b = 0; b < kB; b++)
      if (nd[b] < dd[b] && sssp_relax_edge(nd[b], e[b].dest, round, dist, stamp)) mine++;
  });
  cp_striped_add<uint32_t, kBfsStripeWords>(found, wv::reduce_add(mine), red);
}

// ---- weakly connected components: min-label propagation with pointer jumping ---------------------------------------------
// Invariants: labels only fall; labels[x] <= x; labels[x] is a vertex of x's component.  A hook pass that finds no edge
// with two labels leaves labels constant on every component; the constant c is a vertex of the component and the
// component's smallest vertex m has labels[m] <= m, so c = m.
PMA_KERNEL void k_cc_init(uint32_t *labels, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) labels[v] = (uint32_t)v;
}
// One streaming pass: an edge whose ends carry different labels lowers the end with the larger label, and the entry of that
// larger label itself (the vertex it pointed to — this is what merges whole trees instead of single vertices, so a long chain
// finishes in few rounds).  Loads may be stale (too large): the atomic min decides.  `found` counts the edges that differed.
// This kernel keeps the pass loop of cp_stream and the run combiner of cp_combine_runs WRITTEN OUT: over the shared pieces it
// compiles to other code (54 SGPRs for 56), with which components over 8 partitions of a scale-18 graph took 3-6 % longer
// (0.90 -> 0.93 ms; one array was 1.5 % faster) — DESIGN 4c.  What is written here is what those two pieces say.
constexpr int kCcRunLanes = 8;  // lanes of a wave on one source from which its run is reduced before the atomic
PMA_KERNEL void k_cc_hook(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t *labels, uint32_t *found) {
  PMA_SHARED uint32_t red[4];
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  const Edge *const items0 = tab[0].items;
  const uint64_t N0 = tab[0].N;
  const uint32_t n0 = tab[0].n;
  uint32_t mine = 0;
  constexpr int kB = 4;
  for (uint64_t ch0 = wv::uni(cp_wave() * kB); ch0 < nchunks; ch0 += wstride * kB) {
    Edge e[kB];
    uint32_t src[kB];
    bool live[kB];
    cp_load_chunks<kB>(tab, P, n, items0, N0, n0, ch0, nchunks, lane, e, src, live);
    uint32_t lu[kB], lv[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) live[b] = live[b] && src[b] != e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      lu[b] = live[b] ? labels[src[b]] : 0u;
      lv[b] = live[b] ? labels[e[b].dest] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const bool diff = lu[b] != lv[b];
      uint32_t lo = lu[b] < lv[b] ? lu[b] : lv[b];
      const uint32_t hi = lu[b] < lv[b] ? lv[b] : lu[b];
      const uint32_t x = lu[b] < lv[b] ? e[b].dest : src[b];
      // Lanes that lower THEIR SOURCE share the target with their neighbours: their runs are reduced to the smallest label
      // and one lane issues it (the rule of cp_combine_runs; the others' edges still count as differing, and whatever they
      // would have stored is not below that minimum).  Lanes that lower their destination issue their own.
      bool issue = diff;
      const bool own = diff && x == src[b];
      const uint64_t pend = wv::ballot(own);
      if (pend) {
        const int ends[2] = {wv::ctz64(pend), 63 - wv::clz64(pend)};
        for (int t = 0; t < 2; t++) {
          const uint32_t key = wv::bcast(x, ends[t]);
          const bool in = own && issue && x == key;
          const uint64_t grp = wv::ballot(in);
          if (wv::popc64(grp) < kCcRunLanes) continue;
          uint32_t m = in ? lo : 0xFFFFFFFFu;
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = wv::shfl(m, lane ^ d);
            m = o < m ? o : m;
          }
          if (in) {
            lo = m;
            issue = lane == wv::ctz64(grp);
          }
        }
      }
      if (issue) {
        wv::atomic_min_u32(&labels[x], lo);
        if (hi != x) wv::atomic_min_u32(&labels[hi], lo);
      }
      if (diff) mine++;
    }
  }
  cp_striped_add<uint32_t, kBfsStripeWords>(found, wv::reduce_add(mine), red);
}
// labels[v] = the end of v's label chain.  labels[x] <= x, so a chain falls strictly until it meets a fixed point; only
// thread v stores to labels[v], and what it stores is not above what it read there.
PMA_KERNEL void k_cc_jump(uint32_t *labels, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    const uint32_t l0 = labels[v];
    uint32_t l = l0, next = labels[l];
    while (next != l) {
      l = next;
      next = labels[l];
    }
    if (l != l0) labels[v] = l;
  }
}

}  // namespace ppcsr
