// Shortest-path counts and betweenness centrality (Brandes 2001) over the table of gapped arrays (pma_consumer.h).  The edge
// set is the one the BFS kernels walk: the live edges of cp_load_chunks, directed, values unused.
//   forward   level by level: levels[] as BFS gives them, sigma[w] = number of shortest paths from the source to w (fp64)
//   backward  from the deepest level - 1 down to 0: delta[v] = sum over edges (v, w) with level[w] = level[v] + 1 of
//             (sigma[v] / sigma[w]) * (1 + delta[w])
//   per source  bc[v] += delta[v], v != source
// Every launch handles ONE level: what it reads of the neighbouring level (sigma[v] of level L going forward, sigma[w] and
// delta[w] of level L + 1 going backward) was completed by an earlier launch.
#pragma once
#include "pma_consumer.h"

namespace ppcsr {

// fp64 add into a word that other waves add into.  The buffers are the call's own gpu::dmalloc allocations — coarse-grained
// device memory — so the hardware's fp64 add (global_atomic_add_f64, executed at the memory side) is valid; nothing reads the
// old value.  The emulator runs its lanes one after the other: a plain add.
PMA_DEV void bc_atomic_add(double *p, double v) {
#if defined(PPCSR_SIM)
  *p += v;
#else
  unsafeAtomicAdd(p, v);
#endif
}
PMA_DEV double bc_shfl(double v, int src) {
  unsigned long long b;
  __builtin_memcpy(&b, &v, 8);
  b = cp_shfl(b, src);
  __builtin_memcpy(&v, &b, 8);
  return v;
}
// sum over the wave's 64 lanes, in every lane (a butterfly: fp addition commutes, so all lanes hold the same bits)
PMA_DEV double bc_reduce(double v, int lane) {
  for (int d = 1; d < 64; d <<= 1) v += bc_shfl(v, lane ^ d);
  return v;
}

constexpr uint32_t kBcNoStamp = 0xFFFFFFFFu;

// One source's start state, one launch: levels, sigma, delta and the first frontier list
PMA_KERNEL void k_bc_init(uint32_t *levels, double *sigma, double *delta, uint32_t n, uint32_t start, uint32_t *front) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    levels[v] = v == start ? 0u : kMax;
    sigma[v] = v == start ? 1.0 : 0.0;
    if (delta) delta[v] = 0.0;
    if (v == 0) front[0] = start;
  }
}

// The two per-edge tests of a streaming pass as bitmaps of n / 8 bytes (k_bfs_bits): "is the source one of this pass's
// sources" and "was the destination placed on a level <= `level`" (not among the destinations going forward: neither unseen
// nor claimed for level + 1).  The sources are the whole level (stamp == kBcNoStamp), or — for the pass that finishes a
// per-vertex launch — the hubs that launch left behind: those it stamped in hub_stamp[] with its own number.
PMA_KERNEL void k_bc_bits(const uint32_t *levels, const uint32_t *hub_stamp, uint32_t n, uint32_t level, uint32_t stamp, uint32_t *src_bits,
                          uint32_t *placed_bits) {
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t u = base + (uint64_t)lane;
    const uint32_t lv = u < n ? levels[u] : kMax;
    const bool is_src = stamp == kBcNoStamp ? lv == level : (u < n && hub_stamp[u] == stamp);
    cp_store_bits(src_bits, base, wv::ballot(u < n && is_src), lane);
    cp_store_bits(placed_bits, base, wv::ballot(u < n && lv <= level), lane);
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// An edge (v, w) out of level L: the first to find w unseen claims it for level L + 1 (compare-and-swap: exactly one claim
// per vertex, so the counts are exact), and every such edge — the claiming one and all that find L + 1 — adds sigma[v] to
// sigma[w].  The plain look at levels[w] may be stale only as "unseen": then the compare-and-swap answers.
PMA_DEV bool bc_forward_edge(double sv, uint32_t dst, uint32_t level, uint32_t lw, uint32_t *levels, double *sigma) {
  bool won = false;
  if (lw == kMax) {
    lw = wv::atomic_cas_u32(&levels[dst], kMax, level + 1u);
    won = lw == kMax;
  }
  if (won || lw == level + 1u) bc_atomic_add(&sigma[dst], sv);
  return won;
}
// Small frontier: one wave per frontier vertex (k_bfs_level).  A hub is stamped and left to the streaming pass.
PMA_KERNEL void k_bc_level(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *front, uint32_t nfront, uint32_t level,
                           uint32_t *levels, double *sigma, uint32_t *hub_stamp, uint32_t stamp, uint32_t *next, uint32_t *next_count) {
  const int lane = wv::lane();
  cp_walk_vertices(
      tab, P, front, nfront, &next_count[1], lane,
      [&](uint32_t u) {  // (a hub: k_bc_edges_forward)
        if (lane == 0) hub_stamp[u] = stamp;
      },
      [&](uint32_t u, const Edge *items, const Node &nd) {
        const double su = sigma[u];
        cp_walk_slots(items, nd, lane, [&](uint32_t val, uint32_t dst) {
          bool won = false;
          if (val != 0 && dst < n) won = bc_forward_edge(su, dst, level, levels[dst], levels, sigma);
          cp_append(won, dst, next, next_count, lane);
        });
      });
}
// Large frontier, or the hubs a per-vertex launch left: one streaming pass (k_bfs_edges_bits).  `found` counts the claims.
PMA_KERNEL void k_bc_edges_forward(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t level,
                                   const uint32_t *__restrict__ src_bits, const uint32_t *__restrict__ placed_bits, uint32_t *levels,
                                   double *sigma, uint32_t *found) {
  PMA_SHARED uint32_t red[4];
  uint32_t mine = 0;
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&hit)[kB], int) {
    uint32_t lw[kB];
    double sv[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && cp_bit(src_bits, src[b]);
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && !cp_bit(placed_bits, e[b].dest);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      lw[b] = hit[b] ? levels[e[b].dest] : 0u;
      sv[b] = hit[b] ? sigma[src[b]] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < kB; b++)
      if (hit[b] && bc_forward_edge(sv[b], e[b].dest, level, lw[b], levels, sigma)) mine++;
  });
  cp_striped_add<uint32_t, kBfsStripeWords>(found, wv::reduce_add(mine), red);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// one DAG edge's term: one division, one addition, one multiplication (the build has -ffp-contract=off: nothing is fused)
PMA_DEV double bc_term(double sv, double sw, double dw) { return (sv / sw) * (1.0 + dw); }
// Small level (its list: k_bfs_collect): one wave per vertex, lanes over the slot range, a wave reduction, one plain store.
// A hub is stamped and left to the streaming pass, which adds into its zero.
PMA_KERNEL void k_bc_delta_vertex(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *list, uint32_t nlist,
                                  uint32_t level, const uint32_t *levels, const double *sigma, double *delta, uint32_t *hub_stamp,
                                  uint32_t stamp, uint32_t *count) {
  const int lane = wv::lane();
  if (count[0] < nlist) nlist = count[0];  // (count: [0] the list's length as k_bfs_collect left it, [1] the hub flag)
  cp_walk_vertices(
      tab, P, list, nlist, &count[1], lane,
      [&](uint32_t u) {  // (a hub: k_bc_edges_backward)
        if (lane == 0) hub_stamp[u] = stamp;
      },
      [&](uint32_t u, const Edge *items, const Node &nd) {
        const double su = sigma[u];
        double acc = 0.0;
        cp_walk_slots(items, nd, lane, [&](uint32_t val, uint32_t dst) {
          if (val != 0 && dst < n && levels[dst] == level + 1u) acc += bc_term(su, sigma[dst], delta[dst]);
        });
        acc = bc_reduce(acc, lane);
        if (lane == 0) delta[u] = acc;
      });
}
// Large level, or the hubs a per-vertex launch left: one streaming pass; the edges with the source among src_bits and the
// destination one level further add their term into delta[src].  A vertex's slots are contiguous, so the lanes of a wave
// share few sources: their runs are summed in the wave and one lane issues the add (cp_combine_runs); the other lanes add
// their own.
constexpr int kBcRunLanes = 8;  // lanes of a wave on one source from which its run is reduced before the atomic
PMA_KERNEL void k_bc_edges_backward(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t level,
                                    const uint32_t *__restrict__ src_bits, const uint32_t *__restrict__ levels,
                                    const double *__restrict__ sigma, double *delta) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&hit)[kB], int lane) {
    double sv[kB], sw[kB], dw[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && cp_bit(src_bits, src[b]);
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && levels[e[b].dest] == level + 1u;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      sv[b] = hit[b] ? sigma[src[b]] : 0.0;
      sw[b] = hit[b] ? sigma[e[b].dest] : 1.0;
      dw[b] = hit[b] ? delta[e[b].dest] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      double term = hit[b] ? bc_term(sv[b], sw[b], dw[b]) : 0.0;
      if (cp_combine_runs<kBcRunLanes>(hit[b], src[b], term, 0.0, lane, [](double x, int l) { return bc_reduce(x, l); }))
        bc_atomic_add(&delta[src[b]], term);
    }
  });
}

// bc[v] += delta[v] for every vertex but the source (endpoints are excluded)
PMA_KERNEL void k_bc_accumulate(double *bc, const double *delta, uint32_t n, uint32_t source) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride)
    if (v != source) bc[v] += delta[v];
}

}  // namespace ppcsr
