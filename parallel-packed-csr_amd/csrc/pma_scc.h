// Strongly connected components over the table of gapped arrays (pma_consumer.h): trimming, forward-backward reach from one
// pivot, colouring for what is left (Hong et al., SC'13; Slota et al., "Multistep", IPDPS'14; Orzan's colouring: PAPERS.md).
// The edge set is the one the BFS kernels walk — the live edges of cp_load_chunks — taken as DIRECTED; self-loops are dropped
// by every pass (they change no SCC).
//
// THE fact the schedule rests on.  Let R be a union of whole SCCs of G.  Then the SCCs of G - R are exactly the SCCs of G
// outside R.  Proof: take x, y outside R in one SCC of G; a path x -> y and a path y -> x exist in G, and every vertex z on
// either lies on a closed walk through x, so z is in SCC(x), which is not in R: both paths survive in G - R.  The converse
// (G - R has no new paths) is trivial.  So no phase tracks sub-partitions of the vertex set: every phase removes whole SCCs,
// and "unassigned" (scc[v] == kMax, the LIVE vertices) is the only set there is.  Every pass works on the graph induced by it.
//
// 1. Trim.  A live vertex with no live in-neighbour or no live out-neighbour (other than itself) lies on no cycle of more
//    than one vertex: it is an SCC of its own, scc[v] = v.  One sweep = one streaming pass that raises has_out[u] / has_in[w]
//    for every edge (u, w), u != w, with both ends live, and one per-vertex launch that retires the vertices lacking a flag
//    and rebuilds the live bitmap.  The flags are bytes under plain stores: every writer stores the same value (the argument
//    of k_bfs_edges_bits).  Sweeps repeat until one retires nothing.
// 2. Forward-backward.  From one live pivot p: FW = what p reaches, BW = what reaches p, both inside the live graph.
//    FW n BW = SCC(p) by definition.  Marks are bytes: 0 live and unmarked, 1 marked, 2 not live — so one gather answers
//    "live and not yet marked".  Reach has no levels: a pass reads the marks as they are, so a mark may travel several hops
//    in one pass and never needs more passes than BFS has levels; a pass that marks nothing ends the loop (such a pass has
//    stored nothing, so all it read was the state the launch began with: every edge is closed).  While both directions are
//    open ONE pass advances both.  Backward needs no transposed graph: it is the same pass with the roles of the two ends
//    exchanged, and since there a hub's lanes all mark the same source, runs of equal sources are cut to one store per wave.
// 3. Colouring, for the live rest.  colour[v] = v, then colour[w] = min(colour[w], colour[u]) over the live edges to a
//    fixpoint: colour[v] = the smallest live id that reaches v.  Roots: live r with colour[r] == r.
//    (a) A root is the smallest id of its SCC: every member of SCC(r) reaches r, so none of them is smaller than colour[r] = r.
//    (b) Backward reach from all roots at once along edges whose two ends carry the same colour marks, for colour r, exactly
//        SCC(r): a marked v reaches r, and colour[v] = r says r reaches v; conversely a member v of SCC(r) has colour r
//        (r reaches it, nothing smaller does, or that would reach r too) and a path to r inside SCC(r), all of colour r.
//    (c) The smallest live vertex is a root, so every round retires at least its SCC: the loop ends.
//    Marked vertices get scc[v] = colour[v] — by (a) the smallest id of the SCC — and leave the live set.
// After phase 2 and after every colouring round the trim runs again.
#pragma once
#include "pma_consumer.h"

namespace ppcsr {

constexpr uint32_t kSccStripeWords = 16;  // 64-bit striped counters, one 128-byte line each
constexpr uint8_t kSccOpen = 0, kSccMarked = 1, kSccDead = 2;

// ---- 1. trim -------------------------------------------------------------------------------------------------------------------
// The sweep's streaming pass.  A look at the flag first (possibly stale: then the store is repeated) keeps a hub's run from
// storing the same byte 64 times per wave.
PMA_KERNEL void k_scc_trim_edges(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ live_bits,
                                 uint8_t *has_out, uint8_t *has_in) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&live)[kB], int lane) {
    uint8_t fo[kB], fi[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) live[b] = live[b] && src[b] != e[b].dest && cp_bit(live_bits, src[b]) && cp_bit(live_bits, e[b].dest);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      fo[b] = live[b] ? has_out[src[b]] : (uint8_t)1;
      fi[b] = live[b] ? has_in[e[b].dest] : (uint8_t)1;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (!fo[b]) has_out[src[b]] = 1;
      if (!fi[b]) has_in[e[b].dest] = 1;
    }
  });
}
// The sweep's per-vertex launch, one wave per 64 consecutive vertices: a live vertex that lacks a flag is an SCC of its own;
// the live bitmap is rebuilt and the flags are cleared for the next sweep.  `found` counts the retired vertices.
PMA_KERNEL void k_scc_trim_retire(uint32_t *scc, uint32_t n, uint8_t *has_out, uint8_t *has_in, uint32_t *live_bits, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t mine = 0;
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t u = base + (uint64_t)lane;
    bool alive = false, keep = false;
    if (u < n) {
      alive = scc[u] == kMax;
      keep = alive && has_out[u] != 0 && has_in[u] != 0;
      has_out[u] = 0;
      has_in[u] = 0;
      if (alive && !keep) {
        scc[u] = (uint32_t)u;
        mine++;
      }
    }
    cp_store_bits(live_bits, base, wv::ballot(keep), lane);
  }
  cp_striped_add<unsigned long long, kSccStripeWords>(found, (unsigned long long)wv::reduce_add(mine), red);
}

// ---- 2. the pivot and the two reaches --------------------------------------------------------------------------------------------
// The pivot: the live vertex with the longest slot range, ties to the smaller id — read from nodes[], no pass over the arrays.
// *best = max over the live v of (range << 32 | ~v), which is never 0 (v <= 2^32 - 2); one atomic per workgroup (a few hundred
// on one word: thousands are served one after the other), and only when a plain look says it would raise the word.
PMA_KERNEL void k_scc_pivot(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ live_bits,
                            unsigned long long *best) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t hi = 0, lo = 0;  // the key's two halves
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    if (!cp_bit(live_bits, (uint32_t)v)) continue;
    const uint32_t k = P == 1 ? 0u : cp_owner(tab, P, (uint32_t)v);
    const Node nd = tab[k].nodes[(uint32_t)v - tab[k].first];
    const uint32_t range = nd.end - nd.beginning, inv = kMax - (uint32_t)v;
    if (range > hi || (range == hi && inv > lo)) {
      hi = range;
      lo = inv;
    }
  }
  // (the wave's largest key: the minimum of the complements)
  const unsigned long long wkey = ~cp_wave_min(~(((unsigned long long)hi << 32) | lo), lane);
  if (lane == 0) red[wv::wave_in_block()] = wkey;
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    unsigned long long key = red[0];
    for (int w = 1; w < 4; w++) key = red[w] > key ? red[w] : key;
    if (key > *best) wv::atomic_max_u64(best, key);
  }
}
// The marks of a reach: kSccDead off the live set, else kSccOpen — and, with colours, kSccMarked in bw[] on the roots
// (colour[v] == v).  fw may be null (the colouring rounds reach backward only).
PMA_KERNEL void k_scc_marks(const uint32_t *scc, uint32_t n, const uint32_t *colour, uint8_t *fw, uint8_t *bw) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    const bool dead = scc[v] != kMax;
    if (fw) fw[v] = dead ? kSccDead : kSccOpen;
    bw[v] = dead ? kSccDead : (colour && colour[v] == (uint32_t)v) ? kSccMarked : kSccOpen;
  }
}
// One streaming pass of the reach.  kFw: an edge whose source is marked in fw[] marks its open destination.  kBw: an edge whose
// destination is marked in bw[] marks its open source — with kCol only if both ends carry the same colour.  `found` counts
// the stores: forward ones in the low half of the word, backward ones in the high half (neither reaches 2^32: a pass has
// fewer than 2^32 edges per direction, a store needs an edge).
template <bool kFw, bool kBw, bool kCol>
PMA_DEV void scc_reach_pass(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *colour, uint8_t *fw, uint8_t *bw,
                            unsigned long long *found, unsigned long long *red) {
  uint32_t mine_f = 0, mine_b = 0;
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&live)[kB], int lane) {
    uint8_t fu[kB], fd[kB], bu[kB], bd[kB];
    bool wf[kB], wb[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) live[b] = live[b] && src[b] != e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (kFw) {
        fu[b] = live[b] ? fw[src[b]] : kSccOpen;
        fd[b] = live[b] ? fw[e[b].dest] : kSccDead;
      }
      if (kBw) {
        bd[b] = live[b] ? bw[e[b].dest] : kSccOpen;
        bu[b] = live[b] ? bw[src[b]] : kSccDead;
      }
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      wf[b] = kFw && fu[b] == kSccMarked && fd[b] == kSccOpen;
      wb[b] = kBw && bd[b] == kSccMarked && bu[b] == kSccOpen;
    }
    if (kCol) {
      uint32_t cu[kB], cd[kB];
#pragma unroll
      for (int b = 0; b < kB; b++) {
        cu[b] = wb[b] ? colour[src[b]] : 0u;
        cd[b] = wb[b] ? colour[e[b].dest] : 1u;
      }
#pragma unroll
      for (int b = 0; b < kB; b++) wb[b] = cu[b] == cd[b];
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (kFw && wf[b]) {
        fw[e[b].dest] = kSccMarked;
        mine_f++;
      }
      if (kBw) {
        // a vertex's slots are contiguous: of a run of lanes that mark the same source, the first one stores
        const uint64_t want = wv::ballot(wb[b]);
        const uint32_t prev = wv::shfl(src[b], (lane + 63) & 63);
        const bool dup = lane > 0 && ((want >> (lane - 1)) & 1ull) && prev == src[b];
        if (wb[b] && !dup) {
          bw[src[b]] = kSccMarked;
          mine_b++;
        }
      }
    }
  });
  const unsigned long long mine = (unsigned long long)wv::reduce_add(mine_f) | ((unsigned long long)wv::reduce_add(mine_b) << 32);
  cp_striped_add<unsigned long long, kSccStripeWords>(found, mine, red);
}
PMA_KERNEL void k_scc_reach_both(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint8_t *fw, uint8_t *bw, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  scc_reach_pass<true, true, false>(tab, P, n, nullptr, fw, bw, found, red);
}
PMA_KERNEL void k_scc_reach_fw(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint8_t *fw, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  scc_reach_pass<true, false, false>(tab, P, n, nullptr, fw, nullptr, found, red);
}
PMA_KERNEL void k_scc_reach_bw(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint8_t *bw, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  scc_reach_pass<false, true, false>(tab, P, n, nullptr, nullptr, bw, found, red);
}
PMA_KERNEL void k_scc_reach_colour(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *colour, uint8_t *bw,
                                   unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  scc_reach_pass<false, true, true>(tab, P, n, colour, nullptr, bw, found, red);
}
// *label = the smallest vertex marked in both fw[] and bw[]: one atomic per workgroup
PMA_KERNEL void k_scc_min(const uint8_t *fw, const uint8_t *bw, uint32_t n, uint32_t *label) {
  PMA_SHARED uint32_t red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t m = kMax;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride)
    if (fw[v] == kSccMarked && bw[v] == kSccMarked && (uint32_t)v < m) m = (uint32_t)v;
  m = cp_wave_min(m, lane);
  if (lane == 0) red[wv::wave_in_block()] = m;
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    for (int w = 1; w < 4; w++) m = red[w] < m ? red[w] : m;
    if (m < *label) wv::atomic_min_u32(label, m);
  }
}
// The vertices marked in bw[] — and in fw[], unless it is null — get their label (colour[v], or *label when colour is null)
// and leave the live set: the live bitmap is rebuilt, one wave per 64 consecutive vertices.  `found` counts them.
PMA_KERNEL void k_scc_assign(const uint8_t *fw, const uint8_t *bw, uint32_t n, const uint32_t *colour, const uint32_t *label, uint32_t *scc,
                             uint32_t *live_bits, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t mine = 0;
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t u = base + (uint64_t)lane;
    bool keep = false;
    if (u < n && scc[u] == kMax) {
      if (bw[u] == kSccMarked && (!fw || fw[u] == kSccMarked)) {
        scc[u] = colour ? colour[u] : *label;
        mine++;
      } else {
        keep = true;
      }
    }
    cp_store_bits(live_bits, base, wv::ballot(keep), lane);
  }
  cp_striped_add<unsigned long long, kSccStripeWords>(found, (unsigned long long)wv::reduce_add(mine), red);
}

// ---- 3. colouring ---------------------------------------------------------------------------------------------------------------
// colour[v] = v on the live vertices; kMax elsewhere, which lowers nothing as a source
PMA_KERNEL void k_scc_colour_init(const uint32_t *scc, uint32_t n, uint32_t *colour) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride)
    colour[v] = scc[v] == kMax ? (uint32_t)v : kMax;
}
// One streaming pass of the propagation: colour[w] = min(colour[w], colour[u]) over the edges into live vertices.  The atomic
// is issued only when a plain look says it would lower the word; the look may be stale — too large — so the atomic decides
// (sssp_relax_edge).  `found` counts the atomics that lowered their word.
PMA_KERNEL void k_scc_colour_prop(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ live_bits,
                                  uint32_t *colour, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  uint32_t mine = 0;
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&live)[kB], int lane) {
    uint32_t cu[kB], cd[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) live[b] = live[b] && src[b] != e[b].dest && cp_bit(live_bits, e[b].dest);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      cu[b] = live[b] ? colour[src[b]] : kMax;
      cd[b] = live[b] ? colour[e[b].dest] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kB; b++)
      if (cu[b] < cd[b] && wv::atomic_min_u32(&colour[e[b].dest], cu[b]) > cu[b]) mine++;
  });
  cp_striped_add<unsigned long long, kSccStripeWords>(found, (unsigned long long)wv::reduce_add(mine), red);
}

// the number of SCCs: the vertices that carry their own id
PMA_KERNEL void k_scc_count(const uint32_t *scc, uint32_t n, unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t mine = 0;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride)
    if (scc[v] == (uint32_t)v) mine++;
  cp_striped_add<unsigned long long, kSccStripeWords>(found, (unsigned long long)wv::reduce_add(mine), red);
}

}  // namespace ppcsr
