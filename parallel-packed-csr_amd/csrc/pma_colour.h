// Greedy vertex colouring and the maximal independent set over the table of gapped arrays (pma_consumer.h), both in the
// undirected graph G of pma_cores.h (the upper orientation: {a, b}, a < b < n, is an edge exactly when the pair (a, b) is
// stored) and both under ONE total order of the vertices, so that each has a unique answer (include/ppcsr.h):
//   u PRECEDES w  iff  key[u] > key[w], or the keys are equal and u < w        (k_col_keys: random / degree / id)
//   colour[v] = the smallest colour no preceding neighbour carries  (sequential greedy colouring in that order)
//   in_set[v] = no preceding neighbour is in the set                (the lexicographically first MIS in that order)
//
// The two are built differently, for the reasons pma_cores.h and pma_scc.h give for their own shapes.
//
// COLOURING exports (stage 1 of pma_cores.h: the compact symmetric adjacency) and then runs Jones-Plassmann rounds over
// frontiers (Jones, Plassmann 1993 — PAPERS.md).  Colouring v must look at v's neighbours in both directions and lower a
// counter at each of them, and the array indexes one direction only: k-core's reason.  pred[v] is the number of neighbours
// that precede v (k_col_pred: one streaming pass, the atomics shaped as k_kc_degree's); the first frontier is
// { v : pred[v] == 0 } (k_col_collect).  A ROUND gives every frontier vertex v a wave that walks v's list ONCE: a coloured
// neighbour's colour enters the forbidden set; at an uncoloured neighbour w the wave decrements pred[w], and the one decrement
// that returns 1 appends w to the next frontier; after the walk colour[v] = the first colour outside the forbidden set.
// Invariants, with F(r) the frontier of round r:
//  (1) pred[w] is decremented at most once per incident edge {v, w}, from v's side, when v — which enters one frontier once
//      (3) — is walked, and only while w is uncoloured, which (2) shows to mean "v precedes w": at most pred[w] times in all.
//  (2) When v is in F(r), every neighbour that precedes v is coloured and every neighbour that succeeds v is not.  v is listed
//      when pred[v] reaches 0 (or starts there), that is after every preceding neighbour u has been walked; u was walked in a
//      launch before this one (a vertex appended in a launch is walked in the next), and its colour was stored by that launch.
//      A succeeding neighbour w still counts v among its uncoloured predecessors: pred[w] >= 1, w is in no frontier so far.
//      So "colour[w] != kMax" IS the test for "w precedes v": no keys are read in the rounds.
//  (3) Two vertices of one frontier are never adjacent: of two adjacent vertices the later one is listed only after the
//      earlier one has been walked (2).  Hence no colour that a round reads is written by the same launch — the colours it
//      writes are those of frontier vertices, the colours it reads those of their neighbours — and every vertex enters
//      exactly one frontier: the only way in after the collect is the decrement 1 -> 0, which happens once.
//  (4) Every vertex is coloured at last: the order is total, so among the uncoloured vertices the first one has pred == 0 once
//      its (coloured) predecessors have been walked.  F(r) is exactly the set of vertices at level r of the order's DAG (level
//      0: no preceding neighbour; else 1 + the largest level of one): rounds and frontier sizes are functions of the graph
//      and the order, not of the schedule, and so is every colour — it is the greedy colour by induction over the levels.
//
// The forbidden set.  A list of at most kBfsWaveSlots = 4096 entries has mex <= 4096, so 4096 bits per wave decide it in one
// walk: 64 words of LDS, ORed into during the walk (ds_or_b64), lane l looking at word l afterwards.  A variant that kept the
// colours below 64 out of LDS — every lane ORing 1 << c into a register of its own, one xor butterfly over the 64 registers
// after the walk, LDS only for colours in [64, 4096) and not at all for a list of at most 64 entries — was built and measured
// against this one: it was 1.4 - 3.3 % SLOWER on every graph and order, beyond the run-to-run spread of either (at most
// 1.2 %; profiles/colouring_bench_low_word_variant.json), so the simpler kernel is the one here.  A list beyond 4096 entries
// is deferred, as k_kc_peel defers it, to k_col_long: a workgroup per vertex, a bitmap of `window` bits in LDS, the
// workgroup's waves walking the list in steps of 64; if every colour of the window is taken the next window makes another
// pass over the list (decrements in the first pass only).
//
// MIS works in place, with no export: a streaming pass does not care about hub degrees and the number of rounds is small for
// random orders (Luby 1986; Blelloch, Fineman, Shun 2012: the greedy sequential MIS has polylogarithmic dependence depth in a
// random order — PAPERS.md).  state[v] is UNDECIDED / IN / OUT.  Round r: k_mis_pass streams the upper edges {a, b} against
// the state of round r - 1 — an IN end marks the other end `out`; if both ends are UNDECIDED the succeeding end gets
// blocked = r — and k_mis_step turns an UNDECIDED vertex with `out` into OUT and one that is neither `out` nor blocked in
// round r into IN.  Soundness: v goes IN only when no neighbour is IN and no preceding neighbour is UNDECIDED, so every
// preceding neighbour is OUT: the definition; v goes OUT only next to an IN neighbour w, and w precedes v (were v before w,
// the UNDECIDED v would have blocked w in the round w went IN).  The pass only reads state[] and only the vertex launch writes
// it; the marks are plain stores of one value, so a round's outcome does not depend on the schedule.  The first UNDECIDED
// vertex of the order is never blocked: every round decides at least one vertex, and a vertex takes at most two rounds
// beyond its last preceding neighbour (that one goes IN, then this one OUT).
#pragma once
#include "pma_cores.h"
#include "pma_sample.h"  // sm_draw

namespace ppcsr {

constexpr uint32_t kColOrderRandom = 0, kColOrderDegree = 1, kColOrderId = 2;  // PPCSR_ORDER_* (include/ppcsr.h)
constexpr uint32_t kColWaveWords = (uint32_t)(kBfsWaveSlots / 64);             // 64-bit words of a wave's forbidden set
constexpr uint32_t kColWindowMax = 32768;                                      // colours per pass of k_col_long: 4 KiB of LDS
// counter block of the colouring loop: [0] vertices appended to the next frontier, [1] frontier vertices deferred to
// k_col_long, [2] window passes of k_col_long beyond each vertex's first, [3] the largest colour so far; padded as kKcCntWords
constexpr uint32_t kColCntWords = 8;
constexpr uint8_t kMisOut = 0, kMisIn = 1, kMisUndecided = 2;  // (once nothing is undecided, state[] is in_set[])
constexpr uint32_t kMisStripeWords = 16;                       // 64-bit striped counters, one 128-byte line each

// key[v] of the order (the table of include/ppcsr.h); deg: deg_G, read for kColOrderDegree only
PMA_KERNEL void k_col_keys(uint32_t order, unsigned long long seed, const uint32_t *__restrict__ deg, uint32_t n, unsigned long long *key) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    unsigned long long k = 0;
    if (order != kColOrderId) k = sm_draw(seed, v, 0);
    if (order == kColOrderDegree) k = ((unsigned long long)deg[v] << 32) | (k >> 32);
    key[v] = k;
  }
}
PMA_DEV bool col_precedes(unsigned long long ku, uint32_t u, unsigned long long kw, uint32_t w) { return ku > kw || (ku == kw && u < w); }

// ---- colouring ---------------------------------------------------------------------------------------------------------------------------
// pred[v] = neighbours that precede v: per upper edge one add at the succeeding end.  The source side is counted within the
// wave for a hub's run (kc_source_runs), the destination side is one atomic per edge: the shape of k_kc_degree.
PMA_KERNEL void k_col_pred(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ key, uint32_t *pred) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&a)[kB], bool(&up)[kB], int lane) {
    unsigned long long ka[kB], kb[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) up[b] = up[b] && a[b] < e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      ka[b] = up[b] ? key[a[b]] : 0ull;
      kb[b] = up[b] ? key[e[b].dest] : 0ull;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const bool fwd = col_precedes(ka[b], a[b], kb[b], e[b].dest);  // the source precedes: the destination counts it
      bool lead;
      uint32_t cnt, rank;
      int leader;
      kc_source_runs(up[b] && !fwd, a[b], lane, lead, cnt, rank, leader);
      if (lead) wv::atomic_add_u32(&pred[a[b]], cnt);
      if (up[b] && fwd) wv::atomic_add_u32(&pred[e[b].dest], 1u);
    }
  });
}
// the first frontier: every vertex without a preceding neighbour
PMA_KERNEL void k_col_collect(const uint32_t *__restrict__ pred, uint32_t n, uint32_t *front, uint32_t *cnt) {
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t u = base + (uint64_t)lane;
    cp_append(u < n && pred[u] == 0u, (uint32_t)u, front, cnt, lane);
  }
}
// cnt[3] = the largest colour: a look first (stale means too small: then the atomic is issued for nothing), so that the
// thousands of vertices with small colours do not queue on one word
PMA_DEV void col_note_colour(uint32_t c, uint32_t *cnt) {
  if (c > cnt[3]) wv::atomic_max_u32(&cnt[3], c);
}
// adj[b, e) of frontier vertex v, 64 entries per `step`: coloured neighbours into the forbidden set (colours in
// [lo, lo + span) into bits[]), uncoloured ones decremented and, at 1 -> 0, appended
PMA_DEV void col_walk_range(const uint32_t *__restrict__ adj, uint64_t b, uint64_t e, uint64_t step, int lane, const uint32_t *colour, uint32_t lo,
                            uint32_t span, bool decrement, unsigned long long *bits, uint32_t *pred, uint32_t *next, uint32_t *cnt) {
  for (uint64_t base = b; base < e; base += step) {
    const uint64_t i = base + (uint64_t)lane;
    uint32_t w = 0;
    bool won = false;
    if (i < e) {
      w = adj[i];
      const uint32_t c = colour[w];
      if (c == kMax) {
        if (decrement) won = wv::atomic_add_u32(&pred[w], 0xFFFFFFFFu) == 1u;
      } else if (c - lo < span) {
        wv::lds_or_u64(&bits[(c - lo) >> 6], 1ull << ((c - lo) & 63u));
      }
    }
    if (decrement) cp_append(won, w, next, cnt, lane);
  }
}
// one round: a wave per frontier vertex; a list beyond kBfsWaveSlots entries is left to k_col_long (longl, cnt[1])
PMA_KERNEL void k_col_round(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ front,
                            uint32_t nfront, uint32_t *colour, uint32_t *pred, uint32_t *next, uint32_t *longl, uint32_t *cnt) {
  PMA_SHARED unsigned long long forbid[4][kColWaveWords];
  const int lane = wv::lane();
  unsigned long long *const bits = forbid[wv::wave_in_block()];
  const uint64_t wstride = cp_waves();
  for (uint64_t f = cp_wave(); f < nfront; f += wstride) {
    const uint32_t v = wv::uni(front[f]);
    const uint64_t b = off[v], e = off[(uint64_t)v + 1];
    if (e - b > kBfsWaveSlots) {
      if (lane == 0) longl[wv::atomic_add_u32(&cnt[1], 1u)] = v;
      continue;
    }
    uint32_t c = 0;
    if (e > b) {  // (wave-uniform; a vertex without neighbours takes colour 0)
      bits[lane] = 0ull;
      wv::lds_fence();
      col_walk_range(adj, b, e, 64, lane, colour, 0u, (uint32_t)kBfsWaveSlots, true, bits, pred, next, cnt);
      wv::lds_fence();
      // lane l looks at word l; no free bit at all: the list has 4096 entries with the colours 0 .. 4095
      const unsigned long long word = bits[lane];
      const uint64_t open = wv::ballot(~word != 0ull);
      c = (uint32_t)kBfsWaveSlots;
      if (open) {
        const int l = wv::ctz64(open);
        const unsigned long long wl = ((unsigned long long)wv::bcast((uint32_t)(word >> 32), l) << 32) | wv::bcast((uint32_t)word, l);
        c = (uint32_t)l * 64u + (uint32_t)wv::ctz64(~wl);
      }
      wv::lds_fence();  // (the next vertex of this wave clears the words)
    }
    if (lane == 0) {
      colour[v] = c;
      col_note_colour(c, cnt);
    }
  }
}
// The deferred lists of the round: a workgroup per vertex (every grid_dim-th list), its four waves walking the list in steps of
// 64 entries, the forbidden colours of [lo, lo + window) in LDS; the first free one is the colour, and a full window moves on
// to the next one with another pass over the list (cnt[2] counts those).  mex <= list length, so the loop ends.
PMA_KERNEL void k_col_long(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj, const uint32_t *__restrict__ longl,
                           uint32_t nlong, uint32_t window, uint32_t *colour, uint32_t *pred, uint32_t *next, uint32_t *cnt) {
  PMA_SHARED unsigned long long bits[kColWindowMax / 64];
  PMA_SHARED uint32_t red[4];
  const int lane = wv::lane(), wave = wv::wave_in_block();
  const uint32_t words = window >> 6;
  for (uint64_t i = wv::block_idx(); i < nlong; i += wv::grid_dim()) {
    const uint32_t v = wv::uni(longl[i]);
    const uint64_t b = off[v], e = off[(uint64_t)v + 1];
    for (uint64_t lo = 0;; lo += window) {  // (block-uniform: every thread sees the same red[])
      for (uint32_t j = wv::thread_idx(); j < words; j += wv::block_dim()) bits[j] = 0ull;
      wv::block_sync();
      col_walk_range(adj, b + (uint64_t)wave * 64, e, 256, lane, colour, (uint32_t)lo, window, lo == 0, bits, pred, next, cnt);
      wv::block_sync();
      uint32_t free_bit = kMax;
      for (uint32_t j = wv::thread_idx(); j < words && free_bit == kMax; j += wv::block_dim())
        if (~bits[j] != 0ull) free_bit = j * 64u + (uint32_t)wv::ctz64(~bits[j]);
      free_bit = cp_wave_min(free_bit, lane);
      if (lane == 0) red[wave] = free_bit;
      wv::block_sync();
      for (int q = 0; q < 4; q++) free_bit = red[q] < free_bit ? red[q] : free_bit;
      if (free_bit != kMax) {
        if (wv::thread_idx() == 0) {
          colour[v] = (uint32_t)lo + free_bit;
          col_note_colour((uint32_t)lo + free_bit, cnt);
        }
        break;
      }
      if (wv::thread_idx() == 0) wv::atomic_add_u32(&cnt[2], 1u);
    }
    wv::block_sync();  // (red[] and bits[] are the next vertex's)
  }
}

// ---- maximal independent set ---------------------------------------------------------------------------------------------------------
// The pass of round r.  Phases: the two states; the two keys where both ends are undecided ("after the first rounds most
// edges have a decided end": the states are looked at first); a look at the mark (possibly stale: then the store is
// repeated — it keeps a hub's run from storing one byte 64 times per wave, as k_scc_trim_edges); the stores.
PMA_KERNEL void k_mis_pass(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t r, const unsigned long long *__restrict__ key,
                           const uint8_t *__restrict__ state, uint8_t *out, uint32_t *blocked) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&a)[kB], bool(&up)[kB], int) {
    uint8_t sa[kB], sb[kB];
    unsigned long long ka[kB], kb[kB];
    uint32_t mark[kB], block[kB];  // the vertex to mark `out` / to block (kMax: none)
    bool both[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) up[b] = up[b] && a[b] < e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      sa[b] = up[b] ? state[a[b]] : kMisOut;
      sb[b] = up[b] ? state[e[b].dest] : kMisOut;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      both[b] = sa[b] == kMisUndecided && sb[b] == kMisUndecided;
      ka[b] = both[b] ? key[a[b]] : 0ull;
      kb[b] = both[b] ? key[e[b].dest] : 0ull;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      mark[b] = block[b] = kMax;
      if (sa[b] == kMisIn && sb[b] == kMisUndecided) mark[b] = e[b].dest;
      if (sb[b] == kMisIn && sa[b] == kMisUndecided) mark[b] = a[b];
      if (both[b]) block[b] = col_precedes(ka[b], a[b], kb[b], e[b].dest) ? e[b].dest : a[b];
      if (mark[b] != kMax && out[mark[b]] != 0) mark[b] = kMax;
      if (block[b] != kMax && blocked[block[b]] == r) block[b] = kMax;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (mark[b] != kMax) out[mark[b]] = 1;
      if (block[b] != kMax) blocked[block[b]] = r;
    }
  });
}
// The vertex launch of round r.  found: the striped count — vertices still undecided in the low half of the word, vertices
// that went IN in the high half (neither reaches 2^32: both count vertices).
PMA_KERNEL void k_mis_step(uint32_t n, uint32_t r, uint8_t *state, const uint8_t *__restrict__ out, const uint32_t *__restrict__ blocked,
                           unsigned long long *found) {
  PMA_SHARED unsigned long long red[4];
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t left = 0, in = 0;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    if (state[v] != kMisUndecided) continue;
    if (out[v] != 0) {
      state[v] = kMisOut;
    } else if (blocked[v] != r) {
      state[v] = kMisIn;
      in++;
    } else {
      left++;
    }
  }
  const unsigned long long mine = ((unsigned long long)wv::reduce_add(in) << 32) | (unsigned long long)wv::reduce_add(left);
  cp_striped_add<unsigned long long, kMisStripeWords>(found, mine, red);
}

}  // namespace ppcsr
