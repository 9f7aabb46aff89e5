// Label-propagation communities and modularity over the table of gapped arrays (pma_consumer.h), in the undirected graph G of
// pma_cores.h (the upper orientation: {a, b}, a < b < n, is an edge exactly when the pair (a, b) is stored).  The weight of
// {a, b} is that pair's stored value (weighted form) or 1.  The definition is in include/ppcsr.h; in short:
//   class c  = the vertices of colour c (ppcsr_colouring under the call's order and seed) that have a neighbour
//   a STEP   handles one class: every v of it scores each label by the weight of v's edges to neighbours carrying it (64-bit
//            sums) and, unless its own label reaches the largest score M, takes the smallest label that does
//   a SWEEP  runs the classes 0, 1, ... in turn; the call ends after the first sweep that changes nothing (or max_sweeps)
// A class is an independent set, so a step reads no label that it writes: labels are updated in place, and the result is that
// of the sequential sweep in (colour, id) order — one answer per order and seed, whatever the schedule.  This is the
// semi-synchronous scheme of Cordasco and Gargano 2010 on the label propagation of Raghavan, Albert, Kumara 2007.
// Termination: v changes its label only to one of strictly larger score, and no neighbour of v moves in the same step, so every
// change raises the total weight of the edges whose ends agree by at least 1; that total is bounded by W(G).
//
// The call exports like the colouring does and reuses its stage whole: the compact symmetric adjacency (pma_cores.h) and the
// colours stay on the device.  The weighted form fills a second adjacency of 8-byte entries, (weight << 32) | neighbour
// (k_lp_fill_weighted: k_kc_fill with the value beside the neighbour).  Then a counting sort of the vertices that have a
// neighbour by bucket 3 * colour + tier (k_lp_hist / k_lp_scan / k_lp_class_fill; the order inside a bucket is free: its
// vertices do not see each other) and ONE host read of the bucket offsets: from then on a step is at most three launches over
// host-known ranges of the list, and a sweep costs one read of the striped counters (the number of changes).
//
// The tiers, by list length (the weighted mode of a list is found where the list fits):
//   <= kLpLaneList = 64      k_lp_step_lanes: a wave per vertex, an entry per lane, no LDS.  The distinct labels are retired one
//                            per iteration: broadcast a pending lane's label, ballot the equal ones, add their weights up in
//                            the wave.  After convergence that is one iteration per vertex.
//   <= kLpWaveList = 512     k_lp_step_wave: a wave per vertex and an open-addressing table of its own in LDS (keys claimed by
//                            compare-and-swap, 64-bit scores added with ds_add_u64), sized to the list — the next power of two
//                            >= 2 * length, so a list of 65 entries clears 256 slots and not 1024 — then every lane looks at
//                            its slots and the wave reduces.  512: the table of the longest list (1024 slots, 12 KiB) times
//                            four waves is 48 KiB, which leaves three workgroups to a CU; a retire loop over such lists would
//                            run up to 512 iterations of a broadcast and two ballots in the first sweep, where labels differ.
//   longer                   k_lp_step_block: a workgroup per vertex, one table of `slots` slots (the option "lp_table_slots",
//                            at most kLpTableMax = 4096: 48 KiB).  In the first sweep a hub sees as many labels as it has
//                            neighbours, so the table can overflow: the labels are split into K classes by hash, pass k of K
//                            takes those of class k and the best (score, label) and the own label's score are carried
//                            across the passes.  K starts at 1; a pass that claims more than 3/4 of the slots (or finds
//                            none free) gives up, K doubles and the vertex starts over, block-uniformly.  Every pass
//                            rereads the whole list and the labels of all its neighbours: O(K * length) global reads
//                            for the K that succeeds (and as much again for the ones that gave up) — K = 4 with the
//                            shipped 4096 slots for a list of 9192 distinct labels (the longest of the scale-18 test
//                            graph, in its first sweep), 256 with the 64 slots of the tests.  The hash is a bijection of 32-bit words, so K = kLpMaxClasses = 2^26
//                            leaves no pass more than 64 labels and the loop ends; a vertex that overflowed even
//                            there is counted (kLpCntFault) and the driver reports an error instead of trusting that.
// Everywhere the comparison over a whole list is (score descending, label ascending), then the own-label rule.
// The converged regime: once labels settle, most of a list carries ONE label, and 64 lanes adding to one LDS word are served
// one after the other.  lp_insert therefore first combines, in registers, the lanes that share the wave's first pending label
// and lets one of them issue the sum.  (cp_combine_runs of pma_consumer.h is the same idea for global atomics and is what
// lp_tot_add uses; it is not used in lp_insert, which runs once per 64 entries of every list: it looks at both ends of the
// wave and reduces with twelve shuffles each, where here only the head matters, an unweighted run's sum is the popcount of
// its ballot and a weighted one's is two DPP sums of 16-bit halves.)
//
// Modularity takes any labels: one streaming pass (k_lp_mod_pass) adds the weight of every upper edge to tot[label] of both
// ends (64-bit atomics; one per wave where all lanes of a chunk agree) and, per workgroup, the total weight and the weight
// inside communities to striped counters; a vertex pass (k_lp_mod_squares) sums tot_c^2 in 128 bits per thread and writes one
// (lo, hi) partial per workgroup.  The host adds the partials and forms q in doubles.
#pragma once
#include "pma_colour.h"

namespace ppcsr {

constexpr uint32_t kLpWeighted = 1u;                    // PPCSR_COMMUNITY_WEIGHTED (include/ppcsr.h)
constexpr uint32_t kLpLaneList = 64, kLpWaveList = 512;  // longest list of the first / second tier
constexpr uint32_t kLpWaveSlots = 2 * kLpWaveList;      // table of one wave of k_lp_step_wave
constexpr uint32_t kLpTableMax = 4096;                  // table of k_lp_step_block: the default and the top of "lp_table_slots"
constexpr uint32_t kLpStripeWords = 16;                 // 64-bit striped counters, one 128-byte line per stripe
constexpr uint32_t kLpMaxClasses = 1u << 26;            // hash classes of k_lp_step_block beyond which it gives up (never reached)
// words of a stripe: label changes of the sweep, hash passes of k_lp_step_block beyond each vertex's first, labels in use,
// vertices k_lp_step_block gave up on
constexpr uint32_t kLpCntChanges = 0, kLpCntPasses = 1, kLpCntLabels = 2, kLpCntFault = 3;
constexpr uint32_t kLpCntInside = 0, kLpCntWeight = 1;  // (modularity: weight inside communities, W(G))

PMA_DEV uint32_t lp_tier(unsigned long long len) { return len <= kLpLaneList ? 0u : len <= kLpWaveList ? 1u : 2u; }
// a bijection of 32-bit words (the finaliser of MurmurHash3): low bits choose the pass, bits from 16 up the first slot
PMA_DEV uint32_t lp_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
// entry i of a list: the neighbour and the edge's weight
template <bool kW>
PMA_DEV void lp_entry(const uint32_t *__restrict__ adj, const unsigned long long *__restrict__ wadj, uint64_t i, uint32_t &nb, uint32_t &w) {
  if (kW) {
    const unsigned long long x = wadj[i];
    nb = (uint32_t)x;
    w = (uint32_t)(x >> 32);
  } else {
    nb = adj[i];
    w = 1u;
  }
}
// sum of one 32-bit word per lane as 64 bits, in every lane (two 16-bit halves: neither sum reaches 2^22)
PMA_DEV unsigned long long lp_wave_sum(uint32_t w) {
  return (unsigned long long)wv::reduce_add(w & 0xFFFFu) + ((unsigned long long)wv::reduce_add(w >> 16) << 16);
}
PMA_DEV unsigned long long lp_wave_sum64(unsigned long long v, int lane) {
  for (int d = 1; d < 64; d <<= 1) v += cp_shfl(v, lane ^ d);
  return v;
}
PMA_DEV bool lp_better(unsigned long long s, uint32_t l, unsigned long long than_s, uint32_t than_l) { return s > than_s || (s == than_s && l < than_l); }
// the best (score, label) and the largest own score over the wave, in every lane
PMA_DEV void lp_wave_best(unsigned long long &s, uint32_t &l, unsigned long long &own, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long os = cp_shfl(s, lane ^ d), oo = cp_shfl(own, lane ^ d);
    const uint32_t ol = cp_shfl(l, lane ^ d);
    if (lp_better(os, ol, s, l)) {
      s = os;
      l = ol;
    }
    own = oo > own ? oo : own;
  }
}
// this workgroup's count into word `word` of its stripe (cp_striped_add on the stripes of that word; a kernel that counts
// twice gives each count its own red[])
PMA_DEV void lp_count(unsigned long long *stripes, uint32_t word, unsigned long long mine, unsigned long long *red) {
  cp_striped_add<unsigned long long, kLpStripeWords>(stripes + word, mine, red);
}

// ---- the weighted adjacency and the class lists -----------------------------------------------------------------------------------------
// k_kc_fill with the value beside the neighbour: (value << 32) | neighbour, at both ends of every upper edge
PMA_KERNEL void k_lp_fill_weighted(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ off,
                                   uint32_t *fill, unsigned long long *wadj) {
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
        const unsigned long long w = (unsigned long long)e[b].value << 32;
        wadj[off[a[b]] + base + rank] = w | e[b].dest;
        wadj[off[e[b].dest] + wv::atomic_add_u32(&fill[e[b].dest], 1u)] = w | a[b];
      }
    }
  });
}
// hist[3 * colour + tier]: the vertices with a neighbour
PMA_KERNEL void k_lp_hist(const uint32_t *__restrict__ colour, const unsigned long long *__restrict__ off, uint32_t n, uint32_t *hist) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    const unsigned long long len = off[v + 1] - off[v];
    if (len) wv::atomic_add_u32(&hist[3u * colour[v] + lp_tier(len)], 1u);
  }
}
// <<<1, 64>>>: exclusive scan of hist[0, buckets) into first[0, buckets] and a copy of it, the cursors of the fill
PMA_KERNEL void k_lp_scan(const uint32_t *__restrict__ hist, uint32_t buckets, uint32_t *first, uint32_t *cursor) {
  const int lane = wv::lane();
  unsigned long long carry = 0;
  for (uint64_t base = 0; base < buckets; base += 64) {
    const uint64_t i = base + (uint64_t)lane;
    const unsigned long long v = i < buckets ? hist[i] : 0u;
    const unsigned long long s = kc_wave_scan(v, lane);
    if (i < buckets) first[i] = cursor[i] = (uint32_t)(carry + s - v);
    carry += cp_shfl(s, 63);
  }
  if (lane == 0) first[buckets] = (uint32_t)carry;
}
PMA_KERNEL void k_lp_class_fill(const uint32_t *__restrict__ colour, const unsigned long long *__restrict__ off, uint32_t n, uint32_t *cursor,
                                uint32_t *list) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    const unsigned long long len = off[v + 1] - off[v];
    if (len) list[wv::atomic_add_u32(&cursor[3u * colour[v] + lp_tier(len)], 1u)] = (uint32_t)v;
  }
}
// label[v] = v
PMA_KERNEL void k_lp_identity(uint32_t *label, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) label[v] = (uint32_t)v;
}

// ---- the step kernels ----------------------------------------------------------------------------------------------------------------
// the rule at the end of a list: own scores M (>= 1: the list is not empty and weights are not 0) — keep; else the best label
PMA_DEV uint32_t lp_decide(uint32_t own, unsigned long long own_score, unsigned long long best_score, uint32_t best_label) {
  return own_score == best_score ? own : best_label;
}
// first tier: an entry per lane
template <bool kW>
PMA_KERNEL void k_lp_step_lanes(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj,
                                const unsigned long long *__restrict__ wadj, const uint32_t *__restrict__ list, uint32_t count, uint32_t *label,
                                unsigned long long *stripes) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  const uint64_t wstride = cp_waves();
  unsigned long long changes = 0;
  for (uint64_t f = cp_wave(); f < count; f += wstride) {
    const uint32_t v = wv::uni(list[f]);
    const uint64_t b = off[v];
    const uint32_t len = (uint32_t)(off[(uint64_t)v + 1] - b);
    const uint32_t own = wv::uni(label[v]);
    const bool have = (uint32_t)lane < len;
    uint32_t nb = 0, w = 0, l = 0;
    if (have) {
      lp_entry<kW>(adj, wadj, b + (uint64_t)lane, nb, w);
      l = label[nb];
    }
    unsigned long long best_score = 0, own_score = 0;
    uint32_t best_label = kMax;
    for (uint64_t pend = wv::ballot(have); pend;) {
      const uint32_t cand = wv::bcast(l, wv::ctz64(pend));
      const bool eq = have && l == cand;
      const uint64_t m = wv::ballot(eq);
      const unsigned long long s = kW ? lp_wave_sum(eq ? w : 0u) : (unsigned long long)wv::popc64(m);
      if (lp_better(s, cand, best_score, best_label)) {
        best_score = s;
        best_label = cand;
      }
      if (cand == own) own_score = s;
      pend &= ~m;
    }
    const uint32_t now = lp_decide(own, own_score, best_score, best_label);
    if (now != own) {
      if (lane == 0) label[v] = now;
      changes++;
    }
  }
  lp_count(stripes, kLpCntChanges, changes, red);
}

// The lanes with `have` add w to the score of label l in the table keys[] / score[] of mask + 1 slots (whole wave).  The lanes
// that share the first pending label are combined first.  used / cap / overflow (k_lp_step_block; null in a table that cannot
// fill): slots claimed so far, the number from which the pass gives up, the flag that says so.
template <bool kW>
PMA_DEV void lp_insert(bool have, uint32_t l, uint32_t w, uint32_t *keys, unsigned long long *score, uint32_t mask, int lane, uint32_t *used,
                       uint32_t cap, uint32_t *overflow) {
  const uint64_t pend = wv::ballot(have);
  if (pend == 0) return;
  const uint32_t head = wv::bcast(l, wv::ctz64(pend));
  const bool eq = have && l == head;
  const uint64_t m = wv::ballot(eq);
  unsigned long long add = w;
  if (wv::popc64(m) > 1) {
    const unsigned long long s = kW ? lp_wave_sum(eq ? w : 0u) : (unsigned long long)wv::popc64(m);
    if (eq) {
      have = lane == wv::ctz64(m);
      add = s;
    }
  }
  if (!have) return;
  uint32_t h = (lp_hash(l) >> 16) & mask;
  for (uint32_t probes = 0; probes <= mask; probes++, h = (h + 1u) & mask) {
    uint32_t k = keys[h];  // (a look: stale means still empty, and then the compare-and-swap decides)
    if (k == kMax) {
      if (used && *(volatile uint32_t *)used >= cap) break;
      k = wv::lds_cas_u32(&keys[h], kMax, l);
      if (k == kMax) {
        if (used) wv::atomic_add_u32(used, 1u);
        k = l;
      }
    }
    if (k == l) {
      wv::lds_add_u64(&score[h], add);
      return;
    }
  }
  if (overflow) *(volatile uint32_t *)overflow = 1u;  // (never reached without `used`: such a table has a free slot for every label)
}
// this lane's share of the slots [first, slots) in steps of `step`: the best entry and the own label's score
PMA_DEV void lp_scan_slots(const uint32_t *keys, const unsigned long long *score, uint32_t first, uint32_t slots, uint32_t step, uint32_t own,
                           unsigned long long &best_score, uint32_t &best_label, unsigned long long &own_score) {
  for (uint32_t j = first; j < slots; j += step) {
    const uint32_t k = keys[j];
    if (k == kMax) continue;
    const unsigned long long s = score[j];
    if (lp_better(s, k, best_score, best_label)) {
      best_score = s;
      best_label = k;
    }
    if (k == own) own_score = s;
  }
}
// second tier: a wave per vertex, a table per wave
template <bool kW>
PMA_KERNEL void k_lp_step_wave(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj,
                               const unsigned long long *__restrict__ wadj, const uint32_t *__restrict__ list, uint32_t count, uint32_t *label,
                               unsigned long long *stripes) {
  PMA_SHARED uint32_t keys_all[4][kLpWaveSlots];
  PMA_SHARED unsigned long long score_all[4][kLpWaveSlots];
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  uint32_t *const keys = keys_all[wv::wave_in_block()];
  unsigned long long *const score = score_all[wv::wave_in_block()];
  const uint64_t wstride = cp_waves();
  unsigned long long changes = 0;
  for (uint64_t f = cp_wave(); f < count; f += wstride) {
    const uint32_t v = wv::uni(list[f]);
    const uint64_t b = off[v], e = off[(uint64_t)v + 1];
    const uint32_t own = wv::uni(label[v]);
    uint32_t slots = 2u * kLpLaneList;
    while (slots < 2u * (uint32_t)(e - b) && slots < kLpWaveSlots) slots <<= 1;  // (the host sends lists of at most kLpWaveList entries)
    for (uint32_t j = (uint32_t)lane; j < slots; j += 64u) {
      keys[j] = kMax;
      score[j] = 0ull;
    }
    wv::lds_fence();
    for (uint64_t base = b; base < e; base += 64) {
      const uint64_t i = base + (uint64_t)lane;
      uint32_t nb = 0, w = 0, l = 0;
      if (i < e) {
        lp_entry<kW>(adj, wadj, i, nb, w);
        l = label[nb];
      }
      lp_insert<kW>(i < e, l, w, keys, score, slots - 1u, lane, nullptr, 0u, nullptr);
    }
    wv::lds_fence();
    unsigned long long best_score = 0, own_score = 0;
    uint32_t best_label = kMax;
    lp_scan_slots(keys, score, (uint32_t)lane, slots, 64u, own, best_score, best_label, own_score);
    lp_wave_best(best_score, best_label, own_score, lane);
    wv::lds_fence();  // (the next vertex of this wave clears the table)
    const uint32_t now = lp_decide(own, own_score, best_score, best_label);
    if (now != own) {
      if (lane == 0) label[v] = now;
      changes++;
    }
  }
  lp_count(stripes, kLpCntChanges, changes, red);
}
// third tier: a workgroup per vertex (every grid_dim-th of the list), the labels in K hash classes, a pass per class
template <bool kW>
PMA_KERNEL void k_lp_step_block(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ adj,
                                const unsigned long long *__restrict__ wadj, const uint32_t *__restrict__ list, uint32_t count, uint32_t slots,
                                uint32_t *label, unsigned long long *stripes) {
  PMA_SHARED uint32_t keys[kLpTableMax];
  PMA_SHARED unsigned long long score[kLpTableMax];
  PMA_SHARED unsigned long long red_score[4], red_own[4], red[3][4];
  PMA_SHARED uint32_t red_label[4];
  PMA_SHARED uint32_t ctl[2];  // slots claimed by the pass; the pass has given up
  const int lane = wv::lane(), wave = wv::wave_in_block();
  const uint32_t cap = slots - (slots >> 2);
  unsigned long long changes = 0, extra = 0, faults = 0;
  for (uint64_t i = wv::block_idx(); i < count; i += wv::grid_dim()) {
    const uint32_t v = wv::uni(list[i]);
    const uint64_t b = off[v], e = off[(uint64_t)v + 1];
    const uint32_t own = wv::uni(label[v]);
    unsigned long long best_score = 0, own_score = 0, passes = 0;
    uint32_t best_label = kMax;
    for (uint32_t K = 1;; K <<= 1) {  // (block-uniform: every thread reads the same ctl[] and red_*[])
      best_score = own_score = 0;
      best_label = kMax;
      bool over = false;
      for (uint32_t k = 0; k < K && !over; k++) {
        passes++;
        for (uint32_t j = wv::thread_idx(); j < slots; j += wv::block_dim()) {
          keys[j] = kMax;
          score[j] = 0ull;
        }
        if (wv::thread_idx() == 0) ctl[0] = ctl[1] = 0u;
        wv::block_sync();
        for (uint64_t base = b + (uint64_t)wave * 64; base < e; base += 256) {
          const uint64_t at = base + (uint64_t)lane;
          uint32_t nb = 0, w = 0, l = 0;
          bool have = at < e;
          if (have) {
            lp_entry<kW>(adj, wadj, at, nb, w);
            l = label[nb];
            have = (lp_hash(l) & (K - 1u)) == k;
          }
          lp_insert<kW>(have, l, w, keys, score, slots - 1u, lane, &ctl[0], cap, &ctl[1]);
        }
        wv::block_sync();
        over = ctl[1] != 0u;
        if (!over) {
          unsigned long long s = 0, o = 0;
          uint32_t l = kMax;
          lp_scan_slots(keys, score, wv::thread_idx(), slots, wv::block_dim(), own, s, l, o);
          lp_wave_best(s, l, o, lane);
          if (lane == 0) {
            red_score[wave] = s;
            red_label[wave] = l;
            red_own[wave] = o;
          }
          wv::block_sync();
          for (int q = 0; q < 4; q++) {
            if (lp_better(red_score[q], red_label[q], best_score, best_label)) {
              best_score = red_score[q];
              best_label = red_label[q];
            }
            own_score = red_own[q] > own_score ? red_own[q] : own_score;
          }
        }
        wv::block_sync();  // (the next pass clears the table, ctl[] and red_*[])
      }
      if (!over) break;
      if (K == kLpMaxClasses) {  // (checked, not trusted: the vertex keeps its label and the driver reports it)
        faults++;
        best_score = own_score = 0;
        break;
      }
    }
    extra += passes - 1;
    const uint32_t now = lp_decide(own, own_score, best_score, best_label);
    if (now != own) {
      if (wv::thread_idx() == 0) label[v] = now;
      changes++;
    }
  }
  // (one count per workgroup: wave 0 speaks for it)
  lp_count(stripes, kLpCntChanges, wave == 0 ? changes : 0ull, red[0]);
  lp_count(stripes, kLpCntPasses, wave == 0 ? extra : 0ull, red[1]);
  lp_count(stripes, kLpCntFault, wave == 0 ? faults : 0ull, red[2]);
}

// ---- the number of communities ---------------------------------------------------------------------------------------------------------
PMA_KERNEL void k_lp_mark(const uint32_t *__restrict__ label, uint32_t n, uint8_t *mark) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) mark[label[v]] = 1;
}
PMA_KERNEL void k_lp_count_marks(const uint8_t *__restrict__ mark, uint32_t n, unsigned long long *stripes) {
  PMA_SHARED unsigned long long red[4];
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t mine = 0;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) mine += mark[v];
  lp_count(stripes, kLpCntLabels, wv::reduce_add(mine), red);
}

// ---- modularity ------------------------------------------------------------------------------------------------------------------------
// tot[label] += w from the lanes with `up`: the runs of one label at the ends of the wave — in the settled regime the whole
// wave — are added up in the wave and issued once (cp_combine_runs, as k_cc_hook's minima)
PMA_DEV void lp_tot_add(bool up, uint32_t l, unsigned long long w, unsigned long long *tot, int lane) {
  const bool issue = cp_combine_runs<kCcRunLanes>(up, l, w, 0ull, lane, [](unsigned long long x, int ln) { return lp_wave_sum64(x, ln); });
  if (issue) wv::atomic_add_u64(&tot[l], w);
}
template <bool kW>
PMA_KERNEL void k_lp_mod_pass(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ label,
                              unsigned long long *tot, unsigned long long *stripes) {
  PMA_SHARED unsigned long long red[2][4];
  constexpr int kB = 4;
  unsigned long long inside = 0, weight = 0;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&a)[kB], bool(&up)[kB], int lane) {
    uint32_t la[kB], lb[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) up[b] = up[b] && a[b] < e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      la[b] = up[b] ? label[a[b]] : 0u;
      lb[b] = up[b] ? label[e[b].dest] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      const unsigned long long w = kW ? (unsigned long long)e[b].value : 1ull;
      if (up[b]) {
        weight += w;
        if (la[b] == lb[b]) inside += w;
      }
      lp_tot_add(up[b], la[b], w, tot, lane);
      lp_tot_add(up[b], lb[b], w, tot, lane);
    }
  });
  const int lane = wv::lane();
  lp_count(stripes, kLpCntInside, lp_wave_sum64(inside, lane), red[0]);
  lp_count(stripes, kLpCntWeight, lp_wave_sum64(weight, lane), red[1]);
}
// part[2 * block] / part[2 * block + 1] = low / high word of this workgroup's share of the sum of tot_c^2
PMA_KERNEL void k_lp_mod_squares(const unsigned long long *__restrict__ tot, uint32_t n, unsigned long long *part) {
  PMA_SHARED unsigned long long red_lo[4], red_hi[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  unsigned long long lo = 0, hi = 0;
  for (uint64_t c = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); c < n; c += stride) {
    const unsigned long long t = tot[c], pl = t * t;
    lo += pl;
    hi += wv::mulhi64(t, t) + (lo < pl ? 1ull : 0ull);
  }
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long ol = cp_shfl(lo, lane ^ d), oh = cp_shfl(hi, lane ^ d);
    lo += ol;
    hi += oh + (lo < ol ? 1ull : 0ull);
  }
  if (lane == 0) {
    red_lo[wv::wave_in_block()] = lo;
    red_hi[wv::wave_in_block()] = hi;
  }
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    for (uint32_t q = 1; q < (wv::block_dim() >> 6); q++) {
      lo += red_lo[q];
      hi += red_hi[q] + (lo < red_lo[q] ? 1ull : 0ull);
    }
    part[2ull * wv::block_idx()] = lo;
    part[2ull * wv::block_idx() + 1] = hi;
  }
}

}  // namespace ppcsr
