// Minimum spanning forest over the table of gapped arrays (pma_consumer.h): Boruvka's algorithm in streaming passes over the
// arrays in place — no export, no transposed graph, no sort of the edges (Boruvka 1926; the GPU formulations of Vineet et al.,
// HPG'09, and of Nobari et al., PPoPP'12: PAPERS.md).  The edge set is the one k_cc_hook walks — the live edges of cp_load_chunks,
// self-loops dropped — each stored pair (a, b) with value w an UNDIRECTED edge {a, b} of weight w; (a, b) and (b, a) stored both
// are two parallel edges.
//
// The order.  The key of an edge is (w, lo, hi), lo = min(a, b), hi = max(a, b), compared lexicographically; two edges with one
// key are the two directions of a pair stored with equal values and count as one.  Under a strict order the minimum spanning
// forest is unique as a set of keys, and Boruvka's step is safe: the smallest key leaving a component (its lightest CUT edge)
// belongs to that forest.
//
// One round, with comp[v] = the root of v's current tree, FIXED during steps 1 - 3 (the hooks of step 3 go to par[], which equals
// comp[] when the round begins):
//   1. best_w[c]    = the smallest weight over the cut edges of c               (streaming pass, atomic min, 32 bits)
//   2. best_pair[c] = the smallest lo << 32 | hi over the cut edges of c with that weight   (streaming pass, atomic min, 64 bits)
//      (best_w[c], best_pair[c]) is the chosen key of c; no slot address is kept, so the two directions of a pair need no care.
//   3. hook: every root c with a chosen key sets par[c] = o, the component at the other end, and emits the edge — unless o
//      chose the SAME key and c < o: then c stays the root of the two.
//   4. jump: par[v] = par[par[v]] in place until a launch changes nothing: par[v] is a root for every v.
//   5. comp = par, best_w / best_pair cleared.
// The rounds end when step 1 counts no cut edge.
//
// Invariants.
//   (a) comp only ever merges: a hook joins two trees and nothing splits one, so the vertex sets of the trees are unions of the
//       sets of the round before, and every emitted edge joins two of them.
//   (b) No cycle beyond the mutual pair.  Every component compares the same keys the same way.  Follow the hooks c1 -> c2 -> ...:
//       ci's chosen key k(ci) is a cut edge of c(i+1) too, so k(c(i+1)) <= k(ci): the keys never rise along a chain, and on a
//       cycle they are all EQUAL.  One key is one pair {lo, hi} and touches two components: the cycle is c <-> o with one shared
//       key, the one case step 3 breaks by id.  So the hooks of a round form a forest whose roots are the components without a
//       cut edge and the smaller ids of the mutual pairs, every component with a cut edge hooks or is the kept end of a mutual
//       pair — at least halving their number: at most floor(log2 n) + 1 rounds, the last one finding nothing — and every hook
//       emits exactly one edge, no edge twice: the two ends of a shared key are the mutual pair, of which one emits.
//   (c) Stale reads.  The passes look at best_w / best_pair before they issue an atomic and skip it when their value is not
//       below.  These words only fall during a pass, so a stale look is only too LARGE: it can cost an atomic that lowers
//       nothing, never lose a minimum — the atomic decides.  (After a round or two nearly every cut edge touches the giant
//       component: without the look, 10^7 atomics on one word would be served one after the other.  The look is a plain load:
//       reading it at the L2 instead, past the compute unit's cache, was measured and is slower — DESIGN 4i.)  Step 2 reads best_w[] as
//       step 1 left it: a launch boundary lies between.  In step 4 a thread may read par[p] while thread p stores to it: it sees
//       the old or the new value, both ancestors of p, the new one further up — in-place values are always at least as far up
//       as those of a synchronous doubling, so a chain of depth d needs at most ceil(log2 d) + 1 launches, the last one the
//       launch that changes nothing.  No thread chases to the root (as k_cc_jump does, which leans on labels[x] <= x and short
//       chains): an ascending-weight path hooks into ONE chain of n - 1 links in a single round.
#pragma once
#include "pma_consumer.h"
#include "pma_paths.h"

namespace ppcsr {

// the call's striped counters: 64-bit, one 128-byte line per stripe; never cleared during a call — the host takes differences
constexpr uint32_t kMsfStripeWords = 16;
constexpr uint32_t kMsfCntWork = 0;    // word 0: cut edges (step 1) and pointers moved (step 4)
constexpr uint32_t kMsfCntHooks = 1;   // word 1: hooks
constexpr uint32_t kMsfCntWeight = 2;  // word 2: the sum of the emitted weights
constexpr unsigned long long kMsfNoPair = 0xFFFFFFFFFFFFFFFFull;

PMA_DEV void msf_atomic_min(uint32_t *p, uint32_t v) { wv::atomic_min_u32(p, v); }
PMA_DEV void msf_atomic_min(unsigned long long *p, unsigned long long v) { wv::atomic_min_u64(p, v); }
PMA_DEV unsigned long long msf_reduce_add(unsigned long long v, int lane) {
  for (int d = 1; d < 64; d <<= 1) v += cp_shfl(v, lane ^ d);
  return v;
}

// The lanes with `want` lower best[c] to at most v (called by the whole wave).  A hub's run — or, from the second round on, the
// giant component — fills whole waves with one target: runs of kCcRunLanes lanes or more are reduced to their minimum and one
// lane issues it (cp_combine_runs).
template <class T>
PMA_DEV void msf_lower(bool want, uint32_t c, T v, T *best, int lane) {
  if (cp_combine_runs<kCcRunLanes>(want, c, v, (T) ~(T)0, lane, [](T m, int l) { return cp_wave_min(m, l); })) msf_atomic_min(&best[c], v);
}

// ---- steps 1 and 2: the two streaming passes -------------------------------------------------------------------------------------
// kPair false: step 1, both ends of every cut edge lower best_w[] of their component to the edge's weight (an edge may be stored
// in one direction only, so the source's side alone would miss the destination's lightest edge); `cnt` counts the cut edges.
// kPair true: step 2, both ends of every cut edge whose weight IS their component's best lower best_pair[] to lo << 32 | hi.
template <bool kPair>
PMA_DEV void msf_pass(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ comp, uint32_t *best_w,
                      unsigned long long *best_pair, unsigned long long *cnt, unsigned long long *red) {
  uint32_t mine = 0;
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&cut)[kB], int lane) {
    uint32_t cu[kB], cd[kB], bu[kB], bd[kB];
#pragma unroll
    for (int b = 0; b < kB; b++) cut[b] = cut[b] && src[b] != e[b].dest;
#pragma unroll
    for (int b = 0; b < kB; b++) {
      cu[b] = cut[b] ? comp[src[b]] : 0u;
      cd[b] = cut[b] ? comp[e[b].dest] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      cut[b] = cu[b] != cd[b];
      bu[b] = cut[b] ? best_w[cu[b]] : 0u;  // (step 1: a look that may be stale, that is: too large; step 2: final values)
      bd[b] = cut[b] ? best_w[cd[b]] : 0u;
    }
    if (!kPair) {
#pragma unroll
      for (int b = 0; b < kB; b++) {
        const uint32_t w = e[b].value;
        msf_lower<uint32_t>(cut[b] && w < bu[b], cu[b], w, best_w, lane);
        msf_lower<uint32_t>(cut[b] && w < bd[b], cd[b], w, best_w, lane);
        if (cut[b]) mine++;
      }
    } else {
      unsigned long long pu[kB], pd[kB];
      bool hu[kB], hd[kB];
#pragma unroll
      for (int b = 0; b < kB; b++) {
        hu[b] = cut[b] && e[b].value == bu[b];
        hd[b] = cut[b] && e[b].value == bd[b];
        pu[b] = hu[b] ? best_pair[cu[b]] : 0ull;
        pd[b] = hd[b] ? best_pair[cd[b]] : 0ull;
      }
#pragma unroll
      for (int b = 0; b < kB; b++) {
        const uint32_t lo = src[b] < e[b].dest ? src[b] : e[b].dest, hi = src[b] < e[b].dest ? e[b].dest : src[b];
        const unsigned long long pair = ((unsigned long long)lo << 32) | hi;
        msf_lower<unsigned long long>(hu[b] && pair < pu[b], cu[b], pair, best_pair, lane);
        msf_lower<unsigned long long>(hd[b] && pair < pd[b], cd[b], pair, best_pair, lane);
      }
    }
  });
  if (!kPair) cp_striped_add<unsigned long long, kMsfStripeWords>(cnt + kMsfCntWork, (unsigned long long)wv::reduce_add(mine), red);
}
PMA_KERNEL void k_msf_weight(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ comp, uint32_t *best_w,
                             unsigned long long *cnt) {
  PMA_SHARED unsigned long long red[4];
  msf_pass<false>(tab, P, n, comp, best_w, nullptr, cnt, red);
}
PMA_KERNEL void k_msf_pair(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ comp, uint32_t *best_w,
                           unsigned long long *best_pair) {
  msf_pass<true>(tab, P, n, comp, best_w, best_pair, nullptr, nullptr);
}

// ---- step 3: hook -----------------------------------------------------------------------------------------------------------------
// cp_append with a key and a weight per entry — never beyond the list's `cap` entries (a forest has fewer than n edges; the host
// compares the length with its hook counts)
PMA_DEV void msf_append(bool in, unsigned long long key, uint32_t w, unsigned long long *keys, uint32_t *wts, uint32_t *count, uint32_t cap,
                        int lane) {
  const uint32_t at = cp_append_at(in, count, lane);
  if (in && at < cap) {
    keys[at] = key;
    wts[at] = w;
  }
}
// One thread per vertex, one wave per 64 consecutive vertices; a root with a chosen key hooks (header: step 3).  comp[], best_w[]
// and best_pair[] are read only; the stores go to par[c] of the hooking roots, which no thread of this launch reads.  The list
// has room for n - 1 entries: a forest has no more edges.
PMA_KERNEL void k_msf_hook(const uint32_t *__restrict__ comp, uint32_t *par, const uint32_t *__restrict__ best_w,
                           const unsigned long long *__restrict__ best_pair, uint32_t n, unsigned long long *keys, uint32_t *wts, uint32_t *count,
                           unsigned long long *cnt) {
  PMA_SHARED unsigned long long red_h[4];
  PMA_SHARED unsigned long long red_w[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t hooks = 0;
  unsigned long long sum = 0;
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t c = base + (uint64_t)lane;
    bool hook = false;
    uint32_t w = kMax;
    unsigned long long pair = kMsfNoPair;
    if (c < n && comp[c] == (uint32_t)c) {
      w = best_w[c];
      if (w != kMax) pair = best_pair[c];
    }
    const uint32_t lo = (uint32_t)(pair >> 32), hi = (uint32_t)pair;
    if (w != kMax && lo < n && hi < n) {  // (a chosen weight always has its pair: step 2 saw the edge step 1 saw)
      const uint32_t a = comp[lo], b = comp[hi];
      const uint32_t o = a == (uint32_t)c ? b : a;
      const bool mutual = best_w[o] == w && best_pair[o] == pair;
      if (o != (uint32_t)c && !(mutual && (uint32_t)c < o)) {
        par[c] = o;
        hook = true;
        hooks++;
        sum += w;
      }
    }
    msf_append(hook, pair, w, keys, wts, count, n, lane);
  }
  cp_striped_add<unsigned long long, kMsfStripeWords>(cnt + kMsfCntHooks, (unsigned long long)wv::reduce_add(hooks), red_h);
  cp_striped_add<unsigned long long, kMsfStripeWords>(cnt + kMsfCntWeight, msf_reduce_add(sum, lane), red_w);
}

// ---- step 4: jump -----------------------------------------------------------------------------------------------------------------
// one pointer doubling in place; `cnt` counts the pointers moved (header: (c))
PMA_KERNEL void k_msf_jump(uint32_t *par, uint32_t n, unsigned long long *cnt) {
  PMA_SHARED unsigned long long red[4];
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t mine = 0;
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    const uint32_t p = par[v];
    const uint32_t g = par[p];
    if (g != p) {
      par[v] = g;
      mine++;
    }
  }
  cp_striped_add<unsigned long long, kMsfStripeWords>(cnt + kMsfCntWork, (unsigned long long)wv::reduce_add(mine), red);
}

// ---- step 5, and the start ----------------------------------------------------------------------------------------------------
PMA_KERNEL void k_msf_reset(uint32_t *comp, const uint32_t *__restrict__ par, uint32_t *best_w, unsigned long long *best_pair, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) {
    comp[v] = par[v];
    best_w[v] = kMax;
    best_pair[v] = kMsfNoPair;
  }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
// labels[v] = the smallest id under v's root, the convention of k_cc_hook's fixpoint: smallest[c] (all kMax: the cleared
// best_w[]) takes the minimum over the tree of root c, then every vertex reads its root's.  One wave per 64 consecutive vertices.
PMA_KERNEL void k_msf_label_min(const uint32_t *__restrict__ comp, uint32_t *smallest, uint32_t n) {
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < n; base += stride) {
    const uint64_t v = base + (uint64_t)lane;
    const uint32_t c = v < n ? comp[v] : 0u;
    msf_lower<uint32_t>(v < n && (uint32_t)v < smallest[c], c, (uint32_t)v, smallest, lane);
  }
}
PMA_KERNEL void k_msf_label_assign(const uint32_t *__restrict__ comp, const uint32_t *__restrict__ smallest, uint32_t *labels, uint32_t n) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t v = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); v < n; v += stride) labels[v] = smallest[comp[v]];
}
// the sorted list as (src = lo, dest = hi, value = w)
PMA_KERNEL void k_msf_pack(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ wts, uint64_t m, Edge *out) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < m; i += stride) {
    Edge e;
    e.src = (uint32_t)(keys[i] >> 32);
    e.dest = (uint32_t)keys[i];
    e.value = wts[i];
    out[i] = e;
  }
}

}  // namespace ppcsr
