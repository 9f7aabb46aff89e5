// Edge support and truss numbers (k-truss decomposition) over the table of gapped arrays (pma_consumer.h).  The undirected graph G
// is the one k_tri_edges counts in and pma_cores.h peels, the upper orientation: {a, b}, a < b < n, is an edge exactly when the
// pair (a, b) is stored in a live slot (cp_load_chunks).  support(e) = triangles of G through e; truss(e) = the largest k such
// that e lies in a subgraph whose every edge is in at least k - 2 triangles inside it (Cohen 2008; the peel: Wang & Cheng 2012,
// in sub-rounds: PKT, Kabir & Madduri 2017 — PAPERS.md).
//
// An edge is NAMED BY ITS SLOT in the concatenated chunk space (chunk0 * 64 + local slot, a 32-bit id: the host refuses 2^32
// slots or more), and all per-edge state is arrays parallel to the slots: sup[], stamp[], tr[].  There is no edge numbering, no
// sort and no export of the forward lists: the other two edges of a triangle are found where they lie, by isect_probe_slot, the
// gap-aware binary search of pma_intersect.h with the slot handed back — which needs sorted, disjoint vertex ranges (the host
// refuses the sequential regime, as for triangles).  What the array does not index is a vertex's IN-neighbours (the reason
// pma_cores.h gives for exporting), and removing {u, v} destroys triangles whose third vertex lies below u: one list of
// (w, slot of (w, u)) per vertex u is exported — |E| entries, unsorted, offsets from k_tr_init's counts and the scan kernels of
// pma_cores.h.
//
// One routine finds the triangles of an edge e = {u, v} (tr_walk): it walks the full neighbourhood of the endpoint x with the
// fewer (range slots + in-neighbours), 64 positions per step — x's range in place (the slot is the position) and x's in-list (the
// slot is in the entry) — and every lane searches the edge {y, w} between the other endpoint y and its own w: in y's range
// when y < w, in w's range otherwise.  A chosen side beyond kTrWaveSlots positions is deferred to a second launch that splits
// it over waves (k_tr_support_long / k_tr_peel_long: the split of k_kc_peel_long).  The lanes of one walk hold distinct w, hence
// distinct edges {x, w} and {y, w}: no two lanes of a wave ever target one word here, and there is nothing for cp_combine_runs to
// combine (the 5000 decrements of a book's spine come from 5000 waves, as the decrements of a k-core hub do).
//
// Support: every edge counts its own triangles and stores sup[slot] — no atomics (a deferred edge's segments add theirs).  Each
// triangle is found three times.
//
// Peel, the levels and sub-rounds of pma_cores.h with edges for vertices.  stamp[e] is 0 for a slot that holds no edge of G,
// kTrLive for an edge no frontier has taken, and otherwise the number r (1, 2, ... over the whole call) of the sub-round whose
// frontier e is in.  During sub-round r: stamp == r — in the frontier; stamp < r — removed; stamp > r — live (kTrLive, or r + 1:
// appended for the NEXT sub-round, which the lanes still running r must not take for a frontier edge, and do not).  Level k has
// threshold s = k - 2 = the smallest sup among the live edges (k_tr_min; levels no edge has are never run); its first frontier is
// every live edge with sup <= s (k_tr_collect).  A frontier edge e visits its triangles (e, f, g) with f and g not removed: f and
// g outside the frontier are decremented; when f is in the frontier too, only the one of e and f with the smaller slot
// decrements g; with all three in the frontier nothing is left to decrement.  The decrement that returns s + 1 stamps its edge
// r + 1, sets tr = k and appends it (cp_append: one atomic per wave per step).  The plain looks before the atomic follow
// sssp_relax_edge's rule: sup only falls, a stale look is too large, the atomic decides; a stamp changes during a launch only
// from kTrLive to r + 1, both "live".
// Invariants, with L(k) = "level k has ended":
//  (1) sup[g] is decremented at most once per triangle (e, f, g): when the triangle's first edges enter a frontier, by exactly
//      one of them (the rule above), and never again, because those edges are removed afterwards.  So at most support(g) times
//      in all: it never wraps below zero.
//  (2) At L(k) every live edge has sup > s.  Those at or below s when the level starts are taken by the collect; one above s that
//      ends at or below it has passed through the decrement s + 1 -> s (decrements are by one), which stamped it.
//  (3) Every edge enters exactly one frontier, exactly once: the values sup[g] takes are strictly falling, so at most one
//      decrement of a level returns s + 1; an edge the collect took has sup <= s and is never decremented (the look refuses);
//      both stamps are final, and the collect of a later level only sees kTrLive.  The level rises while live edges remain.
//  (4) The level at which e enters is its truss number: the argument (4) of pma_cores.h with "triangles of e inside S" for
//      "neighbours of v inside S" — when level k starts, sup[e] of a live edge is its number of triangles among the live edges S,
//      all >= k - 2, so truss >= k on S; and the first edge of a (k + 1)-truss H to be stamped would have sup >= k - 1 > s
//      when stamped at a level <= k, which neither the collect nor the decrement s + 1 -> s allows.
// The frontier a sub-round appends is a function of the graph (g crosses s exactly when enough of its triangles have an edge in
// frontiers of this level), so levels, sub-rounds and frontier widths equal a synchronous host peel's.
#pragma once
#include "pma_cores.h"      // the scan kernels
#include "pma_intersect.h"  // isect_probe_slot

namespace ppcsr {

constexpr uint32_t kTrLive = kMax;   // stamp of an edge of G that no frontier has taken yet
constexpr uint32_t kTrStripeWords = 16;  // the triangle total: kBfsStripes 64-bit counters on 128-byte lines of their own
// counter block of the host loop, as kKcCntWords: [0] edges appended to the next frontier, [1] edges deferred to the long-range
// kernel, [2] the smallest sup among the live edges (kMax: none left)
constexpr uint32_t kTrCntWords = 8;
// Longest walk that is not deferred, and the segment a wave of the long-range kernels takes.  A position of this walk costs a
// binary search (a dozen dependent loads), not one atomic as a list entry of k_kc_peel does: with kBfsWaveSlots = 4096 positions
// to one wave a sub-round waited 400-700 us for its one longest walk (RMAT scale 18: k_tr_peel 134 us on average over 471
// sub-rounds).
constexpr uint64_t kTrWaveSlots = 1024, kTrSegSlots = 64;
constexpr uint32_t kTrTeamMax = 16;  // most waves that share one frontier edge's walk (k_tr_peel)

// a vertex's array, the global slot id of that array's slot 0, and its slot range [lo, hi)
struct TrRange {
  const Edge *items;
  uint32_t base, lo, hi;
};
PMA_DEV TrRange tr_range(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t a) {
  const uint32_t k = P > 1 ? cp_owner(tab, P, a) : 0u;
  const Node nd = tab[k].nodes[a - tab[k].first];
  TrRange r;
  r.items = tab[k].items;
  r.base = (uint32_t)(tab[k].chunk0 * 64);
  r.lo = nd.beginning + 1u;
  r.hi = nd.end;
  const uint32_t last = (uint32_t)(tab[k].N - 1);  // (slot N-1 is never part of a neighbourhood)
  if (r.hi > last) r.hi = last;
  if (r.hi < r.lo) r.hi = r.lo;
  return r;
}
// the edge in global slot g (wave-uniform): its ends, global ids
PMA_DEV void tr_edge_of(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t g, uint32_t &u, uint32_t &v) {
  const uint32_t k = P > 1 ? cp_chunk_owner(tab, P, (uint64_t)(g >> 6)) : 0u;
  const Edge e = tab[k].items[g - (uint32_t)(tab[k].chunk0 * 64)];
  u = wv::uni(e.src + tab[k].first);
  v = wv::uni(e.dest);
}

// The side of edge {u, v} that is walked (all wave-uniform): x, its range and in-list; the other end y and its range.  The walk's
// positions are [0, len): x's range slots first, then the entries of x's in-list.
struct TrSide {
  uint32_t x, y, rlen;
  uint64_t len, in0;
  TrRange xr, yr;
};
PMA_DEV TrSide tr_side(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t u, uint32_t v, const unsigned long long *__restrict__ inoff) {
  const TrRange ru = tr_range(tab, P, u), rv = tr_range(tab, P, v);
  const uint64_t iu = inoff[u], iv = inoff[v];
  const uint64_t lu = (uint64_t)(ru.hi - ru.lo) + (inoff[(uint64_t)u + 1] - iu), lv = (uint64_t)(rv.hi - rv.lo) + (inoff[(uint64_t)v + 1] - iv);
  TrSide sd;
  const bool wu = lu <= lv;
  sd.x = wu ? u : v;
  sd.y = wu ? v : u;
  sd.xr = wu ? ru : rv;
  sd.yr = wu ? rv : ru;
  // (u and v are the same in every lane, and so is everything loaded for them: scalars for the walk's loop and its searches)
  sd.xr.lo = wv::uni(sd.xr.lo);
  sd.xr.base = wv::uni(sd.xr.base);
  sd.yr.lo = wv::uni(sd.yr.lo);
  sd.yr.hi = wv::uni(sd.yr.hi);
  sd.yr.base = wv::uni(sd.yr.base);
  sd.len = wv::uni((uint64_t)(wu ? lu : lv));
  sd.in0 = wv::uni((uint64_t)(wu ? iu : iv));
  sd.rlen = wv::uni(sd.xr.hi - sd.xr.lo);
  return sd;
}
// global slot of the edge {y, w} of G, kMax when there is none: one lane's search, in the range of the smaller id for the larger
PMA_DEV uint32_t tr_find(const ConsumerPart *__restrict__ tab, uint32_t P, const TrSide &sd, uint32_t w) {
  TrRange r = sd.yr;
  uint32_t key = w;
  if (w < sd.y) {
    r = tr_range(tab, P, w);
    key = sd.y;
  }
  const uint32_t s = isect_probe_slot(r.items, r.lo, r.hi, key);
  return s == kMax ? kMax : r.base + s;
}
// Positions [i0, i1) of the walk of sd, 64 per step, by the whole wave: tri(f, g) is called by all lanes once per step with the
// global slots of {x, w} and {y, w} — g == kMax in a lane whose position holds no third vertex of a triangle.
template <class Tri>
PMA_DEV void tr_walk(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const TrSide &sd, uint64_t i0, uint64_t i1,
                     const uint32_t *__restrict__ inw, const uint32_t *__restrict__ ins, int lane, Tri tri) {
  for (uint64_t base = i0; base < i1; base += 64) {
    const uint64_t i = base + (uint64_t)lane;
    uint32_t w = kMax, f = kMax, g = kMax;
    if (i < i1) {
      if (i < sd.rlen) {
        const uint32_t s = sd.xr.lo + (uint32_t)i;
        const uint32_t val = sd.xr.items[s].value, d = sd.xr.items[s].dest;
        // (dests >= n and sentinels are not below n; a dest at or below x is a self-loop or a backward pair: no edge of G)
        if (val != 0 && val != kMax && d < n && d > sd.x && d != sd.y) {
          w = d;
          f = sd.xr.base + s;
        }
      } else {
        const uint64_t j = sd.in0 + (i - sd.rlen);
        if (inw[j] != sd.y) {
          w = inw[j];
          f = ins[j];
        }
      }
    }
    if (w != kMax) g = tr_find(tab, P, sd, w);
    tri(f, g);
  }
}
// The walk of a deferred edge split over the grid's waves in segments of kTrSegSlots positions (k_kc_peel_long's split): item i
// of list[0, *nlong_at) goes to a group of `per` waves, whose waves take every per-th segment: seg(g, sd, i0, i1).  The number of
// deferred edges is read from the device, where the launch before has left it: the host launches this kernel behind every
// k_tr_support / k_tr_peel without a round trip in between, and a launch that finds none ends at once.
template <class Seg>
PMA_DEV void tr_long(const ConsumerPart *__restrict__ tab, uint32_t P, const unsigned long long *__restrict__ inoff, const uint32_t *__restrict__ list,
                     const uint32_t *nlong_at, Seg seg) {
  const uint32_t nlong = wv::uni(*nlong_at);
  if (nlong == 0) return;
  const uint64_t waves = cp_waves();
  const uint64_t gw = wv::uni(cp_wave());
  const uint64_t per = waves / nlong ? waves / nlong : 1, groups = waves / per;
  if (gw >= groups * per) return;
  for (uint64_t i = gw / per; i < nlong; i += groups) {
    const uint32_t g = wv::uni(list[i]);
    uint32_t u, v;
    tr_edge_of(tab, P, g, u, v);
    const TrSide sd = tr_side(tab, P, u, v, inoff);
    for (uint64_t s = (gw % per) * kTrSegSlots; s < sd.len; s += per * kTrSegSlots) seg(g, sd, s, s + kTrSegSlots < sd.len ? s + kTrSegSlots : sd.len);
  }
}

// ---- stage 1: the edges of G by slot, the in-lists ------------------------------------------------------------------------------------
// one streaming pass, cp_stream's loop with the chunk index kept: stamp[] (kTrLive for an edge of G, 0 for every other slot),
// the in-degrees, and the number of edges of every chunk (scanned into the offsets of the output)
PMA_KERNEL void k_tr_init(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t *stamp, uint32_t *indeg, uint32_t *chunkcnt) {
  constexpr int kB = 4;
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  const Edge *const items0 = tab[0].items;
  const uint64_t N0 = tab[0].N;
  const uint32_t n0 = tab[0].n;
  for (uint64_t ch0 = wv::uni(cp_wave() * kB); ch0 < nchunks; ch0 += wstride * kB) {
    Edge e[kB];
    uint32_t a[kB];
    bool up[kB];
    cp_load_chunks<kB>(tab, P, n, items0, N0, n0, ch0, nchunks, lane, e, a, up);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (ch0 + b >= nchunks) break;
      up[b] = up[b] && a[b] < e[b].dest;
      stamp[(ch0 + b) * 64 + (uint64_t)lane] = up[b] ? kTrLive : 0u;
      if (up[b]) wv::atomic_add_u32(&indeg[e[b].dest], 1u);
      const uint64_t m = wv::ballot(up[b]);
      if (lane == 0) chunkcnt[ch0 + b] = (uint32_t)wv::popc64(m);
    }
  }
}
// in-list of every vertex b: (a, slot of (a, b)) per upper edge, in any order; fill[b]: entries written so far
PMA_KERNEL void k_tr_fill(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ inoff, uint32_t *fill,
                          uint32_t *inw, uint32_t *ins) {
  constexpr int kB = 4;
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  const Edge *const items0 = tab[0].items;
  const uint64_t N0 = tab[0].N;
  const uint32_t n0 = tab[0].n;
  for (uint64_t ch0 = wv::uni(cp_wave() * kB); ch0 < nchunks; ch0 += wstride * kB) {
    Edge e[kB];
    uint32_t a[kB];
    bool up[kB];
    cp_load_chunks<kB>(tab, P, n, items0, N0, n0, ch0, nchunks, lane, e, a, up);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (up[b] && a[b] < e[b].dest) {
        const uint64_t at = inoff[e[b].dest] + wv::atomic_add_u32(&fill[e[b].dest], 1u);
        inw[at] = a[b];
        ins[at] = (uint32_t)((ch0 + b) * 64 + (uint64_t)lane);
      }
    }
  }
}

// ---- support ---------------------------------------------------------------------------------------------------------------------------
// One 64-slot chunk per wave at a time, its edges one after the other on the whole wave; sup[] has been zeroed.  total: the
// striped sum of all supports (3 x the triangles).
PMA_KERNEL void k_tr_support(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ inoff,
                             const uint32_t *__restrict__ inw, const uint32_t *__restrict__ ins, const uint32_t *__restrict__ stamp, uint32_t *sup,
                             uint32_t *longl, uint32_t *cnt, unsigned long long *total) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  unsigned long long mine = 0;  // (wave-uniform)
  for (uint64_t ch = wv::uni(cp_wave()); ch < nchunks; ch += wstride) {
    const uint32_t g0 = (uint32_t)(ch * 64);
    for (uint64_t m = wv::ballot(stamp[g0 + (uint32_t)lane] != 0u); m != 0; m &= m - 1) {
      const uint32_t g = g0 + (uint32_t)wv::ctz64(m);
      uint32_t u, v;
      tr_edge_of(tab, P, g, u, v);
      const TrSide sd = tr_side(tab, P, u, v, inoff);
      if (sd.len > kTrWaveSlots) {
        if (lane == 0) longl[wv::atomic_add_u32(&cnt[1], 1u)] = g;
        continue;
      }
      uint32_t c = 0;
      tr_walk(tab, P, n, sd, 0, sd.len, inw, ins, lane, [&](uint32_t, uint32_t eg) { c += eg != kMax ? 1u : 0u; });
      c = wv::reduce_add(c);
      if (lane == 0) sup[g] = c;
      mine += c;
    }
  }
  cp_striped_add<unsigned long long, kTrStripeWords>(total, mine, red);
}
PMA_KERNEL void k_tr_support_long(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ inoff,
                                  const uint32_t *__restrict__ inw, const uint32_t *__restrict__ ins, const uint32_t *__restrict__ longl, const uint32_t *cnt,
                                  uint32_t *sup, unsigned long long *total) {
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  unsigned long long mine = 0;  // (wave-uniform)
  tr_long(tab, P, inoff, longl, cnt + 1, [&](uint32_t g, const TrSide &sd, uint64_t i0, uint64_t i1) {
    uint32_t c = 0;
    tr_walk(tab, P, n, sd, i0, i1, inw, ins, lane, [&](uint32_t, uint32_t eg) { c += eg != kMax ? 1u : 0u; });
    c = wv::reduce_add(c);
    if (lane == 0 && c) wv::atomic_add_u32(&sup[g], c);
    mine += c;
  });
  cp_striped_add<unsigned long long, kTrStripeWords>(total, mine, red);
}

// ---- peeling ---------------------------------------------------------------------------------------------------------------------------
// cnt[2] = the smallest sup among the live edges (preset to kMax): one atomic per workgroup
PMA_KERNEL void k_tr_min(const uint32_t *__restrict__ sup, const uint32_t *__restrict__ stamp, uint64_t slots, uint32_t *cnt) {
  PMA_SHARED uint32_t red[4];
  const int lane = wv::lane();
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  uint32_t m = kMax;
  for (uint64_t g = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); g < slots; g += stride)
    if (stamp[g] == kTrLive && sup[g] < m) m = sup[g];
  m = cp_wave_min(m, lane);
  if (lane == 0) red[wv::wave_in_block()] = m;
  wv::block_sync();
  if (wv::thread_idx() == 0) {
    for (uint32_t q = 1; q < (wv::block_dim() >> 6); q++) m = red[q] < m ? red[q] : m;
    if (m != kMax) wv::atomic_min_u32(&cnt[2], m);
  }
}
// first frontier of the level with threshold s = cnt[2] (written by the launch before): every live edge with sup <= s gets the
// stamp r of the sub-round about to run and truss s + 2, and is listed
PMA_KERNEL void k_tr_collect(const uint32_t *__restrict__ sup, uint32_t *stamp, uint32_t *tr, uint64_t slots, uint32_t r, uint32_t *front, uint32_t *cnt) {
  const int lane = wv::lane();
  const uint32_t s = cnt[2];
  if (s == kMax) return;
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < slots; base += stride) {
    const uint64_t g = base + (uint64_t)lane;
    const bool in = g < slots && stamp[g] == kTrLive && sup[g] <= s;
    if (in) {
      stamp[g] = r;
      tr[g] = s + 2u;
    }
    cp_append(in, (uint32_t)g, front, cnt, lane);
  }
}
// what the peel kernels pass along
struct TrPeel {
  uint32_t s, r;  // the level's threshold (the truss number is s + 2), the sub-round
  uint32_t *sup, *stamp, *tr, *next, *cnt;
};
// the lanes with `want` decrement sup[t]; the decrement that returns s + 1 moves t into the next frontier.  By the whole wave.
PMA_DEV void tr_dec(const TrPeel &pl, bool want, uint32_t t, int lane) {
  bool won = false;
  // (the look may be stale, that is: too large — the atomic decides, and is issued only for what looked above s)
  if (want && pl.sup[t] > pl.s) won = wv::atomic_add_u32(&pl.sup[t], 0xFFFFFFFFu) == pl.s + 1u;
  if (won) {
    pl.stamp[t] = pl.r + 1u;
    pl.tr[t] = pl.s + 2u;
  }
  cp_append(won, t, pl.next, pl.cnt, lane);
}
// one triangle (e, f, g) per lane of frontier edge e (g == kMax: none in this lane), by the whole wave
PMA_DEV void tr_peel_tri(const TrPeel &pl, uint32_t e, uint32_t f, uint32_t g, int lane) {
  bool df = false, dg = false;
  if (g != kMax) {
    const uint32_t sf = pl.stamp[f], sg = pl.stamp[g];
    if (sf >= pl.r && sg >= pl.r) {  // (neither removed)
      const bool ff = sf == pl.r, gf = sg == pl.r;
      df = !ff && (!gf || e < g);
      dg = !gf && (!ff || e < f);
    }
  }
  tr_dec(pl, df, f, lane);
  tr_dec(pl, dg, g, lane);
}
// One sub-round: a TEAM of `team` consecutive waves per frontier edge (1 .. kTrTeamMax; the host gives a small frontier large
// teams, so that the chip is filled and no wave walks far): the team's waves take every team-th step of 64 positions.  They share
// nothing but the edge — each works out the side for itself.  A walk beyond kTrWaveSlots positions is left to k_tr_peel_long
// (longl, cnt[1]).
PMA_KERNEL void k_tr_peel(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ inoff,
                          const uint32_t *__restrict__ inw, const uint32_t *__restrict__ ins, const uint32_t *__restrict__ front, uint32_t nfront, uint32_t team,
                          TrPeel pl, uint32_t *longl) {
  const int lane = wv::lane();
  const uint64_t gw = wv::uni(cp_wave()), teams = cp_waves() / team;
  const uint64_t mine = gw % team;
  if (gw >= teams * team) return;
  for (uint64_t i = gw / team; i < nfront; i += teams) {
    const uint32_t e = wv::uni(front[i]);
    uint32_t u, v;
    tr_edge_of(tab, P, e, u, v);
    const TrSide sd = tr_side(tab, P, u, v, inoff);
    if (sd.len > kTrWaveSlots) {
      if (mine == 0 && lane == 0) longl[wv::atomic_add_u32(&pl.cnt[1], 1u)] = e;
      continue;
    }
    for (uint64_t s = mine * 64; s < sd.len; s += (uint64_t)team * 64)
      tr_walk(tab, P, n, sd, s, s + 64 < sd.len ? s + 64 : sd.len, inw, ins, lane, [&](uint32_t f, uint32_t g) { tr_peel_tri(pl, e, f, g, lane); });
  }
}
PMA_KERNEL void k_tr_peel_long(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const unsigned long long *__restrict__ inoff,
                               const uint32_t *__restrict__ inw, const uint32_t *__restrict__ ins, const uint32_t *__restrict__ longl, TrPeel pl) {
  const int lane = wv::lane();
  tr_long(tab, P, inoff, longl, pl.cnt + 1, [&](uint32_t e, const TrSide &sd, uint64_t i0, uint64_t i1) {
    tr_walk(tab, P, n, sd, i0, i1, inw, ins, lane, [&](uint32_t f, uint32_t g) { tr_peel_tri(pl, e, f, g, lane); });
  });
}

// ---- output ----------------------------------------------------------------------------------------------------------------------------
// (a, b, val[slot]) of every edge of G in slot order: choff[ch] = edges in the chunks before ch.  out (may be null) takes the
// first cap of them; vmax (may be null): the largest value at every vertex — a hub's run of one source is combined in the wave
// (kc_source_runs gives the reason)
PMA_KERNEL void k_tr_emit(const ConsumerPart *__restrict__ tab, uint32_t P, const uint32_t *__restrict__ stamp, const uint32_t *__restrict__ val,
                          const unsigned long long *__restrict__ choff, Edge *out, uint64_t cap, uint32_t *vmax) {
  const int lane = wv::lane();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  for (uint64_t ch = wv::uni(cp_wave()); ch < nchunks; ch += wstride) {
    const uint32_t g = (uint32_t)(ch * 64) + (uint32_t)lane;
    const bool is = stamp[g] != 0u;
    const uint64_t m = wv::ballot(is);
    if (m == 0) continue;
    const uint32_t k = P > 1 ? cp_chunk_owner(tab, P, ch) : 0u;
    uint32_t a = 0, b = 0, x = 0;
    if (is) {
      const Edge e = tab[k].items[g - (uint32_t)(tab[k].chunk0 * 64)];
      a = e.src + tab[k].first;
      b = e.dest;
      x = val[g];
      const uint64_t at = choff[ch] + dev::lanemask_lt_count(m, lane);
      if (out && at < cap) out[at] = Edge{a, b, x};
    }
    if (vmax) {
      uint32_t inv = ~x;  // (the wave's minimum of the complements is the complement of the maximum)
      const bool issue = cp_combine_runs<kCcRunLanes>(is, a, inv, kMax, lane, [](uint32_t y, int l) { return cp_wave_min(y, l); });
      if (issue) wv::atomic_max_u32(&vmax[a], ~inv);
      if (is) wv::atomic_max_u32(&vmax[b], x);
    }
  }
}

}  // namespace ppcsr
