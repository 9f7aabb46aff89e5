// Consumers that intersect two neighbourhoods: triangle counts and common-neighbour counts over the table of gapped arrays
// (pma_consumer.h).  The edge set is the one the BFS kernels walk: live non-sentinel slots of (beginning, end), slot N-1
// excluded, local src < n_p, global dests < n.
//
// A vertex's live slots are kept in ascending dest order (the update path's search depends on it), so two neighbourhoods are
// intersected where they lie: no CSR export, no sort.  The ranges are gapped — a slot is read, found null and skipped — and
// every routine here takes slot ranges [lo, hi), never element counts.  Three ways to intersect, chosen by slot lengths:
//   isect_lane    both ranges of at most kIsectLaneSlots slots: ONE LANE walks the two ranges with two cursors, so a wave
//                 has 64 pairs in flight (most pairs of an RMAT graph are of this kind)
//   isect_wave    one wave per pair.  The shorter range is loaded 64 slots per step; comparable lengths: the step's dests
//                 are staged in LDS and the longer range is streamed past them from a cursor that only moves forward (a
//                 merge, 64 slots at a time on either side); lopsided lengths (longer > kIsectLopsided x shorter): every
//                 lane searches the longer range for its own dest (isect_probe: a gap-aware binary search)
//   isect_block   a range beyond kBfsWaveSlots: one workgroup per pair, the shorter range staged in LDS kIsectTile slots at
//                 a time, the part of the longer range that can meet the tile found by two searches and then streamed by
//                 all waves (or probed, when it is lopsided the other way)
// The vertex ranges must be sorted and disjoint: the host side refuses the sequential regime (narrow == 0).
#pragma once
#include "pma_consumer.h"

namespace ppcsr {

constexpr uint32_t kIsectNone = 0xFFFFFFFFu;  // LDS tile entry without an element (never a dest below n)
constexpr uint32_t kIsectLaneSlots = 32;      // both ranges at most this long: one lane intersects them
constexpr uint32_t kIsectLopsided = 8;        // longer / shorter above this: probe instead of merging
constexpr uint32_t kIsectTile = 1024;         // slots of the shorter range a workgroup stages at a time (4 KB of LDS)
constexpr uint32_t kTriStripeWords = 16;      // the total: kBfsStripes 64-bit counters on 128-byte lines of their own

// first slot p of [lo, hi] such that every live slot of [lo, p) holds a dest < key (wave-uniform; lo <= hi).  64 samples per
// step narrow the bracket; samples that fall on nulls say nothing, so a step that does not halve the bracket hands over to
// a walk over whole 64-slot chunks.
PMA_DEV uint32_t isect_lower_bound(const Edge *__restrict__ items, uint32_t lo, uint32_t hi, uint32_t key) {
  const int lane = wv::lane();
  while (hi - lo > 64u) {
    const uint32_t len = hi - lo;
    const uint32_t step = (len + 63u) / 64u;
    const uint32_t s = lo + (uint32_t)lane * step;
    uint32_t val = 0, d = 0;
    if (s < hi) {
      val = items[s].value;
      d = items[s].dest;
    }
    const uint64_t mlt = wv::ballot(val != 0 && d < key), mge = wv::ballot(val != 0 && d >= key);
    const uint32_t nlo = mlt ? lo + (uint32_t)(63 - wv::clz64(mlt)) * step + 1u : lo;
    const uint32_t nhi = mge ? lo + (uint32_t)wv::ctz64(mge) * step : hi;
    lo = nlo;
    hi = nhi;
    if (hi < lo) hi = lo;  // (never, for a sorted range)
    if (hi - lo > len / 2u) break;
  }
  for (; lo < hi; lo += 64u) {
    const uint32_t s = lo + (uint32_t)lane;
    uint32_t val = 0, d = 0;
    if (s < hi) {
      val = items[s].value;
      d = items[s].dest;
    }
    const uint64_t mge = wv::ballot(val != 0 && d >= key);
    if (mge) return lo + (uint32_t)wv::ctz64(mge);
  }
  return hi;
}

// the live slot of [lo, hi) that holds dest == key, kMax when there is none.  One lane's own search (every lane of a wave runs
// one, each for its key): a binary search whose probe, landing on a null, walks right to the next live slot.
PMA_DEV uint32_t isect_probe_slot(const Edge *__restrict__ items, uint32_t lo, uint32_t hi, uint32_t key) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t p = mid, d = 0;
    bool live = false;
    for (; p < hi; p++)
      if (items[p].value != 0) {
        d = items[p].dest;
        live = true;
        break;
      }
    if (!live || d > key) hi = mid;
    else if (d == key) return p;
    else lo = p + 1u;
  }
  return kMax;
}
// does a live slot of [lo, hi) hold dest == key?
PMA_DEV bool isect_probe(const Edge *__restrict__ items, uint32_t lo, uint32_t hi, uint32_t key) {
  return isect_probe_slot(items, lo, hi, key) != kMax;
}
// the same over a staged tile: tile[i] = dest, or kIsectNone where the slot held nothing that counts
PMA_DEV bool isect_probe_tile(const uint32_t *tile, uint32_t cnt, uint32_t key) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t p = mid, d = kIsectNone;
    for (; p < hi; p++) {
      d = tile[p];
      if (d != kIsectNone) break;
    }
    if (d == kIsectNone || d > key) hi = mid;
    else if (d == key) return true;
    else lo = p + 1u;
  }
  return false;
}

// |{c : from <= c < n} in both ranges|, one lane: two cursors over the gapped ranges.  tri != nullptr: every c is credited.
PMA_DEV uint32_t isect_lane(const Edge *__restrict__ ia, uint32_t i, uint32_t ahi, const Edge *__restrict__ ib, uint32_t j, uint32_t bhi, uint32_t from,
                            uint32_t n, unsigned long long *tri) {
  uint32_t cnt = 0, da = 0, db = 0;
  bool ha = false, hb = false;
  for (;;) {
    for (; !ha && i < ahi; i++)
      if (ia[i].value != 0) {
        da = ia[i].dest;
        ha = true;
      }
    for (; !hb && j < bhi; j++)
      if (ib[j].value != 0) {
        db = ib[j].dest;
        hb = true;
      }
    if (!ha || !hb || da >= n || db >= n) break;  // (sorted: what follows a dest >= n is >= n as well)
    if (da == db) {
      if (da >= from) {
        cnt++;
        if (tri) wv::atomic_add_u64(&tri[da], 1ull);
      }
      ha = hb = false;
    } else if (da < db) {
      ha = false;
    } else {
      hb = false;
    }
  }
  return cnt;
}

// The same for one wave (all arguments wave-uniform, the result too).  tile: 64 words of LDS of this wave's own.
PMA_DEV uint32_t isect_wave(const Edge *__restrict__ ia, uint32_t alo, uint32_t ahi, const Edge *__restrict__ ib, uint32_t blo, uint32_t bhi,
                            uint32_t from, uint32_t n, uint32_t *tile, unsigned long long *tri) {
  const int lane = wv::lane();
  if (bhi - blo < ahi - alo) {  // a: the shorter range
    const Edge *t = ia;
    ia = ib;
    ib = t;
    uint32_t x = alo;
    alo = blo;
    blo = x;
    x = ahi;
    ahi = bhi;
    bhi = x;
  }
  if (ahi == alo) return 0;
  const bool probe = (bhi - blo) / kIsectLopsided > ahi - alo;
  uint32_t cur = blo, mine = 0;
  for (uint32_t base = alo; base < ahi; base += 64u) {
    const uint32_t s = base + (uint32_t)lane;
    uint32_t val = 0, d = 0;
    if (s < ahi) {
      val = ia[s].value;
      d = ia[s].dest;
    }
    const bool live = val != 0 && d >= from && d < n;  // (a sentinel's dest is 0xFFFFFFFF: never below n)
    const uint64_t m = wv::ballot(live);
    if (m == 0) continue;
    if (probe) {
      if (live && isect_probe(ib, blo, bhi, d)) {
        mine++;
        if (tri) wv::atomic_add_u64(&tri[d], 1ull);
      }
      continue;
    }
    tile[lane] = live ? d : kIsectNone;
    wv::lds_fence();
    const uint32_t tmin = wv::bcast(d, wv::ctz64(m)), tmax = wv::bcast(d, 63 - wv::clz64(m));
    // the longer range from the cursor: a chunk whose last dest reaches the tile's last one may hold dests of the next
    // tile too and stays under the cursor (its dests up to tmax cannot match there again: the next tile lies above tmax)
    while (cur < bhi) {
      const uint32_t q = cur + (uint32_t)lane;
      uint32_t v2 = 0, d2 = 0;
      if (q < bhi) {
        v2 = ib[q].value;
        d2 = ib[q].dest;
      }
      if (v2 != 0 && d2 >= tmin && d2 <= tmax && isect_probe_tile(tile, 64u, d2)) {
        mine++;
        if (tri) wv::atomic_add_u64(&tri[d2], 1ull);
      }
      const uint64_t m2 = wv::ballot(v2 != 0);
      if (m2 != 0 && wv::bcast(d2, 63 - wv::clz64(m2)) >= tmax) break;
      cur += 64u;
    }
    wv::lds_fence();  // (the tile is rewritten by the next step)
  }
  return wv::reduce_add(mine);
}

// The same for one workgroup of 256 threads (all arguments the same in every thread); returns THIS WAVE's share of the
// count.  tile: kIsectTile words of LDS, mm: 2 words.
PMA_DEV uint32_t isect_block(const Edge *__restrict__ ia, uint32_t alo, uint32_t ahi, const Edge *__restrict__ ib, uint32_t blo, uint32_t bhi,
                             uint32_t from, uint32_t n, uint32_t *tile, uint32_t *mm, unsigned long long *tri) {
  const uint32_t t = wv::thread_idx(), nt = wv::block_dim();
  if (bhi - blo < ahi - alo) {  // a: the shorter range
    const Edge *x = ia;
    ia = ib;
    ib = x;
    uint32_t y = alo;
    alo = blo;
    blo = y;
    y = ahi;
    ahi = bhi;
    bhi = y;
  }
  uint32_t mine = 0;
  for (uint32_t base = alo; base < ahi; base += kIsectTile) {
    const uint32_t tl = ahi - base < kIsectTile ? ahi - base : kIsectTile;
    for (uint32_t i = t; i < tl; i += nt) {
      const uint32_t val = ia[base + i].value, d = ia[base + i].dest;
      tile[i] = (val != 0 && d >= from && d < n) ? d : kIsectNone;
    }
    wv::block_sync();
    if (t == 0) {  // the tile's first and last dest (gaps are short: a few reads each)
      uint32_t f = 0, l = tl;
      while (f < tl && tile[f] == kIsectNone) f++;
      while (l > f && tile[l - 1u] == kIsectNone) l--;
      mm[0] = f < tl ? tile[f] : kIsectNone;
      mm[1] = f < tl ? tile[l - 1u] : kIsectNone;
    }
    wv::block_sync();
    const uint32_t tmin = mm[0], tmax = mm[1];
    if (tmin != kIsectNone) {
      // the slots of the longer range that can meet this tile (every wave finds the same two slots)
      const uint32_t p = isect_lower_bound(ib, blo, bhi, tmin);
      const uint32_t q = isect_lower_bound(ib, p, bhi, tmax + 1u);
      if ((q - p) / kIsectLopsided > tl) {
        for (uint32_t i = t; i < tl; i += nt) {
          const uint32_t c = tile[i];
          if (c != kIsectNone && isect_probe(ib, p, q, c)) {
            mine++;
            if (tri) wv::atomic_add_u64(&tri[c], 1ull);
          }
        }
      } else {
        for (uint32_t x = p + t; x < q; x += nt) {
          const uint32_t val = ib[x].value, d = ib[x].dest;
          if (val != 0 && d >= tmin && d <= tmax && isect_probe_tile(tile, tl, d)) {
            mine++;
            if (tri) wv::atomic_add_u64(&tri[d], 1ull);
          }
        }
      }
      blo = q;  // (the next tile lies above tmax)
    }
    wv::block_sync();  // (the tile and mm are rewritten by the next step)
  }
  return wv::reduce_add(mine);
}

// ---- triangles ---------------------------------------------------------------------------------------------------------------
// Upper orientation: the unit of work is a stored edge (a, b) with a < b < n, found by streaming the concatenated chunk space
// like k_cc_hook; its count is |{c > b} in N(a) and in N(b)|.  Both operands are slot suffixes: of a's range, what lies
// behind the slot of b itself; of b's range, what lies behind the first dest above b (isect_lower_bound).
struct TriItem {
  const Edge *items;  // the array of the chunk (wave-uniform)
  uint32_t s;         // the edge's slot
  uint32_t a, b;      // global ids
  uint32_t aend;      // end of a's range
  uint32_t kb, bbeg, bend;  // b's array and range
  bool item, lng;     // a counted edge; one of its operand ranges is beyond kBfsWaveSlots
};
// the edge in slot `lane` of chunk ch, its two node records loaded by the lane itself
PMA_DEV TriItem tri_item(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint64_t ch, int lane) {
  TriItem it;
  const uint32_t k = P > 1 ? cp_chunk_owner(tab, P, ch) : 0u;
  it.items = tab[k].items;
  const uint64_t s = (ch - tab[k].chunk0) * 64 + (uint64_t)lane;
  it.s = (uint32_t)s;
  Edge e = null_edge();
  if (s + 1 < tab[k].N) e = it.items[s];  // (slot N-1 is never part of a neighbourhood)
  it.a = e.src + tab[k].first;
  it.b = e.dest;
  it.item = e.value != 0 && !is_sentinel(e) && e.src < tab[k].n && it.a < it.b && it.b < n;
  it.aend = it.kb = it.bbeg = it.bend = 0;
  it.lng = false;
  if (it.item) {
    it.aend = tab[k].nodes[e.src].end;
    if (it.aend <= it.s) it.aend = it.s + 1u;
    it.kb = P > 1 ? cp_owner(tab, P, it.b) : 0u;
    const Node nb = tab[it.kb].nodes[it.b - tab[it.kb].first];
    it.bbeg = nb.beginning + 1u;
    it.bend = nb.end > it.bbeg ? nb.end : it.bbeg;
    it.lng = it.aend - it.s > kBfsWaveSlots || it.bend - it.bbeg > kBfsWaveSlots;
  }
  return it;
}
// credits of one chunk's edges to their sources and to themselves.  Lanes on one source share the target (a vertex's slots
// are contiguous, see k_cc_hook): each run of equal sources is summed in the wave and one lane issues it.
PMA_DEV void tri_credit(unsigned long long *tri, uint32_t a, uint32_t b, uint32_t cnt) {
  const int lane = wv::lane();
  if (cnt) wv::atomic_add_u64(&tri[b], (unsigned long long)cnt);
  for (uint64_t m = wv::ballot(cnt != 0); m != 0;) {
    const uint32_t key = wv::bcast(a, wv::ctz64(m));
    const bool in = cnt != 0 && a == key;
    const uint32_t sum = wv::reduce_add(in ? cnt : 0u);
    if (lane == 0) wv::atomic_add_u64(&tri[key], (unsigned long long)sum);
    m &= ~wv::ballot(in);
  }
}
// One 64-slot chunk per wave at a time.  Edges with two short ranges: one per lane, all at once; the others one after the
// other on the whole wave; those with a range beyond kBfsWaveSlots are left to k_tri_long (their chunk goes on a list).
// tri may be null (only the total is wanted).  dlist / dcount: the listed chunks (room for every chunk) and their number.
PMA_KERNEL void k_tri_edges(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, unsigned long long *tri, unsigned long long *total,
                            uint32_t *dlist, uint32_t *dcount) {
  PMA_SHARED uint32_t tiles[4][64];
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane(), w = wv::wave_in_block();
  const uint64_t nchunks = tab[P].chunk0;
  const uint64_t wstride = cp_waves();
  unsigned long long mine = 0;  // (wave-uniform)
  for (uint64_t ch = wv::uni(cp_wave()); ch < nchunks; ch += wstride) {
    const TriItem it = tri_item(tab, P, n, ch, lane);
    if (wv::ballot(it.item) == 0) continue;
    if (wv::ballot(it.lng) != 0 && lane == 0) dlist[wv::atomic_add_u32(dcount, 1u)] = (uint32_t)ch;
    const bool small = it.item && !it.lng && it.aend - it.s <= kIsectLaneSlots && it.bend - it.bbeg <= kIsectLaneSlots;
    uint32_t cnt = 0;
    if (small) cnt = isect_lane(it.items, it.s + 1u, it.aend, tab[it.kb].items, it.bbeg, it.bend, it.b + 1u, n, tri);
    for (uint64_t m = wv::ballot(it.item && !it.lng && !small); m != 0; m &= m - 1) {
      const int j = wv::ctz64(m);
      const uint32_t bj = wv::bcast(it.b, j), bhi = wv::bcast(it.bend, j);
      const Edge *ib = tab[wv::bcast(it.kb, j)].items;
      const uint32_t blo = isect_lower_bound(ib, wv::bcast(it.bbeg, j), bhi, bj + 1u);
      const uint32_t c = isect_wave(it.items, wv::bcast(it.s, j) + 1u, wv::bcast(it.aend, j), ib, blo, bhi, bj + 1u, n, tiles[w], tri);
      if (lane == j) cnt = c;
    }
    if (tri) tri_credit(tri, it.a, it.b, cnt);
    mine += wv::reduce_add(cnt);
  }
  cp_striped_add<unsigned long long, kTriStripeWords>(total, mine, red);
}
// The listed chunks again, a quarter of a chunk (16 slots) per workgroup at a time: every edge with a long range is
// intersected by the whole workgroup, so a hub's edges spread over the chip and none of them is one wave's work.
PMA_KERNEL void k_tri_long(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, unsigned long long *tri, unsigned long long *total,
                           const uint32_t *__restrict__ dlist, uint32_t ndefer) {
  PMA_SHARED uint32_t tile[kIsectTile];
  PMA_SHARED uint32_t mm[2];
  PMA_SHARED unsigned long long red[4];
  const int lane = wv::lane();
  unsigned long long mine = 0;  // (this wave's share)
  for (uint64_t u = wv::block_idx(); u < (uint64_t)ndefer * 4; u += wv::grid_dim()) {
    const TriItem it = tri_item(tab, P, n, (uint64_t)dlist[u >> 2], lane);  // (every wave loads the chunk: the same in all four)
    uint32_t cnt = 0;
    for (uint64_t m = wv::ballot(it.item && it.lng) & (0xFFFFull << (16u * (uint32_t)(u & 3u))); m != 0; m &= m - 1) {
      const int j = wv::ctz64(m);
      const uint32_t bj = wv::bcast(it.b, j), bhi = wv::bcast(it.bend, j);
      const Edge *ib = tab[wv::bcast(it.kb, j)].items;
      const uint32_t blo = isect_lower_bound(ib, wv::bcast(it.bbeg, j), bhi, bj + 1u);
      const uint32_t c = isect_block(it.items, wv::bcast(it.s, j) + 1u, wv::bcast(it.aend, j), ib, blo, bhi, bj + 1u, n, tile, mm, tri);
      if (lane == j) cnt = c;
    }
    if (tri) tri_credit(tri, it.a, it.b, cnt);  // (each wave credits its share)
    mine += wv::reduce_add(cnt);
  }
  cp_striped_add<unsigned long long, kTriStripeWords>(total, mine, red);
}

// ---- common neighbours -------------------------------------------------------------------------------------------------------
// counts[i] = |{c < n} in N(a[i]) and in N(b[i])|: directed out-neighbourhoods, no orientation filter.  Persistent waves,
// 64 pairs per wave at a time: the pairs and their node records are loaded one per lane (as k_lookup_edges does); pairs of
// two short ranges are intersected by their lane, all at once, the others by the wave, one after the other.
PMA_KERNEL void k_common_neighbours(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ qa,
                                    const uint32_t *__restrict__ qb, uint64_t nq, uint32_t *__restrict__ out) {
  PMA_SHARED uint32_t tiles[4][64];
  const int lane = wv::lane(), w = wv::wave_in_block();
  const uint64_t wpb = wv::block_dim() >> 6;
  const uint64_t waves = (uint64_t)wv::grid_dim() * wpb;
  const uint64_t nblk = (nq + 63) / 64;
  for (uint64_t blk = wv::uni((uint64_t)wv::block_idx() * wpb + (uint64_t)w); blk < nblk; blk += waves) {
    const uint64_t i = blk * 64 + (uint64_t)lane;
    const bool valid = i < nq;
    uint32_t a = kMax, b = kMax;
    if (valid) {
      a = qa[i];
      b = qb[i];
    }
    const bool inr = valid && a < n && b < n;  // (a vertex >= n: no common neighbours, not an error)
    uint32_t ka = 0, kb = 0, alo = 0, ahi = 0, blo = 0, bhi = 0;
    if (inr) {
      ka = P > 1 ? cp_owner(tab, P, a) : 0u;
      kb = P > 1 ? cp_owner(tab, P, b) : 0u;
      const Node na = tab[ka].nodes[a - tab[ka].first], nb = tab[kb].nodes[b - tab[kb].first];
      alo = na.beginning + 1u;
      ahi = na.end > alo ? na.end : alo;
      blo = nb.beginning + 1u;
      bhi = nb.end > blo ? nb.end : blo;
    }
    const bool small = inr && ahi - alo <= kIsectLaneSlots && bhi - blo <= kIsectLaneSlots;
    uint32_t res = 0;
    if (small) res = isect_lane(tab[ka].items, alo, ahi, tab[kb].items, blo, bhi, 0u, n, nullptr);
    for (uint64_t m = wv::ballot(inr && !small); m != 0; m &= m - 1) {
      const int j = wv::ctz64(m);
      const uint32_t c = isect_wave(tab[wv::bcast(ka, j)].items, wv::bcast(alo, j), wv::bcast(ahi, j), tab[wv::bcast(kb, j)].items,
                                    wv::bcast(blo, j), wv::bcast(bhi, j), 0u, n, tiles[w], nullptr);
      if (lane == j) res = c;
    }
    if (valid) out[i] = res;
  }
}

}  // namespace ppcsr
