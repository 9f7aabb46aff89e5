// Batched reads: many edge_exists / get_neighbourhood questions per call (PCSR.cpp:860-869, 901-912), answered with the
// edge value beside the dest.  Nothing here writes the graph.
//   k_lookup_edges   persistent waves, 64 queries per wave at a time: the 64 (src, dst) pairs and the 64 node records are
//                    loaded lane-parallel (all dependent misses in flight together), then the wave runs the engine's own
//                    dev::pma_search for each query in turn — the same search, the same slot as k_edge_exists
//   gather           k_gather_rows (slot range + 64-slot chunk count per queried vertex) -> scan -> chunk -> row map
//                    (k_gather_mark + an inclusive max-scan) -> k_gather_count (live slots per chunk) -> scan ->
//                    k_gather_write (dests + values, CSR order) + k_gather_offsets.  Work is split by 64-slot chunks, so
//                    a hub's range spreads over every wave of the chip instead of one wave walking it.
//   k_xs_reduce / k_xs_scan   reduce-then-scan over tiles of kXsTile elements, one workgroup per tile (the tile sums are
//                    scanned by the same two kernels, recursively: no level is a single workgroup walking the whole input)
#pragma once
#include "pma_scan.h"

namespace ppcsr {

constexpr uint32_t kNoEdge = 0xFFFFFFFFu;  // PPCSR_NO_EDGE: never a stored value (sentinel precondition, PCSR.cpp:64)

// ---- batched edge lookups -----------------------------------------------------------------------------------------
PMA_KERNEL void k_lookup_edges(View v, const uint32_t *__restrict__ qsrc, const uint32_t *__restrict__ qdst, uint64_t nq,
                               uint32_t *__restrict__ out) {
  const int lane = wv::lane();
  const uint64_t wpb = wv::block_dim() >> 6;
  const uint64_t waves = (uint64_t)wv::grid_dim() * wpb;
  const uint64_t nblk = (nq + 63) / 64;
  for (uint64_t b = wv::uni((uint64_t)wv::block_idx() * wpb + (uint64_t)wv::wave_in_block()); b < nblk; b += waves) {
    const uint64_t i = b * 64 + (uint64_t)lane;
    const bool valid = i < nq;
    uint32_t s = kMax, d = 0, beg = 0, end = 0;
    if (valid) {
      s = qsrc[i];
      d = qdst[i];
    }
    const bool inr = valid && s < v.g.n;  // (src >= n: no edge, where the single call reports EINVAL)
    if (inr) {
      const Node nd = v.nodes[s];
      beg = nd.beginning;
      end = nd.end;
    }
    uint32_t res = kNoEdge;
    for (uint64_t m = wv::ballot(inr); m != 0; m &= m - 1) {
      const int j = wv::ctz64(m);
      const uint32_t dj = wv::bcast(d, j);
      // k_edge_exists, for query j
      dev::RangeRec rr;
      rr.on = false;
      dev::SearchHit hit_;
      const uint32_t loc = dev::pma_search(v, dj, wv::bcast(beg, j) + 1, wv::bcast(end, j), rr, &hit_);
      const Edge e = v.items[loc];
      const bool found = !is_null(e) && !is_sentinel(e) && e.dest == dj;
      if (lane == j) res = found ? e.value : kNoEdge;
    }
    if (valid) out[i] = res;
  }
}

// ---- neighbourhood gather -----------------------------------------------------------------------------------------
// per queried vertex: first slot and length of (beginning, end) — empty for vertices >= n and for inverted ranges — and
// its number of 64-slot chunks (counted from the range's first slot)
PMA_KERNEL void k_gather_rows(View v, const uint32_t *__restrict__ q, uint64_t k, uint32_t *__restrict__ rlo, uint32_t *__restrict__ rlen,
                              uint32_t *__restrict__ nch) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < k; i += stride) {
    const uint32_t x = q[i];
    uint32_t lo = 0, len = 0;
    if (x < v.g.n) {
      const Node nd = v.nodes[x];
      lo = nd.beginning + 1u;
      len = nd.end > lo ? nd.end - lo : 0u;
    }
    rlo[i] = lo;
    rlen[i] = len;
    nch[i] = (len + 63u) / 64u;
  }
}
// crow[choff[i]] = i for every row with chunks (crow zeroed before): the inclusive max-scan of crow then maps every
// chunk to its row
PMA_KERNEL void k_gather_mark(const uint32_t *__restrict__ nch, const unsigned long long *__restrict__ choff, uint64_t k,
                              uint32_t *__restrict__ crow) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < k; i += stride)
    if (nch[i] != 0) crow[choff[i]] = (uint32_t)i;
}
// the chunk's place: first slot and number of slots of the range that fall into it (lane-parallel, one chunk per lane)
PMA_DEV void gather_chunk_of(const uint32_t *__restrict__ rlo, const uint32_t *__restrict__ rlen, const unsigned long long *__restrict__ choff,
                             const uint32_t *__restrict__ crow, uint64_t c, uint64_t C, uint32_t &first, uint32_t &cnt) {
  first = 0;
  cnt = 0;
  if (c < C) {
    const uint32_t r = crow[c];
    const uint64_t j = c - choff[r];
    const uint32_t len = rlen[r];
    if (c >= choff[r] && j * 64u < len) {  // (always, for a correct map: never a read outside the row's range)
      first = rlo[r] + (uint32_t)j * 64u;
      cnt = len - (uint32_t)j * 64u < 64u ? len - (uint32_t)j * 64u : 64u;
    }
  }
}
// live slots of every chunk: a wave takes 64 chunks at a time (their row records loaded one per lane), then streams
// them four at a time
PMA_KERNEL void k_gather_count(View v, const uint32_t *__restrict__ rlo, const uint32_t *__restrict__ rlen, const unsigned long long *__restrict__ choff,
                               const uint32_t *__restrict__ crow, uint64_t C, uint32_t *__restrict__ ccnt) {
  const int lane = wv::lane();
  const uint64_t wpb = wv::block_dim() >> 6;
  const uint64_t waves = (uint64_t)wv::grid_dim() * wpb;
  const uint64_t ntile = (C + 63) / 64;
  for (uint64_t t = wv::uni((uint64_t)wv::block_idx() * wpb + (uint64_t)wv::wave_in_block()); t < ntile; t += waves) {
    const uint64_t c = t * 64 + (uint64_t)lane;
    uint32_t first, cnt;
    gather_chunk_of(rlo, rlen, choff, crow, c, C, first, cnt);
    const uint32_t nc = (uint32_t)((C - t * 64) < 64 ? (C - t * 64) : 64);
    uint32_t mine = 0;
    constexpr int K = 4;
    for (uint32_t q0 = 0; q0 < nc; q0 += K) {
      uint32_t val[K];
#pragma unroll
      for (int u = 0; u < K; u++) {
        val[u] = 0;
        if (q0 + u < nc) {
          const uint32_t f = wv::bcast(first, (int)(q0 + u)), n_ = wv::bcast(cnt, (int)(q0 + u));
          if ((uint32_t)lane < n_) val[u] = v.items[f + (uint32_t)lane].value;
        }
      }
#pragma unroll
      for (int u = 0; u < K; u++) {
        const uint32_t live = (uint32_t)wv::popc64(wv::ballot(val[u] != 0));
        if ((uint32_t)lane == q0 + u) mine = live;
      }
    }
    if (c < C) ccnt[c] = mine;
  }
}
// dests (and values) of every chunk at ooff[c] + rank among the chunk's live slots; only positions in [o_lo, o_hi) are
// written, at o - o_lo (the host calls stage the output through a bounded buffer one window at a time)
PMA_KERNEL void k_gather_write(View v, const uint32_t *__restrict__ rlo, const uint32_t *__restrict__ rlen, const unsigned long long *__restrict__ choff,
                               const uint32_t *__restrict__ crow, uint64_t C, const unsigned long long *__restrict__ ooff, uint64_t o_lo, uint64_t o_hi,
                               int *__restrict__ dests, uint32_t *__restrict__ values) {
  const int lane = wv::lane();
  const uint64_t wpb = wv::block_dim() >> 6;
  const uint64_t waves = (uint64_t)wv::grid_dim() * wpb;
  const uint64_t ntile = (C + 63) / 64;
  for (uint64_t t = wv::uni((uint64_t)wv::block_idx() * wpb + (uint64_t)wv::wave_in_block()); t < ntile; t += waves) {
    const uint64_t c = t * 64 + (uint64_t)lane;
    unsigned long long o0 = 0, o1 = 0;
    if (c < C) {
      o0 = ooff[c];
      o1 = ooff[c + 1];
    }
    if (wv::ballot(c < C && o1 > o_lo && o0 < o_hi) == 0) continue;  // nothing of these 64 chunks lies in the window
    uint32_t first, cnt;
    gather_chunk_of(rlo, rlen, choff, crow, c, C, first, cnt);
    const uint32_t nc = (uint32_t)((C - t * 64) < 64 ? (C - t * 64) : 64);
    constexpr int K = 4;
    for (uint32_t q0 = 0; q0 < nc; q0 += K) {
      Edge e[K];
#pragma unroll
      for (int u = 0; u < K; u++) {
        e[u] = null_edge();
        if (q0 + u < nc) {
          const uint32_t f = wv::bcast(first, (int)(q0 + u)), n_ = wv::bcast(cnt, (int)(q0 + u));
          if ((uint32_t)lane < n_) e[u] = v.items[f + (uint32_t)lane];
        }
      }
#pragma unroll
      for (int u = 0; u < K; u++) {
        if (q0 + u >= nc) break;
        const bool live = e[u].value != 0;
        const uint64_t m = wv::ballot(live);
        const uint64_t base = ((uint64_t)wv::bcast((uint32_t)(o0 >> 32), (int)(q0 + u)) << 32) | wv::bcast((uint32_t)o0, (int)(q0 + u));
        const uint64_t o = base + dev::lanemask_lt_count(m, lane);
        if (live && o >= o_lo && o < o_hi) {
          if (dests) dests[o - o_lo] = (int)e[u].dest;
          if (values) values[o - o_lo] = e[u].value;
        }
      }
    }
  }
}
// row_offsets[i] = base + ooff[choff[i]] for i <= k (choff[k] = C, ooff[C] = the block's total)
PMA_KERNEL void k_gather_offsets(const unsigned long long *__restrict__ choff, const unsigned long long *__restrict__ ooff, uint64_t k,
                                 uint64_t base, unsigned long long *__restrict__ rows) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i <= k; i += stride) rows[i] = base + ooff[choff[i]];
}

// ---- scan over any length: reduce-then-scan by tiles ---------------------------------------------------------------
constexpr uint32_t kXsThreads = 256, kXsItems = 16, kXsTile = kXsThreads * kXsItems;

PMA_DEV unsigned long long xs_op(unsigned long long a, unsigned long long b, bool mx) { return mx ? (a > b ? a : b) : a + b; }

// bsum[b] = sum (or max) of tile b of in[0, n)
template <class TI>
PMA_KERNEL void k_xs_reduce(const TI *__restrict__ in, uint64_t n, uint32_t mx, unsigned long long *__restrict__ bsum) {
  PMA_SHARED unsigned long long part[kXsThreads];
  const uint32_t t = wv::thread_idx();
  const uint64_t base = (uint64_t)wv::block_idx() * kXsTile;
  unsigned long long acc = 0;
  for (uint32_t u = 0; u < kXsItems; u++) {
    const uint64_t i = base + (uint64_t)u * kXsThreads + t;
    if (i < n) acc = xs_op(acc, (unsigned long long)in[i], mx != 0);
  }
  part[t] = acc;
  wv::block_sync();
  for (uint32_t s = kXsThreads / 2; s > 0; s >>= 1) {
    if (t < s) part[t] = xs_op(part[t], part[t + s], mx != 0);
    wv::block_sync();
  }
  if (t == 0) bsum[wv::block_idx()] = part[0];
}
// scan of tile b of in[0, n), starting from bbase[b] (nullptr: a single tile, from 0).  incl: out[i] = in[0] op ... op in[i];
// otherwise out[0] = 0 and out[i + 1] = in[0] op ... op in[i] (n + 1 entries).  in == out is allowed for incl (every tile is
// read into LDS before it is written back).
template <class TI, class TO>
PMA_KERNEL void k_xs_scan(const TI *in, uint64_t n, const unsigned long long *__restrict__ bbase, uint32_t mx, uint32_t incl, TO *out) {
  PMA_SHARED unsigned long long tile[kXsTile];
  PMA_SHARED unsigned long long tsum[kXsThreads];
  const uint32_t t = wv::thread_idx();
  const bool m = mx != 0;
  const uint64_t base = (uint64_t)wv::block_idx() * kXsTile;
  for (uint32_t u = 0; u < kXsItems; u++) {
    const uint64_t i = base + (uint64_t)u * kXsThreads + t;
    tile[u * kXsThreads + t] = i < n ? (unsigned long long)in[i] : 0ull;
  }
  wv::block_sync();
  unsigned long long acc = 0;
  for (uint32_t u = 0; u < kXsItems; u++) {
    acc = xs_op(acc, tile[t * kXsItems + u], m);
    tile[t * kXsItems + u] = acc;
  }
  tsum[t] = acc;
  wv::block_sync();
  for (uint32_t off = 1; off < kXsThreads; off <<= 1) {
    const unsigned long long x = t >= off ? tsum[t - off] : 0ull;
    wv::block_sync();
    tsum[t] = xs_op(tsum[t], x, m);
    wv::block_sync();
  }
  const unsigned long long pre = xs_op(bbase ? bbase[wv::block_idx()] : 0ull, t > 0 ? tsum[t - 1] : 0ull, m);
  for (uint32_t u = 0; u < kXsItems; u++) tile[t * kXsItems + u] = xs_op(pre, tile[t * kXsItems + u], m);
  wv::block_sync();
  for (uint32_t u = 0; u < kXsItems; u++) {
    const uint64_t i = base + (uint64_t)u * kXsThreads + t;
    if (i < n) out[incl ? i : i + 1] = (TO)tile[u * kXsThreads + t];
  }
  if (!incl && base == 0 && t == 0) out[0] = (TO)0;
}

}  // namespace ppcsr
