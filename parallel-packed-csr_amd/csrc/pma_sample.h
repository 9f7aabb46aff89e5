// Neighbour sampling, random walks and live degrees over the table of gapped arrays (pma_consumer.h).  The definition is the one
// of include/ppcsr.h: L(v) = the live slots of (beginning, end) in slot order — non-null, non-sentinel, not slot N-1, global
// dest < n —, every entry with a measure (1, or the edge value), W(v) their sum; draw (seed, i, j) is
// r = mulhi(x(seed, i, j), W(v)) and picks the first entry whose inclusive cumulative measure exceeds r.  Nothing depends on
// the launch geometry, the gaps or the partitioning.
//   k_sm_hubs        the vertices with a range beyond kBfsWaveSlots among the queried ones (or among all: the walks), each
//                    listed once (a claim word per vertex): its array, its slot range, its number of 64-slot chunks
//   k_sm_hub_count   measure of every chunk of the listed hubs, split by chunks like the gather (gather_chunk_of over the
//                    chunk -> hub map of k_gather_mark + max-scan); its exclusive scan is the hubs' prefix, built once per call
//   k_sm_sample      one wave per query: sm_draws with `fanout` draws
//   k_sm_walk        one launch per step, one wave per walker: sm_draws with the one draw (seed, i, t)
//   sm_draws         a range of one chunk: loaded once, its lane prefix of measures in LDS, every draw a search of it.  Ordinary
//                    vertex: one counting walk over the range, lane c keeping the measure of chunk c, a wave prefix over the
//                    64 sums (W and the chunk of every draw); hub: a binary search of the call's prefix.  Then the draws, one
//                    per lane, 64 at a time: the wave re-reads each DISTINCT owning chunk once (the ballot loop of
//                    k_lookup_edges) and every draw of that chunk selects its slot from the chunk's lane prefix
//   k_sm_degrees     |L(v)| and the weighted W(v) of every vertex from one streaming pass (sources from the items: either regime)
#pragma once
#include "pma_consumer.h"
#include "pma_query.h"

namespace ppcsr {

constexpr uint32_t kNoVertex = 0xFFFFFFFFu;   // PPCSR_NO_VERTEX
constexpr uint32_t kSmWeighted = 1u;          // flags bit 0: the measure is the edge value
constexpr uint32_t kSmClaimed = 0xFFFFFFFEu;  // hub claim word: taken, index not yet stored (never a hub index)

// ---- the counter-based generator ---------------------------------------------------------------------------------------------
PMA_DEV unsigned long long sm_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
PMA_DEV unsigned long long sm_draw(unsigned long long seed, unsigned long long i, unsigned long long j) {
  return sm_mix(sm_mix(sm_mix(seed) + i) + j);
}
PMA_KERNEL void k_sm_mulhi(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b, uint64_t k,
                           unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < k; i += stride) out[i] = wv::mulhi64(a[i], b[i]);
}

// ---- wave pieces ---------------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the wave's lanes
PMA_DEV unsigned long long sm_wave_scan(unsigned long long v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = cp_shfl(v, lane >= d ? lane - d : lane);
    if (lane >= d) v += o;
  }
  return v;
}
PMA_DEV unsigned long long sm_bcast64(unsigned long long v, int src) {
  return ((unsigned long long)wv::bcast((uint32_t)(v >> 32), src) << 32) | wv::bcast((uint32_t)v, src);
}
// sum over the wave of values below 2^32, as a scalar: the two 16-bit halves are summed apart (each sum stays below 2^22)
PMA_DEV unsigned long long sm_wave_sum(uint32_t m) {
  return ((unsigned long long)wv::reduce_add(m >> 16) << 16) + (unsigned long long)wv::reduce_add(m & 0xFFFFu);
}
// slot first + lane of a chunk of cnt slots (null beyond it; slot N-1 is never part of a neighbourhood)
PMA_DEV Edge sm_load(const Edge *__restrict__ items, uint64_t N, uint64_t first, uint32_t cnt, int lane) {
  Edge e = null_edge();
  const uint64_t s = first + (uint64_t)lane;
  if ((uint32_t)lane < cnt && s + 1 < N) e = items[s];
  return e;
}
// measure of a slot: 0 unless it is an entry of L(v)
PMA_DEV uint32_t sm_measure(const Edge &e, uint32_t n, bool weighted) {
  const bool live = e.value != 0 && !is_sentinel(e) && e.dest < n;
  return live ? (weighted ? e.value : 1u) : 0u;
}
// measure of the chunk the wave has loaded (a scalar)
PMA_DEV unsigned long long sm_chunk_total(uint32_t m, bool weighted) {
  return weighted ? sm_wave_sum(m) : (unsigned long long)wv::popc64(wv::ballot(m != 0));
}

// ---- hubs ------------------------------------------------------------------------------------------------------------------------
struct SmHubs {
  const uint32_t *hid;               // per vertex: index in the hub list (kNoVertex: not listed)
  const uint32_t *part;              // per hub: its array's table entry
  const uint32_t *rlo, *rlen;        // per hub: first slot and length of its range
  const unsigned long long *choff;   // per hub (+ 1): its first chunk in the hubs' chunk space
  const unsigned long long *cpre;    // per chunk (+ 1): measure of the chunks before it
};
// q == nullptr: every vertex (k == n).  The list has room for cap hubs (ranges are disjoint: slots / kBfsWaveSlots bounds them);
// *count may pass it, which the host refuses.
PMA_KERNEL void k_sm_hubs(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ q, uint64_t k, uint32_t *hid,
                          uint32_t *__restrict__ part, uint32_t *__restrict__ rlo, uint32_t *__restrict__ rlen, uint32_t *__restrict__ nch,
                          uint32_t cap, uint32_t *count) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < k; i += stride) {
    const uint32_t v = q ? q[i] : (uint32_t)i;
    if (v >= n) continue;
    const uint32_t kp = P > 1 ? cp_owner(tab, P, v) : 0u;
    const Node nd = tab[kp].nodes[v - tab[kp].first];
    const uint32_t lo = nd.beginning + 1u;
    const uint32_t len = nd.end > lo ? nd.end - lo : 0u;
    if ((uint64_t)len <= kBfsWaveSlots) continue;
    if (wv::atomic_cas_u32(&hid[v], kNoVertex, kSmClaimed) != kNoVertex) continue;
    const uint32_t h = wv::atomic_add_u32(count, 1u);
    if (h >= cap) continue;
    hid[v] = h;
    part[h] = kp;
    rlo[h] = lo;
    rlen[h] = len;
    nch[h] = (len + 63u) / 64u;
  }
}
// cm[c] = measure of chunk c of the hubs' chunk space: a wave takes 64 chunks at a time (their places loaded one per lane),
// then streams them four at a time (k_gather_count)
PMA_KERNEL void k_sm_hub_count(const ConsumerPart *__restrict__ tab, uint32_t n, SmHubs hb, const uint32_t *__restrict__ crow, uint64_t C,
                               uint32_t weighted, unsigned long long *__restrict__ cm) {
  const int lane = wv::lane();
  const uint64_t ntile = (C + 63) / 64;
  const uint64_t waves = cp_waves();
  for (uint64_t t = wv::uni(cp_wave()); t < ntile; t += waves) {
    const uint64_t c = t * 64 + (uint64_t)lane;
    uint32_t first, cnt, kp = 0;
    gather_chunk_of(hb.rlo, hb.rlen, hb.choff, crow, c, C, first, cnt);
    if (c < C) kp = hb.part[crow[c]];
    const uint32_t nc = (uint32_t)((C - t * 64) < 64 ? (C - t * 64) : 64);
    unsigned long long mine = 0;
    constexpr int K = 4;
    for (uint32_t q0 = 0; q0 < nc; q0 += K) {
      Edge e[K];
#pragma unroll
      for (int u = 0; u < K; u++) {
        e[u] = null_edge();
        if (q0 + u < nc) {
          const ConsumerPart &pt = tab[wv::bcast(kp, (int)(q0 + u))];
          e[u] = sm_load(pt.items, pt.N, (uint64_t)wv::bcast(first, (int)(q0 + u)), wv::bcast(cnt, (int)(q0 + u)), lane);
        }
      }
#pragma unroll
      for (int u = 0; u < K; u++) {
        const unsigned long long tot = sm_chunk_total(sm_measure(e[u], n, weighted != 0), weighted != 0);
        if ((uint32_t)lane == q0 + u) mine = tot;
      }
    }
    if (c < C) cm[c] = mine;
  }
}

// ---- the draws of one query, by one wave -----------------------------------------------------------------------------------------
struct SmLds {  // one per wave
  unsigned long long cp[64];  // ordinary vertex: inclusive measure prefix over its chunks
  unsigned long long sp[64];  // the chunk being selected from: inclusive measure prefix over its slots
  uint32_t d[64], v[64];      // that chunk's dests and values
};
// first p of [0, 63] with a[p] > r (a ascending, a[63] > r)
PMA_DEV uint32_t sm_first_above(const unsigned long long *a, unsigned long long r) {
  uint32_t lo = 0, hi = 63;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] > r) hi = mid; else lo = mid + 1u;
  }
  return lo;
}
// Draws (seed, i, j0 + jj) for jj < nd from L(v), written to od[jj] (and the edge values to ov[jj], unless null).  v and every
// other argument is wave-uniform; called by the whole wave.
PMA_DEV void sm_draws(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const SmHubs &hb, uint32_t v, unsigned long long i, uint32_t j0,
                      uint32_t nd, unsigned long long seed, bool weighted, uint32_t *od, uint32_t *ov, SmLds &L, int lane) {
  const Edge *items = nullptr;
  uint64_t N = 0;
  uint32_t lo = 0, len = 0;
  if (v < n) {
    const uint32_t kp = P > 1 ? cp_owner(tab, P, v) : 0u;
    const Node node = tab[kp].nodes[v - tab[kp].first];
    items = tab[kp].items;
    N = tab[kp].N;
    lo = wv::uni(node.beginning + 1u);
    len = wv::uni(node.end > lo ? node.end - lo : 0u);
  }
  if (len != 0 && len <= 64u) {
    // one chunk (most vertices of a sparse graph): loaded once, counted and selected from where it stands
    const Edge e = sm_load(items, N, (uint64_t)lo, len, lane);
    const uint32_t ms = sm_measure(e, n, weighted);
    unsigned long long sp, W1;
    if (weighted) {
      sp = sm_wave_scan((unsigned long long)ms, lane);
      W1 = sm_bcast64(sp, 63);
    } else {
      const uint64_t m = wv::ballot(ms != 0);
      sp = (unsigned long long)(dev::lanemask_lt_count(m, lane) + ms);
      W1 = (unsigned long long)wv::popc64(m);
    }
    L.sp[lane] = sp;
    L.d[lane] = e.dest;
    L.v[lane] = e.value;
    wv::lds_fence();
    for (uint32_t jj = (uint32_t)lane; jj < nd; jj += 64u) {
      uint32_t pd = kNoVertex, pv = 0;
      if (W1 != 0) {
        const uint32_t p = sm_first_above(L.sp, wv::mulhi64(sm_draw(seed, i, (unsigned long long)j0 + jj), W1));
        pd = L.d[p];
        pv = L.v[p];
      }
      od[jj] = pd;
      if (ov) ov[jj] = pv;
    }
    wv::lds_fence();  // (the chunk's arrays are rewritten by the wave's next query)
    return;
  }
  const bool hub = (uint64_t)len > kBfsWaveSlots;
  unsigned long long W = 0, base = 0;
  uint64_t c_lo = 0, c_hi = 0;
  if (hub) {
    const uint32_t h = hb.hid[v];
    c_lo = hb.choff[h];
    c_hi = hb.choff[h + 1u];
    base = hb.cpre[c_lo];
    W = hb.cpre[c_hi] - base;
  } else if (len != 0) {
    // the counting walk: lane c keeps the measure of chunk c, four chunks in flight
    const uint32_t nch = (len + 63u) / 64u;
    unsigned long long mine = 0;
    constexpr int K = 4;
    for (uint32_t c0 = 0; c0 < nch; c0 += K) {
      Edge e[K];
#pragma unroll
      for (int u = 0; u < K; u++) {
        const uint32_t off = (c0 + u) * 64u;
        e[u] = sm_load(items, N, (uint64_t)lo + off, off < len ? (len - off < 64u ? len - off : 64u) : 0u, lane);
      }
#pragma unroll
      for (int u = 0; u < K; u++) {
        const unsigned long long tot = sm_chunk_total(sm_measure(e[u], n, weighted), weighted);
        if ((uint32_t)lane == c0 + u) mine = tot;
      }
    }
    const unsigned long long cp = sm_wave_scan(mine, lane);
    W = sm_bcast64(cp, 63);
    L.cp[lane] = cp;
    wv::lds_fence();
  }
  for (uint32_t jb = 0; jb < nd; jb += 64u) {
    const uint32_t jj = jb + (uint32_t)lane;
    const bool active = jj < nd && W != 0;
    uint32_t crel = 0;         // the draw's chunk, counted from the range's first
    unsigned long long rr = 0;  // what is left of r inside that chunk
    if (active) {
      const unsigned long long r = wv::mulhi64(sm_draw(seed, i, (unsigned long long)j0 + jj), W);
      if (hub) {
        uint64_t a = c_lo, b = c_hi - 1;  // first chunk c with cpre[c + 1] - base > r
        while (a < b) {
          const uint64_t mid = (a + b) >> 1;
          if (hb.cpre[mid + 1] - base > r) b = mid; else a = mid + 1;
        }
        crel = (uint32_t)(a - c_lo);
        rr = r - (hb.cpre[a] - base);
      } else {
        crel = sm_first_above(L.cp, r);
        rr = r - (crel ? L.cp[crel - 1u] : 0ull);
      }
    }
    uint32_t pd = kNoVertex, pv = 0;
    for (uint64_t m = wv::ballot(active); m != 0;) {
      const uint32_t c = wv::bcast(crel, wv::ctz64(m));
      const bool in = active && crel == c;
      const uint32_t off = c * 64u;
      const Edge e = sm_load(items, N, (uint64_t)lo + off, len - off < 64u ? len - off : 64u, lane);
      const uint32_t ms = sm_measure(e, n, weighted);
      L.sp[lane] = weighted ? sm_wave_scan((unsigned long long)ms, lane)
                            : (unsigned long long)(dev::lanemask_lt_count(wv::ballot(ms != 0), lane) + ms);
      L.d[lane] = e.dest;
      L.v[lane] = e.value;
      wv::lds_fence();
      if (in) {
        const uint32_t p = sm_first_above(L.sp, rr);
        pd = L.d[p];
        pv = L.v[p];
      }
      wv::lds_fence();  // (the chunk's arrays are rewritten by the next step)
      m &= ~wv::ballot(in);
    }
    if (jj < nd) {
      od[jj] = pd;
      if (ov) ov[jj] = pv;
    }
  }
  wv::lds_fence();  // (L.cp is rewritten by the wave's next query)
}

// dests[f * fanout + j] (and values) = draw (seed, i0 + f, j) from L(q[f]), one wave per query
PMA_KERNEL void k_sm_sample(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, SmHubs hb, const uint32_t *__restrict__ q, uint64_t k,
                            unsigned long long i0, uint32_t fanout, unsigned long long seed, uint32_t flags, uint32_t *dests, uint32_t *values) {
  PMA_SHARED SmLds lds[4];
  const int lane = wv::lane(), w = wv::wave_in_block();
  const uint64_t wstride = cp_waves();
  for (uint64_t f = wv::uni(cp_wave()); f < k; f += wstride) {
    const uint32_t v = wv::uni(q[f]);
    sm_draws(tab, P, n, hb, v, i0 + f, 0u, fanout, seed, (flags & kSmWeighted) != 0, dests + f * fanout, values ? values + f * fanout : nullptr,
             lds[w], lane);
  }
}
// out[f][0] = the start, or kNoVertex when it is no vertex
PMA_KERNEL void k_sm_walk_init(const uint32_t *__restrict__ q, uint64_t k, uint32_t n, uint32_t length, uint32_t *__restrict__ out) {
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < k; i += stride)
    out[i * ((uint64_t)length + 1)] = q[i] < n ? q[i] : kNoVertex;
}
// step t of every walker: out[f][t + 1] = draw (seed, i0 + f, t) from L(out[f][t]); kNoVertex stays kNoVertex
PMA_KERNEL void k_sm_walk(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, SmHubs hb, uint32_t *out, uint64_t k, unsigned long long i0,
                          uint32_t length, uint32_t t, unsigned long long seed, uint32_t flags) {
  PMA_SHARED SmLds lds[4];
  const int lane = wv::lane(), w = wv::wave_in_block();
  const uint64_t wstride = cp_waves();
  for (uint64_t f = wv::uni(cp_wave()); f < k; f += wstride) {
    uint32_t *row = out + f * ((uint64_t)length + 1);
    const uint32_t v = wv::uni(row[t]);
    sm_draws(tab, P, n, hb, v, i0 + f, t, 1u, seed, (flags & kSmWeighted) != 0, row + t + 1u, nullptr, lds[w], lane);
  }
}

// ---- live degrees ------------------------------------------------------------------------------------------------------------------
// deg[v] += 1 and wsum[v] += value for every live edge of the streaming pass (either may be null; both zeroed before).  A
// vertex's slots are contiguous, so the lanes of a wave share few sources: their runs are summed in the wave and one lane
// issues the add (cp_combine_runs).
constexpr int kSmRunLanes = 8;
PMA_KERNEL void k_sm_degrees(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, uint32_t *deg, unsigned long long *wsum) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&live)[kB], int lane) {
#pragma unroll
    for (int b = 0; b < kB; b++) {
      if (deg) {
        uint32_t one = live[b] ? 1u : 0u;
        if (cp_combine_runs<kSmRunLanes>(live[b], src[b], one, 0u, lane, [](uint32_t x, int) { return wv::reduce_add(x); }))
          wv::atomic_add_u32(&deg[src[b]], one);
      }
      if (wsum) {
        unsigned long long val = live[b] ? (unsigned long long)e[b].value : 0ull;
        if (cp_combine_runs<kSmRunLanes>(live[b], src[b], val, 0ull, lane, [](unsigned long long x, int) {
              // (a run's values are below 2^32 each: the lanes outside it give 0)
              return sm_wave_sum((uint32_t)x);
            }))
          wv::atomic_add_u64(&wsum[src[b]], val);
      }
    }
  });
}

}  // namespace ppcsr
