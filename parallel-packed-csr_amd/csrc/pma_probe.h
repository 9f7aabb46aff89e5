// Debugging probe of the rebalance position chain (ppcsr_debug_chain_probe): kernels that run the PRODUCTION functions of
// pma_geometry.h / pma_rebalance.h on the device — build_chain_table, build_chain_table_publish + rb_table_to_lds, chain_single +
// chain_single_pos, chain_pos, chain_linear_run, chain_segment, chain_sub, div_floor_u53 — and hand back what they return, so
// that the tests can hold the device's branch of that arithmetic (the reciprocal estimate, its u64 -> f64 conversions, clz) to
// the reference's serial fp64 chain.  Nothing here computes a mantissa, a step or a shift of its own, and nothing touches the
// engine's state: every kernel writes into the probe's own buffers only.
#pragma once
#include "pma_rebalance.h"

namespace ppcsr {

constexpr int kProbeDigestLog = 20;      // one digest per block of 2^20 consecutive ranks
constexpr uint32_t kProbeThreads = 256;  // workgroup of the expanding kernels
constexpr uint32_t kProbeTile = 4096;    // ranks per workgroup pass of the expanding kernels (divides 2^kProbeDigestLog)
constexpr uint32_t kProbeWalk = 4096;    // chain_sub steps walked per `segment` case, at most
constexpr uint32_t kProbeFallback = 0xFFFFFFFFu;  // what rb_table_to_lds leaves in its flag when the bounded spin ran out

// order-independent digest of a block of (k, pos_k) pairs: the wrapping sum of splitmix64(pos_k + k * golden)
PMA_HD inline uint64_t probe_mix(uint64_t k, uint64_t pos) {
  uint64_t z = pos + k * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ranks [r_lo, r_hi) expanded by one workgroup from its LDS copy of the table: thread-strided, one segment cursor per thread
// as in the scatter; positions go to pos_out[k] (small cases) or into the digest of k's block (big cases)
PMA_DEV void probe_expand_range(const ChainTable *stb, uint64_t r_lo, uint64_t r_hi, uint64_t *pos_out, unsigned long long *digest) {
  int hint = -1;
  for (uint64_t t0 = r_lo; t0 < r_hi; t0 += kProbeTile) {  // (r_lo is a multiple of kProbeTile: a pass lies in one digest block)
    unsigned long long acc = 0;
    for (uint64_t k = t0 + wv::thread_idx(); k < t0 + kProbeTile && k < r_hi; k += wv::block_dim()) {
      const uint64_t pos = chain_pos(stb, k, &hint);
      if (pos_out) pos_out[k] = pos;
      acc += probe_mix(k, pos);
    }
    if (digest && acc) wv::atomic_add_u64(&digest[t0 >> kProbeDigestLog], acc);
  }
}

// ---- `table`: one thread builds the table (as k_scan_tilesums does), a grid expands it -----------------------------------
PMA_KERNEL void k_probe_table(ChainTable *tb, uint64_t index, uint64_t len, uint64_t j) {
  if (wv::block_idx() == 0 && wv::thread_idx() == 0) build_chain_table(index, len, j, tb);
}
PMA_KERNEL void k_probe_expand(const ChainTable *tb, uint64_t *pos_out, unsigned long long *digest) {
  PMA_SHARED ChainTable stb;
  {  // (the copy k_rb_scatter makes of a table that was built ahead of the launch)
    const uint32_t *g = reinterpret_cast<const uint32_t *>(tb);
    uint32_t *sp = reinterpret_cast<uint32_t *>(&stb);
    const uint32_t words = (uint32_t)((sizeof(ChainTable) - sizeof(ChainSeg) * (size_t)(kMaxSeg - tb->nseg)) / 4);
    for (uint32_t i = wv::thread_idx(); i < words; i += wv::block_dim()) sp[i] = g[i];
  }
  wv::block_sync();
  const uint64_t j = stb.j;
  for (uint64_t r0 = (uint64_t)wv::block_idx() * kProbeTile; r0 < j; r0 += (uint64_t)wv::grid_dim() * kProbeTile)
    probe_expand_range(&stb, r0, r0 + kProbeTile < j ? r0 + kProbeTile : j, pos_out, digest);
}
// literal positions of chosen ranks, straight from the table in device memory
PMA_KERNEL void k_probe_sample(const ChainTable *tb, const uint64_t *ks, uint64_t nk, uint64_t *out) {
  int hint = -1;
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t i = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); i < nk; i += stride) out[i] = chain_pos(tb, ks[i], &hint);
}

// ---- `published`: the hand-off of k_rb_scatter with defer_table ------------------------------------------------------------
// the header, written the way k_scan_tilesums writes it for a deferred table (the segment area has been poisoned before)
PMA_KERNEL void k_probe_header(ChainTable *tb, uint64_t index, uint64_t len, uint64_t j) {
  if (wv::block_idx() == 0 && wv::thread_idx() == 0) {
    tb->index = index;
    tb->len = len;
    tb->j = j;
    tb->nseg = 0;
    tb->overflow = 0;
    tb->pub_nseg = j < 2u ? kTbDone : 0u;
    tb->pub_t = 0;
  }
}
// workgroup 0 builds and publishes; every workgroup takes the rank tile counted from the top of the window down, waits for the
// part of the table its own ranks need, copies that part to LDS and expands its ranks from the copy.  wg_flag[b]: segments
// workgroup b copied, or kProbeFallback.  tile_ranks is a multiple of kProbeTile
PMA_KERNEL void k_probe_published(ChainTable *tb, uint64_t tile_ranks, uint64_t *pos_out, unsigned long long *digest, uint32_t *wg_flag) {
  PMA_SHARED ChainTable stb;
  PMA_SHARED uint32_t s_flag;
  const uint64_t tile = (uint64_t)wv::grid_dim() - 1ull - wv::block_idx();
  const uint64_t jj = tb->j, r0 = tile * tile_ranks;
  rb_table_to_lds(tb, &stb, jj > r0 ? jj - 1ull - r0 : 0ull, wv::block_idx() == 0, &s_flag);
  if (wv::thread_idx() == 0) wg_flag[wv::block_idx()] = s_flag;
  if (r0 >= jj) return;
  probe_expand_range(&stb, r0, r0 + tile_ranks < jj ? r0 + tile_ranks : jj, pos_out, digest);
}

// ---- `single`: the closed form of the in-wave rebalance ---------------------------------------------------------------------
// verdict in tb->nseg (1 = accepted), the segment in tb->seg[0]
PMA_KERNEL void k_probe_single(ChainTable *tb, uint64_t index, uint64_t len, uint64_t j) {
  if (wv::block_idx() == 0 && wv::thread_idx() == 0) {
    ChainSeg sg = {};
    const bool ok = chain_single(index, len, j, &sg);
    tb->index = index;
    tb->len = len;
    tb->j = j;
    tb->overflow = 0;
    tb->seg[0] = sg;
    tb->nseg = ok ? 1 : 0;
  }
}
PMA_KERNEL void k_probe_single_expand(const ChainTable *tb, uint64_t *pos_out, unsigned long long *digest) {
  if (tb->nseg != 1) return;
  const ChainSeg sg = tb->seg[0];
  const uint64_t index = tb->index, j = tb->j;
  for (uint64_t t0 = (uint64_t)wv::block_idx() * kProbeTile; t0 < j; t0 += (uint64_t)wv::grid_dim() * kProbeTile) {
    unsigned long long acc = 0;
    for (uint64_t k = t0 + wv::thread_idx(); k < t0 + kProbeTile && k < j; k += wv::block_dim()) {
      const uint64_t pos = chain_single_pos(sg, index, j, k);
      if (pos_out) pos_out[k] = pos;
      acc += probe_mix(k, pos);
    }
    if (digest && acc) wv::atomic_add_u64(&digest[t0 >> kProbeDigestLog], acc);
  }
}

// ---- `linear`: chain_linear_run on runs of <= 64 consecutive ranks at stride 37 against chain_pos of the same table ----------
// out[0]: positions that differ, out[1]: runs the linear form accepted
PMA_KERNEL void k_probe_linear(const ChainTable *tb, unsigned long long *out) {
  const uint64_t j = tb->j;
  if (j < 3) return;
  const uint64_t nruns = (j - 3) / 37 + 1;  // k0 = 1, 38, 75 ... while k0 + 1 < j
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  int h = -1, h3 = -1;
  unsigned long long bad = 0, taken = 0;
  for (uint64_t r = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx(); r < nruns; r += stride) {
    const uint64_t k0 = 1 + r * 37;
    const uint64_t cnt = (k0 + 64 <= j - 1) ? 64 : (j - 1 - k0);
    uint64_t A, D;
    int shift;
    if (chain_linear_run(tb, k0, cnt, &h3, &A, &D, &shift)) {
      taken++;
      for (uint64_t i = 0; i <= cnt; i++)
        if (((A + i * D) >> shift) != chain_pos(tb, k0 + i, &h)) bad++;  // (the form rb_scatter_chunk evaluates)
    }
  }
  if (bad) wv::atomic_add_u64(&out[0], bad);
  if (taken) wv::atomic_add_u64(&out[1], taken);
}

// ---- `segment`: chain_segment on raw operands, then the device's own subtractions -------------------------------------------
// ops: 4 words per case (bits of x, bits of step, S, es); segs: the six words of the segment (count = the returned step
// count); walk: kProbeWalk words per case, the bits of x - step, x - 2 step ... for min(count + 1, kProbeWalk) steps
PMA_KERNEL void k_probe_segment(const uint64_t *ops, uint64_t n, ChainSeg *segs, uint32_t *nwalk, uint64_t *walk) {
  const uint64_t c = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx();
  if (c >= n) return;
  const double x = bits_dbl(ops[4 * c]), step = bits_dbl(ops[4 * c + 1]);
  ChainSeg sg;
  sg.t0 = 0;
  sg.count = chain_segment(x, ops[4 * c + 2], (int)(int64_t)ops[4 * c + 3], &sg);
  segs[c] = sg;
  const uint32_t steps = sg.count + 1 < (uint64_t)kProbeWalk ? (uint32_t)(sg.count + 1) : kProbeWalk;
  double v = x;
  for (uint32_t i = 0; i < steps; i++) {
    v = chain_sub(v, step);
    walk[c * kProbeWalk + i] = dbl_bits(v);
  }
  nwalk[c] = steps;
}

// ---- `div`: the quotient and, beside it, the raw estimate it was fixed up from ------------------------------------------------
PMA_KERNEL void k_probe_div(const uint64_t *ops, uint64_t n, uint64_t *out) {
  const uint64_t c = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx();
  if (c >= n) return;
  out[2 * c] = div_floor_u53(ops[2 * c], ops[2 * c + 1]);
  out[2 * c + 1] = div_estimate_u53(ops[2 * c], ops[2 * c + 1]);
}

}  // namespace ppcsr
