// TEST INFRASTRUCTURE ONLY: the HOST build of the position-chain arithmetic (csrc/pma_geometry.h) behind a few C entry points,
// as a library of its own (tests/hostsim/libchain_host.so) that can be loaded beside the product library: what the device probe
// returns is compared with these, and the division operands of tests/chain_cases.py are collected here.
#include <string.h>

#include "pma_geometry.h"

#define CH_API extern "C" __attribute__((visibility("default")))

CH_API int chain_host_table(uint64_t index, uint64_t len, uint64_t j, uint64_t *segs /* kMaxSeg x 6 */, int *overflow) {
  static ppcsr::ChainTable tb;
  ppcsr::build_chain_table(index, len, j, &tb);
  if (overflow) *overflow = tb.overflow;
  memcpy(segs, tb.seg, sizeof(ppcsr::ChainSeg) * (size_t)tb.nseg);
  return tb.nseg;
}
CH_API int chain_host_single(uint64_t index, uint64_t len, uint64_t j, uint64_t *seg6, int *div_verdict, uint64_t *div_seg6) {
  ppcsr::ChainSeg sg, sd;
  memset(&sg, 0, sizeof(sg));
  memset(&sd, 0, sizeof(sd));
  const bool a = ppcsr::chain_single(index, len, j, &sg), b = ppcsr::chain_single_div(index, len, j, &sd);
  memcpy(seg6, &sg, sizeof(sg));
  memcpy(div_seg6, &sd, sizeof(sd));
  *div_verdict = b ? 1 : 0;
  return a ? 1 : 0;
}
// the division operands the table build of a window meets: (M1 - Th, Drest) of every segment whose step count takes the
// division (restated from chain_segment: Th = 2^52 + (S >> r) + (any bit of S below r set), M1 = M0 - Dfirst)
CH_API int chain_host_div_operands(uint64_t index, uint64_t len, uint64_t j, uint64_t *ab /* kMaxSeg x 2 */) {
  static ppcsr::ChainTable tb;
  ppcsr::build_chain_table(index, len, j, &tb);
  if (j < 2) return 0;
  const uint64_t sb = ppcsr::dbl_bits(ppcsr::chain_step(len, j));
  const int es = (int)((sb >> 52) & 0x7FF) - 1023;
  const uint64_t S = (sb & 0xFFFFFFFFFFFFFull) | (1ull << 52);
  int n = 0;
  for (int s = 0; s < tb.nseg; s++) {
    const ppcsr::ChainSeg &sg = tb.seg[s];
    const int r = (52 - sg.shift) - es;
    if (sg.shift < 0 || r < 0 || r > 52 || sg.Drest == 0) continue;
    const uint64_t q = r ? (S >> r) : S, rem = r ? (S & ((1ull << r) - 1)) : 0;
    const uint64_t Th = (1ull << 52) + q + (rem ? 1 : 0);
    if (sg.M0 < Th || sg.M0 - sg.Dfirst < Th) continue;
    ab[2 * n] = sg.M0 - sg.Dfirst - Th;
    ab[2 * n + 1] = sg.Drest;
    n++;
  }
  return n;
}
// density thresholds of an array of N slots (compute_geometry): t_up / t_lo per level, kMaxLevels words each; returns H
CH_API int chain_host_thresholds(uint64_t N, uint32_t *t_up, uint32_t *t_lo, int *logN) {
  ppcsr::Geometry g;
  ppcsr::compute_geometry(N, 1, 1, &g);
  memcpy(t_up, g.t_up, sizeof(g.t_up));
  memcpy(t_lo, g.t_lo, sizeof(g.t_lo));
  *logN = g.logN;
  return g.H;
}
