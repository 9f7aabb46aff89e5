// Debugging probe of the neighbourhood intersections (ppcsr_debug_isect_probe): kernels that run the PRODUCTION routines of
// pma_intersect.h — isect_lane, isect_wave (and through it isect_probe / isect_probe_tile), isect_block (and through it
// isect_lower_bound), isect_lower_bound, isect_probe — on slot ranges the caller lays out slot by slot, in the launch shapes the
// consumers use them in, and hand back what they return.  Nothing here compares a dest or moves a cursor of its own, and
// nothing touches the engine's state: every kernel writes into the probe's own buffers only.
#pragma once
#include "pma_intersect.h"

namespace ppcsr {

constexpr uint32_t kIsectProbeThreads = 256;  // workgroup of every probe kernel (four waves, as k_tri_edges / k_tri_long)

// one case: slot ranges [alo, ahi) of the first buffer and [blo, bhi) of the second, the filter from <= c < n (modes that
// intersect) or the key searched for in [blo, bhi) (the other two)
struct IsectCase {
  uint32_t alo, ahi, blo, bhi, fk, n;
};

// one case per lane: the 64 cases of a wave diverge as the 64 edges of a chunk do in k_tri_edges
PMA_KERNEL void k_probe_isect_lane(const Edge *__restrict__ ia, const Edge *__restrict__ ib, const IsectCase *__restrict__ cs, uint64_t nc, uint32_t *out,
                                   unsigned long long *tri) {
  const uint64_t c = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx();
  if (c >= nc) return;
  const IsectCase k = cs[c];
  out[c] = isect_lane(ia, k.alo, k.ahi, ib, k.blo, k.bhi, k.fk, k.n, tri);
}
// one wave per case, four waves per workgroup, each with an LDS tile of its own
PMA_KERNEL void k_probe_isect_wave(const Edge *__restrict__ ia, const Edge *__restrict__ ib, const IsectCase *__restrict__ cs, uint64_t nc, uint32_t *out,
                                   unsigned long long *tri) {
  PMA_SHARED uint32_t tiles[4][64];
  const int w = wv::wave_in_block();
  const uint64_t c = wv::uni((uint64_t)wv::block_idx() * (wv::block_dim() >> 6) + (uint64_t)w);
  if (c >= nc) return;
  const IsectCase k = cs[c];
  const uint32_t r = isect_wave(ia, k.alo, k.ahi, ib, k.blo, k.bhi, k.fk, k.n, tiles[w], tri);
  if (wv::lane() == 0) out[c] = r;
}
// one workgroup per case; out[] has been zeroed: every wave adds its share
PMA_KERNEL void k_probe_isect_block(const Edge *__restrict__ ia, const Edge *__restrict__ ib, const IsectCase *__restrict__ cs, uint32_t *out,
                                    unsigned long long *tri) {
  PMA_SHARED uint32_t tile[kIsectTile];
  PMA_SHARED uint32_t mm[2];
  const IsectCase k = cs[wv::block_idx()];
  const uint32_t r = isect_block(ia, k.alo, k.ahi, ib, k.blo, k.bhi, k.fk, k.n, tile, mm, tri);
  if (wv::lane() == 0 && r) wv::atomic_add_u32(&out[wv::block_idx()], r);
}
// one wave per case: the slot isect_lower_bound returns for (ib, blo, bhi, key)
PMA_KERNEL void k_probe_isect_lower_bound(const Edge *__restrict__ ib, const IsectCase *__restrict__ cs, uint64_t nc, uint32_t *out) {
  const uint64_t c = wv::uni((uint64_t)wv::block_idx() * (wv::block_dim() >> 6) + (uint64_t)wv::wave_in_block());
  if (c >= nc) return;
  const IsectCase k = cs[c];
  const uint32_t r = isect_lower_bound(ib, k.blo, k.bhi, k.fk);
  if (wv::lane() == 0) out[c] = r;
}
// one case per lane: every lane its own search, as in the lopsided form of isect_wave; slot: the slot itself is handed back
// (kMax: none), as tr_find of pma_truss.h takes it
PMA_KERNEL void k_probe_isect_probe(const Edge *__restrict__ ib, const IsectCase *__restrict__ cs, uint64_t nc, uint32_t *out, uint32_t slot) {
  const uint64_t c = (uint64_t)wv::block_idx() * wv::block_dim() + wv::thread_idx();
  if (c >= nc) return;
  const IsectCase k = cs[c];
  if (slot) out[c] = isect_probe_slot(ib, k.blo, k.bhi, k.fk);
  else out[c] = isect_probe(ib, k.blo, k.bhi, k.fk) ? 1u : 0u;
}

}  // namespace ppcsr
