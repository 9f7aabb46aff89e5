// Wavefront primitives used by the PMA kernels.  Product build: gfx950 intrinsics (wave64).
// When PPCSR_SIM is defined (tests/hostsim only — never in the shipped library) the same names are
// provided by a single-threaded fiber SIMT emulator so the kernel source can be debugged on CPU.
#pragma once
#include "pma_types.h"

#if defined(PPCSR_SIM)
#include "sim_runtime.h"
// The emulator's forms of vec / any / all / opaque / setlanes (their product forms and what they are for: below), on the runtime's
// own collectives: vec and opaque make the claim of uni() and are checked like it, any / all are ballots of the live lanes.
namespace ppcsr {
namespace wv {
inline uint32_t vec(uint32_t v) { return (uint32_t)sim::uniform64(v); }
inline uint64_t vec(uint64_t v) { return sim::uniform64(v); }
inline bool any(bool p) { return sim::ballot(p) != 0; }
inline bool all(bool p) { return sim::ballot(!p) == 0; }
inline uint32_t opaque(uint32_t v) { return (uint32_t)sim::uniform64(v); }
template <int K0, int K1, int K2, int K3>
inline uint32_t setlanes(uint32_t v, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  const int l = lane();
  return l == K0 ? x0 : l == K1 ? x1 : l == K2 ? x2 : l == K3 ? x3 : v;
}
}  // namespace wv
}  // namespace ppcsr
#else
#include <hip/hip_runtime.h>
#define PMA_DEV __device__ __forceinline__
#define PMA_KERNEL __global__
#define PMA_LAUNCH_BOUNDS(threads, waves_per_simd) __launch_bounds__(threads, waves_per_simd)
#define PMA_SHARED __shared__

namespace ppcsr {
namespace wv {
PMA_DEV int lane() { return (int)(threadIdx.x & 63u); }
PMA_DEV int wave_in_block() { return (int)(threadIdx.x >> 6); }
PMA_DEV uint64_t ballot(bool p) { return (uint64_t)__ballot(p ? 1 : 0); }
PMA_DEV uint32_t shfl(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }
PMA_DEV float shfl_f32(float v, int src) { return __shfl(v, src, 64); }
PMA_DEV uint32_t first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// Scalar values.  One wave executes one update and every decision about it is the same in all 64 lanes — but the compiler only
// knows that of values it can prove uniform (kernel arguments, ballots): anything that descends from `threadIdx.x >> 6` or comes
// out of a shuffle looks per-lane to it, lives in a vector register and branches through EXEC-mask arithmetic.  uni() states
// that a value is the same in every lane (v_readfirstlane: the result is a scalar register); bcast() reads lane `src` (`src` itself
// uniform: v_readlane, a few cycles, where a shuffle is an LDS round trip).  The CPU emulator checks both claims on every call.
PMA_DEV uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
PMA_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
PMA_DEV bool uni(bool b) { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; }
PMA_DEV uint64_t uni(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// The other way round.  The scalar unit issues one instruction per wave every four cycles and is shared by the CU's four SIMDs; a
// SIMD takes a wave64 vector instruction every two, and in the planning kernels it is mostly idle.  vec() states what uni() states
// — the value is the same in every lane — and keeps it in a VECTOR register: the empty asm hides the value's origin from the
// compiler's uniformity analysis, so the arithmetic that descends from it is VALU and its live range costs no scalar register
// (zero instructions; not volatile: an unused one disappears).  The CPU emulator checks the claim like uni()'s.
PMA_DEV uint32_t vec(uint32_t x) {
  asm("" : "+v"(x));
  return x;
}
PMA_DEV uint64_t vec(uint64_t x) {
  asm("" : "+v"(x));
  return x;
}
// Branches on such values: a ballot compared with 0 / with the full mask (all 64 lanes are active) — v_cmp into VCC and ONE scalar
// branch, never an EXEC-mask region.  `if (p)` on a vec() value is a divergent branch to the compiler; `if (wv::any(p))` is not.
PMA_DEV bool any(bool p) { return __ballot(p ? 1 : 0) != 0ull; }
PMA_DEV bool all(bool p) { return __ballot(p ? 1 : 0) == ~0ull; }
// measurement aid (diagnostics builds only: OptArgs::dbg): the uniform value x, as a scalar the compiler knows nothing about — what
// is computed from it a second time is computed, not reused
PMA_DEV uint32_t opaque(uint32_t x) {
  uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
  asm volatile("" : "+s"(s)::"memory");
  return s;
}
// v with lane K replaced by the scalar `x` (v_writelane_b32; this compiler has no builtin for it)
template <int K>
PMA_DEV uint32_t setlane(uint32_t v, uint32_t x) {
  const uint32_t sx = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);  // (the "s" constraint alone does not move a vector value)
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(sx), "n"(K));
  return v;
}
// v with lanes K0 .. K3 replaced by four scalars, as ONE asm block.  Behind every asm statement that writes a vector register the
// compiler pads the next reader of that register with an s_nop (it cannot see that the statement is no sub-dword write); a chain
// of N setlane() calls is N - 1 pads, each a scalar issue slot.  Writes to one register need no pad among themselves (the
// compiler's own spill code issues them back to back).  Two such blocks that build DIFFERENT registers follow each other without
// a pad as well: a record of many words is built as two interleaved halves and merged with one OR (store_plan_header).
template <int K0, int K1, int K2, int K3>
PMA_DEV uint32_t setlanes(uint32_t v, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)x0), s1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)x1);
  const uint32_t s2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)x2), s3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)x3);
  asm("v_writelane_b32 %0, %1, %5\n\tv_writelane_b32 %0, %2, %6\n\tv_writelane_b32 %0, %3, %7\n\tv_writelane_b32 %0, %4, %8"
      : "+v"(v)
      : "s"(s0), "s"(s1), "s"(s2), "s"(s3), "n"(K0), "n"(K1), "n"(K2), "n"(K3));
  return v;
}
// lanes 0 .. N-1 of v as scalars (N x v_readlane_b32; the emulator does it in one rendezvous)
template <int N>
PMA_DEV void lanes(uint32_t v, uint32_t *out) {
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = (uint32_t)__builtin_amdgcn_readlane((int)v, i);
}
PMA_DEV uint32_t bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(src)); }
// sum over the wave (all 64 lanes active), as a scalar.  DPP adds: an inclusive scan inside each row of 16 lanes (row_shr 1, 2,
// 4, 8), the row totals passed on (row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3), the total read off lane 63 —
// six VALU instructions and a v_readlane where six shuffles were six LDS round trips.
PMA_DEV uint32_t reduce_add(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
  return (uint32_t)__builtin_amdgcn_readlane(x, 63);
}
// orders this wave's LDS + global accesses among its own lanes (same CU: L1 is shared)
PMA_DEV void fence() { __threadfence_block(); }
// orders this wave's LDS accesses only (one wave's DS operations execute in order; this is a compiler barrier that
// does not wait for outstanding global loads / stores / atomics)
PMA_DEV void lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
PMA_DEV void block_sync() { __syncthreads(); }
PMA_DEV uint32_t atomic_min_u32(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
PMA_DEV unsigned long long atomic_min_u64(unsigned long long *p, unsigned long long v) { return atomicMin(p, v); }
PMA_DEV uint32_t atomic_add_u32(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
// num_neighbors: the one word of nodes[] that device-wide atomics change
PMA_DEV void atomic_add_nn(uint32_t *p, uint32_t v) { (void)atomicAdd(p, v); }
PMA_DEV unsigned long long atomic_add_u64(unsigned long long *p, unsigned long long v) { return atomicAdd(p, v); }
PMA_DEV uint32_t atomic_max_u32(uint32_t *p, uint32_t v) { return atomicMax(p, v); }
PMA_DEV unsigned long long atomic_max_u64(unsigned long long *p, unsigned long long v) { return atomicMax(p, v); }
PMA_DEV uint32_t atomic_exch_u32(uint32_t *p, uint32_t v) { return atomicExch(p, v); }
PMA_DEV uint32_t atomic_cas_u32(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
// hand-off flags between workgroups (k_rb_inplace): "my loads have RETURNED" — published after a wait for them, polled with
// agent-scope loads (a plain load may be served from a stale line of this XCD's L2 for ever).  No data travels with the
// flag (the poller only WRITES afterwards), so neither side needs a release / acquire: at agent scope those are an L2
// write-back and a cache invalidate per workgroup, which made the kernel 4x slower than the copy it replaces.
// every global load this wave has issued has returned (a workgroup barrier alone does not wait for vmcnt) — and, vmcnt counting
// stores as well on gfx9, every store it has issued has been acknowledged: the drain in front of a word that PUBLISHES data
// stored before it (build_chain_table_publish); the "memory" clobber keeps the compiler from moving a store across it
PMA_DEV void wait_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
PMA_DEV void flag_publish(uint32_t *p, uint32_t v) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
PMA_DEV uint32_t flag_read(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PMA_DEV void flag_acquire() { asm volatile("" ::: "memory"); }
// data that travels between workgroups INSIDE a launch (the position table of k_rb_scatter): written and read at agent scope,
// word by word — a plain store may sit in the writer's XCD L2 and a plain load may be served from a stale line of the
// reader's, and a release / acquire pair at agent scope is an L2 write-back / invalidate per use
PMA_DEV void store_agent_u64(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PMA_DEV unsigned long long load_agent_u64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// which of the 8 XCDs this wave runs on (HW_REG_XCC_ID bits 3:0) — used for affinity only, never for correctness
PMA_DEV uint32_t xcc_id() { return (uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u; }
// a load of data that is read ONCE by the whole launch (the source of a rebalance pass): the non-temporal hint keeps it from
// displacing the lines the pass is still assembling in L2 (whole-array rebalance at 2^24 slots 115 -> 105 us with it on the
// source reads; the neighbour scan, which writes little, got slower with it: 60 -> 65 us — plain loads there)
PMA_DEV uint32_t load_stream_u32(const uint32_t *p) { return __builtin_nontemporal_load(p); }
PMA_DEV void spin_pause() { __builtin_amdgcn_s_sleep(2); }
PMA_DEV int clz64(uint64_t m) { return __clzll((long long)m); }
PMA_DEV int popc64(uint64_t m) { return __popcll((unsigned long long)m); }
PMA_DEV int ctz64(uint64_t m) { return __ffsll((long long)m) - 1; }
PMA_DEV uint32_t block_idx() { return blockIdx.x; }
PMA_DEV uint32_t thread_idx() { return threadIdx.x; }
PMA_DEV uint32_t block_dim() { return blockDim.x; }
PMA_DEV uint32_t grid_dim() { return gridDim.x; }
}  // namespace wv
}  // namespace ppcsr
#endif

namespace ppcsr {
namespace wv {
// high half of the 128-bit product of two 64-bit words (the draws of pma_sample.h)
#if defined(PPCSR_SIM)
inline unsigned long long mulhi64(unsigned long long a, unsigned long long b) { return (unsigned long long)(((unsigned __int128)a * b) >> 64); }
#else
PMA_DEV unsigned long long mulhi64(unsigned long long a, unsigned long long b) { return __umul64hi(a, b); }
#endif
// device-wide OR into a 64-bit word, the old value back (the source bit sets of pma_msbfs.h)
#if defined(PPCSR_SIM)
inline unsigned long long atomic_or_u64(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = o | v; return o; }
#else
PMA_DEV unsigned long long atomic_or_u64(unsigned long long *p, unsigned long long v) { return atomicOr(p, v); }
#endif
// OR into a 64-bit word of LDS, nothing back (ds_or_b64: the forbidden-colour sets of pma_colour.h)
#if defined(PPCSR_SIM)
inline void lds_or_u64(unsigned long long *p, unsigned long long v) { *p |= v; }
#else
PMA_DEV void lds_or_u64(unsigned long long *p, unsigned long long v) { (void)atomicOr(p, v); }
#endif
// the label tables of pma_community.h, in LDS: claim a 32-bit key word (ds_cmpst_rtn_b32: the old value back) and add to the
// 64-bit score beside it, nothing back (ds_add_u64)
#if defined(PPCSR_SIM)
inline uint32_t lds_cas_u32(uint32_t *p, uint32_t expect, uint32_t v) { uint32_t o = *p; if (o == expect) *p = v; return o; }
inline void lds_add_u64(unsigned long long *p, unsigned long long v) { *p += v; }
#else
PMA_DEV uint32_t lds_cas_u32(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
PMA_DEV void lds_add_u64(unsigned long long *p, unsigned long long v) { (void)atomicAdd(p, v); }
#endif
}  // namespace wv
}  // namespace ppcsr
