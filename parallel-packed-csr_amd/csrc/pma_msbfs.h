// Multi-source BFS (ppcsr_multi_bfs): the levels of up to 64 searches advance together, one bit per source in a 64-bit word per
// vertex.  Bit b of a vertex's word belongs to source 64 g + b of group g; a partial last group leaves its upper bits zero
// everywhere.  Per group: seen[v] (the sources that have reached v), front[v] (those that reached it at the current level),
// next[v] (those that reach it at the next: all zero between two levels) and stamp[v], the last level at which v gained a bit
// (kMax: never) — so the UNION frontier of level L is { v : stamp[v] == L }, which is what k_bfs_bits and k_bfs_collect
// (pma_scan.h) turn into the pass's bitmap and the per-vertex launch's list, unchanged.
// A level is an edge step and a vertex step.  The edge step ORs front[u] & ~seen[w] into next[w] for every live edge (u, w):
// as one streaming pass over all arrays (k_ms_edges) when the union frontier is large, one wave per listed vertex
// (k_ms_level) when it is small.  The vertex step (k_ms_vertices) turns next into the new front, marks it seen, stamps it, counts
// the new vertices of each source and, when asked, writes their level.  The host reads the 64 counts once per level.
#pragma once
#include "pma_consumer.h"

namespace ppcsr {

// Counter block of a level (ConsumerScope::Striped<uint32_t, kMsStripeWords, kMsLead>): lead word 0 = length of the next list,
// lead word 1 = a hub was left to the streaming pass; per stripe, words 0..63 = new vertices of source b, word kMsUnion = vertices
// that gained any bit (the size of the next union frontier).
constexpr uint32_t kMsLead = 32, kMsStripeWords = 80, kMsUnion = 64;

// the sources of a group: verts[0, count) are its DISTINCT source vertices, words[i] the bits of the sources that sit on verts[i]
PMA_KERNEL void k_ms_init(const uint32_t *verts, const unsigned long long *words, uint32_t count, uint32_t n, unsigned long long *seen,
                          unsigned long long *front, uint32_t *stamp, uint32_t *levels_g) {
  const uint32_t t = wv::block_idx() * wv::block_dim() + wv::thread_idx();
  if (t >= count) return;
  const uint32_t v = verts[t];
  const unsigned long long w = words[t];
  seen[v] = w;
  front[v] = w;
  stamp[v] = 0;
  if (levels_g)
    for (uint32_t b = 0; b < 64; b++)
      if ((w >> b) & 1ull) levels_g[(uint64_t)b * n + v] = 0;
}

// Edge step for a LARGE union frontier: one streaming pass.  The bitmap "front word non-zero" (k_bfs_bits over stamp[]: n / 8
// bytes, L2-resident) filters the edges before anything 8 bytes wide is gathered; front[src] and seen[dest] are then in flight
// together.  add = front[u] & ~seen[w] are the searches that reach w over this edge for the first time; kLook: a plain look at
// next[w] (it may be stale: then the OR is merely repeated) sheds the ORs that would add nothing, since on a heavy level most
// edges into a new vertex find their bits already there.  The OR's result is unused (no return value is waited for).
template <bool kLook>
PMA_KERNEL void k_ms_edges(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *__restrict__ front_bits,
                           const unsigned long long *__restrict__ front, const unsigned long long *__restrict__ seen, unsigned long long *next) {
  constexpr int kB = 4;
  cp_stream<kB>(tab, P, n, [&](Edge(&e)[kB], uint32_t(&src)[kB], bool(&hit)[kB], int) {
    unsigned long long add[kB], old[kB];  // (phases: cp_stream)
#pragma unroll
    for (int b = 0; b < kB; b++) hit[b] = hit[b] && cp_bit(front_bits, src[b]);
#pragma unroll
    for (int b = 0; b < kB; b++) {
      add[b] = hit[b] ? front[src[b]] : 0ull;
      old[b] = hit[b] ? seen[e[b].dest] : ~0ull;
    }
#pragma unroll
    for (int b = 0; b < kB; b++) {
      add[b] &= ~old[b];
      hit[b] = add[b] != 0ull;
      old[b] = (kLook && hit[b]) ? next[e[b].dest] : 0ull;
    }
#pragma unroll
    for (int b = 0; b < kB; b++)
      if (hit[b] && (add[b] & ~old[b]) != 0ull) (void)wv::atomic_or_u64(&next[e[b].dest], add[b]);
  });
}

// Edge step for a SMALL union frontier: one wave per listed vertex walks its slot range.  A hub (range beyond kBfsWaveSlots) is
// flagged and left, with its front word, to one streaming pass.  The lane whose OR finds next[w] == 0 appends w to the next
// list: every OR adds a bit, so exactly one of them sees zero, and the list holds each vertex that gains a bit once.  The
// vertex step of a listed level visits the NEXT list only, so this wave clears its own vertex's front word when it is done
// with it (no other wave reads it: a vertex is listed once).
PMA_KERNEL void k_ms_level(const ConsumerPart *__restrict__ tab, uint32_t P, uint32_t n, const uint32_t *list, uint32_t nlist,
                           unsigned long long *front, const unsigned long long *seen, unsigned long long *next, uint32_t *nxt, uint32_t *cnt) {
  const int lane = wv::lane();
  cp_walk_vertices(
      tab, P, list, nlist, &cnt[1], lane, [](uint32_t) {},  // (a hub: k_ms_edges)
      [&](uint32_t u, const Edge *items, const Node &nd) {
        const unsigned long long fu = front[u];
        cp_walk_slots(items, nd, lane, [&](uint32_t val, uint32_t dst) {
          bool won = false;
          if (val != 0 && dst < n) {
            const unsigned long long add = fu & ~seen[dst];
            if (add != 0ull && (add & ~next[dst]) != 0ull) won = wv::atomic_or_u64(&next[dst], add) == 0ull;
          }
          cp_append(won, dst, nxt, cnt, lane);
        });
        if (lane == 0) front[u] = 0ull;
      });
}

// Vertex step of level `level`, lane = vertex: over all n vertices (list == nullptr), or over list[0, cnt[0]) behind a listed
// edge step — and not at all when that step left a hub behind (cnt[1]): the host then runs the pass and the step over all n.
// new = next & ~seen becomes the front word, is added to seen, and stamps the vertex with level + 1.  Over all n the old front
// word of a vertex that gains nothing is cleared as well (stamp[v] == level: it was on the frontier).  The counts per source
// by transposition: the ballot of bit b, counted, goes to lane b's register; one add per lane when the grid-stride loop ends,
// into the workgroup's stripe.  With levels_g (64 rows of n words), the lanes that hold bit b store level + 1 to row b: one
// coalesced store per b over all n.
PMA_KERNEL void k_ms_vertices(uint32_t n, const uint32_t *list, const uint32_t *cnt, uint32_t level, uint32_t nbits, unsigned long long *seen,
                              unsigned long long *front, unsigned long long *next, uint32_t *stamp, uint32_t *levels_g, uint32_t *stripes) {
  const int lane = wv::lane();
  uint64_t count = n;
  if (list) {
    if (wv::uni(cnt[1]) != 0u) return;
    count = wv::uni(cnt[0]);
  }
  uint32_t mine = 0, gained = 0;
  const uint64_t stride = (uint64_t)wv::grid_dim() * wv::block_dim();
  for (uint64_t base = (uint64_t)wv::block_idx() * wv::block_dim() + (wv::thread_idx() & ~63u); base < count; base += stride) {
    const uint64_t i = base + (uint64_t)lane;
    uint32_t v = 0;
    unsigned long long nw = 0ull;
    if (i < count) {
      v = list ? list[i] : (uint32_t)i;
      const unsigned long long nx = next[v];
      if (nx != 0ull) {
        const unsigned long long sn = seen[v];
        nw = nx & ~sn;
        next[v] = 0ull;
        if (nw != 0ull) seen[v] = sn | nw;
      }
      if (nw != 0ull) {
        front[v] = nw;
        stamp[v] = level + 1u;
      } else if (list || stamp[v] == level) {
        front[v] = 0ull;
      }
    }
    const uint64_t any = wv::ballot(nw != 0ull);
    if (any == 0) continue;
    gained += (uint32_t)wv::popc64(any);
    for (uint32_t b = 0; b < nbits; b++) {
      const bool has = ((nw >> b) & 1ull) != 0ull;
      const uint64_t m = wv::ballot(has);
      if (m == 0) continue;
      if ((uint32_t)lane == b) mine += (uint32_t)wv::popc64(m);
      if (levels_g && has) levels_g[(uint64_t)b * n + v] = level + 1u;
    }
  }
  uint32_t *const stripe = stripes + (uint64_t)(wv::block_idx() % kBfsStripes) * kMsStripeWords;
  if (mine) wv::atomic_add_u32(stripe + lane, mine);
  if (lane == 0 && gained) wv::atomic_add_u32(stripe + kMsUnion, gained);
}

}  // namespace ppcsr
