/*
 * ppcsr.h — C ABI of the MI355X-native packed-CSR update engine (libppcsr_hip.so).
 *
 * This is the drop-in boundary for the PMA insert/delete + rebalance hot path of
 * domargan/parallel-packed-csr.  The reference has no FFI layer: its boundary is the C++ classes
 * PCSR (src/pcsr/PCSR.h:64-202) and PPPCSR (src/pppcsr/PPPCSR.h:11-60) consumed by the thread
 * pools (src/thread_pool/thread_pool.cpp:44-48, src/thread_pool_pppcsr/thread_pool_pppcsr.cpp:76-82).
 * Every entry point below names the reference member it replaces.  All functions return 0 on success
 * or a ppcsr_status code; none of them exits the process (the reference calls exit() on allocation
 * failure, PCSR.cpp:49-54).  There is NO CPU fallback: without a visible MI355X ppcsr_create fails.
 *
 * Semantics: a batch is applied with the result of the reference driven in stream order on one thread
 * (the only deterministic mode of the reference): identical N/logN/H, identical
 * edges[] bytes, identical nodes[] triples.
 *
 * Preconditions inherited from the reference's sentinel encoding (PCSR.cpp:64): dst != 0xFFFFFFFF and
 * edge value != 0xFFFFFFFF for user edges.
 */
#ifndef PPCSR_H
#define PPCSR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ppcsr_engine *ppcsr_t;   /* one PCSR instance resident on one GPU            */
typedef struct pppcsr_engine *pppcsr_t; /* vertex-range partitioned set of PCSRs (PPPCSR)   */
typedef struct pppcsr_comm *pppcsr_comm_t; /* RCCL communicator + stream + staging of the native exchange */

/* reference edge_t (PCSR.h:30-35) and node_t (PCSR.h:18-23): same field order, same 12-byte layout */
typedef struct { uint32_t src, dest, value; } ppcsr_edge;
typedef struct { uint32_t beginning, end, num_neighbors; } ppcsr_node;
/* one update of a stream: op == 0 deletes (src,dst); op != 0 adds (src,dst) with edge value = op
 * (reference task record src/utility/task.h:10-15; the pools always add with value 1) */
typedef struct { uint32_t src, dst, op; } ppcsr_op;

typedef enum {
  PPCSR_STATUS_OK = 0,
  PPCSR_STATUS_EINVAL = 1,
  PPCSR_STATUS_ENOMEM = 2,
  PPCSR_STATUS_EHIP = 3,         /* HIP runtime error or no GPU */
  PPCSR_STATUS_EUNSUPPORTED = 4, /* no null slot on either side of a slide (PCSR.cpp:378-383), > 2^31 slots */
  PPCSR_STATUS_EINTERNAL = 5,
  PPCSR_STATUS_ERANGE = 6        /* output buffer too small; *count holds the needed size */
} ppcsr_status;

typedef struct {
  uint64_t N, n;
  int32_t logN, H;
  uint64_t rounds, committed, planned, exclusive_ops, round_syncs;
  uint64_t redistribute_calls, redistribute_slots; /* what the reference's redistribute() would move */
  uint64_t double_calls, half_calls, big_redistributes, rollbacks;
  uint64_t not_found, duplicates, noops, slide_slots;
  uint64_t ops_applied;
  double last_batch_ms;     /* device-only time of the last batch (ops already in HBM)  */
  double last_batch_h2d_ms; /* H2D time of the op array when it came from a host buffer */
  /* option "profile"=1: HIP-event time spent in each round kernel, measured on the engine's own stream */
  double prof_plan_ms, prof_check_ms, prof_apply_ms, prof_compact_ms;
  uint64_t prof_launches; /* launches of each of the three round kernels */
  uint64_t wasted_rounds; /* rounds of speculative epochs that were rolled back (not counted in `rounds`) */
  uint64_t narrow_lost;   /* how often that add_node path was taken */
  uint64_t narrow;        /* 1: regular structure (parallel rounds); 0: add_node after a doubling has left overlapping vertex ranges
                             (PCSR.cpp:533-540, 681-703): updates run one per round until a re-check finds the ranges sane again */
} ppcsr_stats_t;

/* PCSR::PCSR(init_n, src_n, lock_search, domain)  — PCSR.cpp:775-838; `device` replaces the NUMA domain */
int ppcsr_create(uint32_t init_n, uint32_t src_n, int lock_search, int device, ppcsr_t *out);
/* PCSR::~PCSR — PCSR.cpp:840-851 */
int ppcsr_destroy(ppcsr_t h);
/* PCSR::add_edge — PCSR.cpp:706, 1374-1445 */
int ppcsr_add_edge(ppcsr_t h, uint32_t src, uint32_t dst, uint32_t value);
/* PCSR::remove_edge — PCSR.cpp:709-773 */
int ppcsr_remove_edge(ppcsr_t h, uint32_t src, uint32_t dst);
/* PCSR::add_node — PCSR.cpp:681-703 */
int ppcsr_add_node(ppcsr_t h);
/* the worker loop of ThreadPool::execute (thread_pool.cpp:28-61): everything submitted before start() is
 * one batch; applied with sequential stream-order semantics.  Host buffer variant copies H2D first. */
int ppcsr_apply_batch(ppcsr_t h, const ppcsr_op *ops, uint64_t n);
/* same, ops already resident in this GPU's HBM (e.g. the output of the all-to-all exchange) */
int ppcsr_apply_batch_device(ppcsr_t h, const ppcsr_op *d_ops, uint64_t n);
/* PCSR::edge_exists — PCSR.cpp:860-869 */
int ppcsr_edge_exists(ppcsr_t h, uint32_t src, uint32_t dst, int *exists);
/* PCSR::get_n — PCSR.cpp:100 */
int ppcsr_get_n(ppcsr_t h, uint64_t *n);
/* PCSR::getNode — PCSR.h:118-124 */
int ppcsr_get_node(ppcsr_t h, uint32_t v, ppcsr_node *out);
/* edges.N / edges.logN / edges.H — PCSR.h:37-44 */
int ppcsr_geometry(ppcsr_t h, uint64_t *N, int *logN, int *H);
/* PCSR::get_neighbourhood — PCSR.cpp:901-912 (out may be NULL to query the count) */
int ppcsr_get_neighbourhood(ppcsr_t h, int src, int *out, uint64_t cap, uint64_t *count);
/* PCSR::read_neighbourhood — PCSR.cpp:892-899 */
int ppcsr_read_neighbourhood(ppcsr_t h, int src);
/* bulk neighbour scan: get_neighbourhood for every vertex at once as CSR (row_offsets[n+1], dests[total]) */
int ppcsr_scan_all(ppcsr_t h, uint64_t *row_offsets, int *dests, uint64_t cap, uint64_t *total);
/* Batched reads.  Synchronous on the engine's stream (they see every batch applied before them); they write nothing to the
 * graph (state, stats, dirty tags and the snapshot are unchanged).  The host-buffer forms stage through bounded buffers.
 * lookup_edges — PCSR::edge_exists (PCSR.cpp:860-869) for n pairs at once, with the value: values[i] = value of edge
 *   (src[i], dst[i]) exactly when ppcsr_edge_exists would report it (the same search, the same slot), else PPCSR_NO_EDGE;
 *   src[i] >= n gives PPCSR_NO_EDGE (not EINVAL). */
#define PPCSR_NO_EDGE 0xFFFFFFFFu /* cannot be a stored value: see the sentinel precondition at the top */
int ppcsr_lookup_edges(ppcsr_t h, const uint32_t *src, const uint32_t *dst, uint64_t n, uint32_t *values);
int ppcsr_lookup_edges_device(ppcsr_t h, const uint32_t *d_src, const uint32_t *d_dst, uint64_t n, uint32_t *d_values);
/* gather_neighbourhoods — PCSR::get_neighbourhood (PCSR.cpp:901-912) for k vertices at once, as CSR in query order: row i
 *   holds the live slots of (beginning, end) of vertices[i] in slot order, dests[] with the edge value beside each in values[];
 *   vertices >= n give empty rows, repeats are allowed.  row_offsets[k + 1] (may be NULL); dests and values may be NULL (both
 *   NULL: *total only); at most cap edges are written and ERANGE is returned when cap < *total (as ppcsr_scan_all). */
int ppcsr_gather_neighbourhoods(ppcsr_t h, const uint32_t *vertices, uint64_t k, uint64_t *row_offsets, int *dests, uint32_t *values,
                                uint64_t cap, uint64_t *total);
/* the same, every array in this GPU's HBM (total: host) */
int ppcsr_gather_neighbourhoods_device(ppcsr_t h, const uint32_t *d_vertices, uint64_t k, uint64_t *d_row_offsets, int *d_dests,
                                       uint32_t *d_values, uint64_t cap, uint64_t *total);
/* Bulk build of an EMPTY graph from a list of adds — an explicit NON-parity fast path: the reference can
 * only build a graph by single inserts (src/main.cpp:160-189 feeds add_edge one line at a time) and the array layout that
 * produces depends on the insertion history.  This call yields a valid packed-memory array with the same neighbourhoods,
 * the same num_neighbors (every add counts, duplicates keep the last value) and the same invariants, but NOT the slot
 * layout of the one-by-one build; updates applied afterwards go through the ordinary (sequentially exact) path.  Entries
 * with op == 0 or src >= n are ignored, as add_edge ignores them.  Fails with EINVAL if the graph already holds edges.
 * The layout is determined (tests/bulk_model.py holds it slot by slot): with E surviving edges the array keeps its size N or
 * doubles it until (n + E + 1) / N < 3/4, the root's upper density — the root still accepts one more insert; it never
 * shrinks —, and the sequence sentinel 0, edges of vertex 0 ascending, sentinel 1, ... takes the slots redistribute()
 * (PCSR.cpp:207-247) gives n + E elements in the window of the whole array. */
int ppcsr_bulk_build(ppcsr_t h, const ppcsr_op *adds, uint64_t n, double *device_ms);
/* Graph-algorithm consumers run on the device over the gapped array.
 * bfs — src/utility/bfs.h:15-36: levels[v] = BFS level of v from `start`, UINT32_MAX when unreachable (levels: n entries).
 * pagerank — src/utility/pagerank.h:15-29: one push step, out[d] = sum over edges (s, d), in ascending s, of
 *   node_values[s] / num_neighbors(s) in fp32 — added in the reference's order, so the result is bit-identical to the
 *   reference template's (node_values, out: n entries).  device_ms (may be NULL): device time of the traversal. */
int ppcsr_bfs(ppcsr_t h, uint32_t start, uint32_t *levels, double *device_ms);
int ppcsr_pagerank(ppcsr_t h, const float *node_values, float *out, double *device_ms);
/* Two consumers that use the edge values / the edges as undirected pairs, over the edge set ppcsr_bfs walks (live slots of
 * every vertex's (beginning, end), slot N - 1 excluded, destinations >= n skipped).  The weight of an edge is its stored
 * value (a duplicate add has overwritten it: the last add wins).
 * sssp — dist[v] = the smallest sum of values over directed paths from `start` to v; dist[start] = 0; PPCSR_NO_PATH when
 *   there is none (dist: n entries).  Distances are 64-bit and cannot overflow: a value lies in [1, 2^32 - 2] (0 is the null
 *   slot, 0xFFFFFFFF the sentinel precondition) and a simple path has at most n - 1 <= 2^32 - 1 edges, so a distance is
 *   below (2^32 - 1)(2^32 - 2) < 2^64 - 1 = PPCSR_NO_PATH.  Nothing saturates or is checked at run time.
 * components — weakly connected components: labels[v] = the smallest vertex id of v's component, edges taken as
 *   undirected; an isolated vertex labels itself (labels: n entries).  The number of components is the count of
 *   labels[v] == v.
 * Both results are unique.  Same contract as bfs: synchronous, write nothing to the graph, device_ms may be NULL.
 * EINVAL: null handle or output, start >= n. */
#define PPCSR_NO_PATH 0xFFFFFFFFFFFFFFFFull
int ppcsr_sssp(ppcsr_t h, uint32_t start, uint64_t *dist, double *device_ms);
int ppcsr_components(ppcsr_t h, uint32_t *labels, double *device_ms);
/* Shortest-path counts and betweenness centrality (Brandes 2001), over exactly the edge set ppcsr_bfs walks: live non-sentinel
 * slots, slot N - 1 excluded, local src < n, destinations >= n skipped.  The edges are DIRECTED and their values play no part.
 * path_counts — the forward phase alone.  levels[v] is what ppcsr_bfs gives (UINT32_MAX when unreachable); sigma[v] is the
 *   NUMBER of shortest (fewest-edges) directed paths from `start` to v, in fp64: sigma[start] = 1, 0 when unreachable
 *   (levels, sigma: n entries; either may be NULL, not both).  Every addition adds integers, so sigma is exact and does not
 *   depend on the order of the additions while every count is below 2^53; beyond that each sum is rounded to fp64 in an
 *   unspecified order.  Counts are fp64 and not 64-bit integers on purpose: a chain of 70 two-wide diamonds already has 2^70
 *   paths.  Counts beyond the fp64 range (above about 1.8e308) are NOT guarded: they become infinite, and betweenness from
 *   such a source is then NaN.
 * betweenness — for every source s, with level and sigma from s,
 *     delta_s(v) = sum over stored (v, w) with level(w) = level(v) + 1 of (sigma(v) / sigma(w)) * (1 + delta_s(w))
 *     bc[v]      = sum over i < k with sources[i] != v of delta_{sources[i]}(v)                        (bc: n entries)
 *   Endpoints are excluded, nothing is halved and nothing is normalised.  A repeated source counts once each time; k == 0
 *   gives all zeros; sources = 0 .. n - 1 gives exact betweenness.  For a graph stored symmetrically this is twice the
 *   undirected value; it equals networkx betweenness_centrality(DiGraph, normalized=False).  The arithmetic is fp64 as
 *   written — one division, one addition and one multiplication per edge of the shortest-path DAG, unfused — and the sums may
 *   be taken in any order, so the last bits can differ from run to run.
 *   Accuracy: all terms are non-negative, so a sum of m terms in any order or tree carries a relative error of at most
 *   (m - 1) u, u = 2^-53, and a term adds three roundings.  delta of a vertex therefore carries at most dmax + 2 roundings more
 *   than the deepest delta it is built from, where dmax is the largest out-degree; with D the deepest BFS level over the
 *   sources that is D (dmax + 2) u, and bc adds at most k such values: to first order, while sigma is exact,
 *     |bc[v] - exact| <= (D (dmax + 2) + k) * 2^-53 * exact.
 * Same contract as every consumer: synchronous on the engine's stream, sees every batch applied before it, writes nothing to
 * the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL.  The calls intersect nothing, so — as
 * bfs and components — they also answer in the sequential regime (stats.narrow == 0).  EINVAL: null handle; levels and sigma
 * both NULL; bc NULL; sources NULL with k > 0; any sources[i] >= n (checked before the first launch: nothing has run);
 * start >= n. */
int ppcsr_path_counts(ppcsr_t h, uint32_t start, uint32_t *levels, double *sigma, double *device_ms);
int ppcsr_betweenness(ppcsr_t h, const uint32_t *sources, uint64_t k, double *bc, double *device_ms);
/* Core numbers (the k-core decomposition), over the edge set ppcsr_components hooks (live non-sentinel slots, slot N - 1
 * excluded, destinations >= n skipped) and in the undirected graph G ppcsr_triangles counts in, the upper orientation: {a, b},
 * a < b < n, is an edge exactly when the pair (a, b) is stored; stored pairs with src > dst and self-loops play no part — so
 * tri[] and core[] speak about the same graph.  This is the exact answer for a graph stored symmetrically and for one stored
 * as its upper triangle; for any other state it is still one well-defined result.
 * kcore — core[v] = the largest k such that v lies in a subgraph of G whose every vertex has at least k neighbours inside it
 *   (n entries, may be NULL); an isolated vertex has core 0.  *kmax = the largest core number, the degeneracy of G; 0 for
 *   n = 0 or no edges (may be NULL, not both).
 * Both results are unique.  Same contract as components: synchronous on the engine's stream, sees every batch applied before
 * it, writes nothing to the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL.  The call does not
 * intersect sorted ranges, so — as components, and unlike triangles — it also answers in the sequential regime
 * (stats.narrow == 0).  EINVAL: null handle, core and kmax both NULL. */
int ppcsr_kcore(ppcsr_t h, uint32_t *core, uint32_t *kmax, double *device_ms);
/* Greedy vertex colouring and the maximal independent set (MIS), in the undirected graph G that ppcsr_triangles counts in and
 * ppcsr_kcore peels: the edge set ppcsr_components hooks (live non-sentinel slots, slot N - 1 excluded, local src < n,
 * destinations >= n skipped), upper orientation — {a, b}, a < b < n, is an edge exactly when the pair (a, b) is stored; self-loops
 * and stored pairs with src > dst play no part.  A pair is stored at most once, so G is simple.
 * Vertex order.  Every vertex has a 64-bit key; u PRECEDES w iff key(u) > key(w), or the keys are equal and u < w.  With
 * draw(v) = the counter-based draw (seed, v, 0) of ppcsr_sample_neighbours (splitmix64 three times), v the vertex id:
 *   PPCSR_ORDER_RANDOM  key = draw(v)                                   random priorities
 *   PPCSR_ORDER_DEGREE  key = (deg_G(v) << 32) | (draw(v) >> 32)        largest degree first, ties at random
 *   PPCSR_ORDER_ID      key = 0 (the seed is ignored)                   ascending id: sequential first-fit
 * colouring — colour[v] = the smallest non-negative integer that no neighbour w of v that precedes v carries (n entries, may be
 *   NULL): sequential greedy colouring in the order, computed as Jones and Plassmann do.  An isolated vertex gets colour 0;
 *   colour[v] <= deg_G(v).  *ncolours = 1 + the largest colour, 0 for n = 0 (may be NULL, not both).
 * mis — in_set[v] = 1 iff no neighbour w of v that precedes v has in_set[w] = 1, else 0 (n bytes, may be NULL): the
 *   lexicographically first maximal independent set in the order.  *size = the number of members (may be NULL, not both).
 * Everything returned is unique, and for one order and seed in_set[v] == (colour[v] == 0).
 * Same contract as every consumer: synchronous on the engine's stream, sees every batch applied before it, writes nothing to
 * the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL, every refusal is made before the first
 * launch.  Neither call intersects sorted ranges, so — as kcore — both also answer in the sequential regime
 * (stats.narrow == 0).  EINVAL: null handle, both outputs NULL, an order other than the three above.  ENOMEM: a device
 * allocation of the call failed (nothing written).
 * Cost.  Let level(v) = 0 for a vertex without a preceding neighbour, else 1 + the largest level of one.  The colouring exports
 * G as ppcsr_kcore does and then takes one launch and one host read per level; the MIS streams the arrays in place, at most
 * two passes per level.  Random orders give few levels; PPCSR_ORDER_ID on a path of L vertices stored in id order is L levels,
 * as the chains ppcsr_scc warns about.  Both loops are bounded — n rounds for the colouring, 2 n + 1 for the MIS — and report
 * an error past that instead of spinning. */
#define PPCSR_ORDER_RANDOM 0u
#define PPCSR_ORDER_DEGREE 1u
#define PPCSR_ORDER_ID 2u
int ppcsr_colouring(ppcsr_t h, uint32_t order, uint64_t seed, uint32_t *colour, uint32_t *ncolours, double *device_ms);
int ppcsr_mis(ppcsr_t h, uint32_t order, uint64_t seed, uint8_t *in_set, uint64_t *size, double *device_ms);
/* Debugging: what the last colouring / mis call on this engine did — for a pppcsr_* call the engine that ran it, the first
 * partition's (pppcsr_partition).  Kept on the host from the reads the loops make anyway and always on; all zeros before the
 * first call.  Rounds, the widest frontier, members and undecided after round 1 are functions of the graph and the order.
 * colouring:
 *   out[0] rounds = levels of the order                     out[1] the widest frontier
 *   out[2] frontier vertices handed to the long-list kernel (lists beyond 4096 entries)
 *   out[3] adjacency entries, 2 |E(G)|                      out[4] colours
 *   out[5] window passes of the long-list kernel beyond each vertex's first ("colour_window")
 *   out[6] launches                                         out[7] host reads
 * mis:
 *   out[0] rounds                                           out[1] streaming passes of the rounds
 *   out[2] members after round 1 (the local maxima)         out[3] undecided after round 1
 *   out[4] size                                             out[5] degree passes (1 for PPCSR_ORDER_DEGREE, else 0)
 *   out[6] launches                                         out[7] host reads
 * EINVAL: null handle or out. */
int ppcsr_debug_colouring_counters(ppcsr_t h, uint64_t out[8]);
int ppcsr_debug_mis_counters(ppcsr_t h, uint64_t out[8]);
/* Label-propagation communities and modularity, in the same undirected graph G (the paragraph above ppcsr_colouring): {a, b},
 * a < b < n, is an edge iff the pair (a, b) is stored.  The WEIGHT of {a, b} is that stored pair's value with
 * PPCSR_COMMUNITY_WEIGHTED in flags and 1 without it (a stored value lies in [1, 2^32 - 2]); pairs with src > dst, self-loops
 * and destinations >= n play no part.
 * Schedule.  colour[] is the answer of ppcsr_colouring(order, seed).  CLASS c is the set of vertices with colour c and at least
 *   one neighbour.  A SWEEP runs the classes 0, 1, ..., C - 1 in turn; a STEP handles one class.
 * Step.  For every v of the class, score(l) = the sum of the weights of v's edges to neighbours that carry label l, a 64-bit
 *   sum.  M = the largest score.  v keeps its label if its own label scores M; otherwise it takes the SMALLEST label that
 *   scores M.  A class is an independent set, so a step reads no label that it writes: the result is that of the sequential
 *   sweep in (colour, id) order and is unique for one order and seed.
 * Start and end.  Labels start at init[v] (n entries; an entry >= n is EINVAL and nothing is written); init == NULL means
 *   label[v] = v.  Passing the previous answer as init is the warm start after a batch of updates.  The call ends after the
 *   first sweep that changes no label, or after max_sweeps sweeps (0: until convergence).  A vertex without a neighbour keeps
 *   its label.
 * Outputs.  labels[v] (n entries, may be NULL): the raw labels, vertex ids.  *ncommunities: the number of distinct values in
 *   labels.  *sweeps: the sweeps run, the last, changeless one included (0 only for n = 0).  Each may be NULL, not all three.
 * Termination.  A vertex changes its label only to one of strictly larger score, and the members of a class are not adjacent,
 *   so no neighbour moves in the same step: every change raises the total weight of the edges whose two ends agree by at
 *   least 1, and that total is bounded by W(G), the weight of all edges.  So at most W(G) changes happen and a call without
 *   max_sweeps ends after at most W(G) + 1 sweeps (checked, not trusted: past it an error).  This is the semi-synchronous
 *   scheme of Cordasco and Gargano (2010) on the label propagation of Raghavan, Albert and Kumara (2007); a fully synchronous
 *   update can flip for ever on a bipartite graph, this one cannot.
 * Modularity (Newman and Girvan 2004) of ANY labels[] (n entries, each < n, else EINVAL):
 *   out[0] = 2 W(G)                                          out[1] = sum over communities c of 2 in_c: the weight inside, doubled
 *   out[2], out[3] = the low and the high word of S = sum over c of tot_c^2, tot_c = the sum of the weighted degrees of c
 *   *q = out[1] / out[0] - S / out[0]^2, formed in doubles on the host from these exact integers; 0 when out[0] is 0.
 *   out and q may each be NULL, not both.  The sums are 64-bit: W(G) < 2^63 is the caller's to keep.
 * Same contract as every consumer: synchronous, sees every batch applied before it, writes nothing to the graph, device_ms may
 * be NULL, answers in the sequential regime (stats.narrow == 0).  EINVAL, refused before the device is selected: null handle,
 * an unknown order, flag bits other than PPCSR_COMMUNITY_WEIGHTED, a bad init / labels entry, NULL labels for modularity, all
 * outputs NULL.  ENOMEM: a device allocation of the call failed (nothing written).
 * Cost.  ppcsr_colouring's, then per sweep at most three launches per class (lists of at most 64 entries, of at most 512, and
 * longer ones: csrc/pma_community.h) and one host read. */
#define PPCSR_COMMUNITY_WEIGHTED 1u
int ppcsr_label_propagation(ppcsr_t h, uint32_t order, uint64_t seed, uint32_t flags, uint32_t max_sweeps, const uint32_t *init, uint32_t *labels,
                            uint64_t *ncommunities, uint32_t *sweeps, double *device_ms);
int ppcsr_modularity(ppcsr_t h, const uint32_t *labels, uint32_t flags, uint64_t out[4], double *q, double *device_ms);
/* Debugging: what the last label_propagation call on this engine did (for a pppcsr_ call: the first partition's engine).
 *   out[0] sweeps                                            out[1] classes that are not empty
 *   out[2] label changes in all                              out[3] label changes of the last sweep (0 iff converged)
 *   out[4] communities                                       out[5] vertices with a list beyond 512 entries (a workgroup each)
 *   out[6] hash passes of those beyond each one's first, summed over the sweeps ("lp_table_slots"; depends on the scheme)
 *   out[7] launches
 * [0] - [5] are functions of the graph, the order, the flags and init.  EINVAL: null handle or out. */
int ppcsr_debug_community_counters(ppcsr_t h, uint64_t out[8]);
/* Strongly connected components, over exactly the edge set ppcsr_bfs walks (live non-sentinel slots, slot N - 1 excluded, local
 * src < n, destinations >= n skipped), taken as DIRECTED; the edge values play no part.  A self-loop is an ordinary stored edge
 * that changes nothing: a vertex whose only cycle is its self-loop is an SCC of one vertex.
 * scc — labels[v] = the smallest vertex id of v's SCC (n entries, may be NULL): the convention of ppcsr_components, so the two
 *   label arrays compare directly and the SCC labels refine the WCC labels.  *count = the number of SCCs = the number of v with
 *   labels[v] == v; 0 for n = 0 (may be NULL, not both).
 * Both results are unique.  Same contract as components: synchronous on the engine's stream, sees every batch applied before
 * it, writes nothing to the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL.  The call intersects
 * nothing and takes every edge's source from the item itself, so — as components and kcore — it also answers in the
 * sequential regime (stats.narrow == 0).  The number of passes over the array grows with the longest chain of the graph (a
 * directed path of L vertices: about L / 2 trim sweeps; a cycle of L vertices: up to L passes).  EINVAL: null handle, labels
 * and count both NULL. */
int ppcsr_scc(ppcsr_t h, uint32_t *labels, uint64_t *count, double *device_ms);
/* Debugging: what the last scc call on this engine did — for a pppcsr_scc call the engine that ran it, the first partition's
 * (pppcsr_partition).  Kept on the host and always on: no launch, copy or synchronisation is added for it; all zeros before
 * the first call.  The phases cover for each other (whatever trimming or the pivot leave, colouring still labels), so label
 * parity alone cannot show that a phase works; these can.
 *   out[0] vertices labelled by trimming            out[1] trim sweeps
 *   out[2] the pivot's global id (UINT64_MAX when the forward-backward phase did not run)
 *   out[3] vertices labelled by the forward-backward phase
 *   out[4] colouring rounds                         out[5] vertices labelled by colouring
 *   out[6] streaming passes over the arrays, all phases together
 *   out[7] host reads (stream synchronisations inside the timed region)
 * EINVAL: null handle or out. */
int ppcsr_debug_scc_counters(ppcsr_t h, uint64_t out[8]);
/* Minimum spanning forest over the edge VALUES, over the edge set ppcsr_components hooks (live non-sentinel slots, slot N - 1
 * excluded, local src < n, destinations >= n skipped; self-loops play no part).  Every stored pair (a, b), a != b, with value w
 * is one edge {a, b} of weight w of an undirected MULTIGRAPH: if (a, b) and (b, a) are both stored they are two parallel edges,
 * whose weights may differ.  The weight is the stored value, in [1, 2^32 - 2]; a duplicate add has overwritten it (last add wins).
 * The key of an edge is (w, lo, hi), lo = min(a, b), hi = max(a, b), compared lexicographically; two edges with the same key are
 * the two directions of one pair stored with equal values and count as one.  Under this strict order the minimum spanning
 * forest is UNIQUE as a set of keys, and so is everything returned.
 * msf — edges: the forest's edges as (src = lo, dest = hi, value = w), ascending by (lo, hi); at most cap are written and ERANGE
 *   is returned when edges != NULL and cap < *count (as ppcsr_scan_all), the other outputs still delivered (may be NULL).
 *   *count = the number of forest edges = n - (number of components) (may be NULL).  *weight = the sum of the forest's weights,
 *   64-bit: (n - 1)(2^32 - 2) < 2^64, nothing saturates (may be NULL).  labels[v] = the smallest vertex id of v's tree, n
 *   entries: exactly what ppcsr_components returns (may be NULL).  Not all four may be NULL.  n = 0 or no edges: count = 0,
 *   weight = 0.
 * Same contract as components / kcore / scc: synchronous on the engine's stream, sees every batch applied before it, writes
 * nothing to the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL.  The call intersects nothing and
 * takes every edge's source from the item itself, so it also answers in the sequential regime (stats.narrow == 0).  Boruvka
 * rounds over the arrays in place: at most floor(log2 n) + 1 rounds of two streaming passes.  EINVAL: null handle, all four
 * outputs NULL. */
int ppcsr_msf(ppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint64_t *weight, uint32_t *labels, double *device_ms);
/* Debugging: what the last msf call on this engine did — for a pppcsr_msf call the engine that ran it, the first partition's
 * (pppcsr_partition).  Kept on the host from the reads the loop makes anyway and always on; all zeros before the first call.
 *   out[0] rounds: a round is one search for every component's lightest cut edge; the last round finds none
 *   out[1] streaming passes over the arrays: 2 * out[0] - 1 for n > 0 (the last round makes the first of its two passes only)
 *   out[2] pointer-jump launches, all rounds together          out[3] the most pointer-jump launches in one round
 *   out[4] components hooked in the first round                out[5] forest edges = the sum of hooks over all rounds
 *   out[6] components at the end
 *   out[7] host reads (stream synchronisations inside the timed region)
 * EINVAL: null handle or out. */
int ppcsr_debug_msf_counters(ppcsr_t h, uint64_t out[8]);
/* Edge support and truss numbers (the k-truss decomposition), in the undirected graph G that ppcsr_triangles counts in and
 * ppcsr_kcore peels: live non-sentinel slots only, slot N - 1 excluded, local src < n, dest < n; {a, b}, a < b < n, is an edge
 * exactly when the pair (a, b) is stored; self-loops and stored pairs with src > dst play no part.  A pair is stored at most
 * once, so G is simple.
 *   support(e), e = {a, b}: the number of vertices c with {a, c} and {b, c} in G.  The supports sum to 3 x the total of
 *     ppcsr_triangles, and those of the edges at v to 2 x tri[v].
 *   truss(e): the largest k such that e lies in a subgraph of G whose every edge is in at least k - 2 triangles inside that
 *     subgraph (the convention of networkx k_truss and of cuGraph): an edge in no triangle has truss 2, every edge of a clique
 *     on m vertices has truss m.
 * edges — every edge of G as (src = a, dest = b, value = support or truss number), ascending by (a, b); at most cap are written
 *   and ERANGE is returned when edges != NULL and cap < *count (as ppcsr_msf), the other outputs still delivered (may be NULL).
 * *count = |E(G)| (may be NULL; a call that asks for nothing else is a cheap size query).  *total = the number of triangles (may
 * be NULL).  *tmax = the largest truss number, 0 when G has no edge (may be NULL).  vtruss[v], n entries: the largest truss number
 * of an edge at v, 0 for a vertex without an edge in G (may be NULL); vtruss[v] <= core[v] + 1 and tmax <= kmax + 1 against
 * ppcsr_kcore.  Not all outputs may be NULL.  Everything returned is unique.
 * Same contract as every consumer: synchronous on the engine's stream, sees every batch applied before it, writes nothing to
 * the graph (state, stats, dirty tags and snapshot unchanged), device_ms may be NULL, every refusal is made before the first
 * launch.  EINVAL: null handle, all outputs NULL.  ENOMEM: a device allocation of the call failed (nothing written).
 * EUNSUPPORTED, with the reason in ppcsr_last_error: the sequential regime (stats.narrow == 0) — sorted ranges are searched, as
 * ppcsr_triangles refuses it; a table of 2^32 slots or more (slots rounded up to 64 per array) — an edge is named by a 32-bit
 * slot id.  Extra device memory: three words per slot, five per vertex, five per edge of G. */
int ppcsr_edge_support(ppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint64_t *total, double *device_ms);
int ppcsr_ktruss(ppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint32_t *tmax, uint32_t *vtruss, double *device_ms);
/* Debugging: what the last edge_support / ktruss call on this engine did — for a pppcsr_* call the engine that ran it, the first
 * partition's (pppcsr_partition).  Kept on the host from the reads the loop makes anyway and always on; all zeros before the
 * first call.  The peel is synchronous in sub-rounds, so out[2] .. out[5] are functions of the graph (0 after edge_support).
 *   out[0] |E(G)|
 *   out[1] triangles (0 after a size query)
 *   out[2] levels run: distinct truss numbers
 *   out[3] sub-rounds, all levels together
 *   out[4] most sub-rounds in one level
 *   out[5] widest frontier (edges)
 *   out[6] frontier edges handed to the long-range kernel (a walked side beyond 1024 positions)
 *   out[7] host reads (stream synchronisations inside the timed region)
 * EINVAL: null handle or out. */
int ppcsr_debug_ktruss_counters(ppcsr_t h, uint64_t out[8]);
/* Two consumers that intersect two neighbourhoods, over the same edge set (live slots of every vertex's (beginning, end), slot
 * N - 1 excluded, destinations >= n skipped; a (src, dst) pair is stored at most once).  A vertex's live slots lie in
 * ascending destination order, so the neighbourhoods are intersected in place: no export, no sort.
 * triangles — counted in the upper orientation: the undirected graph G has the edge {a, b}, a < b, exactly when the pair
 *   (a, b) is stored; stored pairs with src > dst and self-loops play no part.  A triangle is a triple a < b < c with (a, b),
 *   (a, c) and (b, c) all stored.  tri[v] = triangles that contain v (n entries, 64-bit: a hub's count can pass 2^32; may be
 *   NULL), *total = triangles = sum(tri) / 3 (may be NULL, not both).  This is the exact triangle count of a graph stored
 *   symmetrically (both directions inserted) and of a graph stored as its upper triangle; for any other state it is still
 *   one well-defined number.
 * common_neighbours — counts[i] = |{c < n : (a[i], c) stored and (b[i], c) stored}| for k pairs: directed out-neighbourhoods,
 *   no orientation filter, a self-loop is an ordinary stored edge.  a[i] >= n or b[i] >= n gives 0 (not EINVAL); a[i] == b[i]
 *   gives the number of stored destinations < n; repeats are allowed.  The host form stages the pairs through bounded buffers
 *   ("query_lookup_stage" pairs per round trip); the _device form takes every array in this GPU's HBM.
 * Both results are unique.  Same contract as bfs: synchronous, write nothing to the graph, device_ms may be NULL.
 * EINVAL: null handle, tri and total both NULL, a / b / counts NULL with k > 0.  EUNSUPPORTED: the structure is in the
 * sequential regime (stats.narrow == 0: add_node after a doubling, vertex ranges may be unsorted or overlapping until the
 * next range re-check) — sorted ranges cannot be intersected then, and no number is returned; ppcsr_last_error says so. */
int ppcsr_triangles(ppcsr_t h, uint64_t *tri, uint64_t *total, double *device_ms);
int ppcsr_common_neighbours(ppcsr_t h, const uint32_t *a, const uint32_t *b, uint64_t k, uint32_t *counts, double *device_ms);
int ppcsr_common_neighbours_device(ppcsr_t h, const uint32_t *d_a, const uint32_t *d_b, uint64_t k, uint32_t *d_counts, double *device_ms);
/* Neighbour sampling, random walks and live degrees, on the graph as it stands (no export).
 * Neighbour list — L(v) of a vertex v < n: the live slots of v's range (beginning, end) in slot order, with the consumers' edge
 *   set: the slot is non-null and non-sentinel, it is not slot N - 1, and its destination is < n.  Self-loops count.
 * Measure — every entry of L(v) has a measure: 1 (uniform), or the edge value when flags bit 0 (PPCSR_SAMPLE_WEIGHTED) is set.
 *   W(v) is the sum of the measures, in 64 bits.
 * Draw — a function of (seed, i, j) alone, i the query / walker index, j the draw / step index, all arithmetic mod 2^64:
 *     sm(z): z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *            return z ^ (z >> 31)
 *     x = sm(sm(sm(seed) + i) + j);   r = (x * W(v)) >> 64  (the high half of the 128-bit product)
 *     pick = the first entry of L(v) whose inclusive cumulative measure exceeds r
 *   so the result depends on nothing else: not on the launch geometry, not on where the gaps lie, not on the partitioning (in the
 *   regular regime a PCSR and a PPPCSR that hold the same edges answer word for word alike).  Draws are with replacement.
 * PPCSR_NO_VERTEX is returned for a vertex >= n, for an empty L(v), and in a walk for every position after either; the value
 *   beside it is 0 (never a stored value).
 * sample_neighbours — dests[i * fanout + j] = the destination picked by draw (seed, i, j) from L(vertices[i]), values[...] that
 *   edge's value (values may be NULL).  Repeated vertices are separate queries (i differs).
 * random_walks — out[i * (length + 1)] = starts[i] (PPCSR_NO_VERTEX when >= n), out[i * (length + 1) + t + 1] = the pick of
 *   draw (seed, i, t) from L(out[i * (length + 1) + t]).
 * degrees — deg[v] = |L(v)| (uint32) and wsum[v] = the sum of the values of L(v) (uint64), n entries each, either may be NULL:
 *   one streaming pass that takes every edge's source from the item itself, so it also answers in the sequential regime.
 * The host forms take host pointers; the _device forms take every array in this GPU's HBM.  Same contract as bfs: synchronous,
 * nothing of the graph is written (state, stats, snapshot unchanged), device_ms may be NULL.  Every refusal is made before the
 * first launch.  EINVAL: null handle, vertices / starts or dests / out NULL with k > 0, fanout == 0, length == 0, unknown flags
 * bits, deg and wsum both NULL; k == 0 succeeds and writes nothing.  EUNSUPPORTED (sample_neighbours, random_walks): the
 * structure is in the sequential regime (stats.narrow == 0), where vertex ranges cannot be trusted. */
#define PPCSR_NO_VERTEX 0xFFFFFFFFu
#define PPCSR_SAMPLE_WEIGHTED 1u
int ppcsr_sample_neighbours(ppcsr_t h, const uint32_t *vertices, uint64_t k, uint32_t fanout, uint64_t seed, uint32_t flags, uint32_t *dests,
                            uint32_t *values, double *device_ms);
int ppcsr_sample_neighbours_device(ppcsr_t h, const uint32_t *d_vertices, uint64_t k, uint32_t fanout, uint64_t seed, uint32_t flags,
                                   uint32_t *d_dests, uint32_t *d_values, double *device_ms);
int ppcsr_random_walks(ppcsr_t h, const uint32_t *starts, uint64_t k, uint32_t length, uint64_t seed, uint32_t flags, uint32_t *out,
                       double *device_ms);
int ppcsr_random_walks_device(ppcsr_t h, const uint32_t *d_starts, uint64_t k, uint32_t length, uint64_t seed, uint32_t flags, uint32_t *d_out,
                              double *device_ms);
int ppcsr_degrees(ppcsr_t h, uint32_t *deg, uint64_t *wsum, double *device_ms);
/* Debugging: out[i] = the high half of a[i] * b[i], computed on the device by the wave layer's wrapper the draws use (host
 * pointers, k entries each).  EINVAL: null handle, a null pointer with k > 0. */
int ppcsr_debug_mulhi(ppcsr_t h, const uint64_t *a, const uint64_t *b, uint64_t k, uint64_t *out);
/* ---- multi-source BFS: the levels from k sources in one call, with the sums closeness and eccentricity are made of ----
 * The edge set is ppcsr_bfs's (live, non-sentinel slots other than slot N-1, src < n, dest < n; directed, values unused), and
 * the distances are OUT-distances: from the source along stored edges.  For closeness over incoming paths store the transpose.
 * With c_i(L) = the number of vertices at level L >= 1 from sources[i]:
 *   levels (k * n words, row-major) — row i is what ppcsr_bfs(h, sources[i], ...) returns, word for word (UINT32_MAX: unreachable)
 *   reached[i]  = vertices with a finite level, the source included
 *   far[i]      = sum over L of L * c_i(L)  (64-bit: n (n - 1) < 2^64, nothing saturates)
 *   ecc[i]      = the largest finite level (0 when nothing but the source is reached)
 *   harmonic[i] = sum over L = 1 .. ecc[i] of (double)c_i(L) / (double)L, added in ascending L, left to right, in fp64 on the
 *                 host from the integer counts: one division per level, nothing fused — a bit-reproducible number
 * Each of the five outputs may be NULL, not all five when k > 0.  Repeated sources are separate rows.  Sources are handled 64 at
 * a time, one bit each in a 64-bit word per vertex; a group of 64 costs about the streaming passes of one ppcsr_bfs.
 * Same contract as bfs: synchronous on the engine's stream, sees every batch applied before it, nothing of the graph is
 * written (state, stats, dirty tags, snapshot unchanged), device_ms may be NULL (it covers the level loops, not the copy of
 * levels to the host).  Every refusal is made before the first launch.  EINVAL: null handle, sources NULL with k > 0, all five
 * outputs NULL with k > 0, any sources[i] >= n; k == 0 succeeds and writes nothing.
 * Sequential regime (stats.narrow == 0): the call still answers; every level is then a streaming pass that takes each edge's
 * source from the item itself, as ppcsr_degrees / ppcsr_scc do — node ranges are never walked there. */
int ppcsr_multi_bfs(ppcsr_t h, const uint32_t *sources, uint64_t k, uint32_t *levels, uint64_t *reached, uint64_t *far, uint32_t *ecc,
                    double *harmonic, double *device_ms);
/* Debugging: what the last ppcsr_multi_bfs / pppcsr_multi_bfs run by this engine did, kept on the host from the reads the call
 * makes anyway: [0] groups of 64 sources, [1] level steps (all groups), [2] streaming edge passes, [3] per-vertex edge launches,
 * [4] passes that finished the hubs of a per-vertex launch, [5] largest union frontier of any step, [6] vertex-step launches,
 * [7] host reads inside the timed region.  EINVAL: null handle, out NULL. */
int ppcsr_debug_multi_bfs_counters(ppcsr_t h, uint64_t out[8]);
/* raw state for parity checks: items[N], nodes[n] exactly as the reference holds them (PCSR.h:67,128) */
int ppcsr_export_state(ppcsr_t h, ppcsr_edge *items, ppcsr_node *nodes);
int ppcsr_stats(ppcsr_t h, ppcsr_stats_t *out);
/* knobs (int64 values; every key engine.cc's set_option accepts):
 *   scheduler  "mode" (0 strict prefix rounds, 1 speculative rounds + validated rollback; default 1), "opt_horizon" (round
 *              width cap; default 3 x "resident_waves" = 3 x CUs x 24), "start_horizon", "adaptive", "epoch_ops", "epoch_short", "epoch_grow_after",
 *              "epoch_adapt", "region_slots" / "region_wide" / "region_calm" / "region_rare" / "region_rare_calm" / "region_rare_dist" / "region_rare_cpr", "soft_barrier", "defer_barrier", "small_batch" (batches up to this size take the strict
 *              rounds), "max_horizon" / "min_horizon" / "init_horizon" (strict rounds), "rounds_per_sync"
 *   windows    "big_min" / "big_window" (slots: above big_min a workgroup of the round rebalances the window, above
 *              big_window the update is exclusive), "big_grid", "excl_in_wave"
 *   rebalance  "scatter_variant" (0 LDS-staged, 1 register runs, 2 runs + in-tile leaf scan), "scatter_blocks",
 *              "rb_tile", "rb_min_tiles", "rb_prefetch", "rb_inplace_min" (partial windows of at least this many slots are
 *              rebalanced in place; 0 = always through the scratch array), "rb_inplace_cpw", "rb_inplace_lists"
 *   search     "search_narrow" (0: literal binary walk only)
 *   consumers  "msbfs_look" (0: the streaming pass of ppcsr_multi_bfs issues its ORs without first looking at next[w]; default 1),
 *              "colour_window" (test hook: colours per pass of ppcsr_colouring's long-list kernel over a list beyond 4096 entries;
 *              a multiple of 64 in [64, 32768], anything else is EINVAL; default 32768)
 *              "lp_table_slots" (test hook: slots of the label table a workgroup of ppcsr_label_propagation keeps for a list beyond
 *              512 entries; a power of two in [64, 4096], anything else is EINVAL; default 4096)
 *   measuring  "profile" (1: HIP events around every round kernel, reported through ppcsr_stats), "diag" (1: why updates
 *              did not commit, per epoch, on stderr; 2: also a per-update dependency trace, PPCSR_DIAG_DUMP = file), "marker" (marker kernels for profile cuts), "test_block_rebalance"
 *   reads      test hooks that move the seams of the batched reads (defaults = the shipped sizes; values in [1, 2^32]):
 *              "query_lookup_stage" (host lookups — and host common-neighbour pairs — per H2D / D2H round trip; 2^22), "query_gather_rows" (queried vertices
 *              per gather block; 2^20), "query_gather_chunks" (64-slot chunks per gather block; 2^22), "query_gather_stage"
 *              (edges per D2H window of a host gather; 2^22)
 *   snapshots  test hooks: "snap_grid" (cap on the workgroups of the two kernels that synchronise a snapshot incrementally, in
 *              [1, 4096]; default 4096 — a small value moves their grid-stride seam down to arrays of a few thousand slots),
 *              "snap_count" (1: count what every incremental synchronisation copies, see ppcsr_debug_snap_counters; default 0) */
int ppcsr_set_option(ppcsr_t h, const char *key, int64_t value);
/* device-side copy of the whole state and return to it (used by the benchmark to replay a batch on the same
 * core graph, and by the engine itself as the rollback point of speculative rounds); no reference equivalent.
 * After the first copy both directions are incremental: only leaves / node records written since (dirty tags) move */
int ppcsr_snapshot(ppcsr_t h);
int ppcsr_restore(ppcsr_t h);
/* Debugging: which way the snapshot machinery went.  out[0..3]: full saves, full loads, incremental commits, incremental
 * rollbacks since creation, counted over BOTH snapshots (the user's and the speculative epochs' rollback point), host-side and
 * always on.  out[4], out[5]: leaves / node records copied by the last incremental synchronisation of either snapshot — collected
 * only while option "snap_count" is 1 (0 until then; the option adds a stream synchronisation to every incremental
 * synchronisation, so it is for tests).  EINVAL: null handle or out. */
int ppcsr_debug_snap_counters(ppcsr_t h, uint64_t out[6]);
/* Debugging: entries of the speculative rounds' per-slot reservation table for duplicate overwrites (a power of two; slots that
 * many apart share an entry, which defers the later of two overwrites planned together by a round).  For tests that place edges. */
uint64_t ppcsr_debug_dup_slot_entries(void);
/* debugging / measurement helpers */
int ppcsr_check_invariants(ppcsr_t h, uint64_t *bad_leaves);
int ppcsr_bench_scan_all(ppcsr_t h, double *ms, uint64_t *total);
int ppcsr_bench_rebalance(ppcsr_t h, uint64_t window_slots, int iters, double *ms_per_call);
/* Debugging probe of the rebalance position chain: the functions every rebalance places its elements with, run ON THE DEVICE on
 * a batch of cases, in buffers of the call's own (the engine's state is neither read nor written).  No reference equivalent.
 *   mode  cases (words per case)              what runs                                              comes back
 *   0 table      (index, len, j)              one thread builds the table, a grid expands it         pos, info, segs, samples
 *   1 published  (index, len, j)              the table built INSIDE the expanding launch and handed pos, info, segs, samples, wg
 *                                             from workgroup 0 to the others segment by segment, over a POISONED buffer
 *   2 single     (index, len, j)              the one-segment closed form of the in-wave rebalance   pos (where accepted), info, segs
 *   3 linear     (index, len, j)              linear runs of <= 64 ranks at stride 37 vs the table   info
 *   4 segment    (bits of x, bits of step,    one segment from raw operands, then the device's own   segs (6 words per case), info,
 *                 mantissa S, exponent es)    fp64 subtractions walked along it                      pos (4096 words per case: bits)
 *   5 div        (a, b), both < 2^53, b > 0   the table build's floor division                       pos: (quotient, raw estimate)
 * pos: case c writes pos[pos_off[c] ...]: for j <= 2^22 the j positions, above that one order-independent 64-bit digest per block of
 * 2^20 consecutive ranks (wrapping sum of splitmix64(pos_k + k * 0x9E3779B97F4A7C15)).  sample_*: optional ranks whose literal
 * positions are wanted as well (sample_off: ncases + 1 offsets into sample_k / sample_pos).  info: 4 ints per case — segments,
 * overflow flag, verdict of mode 2 / differing positions of mode 3, runs mode 3 accepted.  segs: optional, 128 segments of 6 words
 * per case (t0, count, M0, Dfirst, Drest, shift).  wg: optional, mode 1, 4 words per case — workgroups, those (other than the
 * builder) that went ahead with a PART of the table, those that gave up waiting and built it themselves, fewest segments copied.
 * grid: mode 1, number of workgroups (0: one per 4096 ranks) */
typedef struct ppcsr_chain_probe_io {
  int32_t mode;
  uint32_t grid;
  uint64_t ncases;
  const uint64_t *cases;
  const uint64_t *pos_off;
  uint64_t *pos;
  const uint64_t *sample_off;
  const uint64_t *sample_k;
  uint64_t *sample_pos;
  int32_t *info;
  uint64_t *segs;
  uint32_t *wg;
} ppcsr_chain_probe_io;
int ppcsr_debug_chain_probe(ppcsr_t h, const ppcsr_chain_probe_io *io);
/* Debugging probe of the neighbourhood intersections (what ppcsr_triangles / ppcsr_common_neighbours stand on): the routines run ON
 * THE DEVICE, alone, on slot ranges of one or two edge buffers of the call's own (the engine's state is neither read nor written).
 * No reference equivalent.  cases: 6 words per case — (alo, ahi, blo, bhi, from_or_key, n): slot ranges [alo, ahi) of items_a and
 * [blo, bhi) of items_b; items_b == NULL, or == items_a with len_b == len_a: both ranges lie in items_a (two vertices of one partition).
 *   mode  what runs                                 launch shape                                       out[case]
 *   0 lane         the one-lane intersection        one case per lane: 64 cases diverge in a wave      |{from <= c < n} in both ranges|
 *   1 wave         the one-wave intersection        one wave per case, four per workgroup, one LDS     the same
 *                  (merge and probe forms)          tile each (the triangle kernel's shape)
 *   2 block        the one-workgroup intersection   one 256-thread workgroup per case                  the same (the four waves' shares added)
 *                  (streamed and probed tiles)
 *   3 lower_bound  the 64-sample search of [blo, bhi) for key, one wave per case                       first slot of [blo, bhi] behind which no
 *                                                                                                      live slot holds a dest < key
 *   4 probe        one lane's gap-aware binary search of [blo, bhi) for key, one case per lane         1: a live slot holds key, else 0
 *                  (reserved == 1: the slot is handed back, as edge_support / ktruss use the search)   reserved == 1: that slot, 0xFFFFFFFF: none
 * A slot is live when its value is not 0; the live dests of every range must ascend (the caller's duty: nothing checks it here).
 * tri: optional, modes 0-2: tri_n 64-bit words, zeroed by the call, tri[c] += 1 for every c counted by any case.
 * EINVAL: a range that leaves its buffer, lo > hi, a case with n > tri_n while tri is asked for, tri with tri_n == 0, more than
 * 2^20 cases, an unknown mode. */
typedef struct ppcsr_isect_probe_io {
  int32_t mode;
  uint32_t reserved;
  uint64_t ncases;
  const uint32_t *cases;
  const ppcsr_edge *items_a;
  uint64_t len_a;
  const ppcsr_edge *items_b;
  uint64_t len_b;
  uint32_t *out;
  uint64_t *tri;
  uint64_t tri_n;
} ppcsr_isect_probe_io;
int ppcsr_debug_isect_probe(ppcsr_t h, const ppcsr_isect_probe_io *io);
/* PCSR::double_list / half_list (PCSR.cpp:251-282, 284-320) alone: the array is doubled and halved back `iters` times; device time
 * per call of each (measurement helper: the array ends at its original size, evenly spread) */
int ppcsr_bench_resize(ppcsr_t h, int iters, double *double_ms, double *half_ms);
const char *ppcsr_strerror(int status);
const char *ppcsr_last_error(void); /* message of the last failing call on this thread */
int ppcsr_device_count(void);

/* ---- PPPCSR: vertex-range partitioning (PPPCSR.cpp:13-34, 58-66); one partition per GPU ------------------- */
/* PPPCSR::PPPCSR(init_n, src_n, lock_search, numDomain, partitionsPerDomain, use_numa): partition p lives on
 * devices[p % n_devices] (n_devices may be 1: all partitions on one GPU) */
int pppcsr_create(uint32_t init_n, uint32_t src_n, int lock_search, int num_domains, int parts_per_domain,
                  const int *devices, int n_devices, pppcsr_t *out);
/* the same layout, but only partitions [first_part, first_part + n_local_parts) are created, all on `device`: the form a
 * multi-process run uses (one rank per GPU holding the partitions of its domain; the other partitions live in other
 * processes and calls that route to them fail with EINVAL) */
int pppcsr_create_local(uint32_t init_n, int lock_search, int num_domains, int parts_per_domain, uint64_t first_part,
                        uint64_t n_local_parts, int device, pppcsr_t *out);
int pppcsr_destroy(pppcsr_t h);
int pppcsr_num_partitions(pppcsr_t h, uint64_t *out);
/* PPPCSR::get_partiton — PPPCSR.cpp:58-66 */
int pppcsr_get_partition(pppcsr_t h, uint64_t vertex, uint64_t *part);
int pppcsr_partition_start(pppcsr_t h, uint64_t part, uint64_t *first_vertex);
int pppcsr_partition(pppcsr_t h, uint64_t part, ppcsr_t *out); /* borrowed handle */
/* PPPCSR::add_edge / remove_edge / edge_exists / get_neighbourhood / getNode / get_n / add_node — PPPCSR.cpp:36-80 */
int pppcsr_add_edge(pppcsr_t h, uint32_t src, uint32_t dst, uint32_t value);
int pppcsr_remove_edge(pppcsr_t h, uint32_t src, uint32_t dst);
int pppcsr_edge_exists(pppcsr_t h, uint32_t src, uint32_t dst, int *exists);
int pppcsr_get_neighbourhood(pppcsr_t h, int src, int *out, uint64_t cap, uint64_t *count);
int pppcsr_get_node(pppcsr_t h, uint32_t v, ppcsr_node *out);
int pppcsr_get_n(pppcsr_t h, uint64_t *n);
int pppcsr_add_node(pppcsr_t h);
/* PPPCSR::edge_exists / get_neighbourhood (PPPCSR.cpp:36-80) batched: queries are routed by owner (src made partition-local,
 * PPPCSR.cpp:46-52), answered per partition by ppcsr_lookup_edges / ppcsr_gather_neighbourhoods on its device and returned in
 * the caller's order (same arguments and results as those).  A query owned by a partition this process does not hold fails
 * with EINVAL, as the single calls do. */
int pppcsr_lookup_edges(pppcsr_t h, const uint32_t *src, const uint32_t *dst, uint64_t n, uint32_t *values);
int pppcsr_gather_neighbourhoods(pppcsr_t h, const uint32_t *vertices, uint64_t k, uint64_t *row_offsets, int *dests, uint32_t *values,
                                 uint64_t cap, uint64_t *total);
/* sizes of the two calls above (test hooks that move their seams; the defaults are the shipped sizes): "query_block" (queries
 * routed at a time; default 2^20), "gather_stage" (edges fetched from one partition at a time; default 2^22).  Values in
 * [1, 2^32]; any other key or value fails with EINVAL. */
int pppcsr_set_option(pppcsr_t h, const char *key, int64_t value);
/* bfs.h:15-36 / pagerank.h:15-29 instantiated with T = PPPCSR (get_neighbourhood / getNode routed as in PPPCSR.cpp:40-42,
 * 76-80): the arguments and results of ppcsr_bfs / ppcsr_pagerank over the GLOBAL vertex ids (levels, node_values, out:
 * pppcsr_get_n entries).  One device call over every partition's array: per BFS level one launch whatever the number of
 * partitions; PageRank adds in ascending global source order, bit-identical to the template.  Destinations >= pppcsr_get_n
 * are skipped, as the single calls skip those >= n.  Synchronous; sees every batch applied before it; writes nothing to any
 * partition.  EINVAL: null handle or output, start >= pppcsr_get_n, or a partition not resident in this process.
 * EUNSUPPORTED: the partitions sit on more than one device (pppcsr_create with several devices) — run the host template. */
int pppcsr_bfs(pppcsr_t h, uint32_t start, uint32_t *levels, double *device_ms);
int pppcsr_pagerank(pppcsr_t h, const float *node_values, float *out, double *device_ms);
/* ppcsr_sssp / ppcsr_components over the GLOBAL vertex ids (dist, labels: pppcsr_get_n entries), one device call over every
 * partition's array: the results do not depend on the partitioning.  Same contract as pppcsr_bfs: synchronous; waits for
 * every partition's stream, runs on the first partition's; writes nothing to any partition.  EINVAL: null handle or output,
 * start >= pppcsr_get_n, or a partition not resident in this process.  EUNSUPPORTED: the partitions sit on more than one
 * device — there is no host form of these two calls. */
int pppcsr_sssp(pppcsr_t h, uint32_t start, uint64_t *dist, double *device_ms);
int pppcsr_components(pppcsr_t h, uint32_t *labels, double *device_ms);
/* ppcsr_kcore over the GLOBAL vertex ids (core: pppcsr_get_n entries), one device call over every partition's array: an edge
 * may have its two vertices in different partitions, and the result does not depend on the partitioning.  Same contract as
 * pppcsr_components; a partition in the sequential regime is answered.  EINVAL: null handle, core and kmax both NULL, or a
 * partition not resident in this process.  EUNSUPPORTED: the partitions sit on more than one device. */
int pppcsr_kcore(pppcsr_t h, uint32_t *core, uint32_t *kmax, double *device_ms);
/* ppcsr_colouring / ppcsr_mis over the GLOBAL vertex ids (colour: pppcsr_get_n entries, in_set: as many bytes; draw(v) takes
 * the global id), one device call over every partition's array: an edge may have its two vertices in different partitions, and
 * no output depends on the partitioning.  Same contract as pppcsr_kcore; a partition in the sequential regime is answered.  The
 * counters are those of the engine that ran the call, the first partition's (pppcsr_partition).  EINVAL: null handle, both
 * outputs NULL, an unknown order, or a partition not resident in this process.  EUNSUPPORTED: the partitions sit on more than
 * one device.  ENOMEM: a device allocation of the call failed (nothing written). */
int pppcsr_colouring(pppcsr_t h, uint32_t order, uint64_t seed, uint32_t *colour, uint32_t *ncolours, double *device_ms);
int pppcsr_mis(pppcsr_t h, uint32_t order, uint64_t seed, uint8_t *in_set, uint64_t *size, double *device_ms);
/* ppcsr_label_propagation / ppcsr_modularity over the GLOBAL vertex ids (init, labels: pppcsr_get_n entries; the colours are
 * pppcsr_colouring's).  Same definitions, same statuses; as for every pppcsr_ consumer, EINVAL for a partition not resident in
 * this process and EUNSUPPORTED for partitions on more than one device.  The answers do not depend on the partitioning. */
int pppcsr_label_propagation(pppcsr_t h, uint32_t order, uint64_t seed, uint32_t flags, uint32_t max_sweeps, const uint32_t *init, uint32_t *labels,
                             uint64_t *ncommunities, uint32_t *sweeps, double *device_ms);
int pppcsr_modularity(pppcsr_t h, const uint32_t *labels, uint32_t flags, uint64_t out[4], double *q, double *device_ms);
/* ppcsr_scc over the GLOBAL vertex ids (labels: pppcsr_get_n entries), one device call over every partition's array: an SCC may
 * span partitions, and the result does not depend on the partitioning.  Same contract as pppcsr_components; a partition in the
 * sequential regime is answered.  EINVAL: null handle, labels and count both NULL, or a partition not resident in this
 * process.  EUNSUPPORTED: the partitions sit on more than one device. */
int pppcsr_scc(pppcsr_t h, uint32_t *labels, uint64_t *count, double *device_ms);
/* ppcsr_msf over the GLOBAL vertex ids (edges' src / dest; labels: pppcsr_get_n entries), one device call over every partition's
 * array: a forest edge may join two partitions, and NO output depends on the partitioning.  Same contract as
 * pppcsr_components; a partition in the sequential regime is answered.  EINVAL: null handle, all four outputs NULL, or a
 * partition not resident in this process.  EUNSUPPORTED: the partitions sit on more than one device. */
int pppcsr_msf(pppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint64_t *weight, uint32_t *labels, double *device_ms);
/* ppcsr_edge_support / ppcsr_ktruss over the GLOBAL vertex ids (edges' src / dest; vtruss: pppcsr_get_n entries), one device call
 * over every partition's array: a triangle may span partitions, and NO output depends on the partitioning.  Same contract as
 * pppcsr_triangles.  EINVAL: null handle, all outputs NULL, or a partition not resident in this process.  EUNSUPPORTED: a
 * partition in the sequential regime, 2^32 slots or more in all, or partitions on more than one device. */
int pppcsr_edge_support(pppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint64_t *total, double *device_ms);
int pppcsr_ktruss(pppcsr_t h, ppcsr_edge *edges, uint64_t cap, uint64_t *count, uint32_t *tmax, uint32_t *vtruss, double *device_ms);
/* ppcsr_path_counts / ppcsr_betweenness over the GLOBAL vertex ids (start, sources; levels, sigma, bc: pppcsr_get_n entries),
 * one device call over every partition's array: path_counts does not depend on the partitioning, betweenness only within its
 * error bound (the order of the sums differs).  Same contract as pppcsr_sssp; a partition in the sequential regime is
 * answered.  EINVAL: as the single calls (start or a source >= pppcsr_get_n), or a partition not resident in this process.
 * EUNSUPPORTED: the partitions sit on more than one device. */
int pppcsr_path_counts(pppcsr_t h, uint32_t start, uint32_t *levels, double *sigma, double *device_ms);
int pppcsr_betweenness(pppcsr_t h, const uint32_t *sources, uint64_t k, double *bc, double *device_ms);
/* ppcsr_triangles / ppcsr_common_neighbours over the GLOBAL vertex ids (tri: pppcsr_get_n entries), one device call over every
 * partition's array: a pair may have its two vertices in different partitions, and the results do not depend on the
 * partitioning.  Same contract as pppcsr_bfs.  EINVAL: as the single calls, or a partition not resident in this process.
 * EUNSUPPORTED: the partitions sit on more than one device, or any partition is in the sequential regime. */
int pppcsr_triangles(pppcsr_t h, uint64_t *tri, uint64_t *total, double *device_ms);
int pppcsr_common_neighbours(pppcsr_t h, const uint32_t *a, const uint32_t *b, uint64_t k, uint32_t *counts, double *device_ms);
/* ppcsr_sample_neighbours / ppcsr_random_walks / ppcsr_degrees over the GLOBAL vertex ids (host pointers; deg, wsum:
 * pppcsr_get_n entries), one device call over every partition's array: a walk crosses partitions freely and the results do not
 * depend on the partitioning.  Same contract as pppcsr_bfs.  EINVAL: as the single calls, or a partition not resident in this
 * process.  EUNSUPPORTED: the partitions sit on more than one device, or (sample_neighbours, random_walks) any partition is in
 * the sequential regime. */
int pppcsr_sample_neighbours(pppcsr_t h, const uint32_t *vertices, uint64_t k, uint32_t fanout, uint64_t seed, uint32_t flags, uint32_t *dests,
                             uint32_t *values, double *device_ms);
int pppcsr_random_walks(pppcsr_t h, const uint32_t *starts, uint64_t k, uint32_t length, uint64_t seed, uint32_t flags, uint32_t *out,
                        double *device_ms);
int pppcsr_degrees(pppcsr_t h, uint32_t *deg, uint64_t *wsum, double *device_ms);
/* ppcsr_multi_bfs over the GLOBAL vertex ids (sources global; levels: k * pppcsr_get_n words), one device call over every
 * partition's array; the results do not depend on the partitioning.  Same contract as pppcsr_bfs; the sequential regime of any
 * partition makes every level a streaming pass.  EINVAL: as the single call, or a partition not resident in this process.
 * EUNSUPPORTED: the partitions sit on more than one device.  The counters are kept by the first partition's engine. */
int pppcsr_multi_bfs(pppcsr_t h, const uint32_t *sources, uint64_t k, uint32_t *levels, uint64_t *reached, uint64_t *far, uint32_t *ecc,
                     double *harmonic, double *device_ms);
/* bucket a host stream by owner (stable: per-partition order == stream order, src made partition-local as in
 * PPPCSR.cpp:46-52) and apply each bucket on its partition's GPU */
int pppcsr_apply_batch(pppcsr_t h, const ppcsr_op *ops, uint64_t n);
/* the same for a batch already resident in HBM (all partitions on that one GPU): device-side stable bucketing, then every
 * partition applies its bucket on its own stream, driven by one host thread each — the reference's ThreadPoolPPPCSR runs
 * its domains' workers concurrently in the same way (thread_pool_pppcsr.cpp:121-156) */
int pppcsr_apply_batch_device(pppcsr_t h, const ppcsr_op *d_ops, uint64_t n);
/* already routed subsequences (partition-local src, stream order), one device pointer per partition of
 * [first_part, first_part + n_parts): what a rank holds after the all-to-all exchange; applied concurrently as above */
int pppcsr_apply_parts_device(pppcsr_t h, uint64_t first_part, uint64_t n_parts, const ppcsr_op *const *d_ops,
                              const uint64_t *counts);
/* owner-bucketing primitive for the multi-process (one rank per GPU) path: counts[p] = ops owned by p,
 * bucketed = ops stably grouped by owner with partition-local src.  Pure host routine. */
int pppcsr_bucket_ops(uint32_t init_n, uint64_t n_parts, const ppcsr_op *ops, uint64_t n, ppcsr_op *bucketed,
                      uint64_t *counts);

/* the same routing for a block of the stream already resident in HBM (multi-GPU exchange): stable counting sort by
 * owner on `stream` (a hipStream_t, may be NULL); d_counts[p] (device memory, n_parts <= 64 entries) receives the bucket sizes */
int pppcsr_bucket_ops_device(uint32_t init_n, uint64_t n_parts, const ppcsr_op *d_ops, uint64_t n, ppcsr_op *d_bucketed,
                             uint64_t *d_counts, void *stream);

/* ---- multi-GPU owner exchange: what replaces ThreadPoolPPPCSR::submit_* (thread_pool_pppcsr.cpp:96-118) across processes ----
 * One process per GPU; each holds the contiguous partition range [rank * P / ranks, (rank + 1) * P / ranks) of the global
 * layout (pppcsr_create_local) and a contiguous block of the global stream in HBM.  The exchange has three steps:
 *   pack      stable device-side bucketing of the block by owner partition (src made partition-local, PPPCSR.cpp:46-52).
 *             The bucketed block IS the send buffer: ranks hold ascending partition ranges, so the rows for peer r are
 *             the contiguous run of its partitions' buckets — nothing is padded, only `counts` rows travel.
 *   transport first the bucket sizes (ppr numbers to and from every peer), then the rows: segment (source r, partition q)
 *             lands directly where the stream of partition q wants it (partition-major, source-rank-minor = global
 *             stream order per partition) — no unpack pass.
 *   apply     every local partition applies its stream concurrently (pppcsr_apply_parts_device).
 * pppcsr_exchange_apply runs all three with RCCL as the carrier (grouped ncclSend / ncclRecv on a HIP stream, bound at run
 * time by dlopen of librccl.so; two small collective steps per batch).  The pppcsr_xchg_* calls expose the same pack /
 * layout / apply code with the transport left to the caller (another carrier, or the tests' gloo transport between two
 * CPU-emulator processes).  pppcsr_xchg_create fails unless P is a multiple of n_ranks and the partitions resident in `h`
 * are exactly this rank's range, on one device.
 * The 128-byte unique id comes from rank 0 (pppcsr_comm_unique_id) and is handed to the other ranks by the host program
 * (any bootstrap: a file, MPI, torch.distributed's store).  Every rank must call pppcsr_exchange_apply for every batch, also
 * with an empty block.  A rank whose bucketing fails tells its peers through the counts, and no rank exchanges rows. */
typedef struct pppcsr_xchg *pppcsr_xchg_t; /* staging of one rank's side of the exchange */
int pppcsr_xchg_create(pppcsr_t h, int n_ranks, int rank, pppcsr_xchg_t *out);
int pppcsr_xchg_destroy(pppcsr_xchg_t x);
/* send_counts[P] (host, may be NULL): rows per partition; partition p's rows start at *d_send + sum(send_counts[0..p)) */
int pppcsr_xchg_pack(pppcsr_xchg_t x, const ppcsr_op *d_ops, uint64_t n, uint64_t *send_counts, const ppcsr_op **d_send);
/* recv_counts[r * ppr + q] = rows source rank r holds for my q-th partition (ppr = P / n_ranks); d_dst[r * ppr + q]
 * (may be NULL) = device address that segment must be written to before pppcsr_xchg_apply */
int pppcsr_xchg_layout(pppcsr_xchg_t x, const uint64_t *recv_counts, ppcsr_op **d_dst);
int pppcsr_xchg_apply(pppcsr_xchg_t x);
int pppcsr_xchg_set_num_neighbors(pppcsr_xchg_t x); /* the routed records are (vertex, num_neighbors, *): see pppcsr_repartition_export */
int pppcsr_xchg_bulk_build(pppcsr_xchg_t x);        /* the routed records are the adds EMPTY partitions are bulk-built from: idem */
int pppcsr_comm_unique_id(void *id_out_128_bytes);
int pppcsr_comm_create(const void *id_128_bytes, int n_ranks, int rank, int device, pppcsr_comm_t *out);
int pppcsr_comm_destroy(pppcsr_comm_t c);
int pppcsr_exchange_apply(pppcsr_t h, pppcsr_comm_t c, const ppcsr_op *d_ops, uint64_t n);
int pppcsr_exchange_set_num_neighbors(pppcsr_t h, pppcsr_comm_t c, const ppcsr_op *d_recs, uint64_t n);
int pppcsr_exchange_bulk_build(pppcsr_t h, pppcsr_comm_t c, const ppcsr_op *d_adds, uint64_t n);

/* ---- repartitioning.  The reference only sketches it (PCSR.h:91-112 is commented out), so there
 * is no reference behaviour to match; the rule here is deterministic and the tests rebuild it with the oracle:
 * new_starts[P] = first global vertex of every partition (new_starts[0] = 0, non-decreasing).  A partition whose vertex
 * range is unchanged keeps its array as it is.  A partition whose range changes is recreated empty at its new size, and
 * the edges of all such partitions are returned as adds of the global stream — (global src, dest, value), ascending
 * (src, dest) — in device memory owned by the handle (valid until the next call).  They are routed like any batch (owner
 * bucketing by the new starts; the exchange across ranks, every rank calling with the same new_starts) into the BULK BUILD
 * of the recreated partitions (ppcsr_bulk_build's rules: a valid packed-memory array with these edges, not the layout
 * one-by-one inserts would leave — there is no reference layout here, and a source-sorted stream through the exact path
 * is the hot-vertex worst case): pppcsr_bulk_build_device in one process, pppcsr_exchange_bulk_build across ranks,
 * pppcsr_xchg_bulk_build with a carrier of your own.  num_neighbors is a counter of calls, not the degree (duplicate adds
 * and deletes of missing edges move it, PCSR.cpp:1380/1409), so it travels beside the edges: d_nn holds one record
 * (global vertex, num_neighbors, 1) per vertex of the changed partitions, routed the same way AFTER the build
 * (pppcsr_set_num_neighbors_device / pppcsr_exchange_set_num_neighbors / pppcsr_xchg_set_num_neighbors).
 * pppcsr_repartition does all of it when every partition is resident in this process.  Updates applied afterwards go
 * through the ordinary (sequentially exact) path.
 * pppcsr_balanced_starts proposes starts of about equal weight, weight(v) = num_neighbors(v) + 1. */
int pppcsr_repartition_export(pppcsr_t h, const uint64_t *new_starts, const ppcsr_op **d_ops, uint64_t *n, const ppcsr_op **d_nn,
                              uint64_t *n_nn);
int pppcsr_set_num_neighbors_device(pppcsr_t h, const ppcsr_op *d_recs, uint64_t n);
/* global src; every receiving partition must be empty (ignored rows are received too); a partition no row is routed to is not touched */
int pppcsr_bulk_build_device(pppcsr_t h, const ppcsr_op *d_adds, uint64_t n);
int pppcsr_repartition(pppcsr_t h, const uint64_t *new_starts);
int pppcsr_balanced_starts(pppcsr_t h, uint64_t *starts_out);

#ifdef __cplusplus
}
#endif
#endif
