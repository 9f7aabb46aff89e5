// Host side of the MI355X PMA engine: owns the HBM-resident state, drives the round scheduler and the
// exclusive executor, and implements the whole-array phases (double_list / half_list / big windows).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "pma_types.h"

namespace ppcsr {

struct View;  // pma_device.h
struct Edge;

// one partition of a consumer call (bfs_over and the others): its engine and its first global vertex
class Engine;
struct ConsumerRef {
  Engine *e;
  uint32_t first;
};

struct EngineStats {
  uint64_t N, n;
  int logN, H;
  uint64_t rounds, committed, planned, exclusive_ops, round_syncs;
  uint64_t redistribute_calls, redistribute_slots;  // algorithmic (what the reference performs)
  uint64_t double_calls, half_calls, big_redistributes, rollbacks;
  uint64_t not_found, duplicates, noops, slide_slots;
  uint64_t ops_applied;
  double last_batch_ms;      // device-only time of the last apply_batch (ops resident in HBM)
  double last_batch_h2d_ms;  // time of the H2D copy of the op array (host-buffer entry point)
  // profile mode (option "profile"=1): HIP-event time of each round kernel on the engine's stream
  double prof_plan_ms, prof_check_ms, prof_apply_ms, prof_compact_ms;
  uint64_t prof_launches;  // launches of EACH of the three kernels
  uint64_t wasted_rounds;  // rounds of speculative epochs that were rolled back (not part of `rounds`)
  uint64_t narrow_lost;    // times add_node-after-doubling switched the structure to the sequential regime
  uint64_t narrow;         // 1: sorted, disjoint vertex ranges (64-ary search narrowing + parallel rounds); 0: sequential regime
};

// ppcsr_debug_chain_probe (include/ppcsr.h: ppcsr_chain_probe_io, same layout)
struct ChainProbeIO {
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
};
// ppcsr_debug_isect_probe (include/ppcsr.h: ppcsr_isect_probe_io, same layout)
struct IsectProbeIO {
  int32_t mode;
  uint32_t reserved;
  uint64_t ncases;
  const uint32_t *cases;
  const Edge *items_a;
  uint64_t len_a;
  const Edge *items_b;
  uint64_t len_b;
  uint32_t *out;
  uint64_t *tri;
  uint64_t tri_n;
};

class Engine {
 public:
  static int create(uint32_t init_n, uint32_t src_n, int lock_search, int device, Engine **out, std::string *errmsg = nullptr);
  ~Engine();

  int apply_batch_host(const Op *ops, uint64_t n);
  int apply_batch_device(const Op *d_ops, uint64_t n);
  int add_edge(uint32_t s, uint32_t d, uint32_t value);
  int remove_edge(uint32_t s, uint32_t d);
  int add_node();
  int edge_exists(uint32_t s, uint32_t d, int *out);
  int get_node(uint32_t v, Node *out);
  int get_neighbourhood(int src, int *out, uint64_t cap, uint64_t *count);
  int read_neighbourhood(int src);
  // batched reads (pma_query.h); the pointers are host memory, or this GPU's memory when on_device
  int lookup_edges(const uint32_t *src, const uint32_t *dst, uint64_t n, uint32_t *values, bool on_device);
  int gather_neighbourhoods(const uint32_t *vertices, uint64_t k, uint64_t *row_offsets, int *dests, uint32_t *values, uint64_t cap,
                            uint64_t *total, bool on_device);
  int scan_all(uint64_t *row_offsets, int *dests, uint64_t cap, uint64_t *total);
  int export_triples_device(uint32_t src_base, Op *d_out, uint64_t cap, uint64_t *total);  // edges as adds of the global stream
  int export_num_neighbors_device(uint32_t base, Op *d_out);       // n records (vertex + base, num_neighbors, 1)
  int set_num_neighbors_device(const Op *d_recs, uint64_t cnt);    // records (local vertex, num_neighbors, *)
  int scan_all_device(double *ms, uint64_t *total);  // device-only timing of the bulk scan (bench)
  // graph-algorithm consumers over the gapped array (reference: src/utility/bfs.h, src/utility/pagerank.h)
  int bulk_build(const Op *host_ops, uint64_t m, double *device_ms);  // non-parity fast path
  int bulk_build_device(const Op *d_adds, uint64_t m, double *device_ms);  // the same, adds already in HBM (pppcsr_repartition)
  // Consumers (engine_consumers.cc) over P engines that hold consecutive vertex ranges of one graph of total_n vertices (a
  // PPPCSR's partitions, in partition order; edges stored with a local src and a global dest); one engine is the one-entry case
  // {this, 0}.  They run on THIS engine's stream and device, which every partition must share, and write nothing to any
  // partition's graph state.
  int bfs_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint32_t *levels, double *device_ms);
  int pagerank_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const float *node_values, float *out, double *device_ms);
  // shortest paths over the edge values (dist: total_n entries, UINT64_MAX = no path) and weakly connected components
  // (labels[v] = smallest vertex id of v's component) (pma_paths.h)
  int sssp_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint64_t *dist, double *device_ms);
  int components_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *labels, double *device_ms);
  // core numbers of the upper-orientation graph triangles counts in (pma_cores.h), in either regime: core (total_n entries,
  // may be null), *kmax (may be null): the largest core number
  int kcore_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *core, uint32_t *kmax, double *device_ms);
  // greedy colouring and the maximal independent set of the same graph in a fixed vertex order (pma_colour.h; the definitions:
  // include/ppcsr.h), in either regime.  order: PPCSR_ORDER_*, anything else is refused before the first launch.  colour
  // (total_n entries) / *ncolours and in_set (total_n bytes) / *size may each be null.  *_counters: what the last call on this
  // engine did (ppcsr_debug_colouring_counters / ppcsr_debug_mis_counters)
  int colouring_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint32_t *colour, uint32_t *ncolours,
                     double *device_ms);
  int mis_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint8_t *in_set, uint64_t *size,
               double *device_ms);
  int colouring_counters(uint64_t out[8]);
  // label-propagation communities under the colouring's schedule, and the modularity of any labels (pma_community.h; the
  // definitions: include/ppcsr.h), in either regime.  order / flags: anything unknown, and an init entry >= total_n, is refused
  // before the device is selected.  init (total_n entries) may be null: label[v] = v.  labels (total_n entries), *ncommunities
  // and *sweeps may each be null.  modularity_over: labels (total_n entries, each < total_n), out[4] and *q (either may be null).
  // community_counters: what the last label_propagation_over on this engine did (ppcsr_debug_community_counters)
  int label_propagation_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t order, uint64_t seed, uint32_t flags,
                             uint32_t max_sweeps, const uint32_t *init, uint32_t *labels, uint64_t *ncommunities, uint32_t *sweeps,
                             double *device_ms);
  int modularity_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *labels, uint32_t flags, uint64_t out[4], double *q,
                      double *device_ms);
  int community_counters(uint64_t out[8]);
  int mis_counters(uint64_t out[8]);
  // strongly connected components (pma_scc.h), in either regime: labels[v] = smallest vertex id of v's SCC (total_n entries, may
  // be null), *count = number of SCCs (may be null).  scc_counters: what the last scc_over on this engine did
  // (ppcsr_debug_scc_counters, include/ppcsr.h)
  int scc_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *labels, uint64_t *count, double *device_ms);
  int scc_counters(uint64_t out[8]);
  // minimum spanning forest over the edge values (pma_msf.h), in either regime: edges (at most cap, ascending by (src, dest) =
  // (lo, hi), may be null), *count = forest edges, *weight = their sum, labels as components_over gives them (total_n entries);
  // each may be null.  PPCSR_ERANGE when edges != null and cap < *count, everything else delivered.  msf_counters: what the last
  // msf_over on this engine did (ppcsr_debug_msf_counters, include/ppcsr.h)
  int msf_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *weight,
               uint32_t *labels, double *device_ms);
  int msf_counters(uint64_t out[8]);
  // edge support and truss numbers of the upper-orientation graph triangles counts in (pma_truss.h; the definitions:
  // include/ppcsr.h), regular regime only.  edges (at most cap, ascending (src, dest) = slot order, value = support / truss
  // number), *count = |E(G)|, *total = triangles, *tmax = the largest truss number, vtruss (total_n entries): the largest at every
  // vertex; each may be null.  PPCSR_ERANGE when edges != null and cap < *count, everything else delivered.  ktruss_counters:
  // what the last of the two calls on this engine did (ppcsr_debug_ktruss_counters)
  int edge_support_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *total,
                        double *device_ms);
  int ktruss_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, Edge *edges, uint64_t cap, uint64_t *count, uint32_t *tmax,
                  uint32_t *vtruss, double *device_ms);
  int ktruss_counters(uint64_t out[8]);
  // shortest-path counts and betweenness centrality (pma_centrality.h), in either regime.  path_counts: levels as bfs_over
  // gives them and sigma[v] = number of fewest-edge paths from `start` to v, in fp64 (total_n entries each; either may be
  // null, not both).  betweenness: bc[v] (total_n entries) = Brandes' dependency of the k sources on v, endpoints
  // excluded, nothing halved or normalised; a source >= total_n is refused before the first launch.
  int path_counts_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t start, uint32_t *levels, double *sigma,
                       double *device_ms);
  int betweenness_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, double *bc,
                       double *device_ms);
  // consumers that intersect two neighbourhoods (pma_intersect.h).  triangles: upper orientation — {a, b}, a < b, is an edge
  // exactly when (a, b) is stored; tri (total_n entries, may be null): triangles through every vertex; *total (may be null):
  // triangles.  common_neighbours: counts[i] = stored dests < total_n shared by a[i] and b[i] (vertices >= total_n: 0); a, b,
  // counts are host memory, or this GPU's when on_device.  Both fail with PPCSR_EUNSUPPORTED while a partition is in the
  // sequential regime (narrow == 0).
  int triangles_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint64_t *tri, uint64_t *total, double *device_ms);
  int common_neighbours_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *a, const uint32_t *b, uint64_t k,
                             uint32_t *counts, bool on_device, double *device_ms);
  // neighbour sampling, random walks and live degrees (pma_sample.h; the definition: include/ppcsr.h).  sample: dests / values
  // [k * fanout] (values may be null); walks: out [k * (length + 1)]; vertices / starts and the outputs are host memory, or
  // this GPU's when on_device.  Both fail with PPCSR_EUNSUPPORTED in the sequential regime (vertex ranges cannot be trusted).
  // degrees: deg[v] = |L(v)|, wsum[v] = the sum of L(v)'s values (total_n entries, either may be null), in either regime.
  // mulhi: the wave layer's 128-bit product on the device, for the tests (host pointers).
  int sample_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *vertices, uint64_t k, uint32_t fanout, uint64_t seed,
                  uint32_t flags, uint32_t *dests, uint32_t *values, bool on_device, double *device_ms);
  int walks_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *starts, uint64_t k, uint32_t length, uint64_t seed,
                 uint32_t flags, uint32_t *out, bool on_device, double *device_ms);
  int degrees_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, uint32_t *deg, uint64_t *wsum, double *device_ms);
  int debug_mulhi(const uint64_t *a, const uint64_t *b, uint64_t k, uint64_t *out);
  // multi-source BFS (pma_msbfs.h; the definition: include/ppcsr.h), in either regime: row i of levels (k * total_n words) as
  // bfs_over gives it from sources[i]; reached / far / ecc / harmonic: k entries each; every output may be null.  A source
  // >= total_n is refused before the first launch; k == 0 writes nothing.  multi_bfs_counters: what the last multi_bfs_over
  // on this engine did (ppcsr_debug_multi_bfs_counters)
  int multi_bfs_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, uint32_t *levels,
                     uint64_t *reached, uint64_t *far, uint32_t *ecc, double *harmonic, double *device_ms);
  int multi_bfs_counters(uint64_t out[8]);
  int export_state(Edge *items, Node *nodes);
  int check_invariants(uint64_t *bad);  // leafcnt == recount(items)
  int stats(EngineStats *out);
  int set_option(const char *key, int64_t value);
  int rebalance_bench(uint64_t wlen, int iters, double *ms_per_call);
  int resize_bench(int iters, double *double_ms, double *half_ms);
  int chain_probe(const ChainProbeIO *io);  // the position-chain functions run on the device, engine state untouched
  int isect_probe(const IsectProbeIO *io);  // the intersection routines of pma_intersect.h likewise
  int snapshot();  // device-side copy of the whole state (items, nodes, leaf counts, geometry)
  int restore();   // back to the last snapshot (device-to-device)  // whole-window rebalance kernel timing

  int snap_counters(uint64_t out[6]);  // ppcsr_debug_snap_counters (include/ppcsr.h)
  static uint64_t dup_slot_entries();  // ppcsr_debug_dup_slot_entries (include/ppcsr.h)

  uint64_t N() const;
  uint32_t n() const;
  int logN() const;
  int H() const;
  int device() const { return device_; }
  const std::string &last_error() const { return err_; }

 private:
  Engine();
  int init(uint32_t init_n, uint32_t src_n, int lock_search, int device);
  int run_rounds(const Op *d_ops, uint64_t n);
  // spec_index != kMax: the update sits at that index of d_ops and runs inside a speculative epoch (stamp-validated);
  // *violation / *resized report what happened
  int run_exclusive(Op op, uint32_t flags, const Op *d_ops = nullptr, uint32_t spec_index = 0xFFFFFFFFu, bool *violation = nullptr,
                    bool *resized = nullptr, bool later_committed = false);
  int resize(uint64_t newN);
  int big_redistribute(uint64_t wstart, uint64_t wlen, bool sync = true);
  int inplace_fault_check();
  int rank_scan(const uint32_t *d_cnt, uint64_t nleaves, bool table = false, uint64_t tb_index = 0, uint64_t tb_len = 0);
  int recheck_ranges();  // narrow == 0: look whether the vertex ranges are sane again and re-enable narrowing + parallel rounds
  int ensure_scratch(uint64_t nleaves);
  int ensure_tiles(uint64_t ntiles);
  int fail(int code, const std::string &msg);
  int pull_stats();

  int run_speculative(const Op *d_ops, uint64_t n);
  int rebalance_fused(const View &nv, const Edge *src_items, uint64_t src_lo, uint64_t src_len, int src_sh, uint32_t *src_cnt,
                      bool inplace, uint64_t tb_index, uint64_t tb_len, Edge *dst, uint64_t dst_bias, uint32_t *dst_cnt, uint64_t dst_nleaves);
  int bulk_build_from(const Op *in_ops, bool on_device, uint64_t m, double *device_ms);
  int xscan(const void *in, bool in64, uint64_t n, void *out, bool out64, bool mx, bool inclusive, unsigned long long *scr = nullptr);
  int gather_prepare(const uint32_t *q, uint64_t kb, uint64_t *kt, uint64_t *C, uint64_t *T);
  int scan_launch(unsigned long long *d_rows, int *d_dst, uint64_t cap, const float *d_values = nullptr, float *d_contrib = nullptr,
                  Op *d_triples = nullptr, uint32_t src_base = 0);
  // the bulk scan of `part`'s array in two halves, launched on THIS engine's stream with part's scratch: the chunk counts and
  // tile sums (edge total in part's d_total), then the writing pass
  int scan_count(Engine *part, uint32_t *tile, uint64_t *ntiles);
  int intersect_regime(const ConsumerRef *parts, uint32_t P, const char *what, std::string *msg);
  int consumer_table(const ConsumerRef *parts, uint32_t P, uint32_t total_n, void **d_tab, uint64_t *slots, int alloc_code);
  // what edge_support_over and ktruss_over share: stage 1, the support phase and, for ktruss, the peel
  int truss_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, bool peel, Edge *edges, uint64_t cap, uint64_t *count, uint64_t *total,
                 uint32_t *tmax, uint32_t *vtruss, double *device_ms);
  // what path_counts_over and betweenness_over share: the forward phase from every source and, when bc is wanted, the backward sweep
  int centrality_over(const ConsumerRef *parts, uint32_t P, uint32_t total_n, const uint32_t *sources, uint64_t k, uint32_t *levels,
                      double *sigma, double *bc, double *device_ms);
  void scan_write(Engine *part, uint32_t tile, uint64_t ntiles, unsigned long long *d_rows, int *d_dst, uint64_t cap, const float *d_values,
                  float *d_contrib, Op *d_triples, uint32_t src_base, uint32_t dest_bound);

 public:
  struct Impl;

 private:
  struct ConsumerScope;  // engine_consumers.cc
  struct SpecRun;        // engine.cc: the steps of run_speculative
  Impl *p_;
  int device_ = 0;
  std::string err_;
};

const char *error_string(int code);
// stable owner bucketing of a device-resident block of the stream (multi-GPU exchange); runs on `stream`
// (starts: the first global vertex of each of the n_parts <= 64 partitions, host memory)
int bucket_ops_device(const uint32_t *starts, uint32_t n_parts, const Op *d_ops, uint64_t n, Op *d_out, unsigned long long *d_counts,
                      void *stream, std::string *errmsg);
}  // namespace ppcsr
int gpu_device_count_for_capi(int *n);
namespace ppcsr {

}  // namespace ppcsr
