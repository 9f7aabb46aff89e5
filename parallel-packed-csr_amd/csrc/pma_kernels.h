// All kernels of the PMA engine (one translation unit: csrc/ppcsr_hip.hip).
//   pma_rounds.h       strict prefix rounds (k_plan / k_check / k_apply) and the exclusive executor (k_exclusive)
//   pma_spec_rounds.h  speculative rounds (o_plan / o_check / o_apply / o_big / o_settle): the default scheduler
//   pma_rebalance.h    whole-array / big-window rebalance, in-place window rebalance, snapshots, maintenance
//   pma_probe.h        debugging probe of the position chain (ppcsr_debug_chain_probe)
//   pma_consumer.h     what the consumers share: the table of gapped arrays, the streaming chunk loader, striped counts, list append
//   pma_scan.h         queries, bulk neighbour scan, bulk build, BFS / PageRank
//   pma_paths.h        shortest paths over the edge values, weakly connected components
//   pma_cores.h        core numbers (k-core decomposition): symmetric adjacency export, peeling in sub-rounds
//   pma_centrality.h   shortest-path counts and betweenness centrality: forward levels with fp64 counts, backward sweep
//   pma_scc.h          strongly connected components: trimming, forward-backward reach from a pivot, colouring
//   pma_msf.h          minimum spanning forest over the edge values: Boruvka rounds of two streaming passes, hook, pointer doubling
//   pma_intersect.h    triangle counts and common-neighbour counts: sorted intersection of two gapped vertex ranges
//   pma_truss.h        edge support and truss numbers: per-edge state by slot, in-lists, slot-returning searches, peeling in sub-rounds
//   pma_isect_probe.h  debugging probe of the intersection routines (ppcsr_debug_isect_probe)
//   pma_query.h        batched reads: edge lookups with values, neighbourhood gathers
//   pma_sample.h       neighbour sampling, random walks, live degrees: rank / weight select over gapped ranges, hub prefix per call
//   pma_msbfs.h        multi-source BFS: 64 sources per 64-bit word and vertex, edge step as a pass or per listed vertex, vertex step
//   pma_exchange.h     owner bucketing for the multi-GPU exchange
#pragma once
#include "pma_rounds.h"
#include "pma_spec_rounds.h"
#include "pma_rebalance.h"
#include "pma_probe.h"
#include "pma_consumer.h"
#include "pma_scan.h"
#include "pma_paths.h"
#include "pma_cores.h"
#include "pma_centrality.h"
#include "pma_scc.h"
#include "pma_msf.h"
#include "pma_intersect.h"
#include "pma_truss.h"
#include "pma_isect_probe.h"
#include "pma_query.h"
#include "pma_sample.h"
#include "pma_colour.h"
#include "pma_community.h"
#include "pma_msbfs.h"
#include "pma_exchange.h"
