"""ppcsr_amd — thin ctypes binding of the MI355X packed-CSR engine (libppcsr_hip.so, C ABI in include/ppcsr.h).

The library is hand-written HIP for gfx950; there is NO CPU fallback: importing works anywhere, but creating
an engine without the built library or without a GPU raises.  Classes mirror the reference's
PCSR / PPPCSR method names (src/pcsr/PCSR.h:64-124, src/pppcsr/PPPCSR.h:11-60).

(The directory name contains a hyphen, so load this package by path — see tests/helpers.py:load_pkg.)
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PPCSR_LIB", os.path.join(_HERE, "csrc", "libppcsr_hip.so"))  # env override: debugging builds only

c_vp, c_u32, c_u64, c_int, c_i64, c_dbl = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.c_int64, ctypes.c_double)


class PpcsrError(RuntimeError):
    pass


class Stats(ctypes.Structure):
    _fields_ = [("N", c_u64), ("n", c_u64), ("logN", ctypes.c_int32), ("H", ctypes.c_int32),
                ("rounds", c_u64), ("committed", c_u64), ("planned", c_u64), ("exclusive_ops", c_u64),
                ("round_syncs", c_u64), ("redistribute_calls", c_u64), ("redistribute_slots", c_u64),
                ("double_calls", c_u64), ("half_calls", c_u64), ("big_redistributes", c_u64), ("rollbacks", c_u64),
                ("not_found", c_u64), ("duplicates", c_u64), ("noops", c_u64), ("slide_slots", c_u64),
                ("ops_applied", c_u64), ("last_batch_ms", c_dbl), ("last_batch_h2d_ms", c_dbl),
                ("prof_plan_ms", c_dbl), ("prof_check_ms", c_dbl), ("prof_apply_ms", c_dbl), ("prof_compact_ms", c_dbl), ("prof_launches", c_u64),
                ("wasted_rounds", c_u64), ("narrow_lost", c_u64), ("narrow", c_u64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ChainProbeIO(ctypes.Structure):
    """ppcsr_chain_probe_io (include/ppcsr.h)"""
    _fields_ = [("mode", ctypes.c_int32), ("grid", c_u32), ("ncases", c_u64), ("cases", c_vp), ("pos_off", c_vp), ("pos", c_vp),
                ("sample_off", c_vp), ("sample_k", c_vp), ("sample_pos", c_vp), ("info", c_vp), ("segs", c_vp), ("wg", c_vp)]


class IsectProbeIO(ctypes.Structure):
    """ppcsr_isect_probe_io (include/ppcsr.h)"""
    _fields_ = [("mode", ctypes.c_int32), ("reserved", c_u32), ("ncases", c_u64), ("cases", c_vp), ("items_a", c_vp), ("len_a", c_u64),
                ("items_b", c_vp), ("len_b", c_u64), ("out", c_vp), ("tri", c_vp), ("tri_n", c_u64)]


ISECT_PROBE_MODES = {"lane": 0, "wave": 1, "block": 2, "lower_bound": 3, "probe": 4}
CHAIN_PROBE_MODES = {"table": 0, "published": 1, "single": 2, "linear": 3, "segment": 4, "div": 5}
CHAIN_PROBE_LITERAL_MAX = 1 << 22  # windows with more elements come back as one digest per 2^20 ranks
CHAIN_PROBE_DIGEST_LOG = 20
CHAIN_PROBE_WALK = 4096
CHAIN_MAX_SEG = 128

EXPORTED = [
    "ppcsr_create", "ppcsr_destroy", "ppcsr_add_edge", "ppcsr_remove_edge", "ppcsr_add_node", "ppcsr_apply_batch",
    "ppcsr_apply_batch_device", "ppcsr_edge_exists", "ppcsr_get_n", "ppcsr_get_node", "ppcsr_geometry",
    "ppcsr_get_neighbourhood", "ppcsr_read_neighbourhood", "ppcsr_scan_all", "ppcsr_bulk_build", "ppcsr_bfs", "ppcsr_pagerank", "ppcsr_export_state", "ppcsr_stats",
    "ppcsr_set_option", "ppcsr_snapshot", "ppcsr_restore", "ppcsr_debug_snap_counters", "ppcsr_check_invariants", "ppcsr_bench_scan_all", "ppcsr_bench_rebalance", "ppcsr_bench_resize", "ppcsr_strerror",
    "ppcsr_last_error", "ppcsr_device_count", "pppcsr_create", "pppcsr_destroy", "pppcsr_num_partitions",
    "pppcsr_get_partition", "pppcsr_partition_start", "pppcsr_partition", "pppcsr_add_edge", "pppcsr_remove_edge",
    "pppcsr_edge_exists", "pppcsr_get_neighbourhood", "pppcsr_get_node", "pppcsr_get_n", "pppcsr_add_node",
    "pppcsr_apply_batch", "pppcsr_bucket_ops", "pppcsr_bucket_ops_device",
    "pppcsr_create_local", "pppcsr_apply_batch_device", "pppcsr_apply_parts_device",
    "pppcsr_comm_unique_id", "pppcsr_comm_create", "pppcsr_comm_destroy", "pppcsr_exchange_apply",
    "pppcsr_xchg_create", "pppcsr_xchg_destroy", "pppcsr_xchg_pack", "pppcsr_xchg_layout", "pppcsr_xchg_apply",
    "pppcsr_repartition_export", "pppcsr_repartition", "pppcsr_balanced_starts", "pppcsr_set_num_neighbors_device",
    "pppcsr_xchg_set_num_neighbors", "pppcsr_exchange_set_num_neighbors", "pppcsr_bulk_build_device", "pppcsr_xchg_bulk_build",
    "pppcsr_exchange_bulk_build", "ppcsr_lookup_edges", "ppcsr_lookup_edges_device", "ppcsr_gather_neighbourhoods",
    "ppcsr_gather_neighbourhoods_device", "pppcsr_lookup_edges", "pppcsr_gather_neighbourhoods", "pppcsr_set_option",
    "pppcsr_bfs", "pppcsr_pagerank", "ppcsr_sssp", "ppcsr_components", "pppcsr_sssp", "pppcsr_components",
    "ppcsr_debug_chain_probe", "ppcsr_debug_isect_probe", "ppcsr_kcore", "pppcsr_kcore",
    "ppcsr_path_counts", "ppcsr_betweenness", "pppcsr_path_counts", "pppcsr_betweenness",
    "ppcsr_scc", "pppcsr_scc", "ppcsr_debug_scc_counters",
    "ppcsr_msf", "pppcsr_msf", "ppcsr_debug_msf_counters",
    "ppcsr_edge_support", "pppcsr_edge_support", "ppcsr_ktruss", "pppcsr_ktruss", "ppcsr_debug_ktruss_counters",
    "ppcsr_triangles", "pppcsr_triangles", "ppcsr_common_neighbours", "ppcsr_common_neighbours_device", "pppcsr_common_neighbours",
    "ppcsr_sample_neighbours", "ppcsr_sample_neighbours_device", "pppcsr_sample_neighbours",
    "ppcsr_random_walks", "ppcsr_random_walks_device", "pppcsr_random_walks", "ppcsr_degrees", "pppcsr_degrees", "ppcsr_debug_mulhi",
    "ppcsr_multi_bfs", "pppcsr_multi_bfs", "ppcsr_debug_multi_bfs_counters", "ppcsr_debug_dup_slot_entries",
    "ppcsr_colouring", "pppcsr_colouring", "ppcsr_mis", "pppcsr_mis", "ppcsr_debug_colouring_counters", "ppcsr_debug_mis_counters",
    "ppcsr_label_propagation", "pppcsr_label_propagation", "ppcsr_modularity", "pppcsr_modularity", "ppcsr_debug_community_counters",
]

NO_PATH = 0xFFFFFFFFFFFFFFFF  # PPCSR_NO_PATH: what sssp reports for a vertex no path reaches
NO_EDGE = 0xFFFFFFFF  # PPCSR_NO_EDGE: what lookup_edges reports for a pair that is not an edge
ORDERS = {"random": 0, "degree": 1, "id": 2}  # PPCSR_ORDER_*: the vertex orders of colouring / mis
COMMUNITY_WEIGHTED = 1  # PPCSR_COMMUNITY_WEIGHTED: label_propagation / modularity weigh an edge by its stored value
NO_VERTEX = 0xFFFFFFFF  # PPCSR_NO_VERTEX: what sample_neighbours / random_walks report where there is nothing to pick from

_LIBS = {}


def dup_slot_entries(lib=None):
    """Debugging (ppcsr_debug_dup_slot_entries): entries of the speculative rounds' per-slot table for duplicate overwrites — two
    slots that many apart share an entry.  (Resolved on use: a library older than the table still loads.)"""
    f = (lib or load_library()).ppcsr_debug_dup_slot_entries
    f.restype, f.argtypes = c_u64, []
    return int(f())


def _share_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7)
    and look it up by its unversioned file name, so if the engine pulled /opt/rocm's copy in first, a later `import torch`
    would load a second runtime that finds no GPU (and the reverse order would starve the engine).  Pre-loading torch's
    copy — without importing torch — makes both resolve to the same object.  Without torch the engine uses /opt/rocm's."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path=None):
    """Load the engine library.  Default: the in-tree HIP build; raises if it has not been built."""
    path = path or LIB_PATH
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise PpcsrError(f"{path} not found: build it with `python __graft_entry__.py` "
                         "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_hip_runtime()
    L = ctypes.CDLL(path)
    L.ppcsr_create.argtypes = [c_u32, c_u32, c_int, c_int, ctypes.POINTER(c_vp)]
    L.ppcsr_destroy.argtypes = [c_vp]
    L.ppcsr_add_edge.argtypes = [c_vp, c_u32, c_u32, c_u32]
    L.ppcsr_remove_edge.argtypes = [c_vp, c_u32, c_u32]
    L.ppcsr_add_node.argtypes = [c_vp]
    L.ppcsr_apply_batch.argtypes = [c_vp, c_vp, c_u64]
    L.ppcsr_apply_batch_device.argtypes = [c_vp, c_vp, c_u64]
    L.ppcsr_edge_exists.argtypes = [c_vp, c_u32, c_u32, ctypes.POINTER(c_int)]
    L.ppcsr_get_n.argtypes = [c_vp, ctypes.POINTER(c_u64)]
    L.ppcsr_get_node.argtypes = [c_vp, c_u32, c_vp]
    L.ppcsr_geometry.argtypes = [c_vp, ctypes.POINTER(c_u64), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    L.ppcsr_get_neighbourhood.argtypes = [c_vp, c_int, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.ppcsr_read_neighbourhood.argtypes = [c_vp, c_int]
    L.ppcsr_scan_all.argtypes = [c_vp, c_vp, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.ppcsr_lookup_edges.argtypes = [c_vp, c_vp, c_vp, c_u64, c_vp]
    L.ppcsr_lookup_edges_device.argtypes = [c_vp, c_vp, c_vp, c_u64, c_vp]
    L.ppcsr_gather_neighbourhoods.argtypes = [c_vp, c_vp, c_u64, c_vp, c_vp, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.ppcsr_gather_neighbourhoods_device.argtypes = [c_vp, c_vp, c_u64, c_vp, c_vp, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.pppcsr_lookup_edges.argtypes = [c_vp, c_vp, c_vp, c_u64, c_vp]
    L.pppcsr_gather_neighbourhoods.argtypes = [c_vp, c_vp, c_u64, c_vp, c_vp, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.pppcsr_set_option.argtypes = [c_vp, ctypes.c_char_p, c_i64]
    L.pppcsr_bfs.argtypes = [c_vp, c_u32, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.pppcsr_pagerank.argtypes = [c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_sssp", "pppcsr_sssp"):
        getattr(L, name).argtypes = [c_vp, c_u32, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_components", "pppcsr_components"):
        getattr(L, name).argtypes = [c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_path_counts", "pppcsr_path_counts"):
        getattr(L, name).argtypes = [c_vp, c_u32, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_betweenness", "pppcsr_betweenness"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_kcore", "pppcsr_kcore"):
        getattr(L, name).argtypes = [c_vp, c_vp, ctypes.POINTER(c_u32), ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_scc", "pppcsr_scc"):
        getattr(L, name).argtypes = [c_vp, c_vp, ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_scc_counters.argtypes = [c_vp, c_vp]
    for name in ("ppcsr_msf", "pppcsr_msf"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_msf_counters.argtypes = [c_vp, c_vp]
    for name in ("ppcsr_edge_support", "pppcsr_edge_support"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_ktruss", "pppcsr_ktruss"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, ctypes.POINTER(c_u64), ctypes.POINTER(c_u32), c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_ktruss_counters.argtypes = [c_vp, c_vp]
    for name in ("ppcsr_triangles", "pppcsr_triangles"):
        getattr(L, name).argtypes = [c_vp, c_vp, ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_common_neighbours", "ppcsr_common_neighbours_device", "pppcsr_common_neighbours"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_vp, c_u64, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_sample_neighbours", "ppcsr_sample_neighbours_device", "pppcsr_sample_neighbours"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, c_u32, c_u64, c_u32, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_random_walks", "ppcsr_random_walks_device", "pppcsr_random_walks"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, c_u32, c_u64, c_u32, c_vp, ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_degrees", "pppcsr_degrees"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_mulhi.argtypes = [c_vp, c_vp, c_vp, c_u64, c_vp]
    for name in ("ppcsr_multi_bfs", "pppcsr_multi_bfs"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u64, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_multi_bfs_counters.argtypes = [c_vp, c_vp]
    for name in ("ppcsr_colouring", "pppcsr_colouring"):
        getattr(L, name).argtypes = [c_vp, c_u32, c_u64, c_vp, ctypes.POINTER(c_u32), ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_mis", "pppcsr_mis"):
        getattr(L, name).argtypes = [c_vp, c_u32, c_u64, c_vp, ctypes.POINTER(c_u64), ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_colouring_counters.argtypes = [c_vp, c_vp]
    for name in ("ppcsr_label_propagation", "pppcsr_label_propagation"):
        getattr(L, name).argtypes = [c_vp, c_u32, c_u64, c_u32, c_u32, c_vp, c_vp, ctypes.POINTER(c_u64), ctypes.POINTER(c_u32),
                                     ctypes.POINTER(ctypes.c_double)]
    for name in ("ppcsr_modularity", "pppcsr_modularity"):
        getattr(L, name).argtypes = [c_vp, c_vp, c_u32, c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_debug_community_counters.argtypes = [c_vp, c_vp]
    L.ppcsr_debug_mis_counters.argtypes = [c_vp, c_vp]
    L.ppcsr_bulk_build.argtypes = [c_vp, c_vp, c_u64, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_bfs.argtypes = [c_vp, c_u32, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_pagerank.argtypes = [c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.ppcsr_export_state.argtypes = [c_vp, c_vp, c_vp]
    L.ppcsr_stats.argtypes = [c_vp, ctypes.POINTER(Stats)]
    L.ppcsr_set_option.argtypes = [c_vp, ctypes.c_char_p, c_i64]
    L.ppcsr_snapshot.argtypes = [c_vp]
    L.ppcsr_restore.argtypes = [c_vp]
    L.ppcsr_debug_snap_counters.argtypes = [c_vp, c_vp]
    L.ppcsr_check_invariants.argtypes = [c_vp, ctypes.POINTER(c_u64)]
    L.ppcsr_bench_scan_all.argtypes = [c_vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_u64)]
    L.ppcsr_bench_rebalance.argtypes = [c_vp, c_u64, c_int, ctypes.POINTER(c_dbl)]
    L.ppcsr_debug_chain_probe.argtypes = [c_vp, ctypes.POINTER(ChainProbeIO)]
    L.ppcsr_debug_isect_probe.argtypes = [c_vp, ctypes.POINTER(IsectProbeIO)]
    L.ppcsr_bench_resize.argtypes = [c_vp, c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl)]
    L.ppcsr_strerror.restype = ctypes.c_char_p
    L.ppcsr_strerror.argtypes = [c_int]
    L.ppcsr_last_error.restype = ctypes.c_char_p
    L.pppcsr_create.argtypes = [c_u32, c_u32, c_int, c_int, c_int, c_vp, c_int, ctypes.POINTER(c_vp)]
    L.pppcsr_destroy.argtypes = [c_vp]
    L.pppcsr_num_partitions.argtypes = [c_vp, ctypes.POINTER(c_u64)]
    L.pppcsr_get_partition.argtypes = [c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.pppcsr_partition_start.argtypes = [c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.pppcsr_partition.argtypes = [c_vp, c_u64, ctypes.POINTER(c_vp)]
    L.pppcsr_add_edge.argtypes = [c_vp, c_u32, c_u32, c_u32]
    L.pppcsr_remove_edge.argtypes = [c_vp, c_u32, c_u32]
    L.pppcsr_edge_exists.argtypes = [c_vp, c_u32, c_u32, ctypes.POINTER(c_int)]
    L.pppcsr_get_neighbourhood.argtypes = [c_vp, c_int, c_vp, c_u64, ctypes.POINTER(c_u64)]
    L.pppcsr_get_node.argtypes = [c_vp, c_u32, c_vp]
    L.pppcsr_get_n.argtypes = [c_vp, ctypes.POINTER(c_u64)]
    L.pppcsr_add_node.argtypes = [c_vp]
    L.pppcsr_apply_batch.argtypes = [c_vp, c_vp, c_u64]
    L.pppcsr_bucket_ops.argtypes = [c_u32, c_u64, c_vp, c_u64, c_vp, c_vp]
    L.pppcsr_bucket_ops_device.argtypes = [c_u32, c_u64, c_vp, c_u64, c_vp, c_vp, c_vp]
    L.pppcsr_create_local.argtypes = [c_u32, c_int, c_int, c_int, c_u64, c_u64, c_int, ctypes.POINTER(c_vp)]
    L.pppcsr_apply_batch_device.argtypes = [c_vp, c_vp, c_u64]
    L.pppcsr_apply_parts_device.argtypes = [c_vp, c_u64, c_u64, c_vp, c_vp]
    L.pppcsr_comm_unique_id.argtypes = [c_vp]
    L.pppcsr_comm_create.argtypes = [c_vp, c_int, c_int, c_int, ctypes.POINTER(c_vp)]
    L.pppcsr_comm_destroy.argtypes = [c_vp]
    L.pppcsr_exchange_apply.argtypes = [c_vp, c_vp, c_vp, c_u64]
    L.pppcsr_xchg_create.argtypes = [c_vp, c_int, c_int, ctypes.POINTER(c_vp)]
    L.pppcsr_xchg_destroy.argtypes = [c_vp]
    L.pppcsr_xchg_pack.argtypes = [c_vp, c_vp, c_u64, c_vp, ctypes.POINTER(c_vp)]
    L.pppcsr_xchg_layout.argtypes = [c_vp, c_vp, c_vp]
    L.pppcsr_xchg_apply.argtypes = [c_vp]
    L.pppcsr_repartition_export.argtypes = [c_vp, c_vp, ctypes.POINTER(c_vp), ctypes.POINTER(c_u64), ctypes.POINTER(c_vp), ctypes.POINTER(c_u64)]
    L.pppcsr_set_num_neighbors_device.argtypes = [c_vp, c_vp, c_u64]
    L.pppcsr_xchg_set_num_neighbors.argtypes = [c_vp]
    L.pppcsr_xchg_bulk_build.argtypes = [c_vp]
    L.pppcsr_bulk_build_device.argtypes = [c_vp, c_vp, c_u64]
    L.pppcsr_exchange_bulk_build.argtypes = [c_vp, c_vp, c_vp, c_u64]
    L.pppcsr_exchange_set_num_neighbors.argtypes = [c_vp, c_vp, c_vp, c_u64]
    L.pppcsr_repartition.argtypes = [c_vp, c_vp]
    L.pppcsr_balanced_starts.argtypes = [c_vp, c_vp]
    _LIBS[path] = L
    return L


def _ops(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    assert a.ndim == 2 and a.shape[1] == 3, "ops must be (n,3) uint32 rows of (src, dst, op)"
    return a


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _lookup(fn, h, src, dst):
    s, d = _u32(src), _u32(dst)
    assert s.size == d.size, "src and dst must have the same length"
    out = np.empty(s.size, np.uint32)
    return fn(h, s.ctypes.data, d.ctypes.data, s.size, out.ctypes.data), out


def _gather(fn, h, vertices, with_values):
    """(rc, row_offsets, dests, values|None): the size query, then the gather into arrays of that size"""
    q = _u32(vertices)
    rows = np.zeros(q.size + 1, np.uint64)
    tot = c_u64()
    rc = fn(h, q.ctypes.data, q.size, rows.ctypes.data, None, None, 0, ctypes.byref(tot))
    if rc != 0:
        return rc, None, None, None
    dests = np.empty(tot.value, np.int32)
    vals = np.empty(tot.value, np.uint32) if with_values else None
    if tot.value:
        rc = fn(h, q.ctypes.data, q.size, rows.ctypes.data, dests.ctypes.data, vals.ctypes.data if with_values else None, tot.value,
                ctypes.byref(tot))
    return rc, rows, dests, vals


class _Consumers:
    """The device consumers (reference: src/utility/bfs.h, src/utility/pagerank.h; include/ppcsr.h): PCSR calls ppcsr_<name>,
    PPPCSR calls pppcsr_<name> over every partition, with global vertex ids."""
    _prefix = None

    def _consumer(self, name, *args):
        ms = ctypes.c_double(0.0)
        self._chk(getattr(self.L, self._prefix + name)(self.h, *args, ctypes.byref(ms)))
        return ms.value

    def bfs(self, start, with_ms=False):
        out = np.empty(self.get_n(), np.uint32)
        ms = self._consumer("bfs", start, out.ctypes.data)
        return (out, ms) if with_ms else out

    def pagerank(self, node_values, with_ms=False):
        vals = np.ascontiguousarray(node_values, np.float32)
        assert len(vals) == self.get_n()
        out = np.empty(len(vals), np.float32)
        ms = self._consumer("pagerank", vals.ctypes.data, out.ctypes.data)
        return (out, ms) if with_ms else out

    def sssp(self, start, with_ms=False):
        """distances over the edge values from `start` (uint64, NO_PATH where no path leads)"""
        out = np.empty(self.get_n(), np.uint64)
        ms = self._consumer("sssp", start, out.ctypes.data)
        return (out, ms) if with_ms else out

    def components(self, with_ms=False):
        """weakly connected components: the smallest vertex id of every vertex's component (uint32)"""
        out = np.empty(self.get_n(), np.uint32)
        ms = self._consumer("components", out.ctypes.data)
        return (out, ms) if with_ms else out

    def path_counts(self, start, with_ms=False):
        """(levels, sigma[, ms]): BFS levels from `start` (uint32, 0xFFFFFFFF where unreachable) and the number of shortest
        directed paths from `start` to every vertex (float64: exact below 2^53, 0 where unreachable)"""
        levels, sigma = np.empty(self.get_n(), np.uint32), np.empty(self.get_n(), np.float64)
        ms = self._consumer("path_counts", start, levels.ctypes.data, sigma.ctypes.data)
        return (levels, sigma, ms) if with_ms else (levels, sigma)

    def betweenness(self, sources, with_ms=False):
        """Brandes' betweenness from `sources` (float64): directed, endpoints excluded, nothing halved or normalised;
        range(n) as sources gives exact betweenness"""
        q = _u32(sources)
        out = np.empty(self.get_n(), np.float64)
        ms = self._consumer("betweenness", q.ctypes.data if q.size else None, q.size, out.ctypes.data)
        return (out, ms) if with_ms else out

    def triangles(self, per_vertex=True, with_ms=False):
        """(tri, total[, ms]): triangles through every vertex (uint64; None unless per_vertex) and their number, counted in the
        upper orientation ({a, b}, a < b, is an edge exactly when (a, b) is stored: include/ppcsr.h)"""
        tri = np.empty(self.get_n(), np.uint64) if per_vertex else None
        total = c_u64()
        ms = self._consumer("triangles", tri.ctypes.data if per_vertex else None, ctypes.byref(total))
        return (tri, total.value, ms) if with_ms else (tri, total.value)

    def kcore(self, with_ms=False):
        """(core, kmax[, ms]): the core number of every vertex (uint32, global ids) and the largest of them, in the upper
        orientation that triangles() counts in"""
        core = np.empty(self.get_n(), np.uint32)
        kmax = c_u32()
        ms = self._consumer("kcore", core.ctypes.data, ctypes.byref(kmax))
        return (core, kmax.value, ms) if with_ms else (core, kmax.value)

    def colouring(self, order="random", seed=0, with_ms=False):
        """(colour, ncolours[, ms]): greedy colouring of the upper-orientation graph kcore() peels, in the vertex order `order`
        (a key of ORDERS or its number) with `seed`: colour[v] (uint32, global ids) is the smallest colour no preceding
        neighbour carries; ncolours = 1 + the largest"""
        colour = np.empty(self.get_n(), np.uint32)
        ncol = c_u32()
        ms = self._consumer("colouring", ORDERS.get(order, order), seed, colour.ctypes.data, ctypes.byref(ncol))
        return (colour, ncol.value, ms) if with_ms else (colour, ncol.value)

    def mis(self, order="random", seed=0, with_ms=False):
        """(mask, size[, ms]): the lexicographically first maximal independent set of the same graph in the same order: mask[v]
        (bool) iff no preceding neighbour is a member — for one order and seed, mask == (colouring()[0] == 0)"""
        mask = np.empty(self.get_n(), np.uint8)
        size = c_u64()
        ms = self._consumer("mis", ORDERS.get(order, order), seed, mask.ctypes.data, ctypes.byref(size))
        return (mask.astype(bool), size.value, ms) if with_ms else (mask.astype(bool), size.value)

    def label_propagation(self, order="random", seed=0, weighted=False, max_sweeps=0, init=None, with_ms=False):
        """(labels, ncommunities, sweeps[, ms]): label-propagation communities of the graph colouring() colours, class by class of
        colouring(order, seed): a vertex takes the label of largest weight among its neighbours (its own on a tie, else the
        smallest), until a sweep changes nothing or max_sweeps (0: none).  labels (uint32, global ids) start at init (the warm
        start: the previous answer) or at the vertex ids; weighted: an edge counts with its stored value"""
        labels = np.empty(self.get_n(), np.uint32)
        start = None if init is None else np.ascontiguousarray(init, np.uint32)
        if start is not None and len(start) != len(labels):
            raise ValueError("init needs one label per vertex")
        ncom, sweeps = c_u64(), c_u32()
        ms = self._consumer("label_propagation", ORDERS.get(order, order), seed, COMMUNITY_WEIGHTED if weighted else 0, max_sweeps,
                            None if start is None else start.ctypes.data, labels.ctypes.data, ctypes.byref(ncom), ctypes.byref(sweeps))
        return (labels, ncom.value, sweeps.value, ms) if with_ms else (labels, ncom.value, sweeps.value)

    def modularity(self, labels, weighted=False, with_ms=False):
        """(q, words[, ms]): Newman-Girvan modularity of any labels (one per vertex, each below n) in the same graph.  words =
        uint64[4]: 2 W(G), twice the weight inside communities, and the low and high word of the sum of tot_c^2 — exact; q is
        formed from them in doubles"""
        lab = np.ascontiguousarray(labels, np.uint32)
        if len(lab) != self.get_n():
            raise ValueError("modularity needs one label per vertex")
        words = np.zeros(4, np.uint64)
        q = ctypes.c_double()
        ms = self._consumer("modularity", lab.ctypes.data, COMMUNITY_WEIGHTED if weighted else 0, words.ctypes.data, ctypes.byref(q))
        return (q.value, words, ms) if with_ms else (q.value, words)

    def scc(self, with_ms=False):
        """(labels, count[, ms]): strongly connected components of the stored DIRECTED graph: the smallest vertex id of every
        vertex's SCC (uint32, global ids: the convention of components()) and the number of SCCs"""
        labels = np.empty(self.get_n(), np.uint32)
        count = c_u64()
        ms = self._consumer("scc", labels.ctypes.data, ctypes.byref(count))
        return (labels, count.value, ms) if with_ms else (labels, count.value)

    def msf(self, with_ms=False):
        """(edges, weight, labels[, ms]): the minimum spanning forest over the edge values, every stored pair an undirected
        edge: edges[count, 3] uint32 rows (lo, hi, w) ascending by (lo, hi), the sum of their weights (a Python int), and the
        smallest vertex id of every vertex's tree (uint32: what components() returns)"""
        n = self.get_n()
        edges = np.empty((max(n, 1) - 1, 3), np.uint32)  # (a forest has at most n - 1 edges)
        labels = np.empty(n, np.uint32)
        count, weight = c_u64(), c_u64()
        ms = self._consumer("msf", edges.ctypes.data, len(edges), ctypes.byref(count), ctypes.byref(weight), labels.ctypes.data)
        edges = edges[: count.value]
        return (edges, weight.value, labels, ms) if with_ms else (edges, weight.value, labels)

    def _edge_list(self, name, *outputs):
        """the size query (edges = NULL), then the call into an array of that size: (edges[count, 3], ms)"""
        count = c_u64()
        self._consumer(name, None, 0, ctypes.byref(count), *[None] * len(outputs))
        edges = np.empty((count.value, 3), np.uint32)
        ms = self._consumer(name, edges.ctypes.data if count.value else None, count.value, ctypes.byref(count), *outputs)
        return edges[: count.value], ms

    def edge_support(self, with_ms=False):
        """(edges, total[, ms]): edges[count, 3] uint32 rows (a, b, support) of every edge {a, b}, a < b, of the upper-orientation
        graph triangles() counts in, ascending by (a, b) — support = the triangles through the edge — and the number of triangles"""
        total = c_u64()
        edges, ms = self._edge_list("edge_support", ctypes.byref(total))
        return (edges, total.value, ms) if with_ms else (edges, total.value)

    def ktruss(self, with_ms=False):
        """(edges, tmax, vtruss[, ms]): edges[count, 3] uint32 rows (a, b, truss number) in the order of edge_support(), the largest
        truss number (0 without an edge) and, per vertex, the largest truss number of an edge at it (uint32, 0 without one)"""
        vtruss = np.empty(self.get_n(), np.uint32)
        tmax = c_u32()
        edges, ms = self._edge_list("ktruss", ctypes.byref(tmax), vtruss.ctypes.data)
        return (edges, tmax.value, vtruss, ms) if with_ms else (edges, tmax.value, vtruss)

    def common_neighbours(self, a, b, with_ms=False):
        """counts[i] = stored destinations < n that a[i] and b[i] share (uint32; vertices >= n give 0)"""
        a, b = _u32(a), _u32(b)
        assert a.size == b.size, "a and b must have the same length"
        out = np.empty(a.size, np.uint32)
        ms = self._consumer("common_neighbours", a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data)
        return (out, ms) if with_ms else out

    NO_VERTEX = NO_VERTEX

    def sample_neighbours(self, vertices, fanout, seed=0, weighted=False, with_values=False, with_ms=False):
        """uint32[k, fanout]: `fanout` neighbours of every vertex drawn with replacement, uniformly or in proportion to the edge
        values (weighted); draw (seed, i, j) is the counter-based pick of include/ppcsr.h, NO_VERTEX where vertices[i] >= n or has
        no neighbour.  with_values: the picked edges' values beside them (0 beside NO_VERTEX)."""
        q = _u32(vertices)
        out = np.empty((q.size, fanout), np.uint32)
        vals = np.empty((q.size, fanout), np.uint32) if with_values else None
        ms = self._consumer("sample_neighbours", q.ctypes.data, q.size, fanout, seed, 1 if weighted else 0, out.ctypes.data,
                            vals.ctypes.data if with_values else None)
        res = (out, vals) if with_values else (out,)
        res = res + (ms,) if with_ms else res
        return res[0] if len(res) == 1 else res

    def random_walks(self, starts, length, seed=0, weighted=False, with_ms=False):
        """uint32[k, length + 1]: row i starts at starts[i] and takes `length` steps, step t the pick of draw (seed, i, t) among the
        current vertex's neighbours; NO_VERTEX from a vertex >= n or without neighbours on"""
        q = _u32(starts)
        out = np.empty((q.size, length + 1), np.uint32)
        ms = self._consumer("random_walks", q.ctypes.data, q.size, length, seed, 1 if weighted else 0, out.ctypes.data)
        return (out, ms) if with_ms else out

    def degrees(self, weighted=False, with_ms=False):
        """the live out-degree of every vertex (uint32: stored destinations < n), or with weighted the sum of their edge values
        (uint64)"""
        out = np.empty(self.get_n(), np.uint64 if weighted else np.uint32)
        ms = self._consumer("degrees", None if weighted else out.ctypes.data, out.ctypes.data if weighted else None)
        return (out, ms) if with_ms else out

    def multi_bfs(self, sources, levels=False, with_ms=False):
        """(reached, far, ecc, harmonic[, levels][, ms]) from every source at once, 64 sources to a 64-bit word per vertex:
        reached[i] = vertices with a finite level from sources[i], itself included (uint64); far[i] = the sum of their levels
        (uint64); ecc[i] = the largest of them (uint32); harmonic[i] = the sum of 1 / level over the others (float64, added level
        by level: include/ppcsr.h).  levels: row i is bfs(sources[i]) (uint32[k, n]).  The distances are OUT-distances, along
        stored edges away from the source; repeated sources are separate rows."""
        q = _u32(sources)
        k, n = q.size, self.get_n()
        reached, far = np.empty(k, np.uint64), np.empty(k, np.uint64)
        ecc, harm = np.empty(k, np.uint32), np.empty(k, np.float64)
        lv = np.empty((k, n), np.uint32) if levels else None
        ms = self._consumer("multi_bfs", q.ctypes.data if k else None, k, lv.ctypes.data if levels else None, reached.ctypes.data,
                            far.ctypes.data, ecc.ctypes.data, harm.ctypes.data)
        res = (reached, far, ecc, harm) + ((lv,) if levels else ()) + ((ms,) if with_ms else ())
        return res

    def closeness(self, sources):
        """(reached - 1) / far per source (float64), 0 where far == 0: the reciprocal of the mean OUT-distance to the vertices
        the source reaches (for closeness over incoming paths store the transpose)"""
        reached, far, _, _ = self.multi_bfs(sources)
        out = np.zeros(reached.size, np.float64)
        np.divide((reached - np.uint64(1)).astype(np.float64), far.astype(np.float64), out=out, where=far != 0)
        return out


class PCSR(_Consumers):
    """Mirror of the reference class PCSR (PCSR.h:64-124) on one GPU."""
    _prefix = "ppcsr_"

    def __init__(self, init_n, src_n=None, lock_search=True, device=0, lib=None, _handle=None):
        self.L = lib or load_library()
        self._own = _handle is None
        if _handle is not None:
            self.h = c_vp(_handle)
        else:
            self.h = c_vp()
            self._chk(self.L.ppcsr_create(init_n, init_n if src_n is None else src_n, int(lock_search), device,
                                          ctypes.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            raise PpcsrError(f"ppcsr status {rc} ({self.L.ppcsr_strerror(rc).decode()}): "
                             f"{self.L.ppcsr_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None) and self._own and self.h.value:
            self.L.ppcsr_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # reference API names
    def add_edge(self, src, dest, value=1): self._chk(self.L.ppcsr_add_edge(self.h, src, dest, value))
    def remove_edge(self, src, dest): self._chk(self.L.ppcsr_remove_edge(self.h, src, dest))
    def add_node(self): self._chk(self.L.ppcsr_add_node(self.h))

    def edge_exists(self, src, dest):
        out = c_int()
        self._chk(self.L.ppcsr_edge_exists(self.h, src, dest, ctypes.byref(out)))
        return bool(out.value)

    def get_n(self):
        n = c_u64()
        self._chk(self.L.ppcsr_get_n(self.h, ctypes.byref(n)))
        return n.value

    def getNode(self, v):
        out = np.zeros(3, np.uint32)
        self._chk(self.L.ppcsr_get_node(self.h, v, out.ctypes.data))
        return tuple(int(x) for x in out)

    def get_neighbourhood(self, src):
        cnt = c_u64()
        self._chk(self.L.ppcsr_get_neighbourhood(self.h, src, None, 0, ctypes.byref(cnt)))
        out = np.empty(cnt.value, np.int32)
        if cnt.value:
            self._chk(self.L.ppcsr_get_neighbourhood(self.h, src, out.ctypes.data, cnt.value, ctypes.byref(cnt)))
        return out

    def read_neighbourhood(self, src): self._chk(self.L.ppcsr_read_neighbourhood(self.h, src))

    # batched reads (include/ppcsr.h: ppcsr_lookup_edges / ppcsr_gather_neighbourhoods)
    def lookup_edges(self, src, dst):
        """uint32 array: value of edge (src[i], dst[i]), NO_EDGE where edge_exists would say no (src >= n included)"""
        rc, out = _lookup(self.L.ppcsr_lookup_edges, self.h, src, dst)
        self._chk(rc)
        return out

    def edges_exist(self, src, dst):
        return self.lookup_edges(src, dst) != NO_EDGE

    def lookup_edges_device(self, src_ptr, dst_ptr, n, out_ptr):
        """the same on device arrays (uint32, n entries each; e.g. torch tensors' data_ptr())"""
        self._chk(self.L.ppcsr_lookup_edges_device(self.h, src_ptr, dst_ptr, n, out_ptr))

    def gather_neighbourhoods(self, vertices, with_values=True):
        """get_neighbourhood of every vertex as CSR in query order -> (row_offsets uint64[k + 1], dests int32, values uint32 | None)"""
        rc, rows, dests, vals = _gather(self.L.ppcsr_gather_neighbourhoods, self.h, vertices, with_values)
        self._chk(rc)
        return rows, dests, vals

    def gather_neighbourhoods_device(self, vertices_ptr, k, rows_ptr, dests_ptr, values_ptr, cap):
        """device arrays (vertices uint32[k], rows uint64[k + 1], dests int32[cap], values uint32[cap]; pointers may be 0 / None
        as in the C call) -> total edges; raises when cap is too small for them"""
        tot = c_u64()
        self._chk(self.L.ppcsr_gather_neighbourhoods_device(self.h, vertices_ptr, k, rows_ptr or None, dests_ptr or None, values_ptr or None,
                                                            cap, ctypes.byref(tot)))
        return tot.value

    # batch + state
    def apply(self, ops):
        a = _ops(ops)
        if len(a):
            self._chk(self.L.ppcsr_apply_batch(self.h, a.ctypes.data, len(a)))

    def apply_device(self, dev_ptr, n):
        self._chk(self.L.ppcsr_apply_batch_device(self.h, dev_ptr, n))

    def bulk_build(self, ops, with_ms=False):
        """NON-parity fast path: build an empty graph from a list of adds in a few device passes"""
        a = _ops(ops)
        ms = ctypes.c_double(0.0)
        self._chk(self.L.ppcsr_bulk_build(self.h, a.ctypes.data, len(a), ctypes.byref(ms)))
        return ms.value if with_ms else None

    # consumers on the device: _Consumers
    def common_neighbours_device(self, a_ptr, b_ptr, k, out_ptr, with_ms=False):
        """common_neighbours with pairs and counts in this GPU's memory (e.g. tensor.data_ptr())"""
        ms = ctypes.c_double(0.0)
        self._chk(self.L.ppcsr_common_neighbours_device(self.h, a_ptr, b_ptr, k, out_ptr, ctypes.byref(ms)))
        return ms.value if with_ms else None

    def sample_neighbours_device(self, vertices_ptr, k, fanout, dests_ptr, values_ptr=None, seed=0, weighted=False, with_ms=False):
        """sample_neighbours with vertices uint32[k], dests and values uint32[k * fanout] in this GPU's memory (values_ptr may be None)"""
        ms = ctypes.c_double(0.0)
        self._chk(self.L.ppcsr_sample_neighbours_device(self.h, vertices_ptr, k, fanout, seed, 1 if weighted else 0, dests_ptr,
                                                        values_ptr or None, ctypes.byref(ms)))
        return ms.value if with_ms else None

    def random_walks_device(self, starts_ptr, k, length, out_ptr, seed=0, weighted=False, with_ms=False):
        """random_walks with starts uint32[k] and out uint32[k * (length + 1)] in this GPU's memory"""
        ms = ctypes.c_double(0.0)
        self._chk(self.L.ppcsr_random_walks_device(self.h, starts_ptr, k, length, seed, 1 if weighted else 0, out_ptr, ctypes.byref(ms)))
        return ms.value if with_ms else None

    def debug_mulhi(self, a, b):
        """Debugging: the high halves of the 128-bit products a[i] * b[i], computed on the device (ppcsr_debug_mulhi)"""
        a, b = np.ascontiguousarray(a, np.uint64).reshape(-1), np.ascontiguousarray(b, np.uint64).reshape(-1)
        assert a.size == b.size
        out = np.empty(a.size, np.uint64)
        self._chk(self.L.ppcsr_debug_mulhi(self.h, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data))
        return out

    def geometry(self):
        N, lg, H = c_u64(), c_int(), c_int()
        self._chk(self.L.ppcsr_geometry(self.h, ctypes.byref(N), ctypes.byref(lg), ctypes.byref(H)))
        return N.value, lg.value, H.value

    def state(self):
        N, _, _ = self.geometry()
        n = self.get_n()
        items = np.empty((N, 3), np.uint32)
        nodes = np.empty((n, 3), np.uint32)
        self._chk(self.L.ppcsr_export_state(self.h, items.ctypes.data, nodes.ctypes.data if n else None))
        return items, nodes

    def scan_all(self):
        tot = c_u64()
        n = self.get_n()
        rows = np.zeros(n + 1, np.uint64)
        rc = self.L.ppcsr_scan_all(self.h, rows.ctypes.data, None, 0, ctypes.byref(tot))
        if rc not in (0, 6):
            self._chk(rc)
        dests = np.empty(tot.value, np.int32)
        self._chk(self.L.ppcsr_scan_all(self.h, rows.ctypes.data, dests.ctypes.data, tot.value, ctypes.byref(tot)))
        return rows, dests

    def stats(self):
        s = Stats()
        self._chk(self.L.ppcsr_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def set_option(self, key, value): self._chk(self.L.ppcsr_set_option(self.h, key.encode(), int(value)))

    def snapshot(self): self._chk(self.L.ppcsr_snapshot(self.h))
    def restore(self): self._chk(self.L.ppcsr_restore(self.h))

    def debug_snap_counters(self):
        """Debugging (ppcsr_debug_snap_counters): dict of full_saves, full_loads, inc_commits, inc_rollbacks — both snapshots,
        since creation — and leaves_copied, nodes_copied of the last incremental synchronisation (option snap_count = 1)"""
        out = np.zeros(6, np.uint64)
        self._chk(self.L.ppcsr_debug_snap_counters(self.h, out.ctypes.data))
        return dict(zip(("full_saves", "full_loads", "inc_commits", "inc_rollbacks", "leaves_copied", "nodes_copied"), (int(x) for x in out)))

    def debug_multi_bfs_counters(self):
        """Debugging (ppcsr_debug_multi_bfs_counters): uint64[8] of the last multi_bfs call on this engine — groups, level steps,
        streaming edge passes, per-vertex edge launches, passes that finished hubs, largest union frontier, vertex-step launches,
        host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_multi_bfs_counters(self.h, out.ctypes.data))
        return out

    def debug_colouring_counters(self):
        """Debugging (ppcsr_debug_colouring_counters): uint64[8] of the last colouring call on this engine — rounds, the widest
        frontier, vertices left to the long-list kernel, adjacency entries, colours, extra window passes, launches, host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_colouring_counters(self.h, out.ctypes.data))
        return out

    def debug_community_counters(self):
        """Debugging (ppcsr_debug_community_counters): uint64[8] of the last label_propagation call on this engine — sweeps,
        classes, label changes, changes of the last sweep, communities, workgroup-tier vertices, extra hash passes, launches"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_community_counters(self.h, out.ctypes.data))
        return out

    def debug_mis_counters(self):
        """Debugging (ppcsr_debug_mis_counters): uint64[8] of the last mis call on this engine — rounds, streaming passes, members
        and undecided after round 1, size, degree passes, launches, host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_mis_counters(self.h, out.ctypes.data))
        return out

    def debug_scc_counters(self):
        """Debugging (ppcsr_debug_scc_counters): uint64[8] of the last scc call on this engine — vertices trimmed, trim sweeps,
        the pivot (2^64 - 1: none), vertices of its SCC, colouring rounds, vertices coloured, streaming passes, host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_scc_counters(self.h, out.ctypes.data))
        return out

    def debug_msf_counters(self):
        """Debugging (ppcsr_debug_msf_counters): uint64[8] of the last msf call on this engine — rounds, streaming passes,
        pointer-jump launches, the most of them in one round, first-round hooks, forest edges, components, host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_msf_counters(self.h, out.ctypes.data))
        return out

    def debug_ktruss_counters(self):
        """Debugging (ppcsr_debug_ktruss_counters): uint64[8] of the last edge_support / ktruss call on this engine — edges,
        triangles, levels run, sub-rounds, the most of them in one level, the widest frontier, frontier edges handed to the
        long-range kernel, host reads"""
        out = np.zeros(8, np.uint64)
        self._chk(self.L.ppcsr_debug_ktruss_counters(self.h, out.ctypes.data))
        return out

    def check_invariants(self):
        bad = c_u64()
        self._chk(self.L.ppcsr_check_invariants(self.h, ctypes.byref(bad)))
        return bad.value

    def bench_scan_all(self):
        ms, tot = c_dbl(), c_u64()
        self._chk(self.L.ppcsr_bench_scan_all(self.h, ctypes.byref(ms), ctypes.byref(tot)))
        return ms.value, tot.value

    def bench_resize(self, iters=3):
        """(double_list ms, half_list ms): device time per call, the array doubled and halved back `iters` times"""
        d, h = c_dbl(), c_dbl()
        self._chk(self.L.ppcsr_bench_resize(self.h, iters, ctypes.byref(d), ctypes.byref(h)))
        return d.value, h.value

    def bench_rebalance(self, window_slots, iters=5):
        ms = c_dbl()
        self._chk(self.L.ppcsr_bench_rebalance(self.h, window_slots, iters, ctypes.byref(ms)))
        return ms.value

    def debug_chain_probe(self, mode, cases, samples=None, grid=0, want_segs=True):
        """Debugging: the rebalance's position-chain functions run on the device (ppcsr_debug_chain_probe); engine state untouched.
        mode "table" / "published" / "single" / "linear": cases = (index, len, j) rows -> dict with `pos` (list: per case the j
        positions, or one digest per 2^20 ranks when j > 2^22; None where "single" declined), `nseg`, `overflow`, `verdict`
        (single) / `mismatches`, `runs` (linear), `segs` (ncases x 128 x 6), `samples` (list, positions of the ranks asked for
        in `samples`), `wg` (published: ncases x 4 = workgroups, partial-table consumers, fallbacks, fewest segments copied).
        mode "segment": cases = (bits of x, bits of step, S, es) rows -> `segs` (ncases x 6), `steps`, `walk` (list of bit arrays).
        mode "div": cases = (a, b) rows -> `q`, `est`."""
        m = CHAIN_PROBE_MODES[mode]
        width = {4: 4, 5: 2}.get(m, 3)
        cs = np.ascontiguousarray(np.asarray(cases, np.uint64).reshape(-1, width))
        n = len(cs)
        io = ChainProbeIO(mode=m, grid=grid, ncases=n, cases=cs.ctypes.data)
        keep = [cs]
        if m == 5:
            out = np.zeros((n, 2), np.uint64)
            io.pos = out.ctypes.data
            self._chk(self.L.ppcsr_debug_chain_probe(self.h, ctypes.byref(io)))
            return {"q": out[:, 0].copy(), "est": out[:, 1].copy()}
        info = np.zeros((n, 4), np.int32)
        io.info = info.ctypes.data
        if m == 4:
            cnt = np.full(n, CHAIN_PROBE_WALK, np.uint64)
            segs = np.zeros((n, 6), np.uint64)
        else:
            j = cs[:, 2]
            cnt = np.where(j <= CHAIN_PROBE_LITERAL_MAX, j, (j + np.uint64((1 << CHAIN_PROBE_DIGEST_LOG) - 1)) >> np.uint64(CHAIN_PROBE_DIGEST_LOG))
            segs = np.zeros((n, CHAIN_MAX_SEG, 6), np.uint64) if want_segs else None
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        pos = np.zeros(int(off[-1]) if m != 3 else 1, np.uint64)
        io.pos_off, io.pos = off.ctypes.data, pos.ctypes.data
        if segs is not None:
            io.segs = segs.ctypes.data
        wg = np.zeros((n, 4), np.uint32)
        io.wg = wg.ctypes.data
        soff = spos = None
        if samples is not None and m in (0, 1):
            ks = [np.ascontiguousarray(np.asarray(k, np.uint64)) for k in samples]
            soff = np.zeros(n + 1, np.uint64)
            np.cumsum([len(k) for k in ks], out=soff[1:])
            sk = np.concatenate(ks) if n else np.zeros(0, np.uint64)
            if len(sk) == 0:
                sk = np.zeros(1, np.uint64)
            spos = np.zeros(max(int(soff[-1]), 1), np.uint64)
            io.sample_off, io.sample_k, io.sample_pos = soff.ctypes.data, sk.ctypes.data, spos.ctypes.data
            keep += [sk]
        self._chk(self.L.ppcsr_debug_chain_probe(self.h, ctypes.byref(io)))
        if m == 4:
            return {"segs": segs, "steps": info[:, 0].copy(),
                    "walk": [pos[int(off[c]):int(off[c]) + int(info[c, 0])].copy() for c in range(n)]}
        res = {"nseg": info[:, 0].copy(), "overflow": info[:, 1].copy(), "segs": segs}
        if m == 3:
            res["mismatches"], res["runs"] = info[:, 2].copy(), info[:, 3].copy()
            return res
        res["pos"] = [pos[int(off[c]):int(off[c + 1])] for c in range(n)]
        if m == 2:
            res["verdict"] = info[:, 2].copy()
            res["pos"] = [p if v else None for p, v in zip(res["pos"], res["verdict"])]
        if m == 1:
            res["wg"] = wg
        if soff is not None:
            res["samples"] = [spos[int(soff[c]):int(soff[c + 1])] for c in range(n)]
        return res

    def debug_isect_probe(self, mode, cases, items_a, items_b=None, tri_n=None, slot=False):
        """Debugging: the intersection routines of triangles / common_neighbours run alone on the device (ppcsr_debug_isect_probe);
        engine state untouched.  mode "lane" / "wave" / "block": count of {from <= c < n} in both ranges; "lower_bound": the slot;
        "probe": 0 or 1.  cases = (alo, ahi, blo, bhi, from_or_key, n) rows over items_a / items_b ((slots, 3) uint32 arrays of
        (src, dest, value), value 0 = a null; items_b None: both ranges in items_a).  The live dests of every range must ascend:
        asserted here.  tri_n: also return the uint64[tri_n] credits of all cases (intersecting modes) -> (out, tri).  slot
        ("probe" only): the slot that holds the key comes back, 0xFFFFFFFF where none does — the form edge_support / ktruss use."""
        m = ISECT_PROBE_MODES[mode]
        cs = np.ascontiguousarray(np.asarray(cases, np.uint32).reshape(-1, 6))
        ia = np.ascontiguousarray(items_a, np.uint32).reshape(-1, 3)
        ib = ia if items_b is None else np.ascontiguousarray(items_b, np.uint32).reshape(-1, 3)
        for buf, lo, hi in ((ia, cs[:, 0], cs[:, 1]), (ib, cs[:, 2], cs[:, 3])):
            if len(cs) and np.all(lo <= hi) and int(hi.max()) <= len(buf):  # (anything else is the library's to refuse)
                # a descent between two consecutive live slots, by index of the second one; no range may contain one
                live = np.nonzero(buf[:, 2] != 0)[0]
                desc = live[1:][buf[live[1:], 1].astype(np.int64) < buf[live[:-1], 1].astype(np.int64)]
                prev = live[np.searchsorted(live, desc) - 1]
                for q, pq in zip(desc.tolist(), prev.tolist()):
                    assert not np.any((lo <= pq) & (q < hi)), f"live dests of a range descend at slot {q}"
        out = np.zeros(len(cs), np.uint32)
        tri = np.zeros(max(tri_n, 1), np.uint64) if tri_n is not None else None  # (tri_n == 0: the library refuses it)
        io = IsectProbeIO(mode=m, reserved=1 if slot and mode == "probe" else 0, ncases=len(cs), cases=cs.ctypes.data, items_a=ia.ctypes.data, len_a=len(ia),
                          items_b=None if items_b is None else ib.ctypes.data, len_b=0 if items_b is None else len(ib),
                          out=out.ctypes.data, tri=None if tri is None else tri.ctypes.data, tri_n=tri_n or 0)
        self._chk(self.L.ppcsr_debug_isect_probe(self.h, ctypes.byref(io)))
        return (out, tri[:tri_n]) if tri_n is not None else out


class PPPCSR(_Consumers):
    """Mirror of the reference class PPPCSR (PPPCSR.h:11-60): vertex-range partitions, one per GPU."""
    _prefix = "pppcsr_"

    def __init__(self, init_n, src_n=None, lock_search=True, numDomain=1, partitionsPerDomain=1, use_numa=False,
                 devices=None, lib=None, local=None):
        """local=(first_part, n_parts, device): create only that range of the layout's partitions (multi-process runs:
        one rank per GPU holds the partitions of its domain)"""
        self.L = lib or load_library()
        self.h = c_vp()
        if local is not None:
            rc = self.L.pppcsr_create_local(init_n, int(lock_search), numDomain, partitionsPerDomain, local[0], local[1],
                                            local[2], ctypes.byref(self.h))
        else:
            devs = np.array(devices if devices else [0], np.int32)
            rc = self.L.pppcsr_create(init_n, init_n if src_n is None else src_n, int(lock_search), numDomain,
                                      partitionsPerDomain, devs.ctypes.data, len(devs), ctypes.byref(self.h))
        if rc != 0:
            raise PpcsrError(f"pppcsr_create: status {rc}: {self.L.ppcsr_last_error().decode()}")

    def _chk(self, rc):
        if rc != 0:
            raise PpcsrError(f"ppcsr status {rc}: {self.L.ppcsr_last_error().decode()}")

    def close(self):
        if getattr(self, "comm", None) is not None and self.comm.value:
            self.L.pppcsr_comm_destroy(self.comm)
            self.comm = None
        if getattr(self, "xchg", None) is not None and self.xchg.value:
            self.L.pppcsr_xchg_destroy(self.xchg)
            self.xchg = None
        if getattr(self, "h", None) and self.h.value:
            self.L.pppcsr_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_partitions(self):
        out = c_u64()
        self._chk(self.L.pppcsr_num_partitions(self.h, ctypes.byref(out)))
        return out.value

    def get_partiton(self, v):  # sic: the reference's spelling (PPPCSR.h:27)
        out = c_u64()
        self._chk(self.L.pppcsr_get_partition(self.h, v, ctypes.byref(out)))
        return out.value

    def partition_start(self, k):
        out = c_u64()
        self._chk(self.L.pppcsr_partition_start(self.h, k, ctypes.byref(out)))
        return out.value

    def partition(self, k):
        out = c_vp()
        self._chk(self.L.pppcsr_partition(self.h, k, ctypes.byref(out)))
        return PCSR(0, lib=self.L, _handle=out.value)

    def debug_multi_bfs_counters(self):
        """the counters of the last multi_bfs call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_multi_bfs_counters()

    def debug_colouring_counters(self):
        """the counters of the last colouring call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_colouring_counters()

    def debug_community_counters(self):
        """the counters of the last label_propagation call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_community_counters()

    def debug_mis_counters(self):
        """the counters of the last mis call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_mis_counters()

    def debug_scc_counters(self):
        """the counters of the last scc call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_scc_counters()

    def debug_msf_counters(self):
        """the counters of the last msf call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_msf_counters()

    def debug_ktruss_counters(self):
        """the counters of the last edge_support / ktruss call: kept by the engine that ran it, the first partition's"""
        return self.partition(0).debug_ktruss_counters()

    def add_edge(self, s, d, v=1): self._chk(self.L.pppcsr_add_edge(self.h, s, d, v))
    def remove_edge(self, s, d): self._chk(self.L.pppcsr_remove_edge(self.h, s, d))
    def add_node(self): self._chk(self.L.pppcsr_add_node(self.h))

    def edge_exists(self, s, d):
        out = c_int()
        self._chk(self.L.pppcsr_edge_exists(self.h, s, d, ctypes.byref(out)))
        return bool(out.value)

    def get_n(self):
        out = c_u64()
        self._chk(self.L.pppcsr_get_n(self.h, ctypes.byref(out)))
        return out.value

    def getNode(self, v):
        out = np.zeros(3, np.uint32)
        self._chk(self.L.pppcsr_get_node(self.h, v, out.ctypes.data))
        return tuple(int(x) for x in out)

    def get_neighbourhood(self, src):
        cnt = c_u64()
        self._chk(self.L.pppcsr_get_neighbourhood(self.h, src, None, 0, ctypes.byref(cnt)))
        out = np.empty(cnt.value, np.int32)
        if cnt.value:
            self._chk(self.L.pppcsr_get_neighbourhood(self.h, src, out.ctypes.data, cnt.value, ctypes.byref(cnt)))
        return out

    def lookup_edges(self, src, dst):
        rc, out = _lookup(self.L.pppcsr_lookup_edges, self.h, src, dst)
        self._chk(rc)
        return out

    def edges_exist(self, src, dst):
        return self.lookup_edges(src, dst) != NO_EDGE

    def gather_neighbourhoods(self, vertices, with_values=True):
        rc, rows, dests, vals = _gather(self.L.pppcsr_gather_neighbourhoods, self.h, vertices, with_values)
        self._chk(rc)
        return rows, dests, vals

    def set_option(self, key, value):
        """sizes of the batched reads: "query_block", "gather_stage" (include/ppcsr.h: pppcsr_set_option)"""
        self._chk(self.L.pppcsr_set_option(self.h, key.encode(), int(value)))

    def apply(self, ops):
        a = _ops(ops)
        if len(a):
            self._chk(self.L.pppcsr_apply_batch(self.h, a.ctypes.data, len(a)))

    def apply_device(self, dev_ptr, n):
        """global stream resident in HBM (all partitions on that GPU): device bucketing + concurrent per-partition apply"""
        self._chk(self.L.pppcsr_apply_batch_device(self.h, dev_ptr, n))

    # native exchange (RCCL send/recv from the engine library; no torch in the data path)
    @staticmethod
    def comm_unique_id(lib=None):
        L = lib or load_library()
        buf = ctypes.create_string_buffer(128)
        rc = L.pppcsr_comm_unique_id(buf)
        if rc != 0:
            raise PpcsrError(f"pppcsr_comm_unique_id: status {rc}: {L.ppcsr_last_error().decode()}")
        return bytes(buf.raw)

    def comm_create(self, unique_id, n_ranks, rank, device):
        self.comm = c_vp()
        self._chk(self.L.pppcsr_comm_create(ctypes.c_char_p(unique_id), n_ranks, rank, device, ctypes.byref(self.comm)))

    def exchange_apply(self, dev_ptr, n):
        """this rank's block of the global stream (device pointer, n updates): route through RCCL + apply the local partitions"""
        self._chk(self.L.pppcsr_exchange_apply(self.h, self.comm, dev_ptr, n))

    # the same exchange with the transport left to the caller (pack -> [carrier of your choice] -> layout -> apply)
    def xchg_create(self, n_ranks, rank):
        self.xchg = c_vp()
        self._chk(self.L.pppcsr_xchg_create(self.h, n_ranks, rank, ctypes.byref(self.xchg)))
        self._xchg_shape = (n_ranks, self.num_partitions() // n_ranks)

    def xchg_pack(self, dev_ptr, n):
        """-> (send_counts[P], device address of the bucketed block); partition p's rows start at sum(send_counts[:p])"""
        counts = np.zeros(self.num_partitions(), np.uint64)
        d_send = c_vp()
        self._chk(self.L.pppcsr_xchg_pack(self.xchg, dev_ptr, n, counts.ctypes.data, ctypes.byref(d_send)))
        return counts, d_send.value or 0

    def xchg_layout(self, recv_counts):
        """recv_counts[r * ppr + q] -> device addresses the segments (source r, local partition q) must be written to"""
        rc = np.ascontiguousarray(recv_counts, np.uint64)
        assert rc.size == self._xchg_shape[0] * self._xchg_shape[1]
        dst = (c_vp * rc.size)()
        self._chk(self.L.pppcsr_xchg_layout(self.xchg, rc.ctypes.data, dst))
        return [int(x or 0) for x in dst]

    def xchg_apply(self):
        self._chk(self.L.pppcsr_xchg_apply(self.xchg))

    def xchg_set_num_neighbors(self):
        self._chk(self.L.pppcsr_xchg_set_num_neighbors(self.xchg))

    def xchg_bulk_build(self):
        self._chk(self.L.pppcsr_xchg_bulk_build(self.xchg))

    def bulk_build_device(self, dev_ptr, n):
        self._chk(self.L.pppcsr_bulk_build_device(self.h, dev_ptr, n))

    def exchange_bulk_build(self, dev_ptr, n):
        self._chk(self.L.pppcsr_exchange_bulk_build(self.h, self.comm, dev_ptr, n))

    def exchange_set_num_neighbors(self, dev_ptr, n):
        self._chk(self.L.pppcsr_exchange_set_num_neighbors(self.h, self.comm, dev_ptr, n))

    def set_num_neighbors_device(self, dev_ptr, n):
        self._chk(self.L.pppcsr_set_num_neighbors_device(self.h, dev_ptr, n))

    # repartitioning (include/ppcsr.h; no reference equivalent: PCSR.h:91-112 is a sketch)
    def repartition(self, new_starts):
        st = np.ascontiguousarray(new_starts, np.uint64)
        assert st.size == self.num_partitions()
        self._chk(self.L.pppcsr_repartition(self.h, st.ctypes.data))

    def repartition_export(self, new_starts):
        """-> ((device address, n) of the edges on the move as adds of the global stream, (device address, n) of the
        num_neighbors records); route the first into the bulk build of the recreated partitions (bulk_build_device /
        exchange_bulk_build / xchg_bulk_build), then the second through the set_num_neighbors calls"""
        st = np.ascontiguousarray(new_starts, np.uint64)
        assert st.size == self.num_partitions()
        d, n, dn, nn = c_vp(), c_u64(), c_vp(), c_u64()
        self._chk(self.L.pppcsr_repartition_export(self.h, st.ctypes.data, ctypes.byref(d), ctypes.byref(n), ctypes.byref(dn), ctypes.byref(nn)))
        return (d.value or 0, n.value), (dn.value or 0, nn.value)

    def balanced_starts(self):
        st = np.zeros(self.num_partitions(), np.uint64)
        self._chk(self.L.pppcsr_balanced_starts(self.h, st.ctypes.data))
        return st

    def apply_parts_device(self, first_part, dev_ptrs, counts):
        """already routed device-resident subsequences, one per partition of [first_part, first_part + len(counts))"""
        k = len(counts)
        ptrs = (c_vp * k)(*[int(x) for x in dev_ptrs])
        cnts = (c_u64 * k)(*[int(x) for x in counts])
        self._chk(self.L.pppcsr_apply_parts_device(self.h, first_part, k, ptrs, cnts))


def bucket_ops(init_n, n_parts, ops, lib=None):
    """stable owner bucketing (PPPCSR.cpp:46-66 routing rule); returns (bucketed ops with local src, counts)"""
    L = lib or load_library()
    a = _ops(ops)
    out = np.empty_like(a)
    counts = np.zeros(n_parts, np.uint64)
    rc = L.pppcsr_bucket_ops(init_n, n_parts, a.ctypes.data, len(a), out.ctypes.data, counts.ctypes.data)
    if rc != 0:
        raise PpcsrError(f"pppcsr_bucket_ops: status {rc}")
    return out, counts
