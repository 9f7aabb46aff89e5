"""GPU (MI355X): ppcsr_snapshot / ppcsr_restore and the epochs' rollback point against a full host copy, on every write path of the
engine.  The scenarios, the driver and the model are the ones tests/test_sim_snapshot.py runs on the emulator (tests/snap_cases.py,
tests/snap_checks.py): every restore must land byte for byte on the state exported at the snapshot, through the path (incremental
or whole-array) the scenario names, having copied at least what differs, and a follow-up batch must stay bit-exact against an
oracle started from that export.  One case more than the emulator's: 2^20 + 300 vertices, where k_snap_sync_nodes takes a second
trip with the shipped grid."""
import numpy as np
import pytest

import snap_cases as sc
import snap_checks as ck
from helpers import hip_runtime, load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    pkg = load_pkg()
    pkg.load_library()  # must be the in-tree HIP build; raises if missing

    import ctypes
    hip = hip_runtime()  # (the runtime the engine library holds already)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]

    class DeviceCopy:
        def __init__(self, a):
            self.p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(self.p), max(a.nbytes, 1)) == 0
            assert hip.hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

        def __del__(self):
            hip.hipFree(self.p)

    def to_device(a):
        d = DeviceCopy(np.ascontiguousarray(a))
        return d.p.value, d
    return ck.Backend(make=lambda n: pkg.PCSR(n), make_pp=lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=1),
                      to_device=to_device, opts=ck.GPU_OPTS, rollback_k=300, followup_sched="spec")


@pytest.fixture(scope="module")
def drivers(backend, streams):
    """one loaded engine per graph, shared by the tests of this file: every scenario starts with its own snapshot and ends with
    a restore, so each finds a graph of the size it was loaded with"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ck.Driver(backend, ck.build_graph(backend, name, streams))
        return cache[name]
    yield get
    for d in cache.values():
        d.e.close()


def fresh(backend, streams, name="mid"):
    return ck.Driver(backend, ck.build_graph(backend, name, streams))


def _ids(ws):
    return [(w.name, s) for w in ws for s in w.scheds]


@pytest.mark.parametrize("form", sc.FORMS)
@pytest.mark.parametrize("name,sched", _ids(sc.ROW_1_2_5))
@pytest.mark.parametrize("graph", ["tiny", "mid", "big"])
def test_snapshot_leaf_sizes(drivers, graph, name, sched, form):
    """single operations, a batch and rebalances that change tags only, at leaves of 8, 16 and 32 slots (8, 4 and 2 leaves per trip
    of the sync kernel; the tiny graph has fewer than 64 leaves: the partial-wave mask)"""
    d = drivers(graph)
    assert d.e.geometry()[1] == {"tiny": 8, "mid": 16, "big": 32}[graph]
    d.run(sc.BY_NAME[name], form, sched, b_may_resize=(graph == "tiny"))


@pytest.mark.parametrize("form", sc.FORMS)
@pytest.mark.parametrize("name,sched", _ids(sc.ROW_3_4))
def test_snapshot_in_step_writers(drivers, name, sched, form):
    """batches with rollbacks inside, workgroup rebalances and exclusive updates, in-place partial windows, the workgroup routine"""
    drivers("mid").run(sc.BY_NAME[name], form, sched)


@pytest.mark.parametrize("form", sc.FORMS)
@pytest.mark.parametrize("name,sched", _ids(sc.ROW_6_7))
def test_snapshot_wholesale_rewrites(backend, streams, name, sched, form):
    """resizes (also back to the same N), bench_resize, add_node: a new generation of the arrays, the whole-array path"""
    d = fresh(backend, streams)
    n0 = d.e.get_n()
    d.run(sc.BY_NAME[name], form, sched)
    if name == "add_nodes" and form != "commit":
        assert d.e.get_n() == n0
        with pytest.raises(load_pkg().PpcsrError):
            d.e.getNode(n0)
    d.e.close()


def test_snapshot_empty_graph_bulk_build(backend, streams):
    """snapshot of an EMPTY graph, bulk_build, restore: the graph is empty again, so a second bulk_build succeeds; restore again"""
    ck.check_empty_bulk(backend, streams)


def test_snapshot_set_num_neighbors(backend, streams):
    """pppcsr_set_num_neighbors_device on a one-partition PPPCSR whose partition handle took the snapshot: node records only"""
    e, pp = ck.build_graph(backend, "mid", streams, pp=True)
    d = ck.Driver(backend, e, pp)
    for form in sc.FORMS:
        d.run(sc.SET_NN, form, "strict")
    pp.close()


def test_snapshot_control_flow(backend, drivers, streams):
    """R; R — S; S (the second commit copies nothing) — R; W; S; W; R — restore before any snapshot is EINVAL"""
    ck.check_control_flow(backend, drivers("mid"), load_pkg())


@pytest.mark.parametrize("grid", [1, 3, 4096])
@pytest.mark.parametrize("form", sc.FORMS)
@pytest.mark.parametrize("name", [w.name for w in sc.SEAM])
@pytest.mark.parametrize("graph", ["g256", "g257", "g513"])
def test_snapshot_grid_stride(drivers, graph, name, form, grid):
    """snap_grid 1 and 3: one workgroup covers 256 leaves or 256 vertices per trip, the arrays hold 512 leaves and 256, 257 and
    513 vertices; writes at the first and the last leaf / vertex and at every leaf.  The default grid gives the same result
    (every run is compared with the same full-copy model); it runs with the counting off, i.e. with the launches as shipped."""
    d = drivers(graph)
    assert d.e.geometry() == (8192, 16, 9) or d.e.geometry()[0] >= 8192
    w = sc.BY_NAME[name]
    d.run(w, form, w.scheds[0], snap_grid=grid, snap_count=0 if grid == 4096 else 1)


@pytest.mark.parametrize("seed", sc.CAMPAIGN_SEEDS)
def test_snapshot_campaign(backend, streams, seed):
    """scripts of 12 steps drawn from {the writes, S, R}: every R is checked like the scenarios' """
    d = fresh(backend, streams)
    ck.run_campaign(d, seed)
    d.e.close()


def test_snapshot_second_trip_of_the_node_sync(backend, streams):
    """n = 2^20 + 300 vertices: the shipped grid of k_snap_sync_nodes (4096 workgroups of 256) covers 2^20 of them per trip.  Edges
    added at vertices 0, 2^20 - 1, 2^20 and n - 1 after the snapshot; restore form, default grid"""
    n = (1 << 20) + 300
    e = backend.make(n)
    d = ck.Driver(backend, e)
    d.reset_options("spec")
    base = streams.random_stream(n, 60000, seed=3)
    base[:, 1] = streams.uniform_ints(4, len(base), sc.FRESH_LO)
    base[:, 2] = 1
    d.apply(base)
    where = np.array([0, (1 << 20) - 1, 1 << 20, n - 1], np.uint32)
    w = sc.W("second_trip", lambda c: [("apply", c.fresh(np.repeat(where, 3)))], "step", ("spec",))
    d.count(True)
    d.snapshot("second trip: S")
    before = d.rec
    d.write(w, "second trip")
    touched = ck.diff_nodes(before.nodes, ck.Rec(e).nodes)
    assert set(where.tolist()) <= set(touched.tolist())
    d.restore("second trip", path="step")
    e.close()
