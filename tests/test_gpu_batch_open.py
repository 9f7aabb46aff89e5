"""GPU (MI355X): how a batch opens — the restore shortcut (the user's snapshot as the first epoch's rollback point) against the
full-copy model on every write path, and the one launch that opens an epoch.  The checks are the ones
tests/test_sim_batch_open.py runs on the emulator (tests/batch_open_checks.py)."""
import pytest

import batch_open_checks as bo
import snap_cases as sc
import snap_checks as ck
from helpers import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    pkg = load_pkg()
    pkg.load_library()  # must be the in-tree HIP build; raises if missing
    # (set_num_neighbors takes device memory: copied there through the runtime the engine library holds already)
    import ctypes

    import numpy as np
    from helpers import hip_runtime
    hip = hip_runtime()
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
    backend = ck.Backend(make=lambda n: pkg.PCSR(n), make_pp=lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=1),
                         to_device=to_device, opts=ck.GPU_OPTS, rollback_k=300, followup_sched="spec")
    return backend, (lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4))


@pytest.fixture(scope="module")
def backend(env):
    return env[0]


@pytest.fixture(scope="module")
def drivers(backend, streams):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ck.Driver(backend, ck.build_graph(backend, name, streams))
        return cache[name]
    yield get
    for d in cache.values():
        d.e.close()


def _sched(w):
    return w.scheds[-1]  # ("spec" where the scenario has it)


@pytest.mark.parametrize("name", [w.name for w in sc.ROW_1_2_5])
@pytest.mark.parametrize("graph", ["tiny", "mid", "big"])
def test_restore_shortcut_leaf_sizes(drivers, graph, name):
    w = sc.BY_NAME[name]
    bo.s_r_w_b_r(drivers(graph), w, f"{graph}/{name}", _sched(w))


@pytest.mark.parametrize("name", [w.name for w in sc.ROW_3_4 + sc.SEAM])
def test_restore_shortcut_in_step_writers(drivers, name):
    w = sc.BY_NAME[name]
    bo.s_r_w_b_r(drivers("mid"), w, f"mid/{name}", _sched(w))


@pytest.mark.parametrize("name", [w.name for w in sc.ROW_6_7])
def test_restore_shortcut_wholesale_rewrites(backend, streams, name):
    w = sc.BY_NAME[name]
    d = ck.Driver(backend, ck.build_graph(backend, "mid", streams))
    bo.s_r_w_b_r(d, w, f"mid/{name}", _sched(w))
    d.e.close()


def test_restore_shortcut_set_num_neighbors(backend, streams):
    e, pp = ck.build_graph(backend, "mid", streams, pp=True)
    bo.s_r_w_b_r(ck.Driver(backend, e, pp), sc.SET_NN, "mid/set_nn", "strict")
    pp.close()


@pytest.mark.parametrize("graph", ["tiny", "mid", "big"])
def test_restore_shortcut_itself_first_epoch(drivers, graph):
    """no write between R and B; the rollback falls into the batch's first epoch"""
    bo.s_r_w_b_r(drivers(graph), None, f"{graph}/shortcut")


def test_restore_shortcut_itself_second_epoch(drivers):
    """epochs of 2 048 updates in batches of 3 000: the second epoch brings the epoch snapshot up to date from its old position"""
    bo.s_r_w_b_r(drivers("big"), None, "big/shortcut-2048", epoch_ops=2048, k=1500)


def test_batch_without_rollback_then_restores(drivers):
    bo.no_rollback_then_r_r(drivers("mid"), "mid/no-rollback")


def test_restore_batch_snapshot_write_restore(drivers):
    bo.r_b_s_w_r(drivers("mid"), "mid/R;B;S;W;R")


def test_doubling_after_full_load(backend, streams):
    d = ck.Driver(backend, ck.build_graph(backend, "mid", streams))
    bo.doubling_after_full_load(d, "mid/doubling")
    d.e.close()


def test_strict_small_batch_then_b(drivers):
    bo.strict_small_then_b(drivers("mid"), "mid/small")


def test_pppcsr_four_partitions(env, streams):
    bo.pppcsr_s_r_b(env[0], env[1], streams)


@pytest.mark.parametrize("rollback_first", [False, True])
@pytest.mark.parametrize("graph", ["tiny", "mid", "g257", "g513"])
def test_epoch_opening_back_to_back(backend, streams, graph, rollback_first):
    """n + 1 = 3, 301, 258 and 514 words of sentinel stamps (none a multiple of 4), 8 to 512 leaves; tiny: N = 64, n = 2"""
    e = ck.build_graph(backend, graph, streams)
    bo.back_to_back(backend, e, f"{graph}/back-to-back", rollback_first)
    e.close()


def test_epoch_opening_two_vertices_from_empty(backend):
    """a fresh engine of two vertices: the smallest arrays there are (fewer than four leaves), growing batch by batch"""
    e = backend.make(2)
    bo.back_to_back(backend, e, "n2/back-to-back")
    e.close()


@pytest.mark.parametrize("stream", bo.CHUNK_STREAMS)
def test_chunk_boundaries(backend, streams, stream):
    """rounds_per_sync 2, opt_horizon 1 024, 20 000 updates on the big graph, speculative rounds: dozens of chunk boundaries"""
    e = ck.build_graph(backend, "big", streams)
    bo.chunk_boundaries(backend, e, stream)
    e.close()


@pytest.mark.parametrize("rps", [32, 4096])
def test_chunk_boundaries_calm_long_chunks(backend, streams, rps):
    e = ck.build_graph(backend, "big", streams)
    bo.chunk_boundaries(backend, e, "calm", rounds_per_sync=rps)
    e.close()
