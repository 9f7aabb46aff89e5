"""GPU (MI355X): ppcsr_bulk_build and what is built on it (pppcsr_bulk_build_device, pppcsr_repartition) against the exact host model
of tests/bulk_model.py.  The scenarios and the driver are the ones tests/test_sim_bulk.py runs on the emulator (tests/bulk_cases.py,
tests/bulk_checks.py): edges[], nodes[] and the geometry must equal the model's bit for bit, and updates applied afterwards must
stay bit-exact against an oracle started from the model.  What only the device has: the radix sort over 32 + bits(n) key bits (n =
1023, 1024, 1025), up to 16 host threads that bulk-build their partitions at once (P = 32), and three large cases — 2^20 + 1 rows
(the tile-sum kernel of the flag scan takes a second tile per thread), 2^21 + 3000 rows and 2^21 + 777 vertices (a second trip of
the grid-stride loops of k_bb_keys / k_bb_flags / k_bb_edges and of k_bb_vertices)."""
import numpy as np
import pytest

import bulk_cases as bc
import bulk_checks as ck
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
    return ck.Backend(pkg=pkg, make=lambda n, lock: pkg.PCSR(n, lock_search=lock),
                      make_pp=lambda n, lock, P: pkg.PPPCSR(n, lock_search=lock, numDomain=1, partitionsPerDomain=P),
                      tune=lambda e: None, to_device=to_device, repartition=lambda pp, new: pp.repartition(new))


@pytest.mark.parametrize("name,lock,form", bc.single_params(bc.SMALL))
def test_bulk_case(backend, streams, name, lock, form):
    ck.run_case(backend, bc.BY_NAME[name], lock, streams, form)


@pytest.mark.parametrize("name,lock,form", bc.single_params(bc.LARGE))
def test_bulk_large_case(backend, streams, name, lock, form):
    ck.run_case(backend, bc.BY_NAME[name], lock, streams, form)


@pytest.mark.parametrize("lock", [True, False])
def test_bulk_refused_on_a_graph_with_one_edge(backend, streams, lock):
    ck.check_refused(backend, lock, streams)


@pytest.mark.parametrize("P", [4, 32])
def test_pp_bulk_build_device(backend, streams, P):
    ck.check_pp_direct(backend, P, streams)


def test_repartition_empty_partition_and_one_vertex_shift(backend, streams):
    ck.check_repartition_shapes(backend, streams)
