"""GPU (MI355X): the intersection routines of pma_intersect.h run alone ON THE DEVICE by PCSR.debug_isect_probe — isect_lane with 64
different cases diverging in a wave, isect_wave in both forms with four waves and four LDS tiles per workgroup, isect_block with
streamed and probed tiles, isect_lower_bound, isect_probe — on slot ranges laid out slot by slot (tests/isect_cases.py: every
length around 32, 64, 1024 and 4096 slots, the 8x ratio from both sides, empty and filtered steps and tiles, the merge cursor's
seams), against numpy; then a constructed graph of 4000 vertices whose exported layout is shown to reach every route and every
seam of the glue code (triangles_model.routes), against the triangle and common-neighbour models.  Every comparison is exact;
the largest buffer is 2^16 slots and every test is a handful of launches."""
import numpy as np
import pytest

import isect_checks as ck
import isect_graphs as ig
from helpers import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.load_library()  # the in-tree HIP build; raises if missing
    return p


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.PCSR(64)
    yield e
    e.close()


@pytest.mark.parametrize("mode", ["lane", "wave", "block"])
def test_isect_counts(eng, mode):
    """counts and tri credits of every case, operands as given and exchanged"""
    assert ck.check_intersect(eng, mode) >= 300


@pytest.mark.parametrize("mode", ["lane", "wave", "block"])
def test_isect_one_buffer(eng, mode):
    ck.check_one_buffer(eng, mode)


def test_isect_lower_bound(eng):
    assert ck.check_lower_bound(eng) >= 200


def test_isect_probe(eng):
    assert ck.check_probe(eng) >= 200


def test_isect_probe_refuses_bad_cases(pkg, eng):
    """EINVAL from the host side — ranges that leave their buffer, lo > hi, tri with n == 0 or short of a case's n, an unknown mode —
    so that a bad case cannot become a device fault; the engine answers correctly afterwards"""
    ck.check_einval(pkg, eng)
    assert ck.check_probe(eng) >= 200


@pytest.fixture(scope="module")
def device_tensors():
    """torch's own start on the device (the graph is bulk-built from a device tensor), once for the module"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [1, 3])
def test_isect_graph(pkg, streams, device_tensors, P):
    """the constructed graph on the device: the route model's conditions on the layout, triangles and per-route common-neighbour
    pairs against the models"""
    pp = ig.build(pkg, None, streams, P)
    rt = ig.check(pp, f"P={P}")
    print(f"P={P}", rt)
    pp.close()
