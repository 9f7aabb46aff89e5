"""GPU (MI355X): the speculative rounds' per-slot rule for duplicate overwrites.  The checks are the ones
tests/test_sim_dup_slots.py runs on the emulator (tests/dup_slot_checks.py)."""
import pytest

import dup_slot_checks as ds
import snap_checks as ck
from helpers import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    pkg = load_pkg()
    lib = pkg.load_library()  # must be the in-tree HIP build; raises if missing
    backend = ck.Backend(make=lambda n: pkg.PCSR(n), make_pp=lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=1),
                         to_device=None, opts=ck.GPU_OPTS, rollback_k=300, followup_sched="spec")
    return backend, (lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4)), pkg.dup_slot_entries(lib)


@pytest.fixture(scope="module")
def backend(env):
    return env[0]


@pytest.fixture
def g16(backend):
    e = ds.g16(backend)
    yield e
    e.close()


def test_distinct_slots_one_round(backend, g16):
    ds.distinct_slots_one_round(backend, g16)


def test_same_slot_stream_order(backend, g16):
    ds.same_slot_stream_order(backend, g16)


@pytest.mark.parametrize("kernel", list(ds.KERNELS))
def test_strong_writers_same_leaves(backend, g16, kernel):
    ds.strong_writers_same_leaves(backend, g16, kernel)


def test_aliased_entries(env, streams):
    ds.aliased_entries(env[0], streams, env[2])


@pytest.mark.parametrize("stream", ["rollbacks", "mixed"])
def test_epochs_and_rollbacks(backend, streams, stream):
    e = ck.build_graph(backend, "mid", streams)
    ds.epochs_and_rollbacks(backend, e, stream)
    e.close()


def test_width_multiples(backend, streams):
    e = ck.build_graph(backend, "big", streams)
    ds.width_multiples(backend, e)
    e.close()


def test_width_multiples_pppcsr(env, streams):
    ds.width_multiples_pppcsr(env[0], env[1], streams)
