"""CPU: the speculative rounds' per-slot rule for duplicate overwrites on the fiber SIMT emulator (tests/hostsim), which compiles
the engine's own kernel and host source.  The checks are the ones tests/test_gpu_dup_slots.py runs on the device
(tests/dup_slot_checks.py)."""
import pytest

import dup_slot_checks as ds
import snap_checks as ck
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim


@pytest.fixture(scope="module")
def env():
    build_sim()
    pkg = load_pkg()
    lib = pkg.load_library(SIM_SO)
    backend = ck.Backend(make=lambda n: pkg.PCSR(n, lib=lib), make_pp=lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=1, lib=lib),
                         to_device=lambda a: (a.ctypes.data, a), opts=ck.SIM_OPTS, rollback_k=300, followup_sched="strict")
    return backend, (lambda n: pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, lib=lib)), pkg.dup_slot_entries(lib)


@pytest.fixture(scope="module")
def backend(env):
    return env[0]


@pytest.fixture
def g16(backend):
    e = ds.g16(backend)
    yield e
    e.close()


def test_sim_distinct_slots_one_round(backend, g16):
    ds.distinct_slots_one_round(backend, g16)


def test_sim_same_slot_stream_order(backend, g16):
    ds.same_slot_stream_order(backend, g16)


@pytest.mark.parametrize("kernel", list(ds.KERNELS))
def test_sim_strong_writers_same_leaves(backend, g16, kernel):
    ds.strong_writers_same_leaves(backend, g16, kernel)


def test_sim_aliased_entries(env, streams):
    ds.aliased_entries(env[0], streams, env[2])


@pytest.mark.parametrize("stream", ["rollbacks", "mixed"])
def test_sim_epochs_and_rollbacks(backend, streams, stream):
    e = ck.build_graph(backend, "mid", streams)
    ds.epochs_and_rollbacks(backend, e, stream)
    e.close()


def test_sim_width_multiples(backend, streams):
    e = ck.build_graph(backend, "big", streams)
    ds.width_multiples(backend, e)
    e.close()


def test_sim_width_multiples_pppcsr(env, streams):
    ds.width_multiples_pppcsr(env[0], env[1], streams)
