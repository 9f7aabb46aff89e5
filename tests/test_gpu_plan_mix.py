"""GPU (MI355X): the round planner's cases of tests/plan_mix_checks.py — parity with the oracle after every batch; the rounds'
counters are printed (the device's rounds are as narrow as the emulator's, but its adaptive width is its own)."""
import pytest

import plan_mix_checks as pm
import snap_checks as ck
from helpers import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    pkg = load_pkg()
    pkg.load_library()  # must be the in-tree HIP build; raises if missing
    return ck.Backend(make=lambda n: pkg.PCSR(n), make_pp=None, to_device=None, opts=ck.GPU_OPTS, rollback_k=300, followup_sched="spec")


@pytest.mark.parametrize("case", list(pm.CASES))
def test_gpu_plan_mix(backend, case):
    pm.CASES[case](backend)
