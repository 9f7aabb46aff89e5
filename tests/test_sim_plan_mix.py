"""CPU: the round planner's cases of tests/plan_mix_checks.py on the fiber SIMT emulator (tests/hostsim), which compiles the
engine's own kernel and host source — every case with the emulator's check of the wave-uniformity claims (wv::uni / wv::vec /
wv::bcast) switched on, and with the rounds' counters pinned to tests/golden/plan_mix_pin.json."""
import pytest

import plan_mix_checks as pm
import snap_checks as ck
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim


@pytest.fixture(scope="module")
def env():
    build_sim()
    pkg = load_pkg()
    lib = pkg.load_library(SIM_SO)
    backend = ck.Backend(make=lambda n: pkg.PCSR(n, lib=lib), make_pp=None, to_device=None, opts=ck.SIM_OPTS, rollback_k=300, followup_sched="strict")
    return backend, lib


@pytest.mark.parametrize("case", list(pm.CASES))
def test_sim_plan_mix(env, case):
    backend, lib = env
    lib.ppcsr_sim_check_uniform(1)
    try:
        got = pm.CASES[case](backend)
    finally:
        lib.ppcsr_sim_check_uniform(0)
    assert got == pm.load_pin()[case], f"{case}: the rounds' counters moved: a plan's footprint changed"
