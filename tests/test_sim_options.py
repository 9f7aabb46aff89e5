"""CPU: what ppcsr_set_option accepts and refuses, on the emulator build of the engine's own host source (tests/hostsim).  The
checks are the ones tests/test_gpu_options.py runs on the device (tests/option_checks.py)."""
import pytest

import option_checks as oc
import snap_checks as ck
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim


@pytest.fixture(scope="module")
def make():
    build_sim()
    pkg = load_pkg()
    lib = pkg.load_library(SIM_SO)
    return lambda n: pkg.PCSR(n, lib=lib)


def test_sim_option_return_codes(make):
    oc.return_codes(make)


def test_sim_batch_after_option_calls(make, streams):
    oc.return_codes(make)
    oc.batch_after(make, {**ck.SIM_OPTS, "mode": 1}, streams)
