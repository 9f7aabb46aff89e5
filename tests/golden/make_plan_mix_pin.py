#!/usr/bin/env python3
"""Records tests/golden/plan_mix_pin.json: rounds / planned / committed / rollbacks of every case of tests/plan_mix_checks.py on
the emulator.  Run it on the commit whose plans are the yardstick, BEFORE a change to the planner — never to make a test pass."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import plan_mix_checks as pm  # noqa: E402
import snap_checks as ck  # noqa: E402
from helpers import load_pkg  # noqa: E402
from test_sim_engine import SIM_SO, build_sim  # noqa: E402

build_sim()
pkg = load_pkg()
lib = pkg.load_library(SIM_SO)
backend = ck.Backend(make=lambda n: pkg.PCSR(n, lib=lib), make_pp=None, to_device=None, opts=ck.SIM_OPTS, rollback_k=300, followup_sched="strict")
pin = {name: case(backend) for name, case in pm.CASES.items()}
with open(pm.PIN, "w") as f:
    json.dump(pin, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(pin, indent=1))
