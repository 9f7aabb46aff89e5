"""CPU: the device probe of the rebalance position chain (PCSR.debug_chain_probe) under the emulator, on the cases the GPU module
runs (windows of at most 2^24 slots here), so that the probe, its digests and the shared comparisons are themselves tested before
they reach a GPU.  The emulator runs workgroups one after another: in `published` mode every consumer finds the table complete, so
this checks the plumbing and the steps each workgroup asks for, not the race.  Its division takes the exact branch, so the integer
fix-up is fed wrong estimates through a hook of its own."""
import ctypes

import numpy as np
import pytest

import chain_cases as cc
import chain_checks as ck
from helpers import load_pkg
from test_sim_engine import SIM_SO, build_sim

SIM_MAX_LG = 24


@pytest.fixture(scope="module")
def eng():
    build_sim()
    pkg = load_pkg()
    return pkg.PCSR(64, lib=pkg.load_library(SIM_SO))


@pytest.fixture(scope="module")
def cases():
    return cc.window_cases(SIM_MAX_LG)[0]


def test_cases_are_in_the_reference_domain():
    """the generator's verdicts, pinned from the oracle alone: the listed cases rise strictly inside their windows, the dropped
    candidates (and the windows named when the domain was found) collide or leave the window"""
    ok, out = cc.window_cases(SIM_MAX_LG)
    assert len(set(cc.small_exhaustive_candidates()) - set(ok)) == 0  # all 4064 small windows are in the domain
    assert len(cc.small_exhaustive_candidates()) == 4064
    for c in ok[::97] + [c for c in ok if c[1] >= 1 << 30]:
        assert cc.domain_status(c) == 0
        if c[2] <= 1 << 20:
            p = cc.oracle_positions(*c).astype(np.int64)
            assert p[0] == c[0] and (np.diff(p) > 0).all() and p[-1] < c[0] + c[1], c
    for c in out:
        assert cc.domain_status(c) != 0, c
        if c[2] <= cc.LITERAL_MAX:
            p = cc.oracle_positions(*c).astype(np.int64)
            assert not ((np.diff(p) > 0).all() and p[-1] < c[0] + c[1]), c
    for c in cc.KNOWN_OUT_OF_DOMAIN:
        assert cc.domain_status(c) != 0, c
    assert cc.domain_status((0, 1 << 29, 331804423)) & 4 and cc.domain_status((0, 1 << 30, 805306368)) & 4  # x goes negative
    # no family is lost to the domain: every window length keeps dense cases
    for lg in range(3, SIM_MAX_LG + 1):
        assert any(c[1] == 1 << lg and 2 * c[2] >= c[1] for c in ok), lg


def test_oracle_digest_is_the_digest_of_the_oracle_positions():
    """po_redistribute_positions_digest == the digest of po_redistribute_positions' output (numpy restatement), block by block, and
    its literal ranges are slices of it; one position moved by one slot, or two swapped, change the digest"""
    for c in [(0, 1 << 22, 3_000_000), (3 << 21, 1 << 21, 1 << 21), (0, 8, 1), (0, 8, 8), (1 << 30, 1 << 30, 2_100_000)]:
        pos = cc.oracle_positions(*c)
        ranges = [(0, min(5, c[2]))] + ([(10, 1000), (c[2] - 7, c[2])] if c[2] > 2000 else [])
        st, dig, lit = cc.oracle_digest(*c, ranges)
        assert st == 0
        for b in range(len(dig)):
            lo = b << cc.DIGEST_LOG
            assert int(dig[b]) == cc.digest_of_positions(pos[lo:lo + (1 << cc.DIGEST_LOG)], lo), (c, b)
        np.testing.assert_array_equal(lit[:sum(b - a for a, b in ranges)], np.concatenate([pos[a:b] for a, b in ranges]))
    pos = cc.oracle_positions(0, 4096, 3000)
    d0 = cc.digest_of_positions(pos)
    moved, swapped = pos.copy(), pos.copy()
    moved[1234] += 1
    swapped[[10, 11]] = swapped[[11, 10]]
    assert cc.digest_of_positions(moved) != d0 and cc.digest_of_positions(swapped) != d0


def test_sim_probe_table(eng, cases):
    tot = ck.check_windows(eng, cases, "table")
    assert tot["cases"] == len(cases) and tot["max_nseg"] < cc.MAX_SEG
    print(f"table: {tot['cases']} cases, largest table {tot['max_nseg']} segments")


def test_sim_probe_published(eng, cases):
    sub = ck.published_cases(cases)
    assert len(sub) >= 50 and any(c[1] == 1 << SIM_MAX_LG for c in sub)
    tot = ck.check_windows(eng, sub, "published")
    assert tot["fallbacks"] == 0 and tot["workgroups"] >= 64 * len(sub)
    ck.check_windows(eng, sub[::9], "published", grid=100)  # a grid that does not divide the ranks evenly


def test_sim_probe_single(eng, cases):
    assert ck.check_single(eng, cases) > len(cases) // 2


def test_sim_probe_linear(eng, cases):
    assert ck.check_linear(eng, cases) > 100000


def test_sim_probe_segment(eng):
    rows = cc.segment_cases()
    assert ck.check_segments(eng, rows) >= 52 * 2 * 4


def test_sim_probe_div(eng, cases):
    pairs = cc.div_cases(cases)
    err, at = ck.check_div(eng, pairs)
    assert err == 0, (err, at)  # (the emulator divides exactly; the GPU module measures the reciprocal's error)


def test_sim_div_fixup_from_wrong_estimates(cases):
    """div_floor_fixup(a, b, estimate) == a // b for estimates off by 0 ... 4096 in either direction (clamped at 0 and at the largest
    quotient whose product with b stays below 2^63, the fix-up's precondition)"""
    build_sim()
    lib = ctypes.CDLL(SIM_SO)
    lib.ppcsr_sim_div_fixup.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    pairs = cc.div_cases(cases)
    ab = np.array(pairs, np.uint64)
    want = np.array([a // b for a, b in pairs], np.uint64)
    out = np.zeros(len(pairs), np.uint64)
    for e in (0, 1, 2, 127, 128, 4096):
        for above in (0, 1):
            out[:] = 0xFFFFFFFFFFFFFFFF
            lib.ppcsr_sim_div_fixup(ab.ctypes.data, len(pairs), e, above, out.ctypes.data)
            np.testing.assert_array_equal(out, want, err_msg=f"estimate off by {e} ({'above' if above else 'below'})")
