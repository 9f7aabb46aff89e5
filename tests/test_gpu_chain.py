"""GPU (MI355X): the arithmetic every rebalance places its elements with, run ON THE DEVICE by PCSR.debug_chain_probe — the table
build with the reciprocal-estimate division, the in-launch hand-off of the table from workgroup 0 to the others over a POISONED
buffer, the one-segment closed form, the linear runs, single segments with forced round-to-even ties, the division alone — and
held to the oracle's serial fp64 chain (PCSR.cpp:237-247), the host build of the same table and exact integer models.  Every
comparison is exact.  The cases (tests/chain_cases.py) all lie in the domain where the reference's chain is a placement."""
import numpy as np
import pytest

import chain_cases as cc
import chain_checks as ck
from helpers import load_pkg
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

MAX_LG = 28
PUBLISHED = dict(workgroups=0, partial=0, fallbacks=0, cases_with_partial=0, cases=0)  # summed over the module's published runs


@pytest.fixture(scope="module")
def eng():
    pkg = load_pkg()
    pkg.load_library()  # the in-tree HIP build; raises if missing
    e = pkg.PCSR(64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    return cc.window_cases(MAX_LG)[0]


def test_table_on_device_matches_oracle_and_host_table(eng, cases):
    """build_chain_table + chain_pos on the device == the oracle's chain for every case; segment words == the host build's; no
    overflow, and the largest table stays below kMaxSeg: the truncated-table path is unreachable inside the reference's domain"""
    assert any(c[1] == 1 << MAX_LG and c[2] > cc.LITERAL_MAX for c in cases)
    tot = ck.check_windows(eng, cases, "table")
    assert tot["cases"] == len(cases)
    print(f"table: {tot['cases']} cases, largest table {tot['max_nseg']} segments")
    assert tot["max_nseg"] < cc.MAX_SEG


def _add(tot):
    for k in PUBLISHED:
        PUBLISHED[k] += tot[k]


def test_published_table_first_and_second_launch(eng, cases):
    """the hand-off of k_rb_scatter (build_chain_table_publish + rb_table_to_lds), every case launched twice — the buffer poisoned
    before each launch, so a workgroup that copies a segment before its words have landed expands garbage"""
    sub = ck.published_cases(cases)
    assert len(sub) >= 100 and sum(1 for c in sub if c[1] >= 1 << 26) >= 30
    for rnd in (1, 2):
        tot = ck.check_windows(eng, sub, "published", label=f"launch {rnd}: ", literal_ranges=(rnd == 1))
        print(f"published launch {rnd}: {tot}")
        _add(tot)


def test_published_table_oversubscribed_grid(eng, cases):
    """a grid of 16384 workgroups — several times what is resident at once — whatever the window holds: the late workgroups find
    the table complete, the early ones do not"""
    sub = ck.published_cases(cases)
    tot = ck.check_windows(eng, sub, "published", grid=16384, label="grid 16384: ", literal_ranges=False)
    print(f"published, 16384 workgroups: {tot}")
    _add(tot)


def test_published_mode_met_partial_tables():
    """what keeps the two tests above honest (they must have run): some workgroup other than the builder went ahead with a PART of
    the table — otherwise the hand-off was never exercised — and the bounded-spin fallback, which the code says never happens,
    stayed below 1 % of the workgroups"""
    print(f"published, whole module: {PUBLISHED}")
    assert PUBLISHED["cases"] > 0, "the published tests did not run"
    assert PUBLISHED["partial"] > 0, PUBLISHED
    assert PUBLISHED["fallbacks"] * 100 <= PUBLISHED["workgroups"], PUBLISHED


def test_single_segment_closed_form(eng, cases):
    assert ck.check_single(eng, cases) > len(cases) // 2


def test_linear_runs(eng, cases):
    assert ck.check_linear(eng, cases) > 1_000_000


def test_segments_with_forced_ties(eng):
    assert ck.check_segments(eng, cc.segment_cases()) >= 52 * 2 * 4


def test_division_quotient_and_estimate_error(eng, cases):
    """div_floor_u53 == a // b for the operands of every window case and for the constructed ones; the reciprocal estimate's
    largest error — the trip count of the fix-up loops — is printed for both sets (the figures recorded above div_estimate_u53
    in pma_geometry.h)"""
    window = cc.div_operands_of(cases)
    assert len(window) > 10000
    err, at = ck.check_div(eng, window)
    print(f"div, window operands: {len(window)} pairs, quotients up to {max(a // b for a, b in window)}, "
          f"largest |estimate - quotient| = {err} at (a, b) = {at}")
    pairs = cc.div_cases(cases)
    err, at = ck.check_div(eng, pairs)
    print(f"div, all operands: {len(pairs)} pairs, largest |estimate - quotient| = {err} at (a, b) = {at} (quotient {at[0] // at[1]})")


def _same(e, o, label):
    assert e.geometry() == o.geometry(), label
    ei, en = e.state()
    oi, on = o.state()
    np.testing.assert_array_equal(en, on, err_msg=label + " nodes")
    np.testing.assert_array_equal(ei, oi, err_msg=label + " items")


def test_deferred_table_rebalance_end_to_end(streams):
    """the real kernels at the sizes where the table is built inside the scatter launch BY DEFAULT: windows from slot 0 of 2^22, 2^23
    and 2^24 slots of one 2^24-slot array (the partial ones through the scratch array: that is the pipeline with the hand-off), the
    fill changed between the calls so that consecutive rebalances do not rewrite the same table, against the oracle's redistribute()"""
    pkg = load_pkg()
    scale = 20
    n = 1 << scale
    s, d = streams.rmat_edges(scale, 10_000_000, seed=1)
    base = streams.adds(s, d)
    e = pkg.PCSR(n)
    e.bulk_build(base)
    N = e.geometry()[0]
    assert N == 1 << 24
    o = Oracle.from_state(*e.state())
    e.set_option("rb_inplace_min", 0)
    uniq = np.unique(base[:, :2], axis=0)
    for rnd, w in enumerate((N, N >> 1, N >> 2, N)):
        e.bench_rebalance(w, 1)
        o.debug_redistribute(0, w)
        _same(e, o, f"window {w}")
        cut = uniq[rnd::37][:60000]  # another slice of the edges leaves (or, last round, returns)
        ops = np.concatenate([cut, np.zeros((len(cut), 1), np.uint32)], axis=1).astype(np.uint32)
        e.apply(ops)
        o.apply(ops)
        _same(e, o, f"deletions after window {w}")
    assert e.check_invariants() == 0
    e.close()
