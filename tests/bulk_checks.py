"""The driver of the bulk-build tests, shared by tests/test_sim_bulk.py (emulator) and tests/test_gpu_bulk.py (device): every state a
bulk build leaves is compared slot by slot with tests/bulk_model.py, and what follows it with an oracle STARTED FROM THE MODEL (not
from the engine's export), again bit for bit.  No tolerances, no sampling: array_equal on edges[], nodes[] and the geometry."""
import math
from dataclasses import dataclass
from typing import Callable

import numpy as np

import bulk_cases as bc
from bulk_model import bulk_model, survivors
from oracle_lib import Oracle

EINVAL = 1  # PPCSR_EINVAL


@dataclass
class Backend:
    pkg: object
    make: Callable        # (n, lock_search) -> PCSR
    make_pp: Callable     # (n, lock_search, P) -> PPPCSR with P partitions on one device
    tune: Callable        # (PCSR) -> None: the options a partition handle needs before it runs updates (emulator: small horizons)
    to_device: Callable   # rows -> (device address, object that keeps it alive)
    repartition: Callable  # (pp, new_starts) -> None


def first_diff(got, want, what):
    """None, or a message that names the first differing rows"""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, model {want.shape}"
    if np.array_equal(got, want):
        return None
    bad = np.nonzero((got != want).any(1))[0]
    lines = [f"{what}: {len(bad)} of {len(got)} differ, first at {bad[:8].tolist()}"]
    lines += [f"  [{i}] engine {tuple(int(x) for x in got[i])}  model {tuple(int(x) for x in want[i])}" for i in bad[:4]]
    return "\n".join(lines)


def assert_state(eng, items, nodes, geom, label):
    assert tuple(eng.geometry()) == tuple(geom), f"{label}: geometry {eng.geometry()}, model {tuple(geom)}"
    ei, en = eng.state()
    for msg in (first_diff(en, nodes, "nodes[]"), first_diff(ei, items, "edges[]")):
        assert msg is None, f"{label}: {msg}"
    assert eng.check_invariants() == 0, label


def prepare(backend, case, lock, streams, form):
    """the engine of the case just before the call -> (engine, owner to close)"""
    if form == "device":
        pp = backend.make_pp(case.n, lock, 1)
        e, owner = pp.partition(0), pp
    else:
        e = owner = backend.make(case.n, lock)
    backend.tune(e)
    if case.pre == "add_nodes":
        for _ in range(5):
            e.add_node()
    elif case.pre == "grown_shrunk":
        a = bc.grow_stream(streams)
        e.apply(a)
        assert e.geometry()[0] == 8192, e.geometry()
        a[:, 2] = 0
        e.apply(a)
    else:
        assert case.pre is None, case.pre
    return e, owner


def run_case(backend, case, lock, streams, form="host"):
    e, owner = prepare(backend, case, lock, streams, form)
    try:
        n = e.get_n()
        N0 = e.geometry()[0]
        if case.expect_N0 is not None:
            assert N0 == case.expect_N0, (N0, case.expect_N0)
        ops = np.ascontiguousarray(case.ops(streams), np.uint32)
        label = f"{case.name} lock_search={lock} {form}"
        if form == "device":
            ptr, keep = backend.to_device(ops)
            owner.bulk_build_device(ptr, len(ops))
            del keep
        else:
            ms = e.bulk_build(ops, with_ms=True)
            assert math.isfinite(ms) and ms >= 0.0, ms
        mi, mn = bulk_model(n, N0, ops, lock_search=lock)
        o = Oracle.from_state(mi, mn, lock)
        if case.expect_E is not None:
            assert len(survivors(n, ops)[0]) == case.expect_E
        if case.expect_N is not None:
            assert len(mi) == case.expect_N, (len(mi), case.expect_N)
        assert_state(e, mi, mn, o.geometry(), label)
        follow = (case.follow or bc.default_follow)(streams, n)
        e.apply(follow)
        o.apply(follow)
        assert_state(e, *o.state(), o.geometry(), label + ", updates afterwards")
        if case.then is not None:
            more = case.then(streams, n)
            e.apply(more)
            o.apply(more)
            assert o.geometry()[0] == case.then_N, (o.geometry(), case.then_N)
            assert_state(e, *o.state(), o.geometry(), label + ", second stream of updates")
    finally:
        owner.close()


def check_refused(backend, lock, streams):
    """a graph that holds one edge is not bulk-built: EINVAL, and the state is what it was, bit for bit"""
    e = backend.make(300, lock)
    backend.tune(e)
    e.add_edge(299, 5, 7)
    geom, (items, nodes) = e.geometry(), e.state()
    try:
        e.bulk_build(streams.random_stream(300, 2000, seed=5))
        raise AssertionError("bulk_build of a graph that holds an edge was to fail")
    except backend.pkg.PpcsrError as err:
        assert f"status {EINVAL} " in str(err), err
    assert_state(e, items, nodes, geom, "after the refused call")
    e.close()


# ---- partitioned --------------------------------------------------------------------------------------------------------------------
def _starts(pp, P):
    return np.array([pp.partition_start(k) for k in range(P)], np.uint64)


def _owners(starts, src):
    return np.searchsorted(starts, src.astype(np.uint64), side="right") - 1   # (the routing rule: the last partition takes src >= n)


def _tune_all(backend, pp, P):
    for k in range(P):
        backend.tune(pp.partition(k))


def check_pp_direct(backend, P, streams, lock=True):
    """pppcsr_bulk_build_device on P fresh partitions: a partition that receives rows — ignored ones count — equals the model of its
    bucket; one that receives none is not touched (it may hold a graph: pppcsr_repartition leaves the unchanged partitions to this
    rule), so it still is the empty engine the oracle creates.  Updates afterwards are bit-exact against oracles started from the
    expected states.  Then the refusal: a receiving partition that holds an edge fails the call and keeps its state."""
    n = bc.PP_N
    pp = backend.make_pp(n, lock, P)
    _tune_all(backend, pp, P)
    starts = _starts(pp, P)
    sizes = np.diff(np.append(starts, n).astype(np.int64))
    ops, silent = bc.pp_direct_rows(streams, starts)
    own = _owners(starts, ops[:, 0])
    counts = np.bincount(own, minlength=P)
    assert len(silent) >= 1 and all(counts[k] == 0 for k in silent) and counts[1] > 0.55 * len(ops) and counts[P - 1] > 0
    ptr, keep = backend.to_device(ops)
    pp.bulk_build_device(ptr, len(ops))
    parts = []
    for k in range(P):
        fresh = Oracle(int(sizes[k]), lock_search=lock)
        if counts[k]:
            sub = ops[own == k].copy()
            sub[:, 0] -= np.uint32(starts[k])
            o = Oracle.from_state(*bulk_model(int(sizes[k]), fresh.geometry()[0], sub, lock_search=lock), lock)
        else:
            o = fresh
        assert_state(pp.partition(k), *o.state(), o.geometry(), f"P={P}: partition {k} ({counts[k]} rows)")
        parts.append(o)
    upd = streams.random_stream(n, 3000, seed=17, p_delete=0.3)
    pp.apply(upd)
    own = _owners(starts, upd[:, 0])
    for k in range(P):
        sub = upd[own == k].copy()
        sub[:, 0] -= np.uint32(starts[k])
        parts[k].apply(sub)
        assert_state(pp.partition(k), *parts[k].state(), parts[k].geometry(), f"P={P}: partition {k}, updates afterwards")
    pp.close()
    # the refusal
    pp = backend.make_pp(n, lock, P)
    _tune_all(backend, pp, P)
    pp.add_edge(int(starts[1]) + 3, 9, 4)
    held = pp.partition(1)
    geom, (items, nodes) = held.geometry(), held.state()
    try:
        pp.bulk_build_device(ptr, len(ops))
        raise AssertionError("a receiving partition that holds an edge was to fail the call")
    except backend.pkg.PpcsrError as err:
        assert "already holds edges" in str(err), err
    assert_state(pp.partition(1), items, nodes, geom, f"P={P}: the partition that refused")
    pp.close()
    del keep


def check_repartition_shapes(backend, streams, lock=True):
    """pppcsr_repartition to a layout with an empty partition, then with one boundary moved by one vertex (exactly two partitions
    change): helpers.check_repartitioned against the model, updates afterwards against oracles started from the expected states"""
    from helpers import check_repartitioned
    n, P = bc.RP_N, bc.RP_P
    pp = backend.make_pp(n, lock, P)
    _tune_all(backend, pp, P)
    pp.apply(bc.rp_core(streams))
    old = _starts(pp, P)
    for name, new, changes in bc.rp_layouts():
        before = [pp.partition(k).state() for k in range(P)]
        end = lambda st, k: int(st[k + 1]) if k + 1 < P else n
        assert [k for k in range(P) if int(old[k]) != int(new[k]) or end(old, k) != end(new, k)] == changes, name
        backend.repartition(pp, new)
        _tune_all(backend, pp, P)
        assert [pp.partition_start(k) for k in range(P)] == [int(x) for x in new]
        after = [pp.partition(k).state() for k in range(P)]
        want = check_repartitioned(after, before, old, new, n, lock_search=lock)
        parts = [Oracle.from_state(*w, lock) if w is not None else None for w in want]
        upd = streams.random_stream(n, 2500, seed=23 + len(changes), p_delete=0.3)
        pp.apply(upd)
        own = _owners(new, upd[:, 0])
        for k in range(P):
            if parts[k] is None:
                assert not (own == k).any()
                continue
            sub = upd[own == k].copy()
            sub[:, 0] -= np.uint32(new[k])
            parts[k].apply(sub)
            assert_state(pp.partition(k), *parts[k].state(), parts[k].geometry(), f"{name}: partition {k}, updates afterwards")
        old = new
    pp.close()
