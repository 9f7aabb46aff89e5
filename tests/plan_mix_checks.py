"""Checks of the round planner (o_plan: dev::plan_op and the reservations behind it) at the smallest shapes at which its parts can
still go wrong (tests/test_sim_plan_mix.py on the emulator, tests/test_gpu_plan_mix.py on the device).

The planner keeps what is the same in all 64 lanes of a wave partly in scalar and partly in vector registers (wv::uni / wv::vec)
and branches on it without EXEC-mask regions; which register file a value lives in must not change a single plan.  Every case is
a PCSR of 64 or 1024 vertices and at most a few thousand updates, run through the speculative rounds and compared with the
oracle after every batch: geometry, every slot of edges[], every nodes[] triple.  What a case is there for — a two-leaf window,
a slide past the window, more than eight sentinels inside the write range, a climb of several levels through the retry and the
"no information" paths — is asserted on the ORACLE alone (its per-update counters and state, PathTrace), so that a case cannot
quietly stop exercising its path.  Every case returns the rounds' own counters (rounds, planned, committed, rollbacks): on the
emulator they are pinned to tests/golden/plan_mix_pin.json, recorded before the planner's instruction mix was touched — a plan
whose footprint changed shows there even where the final state happens to agree.

Nothing here depends on the backend: the test files hand in a snap_checks.Backend."""
import json
import os

import numpy as np

import snap_checks as ck
from helpers import GOLDEN
from oracle_lib import STAT_FIELDS, Oracle

PIN = os.path.join(GOLDEN, "plan_mix_pin.json")
COUNTERS = ("rounds", "planned", "committed", "rollbacks")
SENT = 0xFFFFFFFF
K_HEAD_RANGES = 6  # dev::kHeadRanges: read ranges that travel in the plan record's header


def load_pin():
    with open(PIN) as f:
        return json.load(f)


# ---- the oracle as a witness -------------------------------------------------------------------------------------------------
class PathTrace:
    """the updates of a stream applied ONE BY ONE to a clone of oracle `o` (o itself untouched): per update the deltas of the
    oracle's counters (d[name][i]) and, with states=True, what the update moved: the changed slots' range (lo[i], hi[i]; lo > hi:
    none), whether the first slot of the leaf at `lo` held a sentinel before, and how many sentinels at or below / above src moved"""

    def __init__(self, o, ops, states=False):
        c = o.clone()
        self.geom = c.geometry()
        logN = self.geom[1]
        prev = c.stats()
        rows = []
        self.lo, self.hi, self.first_sent, self.below, self.above = [], [], [], [], []
        it0, nd0 = c.state() if states else (None, None)
        for op in np.asarray(ops, np.uint32):
            c.apply(op[None, :])
            s = c.stats()
            rows.append([s[k] - prev[k] for k in STAT_FIELDS])
            prev = s
            if states:
                it1, nd1 = c.state()
                same = c.geometry() == self.geom and len(nd1) == len(nd0)
                ch = np.nonzero((it1 != it0).any(1))[0] if same else np.zeros(0, np.int64)
                self.lo.append(int(ch[0]) if len(ch) else 1)
                self.hi.append(int(ch[-1]) if len(ch) else 0)
                ws = (int(ch[0]) // logN) * logN if len(ch) else 0
                self.first_sent.append(bool(len(ch)) and int(it0[ws, 1]) == SENT and int(it0[ws, 2]) != 0)
                mv = (nd1[:, 0] != nd0[:, 0]) if same else np.zeros(len(nd1), bool)
                src = int(op[0])
                self.below.append(int(mv[:src + 1].sum()) if src < len(mv) else 0)
                self.above.append(int(mv[src + 1:].sum()) if src < len(mv) else 0)
                it0, nd0, self.geom = it1, nd1, c.geometry()
        self.final_geom = c.geometry()
        c.close()
        a = np.array(rows, np.int64).reshape(len(rows), len(STAT_FIELDS))
        self.d = {k: a[:, i] for i, k in enumerate(STAT_FIELDS)}


def set_options(e, backend, **more):
    for k, v in {**backend.opts, "mode": 1, **more}.items():
        e.set_option(k, v)


def run_batches(e, o, batches, label):
    """the batches on the engine (speculative rounds) and on the oracle, the whole comparison after each -> the rounds' counters"""
    s0 = e.stats()
    for i, ops in enumerate(batches):
        ops = np.ascontiguousarray(ops, np.uint32)
        e.apply(ops)
        o.apply(ops)
        oi, on = o.state()
        ck.assert_same(e, o.geometry(), o.get_n(), oi, on, f"{label}: batch {i}")
    s1 = e.stats()
    d = {k: int(s1[k] - s0[k]) for k in COUNTERS + ("exclusive_ops", "duplicates", "not_found", "noops")}
    print(f"{label}: {sum(len(b) for b in batches)} updates in {len(batches)} batches, {d}")
    assert d["rounds"] > 0, f"{label}: the batches were to go through the rounds"
    return {k: d[k] for k in COUNTERS}


def loaded(backend, n, ops):
    """an engine of n vertices with `ops` applied (strict schedule), and an oracle started from its exported state"""
    e = backend.make(n)
    for k, v in {**backend.opts, "mode": 0}.items():
        e.set_option(k, v)
    if len(ops):
        e.apply(np.ascontiguousarray(ops, np.uint32))
    set_options(e, backend)
    return e, Oracle.from_state(*e.state())


def adds(src, dst, val=None):
    src = np.asarray(src, np.int64)
    val = np.ones(len(src), np.int64) if val is None else np.asarray(val, np.int64)
    return np.stack([src, np.asarray(dst, np.int64), val], 1).astype(np.uint32)


def random_load(n, m, seed, dmax=1 << 20):
    rng = np.random.default_rng(seed)
    return adds(rng.integers(0, n, m), rng.integers(0, dmax, m), 1 + rng.integers(0, 1000, m))


def split(ops, k):
    return [b for b in np.array_split(np.asarray(ops, np.uint32), k) if len(b)]


# ---- 1: every kind in one stream ---------------------------------------------------------------------------------------------
def every_kind(backend, n=64, label="kinds"):
    """inserts, overwrites (one edge seven times in a row, others once), removes, deletes of edges that are not there, and adds /
    deletes whose source is no vertex (src >= n), shuffled into one stream of 1 500 updates over a graph of 600 edges"""
    base = random_load(n, 600, seed=11)
    e, o = loaded(backend, n, base)
    rng = np.random.default_rng(12)
    fresh = random_load(n, 500, seed=13)
    fresh[:, 1] |= 1 << 21  # (dests the load cannot hold)
    over = base[rng.choice(len(base), 300, replace=False)].copy()
    over[:, 2] = 2000 + np.arange(len(over))
    hot = np.repeat(base[:1], 7, axis=0)
    hot[:, 2] = 3000 + np.arange(7)
    gone = base[rng.choice(len(base), 300, replace=False)].copy()
    gone[:, 2] = 0
    missing = adds(rng.integers(0, n, 200), (1 << 22) + rng.integers(0, 1000, 200), np.zeros(200))
    outside = adds(n + rng.integers(0, 5, 193), rng.integers(0, 1000, 193), rng.integers(0, 2, 193))
    parts = np.concatenate([fresh, over, gone, missing, outside])
    stream = parts[rng.permutation(len(parts))]
    stream = np.insert(stream, np.sort(rng.integers(0, len(stream), 7)), hot, axis=0)
    assert len(stream) == 1500
    t = PathTrace(o, stream)
    assert t.d["duplicates"].sum() >= 7 and t.d["not_found"].sum() >= 200 and t.d["ops_del"].sum() >= 500, f"{label}: the stream lost a kind"
    assert (t.d["redistribute_calls"] == 2).sum() > 0  # removes that found their edge
    out = run_batches(e, o, split(stream, 3), label)
    o.close()
    e.close()
    return out


# ---- 2: the ends of the node-record lanes ------------------------------------------------------------------------------------
def first_and_last_vertex(backend, n, label=None):
    """updates of src = 0 and src = n - 1 only (plan_op reads the node records of src - 7 .. src + 8 in one batch: both ends of
    that stretch fall off the array), on an otherwise empty graph: the window of vertex 0 starts at slot 0, the one of n - 1
    ends on the array's last leaf"""
    label = label or f"ends/n{n}"
    e, o = loaded(backend, n, np.zeros((0, 3), np.uint32))
    rng = np.random.default_rng(21)
    src = np.where(rng.integers(0, 2, 400) == 0, 0, n - 1)
    ins = adds(src, rng.permutation(4000)[:400], 1 + np.arange(400))
    dele = ins[rng.choice(400, 150, replace=False)].copy()
    dele[:, 2] = 0
    stream = np.concatenate([ins[:250], np.concatenate([ins[250:], dele])[rng.permutation(300)]])
    t = PathTrace(o, stream[:100], states=True)
    at0 = [i for i in range(100) if stream[i, 0] == 0 and t.lo[i] < t.geom[1] and t.d["redistribute_calls"][i] > 0]
    print(f"{label}: geometry {t.geom}; {len(at0)} of vertex 0's first inserts rebalance a window that starts at slot 0")
    assert at0, f"{label}: none of vertex 0's first inserts rebalanced the leaf at slot 0"
    out = run_batches(e, o, split(stream, 2), label)
    o.close()
    e.close()
    return out


# ---- 3: full leaves, slides -------------------------------------------------------------------------------------------------
def full_leaves_and_slides(backend, n=64, label="slides"):
    """1 200 inserts into a graph of 64 vertices at a density where leaves fill up and slots are taken: among them inserts whose
    leaf becomes exactly full (one rebalance of a two-leaf window), with and without a slide, and slides that end in the leaf
    behind the one the insert rebalances (the gap lies in the next leaf: beyond the one-leaf window)"""
    e, o = loaded(backend, n, random_load(n, 900, seed=31))
    stream = random_load(n, 1200, seed=32)
    logN = o.geometry()[1]
    t = PathTrace(o, stream, states=True)
    lo, hi = np.array(t.lo), np.array(t.hi)
    same_N = (t.d["double_calls"] == 0) & (lo <= hi)
    two_leaf = same_N & (t.d["redistribute_calls"] == 1) & (t.d["redistribute_slots"] == 2 * logN)
    one_leaf = same_N & (t.d["redistribute_calls"] == 1) & (t.d["redistribute_slots"] == logN)
    slid = t.d["slide_steps"] > 0
    beyond = one_leaf & slid & (hi // logN > lo // logN)
    print(f"{label}: leaves of {logN} slots; two-leaf windows {two_leaf.sum()} ({(two_leaf & slid).sum()} with a slide), "
          f"slides into the leaf behind a one-leaf window {beyond.sum()}, slides {slid.sum()}")
    assert (two_leaf & ~slid).sum() > 0 and (two_leaf & slid).sum() > 0 and beyond.sum() > 0, f"{label}: the stream lost a path"
    out = run_batches(e, o, split(stream, 3), label)
    o.close()
    e.close()
    return out


# ---- 4: isolated vertices: many sentinels inside the write range -------------------------------------------------------------
def sentinel_runs(backend, n=1024, label="sentinels"):
    """1 024 vertices without edges stand sentinel beside sentinel; inserts into a few vertices in the middle of that run rebalance
    windows that move more than eight sentinels below and more than eight above `src` (the node records plan_op holds in registers
    reach eight either way: both extension loops run), among them windows whose first slot holds a sentinel (which stays)"""
    e, o = loaded(backend, n, np.zeros((0, 3), np.uint32))
    rng = np.random.default_rng(41)
    hubs = np.array([300, 301, 302, 640, 641, 900])
    stream = adds(hubs[rng.integers(0, len(hubs), 360)], rng.permutation(5000)[:360], 1 + np.arange(360))
    t = PathTrace(o, stream, states=True)
    below, above, first = np.array(t.below), np.array(t.above), np.array(t.first_sent)
    print(f"{label}: most sentinels moved below {below.max()} / above {above.max()}; windows starting on a sentinel {first.sum()}")
    assert ((below > 8) & (above > 8)).sum() > 0, f"{label}: no update moved more than eight sentinels on both sides"
    assert first.sum() > 0, f"{label}: no window started on a sentinel"
    out = run_batches(e, o, split(stream, 3), label)
    o.close()
    e.close()
    return out


# ---- 5: a dense small array --------------------------------------------------------------------------------------------------
def dense_climbs(backend, n=64, label="dense"):
    """a graph of 64 vertices filled to just under its next doubling: the climbs take several levels, some through the
    reference's retry path into the "no information" plan (the oracle's global_path), and the largest windows span 32 leaves or
    more — one read range per level, more than the plan record's header holds"""
    e, o = loaded(backend, n, random_load(n, 1500, seed=51))
    more = random_load(n, 4000, seed=52)
    t = PathTrace(o, more)
    dbl = np.nonzero(t.d["double_calls"] > 0)[0]
    assert len(dbl) >= 2, f"{label}: the fill was to reach two doublings"
    # from just behind one doubling to just in front of the next
    stream = more[:dbl[-1]]
    t = PathTrace(o, stream)
    logN = t.final_geom[1]
    last = slice(int(np.nonzero(t.d["double_calls"] > 0)[0][-1]) + 1, None)
    widest = int(t.d["redistribute_slots"][last].max())
    levels = int(np.log2(max(widest - logN, 1) // logN))
    print(f"{label}: {len(stream)} inserts, geometry {t.final_geom}; global_path {t.d['global_path'].sum()}, widest window {widest} slots ({levels} levels)")
    assert t.d["global_path"].sum() > 0, f"{label}: no insert went through the retries into the no-information plan"
    assert levels + 2 > K_HEAD_RANGES, f"{label}: no climb recorded more than {K_HEAD_RANGES} read ranges"
    out = run_batches(e, o, split(stream, 4), label)
    o.close()
    e.close()
    return out


# ---- 6: a mixed stream over many rounds --------------------------------------------------------------------------------------
def mixed_rounds(backend, n=1024, label="mixed"):
    """4 000 inserts and deletes (half and half, deletes of edges present and absent) over 1 024 vertices with a skewed choice of
    sources, in rounds of at most backend.opts["opt_horizon"] updates: dozens of rounds, and on average more than one update per
    round that has to wait for an earlier one"""
    base = random_load(n, 3000, seed=61)
    e, o = loaded(backend, n, base)
    rng = np.random.default_rng(62)
    src = (n * rng.random(2000) ** 3).astype(np.int64)  # (skewed: the low vertices meet in every round)
    ins = adds(src, (1 << 21) + rng.permutation(1 << 16)[:2000], 1 + np.arange(2000))
    dele = np.concatenate([base[rng.choice(len(base), 1500, replace=False)], random_load(n, 500, seed=63, dmax=1 << 19)])
    dele[:, 2] = 0
    stream = np.concatenate([ins, dele])[rng.permutation(4000)]
    out = run_batches(e, o, split(stream, 2), label)
    assert out["rounds"] >= 4000 // backend.opts["opt_horizon"], f"{label}: {out}"
    assert out["planned"] - out["committed"] >= out["rounds"], f"{label}: fewer deferred updates than rounds: {out}"
    o.close()
    e.close()
    return out


CASES = {
    "kinds": every_kind,
    "ends-n64": lambda b: first_and_last_vertex(b, 64),
    "ends-n1024": lambda b: first_and_last_vertex(b, 1024),
    "slides": full_leaves_and_slides,
    "sentinels": sentinel_runs,
    "dense": dense_climbs,
    "mixed": mixed_rounds,
}
