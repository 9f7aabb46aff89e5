"""Checks of how a batch opens (tests/test_sim_batch_open.py on the emulator, tests/test_gpu_batch_open.py on the device):

  * the restore shortcut: while the live state equals the user's snapshot (restore() or snapshot() came last, nothing wrote
    since) the first speculative epoch takes that snapshot for its rollback point and copies nothing.  Model: the full host copy
    of tests/snap_checks.py and the oracle.  S; R; W; B; compare; R; compare for every write path W of tests/snap_cases.py — a W
    that does not clear the fact leaves B's rollback on a stale copy;
  * the one launch that opens an epoch (stamp clears, stat-shard copy, control block): batches back to back without a restore,
    on arrays whose word counts are no multiples of four.

Nothing here depends on the backend: the test files hand in a snap_checks.Backend."""
import numpy as np

import snap_cases as sc
import snap_checks as ck
from oracle_lib import Oracle, OraclePPPCSR


def _oracle_of(e):
    r = ck.Rec(e)
    return Oracle.from_state(r.items, r.nodes)


def _same_as_oracle(e, o, label):
    oi, on = o.state()
    ck.assert_same(e, o.geometry(), o.get_n(), oi, on, label)


def b_options(d, epoch_ops, **more):
    for k, v in {**ck.B_OPTS, "region_slots": min(256, d.b.opts["region_slots"]), "epoch_ops": epoch_ops, **more}.items():
        d.e.set_option(k, v)


def rollback_b(d, label, epoch_ops=None, k=None, seed=9):
    """B: the rollback recipe on the live state, mirrored on an oracle started from it; the engine must roll back at least once
    and end on the oracle's state.  epoch_ops None: the length of a batch (the rollback falls into the batch's first epoch)"""
    e = d.e
    k = k or d.b.rollback_k
    b_options(d, epoch_ops or 2 * k)
    o = _oracle_of(e)
    r0 = e.stats()["rollbacks"]
    for ops in sc.rollback_batches(ck.Rec(e).ctx(seed, k)):
        d.apply(ops)
        o.apply(ops)
        if e.stats()["rollbacks"] > r0:
            break
    assert e.stats()["rollbacks"] > r0, f"{label}: B was to roll an epoch back"
    _same_as_oracle(e, o, label + ": after B")
    o.close()


def s_r_w_b_r(d, w, label, sched="spec", epoch_ops=None, k=None, seed=0):
    """S; R; W; B; compare; R; compare (w None: the shortcut itself)"""
    d.reset_options(sched)
    d.count(True)
    d.snapshot(label + ": S")
    d.restore(label + ": R", followup=False)
    if w is not None:
        d.write(w, label + ": W", seed)
    rollback_b(d, label, epoch_ops, k)
    d.restore(label + ": last R", followup=False)
    d.restore(label + ": back", followup=False)


def no_rollback_then_r_r(d, label):
    """S; R; B without a rollback — one epoch, no commit of the epoch snapshot: nothing counted — then R; R"""
    e = d.e
    d.reset_options("spec")
    d.count(True)
    d.snapshot(label + ": S")
    d.restore(label + ": R", followup=False)
    e.set_option("epoch_ops", 1 << 20)
    e.set_option("epoch_short", 1 << 20)
    batch = sc.neutral_batch(d.rec.ctx(3, d.b.rollback_k), 128)
    o = _oracle_of(e)
    c0, s0 = d.ctr(), e.stats()
    d.apply(batch)
    c1, s1 = d.ctr(), e.stats()
    o.apply(batch)
    _same_as_oracle(e, o, label + ": after B")
    o.close()
    for key in ("rollbacks", "double_calls", "half_calls"):
        assert s1[key] == s0[key], f"{label}: the neutral batch was to run as one epoch: {key} {s0[key]} -> {s1[key]}"
    assert c1["inc_commits"] == c0["inc_commits"] and c1["full_saves"] == c0["full_saves"], f"{label}: a skipped commit is not a commit: {c0} -> {c1}"
    e.set_option("epoch_short", 16384)
    d.restore(label + ": R1", path="step", followup=False)
    d.restore(label + ": R2", path="step", followup=False)
    c = d.ctr()
    assert (c["leaves_copied"], c["nodes_copied"]) == (0, 0), c


def r_b_s_w_r(d, label):
    """R; B; S; W; R"""
    d.reset_options("spec")
    d.count(True)
    d.snapshot(label + ": S0")
    d.restore(label + ": R", followup=False)
    rollback_b(d, label)
    d.reset_options("spec")
    d.snapshot(label + ": S")
    d.write(sc.BY_NAME["batch"], label + ": W", seed=4)
    d.restore(label + ": last R")
    d.restore(label + ": back", followup=False)


def doubling_after_full_load(d, label):
    """S; B1; R; B2 where both double the array: the restore takes the full-load path, and B2 changes the generation inside an
    epoch that started from the user's snapshot"""
    e = d.e
    d.reset_options("spec")
    d.count(True)
    d.snapshot(label + ": S")
    for rep in (1, 2):
        o = _oracle_of(e)
        ops = sc.w_doubling_batch(ck.Rec(e).ctx(20 + rep, d.b.rollback_k))[0][1]
        s0, s1 = d.apply(ops)
        o.apply(ops)
        assert s1["double_calls"] > s0["double_calls"], f"{label}: B{rep} was to double the array"
        _same_as_oracle(e, o, f"{label}: after B{rep}")
        o.close()
        d.restore(f"{label}: R after B{rep}", path="full", followup=(rep == 2))
    d.restore(label + ": back", followup=False)


def strict_small_then_b(d, label):
    """R, a batch of at most 256 updates (the strict rounds: no epoch snapshot), then B"""
    e = d.e
    d.reset_options("spec", small_batch=256)
    d.count(True)
    d.snapshot(label + ": S")
    d.restore(label + ": R", followup=False)
    small = sc.neutral_batch(d.rec.ctx(6, d.b.rollback_k), 64)
    assert len(small) <= 256
    o = _oracle_of(e)
    d.apply(small)
    o.apply(small)
    _same_as_oracle(e, o, label + ": after the small batch")
    o.close()
    rollback_b(d, label)
    d.restore(label + ": last R", followup=False)
    d.restore(label + ": back", followup=False)


def pppcsr_s_r_b(backend, make_pp4, streams, label="pppcsr"):
    """the PPPCSR form, 4 partitions on one device: S; R on every partition, B through the PPPCSR, against the oracle's partitions"""
    n, _ = sc.GRAPHS["mid"]
    pp = make_pp4(n)
    P = pp.num_partitions()
    assert P == 4
    parts = [pp.partition(k) for k in range(P)]
    opp = OraclePPPCSR(n, num_domains=1, parts_per_domain=4)
    for e in parts:
        for k, v in {**backend.opts, "mode": 0}.items():
            e.set_option(k, v)
    load = sc.graph_ops("mid", streams)
    pp.apply(load)
    opp.apply(load)
    recs = []
    for e in parts:
        for k, v in {**backend.opts, **ck.B_OPTS, "epoch_ops": 1 << 20, "region_slots": min(256, backend.opts["region_slots"])}.items():
            e.set_option(k, v)
        e.snapshot()
        recs.append(ck.Rec(e))
    rng = np.random.default_rng(31)
    for rep in range(2):
        for e in parts:
            e.restore()
        # adds into four adjacent vertices of every partition, then their deletes (snap_cases.rollback_batches, per partition)
        rows = []
        for k in range(P):
            lo = pp.partition_start(k)
            src = lo + rng.integers(0, 4, backend.rollback_k)
            d = sc.FRESH_LO + rng.choice(sc.FRESH_LO, backend.rollback_k, replace=False)
            rows.append(np.stack([src, d, 1 + rng.integers(0, 1000, backend.rollback_k)], 1).astype(np.uint32))
        add = sc.interleave(*rows)
        dele = add[rng.permutation(len(add))].copy()
        dele[:, 2] = 0
        batch = np.concatenate([add, dele])
        pp.apply(batch)
        opp.apply(batch)
        for k, e in enumerate(parts):
            _same_as_oracle(e, opp.partition(k), f"{label}: partition {k} after B {rep}")
        # (every batch leaves the edge set as it found it; the oracle keeps what the batch did to num_neighbors and the layout,
        #  the engine goes back: the next round starts the oracle's partitions over from the records)
        for k, e in enumerate(parts):
            e.restore()
            r = recs[k]
            ck.assert_same(e, r.geom, r.n, r.items, r.nodes, f"{label}: partition {k} after R {rep}")
        if rep == 0:
            opp.close()
            opp = OraclePPPCSR(n, num_domains=1, parts_per_domain=4)
            opp.apply(load)
    print(f"{label}: rollbacks per partition {[e.stats()['rollbacks'] for e in parts]}")
    opp.close()
    pp.close()


# ---- epoch opening ------------------------------------------------------------------------------------------------------------
def back_to_back(backend, e, label, rollback_first=False, seed=1):
    """two different batches one after the other on one engine, no restore in between: stale stamps of the first would defer or
    roll back updates of the second — the state must be the oracle's.  rollback_first: the first batch is the rollback recipe"""
    d = ck.Driver(backend, e)
    d.reset_options("spec")
    o = _oracle_of(e)
    c = ck.Rec(e).ctx(seed, backend.rollback_k)
    if rollback_first:
        b_options(d, 2 * backend.rollback_k)
        r0 = e.stats()["rollbacks"]
        for ops in sc.rollback_batches(c):
            e.apply(ops)
            o.apply(ops)
            if e.stats()["rollbacks"] > r0:
                break
        assert e.stats()["rollbacks"] > r0, f"{label}: the first batch was to roll an epoch back"
        _same_as_oracle(e, o, label + ": after the rollback batch")
    k = max(8, min(600, len(c.ex)))
    for rep in range(2):
        src = c.rng.integers(0, c.n, k)
        batch = c.fresh(src)
        if rep == 1:  # the second batch deletes half of the first and overwrites the rest
            prev[: k // 2, 2] = 0
            prev[k // 2:, 2] += 1
            batch = sc.interleave(batch, prev)
        prev = batch.copy()
        e.apply(batch)
        o.apply(batch)
        _same_as_oracle(e, o, f"{label}: after batch {rep}")
    o.close()


# ---- chunk boundaries (look-ahead group) ----------------------------------------------------------------------------------------
CHUNK_STREAMS = ("calm", "big_windows", "rollbacks", "doubling", "mixed")
CHUNK_UPDATES = 20000


def chunk_boundaries(backend, e, stream, rounds_per_sync=2, label=None):
    """20 000 updates on the `big` graph in chunks of `rounds_per_sync` rounds with rounds of at most 1 024 updates (dozens of chunk
    boundaries at 2: every one re-sizes the grid and may move max_horizon, which must never exceed the launched grid — device
    error 77).  Every stream ends bit-exact against the oracle with as many updates committed as the oracle applied."""
    label = label or f"{stream}/rps{rounds_per_sync}"
    for k, v in {**backend.opts, "mode": 1, "rounds_per_sync": rounds_per_sync, "opt_horizon": 1024}.items():
        e.set_option(k, v)
    c = ck.Rec(e).ctx(77, CHUNK_UPDATES // 2)
    o = _oracle_of(e)
    M = CHUNK_UPDATES
    need = None
    if stream == "calm":
        batches = [c.fresh(c.rng.integers(0, c.n, M))]
    elif stream == "big_windows":
        e.set_option("big_min", 512)
        e.set_option("big_window", 1024)
        k = M // 10
        dele = c.pick(k)
        dele[:, 2] = 0
        batches = [sc.interleave(c.fresh(c.rng.integers(0, c.n, M - 2 * k)), dele, c.fresh(np.full(k, c.n // 3)))]
    elif stream == "rollbacks":
        e.set_option("big_min", 64)
        e.set_option("big_window", 256)
        batches, need = sc.rollback_batches(c), "rollbacks"
    elif stream == "doubling":
        batches, need = [c.fresh(c.rng.integers(0, c.n, M)) for _ in range(8)], "double_calls"
    elif stream == "mixed":
        batches = [sc.followup_batch(c, size=M)]
    else:
        raise AssertionError(stream)
    s0, q0 = e.stats(), o.stats()
    for ops in batches:
        assert len(ops) == M, (stream, len(ops))
        sa, qa = e.stats(), o.stats()
        e.apply(ops)
        o.apply(ops)
        sb, qb = e.stats(), o.stats()
        _same_as_oracle(e, o, label)
        applied = (qb["ops_add"] - qa["ops_add"]) + (qb["ops_del"] - qa["ops_del"])
        print(f"{label}: committed {sb['committed'] - sa['committed']}, oracle applied {applied}, round_syncs {sb['round_syncs'] - sa['round_syncs']}, "
              f"rounds {sb['rounds'] - sa['rounds']}, rollbacks {sb['rollbacks'] - sa['rollbacks']}, exclusive {sb['exclusive_ops'] - sa['exclusive_ops']}, "
              f"doublings {sb['double_calls'] - sa['double_calls']}")
        assert sb["committed"] - sa["committed"] == applied, f"{label}: {sb['committed'] - sa['committed']} updates committed, the oracle applied {applied}"
        if need and sb[need] > s0[need]:
            break
    if need:
        assert e.stats()[need] > s0[need], f"{label}: the stream was to go through {need}"
    o.close()
