"""Checks of the speculative rounds' rule for duplicate overwrites (tests/test_sim_dup_slots.py on the emulator,
tests/test_gpu_dup_slots.py on the device).

A duplicate (an add of an edge that exists: K_DUP) overwrites one slot's value and moves nothing.  Duplicates of DIFFERENT slots
commute, so the rounds order them per slot (a table of ppcsr_debug_dup_slot_entries() entries indexed by the slot modulo its size)
and no longer per leaf; two overwrites of the SAME slot keep their stream order, a strong writer (insert / delete) of the leaf is
ordered against every duplicate of the leaf as before.  Every case ends on the oracle's state: geometry, every slot of edges[],
every nodes[] triple, and the `duplicates` statistic.  Every batch has more than 256 updates and small_batch is 0 on top of
that: the strict rounds keep the per-leaf rule and would test nothing here.

Nothing here depends on the backend: the test files hand in a snap_checks.Backend."""
import numpy as np

import batch_open_checks as bo
import snap_checks as ck
from helpers import live_triples
from oracle_lib import Oracle

sc = bo.sc  # (the stream builders batch_open_checks runs: rollback_batches, followup_batch, interleave)

G16_VERTICES, G16_NEIGHBOURS = 16, 64
# one round takes a whole batch of these cases: fixed width, no adaptation, one epoch
ONE_ROUND = dict(mode=1, small_batch=0, adaptive=0, opt_horizon=1024, start_horizon=1024, resident_waves=0, epoch_ops=1 << 20,
                 epoch_short=1 << 20, rounds_per_sync=8, check_lanes=-1, diag=0)
KERNELS = {"lane": dict(check_lanes=1, diag=0), "wave": dict(check_lanes=0, diag=0), "diag": dict(check_lanes=-1, diag=1)}


def set_options(e, backend, **more):
    for k, v in {**backend.opts, **more}.items():
        e.set_option(k, v)


def g16(backend):
    """16 vertices x 64 neighbours (dests 10, 13, 16, ...: room for new edges in between), inserted edge by edge"""
    e = backend.make(G16_VERTICES)
    set_options(e, backend, mode=0)
    for v in range(G16_VERTICES):
        for j in range(G16_NEIGHBOURS):
            e.add_edge(v, 10 + 3 * j, 1)
    return e


def oracle_of(e):
    return Oracle.from_state(*e.state())


def run(e, o, ops, label):
    """one batch on the engine and on the oracle, then the whole comparison -> the engine's stats delta"""
    s0, q0 = e.stats(), o.stats()
    e.apply(ops)
    o.apply(ops)
    s1, q1 = e.stats(), o.stats()
    oi, on = o.state()
    ck.assert_same(e, o.geometry(), o.get_n(), oi, on, label)
    d = {k: s1[k] - s0[k] for k in ("rounds", "committed", "duplicates", "rollbacks", "exclusive_ops")}
    assert d["duplicates"] == q1["duplicates"] - q0["duplicates"], f"{label}: duplicates {d['duplicates']}, oracle {q1['duplicates'] - q0['duplicates']}"
    d["applied"] = (q1["ops_add"] - q0["ops_add"]) + (q1["ops_del"] - q0["ops_del"])
    print(f"{label}: {len(ops)} updates, {d}")
    return d


def noop_batch(e, k):
    """k deletes with a source beyond n: planned, committed as nothing, never in anybody's way"""
    n = e.get_n()
    return np.stack([n + np.arange(k) % 7, np.arange(k), np.zeros(k)], 1).astype(np.uint32)


def distinct_batch(e, k=600, seed=1):
    ex = live_triples(e.state()[0])
    assert len(ex) == G16_VERTICES * G16_NEIGHBOURS
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(ex))
    ops = ex[order[:k]].copy()
    ops[:, 2] = 2 + np.arange(k)
    return ops, ex[order[k:]], rng


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def distinct_slots_one_round(backend, e, label="distinct"):
    """600 overwrites of pairwise distinct edges, values 2 + i, shuffled: as many rounds as 600 updates that touch nothing.
    (Ordered per leaf the batch needs as many rounds as its fullest leaf holds duplicates: leaves of 16 or 32 slots, more than half
    of every leaf overwritten.)"""
    set_options(e, backend, **ONE_ROUND)
    o = oracle_of(e)
    ops, _, _ = distinct_batch(e)
    dup = run(e, o, ops, label + ": overwrites")
    ctl = run(e, o, noop_batch(e, len(ops)), label + ": control")
    assert dup["duplicates"] == len(ops)
    assert dup["rounds"] == ctl["rounds"], f"{label}: {dup['rounds']} rounds for {len(ops)} overwrites of distinct slots, {ctl['rounds']} for the control"
    o.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def same_slot_stream_order(backend, e, label="same-slot"):
    """the batch of case 1 with one key overwritten 7 times (values 1 .. 7) and another 3 times in between: the last value in stream
    order stays, num_neighbors counts every call"""
    set_options(e, backend, **ONE_ROUND)
    o = oracle_of(e)
    ops, rest, rng = distinct_batch(e)
    a, b = rest[0], rest[1]
    rep = np.array([[a[0], a[1], 1 + i] for i in range(7)] + [[b[0], b[1], 1 + i] for i in range(3)], np.uint32)
    pos = np.concatenate([np.sort(rng.choice(len(ops), 7, replace=False)), np.sort(rng.choice(len(ops), 3, replace=False))])
    # (np.insert keeps the order of rows that go to the same position)
    by_pos = np.argsort(pos, kind="stable")
    batch = np.insert(ops, pos[by_pos], rep[by_pos], axis=0)
    for key, want in ((a, 7), (b, 3)):
        mine = batch[(batch[:, 0] == key[0]) & (batch[:, 1] == key[1]), 2]
        assert list(mine) == list(range(1, want + 1)), mine
    nn0 = e.state()[1][:, 2].astype(np.int64)
    d = run(e, o, batch, label)
    items, nodes = e.state()
    for key, want in ((a, 7), (b, 3)):
        got = items[(items[:, 0] == key[0]) & (items[:, 1] == key[1]) & (items[:, 2] != 0), 2]
        assert list(got) == [want], f"{label}: edge {key[:2]} holds {got}, the stream's last value is {want}"
    np.testing.assert_array_equal(nodes[:, 2].astype(np.int64) - nn0, np.bincount(batch[:, 0], minlength=len(nodes)))
    assert d["duplicates"] == len(batch)
    o.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
SCRIPTS = (("o", "d"), ("d", "i"), ("o", "d", "i"), ("d", "i", "o"), ("o", "o", "d", "i", "o"), ("d", "i", "d", "i"))


def strong_mix_batch(ex, seed):
    """overwrites (keys repeat), fresh inserts into the same vertices, and per-key scripts of overwrite / delete / re-insert whose
    order the shuffle keeps"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(ex))
    scripted, plain = ex[order[:80]], ex[order[80:]]
    rows, when = [], []
    for r in plain[rng.integers(0, len(plain), 300)]:
        rows.append((r[0], r[1], 1 + rng.integers(1, 1000)))
        when.append(rng.random())
    for v, j in zip(rng.integers(0, G16_VERTICES, 150), rng.choice(3 * G16_NEIGHBOURS, 150, replace=False)):
        rows.append((v, 11 + 3 * j, 1 + rng.integers(1, 1000)))  # (dests 11, 14, ...: between the loaded ones and beyond them, new)
        when.append(rng.random())
    for r in scripted:
        s = SCRIPTS[rng.integers(0, len(SCRIPTS))]
        for step, t in zip(s, np.sort(rng.random(len(s)))):
            rows.append((r[0], r[1], 0 if step == "d" else 1 + rng.integers(1, 1000)))
            when.append(t)
    return np.array(rows, np.uint32)[np.argsort(when, kind="stable")]


def strong_writers_same_leaves(backend, e, kernel, seeds=range(5), label=None):
    """e: the 16 x 64 graph; every seed starts from it (snapshot / restore)"""
    label = label or f"mix/{kernel}"
    e.snapshot()
    base = e.state()
    for seed in seeds:
        e.restore()
        set_options(e, backend, mode=1, small_batch=0, opt_horizon=256, start_horizon=256, resident_waves=0, epoch_ops=1 << 20, epoch_short=1 << 20,
                    rounds_per_sync=4, **KERNELS[kernel])
        o = Oracle.from_state(*base)
        batch = strong_mix_batch(live_triples(base[0]), seed)
        assert len(batch) > 256
        d = run(e, o, batch, f"{label}/seed{seed}")
        # (a re-insert that came out as an overwrite, or the reverse, shows in `duplicates`, which run() has compared, and in the slots)
        assert 0 < d["duplicates"] < int((batch[:, 2] != 0).sum())
        o.close()
    set_options(e, backend, check_lanes=-1, diag=0)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def aliased_entries(backend, streams, entries, label="aliased"):
    """an array of twice as many slots as the table has entries: two edges whose slots share an entry, overwritten in one batch among
    300 others — both land (the later one may take a round more)"""
    n, m = 4096, 70000
    e = backend.make(n)
    load = streams.random_stream(n, m, seed=17)
    load[:, 1] = streams.uniform_ints(18, m, sc.FRESH_LO)
    load[:, 2] = 1 + streams.uniform_ints(19, m, 1000)
    e.bulk_build(load.astype(np.uint32))
    set_options(e, backend, **ONE_ROUND)
    items, _ = e.state()
    N = e.geometry()[0]
    assert N == 2 * entries, f"{label}: the array has {N} slots, the table {entries} entries: the case needs N = 2 x entries"
    live = (items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF)
    both = np.nonzero(live[:entries] & live[entries:])[0]
    assert len(both) > 0
    rng = np.random.default_rng(4)
    lo = int(both[rng.integers(0, len(both))])
    pair = items[[lo, lo + entries]].copy()
    pair[:, 2] = (4001, 4002)
    others = np.nonzero(live)[0]
    others = others[(others % entries) != lo]
    rest = items[rng.choice(others, 300, replace=False)].copy()
    rest[:, 2] = 5000 + np.arange(300)
    batch = np.insert(rest, [100, 200], pair, axis=0)
    o = oracle_of(e)
    d = run(e, o, batch, label)
    ctl = run(e, o, noop_batch(e, len(batch)), label + ": control")
    now = e.state()[0]
    assert (now[lo, 2], now[lo + entries, 2]) == (4001, 4002)
    assert d["duplicates"] == len(batch)
    assert ctl["rounds"] <= d["rounds"] <= ctl["rounds"] + 1, f"{label}: {d['rounds']} rounds, the control took {ctl['rounds']}"
    o.close()
    e.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def sprinkle(c, batch):
    """one update in ten an overwrite of an existing edge of the vertices the batch works on (keys repeat), anywhere in the batch"""
    m = max(3, len(batch) // 9)
    pool = c.ex[np.isin(c.ex[:, 0], np.unique(batch[:, 0]))]
    if len(pool) < 4:
        pool = c.ex
    pool = pool[c.rng.choice(len(pool), min(len(pool), max(2, m // 3)), replace=False)]
    over = pool[c.rng.integers(0, len(pool), m)].copy()
    over[:, 2] = 1 + c.rng.integers(1, 1000, m)
    return np.insert(batch, np.sort(c.rng.integers(0, len(batch) + 1, m)), over, axis=0).astype(np.uint32)


def epochs_and_rollbacks(backend, e, stream, label=None):
    """the rollback and the mixed streams of batch_open_checks with overwrites among them, in chunks of 2 rounds: bit-exact,
    commit-exact, and the rollback stream does roll an epoch back"""
    label = label or f"epochs/{stream}"
    d = ck.Driver(backend, e)
    d.reset_options("spec")
    c = ck.Rec(e).ctx(5, backend.rollback_k)
    if stream == "rollbacks":
        bo.b_options(d, 2 * backend.rollback_k, rounds_per_sync=2)
        batches = sc.rollback_batches(c)
    else:
        set_options(e, backend, mode=1, small_batch=0, rounds_per_sync=2)
        batches = [sc.followup_batch(c, size=2048)]
    o = oracle_of(e)
    r0 = e.stats()["rollbacks"]
    for i, ops in enumerate(batches):
        ops = sprinkle(c, ops)
        assert len(ops) > 256
        r = run(e, o, ops, f"{label}/batch{i}")
        assert r["committed"] == r["applied"], f"{label}: {r['committed']} updates committed, the oracle applied {r['applied']}"
        assert r["duplicates"] >= len(ops) // 20
        if stream == "rollbacks" and e.stats()["rollbacks"] > r0:
            break
    if stream == "rollbacks":
        assert e.stats()["rollbacks"] > r0, f"{label}: the stream was to roll an epoch back"
    o.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
WIDTH_UPDATES = 20000


def calm_stream(c, m=WIDTH_UPDATES):
    over = c.pick(m // 20)
    over[:, 2] += 1
    fresh = c.fresh(c.rng.integers(0, c.n, m - len(over)))
    return np.insert(fresh, np.sort(c.rng.integers(0, len(fresh) + 1, len(over))), over, axis=0).astype(np.uint32)


def _width_opts(cap):
    return dict(mode=1, small_batch=0, adaptive=1, resident_waves=64, opt_horizon=cap, start_horizon=64, epoch_ops=1 << 20, epoch_short=1 << 20,
                rounds_per_sync=16)


def width_multiples(backend, e, label="width"):
    """rounds of up to six chip-fulls (resident_waves 64, opt_horizon 384) against three (192) on a calm stream, 5 % overwrites: the
    same state, no device error (apply raises on one), fewer rounds.  e: the `big` graph"""
    e.snapshot()
    base = e.state()
    batch = calm_stream(ck.Rec(e).ctx(6, backend.rollback_k))
    rounds = {}
    for cap in (384, 192):
        e.restore()
        set_options(e, backend, **_width_opts(cap))
        o = Oracle.from_state(*base)
        rounds[cap] = run(e, o, batch, f"{label}/{cap}")["rounds"]
        o.close()
    assert rounds[384] < rounds[192], f"{label}: rounds {rounds}"


def width_multiples_pppcsr(backend, make_pp4, streams, label="width/pppcsr"):
    """the same through a PPPCSR of 4 partitions on one device: every partition the size of the `big` graph (a quarter of it is no
    calm place for 5 000 inserts), bulk-built; the batch goes through the PPPCSR, the model is one oracle per partition, started from
    the partition's state and fed the updates of its vertex range"""
    n1, m1 = sc.GRAPHS["big"]
    n, m = 4 * n1, 4 * m1
    load = np.stack([streams.uniform_ints(61, m, n), streams.uniform_ints(62, m, sc.FRESH_LO), 1 + streams.uniform_ints(63, m, 1000)], 1).astype(np.uint32)
    pp = make_pp4(n)
    P = pp.num_partitions()
    assert P == 4
    parts = [pp.partition(k) for k in range(P)]
    starts = np.array([pp.partition_start(k) for k in range(P)], np.int64)
    own = lambda ops: np.searchsorted(starts, ops[:, 0].astype(np.int64), side="right") - 1

    def local(ops, k):
        sub = ops[own(ops) == k].copy()
        sub[:, 0] -= np.uint32(starts[k])
        return sub
    base = []
    for k, e in enumerate(parts):
        e.bulk_build(local(load, k))
        e.snapshot()
        base.append(e.state())
    rng = np.random.default_rng(8)
    over = load[rng.choice(len(load), WIDTH_UPDATES // 20, replace=False)].copy()
    over[:, 2] += 1
    k_fresh = WIDTH_UPDATES - len(over)
    fresh = np.stack([rng.integers(0, n, k_fresh), sc.FRESH_LO + rng.choice(sc.FRESH_LO, k_fresh, replace=False), 1 + rng.integers(0, 1000, k_fresh)], 1).astype(np.uint32)
    batch = np.insert(fresh, np.sort(rng.integers(0, k_fresh + 1, len(over))), over, axis=0).astype(np.uint32)
    rounds = {}
    for cap in (384, 192):
        for e in parts:
            e.restore()
            set_options(e, backend, **_width_opts(cap))
        s0 = [e.stats() for e in parts]
        pp.apply(batch)
        rounds[cap] = 0
        for k, e in enumerate(parts):
            o = Oracle.from_state(*base[k])
            o.apply(local(batch, k))
            oi, on = o.state()
            ck.assert_same(e, o.geometry(), o.get_n(), oi, on, f"{label}/{cap}: partition {k}")
            s1 = e.stats()
            assert s1["duplicates"] - s0[k]["duplicates"] == o.stats()["duplicates"], f"{label}/{cap}: partition {k}: duplicates"
            rounds[cap] += s1["rounds"] - s0[k]["rounds"]
            o.close()
    print(f"{label}: rounds {rounds}")
    assert rounds[384] < rounds[192], f"{label}: rounds {rounds}"
    pp.close()
