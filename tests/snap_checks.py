"""Driver and model of the snapshot / restore tests (scenarios: tests/snap_cases.py; run by tests/test_sim_snapshot.py on the
emulator and tests/test_gpu_snapshot.py on the device).

The model is a full host copy.  At every snapshot() the driver records geometry(), get_n() and the arrays of state()
(ppcsr_export_state: a plain whole-array device-to-host copy that shares nothing with the dirty tags).  After every restore() it
asserts (a) geometry and n, (b) items[] and nodes[] byte for byte, (c) check_invariants() == 0, and (d) that a follow-up batch
leaves the engine and an oracle started from the record bit-identical with equal redistribute counters — the leaf counts are not
exported, and stale ones show only when a later rebalance misplaces elements.  The path a synchronisation took (incremental or
whole-array) and what it copied come from ppcsr_debug_snap_counters."""
import numpy as np

import snap_cases as sc
from helpers import live_triples
from oracle_lib import Oracle

# what every scenario starts from (its steps may change any of it): the emulator's set keeps rounds narrow (every emulated
# workgroup is a set of fibers) and small batches on the scheduler under test
SIM_OPTS = dict(opt_horizon=64, epoch_ops=1024, region_slots=64, max_horizon=32, min_horizon=4, init_horizon=8, rounds_per_sync=2,
                small_batch=0, big_grid=2, big_min=512, big_window=131072, rb_inplace_min=1 << 19, excl_in_wave=4096,
                rb_bench_upper=0, snap_grid=4096, snap_count=1)
# (the device runs the same narrow schedule — the scenarios were laid out on the emulator, and a rollback or an exclusive update
#  they count on comes from the round width as much as from the stream; resident_waves 0: no quantisation of the adapted width)
GPU_OPTS = {**SIM_OPTS, "resident_waves": 0}
SCHED = {"strict": dict(mode=0), "spec": dict(mode=1)}
# B of the other-snapshot form: speculative, small epochs and regions, small exclusive windows (see snap_cases.rollback_batches)
B_OPTS = dict(mode=1, small_batch=0, epoch_ops=1024, big_window=256, big_min=64)


class Backend:
    """how a test file reaches its build: make(n) -> PCSR, make_pp(n) -> one-partition PPPCSR, to_device(array) -> (pointer,
    keep-alive), the option set, the adds per rollback batch and the scheduler of the follow-up batch"""

    def __init__(self, make, make_pp, to_device, opts, rollback_k, followup_sched):
        self.make, self.make_pp, self.to_device, self.opts, self.rollback_k, self.followup_sched = make, make_pp, to_device, opts, rollback_k, followup_sched


class Rec:
    def __init__(self, e):
        self.geom, self.n = e.geometry(), e.get_n()
        self.items, self.nodes = e.state()

    def ctx(self, seed, rollback_k):
        return sc.Ctx(self.n, self.geom, live_triples(self.items), seed, rollback_k)


def diff_leaves(a, b, logN):
    """leaves whose slots differ between two exports of one geometry"""
    return np.nonzero((a != b).any(1).reshape(-1, logN).any(1))[0]


def diff_nodes(a, b):
    return np.nonzero((a != b).any(1))[0]


def assert_same(e, geom, n, items, nodes, label):
    assert e.geometry() == geom, f"{label}: geometry {e.geometry()}, expected {geom}"
    assert e.get_n() == n, f"{label}: n = {e.get_n()}, expected {n}"
    ei, en = e.state()
    bad = diff_nodes(en, nodes)
    assert len(bad) == 0, f"{label}: nodes[] differ at {len(bad)} vertices, first {bad[:8]}: {en[bad[:3]].tolist()} vs {nodes[bad[:3]].tolist()}"
    bad = diff_leaves(ei, items, geom[1])
    assert len(bad) == 0, f"{label}: items[] differ in {len(bad)} leaves of {geom[1]} slots, first {bad[:8]}"
    assert e.check_invariants() == 0, f"{label}: leaf counts differ from a recount"


class Driver:
    def __init__(self, backend, e, pp=None):
        self.b, self.e, self.pp = backend, e, pp
        self.rec = None
        self.sched = "strict"
        self.dirty_full = True  # the model of the path: does the next synchronisation of the user's snapshot copy everything?
        self.steps = 0
        self._count_off = False  # snap_count switched off for a run: the launches as shipped, no copy counts to compare

    # -- options
    def reset_options(self, sched, **more):
        self.sched = sched
        for k, v in {**self.b.opts, **SCHED[sched], **more}.items():
            self.e.set_option(k, v)

    def ctr(self):
        return self.e.debug_snap_counters()

    # -- snapshot / restore with the model
    def snapshot(self, label, path=None):
        live = Rec(self.e)
        c0 = self.ctr()
        self.e.snapshot()
        c1 = self.ctr()
        want = "full" if self.dirty_full else "step"
        assert path is None or path == want, f"{label}: the scenario expects a {path} save, the writes since the last one make it {want}"
        self._path(label + " (snapshot)", c0, c1, want, "full_saves", "inc_commits", self.rec, live)
        self.rec = live
        self.dirty_full = False
        return live

    def restore(self, label, path=None, followup=True, exact=None):
        before = Rec(self.e)
        c0 = self.ctr()
        self.e.restore()
        c1 = self.ctr()
        want = "full" if self.dirty_full else "step"
        assert path is None or path == want, f"{label}: the scenario expects a {path} load, the writes since the snapshot make it {want}"
        self._path(label + " (restore)", c0, c1, want, "full_loads", "inc_rollbacks", self.rec, before, exact)
        self.dirty_full = False
        r = self.rec
        assert_same(self.e, r.geom, r.n, r.items, r.nodes, label + ": after restore")
        if followup:
            self.followup(label)

    def _path(self, label, c0, c1, want, full_key, inc_key, old, new, exact=None):
        d = {k: c1[k] - c0[k] for k in c1}
        print(f"{label}: {want}; counters {c1}")
        if want == "full":
            assert d[full_key] == 1 and d[inc_key] == 0, f"{label}: expected the whole-array path: {d}"
            return
        assert d[inc_key] == 1 and d[full_key] == 0, f"{label}: expected the incremental path: {d}"
        if not self.b.opts.get("snap_count") or self._count_off:
            return
        assert old.geom == new.geom and old.n == new.n, f"{label}: in step over two geometries?"
        dl, dn = len(diff_leaves(old.items, new.items, old.geom[1])), len(diff_nodes(old.nodes, new.nodes))
        print(f"{label}: {dl} leaves / {dn} node records differ, {c1['leaves_copied']} / {c1['nodes_copied']} copied of {old.geom[0] // old.geom[1]} / {old.n}")
        assert c1["leaves_copied"] >= dl, f"{label}: {dl} leaves differ, {c1['leaves_copied']} copied"
        assert c1["nodes_copied"] >= dn, f"{label}: {dn} node records differ, {c1['nodes_copied']} copied"
        assert c1["leaves_copied"] <= old.geom[0] // old.geom[1] and c1["nodes_copied"] <= old.n, f"{label}: more copied than there is: {c1}"
        if exact is not None:
            assert (dl, dn) == exact, f"{label}: the write was to change {exact} leaves / node records, the exports differ in {(dl, dn)}"
            assert (c1["leaves_copied"], c1["nodes_copied"]) == exact, f"{label}: exactly {exact} were to be copied: {c1}"

    def count(self, on):
        self._count_off = not on
        self.e.set_option("snap_count", 1 if on else 0)

    # -- check (d)
    def followup(self, label):
        e, r = self.e, self.rec
        batch = sc.followup_batch(r.ctx(1000 + self.steps, self.b.rollback_k))
        o = Oracle.from_state(r.items, r.nodes)
        keep = {k: self.b.opts[k] for k in ("big_min", "big_window", "rb_inplace_min", "excl_in_wave")}
        for k, v in {**keep, **SCHED[self.b.followup_sched]}.items():
            e.set_option(k, v)
        s0 = e.stats()
        self.apply(batch)
        s1 = e.stats()
        o.apply(batch)
        so = o.stats()
        oi, on = o.state()
        assert_same(e, o.geometry(), o.get_n(), oi, on, label + ": after the follow-up batch")
        for k in ("redistribute_calls", "redistribute_slots"):
            assert s1[k] - s0[k] == so[k], f"{label}: follow-up batch: {k} {s1[k] - s0[k]}, oracle {so[k]}"
        o.close()
        e.set_option("mode", SCHED[self.sched]["mode"])

    # -- writes
    def apply(self, ops):
        s0 = self.e.stats()
        self.e.apply(ops)
        s1 = self.e.stats()
        if s1["double_calls"] != s0["double_calls"] or s1["half_calls"] != s0["half_calls"]:
            self.dirty_full = True
        return s0, s1

    def write(self, w, label, seed=0):
        """carry out the steps of scenario w on the engine and, where they are parity operations, on an oracle started from the
        state in front of them; returns the stats deltas the scenario's `needs` are checked against"""
        e = self.e
        self.steps += 1
        start = Rec(e)
        steps = w.build(start.ctx(seed * 7919 + self.steps, self.b.rollback_k))
        o = Oracle.from_state(start.items, start.nodes)
        parity = True
        s0 = e.stats()
        keep = []
        for st in steps:
            kind = st[0]
            if kind == "opt":
                e.set_option(st[1], st[2])
            elif kind == "add_edge":
                self._single(lambda: e.add_edge(*st[1:]))
                o.add_edge(*st[1:])
            elif kind == "remove_edge":
                self._single(lambda: e.remove_edge(*st[1:]))
                o.remove_edge(*st[1:])
            elif kind == "apply":
                self.apply(st[1])
                o.apply(st[1])
            elif kind == "rollbacks":
                r0 = e.stats()["rollbacks"]
                for ops in st[1]:
                    self.apply(ops)
                    o.apply(ops)
                    if e.stats()["rollbacks"] > r0:
                        break
            elif kind == "rebalance":
                e.set_option("rb_bench_upper", st[2])
                e.bench_rebalance(st[1], 1)
                o.debug_redistribute(start.geom[0] - st[1] if st[2] else 0, st[1])
            elif kind == "block_rebalance":
                e.set_option("test_block_rebalance", (st[1] << 32) | st[2])
                o.debug_redistribute(st[1], st[2])
            elif kind == "bench_resize":
                e.bench_resize(1)
                parity, self.dirty_full = False, True
            elif kind == "add_node":
                e.add_node()
                o.add_node()
                self.dirty_full = True
            elif kind == "bulk_build":
                e.bulk_build(st[1])
                parity, self.dirty_full = False, True
            elif kind == "set_nn":
                ptr, k = self.b.to_device(st[1])
                keep.append(k)
                self.pp.set_num_neighbors_device(ptr, len(st[1]))
                for v, nn, _ in st[1]:
                    o.set_num_neighbors(int(v), int(nn))
            else:
                raise AssertionError(kind)
        s1 = e.stats()
        if parity:
            oi, on = o.state()
            assert_same(e, o.geometry(), o.get_n(), oi, on, label + ": live state after the writes")
        o.close()
        d = {k: s1[k] - s0[k] for k in ("rollbacks", "exclusive_ops", "big_redistributes", "double_calls", "half_calls")}
        d["same_N"] = int(e.geometry() == start.geom)
        for k in w.needs:
            assert d[k] > 0, f"{label}: the scenario is to go through {k}: {d}"
        if w.path == "step":
            assert d["double_calls"] == 0 and d["half_calls"] == 0 and d["same_N"], f"{label}: an in-step scenario resized: {d}"
        if w.nodes_only:
            now = Rec(e)
            assert len(diff_leaves(start.items, now.items, start.geom[1])) == 0 and len(diff_nodes(start.nodes, now.nodes)) > 0, f"{label}: node records only"
        return d

    def _single(self, call):
        s0 = self.e.stats()
        call()
        s1 = self.e.stats()
        if s1["double_calls"] != s0["double_calls"] or s1["half_calls"] != s0["half_calls"]:
            self.dirty_full = True

    # -- the three forms of a scenario
    def run(self, w, form, sched, seed=0, b_may_resize=False, **opts):
        """b_may_resize: the array is too small to take B without a resize (the 64-slot graph): the restore then takes the path
        the model predicts from what B did instead of the scenario's"""
        label = f"{w.name}/{form}/{sched}"
        self.reset_options(sched, **opts)
        self.count(opts.get("snap_count", 1))
        self.snapshot(label + ": S")
        self.write(w, label, seed)
        if form == "restore":
            self.restore(label, path=w.path, exact=w.exact)
        elif form == "commit":
            # S; W; S'; V; R lands on S': what W wrote without a stamp is not in the snapshot, and V's stamps drag the stale copy back
            self.snapshot(label + ": S'", path=w.path)
            self.e.set_option("rb_bench_upper", 0)
            self.e.bench_rebalance(self.rec.geom[0], 1)
            self.apply(sc.verify_batch(self.rec.ctx(seed + 5, self.b.rollback_k)))
            assert self.e.geometry() == self.rec.geom, f"{label}: V was not to resize"
            self.restore(label, path="step")
        elif form == "other":
            # S; W; B; R: the epochs' rollback point works on the same tags in between (newtag, other.gen)
            for k, v in {**B_OPTS, "region_slots": min(256, self.b.opts["region_slots"])}.items():
                self.e.set_option(k, v)
            r0 = self.e.stats()["rollbacks"]
            for ops in sc.rollback_batches(Rec(self.e).ctx(seed + 9, self.b.rollback_k)):
                self.apply(ops)
                if self.e.stats()["rollbacks"] > r0:
                    break
            assert self.e.stats()["rollbacks"] > r0, f"{label}: B was to roll an epoch back"
            self.restore(label, path=None if b_may_resize else w.path)
        else:
            raise AssertionError(form)
        # the follow-up batch moved on from the snapshot: one more restore, checked, and the engine (the tests share one per
        # graph) is back at a state of the size it started from
        self.restore(label + ": back", followup=False)


def build_graph(backend, name, streams, pp=False):
    """a loaded engine for graph `name` (tests/snap_cases.py GRAPHS); pp: as the one partition of a PPPCSR -> (engine, pp)"""
    n, _ = sc.GRAPHS[name]
    owner = backend.make_pp(n) if pp else None
    e = owner.partition(0) if pp else backend.make(n)
    for k, v in {**backend.opts, "mode": 0}.items():
        e.set_option(k, v)
    e.apply(sc.graph_ops(name, streams))
    if name == "tiny":  # ten more edges, deleted again: the deletes halve the array down to N < 2^8, leaves of 8 slots
        for i in range(10):
            e.add_edge(i % 2, 900000 + i, 1)
        for i in range(10):
            e.remove_edge(i % 2, 900000 + i)
        assert e.geometry()[1] == 8, e.geometry()
    return (e, owner) if pp else e


def check_empty_bulk(backend, streams, n=150):
    """row 8: snapshot of an EMPTY graph, bulk_build, restore (whole-array: bulk_build starts a new generation), bulk_build
    again — only an empty graph can be bulk-built, so it succeeds only if the leaf counts went back too — and a second restore"""
    e = backend.make(n)
    d = Driver(backend, e)
    d.reset_options("strict")
    d.count(True)
    d.snapshot("empty: S")
    ops = streams.random_stream(n, 3000, seed=41)
    for rep in range(2):
        e.bulk_build(ops)
        d.dirty_full = True
        assert e.geometry() != d.rec.geom or len(live_triples(e.state()[0])) > 0
        d.restore(f"empty: bulk_build {rep}", path="full", followup=(rep == 1))
    d.restore("empty: back", followup=False)
    assert len(live_triples(e.state()[0])) == 0
    e.close()


def check_control_flow(backend, d, pkg):
    """row 10"""
    e = d.e
    w = sc.BY_NAME["batch"]
    fresh = backend.make(5)
    try:
        fresh.restore()
        raise AssertionError("restore before any snapshot was to fail")
    except pkg.PpcsrError as err:
        assert "status 1 " in str(err) or "EINVAL" in str(err).upper() or "invalid" in str(err).lower(), err
    for bad in (0, 4097):  # snap_grid is a cap in [1, 4096]
        try:
            fresh.set_option("snap_grid", bad)
            raise AssertionError(f"snap_grid = {bad} was to be refused")
        except pkg.PpcsrError as err:
            assert "status 1 " in str(err), err
    assert fresh.debug_snap_counters() == dict(full_saves=0, full_loads=0, inc_commits=0, inc_rollbacks=0, leaves_copied=0, nodes_copied=0)
    fresh.close()
    for sched in ("strict", "spec"):
        d.reset_options(sched)
        d.count(True)
        d.snapshot("flow: S")
        # S; S: nothing was written in between
        d.snapshot("flow: S; S", path="step")
        c = d.ctr()
        assert (c["leaves_copied"], c["nodes_copied"]) == (0, 0), c
        # R; R: the second finds nothing to do either way and lands on the same record
        d.write(w, "flow: W")
        d.restore("flow: R", path="step", followup=False)
        d.restore("flow: R; R", path="step", followup=False)
        c = d.ctr()
        assert (c["leaves_copied"], c["nodes_copied"]) == (0, 0), c
        # R; W; S; W; R
        d.write(w, "flow: R; W", seed=1)
        d.snapshot("flow: R; W; S", path="step")
        d.write(sc.BY_NAME["single_ops"], "flow: R; W; S; W", seed=2)
        d.restore("flow: R; W; S; W; R", path="step")
        d.restore("flow: back", followup=False)


def run_campaign(d, seed):
    script = sc.campaign_script(seed)
    print("script:", script)
    d.reset_options("spec")
    d.count(True)
    for i, step in enumerate(script):
        label = f"campaign {seed} step {i} {step}"
        if step == "S":
            d.snapshot(label)
        elif step == "R":
            d.restore(label)
        else:
            w = sc.BY_NAME[step]
            sched = w.scheds[(seed + i) % len(w.scheds)]
            d.reset_options(sched)
            d.count(True)
            d.write(_lenient(w), label, seed=seed * 100 + i)
    d.restore(f"campaign {seed}: last", followup=False)


def _lenient(w):
    """a write of the campaign runs on whatever the script has left: it need not meet the scenario's own expectations (which
    path the restore takes follows from what happened: Driver.dirty_full)"""
    return sc.W(w.name, w.build, "any", w.scheds)
