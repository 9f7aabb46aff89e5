"""Device label-propagation communities and modularity (ppcsr_label_propagation / ppcsr_modularity) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

on one PCSR, with edge values 1 .. 4 that depend on the pair alone.  Per graph, for the three vertex orders and both flags: ms per
call, ms per sweep after the first (a run with max_sweeps = 1 beside the full one), sweeps, classes, communities, q — with
ppcsr_colouring alone (its export and colours are the call's fixed cost), one modularity call and one ppcsr_bench_scan_all
beside them, all INTERLEAVED: every repeat runs every variant once, in the same order; medians with all the samples (device ms
of the whole call: host round trips included).  An order whose colouring needs more than --max-rounds rounds is run once and not
repeated (`id` on an RMAT graph is a long chain).  Then a batch of 1 M fresh RMAT inserts, applied once, and a cold start against
a warm start from the labels of before the batch, interleaved and repeated like the rest.
  baseline    s18: what a user has without the calls — gather_neighbourhoods of every vertex to the host, then the numpy replica
              of tests/community_model.py and its modularity integers, in the random order, beside the device call in the
              same order (host_over_device); equal arrays and words are asserted

Writes profiles/community_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE weighted call (random order) per graph under rocprofv3 --kernel-trace --stats, in a run of its own,
                 and writes profiles/community_kernel_stats.csv: the split export / colouring / class lists / steps."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from community_model import colours, modularity_ints, replica_sweeps, weighted_csr  # noqa: E402
from helpers import load_pkg, load_streams  # noqa: E402

GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
ORDERS = ("random", "degree", "id")
SEED = 3
BATCH = 1_000_000


def weigh(ops):
    ops = ops.copy()
    ops[:, 2] = 1 + (ops[:, 0].astype(np.uint64) * 7 + ops[:, 1].astype(np.uint64) * 13) % 4
    return ops


def graph(st, which):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    return 1 << scale, weigh(st.adds(s, d))


def med(xs):
    return round(float(np.median(xs)), 3)


def call(g, order, weighted, max_sweeps=0, init=None):
    labels, ncom, sweeps, ms = g.label_propagation(order, SEED, weighted, max_sweeps, init, with_ms=True)
    return (labels, ncom, sweeps), ms


def measure(g, reps, max_rounds):
    results, counters, variants, once = {}, {}, {}, {}
    for order in ORDERS:
        _, _, col_ms = g.colouring(order, SEED, with_ms=True)
        long_chain = g.debug_colouring_counters()[0] > max_rounds
        if not long_chain:
            variants["colouring", order] = lambda order=order: (None, g.colouring(order, SEED, with_ms=True)[2])
        for weighted in (False, True):
            k = ("lp", order, weighted)
            results[k], ms = call(g, order, weighted)
            counters[k] = g.debug_community_counters().tolist()
            if long_chain:
                once[k] = {"ms": round(ms, 3), "colouring_ms": round(col_ms, 3)}
            else:
                variants[k] = lambda order=order, weighted=weighted: call(g, order, weighted)
                variants["lp1", order, weighted] = lambda order=order, weighted=weighted: call(g, order, weighted, max_sweeps=1)
    labels = results["lp", "random", True][0]
    variants["modularity", ""] = lambda: (None, g.modularity(labels, True, with_ms=True)[2])
    variants["scan", ""] = lambda: (None, g.bench_scan_all()[0])
    samples = {k: [] for k in variants}
    for _ in range(reps):
        for k, run in variants.items():
            out, ms = run()
            samples[k].append(round(ms, 3))
            if k[0] == "lp":
                assert np.array_equal(out[0], results[k][0]) and out[1:] == results[k][1:], k
    return results, counters, samples, once


def report(g, results, counters, samples, once):
    res = {"scan_all_ms": med(samples["scan", ""]), "scan_all_ms_all": samples["scan", ""], "modularity_ms": med(samples["modularity", ""]),
           "modularity_ms_all": samples["modularity", ""]}
    for order in ORDERS:
        res[order] = {}
        if ("colouring", order) in samples:
            res[order]["colouring_ms"] = med(samples["colouring", order])
            res[order]["colouring_ms_all"] = samples["colouring", order]
        for weighted in (False, True):
            k = ("lp", order, weighted)
            c = counters[k]
            q, _ = g.modularity(results[k][0], weighted)
            rec = {"sweeps": c[0], "classes": c[1], "label_changes": c[2], "communities": c[4], "workgroup_tier_vertices": c[5],
                   "extra_hash_passes": c[6], "launches": c[7], "q": round(q, 6)}
            if k in once:
                rec["single_run_not_repeated"] = once[k]
            else:
                a, one = samples[k], samples["lp1", order, weighted]
                rec.update(ms=med(a), ms_all=a, one_sweep_ms=med(one), spread=round((max(a) - min(a)) / med(a), 3),
                           ms_per_sweep_after_the_first=round((med(a) - med(one)) / max(c[0] - 1, 1), 3),
                           over_colouring=round(med(a) / res[order]["colouring_ms"], 2))
            res[order]["weighted" if weighted else "unweighted"] = rec
    return res


def warm_start(g, st, which, before, reps):
    """1 M fresh inserts, applied once; then cold against warm from the labels of before the batch (random order, weighted),
    interleaved, medians of `reps` calls each"""
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, BATCH, seed=seed + 100)
    g.apply(weigh(st.adds(s, d)))
    out = {"batch_inserts": BATCH, "reps": reps}
    samples = {"cold": [], "warm": []}
    for _ in range(reps):
        for name, init in (("cold", None), ("warm", before)):
            (labels, _, _), ms = call(g, "random", True, init=init)
            samples[name].append(round(ms, 3))
            c = g.debug_community_counters().tolist()
            out[name] = {"sweeps": c[0], "label_changes": c[2], "communities": c[4], "launches": c[7], "q": round(g.modularity(labels, True)[0], 6)}
    for name, a in samples.items():
        out[name].update(ms=med(a), ms_all=a)
    return out


def baseline(g, n, results):
    """gather every neighbourhood to the host, then the numpy replica and the modularity integers (random order, both flags)"""
    out = {}
    t0 = time.perf_counter()
    rows, dests, values = g.gather_neighbourhoods(np.arange(n, dtype=np.uint32), with_values=True)[:3]
    t1 = time.perf_counter()
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rows, np.int64)))
    dst, val = np.asarray(dests, np.int64), np.asarray(values, np.int64)
    out["gather_and_d2h_ms"] = round((t1 - t0) * 1e3, 1)
    same = True
    for weighted in (False, True):
        t2 = time.perf_counter()
        rws, nbr, wt = weighted_csr(src, dst, val, n, weighted)
        _, classes = colours(src, dst, n, ORDERS.index("random"), SEED)
        r = replica_sweeps(rws, nbr, wt, classes)
        t3 = time.perf_counter()
        words = modularity_ints(rws, nbr, wt, r["labels"])[0]
        t4 = time.perf_counter()
        got = results["lp", "random", weighted]
        ok = bool(np.array_equal(r["labels"], got[0]) and r["sweeps"] == got[2] and [int(x) for x in g.modularity(got[0], weighted)[1]] == words)
        same = same and ok
        out["weighted" if weighted else "unweighted"] = {"order": "random", "host_replica_ms": round((t3 - t2) * 1e3, 1),
                                                          "host_modularity_ms": round((t4 - t3) * 1e3, 1), "equal_arrays": ok}
    out["equal_arrays"] = same
    return out


def kernel_stats(args):
    out = os.path.join(args.out_dir, "community_kernel_stats.csv")
    lines = ["graph,kernel,calls,total_us,avg_us,min_us,max_us"]
    for which in GRAPHS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--trace-pass", which]
            subprocess.run(cmd, check=True, timeout=600)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            rows = list(csv.DictReader(open(found[0])))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace(",", ";")
            if not any(t in name for t in ("ppcsr::k_kc", "ppcsr::k_col", "ppcsr::k_lp")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """ONE weighted call, random order, and one modularity call"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = pkg.PCSR(n)
    g.bulk_build(ops)
    labels, ncom, sweeps = g.label_propagation("random", SEED, True)
    q, _ = g.modularity(labels, True)
    print(json.dumps({"trace_pass": args.trace_pass, "communities": int(ncom), "sweeps": int(sweeps), "q": q}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=2000)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=list(GRAPHS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_stats:
        return kernel_stats(args)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), values 1 .. 4, bulk-built, one PCSR" for k, v in GRAPHS.items()},
           "reps": args.reps, "seed": SEED,
           "timing": "device events on the engine's stream (device_ms of the calls), every variant once per repeat, interleaved; "
                     "the baseline: host wall clock"}
    ok = True
    for which in GRAPHS:
        print(which, file=sys.stderr, flush=True)
        n, ops = graph(st, which)
        g = pkg.PCSR(n)
        g.bulk_build(ops)
        results, counters, samples, once = measure(g, args.reps, args.max_rounds)
        rec = report(g, results, counters, samples, once)
        rec["slots"] = int(g.geometry()[0])
        if which == "s18":
            rec["baseline"] = baseline(g, n, results)
            for name in ("unweighted", "weighted"):  # like with like: the random order on both sides
                b = rec["baseline"][name]
                b["device_ms"] = rec["random"][name]["ms"]
                b["host_over_device"] = round((rec["baseline"]["gather_and_d2h_ms"] + b["host_replica_ms"]) / b["device_ms"], 1)
            ok = ok and rec["baseline"]["equal_arrays"]
        rec["after_a_batch"] = warm_start(g, st, which, results["lp", "random", True][0], args.reps)
        g.close()
        res[which] = rec
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "community_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "community_bench: a check failed (equal results: see the record)"


if __name__ == "__main__":
    main()
