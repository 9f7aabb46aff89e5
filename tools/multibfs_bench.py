"""Device multi-source BFS (ppcsr_multi_bfs) on one PCSR holding

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the other tools: RMAT scale 18, 2 M adds (seed 31), bulk-built

Sources: 1024 vertices with an out-edge, drawn with a fixed seed; the first 64 of them are the 64-source call's.  Per graph:
device ms and host wall ms (median of --reps runs after a warm-up) of one call with 64 and one with 1024 sources, aggregates only
and with levels; the counters of ppcsr_debug_multi_bfs_counters; the same 64-source call with the pass's plain look at next[w]
switched off (set_option "msbfs_look" 0); and the baseline: the loop of 64 ppcsr_bfs calls from the same sources on the same
engine, as the sum of their device ms and as wall time.  The rows of the 64-source call must equal the loop's rows and its
aggregates what numpy makes of them (asserted).  No ratio is asked for: loop_over_multi is what was measured.

--kernel-stats (default on; --no-kernel-stats skips it) reruns ONE 64-source call per graph and variant under rocprofv3
--kernel-trace --stats, each in a run of its own, and adds the per-kernel split to the record and to
profiles/multibfs_kernel_stats.csv.  Writes profiles/multibfs_bench.json (--out-dir: elsewhere)."""
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
from helpers import load_pkg, load_streams  # noqa: E402
from multibfs_model import aggregates, hist_of  # noqa: E402

GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
COUNTERS = ("groups", "level_steps", "streaming_passes", "per_vertex_launches", "hub_passes", "largest_union_frontier",
            "vertex_step_launches", "host_reads")
KERNELS = ("ppcsr::k_ms_", "ppcsr::k_bfs_bits", "ppcsr::k_bfs_collect")


def graph(st, which):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    n = 1 << scale
    ops = st.adds(s, d)
    busy = np.unique(ops[ops[:, 1] < n, 0])
    sources = np.random.default_rng(2026).choice(busy, 1024, replace=False).astype(np.uint32)
    return n, ops, sources


def build(pkg, n, ops):
    g = pkg.PCSR(n)
    g.bulk_build(ops)
    return g


def timed(call, reps):
    call()  # warm-up
    dev, wall, out = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out, ms = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms)
    return out, {"device_ms": round(float(np.median(dev)), 3), "wall_ms": round(float(np.median(wall)), 3),
                 "device_ms_all": [round(x, 3) for x in dev]}


def measure(pkg, st, which, reps):
    n, ops, sources = graph(st, which)
    g = build(pkg, n, ops)
    s64 = sources[:64]
    res = {"n": n, "slots": int(g.geometry()[0]), "sources": "1024 with an out-edge, rng 2026; the first 64 for the 64-source call"}

    def multi(q, levels):
        def call():
            r = g.multi_bfs(q, levels=levels, with_ms=True)
            return r[:-1], r[-1]
        return call

    def loop():
        rows, ms = [], 0.0
        for v in s64:
            row, t = g.bfs(int(v), with_ms=True)
            rows.append(row)
            ms += t
        return rows, ms

    rows, res["bfs_loop_64"] = timed(loop, reps)
    got, res["multi_64"] = timed(multi(s64, False), reps)
    res["counters_64"] = dict(zip(COUNTERS, (int(x) for x in g.debug_multi_bfs_counters())))
    got_lv, res["multi_64_levels"] = timed(multi(s64, True), reps)
    _, res["multi_1024"] = timed(multi(sources, False), max(reps // 2, 1))
    res["counters_1024"] = dict(zip(COUNTERS, (int(x) for x in g.debug_multi_bfs_counters())))
    _, res["multi_1024_levels"] = timed(multi(sources, True), 1)
    g.set_option("msbfs_look", 0)
    got_nl, res["multi_64_no_look"] = timed(multi(s64, False), reps)
    g.set_option("msbfs_look", 1)
    same = all(np.array_equal(got_lv[4][i], rows[i]) for i in range(64))
    for i in range(64):
        r, f, e, h = aggregates(hist_of(rows[i]))
        same = same and (int(got[0][i]), int(got[1][i]), int(got[2][i]), float(got[3][i])) == (r, f, e, h)
    same = same and all(np.array_equal(a, b) for a, b in zip(got, got_nl)) and all(np.array_equal(a, b) for a, b in zip(got, got_lv[:4]))
    res["rows_and_aggregates_equal_the_loops"] = bool(same)
    base = res["bfs_loop_64"]
    res["us_per_single_bfs"] = round(base["device_ms"] * 1e3 / 64, 1)
    res["loop_over_multi_device"] = round(base["device_ms"] / res["multi_64"]["device_ms"], 2)
    res["loop_over_multi_wall"] = round(base["wall_ms"] / res["multi_64"]["wall_ms"], 2)
    res["loop_over_multi_levels_device"] = round(base["device_ms"] / res["multi_64_levels"]["device_ms"], 2)
    res["loop_over_multi_levels_wall"] = round(base["wall_ms"] / res["multi_64_levels"]["wall_ms"], 2)
    res["no_look_over_look_device"] = round(res["multi_64_no_look"]["device_ms"] / res["multi_64"]["device_ms"], 2)
    res["us_per_source_1024"] = round(res["multi_1024"]["device_ms"] * 1e3 / 1024, 1)
    res["multi_64_beats_the_loop"] = bool(res["multi_64"]["device_ms"] < base["device_ms"] and res["multi_64"]["wall_ms"] < base["wall_ms"])
    g.close()
    return res, same


def kernel_stats(out_dir):
    """{graph: {variant: [{kernel, calls, total_us, avg_us}]}} of ONE 64-source call, and the csv"""
    lines = ["graph,variant,kernel,calls,total_us,avg_us,min_us,max_us"]
    split = {}
    for which in GRAPHS:
        split[which] = {}
        for look in (1, 0):
            with tempfile.TemporaryDirectory() as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                       os.path.abspath(__file__), "--trace-pass", which, "--look", str(look)]
                subprocess.run(cmd, check=True, timeout=600)
                found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                assert found, "rocprofv3 wrote no kernel_stats.csv"
                rows = list(csv.DictReader(open(found[0])))
            variant = "look" if look else "no_look"
            split[which][variant] = []
            for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
                name = r["Name"].split("(")[0].replace(",", ";").replace("void ", "")  # (a template's name carries its return type)
                if not name.startswith(KERNELS):
                    continue
                split[which][variant].append({"kernel": name, "calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 2),
                                              "avg_us": round(float(r["AverageNs"]) / 1e3, 2)})
                lines.append(f"{which},{variant},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                             f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(os.path.join(out_dir, "multibfs_kernel_stats.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return split


def trace_pass(args):
    """ONE 64-source call, aggregates only"""
    pkg, st = load_pkg(), load_streams()
    n, ops, sources = graph(st, args.trace_pass)
    g = build(pkg, n, ops)
    g.set_option("msbfs_look", args.look)
    reached = g.multi_bfs(sources[:64])[0]
    print(json.dumps({"trace_pass": args.trace_pass, "look": args.look, "reached": int(reached.sum()),
                      "counters": [int(x) for x in g.debug_multi_bfs_counters()]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-stats", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=list(GRAPHS), help=argparse.SUPPRESS)
    ap.add_argument("--look", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), bulk-built, one PCSR" for k, v in GRAPHS.items()}, "reps": args.reps,
           "timing": "device_ms: device events on the engine's stream around the level loops (host reads included, the copy of levels "
                     "excluded), for the loop the sum over its 64 calls; wall_ms: host clock around the whole call or loop, copies included"}
    ok = True
    for which in GRAPHS:
        print(which, file=sys.stderr, flush=True)
        res[which], same = measure(pkg, st, which, args.reps)
        ok = ok and same
    if args.kernel_stats:
        res["kernel_split_of_one_64_source_call"] = kernel_stats(args.out_dir)
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "multibfs_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "multibfs_bench: the rows or aggregates of the 64-source call differ from the loop of single calls"


if __name__ == "__main__":
    main()
