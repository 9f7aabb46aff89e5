"""Device greedy colouring and maximal independent set (ppcsr_colouring / ppcsr_mis) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

on one PCSR (s18 also on 8 partitions on one GPU).  Per graph: both calls for the three vertex orders, ppcsr_kcore and one
ppcsr_bench_scan_all beside them, all INTERLEAVED — every repeat runs every variant once, in the same order — and reported as
medians with all the samples (device ms of the whole call: host round trips included).  An order whose colouring needs more than
--max-rounds rounds on a graph is run once and not repeated (its count is recorded: `id` on an RMAT graph is a long chain).
With each time its yardstick:
  colouring   ppcsr_kcore on the same graph in the same run: the same export and the same loop shape, a launch and a host read
              per round (us_per_round of both are recorded)
  mis         rounds x one scan of the array, the floor its design implies
  composition s18: what a user has without the calls — gather_neighbourhoods of every vertex to the host, then the host greedy
              of tests/colouring_model.py (colouring and MIS); equal arrays are asserted

Writes profiles/colouring_bench.json (--out-dir: elsewhere).  (profiles/colouring_bench_low_word_variant.json is this tool's record
from a build whose round kernel could also keep the colours below 64 in a lane-private register, both variants interleaved: that
one was the slower and is not in the library.)
--kernel-stats   reruns ONE colouring and ONE mis call (random order) per graph under rocprofv3 --kernel-trace --stats, in a run of
                 its own, and writes profiles/colouring_kernel_stats.csv: the split export / pred / rounds, pass / vertex step."""
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
from colouring_model import graph as model_graph, model_colouring, model_mis  # noqa: E402
from helpers import load_pkg, load_streams  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
ORDERS = ("random", "degree", "id")
SEED = 3


def graph(st, which):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    return 1 << scale, st.adds(s, d)


def build(pkg, n, ops, parts):
    import torch
    if parts == 1:
        g = pkg.PCSR(n)
        g.bulk_build(ops)
        return g
    g = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=parts)
    t = torch.from_numpy(ops.view(np.int32)).cuda()
    torch.cuda.synchronize()
    g.bulk_build_device(t.data_ptr(), len(ops))
    del t
    torch.cuda.empty_cache()
    return g


def med(xs):
    return round(float(np.median(xs)), 3)


def measure(g, parts, reps, max_rounds):
    """every variant once per repeat, interleaved"""
    results, counters, variants = {}, {}, {}

    def colouring(order):
        def run():
            colour, ncol, ms = g.colouring(order, SEED, with_ms=True)
            return (colour, ncol), ms
        return run

    def mis(order):
        def run():
            mask, size, ms = g.mis(order, SEED, with_ms=True)
            return (mask, size), ms
        return run

    def kcore():
        core, kmax, ms = g.kcore(with_ms=True)
        return kmax, ms

    def scan():
        if parts == 1:
            return None, g.bench_scan_all()[0]
        return None, sum(g.partition(k).bench_scan_all()[0] for k in range(parts))

    once = {}
    for order in ORDERS:  # warm-up: results and counters; the orders that are too long a chain to repeat
        results["colouring", order], ms = colouring(order)()
        counters["colouring", order] = g.debug_colouring_counters().tolist()
        if counters["colouring", order][0] > max_rounds:
            once[order] = round(ms, 3)
        else:
            variants["colouring", order] = colouring(order)
        results["mis", order], _ = mis(order)()
        counters["mis", order] = g.debug_mis_counters().tolist()
        variants["mis", order] = mis(order)
    variants["kcore", ""] = kcore
    variants["scan", ""] = scan
    kcore(), scan()
    samples = {k: [] for k in variants}
    for _ in range(reps):
        for k, run in variants.items():
            out, ms = run()
            samples[k].append(round(ms, 3))
            if k[0] == "colouring":
                assert np.array_equal(out[0], results[k][0]) and out[1] == results[k][1], k
    return results, counters, samples, once


def report(results, counters, samples, once):
    scan_ms, kcore_ms = med(samples["scan", ""]), med(samples["kcore", ""])
    res = {"scan_all_ms": scan_ms, "scan_all_ms_all": samples["scan", ""], "kcore_ms": kcore_ms, "kcore_ms_all": samples["kcore", ""]}
    for order in ORDERS:
        c, m = counters["colouring", order], counters["mis", order]
        col = {"rounds": c[0], "widest_frontier": c[1], "long_lists": c[2], "adjacency_entries": c[3], "colours": c[4], "extra_window_passes": c[5],
               "launches": c[6], "host_reads": c[7]}
        if order in once:
            col["ms_single_run_not_repeated"] = once[order]
        else:
            a = samples["colouring", order]
            col.update(ms=med(a), ms_all=a, us_per_round=round(med(a) * 1e3 / max(c[0], 1), 2), over_kcore=round(med(a) / kcore_ms, 2),
                       spread=round((max(a) - min(a)) / med(a), 3))
        s = samples["mis", order]
        floor = round(m[1] * scan_ms + m[5] * scan_ms, 3)
        res[order] = {"colouring": col,
                      "mis": {"rounds": m[0], "passes": m[1], "members_after_round_1": m[2], "undecided_after_round_1": m[3], "size": m[4],
                              "degree_passes": m[5], "launches": m[6], "host_reads": m[7], "ms": med(s), "ms_all": s,
                              "floor_passes_x_scan_ms": floor, "over_floor": round(med(s) / floor, 2) if floor else None,
                              "in_set_is_colour_0": bool(np.array_equal(results["mis", order][0], results["colouring", order][0] == 0))}}
    return res


def composition(g, n, results):
    """gather every neighbourhood to the host, keep the upper pairs, colour and pick greedily on the host (the model)"""
    out = {}
    t0 = time.perf_counter()
    rows, dests = g.gather_neighbourhoods(np.arange(n, dtype=np.uint32), with_values=False)[:2]
    t1 = time.perf_counter()
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rows, np.int64)))
    dst = np.asarray(dests, np.int64)
    out["gather_and_d2h_ms"] = round((t1 - t0) * 1e3, 1)
    same = True
    for order in ("random", "degree"):
        t2 = time.perf_counter()
        rws, nbr, keys, _ = model_graph(src, dst, n, ORDERS.index(order), SEED)
        colour = model_colouring(rws, nbr, keys)
        t3 = time.perf_counter()
        mask = model_mis(rws, nbr, keys)
        t4 = time.perf_counter()
        ok = bool(np.array_equal(colour, results["colouring", order][0]) and np.array_equal(mask, results["mis", order][0]))
        same = same and ok
        out[order] = {"host_colouring_ms": round((t3 - t2) * 1e3, 1), "host_mis_ms": round((t4 - t3) * 1e3, 1), "equal_arrays": ok}
    out["equal_arrays"] = same
    return out


def kernel_stats(args):
    out = os.path.join(args.out_dir, "colouring_kernel_stats.csv")
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
            if not name.startswith(("ppcsr::k_kc", "ppcsr::k_col", "ppcsr::k_mis", "void ppcsr::k_col")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE colouring and ONE mis call, random order"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    _, ncol = g.colouring("random", SEED)
    _, size = g.mis("random", SEED)
    print(json.dumps({"trace_pass": args.trace_pass, "colours": int(ncol), "mis_size": int(size)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
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
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), bulk-built" for k, v in GRAPHS.items()}, "reps": args.reps, "seed": SEED,
           "timing": "device events on the engine's stream (device_ms of the calls), every variant once per repeat, interleaved; "
                     "the composition: host wall clock"}
    ok = True
    for which, forms in (("c2", (1,)), ("s18", (1, P))):
        n, ops = graph(st, which)
        first = None
        for parts in forms:
            print(f"{which} x{parts}", file=sys.stderr, flush=True)
            g = build(pkg, n, ops, parts)
            results, counters, samples, once = measure(g, parts, args.reps, args.max_rounds)
            rec = report(results, counters, samples, once)
            rec["partitions"] = parts
            rec["slots"] = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))
            ok = ok and all(rec[o]["mis"]["in_set_is_colour_0"] for o in ORDERS)
            if which == "s18" and parts == 1:
                rec["composition"] = composition(g, n, results)
                ok = ok and rec["composition"]["equal_arrays"]
            if first is None:
                first = results
            else:
                rec["equal_to_one_pcsr"] = bool(all(np.array_equal(results[k][0], first[k][0]) and results[k][1] == first[k][1] for k in first))
                ok = ok and rec["equal_to_one_pcsr"]
            g.close()
            res[which + ("_pcsr" if parts == 1 else "_pppcsr")] = rec
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "colouring_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "colouring_bench: a check failed (equal results: see the record)"


if __name__ == "__main__":
    main()
