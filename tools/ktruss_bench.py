"""Device edge support and truss numbers (ppcsr_edge_support / ppcsr_ktruss and the pppcsr_ forms) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the other consumers' tools: RMAT scale 18, 2 M adds (seed 31), bulk-built

each on one PCSR and on 8 partitions on one GPU, results checked equal.  Per graph and form: device ms of the whole call (median
of --reps runs after a warm-up; device events on the engine's stream) of edge_support and of ktruss, the counters of
ppcsr_debug_ktruss_counters, and beside them on the same graph the ms of ppcsr_triangles (support finds every triangle three
times where triangles finds it once: the ratio is recorded, whatever it is), of ppcsr_kcore and of ppcsr_bench_scan_all.

On s18 the counters are compared with the model's levels and sub-rounds (tests/truss_model.py: a synchronous peel on the host),
and the composition baseline is timed: what a user could do before these calls — gather_neighbourhoods_device, a copy to the
host, the numpy sub-round peel of tests/truss_model.py — wall clock around the whole of it, once.  The tool asserts identical
truss numbers and records the ratio; it asserts nothing about its size.  (The model is not run on c2: its wedge enumeration
there is beyond a tool's patience; the two forms are still checked equal.)

Writes profiles/ktruss_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE ktruss call per graph (one PCSR) under rocprofv3 --kernel-trace --stats, in a run of its own, and
                 writes profiles/ktruss_kernel_stats.csv."""
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
from truss_model import counters_of, model_truss  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
COUNTERS = ("edges", "triangles", "levels", "subrounds", "max_subrounds_in_a_level", "widest_frontier", "frontier_edges_to_long_kernel", "host_reads")


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


def timed(call, reps):
    call()  # warm-up
    ms, out = [], None
    for _ in range(reps):
        out, t = call()
        ms.append(t)
    return out, round(float(np.median(ms)), 3), [round(x, 3) for x in ms]


def measure(pkg, n, ops, parts, reps):
    g = build(pkg, n, ops, parts)
    slots = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))
    m = g.edge_support()[0].shape[0]
    buf, vt = np.empty((m, 3), np.uint32), np.empty(n, np.uint32)
    import ctypes
    count, total, tmax = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()

    # (the calls themselves, into buffers of the known size: the binding's size query is not part of the time)
    def support():
        ms = g._consumer("edge_support", buf.ctypes.data, m, ctypes.byref(count), ctypes.byref(total))
        return (buf.copy(), total.value), ms

    def ktruss():
        ms = g._consumer("ktruss", buf.ctypes.data, m, ctypes.byref(count), ctypes.byref(tmax), vt.ctypes.data)
        return (buf.copy(), tmax.value, vt.copy()), ms

    sup, sup_ms, sup_all = timed(support, reps)
    tr, tr_ms, tr_all = timed(ktruss, reps)
    ctr = [int(x) for x in g.debug_ktruss_counters()]
    (_, tri_total), tri_ms, _ = timed(lambda: (lambda r: ((None, r[1]), r[2]))(g.triangles(per_vertex=False, with_ms=True)), reps)
    _, kc_ms, _ = timed(lambda: (None, g.kcore(with_ms=True)[2]), reps)
    scan = [g.bench_scan_all()[0] for _ in range(reps + 1)][1:] if parts == 1 else \
        [sum(g.partition(k).bench_scan_all()[0] for k in range(parts)) for _ in range(reps + 1)][1:]
    scan_ms = round(float(np.median(scan)), 3)
    res = {"partitions": parts, "slots": slots, "upper_edges": m, "triangles": int(sup[1]), "triangles_is_ppcsr_triangles": bool(sup[1] == tri_total),
           "tmax": int(tr[1]), "counters": dict(zip(COUNTERS, ctr)), "edge_support_ms": sup_ms, "edge_support_ms_all": sup_all, "ktruss_ms": tr_ms,
           "ktruss_ms_all": tr_all, "us_per_subround": round((tr_ms - sup_ms) * 1e3 / max(ctr[3], 1), 2), "triangles_ms": tri_ms, "kcore_ms": kc_ms,
           "scan_all_ms": scan_ms, "edge_support_over_triangles": round(sup_ms / tri_ms, 2), "ktruss_over_kcore": round(tr_ms / kc_ms, 2),
           "ktruss_over_scan": round(tr_ms / scan_ms, 2)}
    return res, g, sup, tr


def composition(g, n):
    """truss numbers from the other public calls: gather on the device, a copy to the host, the numpy peel of the model"""
    import torch
    verts = torch.arange(n, dtype=torch.int32, device="cuda")
    rows = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cap = g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), 0, 0, 0)
    dests = torch.empty(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), dests.data_ptr(), 0, cap)
    torch.cuda.synchronize()
    r, d = rows.cpu().numpy(), dests.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    t1 = time.perf_counter()
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(r))
    mt = model_truss(src, d, n)
    t2 = time.perf_counter()
    return mt, {"ms": round((t2 - t0) * 1e3, 1), "gather_and_copy_ms": round((t1 - t0) * 1e3, 1), "host_peel_ms": round((t2 - t1) * 1e3, 1)}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "ktruss_kernel_stats.csv")
    lines = ["graph,kernel,calls,total_us,avg_us,min_us,max_us"]
    for which in args.graphs:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--trace-pass", which]
            subprocess.run(cmd, check=True, timeout=900)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            rows = list(csv.DictReader(open(found[0])))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace(",", ";")
            if not name.startswith(("ppcsr::k_tr_", "ppcsr::k_kc_")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE ktruss call into buffers of the known size (the size query before it runs stage 1 only)"""
    import ctypes
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    count, tmax = ctypes.c_uint64(), ctypes.c_uint32()
    g._consumer("ktruss", None, 0, ctypes.byref(count), None, None)
    buf = np.empty((count.value, 3), np.uint32)
    g._consumer("ktruss", buf.ctypes.data, count.value, ctypes.byref(count), ctypes.byref(tmax), None)
    print(json.dumps({"trace_pass": args.trace_pass, "edges": int(count.value), "tmax": int(tmax.value)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--graphs", nargs="+", choices=list(GRAPHS), default=list(GRAPHS))
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=list(GRAPHS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_stats:
        return kernel_stats(args)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {k: f"RMAT scale {GRAPHS[k][0]}, {GRAPHS[k][1]} adds (seed {GRAPHS[k][2]}), bulk-built" for k in args.graphs}, "reps": args.reps,
           "timing": "device events on the engine's stream (device_ms of the calls, the whole call); the composition: wall clock, once",
           "support_variant": "every edge counts its own triangles (each triangle found three times); the anchored variant was not built"}
    ok = True
    for which in args.graphs:
        n, ops = graph(st, which)
        print(f"{which} x1", file=sys.stderr, flush=True)
        one, g, sup1, tr1 = measure(pkg, n, ops, 1, args.reps)
        if which == "s18":
            mt, comp = composition(g, n)
            comp["same_truss_numbers"] = bool(np.array_equal(tr1[0][:, 2], mt["truss"]) and np.array_equal(tr1[0][:, 0], mt["a"]) and np.array_equal(tr1[0][:, 1], mt["b"]))
            comp["ratio_composition_over_ktruss"] = round(comp["ms"] / one["ktruss_ms"], 1)
            one["composition"] = comp
            one["model_counters"] = dict(zip(COUNTERS[:6], counters_of(mt)))
            one["counters_are_the_models"] = bool(list(one["counters"].values())[:6] == counters_of(mt))
            ok = ok and comp["same_truss_numbers"] and one["counters_are_the_models"]
        g.close()
        print(f"{which} x{P}", file=sys.stderr, flush=True)
        many, g, sup8, tr8 = measure(pkg, n, ops, P, args.reps)
        g.close()
        many["equal_to_one_pcsr"] = bool(np.array_equal(sup1[0], sup8[0]) and sup1[1] == sup8[1] and np.array_equal(tr1[0], tr8[0]) and tr1[1] == tr8[1]
                                         and np.array_equal(tr1[2], tr8[2]) and list(one["counters"].values())[:6] == list(many["counters"].values())[:6])  # ([6] depends on the slot layout)
        many["ktruss_ratio_over_one_pcsr"] = round(many["ktruss_ms"] / one["ktruss_ms"], 3)
        ok = ok and many["equal_to_one_pcsr"] and one["triangles_is_ppcsr_triangles"]
        res[which + "_pcsr"], res[which + "_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "ktruss_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "ktruss_bench: a check failed (equal results on both forms, the model's truss numbers and counters: see the record)"


if __name__ == "__main__":
    main()
