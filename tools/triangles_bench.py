"""Device triangle counts and common-neighbour counts (ppcsr_triangles / ppcsr_common_neighbours and their pppcsr_ forms) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

each on one PCSR and on 8 partitions on one GPU.  Per graph and form, device ms (median of --reps runs after a warm-up) of
triangles with and without tri[], stored edges with src < dst per second, triangles found, and common-neighbour pairs per
second for 1 M random pairs and for 1 M pairs drawn from stored edges (device form on one PCSR, host form on 8 partitions:
there is no device form over partitions).

Two yardsticks, on one PCSR:
  composition   s18 only (88.8 M wedges: the wedge list fits): what a user could do before this call — gather_neighbourhoods_device
                gives the CSR, torch keeps the upper part and enumerates the wedges (a, b, c), lookup_edges_device decides
                (a, c).  Timed with device events around the whole composition; it must find the same number of triangles and
                the dedicated call must be faster (asserted; both times and the ratio are recorded).
  scan          ppcsr_bench_scan_all on the same array, one pass over the slots: triangles ms over scan ms says how far from a
                streaming pass the call is (no threshold).

Writes profiles/triangles_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns a short pass per graph (one triangles call with tri[], one without, one common-neighbours call over the
                 edge pairs, on one PCSR) under rocprofv3 --kernel-trace --stats, in a run of its own, and writes
                 profiles/triangles_kernel_stats.csv."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import load_pkg, load_streams  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
PAIRS = 1_000_000
NO_EDGE = 0xFFFFFFFF


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


def pair_sets(n, ops):
    rng = np.random.default_rng(9)
    pick = rng.choice(len(ops), PAIRS, replace=False)
    return {"random": (rng.integers(0, n, PAIRS).astype(np.uint32), rng.integers(0, n, PAIRS).astype(np.uint32)),
            "edges": (np.ascontiguousarray(ops[pick, 0]), np.ascontiguousarray(ops[pick, 1]))}


def measure(pkg, n, ops, parts, reps):
    import torch
    g = build(pkg, n, ops, parts)
    key = np.unique(ops[:, 0].astype(np.uint64) * np.uint64(n) + ops[:, 1].astype(np.uint64))
    upper = int(np.count_nonzero((key // np.uint64(n)) < (key % np.uint64(n))))
    slots = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))
    res = {"partitions": parts, "slots": slots, "stored_pairs": int(len(key)), "edges_src_lt_dst": upper}

    def with_tri():
        tri, total, ms = g.triangles(with_ms=True)
        return (tri, total), ms

    def without_tri():
        _, total, ms = g.triangles(per_vertex=False, with_ms=True)
        return total, ms

    (tri, total), ms, ms_all = timed(with_tri, reps)
    total2, ms2, ms2_all = timed(without_tri, reps)
    res["triangles"] = {"found": int(total), "largest_tri": int(tri.max()), "vertices_in_a_triangle": int(np.count_nonzero(tri)),
                        "sum_tri_is_3_total": bool(int(tri.sum()) == 3 * total), "totals_equal": bool(total == total2),
                        "ms_with_tri": ms, "ms_with_tri_all": ms_all, "ms_total_only": ms2, "ms_total_only_all": ms2_all,
                        "edges_src_lt_dst_per_s": round(upper / (ms * 1e-3)), "edges_src_lt_dst_per_s_total_only": round(upper / (ms2 * 1e-3))}
    res["common_neighbours"] = {}
    counts = {}
    for name, (a, b) in pair_sets(n, ops).items():
        if parts == 1:
            da, db = torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda()
            out = torch.zeros(PAIRS, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            _, cms, call = timed(lambda: (None, g.common_neighbours_device(da.data_ptr(), db.data_ptr(), PAIRS, out.data_ptr(), with_ms=True)), reps)
            c = out.cpu().numpy().view(np.uint32)
        else:
            c, cms, call = timed(lambda: g.common_neighbours(a, b, with_ms=True), reps)
        counts[name] = c
        res["common_neighbours"][name] = {"pairs": PAIRS, "form": "device" if parts == 1 else "host", "kernel_ms": cms, "kernel_ms_all": call,
                                          "pairs_per_s": round(PAIRS / (cms * 1e-3)), "pairs_with_a_common_neighbour": int(np.count_nonzero(c)),
                                          "largest_count": int(c.max())}
    scan = [g.bench_scan_all()[0] for _ in range(reps + 1)][1:] if parts == 1 else \
        [sum(g.partition(k).bench_scan_all()[0] for k in range(parts)) for _ in range(reps + 1)][1:]
    res["scan_all_ms"] = round(float(np.median(scan)), 3)
    res["triangles_over_scan"] = round(ms / res["scan_all_ms"], 2)
    return res, g, tri, total, counts


def composition(g, n, reps):
    """triangles of the upper orientation from today's other public device calls: gather -> wedges in torch -> lookups"""
    import torch
    dev = "cuda"
    verts = torch.arange(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cap = g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), 0, 0, 0)
    dests = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def once():
        t0, t1, t2, t3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        t0.record()
        g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), dests.data_ptr(), 0, cap)
        t1.record()
        deg = rows[1:] - rows[:-1]
        src = torch.repeat_interleave(torch.arange(n, device=dev), deg)
        dst = dests.to(torch.int64)
        up = (src < dst) & (dst < n)
        a, b = src[up], dst[up]  # ascending (a, b): the gather keeps slot order, which is ascending dest
        udeg = torch.bincount(a, minlength=n)
        urows = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        urows[1:] = torch.cumsum(udeg, 0)
        lens = udeg[b]
        cum = torch.cumsum(lens, 0) - lens
        eidx = torch.repeat_interleave(torch.arange(len(a), device=dev), lens)
        off = torch.arange(len(eidx), device=dev) - cum[eidx]
        c = b[urows[b[eidx]] + off]
        qa, qc = a[eidx].to(torch.int32).contiguous(), c.to(torch.int32).contiguous()
        val = torch.empty(len(qa), dtype=torch.int32, device=dev)
        t2.record()
        torch.cuda.synchronize()
        g.lookup_edges_device(qa.data_ptr(), qc.data_ptr(), len(qa), val.data_ptr())
        found = int((val != -1).sum())
        t3.record()
        torch.cuda.synchronize()
        return (found, len(qa), int(up.sum())), (t0.elapsed_time(t3), t0.elapsed_time(t1), t1.elapsed_time(t2), t2.elapsed_time(t3))

    once()  # warm-up
    runs = [once() for _ in range(reps)]
    (found, wedges, upper) = runs[0][0]
    med = [round(float(np.median([r[1][k] for r in runs])), 3) for k in range(4)]
    return {"triangles": found, "wedges": wedges, "edges_src_lt_dst": upper, "ms": med[0], "ms_all": [round(r[1][0], 3) for r in runs],
            "gather_ms": med[1], "wedges_torch_ms": med[2], "lookups_ms": med[3]}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "triangles_kernel_stats.csv")
    lines = ["graph,kernel,calls,total_us,avg_us,min_us,max_us"]
    for which in GRAPHS:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--trace-pass", which]
            subprocess.run(cmd, check=True, timeout=900)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            rows = list(csv.DictReader(open(found[0])))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace(",", ";")
            if not name.startswith(("ppcsr::k_tri", "ppcsr::k_common")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE triangles call with tri[], ONE without, ONE common-neighbours call over the edge pairs"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    _, total = g.triangles()
    _, total2 = g.triangles(per_vertex=False)
    a, b = pair_sets(n, ops)["edges"]
    c = g.common_neighbours(a, b)
    print(json.dumps({"trace_pass": args.trace_pass, "triangles": total, "equal": total == total2, "pairs_with_a_common_neighbour": int(np.count_nonzero(c))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=list(GRAPHS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_stats:
        return kernel_stats(args)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), bulk-built" for k, v in GRAPHS.items()}, "reps": args.reps,
           "timing": "device events on the engine's stream (device_ms of the calls); the composition: device events around the whole of it"}
    ok = True
    for which in GRAPHS:
        n, ops = graph(st, which)
        print(f"{which} x1", file=sys.stderr, flush=True)
        one, g, tri1, total1, c1 = measure(pkg, n, ops, 1, args.reps)
        if which == "s18":
            comp = composition(g, n, max(3, args.reps // 2))
            comp["ratio_composition_over_triangles"] = round(comp["ms"] / one["triangles"]["ms_with_tri"], 2)
            comp["same_count"] = bool(comp["triangles"] == total1)
            comp["dedicated_call_is_faster"] = bool(one["triangles"]["ms_with_tri"] < comp["ms"])
            one["composition"] = comp
            ok = ok and comp["same_count"] and comp["dedicated_call_is_faster"]
        g.close()
        print(f"{which} x{P}", file=sys.stderr, flush=True)
        many, g, tri8, total8, c8 = measure(pkg, n, ops, P, args.reps)
        g.close()
        many["equal_to_one_pcsr"] = bool(total1 == total8 and np.array_equal(tri1, tri8) and all(np.array_equal(c1[k], c8[k]) for k in c1))
        many["ratio_over_one_pcsr"] = round(many["triangles"]["ms_with_tri"] / one["triangles"]["ms_with_tri"], 3)
        ok = ok and many["equal_to_one_pcsr"] and one["triangles"]["sum_tri_is_3_total"] and one["triangles"]["totals_equal"]
        res[which + "_pcsr"], res[which + "_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "triangles_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "triangles_bench: a check failed (equal results, or the dedicated call against the composition: see the record)"


if __name__ == "__main__":
    main()
