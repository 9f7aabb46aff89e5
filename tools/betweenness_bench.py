"""Device betweenness centrality and shortest-path counts (ppcsr_betweenness / ppcsr_path_counts and their pppcsr_ forms) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

each on one PCSR and on 8 partitions on one GPU, from K sources (the vertex of largest out-degree and K - 1 spread over the
ids).  Per graph and form, device ms per source (median of --reps runs after a warm-up): the whole betweenness call, its
forward phase alone (path_counts from the same sources), the backward sweep as the difference, and ppcsr_bfs from the same
sources in the same run — the per-source time is recorded as a multiple of that BFS (reporting, no threshold).

Yardstick:
  composition   s18, one PCSR: what a user could do before this call — gather_neighbourhoods_device gives the CSR, then a
                level-synchronous Brandes in torch (fp64, index_add_ per level).  Timed with device events around the whole of
                it; it must agree with the dedicated call within twice the bound of include/ppcsr.h (both sides carry the
                error), and both times and the ratio are recorded.

Writes profiles/betweenness_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE betweenness call per graph (one PCSR, the same K sources) under rocprofv3 --kernel-trace --stats, in
                 a run of its own, and writes profiles/betweenness_kernel_stats.csv."""
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

P, K = 8, 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
NO_LEVEL = 0xFFFFFFFF


def graph(st, which):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    n = 1 << scale
    top = int(np.bincount(s, minlength=n).argmax())
    return n, st.adds(s, d), [top] + [int(x) for x in (np.arange(1, K) * (n // K) + 5)]


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


def median_ms(call, reps):
    call()  # warm-up
    ms = [call() for _ in range(reps)]
    return round(float(np.median(ms)), 3), [round(x, 3) for x in ms]


def measure(pkg, n, ops, sources, parts, reps):
    g = build(pkg, n, ops, parts)
    bc = g.betweenness(sources)
    shape = []
    for s in sources:
        lv, sg = g.path_counts(s)
        reached = lv != NO_LEVEL
        shape.append({"source": s, "reached": int(reached.sum()), "depth": int(lv[reached].max()), "max_sigma": float(sg.max()),
                      "widest_level": int(np.bincount(lv[reached]).max())})
    total, total_all = median_ms(lambda: g.betweenness(sources, with_ms=True)[1], reps)
    fwd, _ = median_ms(lambda: sum(g.path_counts(s, with_ms=True)[2] for s in sources), reps)
    bfs, _ = median_ms(lambda: sum(g.bfs(s, with_ms=True)[1] for s in sources), reps)
    k = len(sources)
    res = {"partitions": parts, "sources": k, "ms_per_source": round(total / k, 3), "forward_ms_per_source": round(fwd / k, 3),
           "backward_ms_per_source": round((total - fwd) / k, 3), "bfs_ms_per_source": round(bfs / k, 3),
           "per_source_over_bfs": round(total / bfs, 2), "forward_over_bfs": round(fwd / bfs, 2), "call_ms_all": total_all,
           "per_source": shape, "nonzero_bc": int(np.count_nonzero(bc))}
    return res, g, bc


def composition(g, n, sources, reps):
    """betweenness from the other public device calls: gather -> CSR, then Brandes level by level with tensor ops"""
    import torch
    dev = "cuda"
    verts = torch.arange(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cap = g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), 0, 0, 0)
    dests = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def once():
        t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t0.record()
        g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), dests.data_ptr(), 0, cap)
        src = torch.repeat_interleave(torch.arange(n, device=dev), rows[1:] - rows[:-1])
        dst = dests.to(torch.int64)
        ok = dst < n
        src, dst = src[ok], dst[ok]
        rowp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rowp[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
        t1.record()
        bc = torch.zeros(n, dtype=torch.float64, device=dev)
        depth = 0
        for s in sources:
            level = torch.full((n,), -1, dtype=torch.int64, device=dev)
            sigma = torch.zeros(n, dtype=torch.float64, device=dev)
            level[s], sigma[s] = 0, 1.0
            front = torch.tensor([s], device=dev)
            stack, lv = [], 0
            while front.numel():
                lens = rowp[front + 1] - rowp[front]
                idx = torch.repeat_interleave(rowp[front] - torch.cumsum(lens, 0) + lens, lens)
                idx += torch.arange(idx.numel(), device=dev)
                w, v = dst[idx], torch.repeat_interleave(front, lens)
                level[w[level[w] < 0]] = lv + 1
                on = level[w] == lv + 1
                v, w = v[on], w[on]
                sigma.index_add_(0, w, sigma[v])
                stack.append((v, w))
                front = torch.unique(w)
                lv += 1
            depth = max(depth, lv - 1)
            delta = torch.zeros(n, dtype=torch.float64, device=dev)
            for v, w in reversed(stack):
                delta.index_add_(0, v, (sigma[v] / sigma[w]) * (1.0 + delta[w]))
            delta[s] = 0.0
            bc += delta
        t2.record()
        torch.cuda.synchronize()
        dmax = int((rowp[1:] - rowp[:-1]).max())
        return (bc.cpu().numpy(), depth, dmax), (t0.elapsed_time(t2), t0.elapsed_time(t1), t1.elapsed_time(t2))

    once()  # warm-up
    runs = [once() for _ in range(reps)]
    bc, depth, dmax = runs[0][0]
    med = [round(float(np.median([r[1][k] for r in runs])), 3) for k in range(3)]
    return bc, depth, dmax, {"ms": med[0], "ms_all": [round(r[1][0], 3) for r in runs], "export_ms": med[1], "brandes_ms": med[2]}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "betweenness_kernel_stats.csv")
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
            if not (name.startswith("ppcsr::k_bc") or name.startswith("ppcsr::k_bfs_collect")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE betweenness call from the K sources"""
    pkg, st = load_pkg(), load_streams()
    n, ops, sources = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    bc = g.betweenness(sources)
    print(json.dumps({"trace_pass": args.trace_pass, "sources": sources, "nonzero_bc": int(np.count_nonzero(bc))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
           "timing": "device events on the engine's stream (device_ms of the calls, summed over the sources for path_counts and "
                     "bfs); the composition: device events around the whole of it"}
    ok = True
    for which in GRAPHS:
        n, ops, sources = graph(st, which)
        print(f"{which} x1", file=sys.stderr, flush=True)
        one, g, bc1 = measure(pkg, n, ops, sources, 1, args.reps)
        if which == "s18":
            cbc, depth, dmax, comp = composition(g, n, sources, max(3, args.reps // 2))
            tol = 2 * (depth * (dmax + 2) + len(sources)) * 2.0 ** -53
            comp["ratio_composition_over_betweenness"] = round(comp["ms"] / (one["ms_per_source"] * len(sources)), 2)
            comp["bound"] = tol
            comp["worst_relative_difference"] = float(np.max(np.abs(cbc - bc1)[cbc > 0] / cbc[cbc > 0]))
            comp["within_the_bound"] = bool(np.all(np.abs(cbc - bc1) <= tol * cbc))
            one["composition"] = comp
            ok = ok and comp["within_the_bound"]
        g.close()
        print(f"{which} x{P}", file=sys.stderr, flush=True)
        many, g, bc8 = measure(pkg, n, ops, sources, P, args.reps)
        g.close()
        many["worst_relative_difference_to_one_pcsr"] = float(np.max(np.abs(bc8 - bc1)[bc1 > 0] / bc1[bc1 > 0]))
        many["same_support_as_one_pcsr"] = bool(np.array_equal(bc8 > 0, bc1 > 0))
        ok = ok and many["same_support_as_one_pcsr"]
        res[which + "_pcsr"], res[which + "_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "betweenness_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "betweenness_bench: a check failed (see the record)"


if __name__ == "__main__":
    main()
