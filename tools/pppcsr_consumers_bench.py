"""Device BFS / PageRank over a partitioned graph (pppcsr_bfs / pppcsr_pagerank) against one engine holding the same graph
(ppcsr_bfs / ppcsr_pagerank), on config #4's core graph: 10 M vertices, 100 M RMAT edges (scale-24 ids % n, permuted labels,
what bench.py's Workload.core makes for config 4), bulk-built into 8 partitions on one GPU and into one PCSR.

  per form   BFS from vertex 0 and two other starts, PageRank with all-ones values: device ms (median of --reps runs after a
             warm-up), levels, vertices reached, edges/s (edges held / device time)
  parity     levels equal and PageRank bitwise equal between the two forms (slot N-1 of every array checked free first)
  single     10^4 single get_neighbourhood calls on the PPPCSR: us per call, and the host-template path (bfs.h / pagerank.h
             with T = PPPCSR: one call per reached vertex, getNode + get_neighbourhood per vertex) EXTRAPOLATED from it

Writes profiles/pppcsr_consumers.json (--out-dir: elsewhere).  --kernel-stats reruns a short PPPCSR-only pass (one BFS from vertex 0, one PageRank)
under rocprofv3 --kernel-trace --stats and writes the kernel split to profiles/pppcsr_consumers_kernel_stats.csv."""
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

N_VERT, SCALE, EDGES, P = 10_000_000, 24, 100_000_000, 8


def core_graph(st, edges):
    s, d = st.rmat_edges_folded(N_VERT, SCALE, edges, seed=1)
    return st.adds(st.permute_labels(s, N_VERT), st.permute_labels(d, N_VERT))


def last_slots_free(engines):
    for e in engines:
        items, _ = e.state()
        v = items[-1]
        if v[2] != 0 and v[1] != 0xFFFFFFFF and v[2] != 0xFFFFFFFF:
            return False
    return True


def measure(g, starts, reps, edges):
    out = {"bfs": []}
    levels = {}
    for s in starts:
        g.bfs(s, with_ms=True)  # warm-up
        ms = []
        for _ in range(reps):
            lv, t = g.bfs(s, with_ms=True)
            ms.append(t)
        levels[s] = lv
        reached = lv != 0xFFFFFFFF
        med = float(np.median(ms))
        out["bfs"].append({"start": int(s), "device_ms_median": round(med, 3), "device_ms_all": [round(x, 3) for x in ms],
                           "levels": int(lv[reached].max()) + 1, "reached": int(reached.sum()),
                           "edges_per_s": round(edges / (med * 1e-3))})
    ones = np.ones(N_VERT, np.float32)
    g.pagerank(ones, with_ms=True)
    ms = []
    for _ in range(reps):
        pr, t = g.pagerank(ones, with_ms=True)
        ms.append(t)
    med = float(np.median(ms))
    out["pagerank"] = {"device_ms_median": round(med, 3), "device_ms_all": [round(x, 3) for x in ms], "edges_per_s": round(edges / (med * 1e-3))}
    return out, levels, pr


def kernel_stats(args):
    """the short pass under rocprofv3; its stats CSV rewritten as kernel,calls,total_us,avg_us,min_us,max_us"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--trace-pass", "--edges", str(args.edges)]
        subprocess.run(cmd, check=True, timeout=1500)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        assert found, "rocprofv3 wrote no kernel_stats.csv"
        rows = list(csv.DictReader(open(found[0])))
    out = os.path.join(args.out_dir, "pppcsr_consumers_kernel_stats.csv")
    with open(out, "w") as f:
        f.write("kernel,calls,total_us,avg_us,min_us,max_us\n")
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace(",", ";")
            f.write(f"{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                    f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}\n")
    print(open(out).read())


def trace_pass(args):
    import torch
    pkg, st = load_pkg(), load_streams()
    core = core_graph(st, args.edges)
    pp = pkg.PPPCSR(N_VERT, numDomain=1, partitionsPerDomain=P)
    t = torch.from_numpy(core.view(np.int32)).cuda()
    torch.cuda.synchronize()
    pp.bulk_build_device(t.data_ptr(), len(core))
    del t
    lv = pp.bfs(0)
    pp.pagerank(np.ones(N_VERT, np.float32))
    print(json.dumps({"trace_pass": True, "bfs_levels_from_0": int(lv[lv != 0xFFFFFFFF].max()) + 1, "partitions": P}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--single", type=int, default=10_000)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_stats:
        return kernel_stats(args)
    import torch
    pkg, st = load_pkg(), load_streams()
    t0 = time.perf_counter()
    core = core_graph(st, args.edges)
    t_gen = time.perf_counter() - t0
    pp = pkg.PPPCSR(N_VERT, numDomain=1, partitionsPerDomain=P)
    t = torch.from_numpy(core.view(np.int32)).cuda()
    torch.cuda.synchronize()
    pp.bulk_build_device(t.data_ptr(), len(core))
    del t
    torch.cuda.empty_cache()
    one = pkg.PCSR(N_VERT)
    one.bulk_build(core)
    parts = [pp.partition(k) for k in range(P)]
    slots_free = last_slots_free(parts + [one])
    edges = int(one.scan_all()[0][-1])
    rng = np.random.default_rng(4)
    starts = [0] + [int(x) for x in rng.integers(1, N_VERT, 2)]
    r_pp, lv_pp, pr_pp = measure(pp, starts, args.reps, edges)
    r_one, lv_one, pr_one = measure(one, starts, args.reps, edges)
    equal_levels = all(np.array_equal(lv_pp[s], lv_one[s]) for s in starts)
    equal_pr = pr_pp.tobytes() == pr_one.tobytes()
    # the host-template path: single calls through the C ABI
    q = rng.integers(0, N_VERT, args.single).astype(np.int64)
    pp.get_neighbourhood(int(q[0]))
    t0 = time.perf_counter()
    for v in q:
        pp.get_neighbourhood(int(v))
    us = (time.perf_counter() - t0) / len(q) * 1e6
    reached = r_pp["bfs"][0]["reached"]
    res = {
        "graph": f"config #4 core: {N_VERT} vertices, {args.edges} RMAT adds (scale-{SCALE} ids % n, permuted labels), bulk-built",
        "edges_held": edges, "partitions": P, "slots_pppcsr": int(sum(e.geometry()[0] for e in parts)), "slots_pcsr": int(one.geometry()[0]),
        "graph_generation_s": round(t_gen, 1),
        "pppcsr": r_pp, "pcsr": r_one,
        "ratio_pppcsr_over_pcsr": {"bfs": [round(a["device_ms_median"] / b["device_ms_median"], 3) for a, b in zip(r_pp["bfs"], r_one["bfs"])],
                                   "pagerank": round(r_pp["pagerank"]["device_ms_median"] / r_one["pagerank"]["device_ms_median"], 3)},
        "last_slots_free": slots_free, "levels_equal": equal_levels, "pagerank_bitwise_equal": equal_pr,
        "single_get_neighbourhood_us": round(us, 2),
        "host_template_EXTRAPOLATED": {
            "note": "not measured: the single-call time above times the calls the templates make",
            "bfs_from_0_s": round(reached * us * 1e-6, 1), "pagerank_s": round(2 * N_VERT * us * 1e-6, 1)},
    }
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "pppcsr_consumers.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
