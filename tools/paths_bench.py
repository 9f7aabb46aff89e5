"""Device shortest paths and connected components (ppcsr_sssp / ppcsr_components and their pppcsr_ forms) on the two graphs the
other consumers are measured on:

  c2   config #2's graph: RMAT scale 20, 10 M adds, bulk-built into one PCSR
  c4   config #4's core graph: 10 M vertices, --edges RMAT adds (scale-24 ids % n, permuted labels), bulk-built into 8
       partitions on one GPU and into one PCSR

Per graph and form, device ms (median of --reps runs after a warm-up) of
  unit     sssp with every value 1, beside bfs from the same starts in the same process (levels must equal distances)
  weighted sssp with values uniform in [1, 2^20] (the counter hash of streams.py)
  cc       components
and on c4 the 8-partition form against the one PCSR: results equal, time ratio.

Writes profiles/paths_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns a short pass per graph (one weighted sssp from the first start, one components call) under
                 rocprofv3 --kernel-trace --stats and writes profiles/paths_kernel_stats.csv: the launch counts are the
                 rounds of the calls, the k_cc_hook / k_sssp_edges times the streaming rates.
--passes-model   no GPU: the relaxation work of the frontier schedule on c2, counted by a synchronous numpy replica (rounds,
                 edges relaxed per reachable edge — one is what Dijkstra needs); merged into the JSON record."""
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

N4, SCALE4, EDGES4, P = 10_000_000, 24, 100_000_000, 8
N2, SCALE2, EDGES2 = 1 << 20, 20, 10_000_000
W_HI = 1 << 20
NO_PATH, NO_LEVEL = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF


_GRAPHS = {}


def graph(st, which, edges, weighted):
    """(n, adds) of a graph; generated once per process"""
    key = (which, edges, weighted)
    if key not in _GRAPHS:
        _GRAPHS[key] = _graph(st, which, edges, weighted)
    return _GRAPHS[key]


def _graph(st, which, edges, weighted):
    if which == "c2":
        s, d = st.rmat_edges(SCALE2, EDGES2, seed=1)
        n = N2
    else:
        s, d = st.rmat_edges_folded(N4, SCALE4, edges, seed=1)
        s, d = st.permute_labels(s, N4), st.permute_labels(d, N4)
        n = N4
    ops = st.adds(s, d)
    if weighted:
        ops[:, 2] = (st.uniform_ints(77, len(ops), W_HI) + 1).astype(np.uint32)
    return n, ops


def starts_of(which, n, ops):
    """c4: the starts of tools/pppcsr_consumers_bench.py (its BFS times are the yardstick); c2: vertex 0 and the sources of two
    adds (most vertices of the scale-20 graph have no out-edge: a random start reaches nothing)"""
    if which == "c2":
        return [0, int(ops[1, 0]), int(ops[len(ops) // 2, 0])]
    rng = np.random.default_rng(4)
    return [0] + [int(x) for x in rng.integers(1, n, 2)]


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


def slots_of(g, parts):
    return int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))


def timed(call, reps):
    call()  # warm-up
    ms, out = [], None
    for _ in range(reps):
        out, t = call()
        ms.append(t)
    return out, round(float(np.median(ms)), 3), [round(x, 3) for x in ms]


def measure(pkg, st, which, edges, parts, reps):
    """one graph in one form: the unit-value build (bfs beside sssp, components), then the weighted build (sssp)"""
    n, ops = graph(st, which, edges, weighted=False)
    starts = starts_of(which, n, ops)
    print(f"{which} x{parts}: unit values", file=sys.stderr, flush=True)
    g = build(pkg, n, ops, parts)
    res = {"partitions": parts, "slots": slots_of(g, parts), "unit": [], "weighted": []}
    keep = {}
    for s in starts:
        lv, b_ms, b_all = timed(lambda: g.bfs(s, with_ms=True), reps)
        ds, s_ms, s_all = timed(lambda: g.sssp(s, with_ms=True), reps)
        want = lv.astype(np.uint64)
        want[lv == NO_LEVEL] = NO_PATH
        res["unit"].append({"start": s, "bfs_ms": b_ms, "bfs_ms_all": b_all, "sssp_ms": s_ms, "sssp_ms_all": s_all,
                            "ratio_sssp_over_bfs": round(s_ms / b_ms, 3), "levels": int(lv[lv != NO_LEVEL].max()) + 1,
                            "reached": int((lv != NO_LEVEL).sum()), "levels_equal_distances": bool(np.array_equal(ds, want))})
    lab, c_ms, c_all = timed(lambda: g.components(with_ms=True), reps)
    res["components"] = {"ms": c_ms, "ms_all": c_all, "components": int(np.count_nonzero(lab == np.arange(n, dtype=np.uint32))),
                         "largest": int(np.bincount(lab).max())}
    keep["labels"] = lab
    g.close()
    n, ops = graph(st, which, edges, weighted=True)
    print(f"{which} x{parts}: weighted", file=sys.stderr, flush=True)
    g = build(pkg, n, ops, parts)
    for s in starts:
        ds, s_ms, s_all = timed(lambda: g.sssp(s, with_ms=True), reps)
        reached = ds != np.uint64(NO_PATH)
        res["weighted"].append({"start": s, "sssp_ms": s_ms, "sssp_ms_all": s_all, "reached": int(reached.sum()),
                                "max_distance": int(ds[reached].max())})
        keep[s] = ds
    g.close()
    return res, keep


def kernel_stats(args):
    """a short pass per graph under rocprofv3; the stats CSVs rewritten as graph,kernel,calls,total_us,avg_us,min_us,max_us"""
    out = os.path.join(args.out_dir, "paths_kernel_stats.csv")
    lines = ["graph,kernel,calls,total_us,avg_us,min_us,max_us"]
    for which in ("c2", "c4"):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--trace-pass", which, "--edges", str(args.edges)]
            subprocess.run(cmd, check=True, timeout=900)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            assert found, "rocprofv3 wrote no kernel_stats.csv"
            rows = list(csv.DictReader(open(found[0])))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"].split("(")[0].replace(",", ";")
            if not name.startswith(("ppcsr::k_sssp", "ppcsr::k_cc", "ppcsr::k_bfs")):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """c2 on one PCSR, c4 on 8 partitions: ONE weighted sssp from the first start and ONE components call, nothing else that
    launches their kernels (k_bfs_bits runs once per streaming round of the sssp, k_bfs_collect once per rebuilt list)"""
    pkg, st = load_pkg(), load_streams()
    which = args.trace_pass
    n, ops = graph(st, which, args.edges, weighted=True)
    g = build(pkg, n, ops, 1 if which == "c2" else P)
    ds = g.sssp(0)
    lab = g.components()
    print(json.dumps({"trace_pass": which, "reached": int((ds != np.uint64(NO_PATH)).sum()), "slots": slots_of(g, 1 if which == "c2" else P),
                      "components": int(np.count_nonzero(lab == np.arange(n, dtype=np.uint32)))}))


def passes_model(args):
    """the frontier schedule replayed synchronously on c2's weighted graph, from the stream alone (the last add of a pair
    wins): every round relaxes the out-edges of the vertices whose distance fell in the round before"""
    st = load_streams()
    n, ops = graph(st, "c2", 0, weighted=True)
    stream = ops
    key = (ops[:, 0].astype(np.uint64) << np.uint64(32)) | ops[:, 1].astype(np.uint64)
    _, idx = np.unique(key[::-1], return_index=True)
    ops = ops[::-1][idx]  # sorted by (src, dst), the last add of every pair
    src, dst, val = ops[:, 0].astype(np.int64), ops[:, 1].astype(np.int64), ops[:, 2].astype(np.uint64)
    rows = np.searchsorted(src, np.arange(n + 1))
    big = max(64, n // 256)
    out = []
    for start in starts_of("c2", n, stream):
        dist = np.full(n, NO_PATH, np.uint64)
        dist[start] = 0
        active = np.array([start], np.int64)
        rounds = relaxed = streamed = 0
        sizes = []
        while len(active):
            a, lens = rows[active], rows[active + 1] - rows[active]
            e = np.repeat(a - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
            nd, t = np.repeat(dist[active], lens) + val[e], dst[e]
            order = np.lexsort((nd, t))
            t, nd = t[order], nd[order]
            first = np.ones(len(t), bool)
            first[1:] = t[1:] != t[:-1]
            t, nd = t[first], nd[first]
            fell = nd < dist[t]
            dist[t[fell]] = nd[fell]
            rounds += 1
            relaxed += len(e)
            streamed += int(len(active) >= big)
            sizes.append(int(len(active)))
            active = t[fell]
        reached = dist != np.uint64(NO_PATH)
        reach_edges = int((rows[1:] - rows[:-1])[reached].sum())
        out.append({"start": start, "rounds": rounds, "streaming_rounds": streamed, "active_per_round": sizes,
                    "edges_relaxed": int(relaxed), "reachable_edges": reach_edges,
                    "relaxations_per_reachable_edge": round(relaxed / max(reach_edges, 1), 3)})
    path = os.path.join(args.out_dir, "paths_bench.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec["passes_model_c2"] = {"note": "synchronous numpy replica of the frontier schedule (no GPU): counts, not times", "edges_held": int(len(ops)),
                              "streaming_threshold": big, "per_start": out}
    with open(path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec["passes_model_c2"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--edges", type=int, default=EDGES4)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--passes-model", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=["c2", "c4"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args)
    if args.kernel_stats:
        return kernel_stats(args)
    if args.passes_model:
        return passes_model(args)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {"c2": f"config #2: {N2} vertices, {EDGES2} RMAT adds (scale {SCALE2}), bulk-built",
                      "c4": f"config #4 core: {N4} vertices, {args.edges} RMAT adds (scale-{SCALE4} ids % n, permuted labels), bulk-built"},
           "values": f"unit: all 1; weighted: uniform in [1, {W_HI}]", "reps": args.reps}
    res["c2_pcsr"], _ = measure(pkg, st, "c2", args.edges, 1, args.reps)
    res["c4_pppcsr"], k8 = measure(pkg, st, "c4", args.edges, P, args.reps)
    res["c4_pcsr"], k1 = measure(pkg, st, "c4", args.edges, 1, args.reps)
    a, b = res["c4_pppcsr"], res["c4_pcsr"]
    res["c4_equal"] = {"distances": all(np.array_equal(k8[s], k1[s]) for s in k1 if s != "labels"), "labels": bool(np.array_equal(k8["labels"], k1["labels"]))}
    res["c4_ratio_pppcsr_over_pcsr"] = {
        "sssp_unit": [round(x["sssp_ms"] / y["sssp_ms"], 3) for x, y in zip(a["unit"], b["unit"])],
        "sssp_weighted": [round(x["sssp_ms"] / y["sssp_ms"], 3) for x, y in zip(a["weighted"], b["weighted"])],
        "components": round(a["components"]["ms"] / b["components"]["ms"], 3), "target": 1.25, "bfs_pair_measured": 1.13}
    ok = res["c4_equal"]["distances"] and res["c4_equal"]["labels"] and all(
        u["levels_equal_distances"] for k in ("c2_pcsr", "c4_pppcsr", "c4_pcsr") for u in res[k]["unit"])
    res["checks_passed"] = bool(ok)
    path = os.path.join(args.out_dir, "paths_bench.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    if "passes_model_c2" in old:
        res["passes_model_c2"] = old["passes_model_c2"]
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")
    if not ok:
        sys.exit("paths_bench: a check failed (see checks in the record)")


if __name__ == "__main__":
    main()
