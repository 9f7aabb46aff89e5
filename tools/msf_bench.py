"""Device minimum spanning forest (ppcsr_msf / pppcsr_msf) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the other tools: RMAT scale 18, 2 M adds (seed 31), bulk-built

with edge values uniform in [1, 2^20] (a hash of the pair, so that the repeats of a pair carry one value) and with all values 1,
each on one PCSR and on 8 partitions on one GPU.  Per graph, values and form: device ms of the whole call (median of --reps runs
after a warm-up), the counters of ppcsr_debug_msf_counters (rounds, streaming passes, pointer-jump launches, hooks, host reads),
GB/s over the slots the passes streamed (12 bytes a slot), and the hooks per round of the synchronous numpy replica of the
schedule (tests/msf_model.model_rounds), which the device's round count and first-round hooks must equal.

Yardsticks (no thresholds):
  components    the ms of ppcsr_components on the same graph, and the ratio msf / components
  bfs           the ms of one ppcsr_bfs from the vertex of the largest out-degree
  composition   one PCSR: what a user could do before this call — gather_neighbourhoods_device gives the CSR with values, a D2H
                copy takes it to the host, every unordered pair is collapsed to its lightest stored value, and
                scipy.sparse.csgraph.minimum_spanning_tree runs on that.  Wall time of the whole composition; its weight must
                equal *weight exactly (asserted: sums below 2^53 are exact in fp64) and its edge count *count.

Writes profiles/msf_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE msf call per graph (one PCSR, values in [1, 2^20]) under rocprofv3 --kernel-trace --stats, in a run of
                 its own, and writes profiles/msf_kernel_stats.csv: the calls of a kernel are its launches over all rounds."""
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
from msf_model import model_rounds  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
VALUES = ("uniform20", "ones")
COUNTERS = ("rounds", "streaming_passes", "jump_launches", "max_jump_launches_in_a_round", "first_round_hooks", "forest_edges",
            "components", "host_reads")


def graph(st, which, values):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    ops = st.adds(s, d)
    if values == "uniform20":
        key = s.astype(np.uint64) * np.uint64(1 << scale) + d.astype(np.uint64)
        ops[:, 2] = (st.splitmix64(key) % np.uint64(1 << 20)).astype(np.uint32) + 1
    return 1 << scale, ops


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


def measure(pkg, n, ops, parts, reps, shape):
    g = build(pkg, n, ops, parts)
    slots = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))

    def msf():
        edges, weight, labels, ms = g.msf(with_ms=True)
        return (edges, weight, labels), ms

    (edges, weight, labels), ms, ms_all = timed(msf, reps)
    c = dict(zip(COUNTERS, (int(x) for x in g.debug_msf_counters())))
    if "hooks" not in shape:  # (the same graph for both forms: replayed on the host once)
        shape["hooks"], shape["depth"] = model_rounds(ops[:, 0], ops[:, 1], ops[:, 2], n)
    hooks = shape["hooks"]
    top = int(np.bincount(ops[:, 0], minlength=n).argmax())
    cc, cc_ms, _ = timed(lambda: g.components(with_ms=True), reps)
    _, bfs_ms, _ = timed(lambda: (None, g.bfs(top, with_ms=True)[1]), reps)
    streamed = c["streaming_passes"] * slots * 12
    res = {"partitions": parts, "slots": slots, "forest_edges": int(len(edges)), "weight": int(weight), "components": int(n - len(edges)),
           "ms": ms, "ms_all": ms_all, "counters": c, "GBps_over_streamed_slots": round(streamed / (ms * 1e-3) / 1e9, 1),
           "replica_hooks_per_round": hooks, "replica_deepest_chain_per_round": shape["depth"],
           "rounds_are_the_replicas": bool(c["rounds"] == len(hooks) + 1 and c["first_round_hooks"] == (hooks[0] if hooks else 0)
                                            and c["forest_edges"] == sum(hooks)),
           "labels_are_components": bool(np.array_equal(labels, cc)),
           "components_ms": cc_ms, "bfs_ms": bfs_ms, "bfs_start": top,
           "msf_over_components": round(ms / cc_ms, 2), "msf_over_bfs": round(ms / bfs_ms, 2)}
    return res, g, (edges, weight, labels)


def composition(g, n, reps):
    """the forest's weight from the other public calls: gather with values on the device -> D2H -> lightest value per unordered
    pair -> scipy minimum_spanning_tree"""
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    dev = "cuda"
    verts = torch.arange(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cap = g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), 0, 0, 0)
    dests = torch.empty(cap, dtype=torch.int32, device=dev)
    vals = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def once():
        t0 = time.perf_counter()
        g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), dests.data_ptr(), vals.data_ptr(), cap)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        indptr, indices, values = rows.cpu().numpy(), dests.cpu().numpy().astype(np.int64), vals.cpu().numpy().view(np.uint32).astype(np.int64)
        t2 = time.perf_counter()
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        keep = (indices >= 0) & (indices < n) & (indices != src)  # (destinations >= n are no vertices; self-loops play no part)
        lo, hi, w = np.minimum(src, indices)[keep], np.maximum(src, indices)[keep], values[keep]
        order = np.lexsort((w, hi, lo))
        lo, hi, w = lo[order], hi[order], w[order]
        first = np.ones(len(lo), bool)
        first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])  # the lightest value of every unordered pair
        tree = minimum_spanning_tree(coo_matrix((w[first].astype(np.float64), (lo[first], hi[first])), shape=(n, n)).tocsr())
        weight, count = int(round(float(tree.sum()))), int(tree.nnz)
        t3 = time.perf_counter()
        return (weight, count), [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]

    once()  # warm-up
    runs = [once() for _ in range(reps)]
    med = [round(float(np.median([r[1][k] for r in runs])), 3) for k in range(4)]
    return runs[0][0], {"ms": med[0], "ms_all": [round(r[1][0], 3) for r in runs], "gather_ms": med[1], "d2h_ms": med[2], "scipy_ms": med[3],
                        "timing": "host wall clock around the whole composition"}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "msf_kernel_stats.csv")
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
            if not (name.startswith("ppcsr::k_msf") or name.startswith("ppcsr::k_cc_init") or "radix_sort" in name):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR, values in [1, 2^20]: ONE msf call"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass, "uniform20")
    g = build(pkg, n, ops, 1)
    edges, weight, labels = g.msf()
    print(json.dumps({"trace_pass": args.trace_pass, "forest_edges": int(len(edges)), "counters": [int(x) for x in g.debug_msf_counters()]}))


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
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), bulk-built" for k, v in GRAPHS.items()},
           "values": {"uniform20": "a hash of the pair, uniform in [1, 2^20]", "ones": "all 1"}, "reps": args.reps,
           "timing": "device events on the engine's stream (device_ms of the calls: the whole call, host reads included); the composition: host wall clock"}
    ok = True
    for which in GRAPHS:
        for values in VALUES:
            n, ops = graph(st, which, values)
            shape = {}
            print(f"{which} {values} x1", file=sys.stderr, flush=True)
            one, g, (e1, w1, l1) = measure(pkg, n, ops, 1, args.reps, shape)
            (cw, cc), comp = composition(g, n, 2)
            comp["ratio_composition_over_msf"] = round(comp["ms"] / one["ms"], 1)
            comp["same_weight_and_count"] = bool(cw == w1 and cc == len(e1))
            one["composition"] = comp
            ok = ok and comp["same_weight_and_count"]
            g.close()
            print(f"{which} {values} x{P}", file=sys.stderr, flush=True)
            many, g, (e8, w8, l8) = measure(pkg, n, ops, P, args.reps, shape)
            g.close()
            many["equal_to_one_pcsr"] = bool(np.array_equal(e1, e8) and w1 == w8 and np.array_equal(l1, l8))
            many["ratio_over_one_pcsr"] = round(many["ms"] / one["ms"], 3)
            ok = ok and many["equal_to_one_pcsr"] and one["rounds_are_the_replicas"] and many["rounds_are_the_replicas"]
            ok = ok and one["labels_are_components"] and many["labels_are_components"]
            res[f"{which}_{values}_pcsr"], res[f"{which}_{values}_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "msf_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "msf_bench: a check failed (equal outputs, the replica's rounds, or the composition's weight: see the record)"


if __name__ == "__main__":
    main()
