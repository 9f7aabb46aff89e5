"""Device strongly connected components (ppcsr_scc / pppcsr_scc) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the other tools: RMAT scale 18, 2 M adds (seed 31), bulk-built

each on one PCSR and on 8 partitions on one GPU.  Per graph and form: device ms of the whole call (median of --reps runs after a
warm-up), the counters of ppcsr_debug_scc_counters (vertices per phase, trim sweeps, colouring rounds, streaming passes, host
reads), and beside them the pass counts of the synchronous numpy replica of the schedule (tests/scc_model.replica, from the
device's own pivot): a device pass reads the marks as they are, so no loop should need more passes than the replica's, whose
counts include the last pass of every loop, the one that finds nothing.  The replica must reproduce the device's labels.

Yardsticks (no thresholds):
  components    the ms of ppcsr_components on the same graph
  bfs           the ms of one ppcsr_bfs from the vertex of the largest out-degree
  composition   one PCSR: what a user could do before this call — gather_neighbourhoods_device gives the CSR, a D2H copy
                takes it to the host, scipy.sparse.csgraph.connected_components(connection="strong") labels it and a numpy
                pass renames every component to its smallest id.  Wall time of the whole composition; it must give identical
                labels and the dedicated call must be faster (asserted; both times and the ratio are recorded).

Writes profiles/scc_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE scc call per graph (one PCSR) under rocprofv3 --kernel-trace --stats, in a run of its own, and
                 writes profiles/scc_kernel_stats.csv: the calls of a kernel are the passes of its phase."""
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
from scc_model import replica  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
COUNTERS = ("trimmed", "trim_sweeps", "pivot", "pivot_scc", "colouring_rounds", "coloured", "streaming_passes", "host_reads")


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


def measure(pkg, n, ops, parts, reps, shape):
    g = build(pkg, n, ops, parts)
    slots = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))

    def scc():
        labels, count, ms = g.scc(with_ms=True)
        return (labels, count), ms

    (labels, count), ms, ms_all = timed(scc, reps)
    c = dict(zip(COUNTERS, (int(x) for x in g.debug_scc_counters())))
    if "replica" not in shape:  # (the same graph for both forms: replayed on the host once, from the device's pivot)
        want, passes = replica(ops[:, 0], ops[:, 1], n, pivot=c["pivot"])
        shape["replica"], shape["labels"] = passes, want
    rep = shape["replica"]
    top = int(np.bincount(ops[:, 0], minlength=n).argmax())
    _, cc_ms, _ = timed(lambda: (None, g.components(with_ms=True)[1]), reps)
    _, bfs_ms, _ = timed(lambda: (None, g.bfs(top, with_ms=True)[1]), reps)
    sizes = np.bincount(labels, minlength=n)
    replica_passes = rep["trim_sweeps"] + max(rep["fw_passes"], rep["bw_passes"]) + rep["prop_passes"] + rep["reach_passes"]
    res = {"partitions": parts, "slots": slots, "sccs": int(count), "largest_scc": int(sizes.max()), "nontrivial_sccs": int((sizes > 1).sum()),
           "ms": ms, "ms_all": ms_all, "counters": c, "us_per_pass": round(ms * 1e3 / max(c["streaming_passes"], 1), 2),
           "replica": rep, "replica_passes_both_reaches_in_one": replica_passes,
           "device_passes_within_replica": bool(c["streaming_passes"] <= replica_passes),
           "labels_are_the_replicas": bool(np.array_equal(labels, shape["labels"])),
           "components_ms": cc_ms, "bfs_ms": bfs_ms, "bfs_start": top,
           "scc_over_components": round(ms / cc_ms, 2), "scc_over_bfs": round(ms / bfs_ms, 2)}
    return res, g, labels


def composition(g, n, reps):
    """SCC labels from the other public calls: gather on the device -> D2H -> scipy strong components -> smallest ids"""
    import torch
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    dev = "cuda"
    verts = torch.arange(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cap = g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), 0, 0, 0)
    dests = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def once():
        t0 = time.perf_counter()
        g.gather_neighbourhoods_device(verts.data_ptr(), n, rows.data_ptr(), dests.data_ptr(), 0, cap)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        indptr, indices = rows.cpu().numpy(), dests.cpu().numpy()
        t2 = time.perf_counter()
        keep = (indices >= 0) & (indices < n)  # (destinations >= n are no vertices)
        if not keep.all():
            src = np.repeat(np.arange(n), np.diff(indptr))[keep]
            indptr, indices = np.searchsorted(src, np.arange(n + 1)), indices[keep]
        m = csr_matrix((np.ones(len(indices), np.int8), indices, indptr), shape=(n, n))
        ncomp, lab = connected_components(m, directed=True, connection="strong")
        smallest = np.full(ncomp, n, np.int64)
        np.minimum.at(smallest, lab, np.arange(n))
        out = smallest[lab].astype(np.uint32)
        t3 = time.perf_counter()
        return out, [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]

    once()  # warm-up
    runs = [once() for _ in range(reps)]
    med = [round(float(np.median([r[1][k] for r in runs])), 3) for k in range(4)]
    return runs[0][0], {"ms": med[0], "ms_all": [round(r[1][0], 3) for r in runs], "gather_ms": med[1], "d2h_ms": med[2], "scipy_ms": med[3],
                        "timing": "host wall clock around the whole composition"}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "scc_kernel_stats.csv")
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
            if not name.startswith("ppcsr::k_scc"):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE scc call"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    labels, count = g.scc()
    print(json.dumps({"trace_pass": args.trace_pass, "sccs": int(count), "counters": [int(x) for x in g.debug_scc_counters()]}))


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
           "timing": "device events on the engine's stream (device_ms of the calls: the whole call, host reads included); the composition: host wall clock"}
    ok = True
    for which in GRAPHS:
        n, ops = graph(st, which)
        shape = {}
        print(f"{which} x1", file=sys.stderr, flush=True)
        one, g, labels1 = measure(pkg, n, ops, 1, args.reps, shape)
        clabels, comp = composition(g, n, 3)
        comp["ratio_composition_over_scc"] = round(comp["ms"] / one["ms"], 1)
        comp["same_labels"] = bool(np.array_equal(clabels, labels1))
        comp["dedicated_call_is_faster"] = bool(one["ms"] < comp["ms"])
        one["composition"] = comp
        ok = ok and comp["same_labels"] and comp["dedicated_call_is_faster"]
        g.close()
        print(f"{which} x{P}", file=sys.stderr, flush=True)
        many, g, labels8 = measure(pkg, n, ops, P, args.reps, shape)
        g.close()
        many["equal_to_one_pcsr"] = bool(np.array_equal(labels1, labels8) and many["sccs"] == one["sccs"])
        many["ratio_over_one_pcsr"] = round(many["ms"] / one["ms"], 3)
        ok = ok and many["equal_to_one_pcsr"] and one["labels_are_the_replicas"]
        res[which + "_pcsr"], res[which + "_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "scc_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "scc_bench: a check failed (equal labels, or the dedicated call against the composition: see the record)"


if __name__ == "__main__":
    main()
