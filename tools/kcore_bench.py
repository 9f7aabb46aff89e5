"""Device core numbers (ppcsr_kcore / pppcsr_kcore) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

each on one PCSR and on 8 partitions on one GPU.  Per graph and form: device ms (median of --reps runs after a warm-up), kmax,
upper edges per second, and levels and sub-rounds.  The last two are the MODEL's: a synchronous peel of the same graph on the
host (tests/kcore_model.hardness), which must reproduce the device's core numbers; the call itself exports no counts — its
launches are counted by --kernel-stats (k_kc_min runs once per level and once more to find none left, k_kc_peel once per
sub-round).  The device ms is that of the whole call: it includes the host round trips of the peel and, between the scan and
the fill pass, one host read and the allocation of the adjacency lists.

Yardsticks:
  components    the ms of ppcsr_components on the same graph (no threshold)
  scan          the ms of ppcsr_bench_scan_all on the same array(s), one pass over the slots (no threshold)
  composition   s18, one PCSR: what a user could do before this call — gather_neighbourhoods_device gives the CSR, torch keeps
                the upper part, symmetrises it and peels in sub-rounds with tensor ops (about ten launches per sub-round).  Timed
                with device events around the whole composition; it must give identical core numbers and the dedicated call must
                be faster (asserted; both times and the ratio are recorded).

Writes profiles/kcore_bench.json (--out-dir: elsewhere).
--kernel-stats   reruns ONE kcore call per graph (one PCSR) under rocprofv3 --kernel-trace --stats, in a run of its own, and
                 writes profiles/kcore_kernel_stats.csv."""
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
from kcore_model import hardness  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}


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


def stored_pairs(n, ops):
    """(src, dst) of the distinct pairs a bulk build of `ops` stores"""
    key = np.unique(ops[:, 0].astype(np.int64) * n + ops[:, 1].astype(np.int64))
    return key // n, key % n


def measure(pkg, n, ops, parts, reps, shape):
    g = build(pkg, n, ops, parts)
    slots = int(g.geometry()[0]) if parts == 1 else int(sum(g.partition(k).geometry()[0] for k in range(parts)))

    def kcore():
        core, kmax, ms = g.kcore(with_ms=True)
        return (core, kmax), ms

    (core, kmax), ms, ms_all = timed(kcore, reps)
    if "h" not in shape:  # (the same graph for both forms: peeled on the host once)
        shape["h"] = hardness(*stored_pairs(n, ops), n, core)
    h = shape["h"]
    _, cc_ms, _ = timed(lambda: (None, g.components(with_ms=True)[1]), reps)
    scan = [g.bench_scan_all()[0] for _ in range(reps + 1)][1:] if parts == 1 else \
        [sum(g.partition(k).bench_scan_all()[0] for k in range(parts)) for _ in range(reps + 1)][1:]
    res = {"partitions": parts, "slots": slots, "upper_edges": h["edges"], "kmax": int(kmax), "kmax_is_the_models": bool(kmax == h["kmax"]),
           "levels": h["levels"], "subrounds": h["subrounds"], "max_subrounds_in_a_level": h["max_subrounds"], "widest_frontier": h["widest"],
           "largest_degree": h["maxdeg"], "ms": ms, "ms_all": ms_all, "upper_edges_per_s": round(h["edges"] / (ms * 1e-3)),
           "us_per_subround": round(ms * 1e3 / h["subrounds"], 2), "components_ms": cc_ms, "scan_all_ms": round(float(np.median(scan)), 3)}
    res["kcore_over_components"] = round(ms / cc_ms, 2)
    res["kcore_over_scan"] = round(ms / res["scan_all_ms"], 2)
    return res, g, core


def composition(g, n, reps):
    """core numbers of the upper orientation from the other public device calls: gather -> symmetric CSR in torch -> sub-round
    peeling with tensor ops"""
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
        out_deg = rows[1:] - rows[:-1]
        src = torch.repeat_interleave(torch.arange(n, device=dev), out_deg)
        dst = dests.to(torch.int64)
        up = (src < dst) & (dst < n)
        a, b = src[up], dst[up]
        u, v = torch.cat([a, b]), torch.cat([b, a])
        v = v[torch.argsort(u)]
        deg = torch.bincount(u, minlength=n)
        rowp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rowp[1:] = torch.cumsum(deg, 0)
        core = torch.full((n,), -1, dtype=torch.int64, device=dev)
        t1.record()
        levels = subrounds = 0
        while True:
            left = core < 0
            if not bool(left.any()):
                break
            k = deg[left].min()
            levels += 1
            front = torch.nonzero(left & (deg <= k)).squeeze(1)
            while front.numel():
                subrounds += 1
                core[front] = k
                lens = rowp[front + 1] - rowp[front]
                idx = torch.repeat_interleave(rowp[front] - torch.cumsum(lens, 0) + lens, lens)
                idx += torch.arange(idx.numel(), device=dev)
                deg -= torch.bincount(v[idx], minlength=n)
                front = torch.nonzero((core < 0) & (deg <= k)).squeeze(1)
        t2.record()
        torch.cuda.synchronize()
        return (core.cpu().numpy().astype(np.uint32), levels, subrounds), (t0.elapsed_time(t2), t0.elapsed_time(t1), t1.elapsed_time(t2))

    once()  # warm-up
    runs = [once() for _ in range(reps)]
    core, levels, subrounds = runs[0][0]
    med = [round(float(np.median([r[1][k] for r in runs])), 3) for k in range(3)]
    return core, {"levels": levels, "subrounds": subrounds, "ms": med[0], "ms_all": [round(r[1][0], 3) for r in runs], "export_ms": med[1],
                  "peel_ms": med[2]}


def kernel_stats(args):
    out = os.path.join(args.out_dir, "kcore_kernel_stats.csv")
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
            if not name.startswith("ppcsr::k_kc"):
                continue
            lines.append(f"{which},{name},{r['Calls']},{float(r['TotalDurationNs']) / 1e3:.2f},{float(r['AverageNs']) / 1e3:.2f},"
                         f"{float(r['MinNs']) / 1e3:.2f},{float(r['MaxNs']) / 1e3:.2f}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out).read())


def trace_pass(args):
    """one PCSR: ONE kcore call"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, args.trace_pass)
    g = build(pkg, n, ops, 1)
    core, kmax = g.kcore()
    print(json.dumps({"trace_pass": args.trace_pass, "kmax": int(kmax), "vertices_with_a_core": int(np.count_nonzero(core))}))


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
        shape = {}
        print(f"{which} x1", file=sys.stderr, flush=True)
        one, g, core1 = measure(pkg, n, ops, 1, args.reps, shape)
        if which == "s18":
            ccore, comp = composition(g, n, max(3, args.reps // 2))
            comp["ratio_composition_over_kcore"] = round(comp["ms"] / one["ms"], 2)
            comp["same_core_numbers"] = bool(np.array_equal(ccore, core1))
            comp["same_levels_and_subrounds"] = bool(comp["levels"] == one["levels"] and comp["subrounds"] == one["subrounds"])
            comp["dedicated_call_is_faster"] = bool(one["ms"] < comp["ms"])
            one["composition"] = comp
            ok = ok and comp["same_core_numbers"] and comp["dedicated_call_is_faster"]
        g.close()
        print(f"{which} x{P}", file=sys.stderr, flush=True)
        many, g, core8 = measure(pkg, n, ops, P, args.reps, shape)
        g.close()
        many["equal_to_one_pcsr"] = bool(np.array_equal(core1, core8) and many["kmax"] == one["kmax"])
        many["ratio_over_one_pcsr"] = round(many["ms"] / one["ms"], 3)
        ok = ok and many["equal_to_one_pcsr"] and one["kmax_is_the_models"]
        res[which + "_pcsr"], res[which + "_pppcsr"] = one, many
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "kcore_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "kcore_bench: a check failed (equal results, or the dedicated call against the composition: see the record)"


if __name__ == "__main__":
    main()
