"""Device neighbour sampling, random walks and live degrees (ppcsr_sample_neighbours / ppcsr_random_walks / ppcsr_degrees) on

  c2    config #2's graph: RMAT scale 20, 10 M adds, bulk-built
  s18   the graph of the GPU tests: RMAT scale 18, 2 M adds (seed 31), bulk-built

with edge values 1 .. 1000, on one PCSR through the device forms (torch tensors).  Per graph, device ms (median of --reps runs
after a warm-up) and the rates: draws/s of sample_neighbours at fanout 10 and 25 over 2^16 and 2^20 seeds, steps/s of 2^16 and
2^20 walkers of length 80, uniform and weighted, and degrees beside one BFS.  8 partitions answer the 2^16-seed cases through the
host forms and must give the same arrays.

The yardstick is the composition a user had before these calls: per step, gather_neighbourhoods of the current vertices, the
copy to the host, and the same pick in numpy (the definition's own arithmetic, so the results must be equal, and are compared).
It is timed on the host clock over 2^16 seeds at fanout 10 and over the first --comp-steps steps of 2^16 walkers; the record
states both rates and their ratio to the device calls (wall clock of the host forms against wall clock: like against like).

The kernel split comes from a run of its own under rocprofv3 --kernel-trace --stats (one sample call and one walk per graph).
Writes profiles/sampling_bench.json (--out-dir: elsewhere)."""
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
from sampling_model import draw_x, mulhi  # noqa: E402

P = 8
GRAPHS = {"c2": (20, 10_000_000, 1), "s18": (18, 2_000_000, 31)}
LENGTH = 80
NO_VERTEX = 0xFFFFFFFF


def graph(st, which):
    scale, edges, seed = GRAPHS[which]
    s, d = st.rmat_edges(scale, edges, seed=seed)
    val = (st.uniform_ints(seed + 7, edges, 1000) + 1).astype(np.uint32)
    return 1 << scale, np.stack([s, d, val], 1).astype(np.uint32)


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
    ms = [call() for _ in range(reps)]
    return round(float(np.median(ms)), 3), [round(x, 3) for x in ms]


def pick_from_csr(rows, dests, vals, n, cur, seed, i, j, weighted):
    """the definition's pick from gathered rows (row r: the neighbourhood of cur[r]), in numpy"""
    U = np.uint64
    lens = np.diff(rows.astype(np.int64))
    rid = np.repeat(np.arange(len(cur)), lens)
    keep = (dests >= 0) & (dests.astype(np.int64) < n)
    d, v, rid = dests[keep].astype(np.uint32), vals[keep], rid[keep]
    cnt = np.bincount(rid, minlength=len(cur))
    r0 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(v.astype(U) if weighted else np.ones(len(d), U), dtype=U)]).astype(U)
    a, b = r0[:-1], r0[1:]
    ok = b > a
    W = np.where(ok, cum[b] - cum[a], U(1)).astype(U)
    e = np.searchsorted(cum, cum[a] + mulhi(draw_x(seed, i, j), W), side="right").astype(np.int64) - 1
    e = np.minimum(np.where(ok, e, 0), max(len(d) - 1, 0))
    return np.where(ok, d[e] if len(d) else 0, NO_VERTEX).astype(np.uint32)


def composition(g, n, seeds, fanout, walkers, steps, seed):
    """gather + D2H + numpy pick, per step; -> (sample array, seconds), (walk array, seconds)"""
    U = np.uint64
    t0 = time.perf_counter()
    rows, dests, vals = g.gather_neighbourhoods(seeds)
    k = len(seeds)
    lens = np.diff(rows.astype(np.int64))
    # fanout draws per row: every row repeated fanout times would copy the CSR; the pick is made per draw index instead
    out = np.empty((k, fanout), np.uint32)
    for j in range(fanout):
        out[:, j] = pick_from_csr(rows, dests, vals, n, seeds, seed, np.arange(k, dtype=U), np.full(k, j, U), False)
    t_sample = time.perf_counter() - t0
    del lens
    t0 = time.perf_counter()
    walk = np.empty((len(walkers), steps + 1), np.uint32)
    walk[:, 0] = walkers
    for t in range(steps):
        cur = walk[:, t]
        rows, dests, vals = g.gather_neighbourhoods(cur)  # (a vertex >= n, NO_VERTEX included, gathers an empty row)
        walk[:, t + 1] = pick_from_csr(rows, dests, vals, n, cur, seed, np.arange(len(cur), dtype=U), np.full(len(cur), t, U), False)
    t_walk = time.perf_counter() - t0
    return (out, t_sample), (walk, t_walk)


def measure(pkg, st, which, reps, comp_steps):
    import torch
    n, ops = graph(st, which)
    g = build(pkg, n, ops, 1)
    rng = np.random.default_rng(11)
    res = {"slots": int(g.geometry()[0]), "adds": len(ops)}
    verts = {16: rng.integers(0, n, 1 << 16).astype(np.uint32), 20: rng.integers(0, n, 1 << 20).astype(np.uint32)}
    dverts = {b: torch.from_numpy(v.view(np.int32)).cuda() for b, v in verts.items()}
    res["sample_neighbours"] = {}
    for b, q in verts.items():
        for fanout in (10, 25):
            out = torch.zeros((len(q), fanout), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for weighted in (False, True):
                ms, ms_all = timed(lambda: g.sample_neighbours_device(dverts[b].data_ptr(), len(q), fanout, out.data_ptr(), None, seed=3,
                                                                      weighted=weighted, with_ms=True), reps)
                res["sample_neighbours"][f"seeds_2^{b}_fanout_{fanout}_{'weighted' if weighted else 'uniform'}"] = {
                    "device_ms": ms, "device_ms_all": ms_all, "draws_per_s": round(len(q) * fanout / (ms * 1e-3))}
            del out
    res["random_walks"] = {}
    for b, q in verts.items():
        out = torch.zeros((len(q), LENGTH + 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for weighted in (False, True):
            ms, ms_all = timed(lambda: g.random_walks_device(dverts[b].data_ptr(), len(q), LENGTH, out.data_ptr(), seed=3, weighted=weighted,
                                                             with_ms=True), reps)
            w = out.cpu().numpy().view(np.uint32)
            live = int(np.count_nonzero(w[:, 1:] != NO_VERTEX))  # (RMAT: many vertices have no out-edge, and a walk that meets one ends)
            res["random_walks"][f"walkers_2^{b}_{'weighted' if weighted else 'uniform'}"] = {
                "device_ms": ms, "device_ms_all": ms_all, "steps_per_s": round(len(q) * LENGTH / (ms * 1e-3)),
                "steps_that_picked_a_vertex": live, "picked_steps_per_s": round(live / (ms * 1e-3)),
                "walks_that_end_early": int(np.count_nonzero(w[:, -1] == NO_VERTEX))}
        del out
    dms, _ = timed(lambda: g.degrees(with_ms=True)[1], reps)
    wms, _ = timed(lambda: g.degrees(weighted=True, with_ms=True)[1], reps)
    bms, _ = timed(lambda: g.bfs(int(np.argmax(g.degrees())), with_ms=True)[1], reps)
    res["degrees"] = {"deg_ms": dms, "wsum_ms": wms, "bfs_from_the_busiest_vertex_ms": bms, "deg_over_bfs": round(dms / bms, 3)}
    # the composition, wall clock against wall clock of the host forms
    q = verts[16]
    t0 = time.perf_counter()
    host_sample = g.sample_neighbours(q, 10, seed=3)
    t_sample = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_walk = g.random_walks(q, comp_steps, seed=3)
    t_walk = time.perf_counter() - t0
    (c_sample, ct_sample), (c_walk, ct_walk) = composition(g, n, q, 10, q, comp_steps, 3)
    res["composition"] = {
        "what": "gather_neighbourhoods of the current vertices, D2H, the same pick in numpy, per step; wall clock, 2^16 seeds / walkers",
        "sample_fanout_10": {"composition_s": round(ct_sample, 4), "sample_neighbours_host_form_s": round(t_sample, 4),
                             "draws_per_s_composition": round(len(q) * 10 / ct_sample), "draws_per_s_call": round(len(q) * 10 / t_sample),
                             "ratio": round(ct_sample / t_sample, 1), "equal": bool(np.array_equal(c_sample, host_sample))},
        "walks": {"steps": comp_steps, "composition_s": round(ct_walk, 4), "random_walks_host_form_s": round(t_walk, 4),
                  "steps_per_s_composition": round(len(q) * comp_steps / ct_walk), "steps_per_s_call": round(len(q) * comp_steps / t_walk),
                  "ratio": round(ct_walk / t_walk, 1), "equal": bool(np.array_equal(c_walk, host_walk))}}
    ok = res["composition"]["sample_fanout_10"]["equal"] and res["composition"]["walks"]["equal"]
    g.close()
    # 8 partitions: the same arrays
    pp = build(pkg, n, ops, P)
    (s8, sms), (w8, wms8) = pp.sample_neighbours(q, 10, seed=3, with_ms=True), pp.random_walks(q, comp_steps, seed=3, with_ms=True)
    res["pppcsr"] = {"partitions": P, "sample_2^16_fanout_10_device_ms": round(sms, 3), f"walks_2^16_length_{comp_steps}_device_ms": round(wms8, 3),
                     "equal_to_one_pcsr": bool(np.array_equal(s8, host_sample) and np.array_equal(w8, host_walk))}
    pp.close()
    return res, ok and res["pppcsr"]["equal_to_one_pcsr"]


def kernel_split(which):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--trace-pass", which]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        assert found, "rocprofv3 wrote no kernel_stats.csv"
        rows = list(csv.DictReader(open(found[0])))
    out = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0]
        if name.startswith(("ppcsr::k_sm_", "ppcsr::k_gather_mark", "void ppcsr::k_xs_", "ppcsr::k_xs_")):
            out[name] = {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 2)}
    return out


def trace_pass(which):
    """one PCSR: ONE sample call (2^20 seeds, fanout 10) and ONE walk (2^20 walkers, length 80), both uniform, and the degrees"""
    pkg, st = load_pkg(), load_streams()
    n, ops = graph(st, which)
    g = build(pkg, n, ops, 1)
    q = np.random.default_rng(11).integers(0, n, 1 << 20).astype(np.uint32)
    a = g.sample_neighbours(q, 10, seed=3)
    w = g.random_walks(q, LENGTH, seed=3)
    d = g.degrees()
    print(json.dumps({"trace_pass": which, "picked": int(np.count_nonzero(a != NO_VERTEX)), "alive": int(np.count_nonzero(w[:, -1] != NO_VERTEX)),
                      "edges": int(d.sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--comp-steps", type=int, default=5)
    ap.add_argument("--no-kernel-split", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-pass", choices=list(GRAPHS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_pass:
        return trace_pass(args.trace_pass)
    pkg, st = load_pkg(), load_streams()
    res = {"graphs": {k: f"RMAT scale {v[0]}, {v[1]} adds (seed {v[2]}), values 1..1000, bulk-built" for k, v in GRAPHS.items()},
           "reps": args.reps, "walk_length": LENGTH,
           "timing": "device_ms of the calls (device events on the engine's stream); the composition and the host forms beside it: host wall clock"}
    ok = True
    for which in GRAPHS:
        print(which, file=sys.stderr, flush=True)
        res[which], good = measure(pkg, st, which, args.reps, args.comp_steps)
        ok = ok and good
    if not args.no_kernel_split:
        res["kernel_split_us"] = {"what": "rocprofv3 --kernel-trace --stats over one sample call (2^20 seeds, fanout 10), one walk (2^20 walkers, "
                                          "length 80) and one degrees call, uniform, one PCSR"}
        for which in GRAPHS:
            res["kernel_split_us"][which] = kernel_split(which)
    res["checks_passed"] = bool(ok)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out_dir, "sampling_bench.json"), "w") as f:
        f.write(line + "\n")
    assert ok, "sampling_bench: a check failed (the composition or the 8 partitions gave other arrays: see the record)"


if __name__ == "__main__":
    main()
