"""Batched reads on config #2's graph (RMAT scale 20, 10 M-edge core, streams.py): prints one JSON line.

  lookups      ppcsr_lookup_edges_device, 2^22 pairs (half of them edges): lookups/s
  gather       ppcsr_gather_neighbourhoods_device, 2^20 random vertices: edges/s and GB/s (12 B per slot of the rows' ranges
               read twice — count and write pass — plus 8 B per edge written)
  hub          the same for ONE bulk-built vertex of 2^22 edges: GB/s at 12 B per slot of its range (the issue's yardstick)
  edge_exists  the single call in a loop, for comparison: us per call

Timed: wall clock around the synchronous device calls (torch tensors in HBM, no host copies), best of --reps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import load_pkg, load_streams  # noqa: E402


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lookups", type=int, default=1 << 22)
    ap.add_argument("--gather", type=int, default=1 << 20)
    ap.add_argument("--hub", type=int, default=1 << 22)
    ap.add_argument("--single", type=int, default=2000)
    args = ap.parse_args()
    import torch
    pkg, st = load_pkg(), load_streams()
    n = 1 << 20
    s, d = st.rmat_edges(20, 10_000_000, seed=1)
    e = pkg.PCSR(n)
    e.apply(st.adds(s, d))
    items, nodes = e.state()
    live = np.nonzero((items[:, 2] != 0) & (items[:, 1] != 0xFFFFFFFF) & (items[:, 2] != 0xFFFFFFFF))[0]
    rng = np.random.default_rng(1)
    m = args.lookups
    qs = rng.integers(0, n, m).astype(np.uint32)
    qd = rng.integers(0, n, m).astype(np.uint32)
    pick = live[rng.integers(0, len(live), m // 2)]
    qs[:m // 2], qd[:m // 2] = items[pick, 0], items[pick, 1]
    perm = rng.permutation(m)
    qs, qd = qs[perm], qd[perm]
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()  # noqa: E731
    ts, td, tv = dev(qs), dev(qd), torch.empty(m, dtype=torch.int32, device="cuda")
    look = lambda: e.lookup_edges_device(ts.data_ptr(), td.data_ptr(), m, tv.data_ptr())  # noqa: E731
    look()
    t_look = best(look, args.reps)
    found = float((tv.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).mean())

    def gather_rate(eng, verts):
        tq = dev(verts)
        trow = torch.empty(len(verts) + 1, dtype=torch.int64, device="cuda")
        tot = eng.gather_neighbourhoods_device(tq.data_ptr(), len(verts), trow.data_ptr(), 0, 0, 0)
        tdst = torch.empty(max(tot, 1), dtype=torch.int32, device="cuda")
        tval = torch.empty(max(tot, 1), dtype=torch.int32, device="cuda")
        fn = lambda: eng.gather_neighbourhoods_device(tq.data_ptr(), len(verts), trow.data_ptr(), tdst.data_ptr(), tval.data_ptr(), tot)  # noqa: E731
        fn()
        t = best(fn, args.reps)
        it, nd = eng.state()
        v = verts[verts < len(nd)].astype(np.int64)
        slots = int(np.maximum(nd[v, 1].astype(np.int64) - nd[v, 0].astype(np.int64) - 1, 0).sum())
        return t, tot, slots

    verts = rng.integers(0, n, args.gather).astype(np.uint32)
    t_g, tot_g, slots_g = gather_rate(e, verts)
    # hub: one vertex with args.hub edges among 2^16 vertices, bulk-built
    hn, hub = 1 << 16, 7
    hd = rng.choice(1 << 30, args.hub + 4096, replace=False).astype(np.uint32)[:args.hub]
    adds = np.stack([np.full(args.hub, hub, np.uint32), hd, np.ones(args.hub, np.uint32)], 1)
    h = pkg.PCSR(hn)
    h.bulk_build(adds)
    t_h, tot_h, slots_h = gather_rate(h, np.array([hub], np.uint32))
    # the single call, for comparison
    k = args.single
    t0 = time.perf_counter()
    for j in range(k):
        e.edge_exists(int(qs[j]), int(qd[j]))
    t_single = (time.perf_counter() - t0) / k
    out = {
        "graph": "RMAT scale 20, 10 M-edge core (config #2)", "N": int(e.geometry()[0]),
        "lookups": m, "lookup_found_frac": round(found, 3), "lookup_ms": round(t_look * 1e3, 3), "lookups_per_s": round(m / t_look),
        "gather_vertices": len(verts), "gather_edges": tot_g, "gather_slots": slots_g, "gather_ms": round(t_g * 1e3, 3),
        "gather_edges_per_s": round(tot_g / t_g), "gather_GBps": round((24 * slots_g + 8 * tot_g) / t_g / 1e9, 1),
        "hub_edges": tot_h, "hub_slots": slots_h, "hub_ms": round(t_h * 1e3, 3), "hub_edges_per_s": round(tot_h / t_h),
        "hub_GBps_12B_per_slot": round(12 * slots_h / t_h / 1e9, 1),
        "edge_exists_single_us": round(t_single * 1e6, 2), "edge_exists_single_per_s": round(1 / t_single),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
