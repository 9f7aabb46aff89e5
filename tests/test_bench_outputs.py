"""bench.py --dump-outputs and the plain run: the dump writer on the CPU (bounded, exact, the same sample every run), and on
the GPU a plain run at a small size whose dump is the oracle's state after the core + the last timed batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, _load

BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    return _load("ppcsr_bench", BENCH)


def test_write_outputs_is_exact_bounded_and_fixed(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(7)
    items = rng.integers(0, 1 << 32, size=(3_000_000, 3), dtype=np.uint64).astype(np.uint32)
    items[::5] = 0xFFFFFFFF
    nodes = rng.integers(0, 1 << 32, size=(700_000, 3), dtype=np.uint64).astype(np.uint32)
    states = [(items[:2_000_000], nodes[:300_000]), (items[2_000_000:], nodes[300_000:])]
    geoms = [(2_000_000, 32, 5), (1_000_000, 32, 4)]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    files = bench.write_outputs(a, states, geoms)
    assert bench.write_outputs(b, states, geoms) == files
    assert sum(os.path.getsize(os.path.join(a, f)) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float64 and np.array_equal(x, y), f
    np.testing.assert_array_equal(np.load(os.path.join(a, "geometry.npy")), np.array(geoms, np.float64))
    for name, full in (("edges", items), ("nodes", nodes)):
        rows = np.load(os.path.join(a, name + "_rows.npy")).astype(np.int64)
        assert len(rows) == bench.DUMP_ROWS[name] and (np.diff(rows) > 0).all()
        np.testing.assert_array_equal(np.load(os.path.join(a, name + ".npy")), full[rows].astype(np.float64))
    # below the budget every row is written, in order, without a row file
    small = bench.write_outputs(str(tmp_path / "c"), [(items[:1000], nodes[:100])], [geoms[0]], world=2, rank=1)
    assert sorted(small) == ["edges_rank1.npy", "geometry_rank1.npy", "nodes_rank1.npy"]
    np.testing.assert_array_equal(np.load(str(tmp_path / "c" / "edges_rank1.npy")), items[:1000].astype(np.float64))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """a plain run (no --full) on a small config #2 graph: the result line's headline fields, no parity / baseline / roofline
    work, and the dumped state equal to the oracle's after the core + the batch of the last timed step"""
    from helpers import load_streams
    from oracle_lib import Oracle
    scale, core_edges, batch, steps, warmup = 14, 100_000, 20_000, 3, 1
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--scale", str(scale),
           "--core-edges", str(core_edges), "--batch", str(batch), "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["metric"] == "edge-updates/sec" and out["unit"] == "edge-updates/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u32" and out["steps"] == steps and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(batch / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert "parity_checked" not in out and out["roofline"] is None and out["cpu_baseline"] is None and out["end_to_end"] is None
    st = load_streams()
    wl = _bench().Workload(st, 2, 1 << scale, scale, core_edges, batch, False)
    nb = min(4, warmup + steps)  # bench.py's --distinct-batches default
    o = Oracle(1 << scale)
    o.apply(np.concatenate([wl.core(0, core_edges), wl.updates((warmup + steps - 1) % nb, 0, batch)]))
    items, nodes = o.state()
    np.testing.assert_array_equal(np.load(os.path.join(out_dir, "geometry.npy")), np.array([o.geometry()], np.float64))
    np.testing.assert_array_equal(np.load(os.path.join(out_dir, "edges.npy")), items.astype(np.float64))
    np.testing.assert_array_equal(np.load(os.path.join(out_dir, "nodes.npy")), nodes.astype(np.float64))
    o.close()
