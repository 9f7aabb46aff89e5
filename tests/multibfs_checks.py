"""What the emulator tests and the GPU tests of multi_bfs share: one call checked exactly against tests/multibfs_model.py."""
import numpy as np

from consumers_model import global_edges, partition_states
from multibfs_model import model_multi_bfs


class One:
    """a PCSR with the calls the checks make on a PPPCSR"""

    def __init__(self, e):
        self.e = e

    def __getattr__(self, name):
        return getattr(self.e, name)

    def num_partitions(self): return 1
    def partition(self, k): return self.e
    def partition_start(self, k): return 0


def assert_equals_model(got, m, label):
    """got = (reached, far, ecc, harmonic[, levels]) of the package, m = the model's dict: everything exact, harmonic bit for bit"""
    reached, far, ecc, harm = got[:4]
    assert reached.dtype == np.uint64 and far.dtype == np.uint64 and ecc.dtype == np.uint32 and harm.dtype == np.float64
    assert [int(x) for x in reached] == m["reached"], f"{label}: reached"
    assert [int(x) for x in far] == m["far"], f"{label}: far"
    assert [int(x) for x in ecc] == m["ecc"], f"{label}: ecc"
    np.testing.assert_array_equal(harm.view(np.uint64), m["harmonic"].view(np.uint64), err_msg=f"{label}: harmonic, bit for bit")
    if len(got) > 4:
        np.testing.assert_array_equal(got[4], m["levels"], err_msg=f"{label}: levels")


def check(g, sources, label, bfs_rows=8):
    """g: a PPPCSR, or One(PCSR).  With and without levels against the model; the rows of up to bfs_rows sources (None: all)
    against g.bfs; nothing written (states and stats).  Returns (model, got with levels, counters of the call with levels)."""
    n, P = g.get_n(), g.num_partitions()
    states = partition_states(g)
    stats = [g.partition(k).stats() for k in range(P)]
    sources = np.asarray(sources, np.uint32)
    m = model_multi_bfs(*global_edges(states), n, sources)
    assert_equals_model(g.multi_bfs(sources), m, label + " (aggregates only)")
    got = g.multi_bfs(sources, levels=True)
    ctr = g.debug_multi_bfs_counters()
    assert got[4].shape == (len(sources), n)
    assert_equals_model(got, m, label)
    assert int(ctr[0]) == (len(sources) + 63) // 64, (label, ctr)
    rows = range(len(sources)) if bfs_rows is None else np.linspace(0, len(sources) - 1, min(bfs_rows, len(sources))).astype(int)
    for i in rows:
        np.testing.assert_array_equal(got[4][i], g.bfs(int(sources[i])), err_msg=f"{label}: row {i} against bfs({sources[i]})")
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(g)):
        assert f0 == f1
        np.testing.assert_array_equal(i0, i1, err_msg=label)
        np.testing.assert_array_equal(n0, n1, err_msg=label)
    assert stats == [g.partition(k).stats() for k in range(P)], label
    return m, got, ctr
