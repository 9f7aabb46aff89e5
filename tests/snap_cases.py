"""Scenario scripts of the snapshot / restore tests (tests/test_sim_snapshot.py on the emulator, tests/test_gpu_snapshot.py on the
device; the driver and the full-copy model are tests/snap_checks.py).  Pure data: nothing here touches an engine.

A scenario is a write path W of the engine, given as a list of steps that the driver carries out between a snapshot and the check:
    ("opt", key, value)            ppcsr_set_option
    ("add_edge", s, d, v)          single-op entry points
    ("remove_edge", s, d)
    ("apply", ops)                 one batch
    ("rollbacks", [ops, ...])      batches applied one after the other until stats.rollbacks has grown (all of them at most)
    ("rebalance", w, upper)        bench_rebalance(w) on [0, w) or, upper = 1, on [N - w, N)
    ("block_rebalance", ws, wl)    option test_block_rebalance on [ws, ws + wl)
    ("bench_resize",)              the array doubled and halved back
    ("add_node",)
    ("bulk_build", ops)
    ("set_nn", recs)               pppcsr_set_num_neighbors_device (rows of (vertex, num_neighbors, *))
Every builder takes a Ctx (the state recorded at the snapshot) and returns the steps.  `path` is the way the table of the
scenarios says the restore must take: "step" (incremental, dirty tags) or "full" (whole-array copy)."""
import numpy as np

FRESH_LO = 1 << 20  # the graphs are loaded with dests below this: anything from here on is a new edge (or a missing one)

# name -> (vertices, edges loaded).  logN (the leaf size) is 8 for N < 2^8, 16 for N < 2^16 and 32 from there on: tiny (shrunk
# to N = 64 by deletes: snap_checks.build_graph), mid and big hold one of each; fewer than 64 leaves (tiny) is the partial-wave tag
# mask of k_snap_sync_leaves.  g256 / g257 / g513: N = 2^13, 512 leaves, and 1, 2 and 3 trips of 256 vertices through
# k_snap_sync_nodes at snap_grid = 1.
GRAPHS = {"tiny": (2, 13), "mid": (300, 3500), "big": (4096, 40000), "g256": (256, 3500), "g257": (257, 3500), "g513": (513, 3500)}


def graph_ops(name, streams):
    n, m = GRAPHS[name]
    if name == "tiny":
        return np.array([[i % 2, 5 + 7 * i, 1 + i] for i in range(m)], np.uint32)
    ops = streams.random_stream(n, m, seed=5 + n)
    ops[:, 1] = streams.uniform_ints(77 + n, m, FRESH_LO)
    ops[:, 2] = 1 + streams.uniform_ints(78 + n, m, 1000)
    return ops.astype(np.uint32)


class Ctx:
    """what a builder may look at: the state recorded at the snapshot"""

    def __init__(self, n, geom, existing, seed, rollback_k):
        self.n, self.N, self.logN = n, geom[0], geom[1]
        self.ex = existing  # live edges (src, dest, value) in array order
        self.rng = np.random.default_rng(seed)
        self.rollback_k = rollback_k

    def pick(self, k):
        k = min(k, len(self.ex))
        return self.ex[self.rng.choice(len(self.ex), k, replace=False)].copy() if k else np.zeros((0, 3), np.uint32)

    def fresh(self, src):
        src = np.asarray(src, np.uint32)
        d = FRESH_LO + self.rng.choice(FRESH_LO, len(src), replace=False)
        return np.stack([src, d, 1 + self.rng.integers(0, 1000, len(src))], 1).astype(np.uint32)


def interleave(*parts):
    parts = [p for p in parts if len(p)]
    out = np.concatenate(parts)
    order = np.argsort(np.concatenate([np.arange(len(p)) * len(parts) + i for i, p in enumerate(parts)]), kind="stable")
    return out[order].astype(np.uint32)


def neutral_batch(c, k):
    """k overwrites of existing edges, k deletes of existing edges, k adds of new edges: the edge count stays, nothing resizes.
    The two-vertex graph sits at the density where the loss of one edge of the wrong leaf halves the array: there the deletes
    take the batch's own adds away again."""
    k = max(1, min(k, len(c.ex) // 4))
    two = c.pick(2 * k)
    over, dele = two[:k].copy(), two[k:].copy()
    over[:, 2] += 3
    add = c.fresh(c.rng.integers(0, c.n, len(dele)))
    if len(c.ex) < 64:
        dele = add.copy()
        dele[:, 2] = 0
        return np.concatenate([interleave(add, over), dele])
    dele[:, 2] = 0
    return interleave(add, over, dele)


# ---- the writes W -------------------------------------------------------------------------------------------------------------
def w_single_ops(c):
    e = c.pick(2)
    f = c.fresh([c.n - 1])[0]
    return [("add_edge", int(f[0]), int(f[1]), 7), ("add_edge", int(e[0][0]), int(e[0][1]), int(e[0][2]) + 5),
            ("remove_edge", int(e[1][0]), int(e[1][1])), ("remove_edge", 0, FRESH_LO + 12345)]


def w_dup_overwrite(c):
    e = c.pick(1)[0]
    return [("add_edge", int(e[0]), int(e[1]), int(e[2]) + 5)]


def w_remove_missing(c):
    return [("remove_edge", c.n - 1, FRESH_LO + 4242)]


def w_batch(c):
    return [("apply", neutral_batch(c, 128))]


def rollback_batches(c, tries=6):
    """adds into four adjacent vertices, then their deletes: with small exclusive windows (big_window 256) some update turns
    exclusive after later ones were committed inside its window, which rolls the epoch back.  Every batch leaves the edge set as
    it found it."""
    out = []
    h = int(c.rng.integers(0, max(1, c.n - 4)))
    for _ in range(tries):
        add = c.fresh(h + c.rng.integers(0, min(4, c.n), c.rollback_k))
        dele = add[c.rng.permutation(len(add))].copy()
        dele[:, 2] = 0
        out.append(np.concatenate([add, dele]))
    return out


def w_spec_rollbacks(c):
    return [("opt", "big_window", 256), ("opt", "big_min", 64), ("rollbacks", rollback_batches(c))]


def w_big_windows(c):
    """a hub grows by what the rest of the graph loses: windows above big_min go to a workgroup of the round, those above
    big_window make the update exclusive"""
    k = min(800, len(c.ex) // 4)
    dele = c.pick(k)
    dele[:, 2] = 0
    hub = c.fresh(np.full(k, c.n // 3))
    return [("opt", "big_min", 512), ("opt", "big_window", 1024), ("apply", dele), ("apply", hub)]


def w_inplace(c):
    k = min(300, len(c.ex) // 4)
    dele = c.pick(k)
    dele[:, 2] = 0
    hub = c.fresh(np.full(k, c.n // 2))
    return [("opt", "rb_inplace_min", 2048), ("opt", "big_window", 1024), ("opt", "excl_in_wave", 64), ("apply", interleave(dele, hub)),
            ("rebalance", c.N // 2, 0), ("rebalance", c.N // 4, 1)]


def w_block_rebalance(c):
    wl = min(1024, c.N // 2)
    return [("block_rebalance", c.N // 2, wl), ("block_rebalance", 0, wl)]


def rebalance_windows(N):
    return sorted({min(w, N) for w in (N, N // 2, 4096)}, reverse=True)


def w_rebalance(w_index, upper):
    def build(c):
        ws = rebalance_windows(c.N)
        return [("rebalance", ws[min(w_index, len(ws) - 1)], upper)]
    return build


def w_doubling_batch(c):
    k = c.N  # more new edges than the array has slots
    return [("apply", c.fresh(c.rng.integers(0, c.n, k)))]


def w_grow_and_back(c):
    """inserts that double the array, then deletes (the inserts and most of what was there) until it is back at its size: the same
    N over a new generation of the arrays"""
    add = c.fresh(c.rng.integers(0, c.n, c.N // 2))
    dele = np.concatenate([add, c.ex[: len(c.ex) * 3 // 4]])
    dele = dele[c.rng.permutation(len(dele))].copy()
    dele[:, 2] = 0
    return [("apply", add), ("apply", dele), ("apply", c.ex[: len(c.ex) * 3 // 4].copy())]


def w_bench_resize(c):
    return [("bench_resize",)]


def w_add_nodes(c):
    new = np.repeat(np.arange(c.n, c.n + 3), 5)
    return [("add_node",), ("add_node",), ("add_node",), ("apply", c.fresh(new))]


def w_set_nn(c):
    v = np.unique(np.concatenate([[0, c.n - 1], c.rng.integers(0, c.n, 40)])).astype(np.uint32)
    return [("set_nn", np.stack([v, 1000 + v, np.ones_like(v)], 1).astype(np.uint32))]


# seam writes of the grid-stride loops: the first leaf / vertex 0, the last leaf / vertex n - 1, every leaf
def w_first(c):
    return [("add_edge", 0, 1, 9)]  # (dest 1 sorts in front of everything vertex 0 holds: its first leaf)


def w_last(c):
    return [("apply", c.fresh(np.full(48, c.n - 1)))]  # a hub on the last vertex slides towards slot N - 1


def w_every_leaf(c):
    return [("rebalance", c.N, 0)]


class W:
    def __init__(self, name, build, path, scheds=("strict",), exact=None, nodes_only=False, needs=()):
        self.name, self.build, self.path, self.scheds, self.exact, self.nodes_only, self.needs = name, build, path, scheds, exact, nodes_only, needs


BOTH = ("strict", "spec")
# rows 1, 2 and 5 of the table: run at every leaf size
ROW_1_2_5 = [
    W("single_ops", w_single_ops, "step", BOTH),
    W("dup_overwrite", w_dup_overwrite, "step", BOTH, exact=(1, 1)),  # one leaf and one node record differ: exactly those move
    W("remove_missing", w_remove_missing, "step", BOTH, nodes_only=True),
    W("batch", w_batch, "step", BOTH),
] + [W(f"rebalance_w{i}_{'upper' if u else 'lower'}", w_rebalance(i, u), "step") for i in range(3) for u in (0, 1)]
# rows 3, 4, 6 and 7: the mid graph
ROW_3_4 = [
    W("spec_rollbacks", w_spec_rollbacks, "step", ("spec",), needs=("rollbacks",)),
    W("big_windows", w_big_windows, "step", ("spec",), needs=("exclusive_ops",)),
    W("inplace_windows", w_inplace, "step", ("spec",), needs=("big_redistributes",)),
    W("block_rebalance", w_block_rebalance, "step"),
]
ROW_6_7 = [
    W("doubling_batch", w_doubling_batch, "full", BOTH, needs=("double_calls",)),
    W("grow_and_back", w_grow_and_back, "full", ("strict",), needs=("double_calls", "half_calls", "same_N")),
    W("bench_resize", w_bench_resize, "full", needs=("same_N",)),
    W("add_nodes", w_add_nodes, "full", BOTH),
]
SEAM = [W("first", w_first, "step"), W("last", w_last, "step", ("spec",)), W("every_leaf", w_every_leaf, "step")]
SET_NN = W("set_nn", w_set_nn, "step", nodes_only=True)
BY_NAME = {w.name: w for w in ROW_1_2_5 + ROW_3_4 + ROW_6_7 + SEAM + [SET_NN]}
FORMS = ("restore", "commit", "other")


def verify_batch(c):
    """V of the commit form (after the whole-array rebalance): a small batch that resizes nothing"""
    return neutral_batch(c, 16)


def followup_batch(c, size=2048):
    """check (d): updates, deletes and adds of existing and new edges in equal parts (the edge count stays where it was)"""
    q = size // 4
    have = c.ex[c.rng.integers(0, len(c.ex), 2 * q)].copy() if len(c.ex) else c.fresh(c.rng.integers(0, c.n, 2 * q))
    over, dele = have[:q].copy(), have[q:].copy()
    over[:, 2] += 1
    dele[:, 2] = 0
    add = c.fresh(c.rng.integers(0, c.n, q))
    miss = c.fresh(c.rng.integers(0, c.n, q))
    miss[:, 2] = 0
    return interleave(over, add, dele, miss)


# the random campaign: scripts of 12 steps over {S, R, the writes}; the seeds are the test's parameters
CAMPAIGN_SEEDS = (11, 12, 13, 14, 15, 16)
CAMPAIGN_WRITES = ("single_ops", "dup_overwrite", "remove_missing", "batch", "big_windows", "inplace_windows", "block_rebalance",
                   "rebalance_w0_lower", "rebalance_w1_upper", "rebalance_w2_upper", "doubling_batch", "bench_resize", "add_nodes")


def campaign_script(seed, steps=12):
    rng = np.random.default_rng(seed)
    out = ["S"]
    for _ in range(steps - 1):
        r = rng.random()
        out.append("S" if r < 0.2 else ("R" if r < 0.5 else str(rng.choice(CAMPAIGN_WRITES))))
    if "R" not in out[-3:]:
        out[-1] = "R"
    return out
