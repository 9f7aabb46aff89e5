"""The scenarios of the bulk-build tests as data (tests/test_sim_bulk.py runs the small ones on the emulator, tests/test_gpu_bulk.py
all of them on the device; the driver is tests/bulk_checks.py, the expectation tests/bulk_model.py).  Every stream is deterministic:
counter-based draws from streams.py and explicit arrays.  The shapes are the smallest at which each piece of ppcsr_bulk_build can
go wrong: the degenerate vertex ranges of k_bb_vertices, the key range of the device's radix sort (32 + bits(n) key bits), runs
of duplicates, the array-size rule from both sides of its threshold, the tile seams of the flag scan (kScanTile = 1024 flags per
workgroup; the tile-sum kernel takes more than one tile per thread past 2^20 rows) and the grid-stride loops (grid_for caps the grid
at 8192 workgroups of 256)."""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

MAX = 0xFFFFFFFF
U32 = np.uint32


@dataclass(frozen=True)
class Case:
    name: str
    n: int                                  # vertices the engine is created with
    ops: Callable                           # streams -> rows (src, dst, value) handed to bulk_build
    follow: Optional[Callable] = None       # (streams, n) -> updates applied afterwards; None: default_follow
    pre: Optional[str] = None               # history of the engine before the call: "add_nodes" | "grown_shrunk"
    large: bool = False                     # device only, lock_search True only, host form only
    expect_N0: Optional[int] = None         # array size just before the call (None: whatever a fresh engine has)
    expect_N: Optional[int] = None          # array size the rule must choose
    then: Optional[Callable] = None         # (streams, n) -> a second stream of updates after `follow`
    then_N: Optional[int] = None            # array size the oracle started from the model must have after `then`
    expect_E: Optional[int] = None          # surviving edges

    @property
    def locks(self):
        return (True,) if self.large else (True, False)


def rows(src, dst, val):
    src, dst, val = (np.asarray(x, np.uint64) for x in (src, dst, val))
    return np.ascontiguousarray(np.stack([src, dst, val], 1).astype(U32))


def none():
    return np.zeros((0, 3), U32)


def default_follow(streams, n, count=600, seed=7):
    """adds and deletes over the whole vertex range (about a third of the deletes hit nothing: num_neighbors moves on its own)"""
    return streams.random_stream(n, count, seed=seed, p_delete=0.35)


def with_ignored(ops, n, every=9):
    """every `every`-th row becomes a row to ignore, the two kinds and the extreme source in turn"""
    ops = ops.copy()
    ops[0::3 * every, 2] = 0
    ops[every::3 * every, 0] = n
    ops[2 * every::3 * every, 0] = MAX
    return ops


# ---- degenerate vertex ranges ----------------------------------------------------------------------------------------------------
def _isolated_ends(streams, n, k, m, ignored):
    s = streams.uniform_ints(11, m, n - 2 * k - 1) + (k + 1)  # sources in (k, n - k): vertices 0..k and n - k.. stay isolated
    ops = rows(s, streams.uniform_ints(12, m, 500), streams.uniform_ints(13, m, 90) + 1)
    return with_ignored(ops, n) if ignored else ops


DEGENERATE = [
    Case("n1_m0", 1, lambda st: none(), expect_E=0),
    Case("n1_50_adds", 1, lambda st: rows(np.zeros(50), (np.arange(50) * 7) % 31, np.arange(50) + 1), expect_E=31),
    Case("n2", 2, lambda st: rows(st.uniform_ints(3, 40, 3), st.uniform_ints(4, 40, 9), np.arange(40) % 5)),  # (src 2, value 0: ignored)
    Case("all_ignored", 50, lambda st: rows(np.where(np.arange(200) % 2, 50 + np.arange(200), np.arange(200) % 50), np.arange(200) % 17,
                                            np.arange(200) % 2), expect_E=0),
    Case("only_vertex_0", 64, lambda st: rows(np.zeros(300), st.uniform_ints(5, 300, 4000), np.arange(300) + 1)),
    Case("only_last_vertex", 64, lambda st: rows(np.full(300, 63), st.uniform_ints(6, 300, 4000), np.arange(300) + 1)),
    Case("isolated_ends", 200, lambda st: _isolated_ends(st, 200, 10, 900, True)),    # rank[a] read at the first ignored key
    Case("isolated_tail_a_eq_m", 200, lambda st: _isolated_ends(st, 200, 10, 900, False)),  # no ignored rows: a == m for the tail
]


# ---- key and sort range ----------------------------------------------------------------------------------------------------------
EDGE_DSTS = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], np.uint64)


def _key_range(streams, n):
    m = 3000
    s = streams.uniform_ints(21 + n, m, n)
    s[::7] = n - 1                                        # the last source: the highest key the sort must keep below the ignored ones
    d = streams.uniform_ints(22 + n, m, 1 << 32)
    d[::4] = EDGE_DSTS[(np.arange(len(d[::4])) // 3) % len(EDGE_DSTS)]
    v = streams.uniform_ints(23 + n, m, 0xFFFFFFFE) + 1  # 1 .. 0xFFFFFFFE
    v[::50] = 0xFFFFFFFE
    d[d == MAX] = 5
    ops = with_ignored(rows(s, d, v), n, every=5)
    ops[7::90, 0] = n + 1
    return ops


def _key_follow(streams, n):
    f = streams.random_stream(n, 500, seed=31, p_delete=0.3)
    f[::6, 1] = EDGE_DSTS[np.arange(len(f[::6])) % len(EDGE_DSTS)].astype(U32)
    f[::6, 0] = n - 1
    return f


KEY_RANGE = [Case(f"keys_n{n}", n, (lambda st, n=n: _key_range(st, n)), follow=_key_follow) for n in (1023, 1024, 1025)]


# ---- duplicates ------------------------------------------------------------------------------------------------------------------
def _dup_5000(streams):
    other = streams.random_stream(300, 20000, seed=41)
    other[:, 2] = streams.uniform_ints(42, 20000, 1000) + 1
    other[(other[:, 0] == 7) & (other[:, 1] == 9), 1] = 10   # the repeated key belongs to the copies alone
    ops = np.empty((25000, 3), U32)
    ops[0::5] = rows(np.full(5000, 7), np.full(5000, 9), np.arange(5000) + 1)
    for r in range(1, 5):
        ops[r::5] = other[r - 1::4]
    return ops


def _dup_tail(streams, n, ignored):
    """the highest key of the stream, (n - 1, 0xFFFFFFFE), four times with values 11..14: with ignored rows they follow it directly
    in sorted order, without them its last copy is the last row of the sorted stream (i + 1 == m)"""
    ops = streams.random_stream(n, 700, seed=43)
    ops[:, 2] = 3
    if ignored:
        ops = with_ignored(ops, n)
    ops[[100, 250, 400, 699]] = rows(np.full(4, n - 1), np.full(4, 0xFFFFFFFE), [11, 12, 13, 14])
    return ops


DUPLICATES = [
    Case("dup_5000_copies", 300, _dup_5000),
    Case("dup_last_valid_key", 120, lambda st: _dup_tail(st, 120, True)),
    Case("dup_last_row", 120, lambda st: _dup_tail(st, 120, False)),
    Case("all_copies_of_one_edge", 10, lambda st: rows(np.full(777, 3), np.full(777, 5), np.arange(777) + 1), expect_E=1),
]


# ---- the array-size rule: n = 1000 vertices in 2048 slots; (n + E + 1) / N < 0.75 holds up to E = 534 (N = 2048) and E = 2070 (4096) --
def _distinct(E, n=1000):
    i = np.arange(E)
    return rows(i % n, 7 + i // n, i % 5 + 1)


# At E = 534 and 2070 the array is as full as the rule lets it be.  One more add follows, then adds to one vertex until the root's
# density bound is consulted — the reference looks at it only when every window below it overflows, so the one add alone leaves the
# array size as it is (in the oracle: checked) —: the oracle started from the model doubles, and the engine must with it.
def _one_more(streams, n):
    return rows([n // 2], [0xABCDEF], [1])


def _hub(streams, n):
    return rows(np.full(600, n // 2), 0x1000000 + 3 * np.arange(600), np.arange(600) % 7 + 1)


SIZE_RULE = [Case(f"size_E{E}", 1000, (lambda st, E=E: _distinct(E)), expect_N0=2048, expect_N=N, expect_E=E,
                  follow=_one_more if grow else None, then=_hub if grow else None, then_N=2 * N if grow else None)
             for E, N, grow in [(533, 2048, False), (534, 2048, True), (535, 4096, False), (536, 4096, False), (2070, 4096, True),
                                (2071, 8192, False), (2072, 8192, False)]]


# ---- seams of the flag scan ------------------------------------------------------------------------------------------------------
def _scan_rows(streams, n, m):
    ops = streams.random_stream(n, m, seed=50 + m % 97)
    ops[:, 2] = streams.uniform_ints(51, m, 7) + 1
    ops[-1] = (n - 1, 0xFFFFFFF0, 9)          # the last row of the sorted stream is a survivor: the flag at index m - 1
    return ops


SCAN_SEAMS = [Case(f"scan_m{m}", 300, (lambda st, m=m: _scan_rows(st, 300, m))) for m in (1023, 1024, 1025, 2049)]
SCAN_LARGE = [Case("scan_m2p20_plus_1", 65536, lambda st: _scan_rows(st, 65536, (1 << 20) + 1), large=True,
                   follow=lambda st, n: default_follow(st, n, 4000))]


# ---- grid-stride seams (8192 workgroups of 256 = 2^21 threads per trip) ----------------------------------------------------------------
def _many_vertices(streams, n, m):
    ops = streams.random_stream(n, m, seed=61)
    ops[:, 2] = 2
    trip = 1 << 21
    ops[:12, 0] = [0, 1, trip - 2, trip - 1, trip, trip + 1, n - 2, n - 1, trip - 1, trip, n - 1, 0]
    return with_ignored(ops, n, every=101)


def _many_vertices_follow(streams, n):
    f = default_follow(streams, n, 4000)
    trip = 1 << 21
    f[:6, 0] = [trip - 1, trip, trip + 1, n - 1, 0, trip]
    return f


GRID_STRIDE = [
    Case("grid_rows_2p21_plus_3000", 3000, lambda st: with_ignored(_scan_rows(st, 3000, (1 << 21) + 3000), 3000, every=1001), large=True,
         follow=lambda st, n: default_follow(st, n, 4000)),
    Case("grid_vertices_2p21_plus_777", (1 << 21) + 777, lambda st: _many_vertices(st, (1 << 21) + 777, 100000), large=True,
         follow=_many_vertices_follow),
]


# ---- prior history of the engine -------------------------------------------------------------------------------------------------
def _history_rows(streams, n, m):
    ops = streams.random_stream(n, m, seed=71)
    ops[:, 2] = streams.uniform_ints(72, m, 9) + 1
    return with_ignored(ops, n)


def grow_stream(streams):
    """4000 adds that take a 100-vertex engine from 2048 to 8192 slots; deleted again, the array is halved down to 512"""
    a = streams.random_stream(100, 4000, seed=3)
    a[:, 2] = 1
    return a


HISTORY = [
    Case("after_5_add_node", 100, lambda st: _history_rows(st, 105, 2500), pre="add_nodes"),  # (sources 100..104 exist by then)
    Case("grown_8192_shrunk_512", 100, lambda st: _history_rows(st, 100, 1800), pre="grown_shrunk", expect_N0=512),
]


SMALL = DEGENERATE + KEY_RANGE + DUPLICATES + SIZE_RULE + SCAN_SEAMS + HISTORY
LARGE = SCAN_LARGE + GRID_STRIDE
BY_NAME = {c.name: c for c in SMALL + LARGE}
assert len(BY_NAME) == len(SMALL) + len(LARGE)


def single_params(cases, forms=("host", "device")):
    """(case name, lock_search, form) of every run: the device form (rows already in device memory, through a one-partition
    PPPCSR) for every case with rows and without a history — the routed call does nothing for an empty block —, the host form for all"""
    out = []
    for c in cases:
        for lock in c.locks:
            for form in forms:
                if form == "device" and (c.large or c.pre or c.name == "n1_m0"):
                    continue
                out.append((c.name, lock, form))
    return out


# ---- partitioned: pppcsr_bulk_build_device itself ----------------------------------------------------------------------------------
PP_N = 4000


def pp_direct_rows(streams, starts, n=PP_N, m=6000):
    """global-src adds for the partitions that start at `starts`: 60 % of the rows go to partition 1, every third partition from
    the third on receives nothing at all, the rest share what is left; ignored rows of both kinds are spread over the stream (op == 0
    in receiving partitions only; src >= n goes to the last partition, as the routing rule says)"""
    P = len(starts)
    ends = np.append(starts[1:], n).astype(np.int64)
    starts = np.asarray(starts, np.int64)
    recv = np.array([k for k in range(P) if k < 2 or k % 3 != 2 or k == P - 1], np.int64)
    recv = recv[ends[recv] > starts[recv]]
    pick = streams.uniform_ints(81, m, 1000)
    part = np.where(pick < 600, 1, recv[streams.uniform_ints(82, m, len(recv))])
    size = ends[part] - starts[part]
    s = starts[part] + (streams.uniform_ints(83, m, 1 << 30).astype(np.int64) % size)
    ops = rows(s, streams.uniform_ints(84, m, 300), streams.uniform_ints(85, m, 50) + 1)
    ops[0::13, 2] = 0
    ops[5::29, 0] = n + np.arange(len(ops[5::29]), dtype=U32)
    ops[11::301, 0] = MAX
    silent = [k for k in range(P) if k not in set(recv.tolist())]
    return ops, silent


# ---- partitioned: repartition shapes ------------------------------------------------------------------------------------------------
RP_N, RP_P = 1400, 4


def rp_core(streams):
    core = streams.random_stream(RP_N, 9000, seed=91, p_delete=0.15)   # duplicates and deletes of missing edges: num_neighbors != degree
    return core


def rp_layouts():
    """an empty partition ([0, 100, 100, 700]-style, scaled to n), then one boundary moved by one vertex: exactly two partitions change"""
    empty = np.array([0, RP_N // 7, RP_N // 7, RP_N // 2], np.uint64)
    shift = empty.copy()
    shift[3] += 1
    return [("empty_partition", empty, [0, 1, 2, 3]), ("one_vertex_shift", shift, [2, 3])]
