"""What tests/test_sim_ktruss.py (the emulator) and tests/test_gpu_ktruss.py (the device) share: the comparison of
ppcsr_edge_support / ppcsr_ktruss with tests/truss_model.py, and the constructed graphs.  Everything is compared exactly."""
import ctypes

import numpy as np

from consumers_model import global_edges, partition_states
from truss_model import assert_hard, counters_of, hardness, model_truss, rows_of

EINVAL, ENOMEM, EUNSUPPORTED, ERANGE = 1, 2, 4, 6
WAVE_SLOTS = 4096  # kBfsWaveSlots


def model_of(pp):
    states = partition_states(pp)
    src, dst = global_edges(states)
    n = pp.get_n()
    mt = model_truss(src, dst, n)
    return states, src, dst, mt, hardness(src, dst, n, mt, firsts=[f for f, _, _ in states])


def check(pp, label, identities=True, **hard):
    """edge list and order, count, total, tmax, vtruss and counters [0] .. [5] against the model; the conditions on the input
    from the model; the identities with triangles() and kcore() on the same engine; nothing written (states and stats)"""
    n = pp.get_n()
    stats = [pp.partition(k).stats() for k in range(pp.num_partitions())]
    states, src, dst, mt, h = model_of(pp)
    assert_hard(h, label, **hard)
    sup, total, ms = pp.edge_support(with_ms=True)
    np.testing.assert_array_equal(sup, rows_of(mt["a"], mt["b"], mt["support"]), err_msg=f"{label}: support")
    assert total == mt["total"] and ms >= 0.0, (label, total, mt["total"])
    ctr = pp.debug_ktruss_counters()
    assert ctr[:6].tolist() == [len(mt["a"]), mt["total"], 0, 0, 0, 0], (label, ctr)
    edges, tmax, vtruss, ms = pp.ktruss(with_ms=True)
    np.testing.assert_array_equal(edges, rows_of(mt["a"], mt["b"], mt["truss"]), err_msg=f"{label}: truss")
    assert tmax == mt["tmax"] and ms >= 0.0, (label, tmax, mt["tmax"])
    np.testing.assert_array_equal(vtruss, mt["vtruss"], err_msg=f"{label}: vtruss")
    ctr = pp.debug_ktruss_counters()
    assert ctr[:6].tolist() == counters_of(mt), (label, ctr, counters_of(mt))
    assert ctr[7] >= 2 + mt["levels"] + sum(mt["subrounds"]), (label, ctr)
    if identities:
        tri, tri_total = pp.triangles()
        assert int(sup[:, 2].sum(dtype=np.int64)) == 3 * tri_total, label
        at = np.bincount(sup[:, 0], weights=sup[:, 2], minlength=n) + np.bincount(sup[:, 1], weights=sup[:, 2], minlength=n)
        np.testing.assert_array_equal(at.astype(np.uint64), 2 * tri, err_msg=f"{label}: support per vertex")
        core, kmax = pp.kcore()
        assert np.all(vtruss <= core + 1) and tmax <= kmax + 1, label
    for (f0, i0, n0), (f1, i1, n1) in zip(states, partition_states(pp)):
        assert f0 == f1 and np.array_equal(i0, i1) and np.array_equal(n0, n1), label
    assert stats == [pp.partition(k).stats() for k in range(pp.num_partitions())], label
    return mt, h, ctr


def upper(pairs):
    """rows (min, max, 1) of undirected pairs"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.stack([p.min(axis=1), p.max(axis=1), np.ones(len(p), np.int64)], axis=1).astype(np.uint32)


def clique(ids):
    ids = np.asarray(ids)
    i, j = np.triu_indices(len(ids), 1)
    return np.stack([ids[i], ids[j]], axis=1)


def cylinder(rings, base=0):
    """a triangulated cylinder of `rings` rings of 4 vertices: the ring cycles, and per quad one vertical and one diagonal edge"""
    i, j = np.meshgrid(np.arange(rings), np.arange(4), indexing="ij")
    v = lambda a, b: base + 4 * a + b % 4
    ring = np.stack([v(i, j), v(i, j + 1)], axis=-1).reshape(-1, 2)
    up = i < rings - 1
    vert = np.stack([v(i, j)[up], v(i + 1, j)[up]], axis=-1)
    diag = np.stack([v(i, j)[up], v(i + 1, j + 1)[up]], axis=-1)
    return np.concatenate([ring, vert, diag])


def check_k9(make):
    """K9 alone: every edge has support 7 and truss 9, all in one sub-round"""
    pp = make(12)
    pp.apply(upper(clique(np.arange(1, 10))))
    mt, h, ctr = check(pp, "K9")
    assert np.all(mt["support"] == 7) and np.all(mt["truss"] == 9) and ctr[:6].tolist() == [36, 84, 1, 1, 1, 36]
    assert pp.ktruss()[2].tolist() == [0] + [9] * 9 + [0, 0]
    pp.close()


def check_closed_forms(make, seed):
    """K9, a K6 and a K5 sharing an edge (truss 6 on the K6, the shared edge included, 5 on the rest of the K5), a cycle and a
    tree (truss 2) and isolated vertices (vtruss 0), on permuted ids in one shuffled stream; then the orientation convention"""
    n = 300
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    k9, k6, k5x, cyc, tree, lone = perm[:9], perm[9:15], perm[15:18], perm[18:60], perm[60:160], perm[160:]
    k5 = np.concatenate([k6[:2], k5x])
    pairs = [clique(k9), clique(k6), clique(k5)[1:], np.stack([cyc, np.roll(cyc, -1)], axis=1),
             np.array([[tree[i], tree[rng.integers(0, i)]] for i in range(1, len(tree))])]  # (clique(k5)[0] is the shared edge)
    ops = upper(np.concatenate(pairs))
    ops = ops[rng.permutation(len(ops))]
    pp = make(n)
    pp.apply(ops)
    mt, h, _ = check(pp, "closed forms", gaps=2, distinct=4)
    want = {}
    for ids, k in ((k9, 9), (k5, 5), (k6, 6)):  # (the K6 last: the shared edge takes its 6)
        for x, y in clique(ids):
            want[min(x, y), max(x, y)] = k
    for a, b, t in zip(mt["a"].tolist(), mt["b"].tolist(), mt["truss"].tolist()):
        assert t == want.get((a, b), 2), (a, b, t)
    edges, tmax, vtruss = pp.ktruss()
    assert tmax == 9 and not vtruss[lone].any() and np.all(vtruss[cyc] == 2) and np.all(vtruss[tree] == 2) and np.all(vtruss[k9] == 9)
    assert np.all(vtruss[k6] == 6) and np.all(vtruss[k5x] == 5)
    # a self-loop, a destination >= n and backward pairs (between isolated vertices, and inside the tree) change nothing
    a, b = sorted(int(x) for x in lone[:2])
    pp.apply(np.array([[a, a, 1], [a, n + 3, 1], [b, a, 1], [max(tree[0], tree[5]), min(tree[0], tree[5]), 1]], np.uint32))
    check(pp, "closed forms + no-ops", backward=2, loops=1, beyond=1)
    again, tmax2, vtruss2 = pp.ktruss()
    np.testing.assert_array_equal(again, edges)
    np.testing.assert_array_equal(vtruss2, vtruss)
    # both directions stored: the same results as the upper triangle alone
    pp.apply(ops[:, [1, 0, 2]])
    sym, tmax3, vtruss3 = pp.ktruss()
    np.testing.assert_array_equal(sym, edges)
    np.testing.assert_array_equal(vtruss3, vtruss)
    np.testing.assert_array_equal(pp.edge_support()[0][:, 2], mt["support"])
    check(pp, "closed forms, symmetric", backward=len(ops))
    pp.close()


def check_cylinder(make):
    """150 rings: every edge has truss 3, in ONE level of as many sub-rounds as the model's peel takes from the two ends inward"""
    rings = 150
    n = 4 * rings + 8
    ops = upper(cylinder(rings, base=3))
    pp = make(n)
    pp.apply(ops[np.random.default_rng(2).permutation(len(ops))])
    mt, h, ctr = check(pp, "cylinder", max_subrounds=rings // 2, below_support=len(ops) // 2)
    assert np.all(mt["truss"] == 3) and mt["levels"] == 1 and mt["widest"] <= 16 and ctr[2] == 1 and ctr[3] == ctr[4] == mt["subrounds"][0]
    pp.close()


def check_book(make, pages=5000):
    """spine {0, 1} with `pages` pages: one sub-round of 2 * pages frontier edges, every triangle with two of them (the
    smaller-slot rule), `pages` decrements of the spine's word, and the spine itself — both of its sides beyond one wave's
    reach — handed to the long-range kernel, in the support phase and in the peel"""
    n = pages + 10
    p = np.arange(2, pages + 2)
    ops = upper(np.concatenate([[[0, 1]], np.stack([np.zeros_like(p), p], axis=1), np.stack([np.ones_like(p), p], axis=1)]))
    pp = make(n)
    pp.apply(ops[np.random.default_rng(4).permutation(len(ops))])
    for v in (0, 1):
        node = pp.getNode(v)
        assert node[1] - node[0] - 1 > WAVE_SLOTS, node
    mt, h, ctr = check(pp, "book", max_support=pages, widest=2 * pages)
    assert np.all(mt["truss"] == 3) and mt["support"][0] == pages and mt["subrounds"] == [2]
    assert ctr[6] == 1, ctr  # (the spine, in the second sub-round)
    pp.close()


def rmat_stream(streams, n, scale, adds, seed, folded):
    """(core adds, a mixed stream over stored and fresh pairs with destinations >= n and a planted K_32, which the shifted destinations thin out: levels with gaps)"""
    s, d = (streams.rmat_edges_folded(n, scale, adds, seed=seed) if folded else streams.rmat_edges(scale, adds, seed=seed))
    core = streams.adds(s, d)
    s2, d2 = (streams.rmat_edges_folded(n, scale, adds // 40, seed=seed + 1) if folded else streams.rmat_edges(scale, adds // 40, seed=seed + 1))
    fresh = streams.adds(s2, (d2 + np.uint32(7)) % np.uint32(n))
    gone = core[np.random.default_rng(seed).choice(len(core), len(core) // 20, replace=False)].copy()
    gone[:, 2] = 0
    planted = upper(clique(np.random.default_rng(seed + 2).choice(n, 32, replace=False)))
    mixed = np.concatenate([fresh, gone, planted, core[::7], np.array([[5, 5, 1]], np.uint32)])  # (core[::7]: duplicate adds)
    mixed = mixed[np.random.default_rng(seed + 3).permutation(len(mixed))]
    mixed[::19, 1] += np.uint32(n)  # destinations beyond the graph
    return core, np.ascontiguousarray(mixed)


def same(x, y):
    """two ktruss() / edge_support() results, word for word"""
    assert len(x) == len(y)
    for p, q in zip(x, y):
        if isinstance(p, np.ndarray):
            np.testing.assert_array_equal(p, q)
        else:
            assert p == q


def check_status_codes(pkg, make, streams, n, lib=None):
    """each EINVAL; ERANGE with everything else delivered; the size query; EUNSUPPORTED in the sequential regime, with its
    message; n vertices without an upper edge"""
    pp = make(n, 3)
    L, h = pp.L, pp.h
    e = pp.partition(0)
    count, total, tmax = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(77)
    vt = np.full(n, 77, np.uint32)
    ms = ctypes.c_double(-1.0)
    # no upper edge: nothing stored, then backward pairs and a self-loop only
    for ops in (None, np.array([[9, 2, 1], [4, 4, 1], [n - 1, 0, 1]], np.uint32)):
        if ops is not None:
            pp.apply(ops)
        assert L.pppcsr_ktruss(h, None, 0, ctypes.byref(count), ctypes.byref(tmax), vt.ctypes.data, None) == 0
        assert count.value == 0 and tmax.value == 0 and not vt.any()
        assert L.pppcsr_edge_support(h, None, 0, ctypes.byref(count), ctypes.byref(total), None) == 0 and count.value == 0 and total.value == 0
        edges, t, v = pp.ktruss()
        assert edges.shape == (0, 3) and t == 0 and not v.any()
        assert not pp.debug_ktruss_counters()[:7].any()
        vt[:] = 77
    s, d = streams.rmat_edges_folded(n, int(np.ceil(np.log2(n))), 10 * n, seed=2)
    pp.apply(np.concatenate([streams.adds(s, d), streams.random_stream(n, 4 * n, seed=1)]))
    _, _, _, mt, hh = model_of(pp)
    m = len(mt["a"])
    assert hh["tmax"] >= 4 and m > 100
    buf = np.zeros((m, 3), np.uint32)
    for sup_fn, tr_fn, hh_, nv in ((L.pppcsr_edge_support, L.pppcsr_ktruss, h, n), (L.ppcsr_edge_support, L.ppcsr_ktruss, e.h, e.get_n())):
        assert sup_fn(hh_, None, 0, None, None, None) == EINVAL and tr_fn(hh_, None, 0, None, None, None, None) == EINVAL
        assert sup_fn(None, None, 0, ctypes.byref(count), None, None) == EINVAL and tr_fn(None, None, 0, ctypes.byref(count), None, None, None) == EINVAL
        count.value = 1 << 40
        assert sup_fn(hh_, None, 0, ctypes.byref(count), None, None) == 0 and count.value < 1 << 40  # cap = 0 with edges = NULL: the size query
        total.value = 1 << 40
        assert sup_fn(hh_, None, 0, None, ctypes.byref(total), ctypes.byref(ms)) == 0 and total.value < 1 << 40 and ms.value >= 0.0
        tmax.value = 77
        assert tr_fn(hh_, None, 0, None, ctypes.byref(tmax), None, None) == 0 and tmax.value != 77
        vt[:] = 77
        assert tr_fn(hh_, None, 0, None, None, vt.ctypes.data, None) == 0 and int(vt[:nv].max()) == tmax.value and np.all(vt[nv:] == 77)
    # ERANGE at cap = count - 1: count, tmax and vtruss delivered, the first cap entries right, nothing behind them written
    want = rows_of(mt["a"], mt["b"], mt["truss"])
    buf[:] = 0xABABABAB
    vt[:] = 77
    assert L.pppcsr_ktruss(h, buf.ctypes.data, m - 1, ctypes.byref(count), ctypes.byref(tmax), vt.ctypes.data, None) == ERANGE
    assert count.value == m and tmax.value == mt["tmax"]
    np.testing.assert_array_equal(vt, mt["vtruss"])
    np.testing.assert_array_equal(buf[: m - 1], want[: m - 1])
    assert np.all(buf[m - 1] == 0xABABABAB)
    buf[:] = 0xABABABAB
    assert L.pppcsr_edge_support(h, buf.ctypes.data, m - 1, ctypes.byref(count), ctypes.byref(total), None) == ERANGE
    assert count.value == m and total.value == mt["total"]
    np.testing.assert_array_equal(buf[: m - 1], rows_of(mt["a"], mt["b"], mt["support"])[: m - 1])
    assert np.all(buf[m - 1] == 0xABABABAB)
    assert L.pppcsr_ktruss(h, buf.ctypes.data, m + 5, ctypes.byref(count), None, None, None) == 0  # (room to spare)
    np.testing.assert_array_equal(buf, want)
    # the sequential regime is refused, before anything runs, with the reason
    before = pp.debug_ktruss_counters()
    last = pp.partition(2)
    last.set_option("search_narrow", 0)
    assert last.stats()["narrow"] == 0
    for rc in (L.pppcsr_ktruss(h, None, 0, ctypes.byref(count), ctypes.byref(tmax), None, None),
               L.pppcsr_edge_support(h, None, 0, ctypes.byref(count), ctypes.byref(total), None),
               L.ppcsr_ktruss(last.h, None, 0, ctypes.byref(count), ctypes.byref(tmax), None, None),
               L.ppcsr_edge_support(last.h, None, 0, ctypes.byref(count), ctypes.byref(total), None)):
        assert rc == EUNSUPPORTED
        assert "sequential regime" in L.ppcsr_last_error().decode()
    assert "ktruss" in L.ppcsr_last_error().decode() or "edge_support" in L.ppcsr_last_error().decode()
    np.testing.assert_array_equal(pp.debug_ktruss_counters(), before)
    assert L.ppcsr_ktruss(e.h, None, 0, ctypes.byref(count), None, None, None) == 0  # (a partition in the regular regime answers)
    last.set_option("search_narrow", 1)
    same(pp.ktruss(), (want, mt["tmax"], mt["vtruss"]))
    assert L.ppcsr_debug_ktruss_counters(e.h, None) == EINVAL and L.ppcsr_debug_ktruss_counters(None, vt.ctypes.data) == EINVAL
    # a handle that holds only some partitions of its layout
    loc = pkg.PPPCSR(n, numDomain=1, partitionsPerDomain=4, local=(1, 2, 0), **({"lib": lib} if lib is not None else {}))
    assert L.pppcsr_ktruss(loc.h, None, 0, ctypes.byref(count), None, None, None) == EINVAL
    assert "not resident" in L.ppcsr_last_error().decode()
    assert L.pppcsr_edge_support(loc.h, None, 0, ctypes.byref(count), None, None) == EINVAL
    loc.close()
    return pp


def slot_search_cases():
    """-> (items, rows, want): one buffer for the slot-returning search (ppcsr_debug_isect_probe, mode probe, reserved = 1) — keys
    on the first and the last live slot, below, above and between the live dests, a first probe that lands in a null run of 64,
    65 and 200 slots (with the key on either side of the run), and a sentinel inside the range"""
    N = 4096
    e = np.zeros((N, 3), np.uint32)
    e[:, 0] = 0xFFFFFFFF
    e[:, 1] = np.random.default_rng(1).integers(0, 3 * N, N)  # junk under the nulls
    rows, want = [], []

    def put(slots):
        e[slots, 0], e[slots, 1], e[slots, 2] = 3, 100 + 3 * np.asarray(slots), 1

    def ask(lo, hi, key):
        rows.append((0, 0, lo, hi, key, 0))
        hit = [s for s in range(lo, hi) if e[s, 2] != 0 and e[s, 1] == key]
        assert len(hit) <= 1
        want.append(hit[0] if hit else 0xFFFFFFFF)

    base = 0
    for run in (64, 65, 200):
        # live slots, a null run around the range's midpoint, live slots: [base, base + 2 * run + 40)
        lo, hi = base, base + 2 * run + 40
        left = np.arange(lo, lo + 20 + run // 2)[::2]
        right = np.arange(lo + 20 + run // 2 + run, hi)[::3]
        put(left)
        put(right)
        mid = lo + (hi - lo) // 2
        assert left[-1] < mid < right[0] and not e[left[-1] + 1: right[0], 2].any() and right[0] - left[-1] - 1 >= run
        live = np.concatenate([left, right])
        for s in (live[0], live[-1], left[-1], right[0], left[len(left) // 2], right[len(right) // 2]):
            ask(lo, hi, 100 + 3 * int(s))  # on the first and the last live slot, on both rims of the run, inside either half
        for key in (0, 99, 100 + 3 * int(live[0]) - 1, 100 + 3 * int(live[-1]) + 1, 0xFFFFFFFE, 100 + 3 * int(left[-1]) + 1,
                    100 + 3 * int(right[0]) - 1, 100 + 3 * int(left[1]) + 1, 100 + 3 * mid):
            ask(lo, hi, key)  # below, above, inside the run's span, between two live dests
        ask(lo, lo, 100 + 3 * lo)  # an empty range
        ask(int(live[0]), int(live[0]) + 1, 100 + 3 * int(live[0]))
        ask(int(live[0]) + 1, hi, 100 + 3 * int(live[0]))  # the key's slot just outside the range
        base = hi + 17
    # a sentinel inside the range, behind the last live slot (live dests ascend): dest 0xFFFFFFFF, above every key
    lo, hi = base, base + 90
    put(np.arange(lo, lo + 60)[::2])
    e[lo + 60] = (3, 0xFFFFFFFF, 0xFFFFFFFF)
    for t in (lo, lo + 20, lo + 44):
        ask(lo, hi, 100 + 3 * t)
    ask(lo, hi, 0xFFFFFFFF)
    rows.append((0, 0, lo, hi, 0xFFFFFFFE, 0))
    want.append(0xFFFFFFFF)
    rows, want = np.array(rows, np.uint32), np.array(want, np.uint32)
    assert np.count_nonzero(want != 0xFFFFFFFF) >= 20 and np.count_nonzero(want == 0xFFFFFFFF) >= 20
    return np.ascontiguousarray(e), rows, want


def check_slot_search(eng):
    """the slot-returning search alone on the device, and on the search cases of tests/isect_cases.py"""
    import isect_cases as ic
    items, rows, want = slot_search_cases()
    got = eng.debug_isect_probe("probe", rows, items, slot=True)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(rows[i].tolist(), int(got[i]), int(want[i])) for i in bad[:8]]
    np.testing.assert_array_equal(eng.debug_isect_probe("probe", rows, items), (want != 0xFFFFFFFF).astype(np.uint32))
    s = ic.search_cases()
    e, pr = s["items"], s["probe_rows"]
    want = np.full(len(pr), 0xFFFFFFFF, np.uint32)
    for i, (_, _, lo, hi, key, _) in enumerate(pr.tolist()):
        r = e[lo:hi]
        hit = np.nonzero((r[:, 2] != 0) & (r[:, 1] == key))[0]
        if len(hit):
            want[i] = lo + int(hit[0])
    assert np.array_equal(want != 0xFFFFFFFF, ic.want_probe(e, pr) != 0)
    np.testing.assert_array_equal(eng.debug_isect_probe("probe", pr, e, slot=True), want)
