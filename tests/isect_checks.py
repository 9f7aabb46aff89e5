"""The comparisons of the intersection probe (PCSR.debug_isect_probe) with the numpy model of tests/isect_cases.py, shared by the
emulator module and the GPU module.  Every comparison is exact."""
import functools

import numpy as np

import isect_cases as ic


@functools.lru_cache(maxsize=None)
def intersect_set():
    """the cases of the intersecting modes with their expected counts and credits, computed once"""
    c = ic.intersect_cases()
    c["want"], c["want_tri"] = ic.want_counts(c["items_a"], c["items_b"], c["rows"], tri_n=ic.N_MAX)
    c["lane"] = np.array(["lane" in t for t in c["tags"]])
    return c


@functools.lru_cache(maxsize=None)
def search_set():
    s = ic.search_cases()
    s["want_lb"] = ic.want_lower_bound(s["items"], s["lb_rows"])
    s["want_probe"] = ic.want_probe(s["items"], s["probe_rows"])
    return s


def _report(c, sel, got, want, label):
    bad = np.nonzero(got != want)[0]
    rows, tags = c["rows"][sel], [t for t, s in zip(c["tags"], sel) if s]
    lines = [f"case {rows[i].tolist()} {sorted(tags[i])}: got {int(got[i])}, want {int(want[i])}" for i in bad[:8].tolist()]
    assert not len(bad), f"{label}: {len(bad)} of {len(got)} cases differ\n" + "\n".join(lines)


def check_intersect(eng, mode):
    """counts of every case and the credits of all of them, operands in the given order and exchanged; -> cases run"""
    c = intersect_set()
    sel = c["lane"] if mode == "lane" else np.ones(len(c["rows"]), bool)
    rows, want = c["rows"][sel], c["want"][sel]
    want_tri = c["want_tri"] if mode != "lane" else ic.want_counts(c["items_a"], c["items_b"], rows, tri_n=ic.N_MAX)[1]
    got, tri = eng.debug_isect_probe(mode, rows, c["items_a"], c["items_b"], tri_n=ic.N_MAX)
    _report(c, sel, got, want, mode)
    np.testing.assert_array_equal(tri, want_tri, err_msg=f"{mode}: credits")
    got = eng.debug_isect_probe(mode, ic.swapped(rows), c["items_b"], c["items_a"])  # (no tri: the routines' null branch)
    _report(c, sel, got, want, f"{mode}, operands exchanged")
    return int(sel.sum())


def check_one_buffer(eng, mode):
    """two ranges of ONE buffer (items_b left out), as for two vertices of one partition: ranges of the first buffer against each
    other, overlapping and identical ones included"""
    c = intersect_set()
    ia = c["items_a"]
    rows = c["rows"][c["lane"]] if mode == "lane" else c["rows"]
    rng = np.random.default_rng(5)
    k = 150
    x, y = rows[rng.integers(0, len(rows), k)], rows[rng.integers(0, len(rows), k)]
    one = np.stack([x[:, 0], x[:, 1], y[:, 0], y[:, 1], np.minimum(x[:, 4], y[:, 4]), np.maximum(x[:, 5], y[:, 5])], axis=1)
    one = np.concatenate([one, x[:40, [0, 1, 0, 1, 4, 5]]])  # a range with itself
    # (ranges of one buffer may span several constructed ranges: the binding's ascending-order assertion decides which are usable)
    keep = [i for i, r in enumerate(one) if all(np.all(np.diff(ic.live_dests(ia, int(lo), int(hi))) > 0) for lo, hi in ((r[0], r[1]), (r[2], r[3])))]
    one = np.ascontiguousarray(one[keep].astype(np.uint32))
    assert len(one) >= 100
    want, want_tri = ic.want_counts(ia, ia, one, tri_n=ic.N_MAX)
    assert np.count_nonzero(want) >= 20
    got, tri = eng.debug_isect_probe(mode, one, ia, None, tri_n=ic.N_MAX)
    np.testing.assert_array_equal(got, want, err_msg=f"{mode}: one buffer")
    np.testing.assert_array_equal(tri, want_tri, err_msg=f"{mode}: one buffer, credits")


def check_lower_bound(eng):
    s = search_set()
    got = eng.debug_isect_probe("lower_bound", s["lb_rows"], s["items"])
    bad = np.nonzero(got != s["want_lb"])[0]
    assert not len(bad), [(s["lb_rows"][i].tolist(), int(got[i]), int(s["want_lb"][i])) for i in bad[:8]]
    return len(got)


def check_probe(eng):
    s = search_set()
    got = eng.debug_isect_probe("probe", s["probe_rows"], s["items"])
    bad = np.nonzero(got != s["want_probe"])[0]
    assert not len(bad), [(s["probe_rows"][i].tolist(), int(got[i]), int(s["want_probe"][i])) for i in bad[:8]]
    assert 0 < np.count_nonzero(got) < len(got)
    return len(got)


def check_einval(pkg, eng):
    """a bad case is refused on the host: ranges that leave their buffer, lo > hi, tri with n == 0, n beyond tri, unknown mode"""
    items = np.zeros((100, 3), np.uint32)
    items[:, 1] = np.arange(100)
    items[:, 2] = 1
    small = np.ascontiguousarray(items[:40])
    ok = [0, 100, 0, 40, 0, 50]
    assert eng.debug_isect_probe("lane", [ok], items, small)[0] == 40
    for mode in ic_modes():
        for bad in ([0, 101, 0, 40, 0, 50], [0, 100, 0, 41, 0, 50], [5, 4, 0, 40, 0, 50], [0, 100, 9, 8, 0, 50],
                    [0, 100, 0xFFFFFFFF, 0xFFFFFFFF, 0, 50], [0xFFFFFFF0, 0xFFFFFFFF, 0, 40, 0, 50]):
            with np.testing.assert_raises_regex(pkg.PpcsrError, "status 1 "):
                eng.debug_isect_probe(mode, [ok, bad], items, small)
        with np.testing.assert_raises_regex(pkg.PpcsrError, "status 1 "):
            eng.debug_isect_probe(mode, [[0, 100, 0, 100, 0, 50]], items, small)  # (b's range lies in the 40-slot buffer)
        if mode in ("lane", "wave", "block"):
            with np.testing.assert_raises_regex(pkg.PpcsrError, "status 1 "):
                eng.debug_isect_probe(mode, [ok], items, small, tri_n=0)
            with np.testing.assert_raises_regex(pkg.PpcsrError, "status 1 "):
                eng.debug_isect_probe(mode, [ok], items, small, tri_n=49)
            got, tri = eng.debug_isect_probe(mode, [ok], items, small, tri_n=50)
            assert got[0] == 40 and tri.sum() == 40
    import ctypes
    io = pkg.IsectProbeIO(mode=5, ncases=0)
    assert eng.L.ppcsr_debug_isect_probe(eng.h, ctypes.byref(io)) == 1
    assert eng.L.ppcsr_debug_isect_probe(eng.h, None) == 1
    io = pkg.IsectProbeIO(mode=0, ncases=0)
    assert eng.L.ppcsr_debug_isect_probe(eng.h, ctypes.byref(io)) == 0
    # the binding refuses a range whose live dests descend before the library sees it
    items[50, 1] = 3
    with np.testing.assert_raises(AssertionError):
        eng.debug_isect_probe("wave", [ok], items, small)
    assert eng.debug_isect_probe("wave", [[0, 50, 0, 40, 0, 50]], items, small)[0] == 40


def ic_modes():
    return ["lane", "wave", "block", "lower_bound", "probe"]
