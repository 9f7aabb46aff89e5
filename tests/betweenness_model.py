"""Model of ppcsr_path_counts / ppcsr_betweenness, built from the partitions' exported states like tests/paths_model.py: the
edge set is the one BFS walks (paths_model.global_edges_valued without the values; destinations >= n skipped), directed.
Brandes' algorithm level by level.  The number of shortest paths is kept in Python integers, so it is exact at any size.
The dependencies come in two forms: exact, on fractions.Fraction, and fp64 with the device's three operations per DAG edge
(numpy, np.add.at per level) for graphs where Fractions would take too long.

tolerance() is the bound derived in include/ppcsr.h — nothing here is measured: all terms are non-negative, so a sum of m
terms in any order carries a relative error of at most (m - 1) u, u = 2^-53; a term adds three roundings (the division, the
addition, the multiplication).  delta of a vertex D' levels above the deepest one therefore carries at most
D' (dmax - 1 + 3) u to first order, and bc adds k such values: (D (dmax + 2) + k) u."""
from fractions import Fraction

import numpy as np

from consumers_model import NO_LEVEL

U = 2.0 ** -53


def tolerance(D, dmax, k, against_fp64=False):
    """relative bound on |bc - exact|; against the fp64 model, which carries the same error itself, twice that"""
    t = (D * (dmax + 2) + k) * U
    return 2 * t if against_fp64 else t


def csr(src, dst, n):
    ok = dst < n
    s, d = src[ok], dst[ok]
    if len(s) and not np.all(s[:-1] <= s[1:]):
        order = np.argsort(s, kind="stable")
        s, d = s[order], d[order]
    return np.searchsorted(s, np.arange(n + 1)), d


def dag(rows, d, n, start):
    """levels from `start`, and per level L the arrays (v, w) of the stored edges with level[v] = L, level[w] = L + 1"""
    lv = np.full(n, NO_LEVEL, np.uint32)
    lv[start] = 0
    front = np.array([start], np.int64)
    per_level, sizes = [], [1]
    level = 0
    while len(front):
        a, lens = rows[front], rows[front + 1] - rows[front]
        idx = np.repeat(a - np.cumsum(lens) + lens, lens) + np.arange(int(lens.sum()))
        nb, sv = d[idx], np.repeat(front, lens)
        new = np.unique(nb[lv[nb] == NO_LEVEL])
        lv[new] = level + 1
        on = lv[nb] == level + 1
        if len(new):
            per_level.append((sv[on], nb[on]))
            sizes.append(len(new))
        front = new
        level += 1
    return lv, per_level, sizes


def sigma_exact(per_level, n, start):
    sg = [0] * n
    sg[start] = 1
    for v, w in per_level:
        for a, b in zip(v.tolist(), w.tolist()):
            sg[b] += sg[a]
    return sg


def model_path_counts(src, dst, n, start):
    """(levels uint32, sigma as a list of Python integers, info)"""
    rows, d = csr(src, dst, n)
    lv, per_level, sizes = dag(rows, d, n, start)
    sg = sigma_exact(per_level, n, start)
    return lv, sg, dict(D=len(sizes) - 1, widest=max(sizes), reached=int(sum(sizes)), max_sigma=max(sg))


def sigma_as_f64(sg):
    return np.array([float(x) for x in sg], np.float64)  # (int -> float rounds to nearest: what an exact sum stores)


def model_betweenness(src, dst, n, sources, exact, counts=None):
    """(bc, info).  exact: bc is a list of Fractions, sigma Python integers.  Otherwise bc is float64: sigma float64 sums
    (exact below 2^53, asserted by the callers through info['max_sigma']), delta with (sv / sw) * (1 + dw) per edge.
    info: D (deepest level over the sources), dmax (largest out-degree), widest level, most vertices reached, max sigma.
    counts (a dict, fp64 form): filled with {source: (levels, sigma)} of the same run"""
    rows, d = csr(src, dst, n)
    info = dict(D=0, dmax=int(np.diff(rows).max()) if n else 0, widest=0, reached=0, max_sigma=0)
    bc = [Fraction(0)] * n if exact else np.zeros(n, np.float64)
    for s in [int(x) for x in sources]:
        lv, per_level, sizes = dag(rows, d, n, s)
        info["D"] = max(info["D"], len(sizes) - 1)
        info["widest"] = max(info["widest"], max(sizes))
        info["reached"] = max(info["reached"], int(sum(sizes)))
        if exact:
            sg = sigma_exact(per_level, n, s)
            info["max_sigma"] = max(info["max_sigma"], max(sg))
            delta = [Fraction(0)] * n
            for v, w in reversed(per_level):
                for a, b in zip(v.tolist(), w.tolist()):
                    delta[a] += Fraction(sg[a], sg[b]) * (1 + delta[b])
            for v in range(n):
                if v != s and delta[v]:
                    bc[v] += delta[v]
        else:
            sg = np.zeros(n, np.float64)
            sg[s] = 1.0
            for v, w in per_level:
                np.add.at(sg, w, sg[v])
            info["max_sigma"] = max(info["max_sigma"], float(sg.max()))
            if counts is not None:
                counts[s] = (lv, sg)
            delta = np.zeros(n, np.float64)
            for v, w in reversed(per_level):
                np.add.at(delta, v, (sg[v] / sg[w]) * (1.0 + delta[w]))
            delta[s] = 0.0
            bc += delta
    return bc, info


def assert_bc(got, want, tol, label=""):
    """|got - want| <= tol * want for every vertex (want: Fractions or float64; a zero must be an exact zero)"""
    got = np.asarray(got, np.float64)
    assert len(got) == len(want), label
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), label
    if isinstance(want, np.ndarray):
        err = np.abs(got - want)
        bad = np.nonzero(err > tol * want)[0]
        worst = float(np.max(err[want > 0] / want[want > 0])) if np.any(want > 0) else 0.0
    else:
        t = Fraction(tol)
        bad, worst = [], 0.0
        for v, (g, w) in enumerate(zip(got.tolist(), want)):
            e = abs(Fraction(g) - w)
            if e > t * w:
                bad.append(v)
            if w:
                worst = max(worst, float(e / w))
    assert len(bad) == 0, f"{label}: {len(bad)} vertices beyond the bound {tol:.3g}, first {list(bad[:5])}, worst relative error {worst:.3g}"
    return worst


def non_integers(want):
    if isinstance(want, np.ndarray):
        return int(np.count_nonzero(want != np.floor(want)))
    return sum(1 for w in want if w.denominator != 1)


def diamond_chain(n, links, seed):
    """a chain of `links` two-wide diamonds over permuted ids: a_i -> {b_i, c_i} -> a_(i+1); 2^i paths reach a_i"""
    perm = np.random.default_rng(seed).permutation(n)
    a, b, c = perm[: links + 1], perm[links + 1: 2 * links + 1], perm[2 * links + 1: 3 * links + 1]
    ops = []
    for i in range(links):
        ops += [[a[i], b[i], 1], [a[i], c[i], 1], [b[i], a[i + 1], 1], [c[i], a[i + 1], 1]]
    return np.array(ops, np.uint32), a
