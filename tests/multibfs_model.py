"""Model of ppcsr_multi_bfs (include/ppcsr.h) in numpy and Python integers, with nothing of the package: per source a
level-synchronous BFS over the edges consumers_model.global_edges() gives, and from its level histogram reached, far and ecc as
Python ints and harmonic as the fp64 sum the header defines: (double)c(L) / (double)L added in ascending L, left to right."""
import numpy as np

NO_LEVEL = 0xFFFFFFFF


def adjacency(src, dst, n):
    """CSR rows over the edges with a destination < n (src ascending, as global_edges returns them)"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ok = dst < n
    s, d = src[ok], dst[ok]
    order = np.argsort(s, kind="stable")
    s, d = s[order], d[order]
    return np.searchsorted(s, np.arange(n + 1)), d


def levels_from(rows, d, n, start):
    """(levels uint32[n], hist): hist[L] = vertices at level L, hist[0] == 1"""
    lv = np.full(n, NO_LEVEL, np.uint32)
    lv[start] = 0
    front = np.array([start], np.int64)
    hist = [1]
    while True:
        a, lens = rows[front], rows[front + 1] - rows[front]
        total = int(lens.sum())
        if total == 0:
            break
        idx = np.repeat(a - np.cumsum(lens) + lens, lens) + np.arange(total)
        nb = d[idx]
        nb = np.unique(nb[lv[nb] == NO_LEVEL])
        if len(nb) == 0:
            break
        lv[nb] = len(hist)
        hist.append(len(nb))
        front = nb
    return lv, hist


def aggregates(hist):
    """(reached, far, ecc, harmonic) of one level histogram"""
    reached = sum(int(c) for c in hist)
    far = sum(L * int(c) for L, c in enumerate(hist))
    ecc = len(hist) - 1
    harmonic = 0.0
    for L in range(1, len(hist)):
        harmonic = harmonic + float(int(hist[L])) / float(L)
    return reached, far, ecc, harmonic


def hist_of(levels_row):
    """the level histogram of a row of levels (the aggregates of a device row, recomputed)"""
    lv = np.asarray(levels_row)
    lv = lv[lv != NO_LEVEL].astype(np.int64)
    return np.bincount(lv).tolist()


def model_multi_bfs(src, dst, n, sources):
    """dict: levels uint32[k, n], reached / far / ecc: lists of Python ints, harmonic float64[k], hists: the histograms; a repeated
    source is computed once and copied"""
    rows, d = adjacency(src, dst, n)
    sources = [int(s) for s in np.asarray(sources).ravel()]
    done = {}
    out = dict(levels=np.empty((len(sources), n), np.uint32), reached=[], far=[], ecc=[], harmonic=np.empty(len(sources), np.float64), hists=[])
    for i, s in enumerate(sources):
        assert 0 <= s < n
        if s not in done:
            done[s] = levels_from(rows, d, n, s)
        lv, hist = done[s]
        r, f, e, h = aggregates(hist)
        out["levels"][i] = lv
        out["reached"].append(r)
        out["far"].append(f)
        out["ecc"].append(e)
        out["harmonic"][i] = h
        out["hists"].append(hist)
    return out
