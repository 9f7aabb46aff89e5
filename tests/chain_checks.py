"""The comparisons of the position-chain probe (PCSR.debug_chain_probe) with the oracle's serial chain, the host build of the
table and exact integer models — shared by tests/test_sim_chain.py (emulator) and tests/test_gpu_chain.py (MI355X).  Every
comparison is exact.  TEST INFRASTRUCTURE ONLY."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import chain_cases as cc

POS_BUDGET = 1 << 24  # output words per probe call


def _batches(cases):
    """cases in list order, cut where a call's outputs would exceed POS_BUDGET words (a big case is a call of its own)"""
    out, cur, words = [], [], 0
    for c in cases:
        w = c[2] if c[2] <= cc.LITERAL_MAX else 0
        if cur and (words + w > POS_BUDGET or len(cur) >= 1024 or c[2] > cc.LITERAL_MAX or cur[-1][2] > cc.LITERAL_MAX):
            out.append(cur)
            cur, words = [], 0
        cur.append(c)
        words += w
    if cur:
        out.append(cur)
    return out


_DIGESTS = {}  # big case -> the oracle's digests (a serial pass of up to 2^28 steps each: shared by the modes of one session)


def _expected(case, literal_ranges=False):
    """what the oracle's serial chain gives: ("lit", positions) or ("dig", digests, ranges, positions of the ranks in them)"""
    idx, ln, j = case
    if j <= cc.LITERAL_MAX:
        return ("lit", cc.oracle_positions(idx, ln, j))
    if not literal_ranges and case in _DIGESTS:
        return ("dig", _DIGESTS[case], (), None)
    ranges = cc.big_case_ranges(case) if literal_ranges else ()
    st, dig, lit = cc.oracle_digest(idx, ln, j, ranges)
    assert st == 0, case  # (the lists hold cases of the reference's domain only)
    _DIGESTS[case] = dig
    return ("dig", dig, ranges, lit)


def check_windows(eng, cases, mode, grid=0, label="", literal_ranges=True):
    """`table` / `published`: positions == oracle chain, segment words == the host build's, nseg equal, overflow 0.  Big cases
    (j > 2^22): digests per 2^20 ranks, and with literal_ranges the literal positions of big_case_ranges as well.
    Returns dict(max_nseg, workgroups, partial, fallbacks, cases_with_partial)."""
    tot = dict(max_nseg=0, workgroups=0, partial=0, fallbacks=0, cases_with_partial=0, cases=0)
    with ThreadPoolExecutor(cc.WORKERS) as ex:
        for batch in _batches(cases):
            exp_f = [ex.submit(_expected, c, literal_ranges) for c in batch]
            exp = [f.result() for f in exp_f]
            samples = [np.concatenate([np.arange(a, b, dtype=np.uint64) for a, b in e[2]]) if e[0] == "dig" and e[2] else np.zeros(0, np.uint64)
                       for e in exp]
            res = eng.debug_chain_probe(mode, batch, samples=samples, grid=grid)
            for c, case in enumerate(batch):
                tag = f"{label}{mode} {case}"
                hseg, hov = cc.host_table(*case)
                assert hov == 0 and res["overflow"][c] == 0, tag
                assert res["nseg"][c] == len(hseg), (tag, res["nseg"][c], len(hseg))
                np.testing.assert_array_equal(res["segs"][c][:len(hseg)], hseg, err_msg=tag + " segment words")
                assert not res["segs"][c][len(hseg):].any(), tag
                e = exp[c]
                if e[0] == "lit":
                    np.testing.assert_array_equal(res["pos"][c], e[1], err_msg=tag + " positions")
                else:
                    if e[2]:
                        np.testing.assert_array_equal(res["samples"][c], e[3][:len(res["samples"][c])], err_msg=tag + " literal ranks")
                    np.testing.assert_array_equal(res["pos"][c], e[1], err_msg=tag + " digests per 2^20 ranks")
                tot["max_nseg"] = max(tot["max_nseg"], len(hseg))
                tot["cases"] += 1
                if mode == "published":
                    w = res["wg"][c]
                    tot["workgroups"] += int(w[0])
                    tot["partial"] += int(w[1])
                    tot["fallbacks"] += int(w[2])
                    tot["cases_with_partial"] += 1 if w[1] else 0
    return tot


def published_cases(cases, min_workgroups=64):
    """the cases the hand-off is tested on: at least two segments and enough elements for `min_workgroups` tiles of 4096 ranks"""
    return [c for c in cases if c[2] >= min_workgroups * 4096 and len(cc.host_table(*c)[0]) >= 2]


def check_single(eng, cases):
    """verdict and segment == host chain_single and chain_single_div; positions == oracle where accepted; aligned windows away from
    slot 0 are always accepted.  Returns the number of accepted cases."""
    taken = 0
    with ThreadPoolExecutor(cc.WORKERS) as ex:
        for batch in _batches(cases):
            exp = list(ex.map(_expected, batch))
            res = eng.debug_chain_probe("single", batch)
            for c, case in enumerate(batch):
                idx, ln, j = case
                hv, hs, dv, ds = cc.host_single(*case)
                assert res["verdict"][c] == hv == dv, (case, res["verdict"][c], hv, dv)
                if j >= 2 and idx >= ln and idx % ln == 0:
                    assert hv == 1, case
                if not hv:
                    assert res["pos"][c] is None
                    continue
                taken += 1
                np.testing.assert_array_equal(res["segs"][c][0], hs, err_msg=f"single {case} segment")
                np.testing.assert_array_equal(hs[[2, 3, 4, 5]], ds[[2, 3, 4, 5]], err_msg=f"single {case} vs the division form")
                e = exp[c]
                if e[0] == "lit":
                    np.testing.assert_array_equal(res["pos"][c], e[1], err_msg=f"single {case} positions")
                else:
                    np.testing.assert_array_equal(res["pos"][c], e[1], err_msg=f"single {case} digests")
    return taken


def check_linear(eng, cases):
    """every run the linear form accepts reproduces chain_pos; returns the number of accepted runs"""
    runs = 0
    for lo in range(0, len(cases), 1024):
        batch = cases[lo:lo + 1024]
        res = eng.debug_chain_probe("linear", batch, want_segs=False)
        bad = [(c, int(m)) for c, m in zip(batch, res["mismatches"]) if m]
        assert not bad, bad[:10]
        assert not res["overflow"].any()
        runs += int(res["runs"].astype(np.int64).sum())
    return runs


def check_segments(eng, rows):
    """chain_segment's words and step count == the integer model; the device's walked subtractions == the same integers"""
    res = eng.debug_chain_probe("segment", rows)
    ties = 0
    for c, (xb, sb, S, es) in enumerate(rows):
        M0, shift, Df, Dr, count, walked = cc.segment_model(xb, S, es)
        got = res["segs"][c]
        tag = f"segment x={xb:#x} step={sb:#x}"
        assert (int(got[2]), int(got[3]), int(got[4]), int(got[5]) & 0xFFFFFFFF) == (M0, Df, Dr, shift & 0xFFFFFFFF), (tag, got, (M0, Df, Dr, shift))
        assert int(got[1]) == count, (tag, int(got[1]), count)
        assert res["steps"][c] == len(walked), tag
        np.testing.assert_array_equal(res["walk"][c], np.array(walked, np.uint64), err_msg=tag + " walked values")
        # the model against itself: on the segment the walked mantissas ARE the arithmetic progression the table stores
        e = ((xb >> 52) & 0x7FF) - 1023
        for i in range(1, min(count, len(walked)) + 1):
            m = M0 - Df - (i - 1) * Dr
            assert walked[i - 1] == (((e + 1023) << 52) | (m & ((1 << 52) - 1))), (tag, i)
        r = e - es
        if r >= 1 and (S & ((1 << r) - 1)) == (1 << (r - 1)):
            ties += 1
    return ties


def check_div(eng, pairs):
    """quotient == a // b for every pair; returns the largest |estimate - quotient| and the pair it was seen on"""
    arr = np.array(pairs, np.uint64)
    res = eng.debug_chain_probe("div", arr)
    want = np.array([a // b for a, b in pairs], np.uint64)
    np.testing.assert_array_equal(res["q"], want)
    err = np.abs(res["est"].astype(np.int64) - want.astype(np.int64))  # (quotients are below 2^53)
    w = int(err.argmax())
    return int(err[w]), pairs[w]
