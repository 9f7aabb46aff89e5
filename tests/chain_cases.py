"""The cases of the rebalance position chain, shared by the CPU (emulator) and the GPU tests (TEST INFRASTRUCTURE ONLY).

A window case is (index, len, j): a window of `len` slots from slot `index` holding `j` live elements.  Every case a test runs
lies in the REFERENCE'S DOMAIN: the oracle's serial fp64 chain (PCSR.cpp:237-247) gives strictly rising positions — pos_1 >
pos_0 = index included — that stay below index + len.  Outside it (rounding accumulated over 10^7 ... 10^9 subtractions lets the
lowest ranks drift onto each other, below the window, or below zero) there is nothing to be bit-identical to.  The domain is
decided here, when the lists are generated, from the oracle alone; the candidates it drops are kept in OUT_OF_DOMAIN lists and
nothing is skipped when a test runs.  The generators are deterministic.
"""
import ctypes
import functools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle_lib import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "hostsim")
CSRC = os.path.join(ROOT, "parallel-packed-csr_amd", "csrc")
HOST_SO = os.path.join(SIM_DIR, "libchain_host.so")

LITERAL_MAX = 1 << 22   # the probe returns every position up to this many elements, digests above
DIGEST_LOG = 20
MAX_SEG = 128           # kMaxSeg
SAMPLE = 4096           # literal ranks at either end and either side of every segment boundary of a big case
KNEVER = 0xFFFFFFFF
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
c_u64 = ctypes.c_uint64
WORKERS = min(16, os.cpu_count() or 1)


# ---- the host build of the chain arithmetic (tests/hostsim/chain_host.cpp) --------------------------------------------------
@functools.lru_cache(None)
def host_lib():
    src = os.path.join(SIM_DIR, "chain_host.cpp")
    deps = [src, os.path.join(CSRC, "pma_geometry.h"), os.path.join(CSRC, "pma_types.h")]
    if not os.path.exists(HOST_SO) or os.path.getmtime(HOST_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fvisibility=hidden",
                        "-fvisibility-inlines-hidden", "-fPIC", "-shared", "-I" + CSRC, src, "-o", HOST_SO], check=True)
    L = ctypes.CDLL(HOST_SO)
    L.chain_host_table.argtypes = [c_u64, c_u64, c_u64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    L.chain_host_single.argtypes = [c_u64, c_u64, c_u64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    L.chain_host_div_operands.argtypes = [c_u64, c_u64, c_u64, ctypes.c_void_p]
    L.chain_host_thresholds.argtypes = [c_u64, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    return L


def host_table(index, ln, j):
    """(segments as an (nseg, 6) uint64 array: t0, count, M0, Dfirst, Drest, shift; overflow flag) of the HOST build"""
    segs = np.zeros((MAX_SEG, 6), np.uint64)
    ov = ctypes.c_int(0)
    n = host_lib().chain_host_table(index, ln, j, segs.ctypes.data, ctypes.byref(ov))
    return segs[:n].copy(), ov.value


def host_single(index, ln, j):
    """(verdict, segment) of chain_single and of chain_single_div on the host"""
    a, b = np.zeros(6, np.uint64), np.zeros(6, np.uint64)
    dv = ctypes.c_int(0)
    v = host_lib().chain_host_single(index, ln, j, a.ctypes.data, ctypes.byref(dv), b.ctypes.data)
    return v, a, dv.value, b


@functools.lru_cache(None)
def thresholds(N):
    """(H, logN, t_up[0..H], t_lo[0..H]) of an array of N slots (compute_geometry)"""
    up, lo = np.zeros(36, np.uint32), np.zeros(36, np.uint32)
    lg = ctypes.c_int(0)
    H = host_lib().chain_host_thresholds(N, up.ctypes.data, lo.ctypes.data, ctypes.byref(lg))
    return H, lg.value, [int(x) for x in up[:H + 1]], [int(x) for x in lo[:H + 1]]


# ---- the oracle's chain ------------------------------------------------------------------------------------------------------
def oracle_positions(index, ln, j):
    out = np.zeros(j, np.uint64)
    oracle_lib().po_redistribute_positions(index, ln, j, out.ctypes.data)
    return out


def oracle_digest(index, ln, j, ranges=()):
    """(domain status, digests per 2^20 ranks, literal positions of the ranks in `ranges`) from one pass of the serial chain"""
    dig = np.zeros(((j + (1 << DIGEST_LOG) - 1) >> DIGEST_LOG) or 1, np.uint64)
    lo = np.array([r[0] for r in ranges], np.uint64)
    hi = np.array([r[1] for r in ranges], np.uint64)
    out = np.zeros(max(int((hi - lo).sum()), 1), np.uint64)
    st = oracle_lib().po_redistribute_positions_digest(index, ln, j, DIGEST_LOG, dig.ctypes.data, len(ranges),
                                                       lo.ctypes.data if len(ranges) else None,
                                                       hi.ctypes.data if len(ranges) else None, out.ctypes.data)
    return st, dig, out


def digest_of_positions(pos, k0=0):
    """the same digest from literal positions, in numpy (third statement: checks the oracle's and the probe's against each other
    on small cases)"""
    with np.errstate(over="ignore"):
        k = np.arange(k0, k0 + len(pos), dtype=np.uint64)
        z = pos.astype(np.uint64) + k * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))


@functools.lru_cache(None)
def domain_status(case):
    """0 = the oracle's chain is a strictly rising placement inside the window (see po_redistribute_positions_digest)"""
    return oracle_lib().po_redistribute_positions_digest(case[0], case[1], case[2], DIGEST_LOG, None, 0, None, None, None)


def split_by_domain(cands):
    """(cases in the reference's domain, the others), order kept, duplicates dropped; decided by the oracle alone"""
    cands = list(dict.fromkeys(cands))
    with ThreadPoolExecutor(WORKERS) as ex:  # (ctypes releases the GIL: the serial chains of the big windows run side by side)
        st = list(ex.map(domain_status, cands))
    return [c for c, s in zip(cands, st) if s == 0], [c for c, s in zip(cands, st) if s != 0]


# ---- the case list of test_chain_table_matches_serial_fp64_chain, unchanged ---------------------------------------------------
def legacy_cases():
    rng = np.random.default_rng(5)
    cases = [(0, 1 << 24, 10_000_000), (0, 1 << 24, 4_194_305), (1 << 30, 1 << 30, 3_000_001), (0, 1 << 31, 2_500_000),
             (4096, 4096, 4095), (0, 8, 1), (0, 8, 2), (64, 64, 64), (12288, 8192, 3), (16384, 8192, 3), (8192, 8192, 7000)]
    for _ in range(60):
        lg = int(rng.integers(3, 25))
        ln = 1 << lg
        idx = int(rng.integers(0, 1 << (30 - lg))) * ln
        j = int(rng.integers(1, ln + 1))
        cases.append((idx, ln, j))
    # the windows ONE wave / one workgroup rebalances (closed form without the division): small windows at every kind of
    # start — slot 0, powers of two (the window fills its binade from the bottom), other multiples — and every fill
    for _ in range(2500):
        lg = int(rng.integers(3, 11))
        ln = 1 << lg
        kind = int(rng.integers(0, 4))
        idx = 0 if kind == 0 else ((1 << int(rng.integers(lg, 31))) if kind == 1 else int(rng.integers(1, 1 << (31 - lg))) * ln)
        j = int(rng.integers(1, ln + 1)) if rng.integers(0, 4) else int(rng.choice([1, 2, 3, 4, ln - 1, ln]))
        cases.append((idx, ln, max(j, 1)))
    return cases


# ---- PMA-shaped windows ---------------------------------------------------------------------------------------------------------
def window_fills(lg):
    """fills of a window of 2^lg slots: at and +-1 around every density threshold a window of that length can be rebalanced at (in
    every array of 2^10 ... 2^31 slots that has windows of that length), 1/3, 0.618 and 0.9 of it, 1, 2, 3, len - 1, len"""
    ln = 1 << lg
    js = {1, 2, 3, ln - 1, ln, ln // 3, int(0.618 * ln), int(0.9 * ln)}
    for m in range(max(lg, 10), 32):
        H, logN, up, lo = thresholds(1 << m)
        for L in range(H + 1):
            if (logN << (H - L)) == ln:
                for t in (up[L], lo[L]):
                    if t != KNEVER and t > 0:
                        js.update((t - 1, t, t + 1))
    return sorted(j for j in js if 1 <= j <= ln)


def pma_window_candidates(lg_lo=3, lg_hi=28):
    out = []
    for lg in range(lg_lo, lg_hi + 1):
        ln = 1 << lg
        for idx in dict.fromkeys([0, ln, 3 * ln, (1 << 31) - ln]):
            if idx + ln <= (1 << 31):
                out += [(idx, ln, j) for j in window_fills(lg)]
    return out


def resize_candidates(lo=10, hi=27):
    """(0, 2N, j) and (0, N/2, j) at (and +-1 around) the root thresholds of N: what double_list / half_list / bulk_build produce"""
    out = []
    for m in range(lo, hi + 1):
        N = 1 << m
        _, _, up, lw = thresholds(N)
        for t in (up[0], lw[0]):
            if t == KNEVER or t == 0:
                continue
            for j in (t - 1, t, t + 1):
                if j >= 1:
                    out.append((0, 2 * N, j))
                    if j <= N // 2:
                        out.append((0, N // 2, j))
    return out


def small_exhaustive_candidates():
    """every fill of every window of 2^3 ... 2^9 slots at index 0, len, 2 len, 3 len (4064 cases)"""
    return [(m * ln, ln, j) for ln in (1 << lg for lg in range(3, 10)) for m in range(4) for j in range(1, ln + 1)]


# the windows named in the issue that opened this module: the reference's own chain is no placement there
KNOWN_OUT_OF_DOMAIN = [(0, 1 << 28, 3 << 26), ((1 << 31) - (1 << 25), 1 << 25, 20737776), (3 << 28, 1 << 28, 241591910),
                       (0, 1 << 29, 331804423), (0, 1 << 30, 805306368)]


@functools.lru_cache(None)
def window_cases(max_lg):
    """(cases, out_of_domain) of every window family with windows of at most 2^max_lg slots (the legacy list keeps its sparse 2^30
    and 2^31 windows whatever max_lg is)"""
    cands = [c for c in legacy_cases()]
    cands += small_exhaustive_candidates()
    cands += pma_window_candidates(3, min(max_lg, 28))
    cands += [c for c in resize_candidates() if c[1] <= (1 << max_lg)]
    return split_by_domain(cands)


def big_case_ranges(case):
    """ranks whose literal positions a big case (j > 2^22) is checked on beside its digests: the first and the last 4096 and 4096
    either side of every segment boundary of the host table — merged, ascending, disjoint [lo, hi) ranges"""
    idx, ln, j = case
    segs, _ = host_table(idx, ln, j)
    marks = [0, j] + [j - 1 - int(t0) for t0 in segs[:, 0]]
    iv = sorted((max(0, m - SAMPLE), min(j, m + SAMPLE)) for m in marks)
    out = [list(iv[0])]
    for a, b in iv[1:]:
        if a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out if b > a]


# ---- segments with forced ties (raw operands of chain_segment) ------------------------------------------------------------------
def _dbl_bits(m, e):
    """bits of the double m * 2^(e - 52), 2^52 <= m < 2^53"""
    assert (1 << 52) <= m < (1 << 53) and -1000 < e < 1000
    return ((e + 1023) << 52) | (m & ((1 << 52) - 1))


def segment_cases():
    """(bits of x, bits of step, S, es) rows.  For r = e_x - e_step in 1 ... 52: steps whose low r mantissa bits are exactly half
    (1 then r - 1 zeros: the round-to-even tie of chain_segment) with the bit above 0 and 1 (q even and odd), half +- 1 and 0; x
    at that exponent distance with an even and an odd mantissa, near the top and near the bottom of its binade"""
    rows = []
    es = 1  # step in [2, 4): a density between 1/4 and 1/2, as in a window
    P = 0xA5A5A5A5A5A5A & ((1 << 52) - 1)
    top = 1 << 53
    for r in range(1, 53):
        half = 1 << (r - 1)
        rems = {half, 0}
        if r >= 2:
            rems.update((half - 1, half + 1))
        for rem in sorted(rems):
            for qbit in (0, 1):
                if r == 52:
                    if qbit == 0:
                        continue  # (bit 52 is the hidden bit: q = 1)
                    S = (1 << 52) | rem
                else:
                    S = (1 << 52) | ((P >> (r + 1)) << (r + 1)) | (qbit << r) | rem
                q = S >> r
                for mx in (top - 2, top - 1, top - 12346, top - 12345, (1 << 52) + 6, (1 << 52) + 7,
                           (1 << 52) + 3 * q + 4, (1 << 52) + 3 * q + 5):
                    if (1 << 52) <= mx < top:
                        rows.append((_dbl_bits(mx, es + r), _dbl_bits(S, es), S, es))
    # r = 0: x and step in one binade (x >= step)
    rows.append((_dbl_bits(top - 1, es), _dbl_bits((1 << 52) | 12345, es), (1 << 52) | 12345, es))
    rows.append((_dbl_bits((1 << 52) | 12346, es), _dbl_bits((1 << 52) | 12345, es), (1 << 52) | 12345, es))
    rows.append((_dbl_bits(top - 1, es), _dbl_bits(top - 1, es), top - 1, es))
    return list(dict.fromkeys(rows))


def segment_model(xbits, S, es, walk_cap=4096):
    """chain_segment and the walked subtractions restated in Python integers: x = M0 * 2^(e - 52), step = S * 2^(es - 52), r = e - es.
    While the exact difference stays at or above 2^e the result keeps x's exponent and its mantissa is M - d with
    d = M - RNE((M * 2^r - S) / 2^r): Dfirst = d(M0), Drest = d(M0 - Dfirst) (away from an exact tie d does not depend on M; at a
    tie the first result is even and every later step repeats the second one's choice).  That holds for a step from mantissa M
    iff M * 2^r - S >= 2^52 * 2^r, i.e. M >= Th = 2^52 + ceil(S / 2^r); the count is the number of steps taken from such
    mantissas: 0 if M0 < Th (or the decrement is 0), else 1 if M1 < Th, else 2 + (M1 - Th) // Drest — closed form, no loop.
    Returns (M0, shift, Dfirst, Drest, count, bit patterns of min(count + 1, walk_cap) exactly rounded subtractions from x)."""
    e = ((xbits >> 52) & 0x7FF) - 1023
    M0 = (xbits & ((1 << 52) - 1)) | (1 << 52)
    r = e - es
    shift = 52 - e
    Df = Dr = count = 0
    if shift >= 0 and 0 <= r <= 52:
        def dec(M):
            qq, rem = divmod((M << r) - S, 1 << r)
            if 2 * rem > (1 << r) or (2 * rem == (1 << r) and (qq & 1)):
                qq += 1
            return M - qq
        Df = dec(M0)
        Dr = dec(M0 - Df)
        Th = (1 << 52) + -((-S) >> r)
        M1 = M0 - Df
        if M0 >= Th and Dr > 0:
            count = 1 if M1 < Th else 2 + (M1 - Th) // Dr
    walked = []
    m, ex = M0, e
    for _ in range(min(count + 1, walk_cap)):
        m, ex = _sub_rne(m, ex, S, es)
        walked.append(_pack(m, ex))
    return M0, shift, Df, Dr, count, walked


def _sub_rne(m, ex, S, es):
    """RN-even(m * 2^(ex-52) - S * 2^(es-52)) as (mantissa with hidden bit, exponent); 0 -> (0, -1023); results are positive normal
    numbers or zero in every case the tests build"""
    base = min(ex, es)
    num = (m << (ex - base)) - (S << (es - base))  # exact, in units of 2^(base - 52)
    assert num >= 0
    if num == 0:
        return 0, -1023
    nb = num.bit_length()
    if nb <= 53:
        return num << (53 - nb), base - (53 - nb)
    sh = nb - 53
    q, rem = num >> sh, num & ((1 << sh) - 1)
    if 2 * rem > (1 << sh) or (2 * rem == (1 << sh) and (q & 1)):
        q += 1
    if q == (1 << 53):
        q >>= 1
        sh += 1
    return q, base + sh


def _pack(m, ex):
    if m == 0:
        return 0
    return ((ex + 1023) << 52) | (m & ((1 << 52) - 1))


# ---- operands of the table build's division ----------------------------------------------------------------------------------------
def div_operands_of(cases):
    """(a, b) = (M1 - Th, Drest) of every segment of every window case, collected from the host build"""
    L = host_lib()
    buf = np.zeros((MAX_SEG, 2), np.uint64)
    out = []
    for idx, ln, j in cases:
        n = L.chain_host_div_operands(idx, ln, j, buf.ctypes.data)
        out += [(int(a), int(b)) for a, b in buf[:n]]
    return list(dict.fromkeys(out))


def div_cases(window_list):
    top = (1 << 53) - 1
    pairs = div_operands_of(window_list)
    bs = sorted({b for _, b in pairs})
    # a thinned set of the Drest values (every 7th and the extremes) carries the constructed quotients
    pick = sorted(set(bs[::7] + bs[:3] + bs[-3:]))
    extra_b = {1, top}
    for k in range(1, 53):
        extra_b.update((1 << k, (1 << k) - 1, (1 << k) + 1))
    for b in sorted(set(pick) | {b for b in extra_b if 1 <= b <= top}):
        qs = {0, 1, 2, 3, top // b, top // b - 1, (1 << 31), (1 << 31) - 1, (1 << 20) + 1, 12345678, 999}
        for q in qs:
            if q < 0 or q > (1 << 31):
                continue
            for a in (q * b - 1, q * b, q * b + 1):
                if 0 <= a <= top:
                    pairs.append((a, b))
        pairs += [(0, b), (b - 1, b), (top, b)]
    return list(dict.fromkeys(pairs))
