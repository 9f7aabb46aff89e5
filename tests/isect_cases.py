"""Cases and numpy model of the intersection probe (PCSR.debug_isect_probe), shared by tests/test_sim_isect.py (emulator) and
tests/test_gpu_isect.py (MI355X).

Ranges are laid out slot by slot as Edge arrays (src, dest, value): value == 0 is a null, a sentinel has dest 0xFFFFFFFF.  Nulls
hold JUNK dests — values that would match if a routine looked at them — so that reading a null shows.  The expected answers come
from numpy alone (np.intersect1d / np.isin / the first live slot with dest >= key).  What the generator promises — every length,
both forms of isect_wave on neighbouring lengths, streamed and probed tiles of isect_block, empty and filtered steps and tiles,
the merge cursor's seams — is asserted from the arrays by a route model of the thresholds (which routine FORM answers a case;
never what it answers)."""
import numpy as np

SENT = 0xFFFFFFFF
LANE_SLOTS, STEP, LOPSIDED, TILE, WAVE_SLOTS = 32, 64, 8, 1024, 4096  # pma_intersect.h / pma_scan.h thresholds
N_MAX = 1 << 16      # every case's n is at most this
BUF_MAX = 1 << 16    # slots of the largest buffer
SHORT = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129]
LONG = [1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5]
LANE_MAX = 4200      # longest operand given to the one-lane routine (it has no limit of its own; this bounds the serial walk)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def live_dests(items, lo, hi):
    r = items[lo:hi]
    return r[r[:, 2] != 0, 1].astype(np.int64)


def matches(ia, ib, row):
    """the dests counted by an intersecting case, ascending"""
    alo, ahi, blo, bhi, frm, n = (int(x) for x in row)
    c = np.intersect1d(live_dests(ia, alo, ahi), live_dests(ib, blo, bhi))
    return c[(c >= frm) & (c < n)]


def want_counts(ia, ib, rows, tri_n=None):
    out = np.zeros(len(rows), np.uint32)
    tri = np.zeros(tri_n or 0, np.uint64)
    for i, row in enumerate(rows):
        c = matches(ia, ib, row)
        out[i] = len(c)
        if tri_n:
            tri += np.bincount(c, minlength=tri_n).astype(np.uint64)
    return (out, tri) if tri_n else out


def want_lower_bound(ib, rows):
    out = np.zeros(len(rows), np.uint32)
    for i, row in enumerate(rows):
        blo, bhi, key = int(row[2]), int(row[3]), int(row[4])
        r = ib[blo:bhi]
        at = np.nonzero((r[:, 2] != 0) & (r[:, 1] >= key))[0]
        out[i] = blo + at[0] if len(at) else bhi
    return out


def want_probe(ib, rows):
    return np.array([np.isin(int(r[4]), live_dests(ib, int(r[2]), int(r[3]))) for r in rows], np.uint32)


# ---- the route model: which form of a routine a case takes (thresholds only) ---------------------------------------------------------
def _ordered(ia, ib, row):
    """(shorter items, lo, hi, longer items, lo, hi) as isect_wave / isect_block order them: b is swapped in when strictly shorter"""
    alo, ahi, blo, bhi = (int(x) for x in row[:4])
    if bhi - blo < ahi - alo:
        return ib, blo, bhi, ia, alo, ahi
    return ia, alo, ahi, ib, blo, bhi


def counted(items, lo, hi, frm, n):
    """mask over [lo, hi): the slots a staged tile keeps"""
    r = items[lo:hi]
    return (r[:, 2] != 0) & (r[:, 1] >= frm) & (r[:, 1] < n)


def wave_form(ia, ib, row):
    """'empty' | 'probe' | 'merge'"""
    _, slo, shi, _, llo, lhi = _ordered(ia, ib, row)
    if shi == slo:
        return "empty"
    return "probe" if (lhi - llo) // LOPSIDED > shi - slo else "merge"


def _first_ge(items, lo, hi, key):
    r = items[lo:hi]
    at = np.nonzero((r[:, 2] != 0) & (r[:, 1].astype(np.int64) >= key))[0]
    return lo + int(at[0]) if len(at) else hi


def block_tiles(ia, ib, row):
    """per tile of the shorter operand: 'none' (nothing staged: all null or all filtered) | 'stream' | 'probe', with the tile's
    slot count and the part [p, q) of the longer range"""
    si, slo, shi, li, llo, lhi = _ordered(ia, ib, row)
    frm, n = int(row[4]), int(row[5])
    out = []
    for base in range(slo, shi, TILE):
        tl = min(TILE, shi - base)
        keep = counted(si, base, base + tl, frm, n)
        if not keep.any():
            out.append(("none", tl, llo, llo))
            continue
        d = si[base:base + tl][keep, 1].astype(np.int64)
        p = _first_ge(li, llo, lhi, d[0])
        q = _first_ge(li, p, lhi, d[-1] + 1)
        out.append(("probe" if (q - p) // LOPSIDED > tl else "stream", tl, p, q))
        llo = q
    return out


# ---- building ranges -------------------------------------------------------------------------------------------------------------
class Buffers:
    """two Edge buffers that grow range by range; add() returns the slot range"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parts = {"a": [], "b": []}
        self.size = {"a": 0, "b": 0}

    def add(self, side, dest, live, junk_hi=N_MAX):
        """a range of len(dest) slots: dest[i] where live[i], else a null with a junk dest"""
        L = len(dest)
        e = np.zeros((L, 3), np.uint32)
        e[:, 0] = 7
        e[:, 1] = self.rng.integers(0, junk_hi, L)  # junk under the nulls
        e[live, 1] = np.asarray(dest, np.int64)[live]
        e[live, 2] = 1 + (np.arange(L)[live] % 5)
        e[~live, 0] = SENT  # null_edge(): src kMax, value 0
        d = e[live, 1].astype(np.int64)
        assert np.all(np.diff(d) > 0), "live dests must ascend strictly"
        lo = self.size[side]
        # one null between ranges, so that no range owes its answer to its neighbour's first slot
        pad = np.array([[SENT, self.rng.integers(0, junk_hi), 0]], np.uint32)
        self.parts[side] += [e, pad]
        self.size[side] += L + 1
        return lo, lo + L

    def arrays(self):
        out = []
        for side in "ab":
            a = np.concatenate(self.parts[side]) if self.parts[side] else np.zeros((0, 3), np.uint32)
            assert len(a) <= BUF_MAX, (side, len(a))
            out.append(np.ascontiguousarray(a))
        return out


def fill_mask(rng, L, kind):
    if kind == "full":
        return np.ones(L, bool)
    if kind == "half":
        return rng.random(L) < 0.5
    if kind == "sparse":
        m = np.zeros(L, bool)
        m[rng.integers(0, 16)::16] = True
        return m
    raise KeyError(kind)


def master(rng, L, kind, stride, first):
    """L slots whose slot s, where live, holds first + stride * s + (0 or 1): every master covers the dests in step with its
    slots, so windows cut around the same dest meet, and two masters agree on a dest with probability 1/2 where both are live"""
    return first + stride * np.arange(L, dtype=np.int64) + rng.integers(0, 2, L), fill_mask(rng, L, kind)


CENTRE = 3 * 4096 + 5  # the dest every window is cut around (the middle of the long masters)
# name, slots, fill, dest stride, first dest
MASTERS = [("D", 3 * 4096 + 5, "full", 2, 0), ("H", 3 * 4096 + 5, "half", 2, 0), ("S", 4200, "sparse", 2, CENTRE - 4200), ("W", 1229, "full", 20, 0),
           ("V", 1536, "half", 16, 0)]


def intersect_cases(seed=20):
    """-> dict(items_a, items_b, rows (k, 6) uint32, tags [set], facts dict): the cases of the three intersecting modes.  A case
    tagged 'lane' is short enough for the one-lane routine as well."""
    B = Buffers(seed)
    rng = B.rng
    rows, tags = [], []

    def case(a, b, frm=0, n=N_MAX, *tg):
        rows.append((a[0], a[1], b[0], b[1], frm, n))
        t = set(tg)
        if max(a[1] - a[0], b[1] - b[0]) <= LANE_MAX:
            t.add("lane")
        tags.append(t)
        return len(rows) - 1

    # -- masters, and windows of every length cut around the same dest --
    base = {}
    for side in "ab":
        for name, L, kind, stride, first in MASTERS:
            dest, live = master(rng, L, kind, stride, first)
            base[side, name] = (B.add(side, dest, live)[0], L, stride, first)

    def window(side, name, L):
        lo, ML, stride, first = base[side, name]
        assert L <= ML
        off = min(max((CENTRE - first) // stride - L // 2, 0), ML - L)
        return lo + off, lo + off + L

    lengths = SHORT + LONG
    for i, la in enumerate(lengths):
        for j, lb in enumerate(lengths):
            fa = [m for m in ("D", "H", "S", "W", "V") if la <= base["a", m][1]]
            fb = [m for m in ("D", "H", "S", "W", "V") if lb <= base["b", m][1]]
            ma, mb = fa[(i + 2 * j) % len(fa)], fb[(3 * i + j) % len(fb)]
            frm, n = [(0, N_MAX), (CENTRE - 40, N_MAX), (0, CENTRE + 40), (CENTRE - 700, CENTRE + 900)][(i + j) % 4]
            case(window("a", ma, la), window("b", mb, lb), frm, n, "grid", f"la={la}", f"lb={lb}")
    # -- the lopsided ratio of isect_wave: longer / 8 > shorter flips between 8 s + 7 and 8 s + 8 --
    for s in (33, 64, 100, 512):
        for lng in (8 * s, 8 * s + 7, 8 * s + 8, 8 * s + 9):
            case(window("a", "D", s), window("b", "D", lng), 0, N_MAX, "ratio", f"ratio s={s}")
            case(window("a", "H", lng), window("b", "D", s), 0, N_MAX, "ratio", f"ratio s={s}")
    # -- the ratio of isect_block against [p, q): a tile that is wide in dests against a dense long range (probed), the same tile
    #    against a range as sparse in dests as itself (streamed), and the 16-stride master that sits at the threshold --
    for L in (65, 129, 1024, 1025):
        for m in ("W", "V"):
            case(window("a", m, L), window("b", "D", 3 * 4096 + 5), 0, N_MAX, "block-ratio")
            case(window("a", "D", 3 * 4096 + 5), window("b", m, L), 0, N_MAX, "block-ratio")
            case(window("a", m, L), window("b", m, min(L + 200, base["b", m][1])), 0, N_MAX, "block-ratio")

    # -- constructed pairs --
    def pair(la, lb, live_a, live_b, lo_dest=1000, gap=3, share=0.6):
        """two ranges whose live dests are drawn from one ascending universe; about `share` of the smaller side's dests are in the other"""
        ka, kb = int(live_a.sum()), int(live_b.sum())
        k = max(ka, kb)
        uni = lo_dest + np.cumsum(rng.integers(1, gap + 1, 2 * k + 2))
        pick_big = np.sort(rng.choice(len(uni), k, replace=False))
        small = min(ka, kb)
        from_big = rng.choice(pick_big, int(small * share), replace=False) if small else np.empty(0, np.int64)
        rest = np.setdiff1d(np.arange(len(uni)), pick_big)
        other = rng.choice(rest, small - len(from_big), replace=False) if small else np.empty(0, np.int64)
        pick_small = np.sort(np.concatenate([from_big, other])).astype(np.int64)
        da, db = np.zeros(la, np.int64), np.zeros(lb, np.int64)
        da[live_a] = uni[pick_big if ka >= kb else pick_small]
        db[live_b] = uni[pick_small if ka >= kb else pick_big]
        return B.add("a", da, live_a), B.add("b", db, live_b)

    def holes(L, runs):
        m = np.ones(L, bool)
        for at, ln in runs:
            m[at:at + ln] = False
        return m

    # gaps: a leading run, a trailing run, runs of 64, 65 and 200 nulls inside a range (either side; both merge-sized and lopsided)
    for la, lb in ((300, 340), (340, 300), (120, 1100), (1100, 120)):
        for name, runs_a, runs_b in (("lead", [(0, 70)], [(0, 3)]), ("trail", [(la - 90, 90)], [(lb - 2, 2)]),
                                     ("run64", [(64, 64)], [(17, 64)]), ("run65", [(30, 65)], [(128, 65)]),
                                     ("run200", [(20, 200)], [(10, 200)])):
            runs_a = [(min(at, la - ln), ln) for at, ln in runs_a if ln < la]
            runs_b = [(min(at, lb - ln), ln) for at, ln in runs_b if ln < lb]
            a, b = pair(la, lb, holes(la, runs_a), holes(lb, runs_b))
            case(a, b, 0, N_MAX, "gap", name)
    # a whole 64-slot step, and a whole 1024-slot tile, of the SHORTER operand without a live slot
    a, b = pair(192, 400, holes(192, [(64, 64)]), np.ones(400, bool))
    case(a, b, 0, N_MAX, "null-step")
    a, b = pair(1700, 192, np.ones(1700, bool), holes(192, [(0, 64), (128, 64)]))
    case(a, b, 0, N_MAX, "null-step")
    a, b = pair(2148, 3000, holes(2148, [(1024, 1024)]), np.ones(3000, bool))
    case(a, b, 0, N_MAX, "null-tile")
    a, b = pair(2300, 1100, np.ones(2300, bool), holes(1100, [(0, 1024)]))
    case(a, b, 0, N_MAX, "null-tile")
    # a whole step / tile where every live dest is filtered out: below `from` (the first one), at or above n (the last one)
    a, b = pair(2200, 3000, np.ones(2200, bool), np.ones(3000, bool))
    da = live_dests(B.parts["a"][-2], 0, 2200)
    case(a, b, int(da[1024]), N_MAX, "filtered-tile", "filtered-step")
    case(a, b, 0, int(da[1023]) + 1, "filtered-tile", "filtered-step")
    case(a, b, int(da[1024]), int(da[2047]) + 1, "filtered-tile", "filtered-step")
    a, b = pair(200, 260, np.ones(200, bool), fill_mask(rng, 260, "half") | (np.arange(260) % 3 == 0))
    da = live_dests(B.parts["a"][-2], 0, 200)
    case(a, b, int(da[64]), N_MAX, "filtered-step")
    case(a, b, 0, int(da[127]) + 1, "filtered-step")

    # -- the merge cursor --
    # a chunk of the longer range that holds matched dests of two consecutive steps of the shorter one
    da = 10 * np.arange(128, dtype=np.int64)  # steps: dests 0 .. 630 | 640 .. 1270
    db = np.concatenate([np.arange(600, 664, 2), 10 * np.arange(67, 164)])  # chunk 0 of b: 600, 602 .. 662, then 670, 680 ...
    a = B.add("a", da, np.ones(128, bool))
    b = B.add("b", db, np.ones(len(db), bool))
    case(a, b, 0, N_MAX, "cursor-holds")
    # a longer-side chunk without live slots between two matches (the chunk is aligned to the cursor's 64-slot stride)
    da = 5 * np.arange(100, dtype=np.int64)
    lb = holes(260, [(60, 140)])  # chunks [64, 128) and [128, 192) of b are empty
    db = np.zeros(260, np.int64)
    db[lb] = 5 * np.arange(int(lb.sum()))
    a = B.add("a", da, np.ones(100, bool))
    b = B.add("b", db, lb)
    case(a, b, 0, N_MAX, "cursor-empty-chunk")
    # a match in the very first and in the very last slot of each operand; nothing but those
    for la, lb in ((50, 70), (129, 200), (1025, 1100), (40, 900), (1300, 150)):
        da = 1000 + 4 * np.arange(la, dtype=np.int64)
        db = 1001 + 4 * np.arange(lb, dtype=np.int64)
        da[0] = db[0] = 900
        da[-1] = db[-1] = 1000 + 4 * max(la, lb) + 50
        a = B.add("a", da, np.ones(la, bool))
        b = B.add("b", db, np.ones(lb, bool))
        case(a, b, 0, N_MAX, "ends")
        case(a, b, 901, int(da[-1]), "ends-filtered")
    # no match at all, dests interleaved
    for la, lb in ((31, 31), (100, 130), (1100, 1300), (64, 2000)):
        a = B.add("a", 2 * np.arange(la, dtype=np.int64) * (lb // la + 1), np.ones(la, bool))
        b = B.add("b", 2 * np.arange(lb, dtype=np.int64) + 1, np.ones(lb, bool))
        case(a, b, 0, N_MAX, "interleaved")
    # identical operands: the same dests in both buffers, gapped alike and gapped differently
    for L in (20, 64, 65, 700, 1100):
        dest = 50 + np.cumsum(rng.integers(1, 4, L))
        la = fill_mask(rng, L, "half")
        a = B.add("a", dest, la)
        b = B.add("b", dest, la)
        case(a, b, 0, N_MAX, "identical")
        k = int(la.sum())  # the same dests packed to the front, nulls behind them
        b2 = B.add("b", np.concatenate([dest[la], np.zeros(L - k, np.int64)]), np.arange(L) < k)
        case(a, b2, 0, N_MAX, "identical")

    # -- filters around a matched dest, and a sentinel inside the range --
    for la, lb in ((30, 28), (90, 100), (1100, 1200), (100, 1000)):
        a, b = pair(la, lb, np.ones(la, bool), np.ones(lb, bool))
        items_a, items_b = B.parts["a"][-2], B.parts["b"][-2]
        c = np.intersect1d(live_dests(items_a, 0, la), live_dests(items_b, 0, lb))
        assert len(c) >= 3
        m = int(c[len(c) // 2])
        for frm in (m - 1, m, m + 1):
            case(a, b, frm, N_MAX, "from-edge", f"from-m={frm - m}")
        for n in (m + 1, m):
            case(a, b, 0, n, "n-edge", f"n-m={n - m}")
        case(a, b, m, m + 1, "from-edge", "n-edge")
    for la, lb in ((25, 30), (100, 120), (1100, 1050)):
        da = 10 + 3 * np.arange(la, dtype=np.int64)
        db = 10 + 3 * np.arange(lb, dtype=np.int64)
        la_live, lb_live = np.arange(la) < la - 4, np.arange(lb) < lb - 6
        da[la - 5] = db[lb - 7] = SENT  # the last live slot of each: a sentinel, nulls behind it
        a = B.add("a", da, la_live)
        b = B.add("b", db, lb_live)
        case(a, b, 0, N_MAX, "sentinel")

    items_a, items_b = B.arrays()
    rows = np.array(rows, np.uint32).reshape(-1, 6)
    assert int(rows[:, 5].max()) <= N_MAX
    facts = assert_intersect_presence(items_a, items_b, rows, tags)
    return dict(items_a=items_a, items_b=items_b, rows=rows, tags=tags, facts=facts)


def assert_intersect_presence(ia, ib, rows, tags):
    """what section 2 of the plan promises, read back from the arrays"""
    f = dict(cases=len(rows), lane=sum("lane" in t for t in tags))
    la, lb = rows[:, 1].astype(np.int64) - rows[:, 0], rows[:, 3].astype(np.int64) - rows[:, 2]
    have = set(zip(la.tolist(), lb.tolist()))
    for x in SHORT + LONG:
        for y in SHORT + LONG:
            assert (x, y) in have, (x, y)
    lane_have = {(int(x), int(y)) for x, y, t in zip(la, lb, tags) if "lane" in t}
    assert all((x, y) in lane_have for x in SHORT for y in SHORT)
    # the shorter operand comes first and second
    assert np.any(la < lb) and np.any(lb < la) and np.any(la == lb)
    forms = [wave_form(ia, ib, r) for r in rows]
    f["wave"] = {k: forms.count(k) for k in ("empty", "merge", "probe")}
    assert all(v >= 20 for v in f["wave"].values()), f
    # both forms of isect_wave on neighbouring lengths, either order of the operands
    near = {}
    for r, form in zip(rows, forms):
        s, l = sorted((int(r[1] - r[0]), int(r[3] - r[2])))
        near.setdefault((s, int(r[1] - r[0]) <= int(r[3] - r[2])), {})[l] = form
    flips = sum(1 for (s, _), d in near.items() for l in d if d[l] == "merge" and d.get(l + 1) == "probe" and l == 8 * s + 7)
    assert flips >= 6, flips
    assert any(d.get(8 * s) == "merge" for (s, _), d in near.items())
    # isect_block: streamed and probed tiles, tiles with nothing staged, the last partial tile, and (q - p) / 8 against the tile on
    # both sides within a few slots of the flip
    kinds = dict(none=0, stream=0, probe=0, partial=0, full=0, multi=0)
    margin = []
    for r in rows:
        tl = block_tiles(ia, ib, r)
        kinds["multi"] += len(tl) > 1
        for kind, t, p, q in tl:
            kinds[kind] += 1
            kinds["partial" if t < TILE else "full"] += 1
            if kind != "none":
                margin.append((q - p) // LOPSIDED - t)
        if len(tl) > 1:
            kinds["last-partial"] = kinds.get("last-partial", 0) + (tl[-1][1] < TILE and tl[-1][0] != "none")
    f["block"] = kinds
    assert min(kinds.values()) >= 5, kinds
    margin = np.array(margin)
    f["block_margin"] = (int(margin[margin <= 0].max()), int(margin[margin > 0].min()))
    assert f["block_margin"][0] >= -2 and f["block_margin"][1] <= 2, f  # (q - p) / 8 within two slots of the tile, either side
    # gaps
    def tagged(t):
        idx = [i for i, tg in enumerate(tags) if t in tg]
        assert idx, t
        return idx

    def null_run(items, lo, hi):
        """longest run of nulls in [lo, hi), the leading and the trailing one"""
        z = np.concatenate([[1], (items[lo:hi, 2] != 0).astype(np.int8), [1]])
        edges = np.nonzero(z)[0]
        runs = np.diff(edges) - 1
        return int(runs.max()), int(runs[0]), int(runs[-1])

    for t, want in (("run64", 64), ("run65", 65), ("run200", 200)):
        assert any(null_run(ia, *rows[i][:2])[0] == want for i in tagged(t)) and any(null_run(ib, *rows[i][2:4])[0] == want for i in tagged(t))
    assert any(null_run(ia, *rows[i][:2])[1] >= 64 for i in tagged("lead")) and any(null_run(ia, *rows[i][:2])[2] >= 64 for i in tagged("trail"))
    fills = []
    for i in tagged("grid"):
        for items, lo, hi in ((ia, rows[i][0], rows[i][1]), (ib, rows[i][2], rows[i][3])):
            if hi - lo >= 1000:
                fills.append(float(np.mean(items[lo:hi, 2] != 0)))
    fills = np.array(fills)
    assert np.any(fills == 1.0) and np.any(np.abs(fills - 0.5) < 0.05) and np.any(np.abs(fills - 1 / 16) < 0.01)
    for i in tagged("null-step"):  # a step of the shorter operand without a live slot, between steps that have some
        si, slo, shi, _, _, _ = _ordered(ia, ib, rows[i])
        live = [bool(np.any(si[b:min(b + STEP, shi), 2] != 0)) for b in range(slo, shi, STEP)]
        assert False in live and True in live
    for i in tagged("null-tile"):
        si, slo, shi, _, _, _ = _ordered(ia, ib, rows[i])
        live = [bool(np.any(si[b:min(b + TILE, shi), 2] != 0)) for b in range(slo, shi, TILE)]
        assert False in live and True in live
    for t, width in (("filtered-step", STEP), ("filtered-tile", TILE)):
        ok = 0
        for i in tagged(t):
            si, slo, shi, _, _, _ = _ordered(ia, ib, rows[i])
            for b in range(slo, shi, width):
                hi = min(b + width, shi)
                ok += bool(np.any(si[b:hi, 2] != 0)) and not counted(si, b, hi, int(rows[i][4]), int(rows[i][5])).any()
        assert ok >= 2, t
    # the merge cursor
    for i in tagged("cursor-holds"):
        assert wave_form(ia, ib, rows[i]) == "merge"
        si, slo, shi, li, llo, lhi = _ordered(ia, ib, rows[i])
        c = matches(ia, ib, rows[i])
        step_of = {int(d): (slo_i // STEP) for slo_i, d in zip(np.nonzero(si[slo:shi, 2] != 0)[0], live_dests(si, slo, shi))}
        chunk_of = {int(d): (s // STEP) for s, d in zip(np.nonzero(li[llo:lhi, 2] != 0)[0], live_dests(li, llo, lhi))}
        per_chunk = {}
        for d in c.tolist():
            per_chunk.setdefault(chunk_of[d], set()).add(step_of[d])
        assert any(len(s) >= 2 for s in per_chunk.values()), per_chunk
    for i in tagged("cursor-empty-chunk"):
        assert wave_form(ia, ib, rows[i]) == "merge"
        _, _, _, li, llo, lhi = _ordered(ia, ib, rows[i])
        c = matches(ia, ib, rows[i])
        empty = [b for b in range(llo, lhi, STEP) if not np.any(li[b:min(b + STEP, lhi), 2] != 0)]
        assert empty and np.intersect1d(c, live_dests(li, llo, empty[0])).size and np.intersect1d(c, live_dests(li, empty[0], lhi)).size
    for i in tagged("ends"):
        c = matches(ia, ib, rows[i])
        assert len(c) == 2
        for items, lo, hi in ((ia, rows[i][0], rows[i][1]), (ib, rows[i][2], rows[i][3])):
            assert items[lo, 2] != 0 and items[hi - 1, 2] != 0 and items[lo, 1] == c[0] and items[hi - 1, 1] == c[1]
    for i in tagged("ends-filtered"):
        assert len(matches(ia, ib, rows[i])) == 0
    for i in tagged("interleaved"):
        assert len(matches(ia, ib, rows[i])) == 0
        a, b = live_dests(ia, *rows[i][:2]), live_dests(ib, *rows[i][2:4])
        assert a.min() < b.max() and b.min() < a.max()
    for i in tagged("identical"):
        assert np.array_equal(live_dests(ia, *rows[i][:2]), live_dests(ib, *rows[i][2:4]))
    # filters
    by = {}
    for i in tagged("from-edge") + tagged("n-edge"):
        by.setdefault(tuple(rows[i][:4].tolist()), []).append(i)
    for key, idx in by.items():
        full = matches(ia, ib, (*key, 0, N_MAX))
        froms = {int(rows[i][4]) for i in idx if "from-edge" in tags[i]}
        ns = {int(rows[i][5]) for i in idx if "n-edge" in tags[i]}
        assert any({m - 1, m, m + 1} <= froms and {m, m + 1} <= ns for m in full.tolist()), key
    for i in tagged("sentinel"):
        a, b = live_dests(ia, *rows[i][:2]), live_dests(ib, *rows[i][2:4])
        assert a[-1] == SENT and b[-1] == SENT and SENT not in matches(ia, ib, rows[i]) and len(matches(ia, ib, rows[i])) > 0
    f["matches"] = int(sum(len(matches(ia, ib, r)) for r in rows))
    assert f["matches"] > 10 * len(rows)
    return f


def search_cases(seed=30):
    """-> dict(items, lb_rows, probe_rows, facts): the cases of `lower_bound` and `probe` over one buffer of 2^16 slots, the ranges
    being windows of it"""
    rng = np.random.default_rng(seed)
    N = BUF_MAX
    e = np.zeros((N, 3), np.uint32)
    e[:, 0] = SENT
    live = rng.random(N) < 0.5
    dest = 100 + 3 * np.arange(N, dtype=np.int64) + rng.integers(0, 2, N)  # (live dests differ by 2 at least: a key fits between)
    ranges = {}
    ranges["whole"] = (0, N)
    ranges["r64"] = (300, 364)
    ranges["r65"] = (1000, 1065)
    ranges["r4097"] = (2000, 2000 + 4097)
    # every one of the 64 sample positions of [10000, 10000 + 4097) on a null: step = ceil(4097 / 64) = 65
    ranges["unsampled"] = (10000, 10000 + 4097)
    live[10000:10000 + 4097] = True
    live[10000 + 65 * np.arange(64)] = False
    ranges["dense"] = (20000, 20000 + 9000)
    live[20000:29000] = True
    ranges["no-live"] = (30000, 30300)
    live[30000:30300] = False
    ranges["empty"] = (31000, 31000)
    ranges["one"] = (31001, 31002)
    live[31001] = True
    ranges["one-null"] = (31003, 31004)
    live[31003] = False
    # live slots only in the first eighth: a midpoint's walk to the right meets no live slot before hi
    ranges["head-only"] = (40000, 40800)
    live[40100:40800] = False
    live[40000:40100] |= np.arange(100) % 2 == 0
    ranges["head-only-65"] = (42000, 42065)
    live[42000:42065] = False
    live[42000:42005] = True
    ranges["sparse"] = (45000, 45000 + 5000)
    live[45000:50000] = False
    live[45000 + 37:50000:97] = True
    e[:, 1] = rng.integers(0, 3 * N, N)  # junk under the nulls: dests that lie inside the range's own span
    e[live, 1] = dest[live]
    e[live, 2] = 1 + np.arange(N)[live] % 3
    e[live, 0] = 3
    rows_lb, rows_pr, kinds = [], [], {}
    for name, (lo, hi) in ranges.items():
        d = live_dests(e, lo, hi)
        keys = {0: "below", 99: "below", 0xFFFFFFFE: "above"}
        if len(d):
            keys.update({int(d[0]) - 1: "below", int(d[-1]) + 1: "above", int(d[-1]) + 1000: "above"})
            pick = np.unique(np.concatenate([[0, len(d) - 1, len(d) // 2], rng.integers(0, len(d), 12)]))
            for i in pick.tolist():
                keys[int(d[i])] = "equal"
                if i + 1 < len(d) and d[i + 1] - d[i] >= 2:
                    keys[int(d[i]) + 1] = "between"
        r = e[lo:hi]  # junk dests of nulls inside the range: keys that only a null holds
        for k in r[(r[:, 2] == 0), 1][:4].tolist():
            if k not in d:
                keys[int(k)] = "junk"
        for k, kind in keys.items():
            rows_lb.append((0, 0, lo, hi, k, 0))
            rows_pr.append((0, 0, lo, hi, k, 0))
            kinds[name, kind] = kinds.get((name, kind), 0) + 1
    rows_lb = np.array(rows_lb, np.uint32)
    rows_pr = np.array(rows_pr, np.uint32)
    # presence
    for name in ("whole", "r64", "r65", "r4097", "unsampled", "dense", "sparse", "head-only"):
        for kind in ("below", "above", "equal", "between"):
            assert kinds.get((name, kind), 0) >= 1, (name, kind)
    lo, hi = ranges["unsampled"]
    step = (hi - lo + 63) // 64
    assert np.all(e[lo + step * np.arange(64), 2] == 0) and lo + step * 63 < hi and np.count_nonzero(e[lo:hi, 2]) == hi - lo - 64
    assert not np.any(e[slice(*ranges["no-live"]), 2]) and ranges["whole"] == (0, 1 << 16)
    assert sorted(ranges[k][1] - ranges[k][0] for k in ("r64", "r65", "r4097", "whole")) == [64, 65, 4097, 1 << 16]
    for name in ("head-only", "head-only-65"):
        lo, hi = ranges[name]
        mid = lo + (hi - lo) // 2
        assert not np.any(e[mid:hi, 2]) and np.any(e[lo:mid, 2])
    return dict(items=np.ascontiguousarray(e), lb_rows=rows_lb, probe_rows=rows_pr, ranges=ranges,
                facts=dict(lower_bound=len(rows_lb), probe=len(rows_pr)))


def swapped(rows):
    """the same cases with the operands exchanged (run with items_a and items_b exchanged as well)"""
    return np.ascontiguousarray(rows[:, [2, 3, 0, 1, 4, 5]])
