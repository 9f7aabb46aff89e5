"""CPU: the definition of the draws alone (include/ppcsr.h, restated in tests/sampling_model.py) — the generator spreads
r = mulhi(x(seed, i, j), W) evenly over [0, W), whichever of i and j varies, and weights come out in their shares.  Deterministic:
the worst bin measured for these seeds and sizes lies 4.31 sigma from uniform; the bound is 6 sigma."""
import numpy as np
import pytest

from sampling_model import draw_x, mulhi, mulhi_int, sm

SEEDS = [0, 1, 12345, 1 << 63]
SIZES = [2, 3, 7, 64, 65, 1000]
DRAWS = 70000


def index_sets():
    a = np.arange(DRAWS, dtype=np.uint64)
    return {"i": (a, np.zeros(DRAWS, np.uint64)), "j": (np.full(DRAWS, 5, np.uint64), a), "both": (a // np.uint64(250), a % np.uint64(250))}


def test_mulhi_by_halves_is_the_128_bit_product():
    edge = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63), (1 << 64) - 1, 0x9E3779B97F4A7C15]
    a = np.array([x for x in edge for _ in edge], np.uint64)
    b = np.array([y for _ in edge for y in edge], np.uint64)
    got = mulhi(a, b)
    for x, y, g in zip(a, b, got):
        assert int(g) == mulhi_int(x, y), (int(x), int(y))


def test_generator_is_splitmix():
    """sm against Python ints, and x = sm(sm(sm(seed) + i) + j)"""
    def sm_int(z):
        z = (z + 0x9E3779B97F4A7C15) % (1 << 64)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
        return z ^ (z >> 31)
    for z in (0, 1, (1 << 64) - 1, 1 << 63, 12345):
        assert int(sm(np.array([z], np.uint64))[0]) == sm_int(z)
    for seed, i, j in ((0, 0, 0), (1 << 63, 7, 9), (12345, (1 << 40) + 3, 1 << 33)):
        want = sm_int((sm_int((sm_int(seed) + i) % (1 << 64)) + j) % (1 << 64))
        assert int(draw_x(seed, np.array([i], np.uint64), np.array([j], np.uint64))[0]) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_are_uniform_within_six_sigma(seed):
    worst = 0.0
    for which, (i, j) in index_sets().items():
        x = draw_x(seed, i, j)
        for W in SIZES:
            r = mulhi(x, np.full(DRAWS, W, np.uint64))
            assert r.max() < W
            cnt = np.bincount(r.astype(np.int64), minlength=W)
            p = 1.0 / W
            dev = np.abs(cnt - DRAWS * p).max() / np.sqrt(DRAWS * p * (1 - p))
            worst = max(worst, dev)
            assert dev < 6.0, (seed, which, W, dev)
    print(f"seed {seed}: worst bin {worst:.2f} sigma")


@pytest.mark.parametrize("seed", SEEDS)
def test_weights_come_out_in_their_shares(seed):
    """weights 1 : 2 : 3 : 4 — the pick is the first entry whose inclusive cumulative weight exceeds r"""
    cum = np.array([1, 3, 6, 10], np.uint64)
    for which, (i, j) in index_sets().items():
        r = mulhi(draw_x(seed, i, j), np.full(DRAWS, 10, np.uint64))
        pick = np.searchsorted(cum, r, side="right")
        cnt = np.bincount(pick, minlength=4)
        for e, w in enumerate((1, 2, 3, 4)):
            p = w / 10.0
            dev = abs(cnt[e] - DRAWS * p) / np.sqrt(DRAWS * p * (1 - p))
            assert dev < 6.0, (seed, which, e, cnt.tolist())
