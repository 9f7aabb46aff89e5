"""CPU: the host policies of the speculative scheduler (csrc/pma_epoch_policy.h) driven directly, without a batch: a wrong min
or max in them changes round counts and speed, never parity, so no batch test sees it.  Every expected value is worked out by
hand from the rules with the default knobs (epoch_ops 2^20, epoch_short 16384, epoch_grow_after 2, epoch_adapt 8, region_slots
1024, region_wide 4096, region_calm 8, region_rare 16384 x 8 at a distance >= 65536 and >= 1536 commits per round)."""
import ctypes
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "hostsim")
CSRC = os.path.join(ROOT, "parallel-packed-csr_amd", "csrc")
HOST_SO = os.path.join(SIM_DIR, "libpolicy_host.so")
c_u64, c_u32 = ctypes.c_uint64, ctypes.c_uint32


@functools.lru_cache(None)
def host_lib():
    src = os.path.join(SIM_DIR, "policy_host.cpp")
    deps = [src, os.path.join(CSRC, "pma_epoch_policy.h")]
    if not os.path.exists(HOST_SO) or os.path.getmtime(HOST_SO) < max(os.path.getmtime(d) for d in deps):
        # (the header alone, with plain g++: it must not need the runtime or the kernels; fp64 as the library: no contraction)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fvisibility=hidden",
                        "-fvisibility-inlines-hidden", "-fPIC", "-shared", "-I" + CSRC, src, "-o", HOST_SO], check=True)
    L = ctypes.CDLL(HOST_SO)
    L.policy_new.restype = ctypes.c_void_p
    L.policy_free.argtypes = [ctypes.c_void_p]
    L.policy_set.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_u32]
    L.policy_set_since_rollback.argtypes = [ctypes.c_void_p, c_u64]
    L.policy_begin_batch.argtypes = [ctypes.c_void_p]
    L.policy_region_shift.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.policy_after_rollback.argtypes = [ctypes.c_void_p]
    L.policy_after_clean_epoch.argtypes = [ctypes.c_void_p, c_u64, c_u64, c_u64]
    L.policy_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.policy_chunk_grid.argtypes = [c_u32, c_u32, c_u64, c_u64]
    L.policy_chunk_grid.restype = c_u32
    L.policy_chunk_rounds.argtypes = [c_u32, c_u64, c_u32, c_u32]
    L.policy_chunk_rounds.restype = c_u32
    L.policy_check_choice.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.policy_big_choice.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return L


class Policy:
    """an EpochPolicy with the default knobs"""

    def __init__(self, **knobs):
        self.L = host_lib()
        self.p = self.L.policy_new()
        for k, v in knobs.items():
            assert self.L.policy_set(self.p, k.encode(), v) == 1, k

    def __del__(self):
        self.L.policy_free(self.p)

    def begin_batch(self):
        self.L.policy_begin_batch(self.p)

    def region_shift(self, logN):
        return self.L.policy_region_shift(self.p, logN)

    def rollback(self, since_rollback=None):
        if since_rollback is not None:
            self.L.policy_set_since_rollback(self.p, since_rollback)
        self.L.policy_after_rollback(self.p)

    def clean(self, updates, committed, rounds):
        self.L.policy_after_clean_epoch(self.p, updates, committed, rounds)

    def state(self):
        u, d = (c_u64 * 8)(), (ctypes.c_double * 2)()
        self.L.policy_state(self.p, u, d)
        names = ("epoch", "epoch_clean", "grow_eff", "region_eff", "region_clean", "since_rollback", "span", "rare_on")
        s = dict(zip(names, (int(x) for x in u)))
        s["rb_dist"], s["cpr_mean"] = d[0], d[1]
        return s


@pytest.mark.parametrize("region_eff,shift", [(1024, 6), (4096, 8), (16384, 10)])
def test_region_shift(region_eff, shift):
    p = Policy(region_eff=region_eff)
    assert p.region_shift(20) == shift


def test_rollbacks_shorten_the_epoch_and_widen_the_regions():
    """sequence A: commits per round below the rare threshold"""
    p = Policy()
    p.begin_batch()
    p.region_shift(20)
    s = p.state()
    assert (s["epoch"], s["region_eff"]) == (1048576, 1024)
    p.rollback(since_rollback=0)  # the first one: the distance starts at 64 x epoch_short
    s = p.state()
    assert s["rb_dist"] == 1048576.0
    assert (s["epoch"], s["grow_eff"], s["region_eff"], s["span"], s["rare_on"]) == (16384, 2, 4096, 0, 0)
    p.clean(16384, 16384, 16)
    assert p.state()["epoch"] == 16384
    p.clean(16384, 16384, 16)
    s = p.state()
    assert s["cpr_mean"] == 1024.0
    assert (s["epoch"], s["since_rollback"]) == (32768, 32768)
    p.rollback()  # since_rollback = 32768: 0.25 x 1048576 + 0.75 x 32768
    s = p.state()
    assert s["rb_dist"] == 286720.0
    assert (s["epoch"], s["grow_eff"], s["since_rollback"]) == (16384, 2, 0)
    p.rollback()  # at once: 0.25 x 286720; an eighth of it is 8960: the epoch is 8192 and doubles after four clean ones
    s = p.state()
    assert s["rb_dist"] == 71680.0
    assert (s["epoch"], s["grow_eff"], s["region_eff"]) == (8192, 4, 4096)
    for i in range(1, 9):
        p.clean(8192, 8192, 8)
        s = p.state()
        assert s["epoch"] == (8192 if i < 4 else 16384 if i < 8 else 32768), i
        assert s["region_eff"] == (4096 if i < 8 else 1024), i


def test_rare_rollbacks_keep_the_regions_wide_for_a_span_of_updates():
    """sequence B: the rare-rollback rule"""
    p = Policy()
    p.begin_batch()
    p.region_shift(20)
    p.clean(1048576, 1048576, 128)
    assert p.state()["cpr_mean"] == 8192.0
    p.rollback()
    s = p.state()
    assert s["rb_dist"] == 1048576.0
    assert (s["region_eff"], s["span"], s["rare_on"]) == (16384, 8388608, 1)
    for _ in range(8):
        p.clean(16384, 16384, 2)
    s = p.state()
    assert (s["region_eff"], s["rare_on"], s["since_rollback"]) == (16384, 1, 131072)
    # ... not by the count of clean epochs: by the updates committed since the rollback, at the first epoch that reaches the span
    p.L.policy_set_since_rollback(p.p, 8388608 - 16384 - 1)
    p.clean(16384, 16384, 2)
    s = p.state()
    assert (s["region_eff"], s["since_rollback"]) == (16384, 8388607)
    p.clean(1, 1, 1)
    s = p.state()
    assert (s["region_eff"], s["span"], s["rare_on"], s["since_rollback"]) == (1024, 0, 0, 8388608)


def test_rare_rule_needs_epoch_adapt():
    p = Policy(epoch_adapt=0)
    p.begin_batch()
    p.region_shift(20)
    p.clean(1048576, 1048576, 128)
    p.rollback()
    s = p.state()
    assert (s["region_eff"], s["span"], s["rare_on"], s["epoch"]) == (4096, 0, 0, 16384)


@pytest.mark.parametrize("width,pending,carry,grid", [(0, 10**6, 0, 21504), (100, 10**6, 0, 1024), (7168, 300, 0, 512),
                                                      (100, 10**6, 3000, 3072)])
def test_chunk_grid(width, pending, carry, grid):
    assert host_lib().policy_chunk_grid(21504, width, pending, carry) == grid


def test_chunk_rounds():
    """as many as rounds_per_sync while the epoch needs them; at the tail pending / (0.85 x commits per round) + 2, where an epoch
    opens on 0.9 x min(width, updates) commits per round; at most 8 for the chunks after an exclusive update"""
    L = host_lib()
    assert L.policy_chunk_rounds(7168, 10**6, 32, 0) == 32   # 10^6 / (0.85 x 6451.2) + 2 = 184
    assert L.policy_chunk_rounds(7168, 10**6, 32, 4) == 8
    assert L.policy_chunk_rounds(7168, 300, 32, 0) == 3      # 300 / (0.85 x 270) + 2 = 3.3
    assert L.policy_chunk_rounds(7168, 300, 32, 4) == 3
    assert L.policy_chunk_rounds(64, 1, 32, 0) == 3          # (never less than a commit per round: 1 / 1 + 2)
    assert L.policy_chunk_rounds(7168, 10**6, 2, 0) == 2


def _check_choice(chunks):
    pl, lg = (c_u64 * len(chunks))(*[c[0] for c in chunks]), (c_u64 * len(chunks))(*[c[1] for c in chunks])
    out = (ctypes.c_int * len(chunks))()
    host_lib().policy_check_choice(pl, lg, len(chunks), out)
    return list(out)


def test_check_choice():
    assert _check_choice([(1024, 17)]) == [0]   # more than 1 in 64 of at least 1024 planned: a wave per update
    assert _check_choice([(1024, 16)]) == [1]
    assert _check_choice([(1023, 100)]) == [1]
    # the counters are running totals: each chunk is judged on its own share
    assert _check_choice([(4096, 0), (1024, 17)]) == [1, 0]
    # from the wave kernel the 24th chunk goes back to the lanes, whatever it saw
    assert _check_choice([(1024, 17)] + [(1024, 1024)] * 24) == [0] * 24 + [1]


def test_big_choice():
    """o_big stays in while the running mean (halved every chunk) of queued windows per round is at least 1 / 12"""
    jobs, rounds = [3, 6, 0, 0, 32], [32, 32, 32, 0, 32]
    out = (ctypes.c_int * 5)()
    host_lib().policy_big_choice((c_u64 * 5)(*jobs), (c_u64 * 5)(*rounds), 5, out)
    # means: 3/64 = 0.047; 0.023 + 6/64 = 0.117; 0.059; unchanged by a chunk without rounds; 0.029 + 0.5 = 0.529
    assert list(out) == [0, 1, 0, 0, 1]
