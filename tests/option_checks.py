"""What ppcsr_set_option answers, key by key (TEST INFRASTRUCTURE ONLY): shared by tests/test_sim_options.py (emulator) and
tests/test_gpu_options.py (device).  The keys that launch kernels ("marker", "test_block_rebalance") are left out."""
import numpy as np

from oracle_lib import Oracle

OK, EINVAL = 0, 1
N = 200  # vertices of the engines (the smallest the emulator tests use)

# keys that refuse values: key -> (accepted: every bound among them, refused: the values just outside among them)
IN_RANGE = {
    "max_horizon": ([1, 1 << 20], [0, (1 << 20) + 1, -1]),
    "opt_horizon": ([1, 1 << 20], [0, (1 << 20) + 1, -1]),
    "start_horizon": ([1, 1 << 20], [0, (1 << 20) + 1, -1]),
    "resident_waves": ([0, 1 << 20], [-1, (1 << 20) + 1]),
    "min_horizon": ([1, 1 << 40], [0, -1]),
    "init_horizon": ([1, 1 << 40], [0, -1]),
    "mode": ([0, 1], [-1, 2]),
    "epoch_ops": ([1, 1 << 24], [0, (1 << 24) + 1, -1]),
    "region_slots": ([1, 2, 1 << 20], [0, -1, 3, 6, -4]),
    "region_wide": ([1, 2, 1 << 20], [0, -1, 3, 6, -4]),
    "region_rare": ([0, 1, 16384], [-1, 3, 6, -4]),
    "big_window": ([64, 128, 1 << 20, 1 << 30], [32, 63, 65, 96, 0, -64]),
    "rb_inplace_lists": ([1, 2, 4, 8], [0, 3, 5, 6, 7, 9, 16, -1, 64, 1 << 40]),
    "query_lookup_stage": ([1, 1 << 32], [0, (1 << 32) + 1, -1]),
    "query_gather_rows": ([1, 1 << 32], [0, (1 << 32) + 1, -1]),
    "query_gather_chunks": ([1, 1 << 32], [0, (1 << 32) + 1, -1]),
    "query_gather_stage": ([1, 1 << 32], [0, (1 << 32) + 1, -1]),
    "snap_grid": ([1, 4096], [0, 4097, -1]),
    "rounds_per_sync": ([1, 4096], [0, 4097, -1]),
}
# keys that take any value (they clamp it, or read it as a flag)
ANY_VALUE = ["epoch_short", "epoch_adapt", "epoch_grow_after", "region_calm", "region_rare_calm", "region_rare_cpr", "region_rare_dist",
             "scatter_blocks", "search_narrow", "small_batch", "excl_in_wave", "big_min", "big_grid", "rb_min_tiles", "rb_inplace_min",
             "rb_bench_upper", "rb_prefetch", "msbfs_look", "scatter_variant", "adaptive", "soft_barrier", "defer_barrier",
             "rb_defer_table", "dbg_repeat", "diag",
             # (not plain stores, but as tolerant)
             "rb_tile", "rb_inplace_cpw", "check_lanes", "snap_count", "profile"]


def _set(e, key, value):
    return e.L.ppcsr_set_option(e.h, key.encode(), int(value))


def return_codes(make):
    e = make(N)
    for key, (good, bad) in IN_RANGE.items():
        for v in good:
            assert _set(e, key, v) == OK, (key, v)
        for v in bad:
            assert _set(e, key, v) == EINVAL, (key, v)
    for key in ANY_VALUE:
        for v in (-1, 0, 1 << 40):
            assert _set(e, key, v) == OK, (key, v)
    for key in ("", "no_such_option", "Mode", "mode ", "epoch"):
        assert _set(e, key, 1) == EINVAL, key
    e.close()


def batch_after(make, opts, streams):
    """an engine created afterwards (no odd option in force) still applies a batch as the oracle does"""
    ops = streams.random_stream(N, 1000, seed=1)
    e, o = make(N), Oracle(N)
    for k, v in opts.items():
        e.set_option(k, v)
    e.apply(ops)
    o.apply(ops)
    assert e.geometry() == o.geometry()
    ei, en = e.state()
    oi, on = o.state()
    np.testing.assert_array_equal(en, on)
    np.testing.assert_array_equal(ei, oi)
    assert e.check_invariants() == 0
    e.close()
