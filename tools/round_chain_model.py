#!/usr/bin/env python3
"""Host model of the speculative rounds' COUNT on config #2 (1 M RMAT inserts on the 10 M-edge RMAT core of scale 20): how many
rounds a batch needs when duplicate overwrites are ordered per LEAF (one per leaf and round: the rule until the per-slot table) and
per SLOT (a duplicate waits only for an earlier pending duplicate of the same key, or an earlier pending strong writer of its leaf).

usage: python tools/round_chain_model.py [seeds=2,12,22,32] [widths=21504,28672,35840,43008] [core_seed=1] [scale=20]
                                          [core=10000000] [batch=1000000]
needs numpy and parallel-packed-csr_amd/streams.py only; runs on the CPU (about a minute per batch at the defaults).

What is modelled: a round plans the whole carry list and then fresh updates up to the width (fixed: no ramp from one chip-full);
an update passes when no earlier planned update writes its leaf (and, for an insert, no earlier planned duplicate sits in it);
a passing update commits unless an earlier planned update of its 1024-slot region did not pass.  Positions are estimates: the slot
of a key is its rank in the sorted core (sentinels counted) divided by the density, leaves hold 32 slots, and commits move nothing.
Windows, slides, read leaves, sentinels and the growth marks are not modelled: against the engine the model overstates the
per-leaf rule's rounds by about 10 % (52 - 71 against 55.8 measured per step) and matches the per-slot rule's within a round."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_streams():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ppcsr_streams", os.path.join(HERE, "..", "parallel-packed-csr_amd", "streams.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def keys_of(s, d):
    return (np.asarray(s, np.uint64) << np.uint64(32)) | np.asarray(d, np.uint64)


class Batch:
    def __init__(self, core_keys, n, N, s, d):
        k = keys_of(s, d)
        pos = np.searchsorted(core_keys, k)
        self.in_core = core_keys[np.minimum(pos, len(core_keys) - 1)] == k
        density = (len(core_keys) + n) / N
        slot = ((pos + np.asarray(s, np.int64) + 1) / density).astype(np.int64)
        self.leaf, self.region = slot >> 5, slot >> 10
        _, first, self.key_id = np.unique(k, return_index=True, return_inverse=True)
        self.first = first[self.key_id]  # stream index of the first update of this key
        self.m = len(k)
        # heaviest leaf / key (duplicates of the core only: what chains under the per-leaf rule)
        dl = self.leaf[self.in_core]
        self.heaviest_leaf = int(np.bincount(dl - dl.min()).max()) if len(dl) else 0
        self.heaviest_key = int(np.bincount(self.key_id[self.in_core]).max()) if len(dl) else 0

    def rounds(self, width, per_slot):
        """-> (rounds, planned updates / updates)"""
        committed = np.zeros(self.m, bool)
        carry = np.zeros(0, np.int64)
        nf, rounds, planned = 0, 0, 0
        big = np.int64(1) << 62
        while nf < self.m or len(carry):
            room = max(0, width - len(carry))
            fresh = np.arange(nf, min(self.m, nf + room), dtype=np.int64)
            nf += len(fresh)
            idx = np.sort(np.concatenate([carry, fresh]))
            rounds += 1
            planned += len(idx)
            leaf, region, kid = self.leaf[idx], self.region[idx], self.key_id[idx]
            # an add of a key that is in the core, or whose first add in this batch has been committed, is a duplicate
            dup = self.in_core[idx] | ((self.first[idx] != idx) & committed[self.first[idx]])
            ul, li = np.unique(leaf, return_inverse=True)
            min_strong = np.full(len(ul), big)
            min_dup = np.full(len(ul), big)
            np.minimum.at(min_strong, li[~dup], idx[~dup])
            np.minimum.at(min_dup, li[dup], idx[dup])
            if per_slot:
                uk, ki = np.unique(kid, return_inverse=True)
                min_key = np.full(len(uk), big)
                np.minimum.at(min_key, ki[dup], idx[dup])
                dup_first = min_key[ki] == idx
            else:
                dup_first = min_dup[li] == idx
            ok = np.where(dup, dup_first & ~(min_strong[li] < idx), (min_strong[li] == idx) & ~(min_dup[li] < idx))
            ur, ri = np.unique(region, return_inverse=True)
            min_fail = np.full(len(ur), big)
            np.minimum.at(min_fail, ri[~ok], idx[~ok])
            commit = ok & ~(min_fail[ri] < idx)
            committed[idx[commit]] = True
            carry = idx[~commit]
        return rounds, planned / self.m


def main():
    opt = dict(seeds="2,12,22,32", widths="21504,28672,35840,43008", core_seed="1", scale="20", core="10000000", batch="1000000")
    for kv in sys.argv[1:]:
        k, v = kv.split("=")
        assert k in opt, f"unknown option {k}"
        opt[k] = v
    st = load_streams()
    scale, n = int(opt["scale"]), 1 << int(opt["scale"])
    cs, cd = st.rmat_edges(scale, int(opt["core"]), seed=int(opt["core_seed"]))
    core_keys = np.unique(keys_of(cs, cd))
    N = 64
    while (len(core_keys) + n) / N > 0.75:  # (the array doubles well before that; close enough for an estimate of positions)
        N *= 2
    print(f"core: {len(core_keys)} distinct edges of {len(cs)}, n = {n}, N = {N} slots, density {(len(core_keys) + n) / N:.3f}")
    widths = [int(w) for w in opt["widths"].split(",")]
    for seed in (int(x) for x in opt["seeds"].split(",")):
        s, d = st.rmat_edges(scale, int(opt["batch"]), seed=seed)
        b = Batch(core_keys, n, N, s, d)
        print(f"batch seed {seed}: {int(b.in_core.sum())} duplicates of the core; heaviest leaf {b.heaviest_leaf} duplicates, heaviest key {b.heaviest_key}")
        for w in widths:
            (r0, f0), (r1, f1) = b.rounds(w, False), b.rounds(w, True)
            print(f"  width {w:6d}: per leaf {r0:3d} rounds, re-plan {f0:.3f} | per slot {r1:3d} rounds, re-plan {f1:.3f}", flush=True)


if __name__ == "__main__":
    main()
