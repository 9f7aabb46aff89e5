#!/usr/bin/env python3
"""Generate tests/golden/ref_digests.json from the UNMODIFIED reference (oracle/_ref/libref_pcsr.so): the case
definitions of tests/test_oracle_vs_ref.py driven through the reference instead of the oracle; and
tests/golden/ref_cli_protocol.json: the reference's own CLI (oracle/_ref/ref_cli) on tests/test_cpp_host.py's protocol cases.

Run where the reference tree exists (`make -C oracle` builds oracle/_ref from it):
    make -C oracle && python tests/golden/make_ref_digests.py
Only digests of expected outputs are stored; no reference source text.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import load_streams  # noqa: E402
from oracle_lib import RefPCSR, have_ref  # noqa: E402
import test_cpp_host as h  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402


def main():
    if not have_ref():
        raise SystemExit("oracle/_ref/libref_pcsr.so missing: run `make -C oracle` where the reference tree exists")
    st = load_streams()
    make = lambda n, lock: RefPCSR(n, lock_search=lock)  # noqa: E731
    out = {key: fn(make) for key, fn in t.cases(st).items()}
    r, starts, vals = t.consumer_graph(make, st)
    out["consumers_rmat14"] = {**{f"bfs_{s}": t._sha(r.bfs(s)) for s in starts}, "pagerank": t._sha(r.pagerank(vals))}
    r.close()
    rec = {"what": "tests/test_oracle_vs_ref.py cases run through the unmodified reference (oracle/_ref/libref_pcsr.so, one "
                   "thread): geometry, tests/helpers.digest of edges[] / nodes[], sha256 of sampled neighbourhoods and of the "
                   "reference's bfs / pagerank template results",
           "generator": "tests/golden/make_ref_digests.py", **dict(sorted(out.items()))}
    json.dump(rec, open(t.REF_DIGESTS, "w"), indent=1)
    print(f"{len(out)} cases written to {os.path.relpath(t.REF_DIGESTS, ROOT)}")
    # the reference's own CLI (oracle/_ref/ref_cli) on the stdout-protocol cases of tests/test_cpp_host.py
    cli = {}
    for flags in h.CLI_CASES:
        with tempfile.TemporaryDirectory() as d:
            keep, elapsed, last_edges = h.cli_protocol(h.REF_CLI, d, flags)
        cli[" ".join(flags)] = {"keep": keep, "elapsed": elapsed, "last_edges": last_edges}
    rec = {"what": "filtered stdout of the unmodified reference CLI (oracle/_ref/ref_cli) on the protocol cases of "
                   "tests/test_cpp_host.py", "generator": "tests/golden/make_ref_digests.py", **cli}
    json.dump(rec, open(h.REF_CLI_RECORD, "w"), indent=1)
    print(f"{len(cli)} CLI cases written to {os.path.relpath(h.REF_CLI_RECORD, ROOT)}")


if __name__ == "__main__":
    main()
