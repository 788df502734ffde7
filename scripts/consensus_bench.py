#!/usr/bin/env python3
"""The distinct splits of a bootstrap on the device: andi_hip_nj_splits beside the plain-Python model.

Trees: one additive tree per size (tests/nj_model.py, seed = n) and --count copies of its distances with seeded symmetric
noise of 1 % each, joined by one andi_hip_nj_batch call -- replicates of one n, as scripts/support_bench.py makes them.
Timed: the wall time around the andi_hip_nj_splits call, a host clock, with the call's copies in and out (the call ends
in a synchronise); the least of --reps runs after one warm-up.  model_s: tests/consensus_model.splits on the same records,
once; the two results must be equal.  consensus_s: andi_hip_consensus and the formatter on the host, once.  Writes one
JSON object to --out (default: profiles/consensus_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[29, 300, 1000])
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD, if there is one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import consensus_model
    import nj_model

    commit = args.commit
    if not commit:
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True)
        commit = p.stdout.decode().strip() if p.returncode == 0 else "unknown"
    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n)
        rng = np.random.default_rng(n)
        Ds = np.empty((args.count, n, n))
        for k in range(args.count):
            E = np.triu(rng.uniform(-0.01, 0.01, (n, n)), 1)
            Ds[k] = D * (1.0 + E + E.T)
        J, bad = lib.nj_batch(ctx, Ds)
        assert (bad == -1).all()
        lib.nj_splits(ctx, J)  # warm-up
        runs, got = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = lib.nj_splits(ctx, J)
            runs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = consensus_model.splits(J)
        model_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        nodes = lib.consensus(J, *got)
        text = lib.newick_consensus(nodes, ["t%d" % i for i in range(n)])
        consensus_s = time.perf_counter() - t0
        row = {"n": n, "count": args.count, "splits_s": min(runs), "splits_runs_s": runs, "model_s": model_s,
               "model_over_splits": model_s / min(runs), "consensus_s": consensus_s, "distinct_splits": int(len(got[1])),
               "majority_splits": int(len(nodes) - n - 1), "newick_bytes": len(text),
               "splits_equal_model": all(a.tobytes() == b.tobytes() for a, b in zip(got, want))}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_nj_splits (wall time with copies, least of the warm runs) beside tests/consensus_model.splits; "
                   "additive trees, replicates with 1% noise joined by andi_hip_nj_batch", "commit": commit, "rows": rows}
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if not all(r["splits_equal_model"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
