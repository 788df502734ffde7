#!/usr/bin/env python3
"""Bootstrap trees: one andi_hip_bootstrap_nj call beside the three calls it replaces.

Counts: --length aligned positions per direction of every pair of n genomes at the tips of an additive tree
(tests/nj_model.py, seed = n; the tree's distances scaled so that the largest is --dmax), mismatches binomial, spread
evenly over the twelve cells -- a matrix M as a scan leaves it.  Timed, for `count` replicates of M, model JC:
  one   andi_hip_bootstrap_nj (D == NULL): draw, estimate and join on the device;
  three andi_hip_bootstrap -> andi_hip_distances per replicate -> andi_hip_nj_batch, the path of the command line before
        --trees-only, with the replicates as models on both sides and as doubles on the host.
Wall time on a host clock with every copy the calls make, the least of --reps runs after one warm-up.  host_bytes: what
the caller must hold besides M -- the records and bad words for `one`; for `three` also the replicates' models and
doubles.  The trees of the two paths are compared: they may differ where the portable logarithm and libm's round a
distance differently AND that decides a join (trees_equal counts the replicates with identical records; their
topologies are not compared here).  Writes one JSON object to --out (default: profiles/boot_trees_bench.json).
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


def counts(n, length, dmax, seed):
    import nj_model
    D, _, _ = nj_model.additive_tree(n, seed=seed)
    D = D * (dmax / D.max())
    rng = np.random.default_rng(seed)
    p = 0.75 * (1.0 - np.exp(-4.0 / 3.0 * D))  # the mismatch rate of a JC distance
    M = np.zeros((n, n, 17), np.uint32)
    mism = rng.binomial(length, p)
    off = [c for c in range(16) if c % 5]
    M[:, :, off] = rng.multinomial(mism.reshape(-1), np.full(12, 1 / 12)).reshape(n, n, 12)
    M[:, :, 0:16:5] = rng.multinomial((length - mism).reshape(-1), np.full(4, 0.25)).reshape(n, n, 4)
    M[:, :, 16] = length
    k = np.arange(n)
    M[k, k] = 0
    M[k, k, 0] = M[k, k, 16] = 1
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["300:100", "1000:100", "3085:20"], help="n:count")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--dmax", type=float, default=0.026)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD, if there is one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boot_trees_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib

    commit = args.commit
    if not commit:
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True)
        commit = p.stdout.decode().strip() if p.returncode == 0 else "unknown"
    ctx = lib.Context(0)
    rows = []
    for case in args.cases:
        n, count = (int(x) for x in case.split(":"))
        M = counts(n, args.length, args.dmax, n)
        nrec = n - 2

        def one():
            return lib.bootstrap_nj(ctx, M, count, lib.M_JC, seed=args.seed)

        def three():
            B = lib.bootstrap(ctx, M, count, seed=args.seed)
            D = np.empty((count, n, n))
            for k in range(count):
                D[k] = lib.distances(B[k], lib.M_JC)
            return lib.nj_batch(ctx, D)

        row = {"n": n, "count": count}
        results = {}
        for name, fn in (("one", one), ("three", three)):
            fn()  # warm-up
            runs = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                results[name] = fn()
                runs.append(time.perf_counter() - t0)
            row[name + "_s"] = min(runs)
            row[name + "_runs_s"] = runs
        records = count * nrec * 40 + count * 8
        row["one_host_bytes"] = records
        row["three_host_bytes"] = records + count * n * n * (68 + 8)
        (J1, bad1), (J3, bad3) = results["one"], results["three"]
        row["three_over_one"] = row["three_s"] / row["one_s"]
        row["bad_one"], row["bad_three"] = int((bad1 >= 0).sum()), int((bad3 >= 0).sum())
        row["trees_equal"] = int(sum(J1[k].tobytes() == J3[k].tobytes() for k in range(count)))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    res = {"what": "andi_hip_bootstrap_nj (D == NULL) beside andi_hip_bootstrap -> andi_hip_distances -> andi_hip_nj_batch "
                   "on the same library, model JC; wall time with copies, least of %d warm runs; counts of %d positions a "
                   "pair on an additive tree, largest distance %g" % (args.reps, args.length, args.dmax),
           "commit": commit, "rows": rows}
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
