#!/usr/bin/env python3
"""Linkage clustering on the device (andi_hip_linkage) beside neighbor-joining (andi_hip_nj) on the same matrices.

Matrices: scripts/nj_bench.py's -- additive trees (random binary trees, branch lengths in [0.01, 0.1)) with 1 % seeded noise
-- at n = 29, 300, 1000 and 3085, for single, complete and average linkage; and a batch of --batch (100) such matrices at
n = --batch-n (1000), each with noise of its own, through andi_hip_linkage_batch.  Device: the wall time of the call -- a
host clock around it; the call ends in a synchronise and includes the H2D copy of D and the D2H copy of the records -- the
least of --reps runs after one warm-up of that shape and method.  The yardstick is andi_hip_nj at the same n, timed the
same way in the same run: a linkage step does strictly less than a neighbor-joining step (no row sums, no search of the
triangle).  Launches: 2 per step (join, caches) plus the mirror and the first caches.  Where SciPy imports, the host time of
scipy.cluster.hierarchy.linkage on the same matrix is recorded beside it (one run; its input is the condensed matrix).  The
restatement (tests/linkage_model.py, O(n^3) in NumPy) runs for n <= --model-max and its records must equal the device's
bit for bit.  Writes one JSON object to --out (default: profiles/linkage_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def least(reps, call):
    call()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[29, 300, 1000, 3085])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-max", type=int, default=300)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batch-n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkage_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import linkage_model
    import nj_model
    try:
        from scipy.cluster import hierarchy
        from scipy.spatial.distance import squareform
    except ImportError:
        hierarchy = None

    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=0.01)
        _, nj_times = least(args.reps, lambda: lib.nj(ctx, D))
        for method in linkage_model.METHODS:
            Z, times = least(args.reps, lambda: lib.linkage(ctx, D, method))
            row = {"n": n, "method": method, "steps": n - 1, "launches": 2 * (n - 1) + 1, "device_s": min(times),
                   "device_runs_s": times, "us_per_step": 1e6 * min(times) / (n - 1), "nj_s": min(nj_times),
                   "nj_runs_s": nj_times, "linkage_over_nj": min(times) / min(nj_times)}
            if hierarchy is not None:
                y = squareform(D, checks=False)
                t0 = time.perf_counter()
                S = hierarchy.linkage(y, method)
                row["scipy_host_s"] = time.perf_counter() - t0
                row["heights_within_1e-12_of_scipy"] = bool(np.allclose(np.sort(Z["height"]), np.sort(S[:, 2]), rtol=1e-12, atol=0))
            if n <= args.model_max:
                t0 = time.perf_counter()
                W = linkage_model.linkage(D, method)
                row["numpy_s"] = time.perf_counter() - t0
                row["equal_to_restatement"] = Z.tobytes() == W.tobytes()
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    batch = []
    if args.batch > 0:
        n = args.batch_n
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=0.0)
        rng = np.random.default_rng(n)
        Ds = np.empty((args.batch, n, n))
        for k in range(args.batch):
            E = np.triu(rng.uniform(-0.01, 0.01, (n, n)), 1)
            Ds[k] = D * (1.0 + E + E.T)
        (_, nj_bad), nj_times = least(args.reps, lambda: lib.nj_batch(ctx, Ds))
        for method in linkage_model.METHODS:
            (Z, bad), times = least(args.reps, lambda: lib.linkage_batch(ctx, Ds, method))
            one = lib.linkage(ctx, Ds[args.batch // 2], method)
            row = {"n": n, "count": args.batch, "method": method, "device_s": min(times), "device_runs_s": times,
                   "ms_per_matrix": 1e3 * min(times) / args.batch, "nj_batch_s": min(nj_times), "nj_batch_runs_s": nj_times,
                   "all_usable": bool((bad == -1).all() and (nj_bad == -1).all()),
                   "equal_to_the_single_call": Z[args.batch // 2].tobytes() == one.tobytes()}
            batch.append(row)
            print(json.dumps(row), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_linkage beside andi_hip_nj on additive trees with 1 % noise; wall time of the call, least of "
                   + "%d warm runs" % args.reps, "rows": rows, "batch": batch}
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if any(r.get("equal_to_restatement") is False for r in rows) or any(not r["equal_to_the_single_call"] for r in batch):
        sys.exit(1)


if __name__ == "__main__":
    main()
