#!/usr/bin/env python3
"""Neighbor-joining on the device (andi_hip_nj) against its NumPy restatement (tests/nj_model.py).

Matrices: additive trees (random binary trees, branch lengths in [0.01, 0.1)) with 1 % seeded noise at n = 29, 300, 1000
and 3085.  Device: the wall time of andi_hip_nj -- a host clock around the call, which ends in a synchronise; it includes
the H2D copy of D and the D2H copy of the records -- the least of --reps runs after one warm-up.  The restatement runs once
for n <= --model-max (it is O(n^3) in NumPy) and its records must equal the device's bit for bit.  Launches: 3 per step
with r >= 4 active nodes (row sums, tile minima, join), plus the mirror and the final record.  --sizes N...: other sizes
(one alone for a kernel trace of it).  Writes one JSON object to --out (default: stdout).

--method nj (the default: andi_hip_nj), bionj (andi_hip_tree with ANDI_TREE_BIONJ, against tests/bionj_model.py) or both:
the two builders on the same matrix in one process, their runs interleaved after a warm-up of each, one row per size and
method; every row also carries the median of its runs and their range.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[29, 300, 1000, 3085])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-max", type=int, default=1000)
    ap.add_argument("--method", choices=("nj", "bionj", "both"), default="nj")
    ap.add_argument("--out")
    args = ap.parse_args()
    from andi_amd import lib
    import bionj_model
    import nj_model

    methods = ("nj", "bionj") if args.method == "both" else (args.method,)
    call = {"nj": lambda c, D: lib.nj(c, D), "bionj": lambda c, D: lib.tree(c, D, "bionj")}
    model = {"nj": nj_model.nj, "bionj": bionj_model.bionj}

    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, splits, names = nj_model.additive_tree(n, seed=n, noise=0.01)
        for m in methods:
            call[m](ctx, D)  # warm-up
        times, J = {m: [] for m in methods}, {}
        for _ in range(args.reps):
            for m in methods:
                t0 = time.perf_counter()
                J[m] = call[m](ctx, D)
                times[m].append(time.perf_counter() - t0)
        for m in methods:
            t = times[m]
            row = {"n": n, "method": m, "steps": n - 3, "launches": 3 * (n - 3) + 2, "device_s": min(t), "device_runs_s": t,
                   "device_median_s": float(np.median(t)), "device_range_s": [min(t), max(t)],
                   "us_per_step": 1e6 * min(t) / max(n - 3, 1),
                   "splits_recovered": nj_model.unrooted_splits(nj_model.parse_newick(lib.newick(J[m], names))[1], names)
                   == splits}
            if n <= args.model_max:
                t0 = time.perf_counter()
                W = model[m](D)
                row["numpy_s"] = time.perf_counter() - t0
                row["equal_to_restatement"] = J[m].tobytes() == W.tobytes()
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    ctx.close()
    res = {"what": "%s on additive trees with 1%% noise" % " and ".join(
        {"nj": "andi_hip_nj", "bionj": "andi_hip_tree(ANDI_TREE_BIONJ)"}[m] for m in methods), "rows": rows}
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    if any(r.get("equal_to_restatement") is False for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
