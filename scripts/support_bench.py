#!/usr/bin/env python3
"""Bootstrap support on the device: andi_hip_nj_batch against as many andi_hip_nj calls, and andi_hip_nj_support.

Matrices: one additive tree per size (tests/nj_model.py, seed = n) and --count copies of its distances with seeded
symmetric noise of 1 % each -- replicates of one n, as a bootstrap gives them.  Timed: the wall time around the call, a
host clock, with the call's copies in and out (both calls end in a synchronise); the least of --reps runs after one
warm-up.  sequential_s: --count andi_hip_nj calls one after the other.  batch_s: one andi_hip_nj_batch call over the same
matrices; its records must equal the sequential ones bit for bit.  support_s: one andi_hip_nj_support call of the point
tree against the batch's records.  Writes one JSON object to --out (default: stdout).
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


def _least(fn, reps):
    fn()  # warm-up
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[29, 300, 1000])
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD, if there is one)")
    ap.add_argument("--out")
    args = ap.parse_args()
    from andi_amd import lib
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
        tree = lib.nj(ctx, D)
        seq_s, seq_runs, singles = _least(lambda: [lib.nj(ctx, Ds[k]) for k in range(args.count)], args.reps)
        batch_s, batch_runs, (J, bad) = _least(lambda: lib.nj_batch(ctx, Ds), args.reps)
        sup_s, sup_runs, support = _least(lambda: lib.nj_support(ctx, tree, J), args.reps)
        row = {"n": n, "count": args.count, "sequential_s": seq_s, "sequential_runs_s": seq_runs, "batch_s": batch_s,
               "batch_runs_s": batch_runs, "sequential_over_batch": seq_s / batch_s, "support_s": sup_s,
               "support_runs_s": sup_runs, "mean_support": float(np.mean(support)) if len(support) else None,
               "batch_equals_sequential": bool((bad == -1).all()) and J.tobytes() == np.stack(singles).tobytes()}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_nj_batch against sequential andi_hip_nj calls, andi_hip_nj_support; additive trees, "
                   "replicates with 1% noise", "commit": commit, "rows": rows}
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    if not all(r["batch_equals_sequential"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
