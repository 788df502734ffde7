#!/usr/bin/env python3
"""Transfer bootstrap support on the device: andi_hip_nj_transfer beside the NumPy model and the instruction floor.

Trees: one additive tree per size (tests/nj_model.py, seed = n) and --count copies of its distances with seeded symmetric
noise of 1 % each, joined by andi_hip_nj_batch (in chunks of 20 matrices: 100 of them are 7.6 GB at n = 3085) --
replicates of one n, as scripts/consensus_bench.py makes them.  Timed: the wall time around the andi_hip_nj_transfer call
(per == NULL, what the command line asks for), a host clock, with the call's copies in and out (the call ends in a
synchronise); the least of --reps runs after one warm-up.  floor_s: the call's (n - 3)^2 * count * ceil(n / 64) word pairs
times four vector instructions (two 32-bit XORs, two v_bcnt_u32_b32) over 256 CUs * 128 lanes per clock * --ghz.
model_s: tests/transfer_model.transfer_numpy on the same records, once, for n <= --model-max; the results must be equal.
zero_is_support: the used replicates with a transfer index of 0 against andi_hip_nj_support, at every size.  Writes one
JSON object to --out (default: profiles/transfer_bench.json).
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[29, 300, 1000, 3085])
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--model-max", type=int, default=1000)
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD, if there is one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import nj_model
    import transfer_model

    commit = args.commit
    if not commit:
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True)
        commit = p.stdout.decode().strip() if p.returncode == 0 else "unknown"
    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n)
        rng = np.random.default_rng(n)
        tree = lib.nj(ctx, D)
        parts = []
        for first in range(0, args.count, 20):
            Ds = np.empty((min(20, args.count - first), n, n))
            for k in range(len(Ds)):
                E = np.triu(rng.uniform(-args.noise, args.noise, (n, n)), 1)
                Ds[k] = D * (1.0 + E + E.T)
            J, bad = lib.nj_batch(ctx, Ds)
            assert (bad == -1).all()
            parts.append(J)
        J = np.concatenate(parts)
        del Ds, parts
        lib.nj_transfer(ctx, tree, J)  # warm-up
        runs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            depth, total = lib.nj_transfer(ctx, tree, J)
            runs.append(time.perf_counter() - t0)
        d2, t2, per = lib.nj_transfer(ctx, tree, J, per=True)
        support = lib.nj_support(ctx, tree, J)
        pairs = (n - 3) ** 2 * args.count * ((n + 63) // 64)
        floor_s = pairs * 4 / (256 * 128 * args.ghz * 1e9)
        row = {"n": n, "count": args.count, "transfer_s": min(runs), "transfer_runs_s": runs, "word_pairs": pairs,
               "floor_s": floor_s, "transfer_over_floor": min(runs) / floor_s,
               "per_equals_sums": bool((per.astype(np.uint64).sum(0) == total).all() and (t2 == total).all()),
               "zero_is_support": bool(((per == 0).sum(0) == support).all()),
               "entries_not_zero": int((per != 0).sum()), "mean_tbe": float(np.mean(1.0 - total / (args.count * (depth - 1.0))))}
        if n <= args.model_max:
            t0 = time.perf_counter()
            want = transfer_model.transfer_numpy(tree, list(J))
            row["model_s"] = time.perf_counter() - t0
            row["model_over_transfer"] = row["model_s"] / min(runs)
            row["equal_to_model"] = bool((want[0] == depth).all() and (want[1] == total).all() and (want[2] == per).all())
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    res = {"what": "andi_hip_nj_transfer (per == NULL; wall time with copies, least of the warm runs) beside its instruction "
                   "floor at %.1f GHz and tests/transfer_model.transfer_numpy; additive trees, replicates with %g%% noise "
                   "joined by andi_hip_nj_batch" % (args.ghz, 100 * args.noise), "commit": commit, "rows": rows}
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if not all(r["zero_is_support"] and r["per_equals_sums"] and r.get("equal_to_model", True) for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
