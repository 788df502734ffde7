#!/usr/bin/env python3
"""Missing distances from quartets on the device (andi_hip_complete) beside what it stands in front of and what bounds it.

Matrices: additive trees (tests/nj_model.py: random binary trees, branch lengths in [0.01, 0.1), no noise) of 3085 leaves
with 0.1 %, 1 % and 10 % of the pairs missing at random, and a batch of 100 matrices of 1000 leaves with 1 % missing
(andi_hip_complete_batch).  Per case, from this one process:
  call_s      the wall time of the call -- a host clock around it; the call ends in a synchronise and includes the H2D copy
              of D, the D2H copies of C and the fills and one synchronisation per round -- the least of --reps runs after a
              warm-up;
  copies_s    the same call on the same matrix with nothing missing: the copies, the mirror and the count, no quartet kernel;
  rounds_s    call_s - copies_s: the quartet kernel and the apply kernel of every round, with the rounds' synchronisations;
  tree_s      andi_hip_tree (neighbor-joining) on the completed matrix: what a user pays anyway;
  candidates  the quartets the kernel went through: the fills' quartets, and for every pair and round that stayed without a
              fill no more than (n - 2)(n - 3) / 2 (not counted: a lower bound of the work);
  floor_bytes_s  8 bytes of D per candidate at the Infinity Cache's measured gather rate (8.6 TB/s) -- a block serves two
              partners of a row per load, so the kernel's own traffic is half of that when rows have that many;
  floor_fp64_s   the 5 double operations per candidate (two sums, the maximum, the difference, the minimum) at the FP64
              vector rate (78.6 TFLOP/s counts an FMA twice: 39.3e12 operations a second).
The vectorised NumPy restatement (tests/complete_model.py) runs at --model-n leaves with 1 % missing, where it finishes, and
must equal the device bit for bit.  Writes one JSON object to --out (default: stdout).
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

CACHE_BYTES_S = 8.6e12
FP64_OPS_S = 39.3e12


def punched(n, frac, seed):
    import nj_model
    T = nj_model.additive_tree(n, seed=seed, noise=0.0)[0]
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n, 1)
    hole = rng.random(len(iu[0])) < frac
    D = T.copy()
    D[iu[0][hole], iu[1][hole]] = np.nan
    D.T[iu[0][hole], iu[1][hole]] = np.nan
    return T, D


def least(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts, out


def floors(row, candidates):
    row["candidates"] = int(candidates)
    row["floor_bytes_s"] = 8.0 * candidates / CACHE_BYTES_S
    row["floor_fp64_s"] = 5.0 * candidates / FP64_OPS_S
    row["rounds_over_floor_bytes"] = row["rounds_s"] / row["floor_bytes_s"] if candidates else None
    row["rounds_over_floor_fp64"] = row["rounds_s"] / row["floor_fp64_s"] if candidates else None
    row["candidates_per_s"] = candidates / row["rounds_s"] if row["rounds_s"] > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3085)
    ap.add_argument("--fractions", type=float, nargs="*", default=[0.001, 0.01, 0.1])
    ap.add_argument("--batch", type=int, nargs=2, default=[100, 1000], metavar=("COUNT", "N"))
    ap.add_argument("--model-n", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    from andi_amd import lib
    import complete_model as cm

    ctx = lib.Context(0)
    rows = []
    for frac in args.fractions:
        T, D = punched(args.n, frac, seed=args.n)
        call_s, runs, (C, fills) = least(lambda: lib.complete(ctx, D), args.reps)
        copies_s = least(lambda: lib.complete(ctx, T), args.reps)[0]
        row = {"case": "n = %d, %g %% missing" % (args.n, 100 * frac), "n": args.n, "missing": len(fills),
               "left": int((fills["round"] == 0).sum()), "rounds": int(fills["round"].max()) if len(fills) else 0,
               "max_abs_error": float(np.abs(fills["value"] - T[fills["i"], fills["j"]]).max()) if len(fills) else 0.0,
               "call_s": call_s, "call_runs_s": runs, "copies_s": copies_s, "rounds_s": call_s - copies_s}
        if row["left"] == 0:
            row["tree_s"] = least(lambda: lib.tree(ctx, C, "nj"), args.reps)[0]
            row["call_over_tree"] = call_s / row["tree_s"]
        floors(row, int(fills["quartets"].sum()))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)

    count, n = args.batch
    Ds = np.stack([punched(n, 0.01, seed=1000 + k)[1] for k in range(count)])
    Ts = np.stack([punched(n, 0.0, seed=1000 + k)[0] for k in range(count)])
    call_s, runs, (Cs, missing, left) = least(lambda: lib.complete_batch(ctx, Ds), args.reps)
    copies_s = least(lambda: lib.complete_batch(ctx, Ts), args.reps)[0]
    row = {"case": "%d matrices of n = %d, 1 %% missing" % (count, n), "n": n, "count": count, "missing": int(missing.sum()),
           "left": int(left.sum()), "call_s": call_s, "call_runs_s": runs, "copies_s": copies_s, "rounds_s": call_s - copies_s}
    if row["left"] == 0:
        row["tree_s"] = least(lambda: lib.tree_batch(ctx, Cs, "nj"), args.reps)[0]
        row["call_over_tree"] = call_s / row["tree_s"]
    floors(row, sum(int(lib.complete(ctx, D)[1]["quartets"].sum()) for D in Ds[:4]) * count // 4)  # (from four of them)
    rows.append(row)
    print(json.dumps(row), file=sys.stderr)

    T, D = punched(args.model_n, 0.01, seed=args.model_n)
    call_s, runs, (C, fills) = least(lambda: lib.complete(ctx, D), args.reps)
    t0 = time.perf_counter()
    wC, wfills = cm.complete(D)
    row = {"case": "n = %d, 1 %% missing, against NumPy" % args.model_n, "n": args.model_n, "missing": len(fills),
           "call_s": call_s, "numpy_s": time.perf_counter() - t0,
           "equal_to_restatement": C.tobytes() == wC.tobytes() and fills.tobytes() == wfills.tobytes()}
    row["numpy_over_call"] = row["numpy_s"] / call_s
    rows.append(row)
    print(json.dumps(row), file=sys.stderr)
    ctx.close()

    res = {"what": "andi_hip_complete and andi_hip_complete_batch on additive trees with pairs missing at random",
           "cache_bytes_per_s": CACHE_BYTES_S, "fp64_ops_per_s": FP64_OPS_S, "rows": rows}
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    if not rows[-1]["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
