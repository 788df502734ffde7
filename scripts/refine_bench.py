#!/usr/bin/env python3
"""Balanced nearest-neighbor interchanges on the device (andi_hip_refine): the time of the call, of a round, and its
yardsticks, in one process.

The trees: fit_bench's -- additive trees with 10 % multiplicative noise on the distances at --sizes (1000 and 3085)
leaves, joined by andi_hip_tree (nj) -- as they are ("nj": a handful of rounds) and after n random interchanges
("perturbed": a real search).  Per start, after one warm-up, the least of --reps runs by a host clock around the call,
which is synchronous and includes its copies and one look of the host a round:
  refine    andi_hip_refine with tol = 1e-9 and max_moves = 10 n: moves + 1 rounds, each the order, the leaf sets, the
            table A of (2n - 3) x n averages, 4 (2n - 3) sums, the gains and the move;
  zero      the same call with max_moves = 0 and a tolerance nothing passes: one round, the call's fixed part with it;
  round     (refine - zero) / moves where moves were made: what one more round costs;
  tree, fit andi_hip_tree and andi_hip_fit on the same matrix: what the user pays anyway, and the nearest relative.
The yardsticks of a round: the table is written once and read about twice (the sums read four rows a node, the table
kernel reads back what it wrote), 3 x 8 (2n - 3) n bytes against the copy ceiling andi_hip_copy_ceiling reports; and
k_paths (tree_paths.h), the table kernel's kin, which has the same n threads and the same chain of dependent loads.
At --model-leaves (200; 0: not at all) the NumPy restatement (tests/bme_model.py) runs on the host and must equal the
device bit for bit.  The kernels' own times come from a traced run of its own (--trace-size N: one warm-up and one timed
call of the perturbed start at N leaves and nothing else, for rocprofv3 --kernel-trace).
Writes one JSON object to --out (default: profiles/refine_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

TOL = 1e-9


def least(fn, reps):
    fn()  # warm-up
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        runs.append(time.perf_counter() - t0)
    return min(runs), runs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 3085])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--model-leaves", type=int, default=200)
    ap.add_argument("--trace-size", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import bme_model
    import nj_model

    ctx = lib.Context(0)
    if args.trace_size:
        n = args.trace_size
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=args.noise)
        P = bme_model.perturb(lib.tree(ctx, D, "nj"), np.random.default_rng(n), n)
        _, _, (K, res) = least(lambda: lib.refine(ctx, P, D, tol=TOL), 1)
        print(json.dumps({"n": n, "moves": int(res["moves"]), "converged": int(res["converged"])}))
        ctx.close()
        return
    ceiling = lib.copy_ceiling(ctx, 1 << 30, 5)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=args.noise)
        E = 2 * n - 3
        t_tree, tree_runs, J = least(lambda: lib.tree(ctx, D, "nj"), args.reps)
        t_fit, fit_runs, _ = least(lambda: lib.fit(ctx, J, D, "ols", per=True), args.reps)
        starts = {"nj": J, "perturbed": bme_model.perturb(J, np.random.default_rng(n), n)}
        for name, S in starts.items():
            t_zero, zero_runs, _ = least(lambda: lib.refine(ctx, S, D, tol=1e300, max_moves=0), args.reps)
            t_ref, ref_runs, (K, res) = least(lambda: lib.refine(ctx, S, D, tol=TOL), args.reps)
            moves = int(res["moves"])
            round_s = (t_ref - t_zero) / moves if moves else None
            traffic = 3 * 8 * E * n
            row = {"n": n, "start": name, "edges": E, "moves": moves, "converged": int(res["converged"]),
                   "changed": len(bme_model.inner_splits(S) - bme_model.inner_splits(K)),
                   "length_before": float(res["length_before"]), "length_after": float(res["length_after"]),
                   "refine_s": t_ref, "refine_runs_s": ref_runs, "zero_moves_s": t_zero, "zero_moves_runs_s": zero_runs,
                   "round_s": round_s, "table_bytes": 8 * E * n, "round_traffic_bytes": traffic,
                   "round_at_copy_ceiling_s": traffic / (ceiling * 1e9),
                   "round_over_copy_ceiling": round_s / (traffic / (ceiling * 1e9)) if moves else None,
                   "tree_s": t_tree, "tree_runs_s": tree_runs, "fit_s": t_fit, "fit_runs_s": fit_runs,
                   "refine_over_tree": t_ref / t_tree, "refine_over_fit": t_ref / t_fit}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    m, model = args.model_leaves, None
    if m >= 3:  # (0: no restatement)
        Dm, _, _ = nj_model.additive_tree(m, seed=m, noise=args.noise)
        Pm = bme_model.perturb(lib.tree(ctx, Dm, "nj"), np.random.default_rng(m), m)
        t0 = time.perf_counter()
        want = bme_model.refine(Pm, Dm, tol=TOL)
        t_model = time.perf_counter() - t0
        t_dev, _, got = least(lambda: lib.refine(ctx, Pm, Dm, tol=TOL, log=True), args.reps)
        model = {"n": m, "moves": int(want[1]["moves"]), "numpy_s": t_model, "device_s": t_dev,
                 "equal_to_restatement": all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))}
        print(json.dumps(model), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_refine (bnni, tol 1e-9, at most 10 n moves) on nj trees of additive matrices with %g %% multiplicative "
                   % (100 * args.noise)
                   + "noise, as joined and after n random interchanges; every call whole, with its copies and one look of the host "
                   + "a round, by a host clock, least of %d after a warm-up, one process" % args.reps,
           "copy_ceiling_gbps": ceiling,
           "yardsticks": {"round_traffic": "the table written once and read about twice: 3 x 8 (2n - 3) n bytes, at the copy ceiling",
                          "k_paths_us_n3085": 3450, "k_paths": "the table kernel's kin (DESIGN.md 10.15): n threads, one chain of "
                                                               + "dependent loads each"},
           "not_measured": "no counters; the kernels' own times are a traced run of its own (profiles/refine_kernel_stats.txt, "
                           + "if it is there)",
           "rows": rows, "restatement": model}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if model and not model["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
