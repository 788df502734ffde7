#!/usr/bin/env python3
"""Least-squares branch lengths on the device (andi_hip_fit): the time of the call beside its two nearest yardsticks, in one
process.

The trees: nj_bench's additive trees with 10 % multiplicative noise on the distances at --sizes (1000 and 3085) leaves,
joined by andi_hip_tree (nj).  Per size, after one warm-up of each call, the least of --reps runs by a host clock around
the call -- each call is synchronous, ends in a synchronise and includes its copies:
  fit       andi_hip_fit with both per-leaf arrays: the matrix up, one pass of (2n - 3) * n(n - 1)/2 pair visits without a
            division, the fold, the lengths, then twice the table of path lengths and the n^2 residual passes;
  root_mad  andi_hip_root (MAD) on the same tree: two passes of the same shape with a division each, and one table;
  tree      andi_hip_tree on the same matrix: what the user pays anyway.
Reported: pair visits a second of the whole call, its ratio to MAD's call, and the floor of the hot loop from its vector
instructions -- counted by hand in the ISA of one build of fit.hip (hipcc -S; the unrolled tile loop of k_fit): count again
when the kernel changes -- at one wave-instruction per 4 cycles and SIMD, 1024 SIMDs of 64 lanes at 2.4 GHz (DESIGN.md
10.14's yardstick).  At --model-leaves (200; 0: not at all) the NumPy restatement (tests/fit_model.py) runs on the host and
must equal the device bit for bit.
Writes one JSON object to --out (default: profiles/fit_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

# vector instructions a pair visit in k_fit's tile loop -- per class a v_and, a v_cmp, two v_cndmask and a v_add_f64 --
# and its LDS reads (a ds_read_b128 serves two visits); by hand from the ISA
FIT_SLOTS, FIT_LDS = 20, 0.5
LANE_INSTRUCTIONS_PER_S = 1024 * 64 / 4 * 2.4e9


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--model-leaves", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import fit_model
    import nj_model

    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=args.noise)
        E = 2 * n - 3
        t_tree, tree_runs, J = least(lambda: lib.tree(ctx, D, "nj"), args.reps)
        t_fit, fit_runs, got = least(lambda: lib.fit(ctx, J, D, "ols", per=True), args.reps)
        t_mad, mad_runs, _ = least(lambda: lib.root(ctx, J, "mad"), args.reps)
        visits = E * (n * (n - 1) // 2)
        floor = visits * FIT_SLOTS / LANE_INSTRUCTIONS_PER_S
        rec = got[1]
        row = {"n": n, "edges": E, "pair_visits": visits, "fit_s": t_fit, "fit_runs_s": fit_runs,
               "visits_per_s_call": visits / t_fit, "floor_hot_loop_s": floor, "call_over_floor": t_fit / floor,
               "root_mad_s": t_mad, "root_mad_runs_s": mad_runs, "fit_over_root_mad": t_fit / t_mad,
               "tree_s": t_tree, "tree_runs_s": tree_runs, "fit_over_tree": t_fit / t_tree,
               "matrix_bytes": 8 * n * n, "table_bytes": 8 * E * n, "sums_bytes": 32 * E * n,
               "fit": {"rss": float(rec["rss"]), "rss_joined": float(rec["rss_joined"]), "r2": float(fit_model.r2(rec)),
                       "r2_joined": float(fit_model.r2(rec, joined=True)), "negative": int(rec["negative"]),
                       "negative_joined": int(rec["negative_joined"])}}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    m, model = args.model_leaves, None
    if m >= 3:  # (0: no restatement, for a kernel trace of one size alone)
        Dm, _, _ = nj_model.additive_tree(m, seed=m, noise=args.noise)
        Jm = lib.tree(ctx, Dm, "nj")
        t0 = time.perf_counter()
        want = fit_model.fit(Jm, Dm, per=True)
        t_model = time.perf_counter() - t0
        t_dev, _, got = least(lambda: lib.fit(ctx, Jm, Dm, "ols", per=True), args.reps)
        model = {"n": m, "numpy_s": t_model, "device_s": t_dev,
                 "equal_to_restatement": all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))}
        print(json.dumps(model), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_fit (ols, with both per-leaf arrays) on nj trees of additive matrices with %g %% multiplicative noise; "
                   % (100 * args.noise)
                   + "every call whole, with its copies, by a host clock, least of %d after a warm-up, one process; " % args.reps
                   + "root_mad: andi_hip_root (MAD) on the same tree",
           "floor": {"slots_per_visit": FIT_SLOTS, "lds_reads_per_visit": FIT_LDS, "lane_instructions_per_s": LANE_INSTRUCTIONS_PER_S,
                     "counted": "by hand from the ISA of one build (hipcc -S): 256 v_add_f64, 512 v_cndmask_b32 and 512 "
                                + "v_and_b32 / v_cmp in the unrolled loop over a tile of 64 leaves"},
           "not_measured": "no counters; the kernels' own times are a traced run of its own "
                           + "(profiles/fit_kernel_stats_n3085.txt, if it is there)",
           "rows": rows, "restatement": model}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if model and not model["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
