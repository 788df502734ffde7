#!/usr/bin/env python3
"""Rooting on the device (andi_hip_root): the time of the call beside its two nearest yardsticks, in one process.

The trees: nj_bench's additive trees with 1 % noise at --sizes (1000 and 3085) leaves, joined by andi_hip_tree (nj).  Per
size, after one warm-up of each call, the least of --reps runs by a host clock around the call -- each call is synchronous,
ends in a synchronise and includes its copies:
  root_mad       andi_hip_root, MAD: the table, 2 passes of (2n - 3) * n(n - 1)/2 pair visits, the choice;
  root_midpoint  andi_hip_root, midpoint: the table and the farthest pair (what MAD pays before its passes);
  place          andi_hip_place (OLS) with nq = n queries, the matrix's own rows, on the same tree: existing code with the
                 same access pattern, 2 * n * (2n - 3) * n leaf visits;
  tree           andi_hip_tree on the same matrix: what the user pays anyway.
Reported: visits a second of root (MAD less midpoint: the two passes alone, and the whole call) and of place, their ratio,
and the floor of the two passes from the inner loops' vector instructions -- counted by hand in the ISA of one build of
root.hip (hipcc -S; the c loops of k_root<1> and k_root<2>): count again when the kernel changes -- with v_rcp_f64 as 4
for its quarter rate, at one wave-instruction per 4 cycles and SIMD, 1024 SIMDs of 64 lanes at 2.4 GHz (DESIGN.md 10.14's
yardstick).  The command line roots every tree with one call: what -b 100 costs at a size is 100 calls, reported as such.
At --model-leaves (200; 0: not at all) the NumPy restatement (tests/root_model.py) runs on the host and must equal the
device bit for bit.
Writes one JSON object to --out (default: profiles/root_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

# vector instructions a pair visit in the c loops (v_rcp_f64 counted 4), and their LDS reads; by hand from the ISA
PASS1_SLOTS, PASS1_LDS = 29, 3
PASS2_SLOTS, PASS2_LDS = 27, 2
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
    ap.add_argument("--model-leaves", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "root_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import nj_model
    import root_model

    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=0.01)
        E = 2 * n - 3
        t_tree, tree_runs, J = least(lambda: lib.tree(ctx, D, "nj"), args.reps)
        t_mad, mad_runs, rec = least(lambda: lib.root(ctx, J, "mad"), args.reps)
        t_mid, mid_runs, mid = least(lambda: lib.root(ctx, J, "midpoint"), args.reps)
        t_place, place_runs, _ = least(lambda: lib.place(ctx, J, D, "ols"), args.reps)
        visits = 2 * E * (n * (n - 1) // 2)
        place_visits = 2 * n * E * n
        floor = E * (n * (n - 1) // 2) * (PASS1_SLOTS + PASS2_SLOTS) / LANE_INSTRUCTIONS_PER_S
        score, ambiguity = root_model.score(rec)
        row = {"n": n, "edges": E, "pairs": int(rec["pairs"]), "pair_visits": visits,
               "root_mad_s": t_mad, "root_mad_runs_s": mad_runs, "root_midpoint_s": t_mid, "root_midpoint_runs_s": mid_runs,
               "passes_s": t_mad - t_mid, "visits_per_s_call": visits / t_mad, "visits_per_s_passes": visits / (t_mad - t_mid),
               "place_s": t_place, "place_runs_s": place_runs, "place_leaf_visits": place_visits,
               "place_visits_per_s": place_visits / t_place,
               "rate_over_place_call": (visits / t_mad) / (place_visits / t_place),
               "rate_over_place_passes": (visits / (t_mad - t_mid)) / (place_visits / t_place),
               "floor_passes_s": floor, "passes_over_floor": (t_mad - t_mid) / floor, "call_over_floor": t_mad / floor,
               "tree_s": t_tree, "tree_runs_s": tree_runs, "root_over_tree": t_mad / t_tree,
               "b100_single_calls_s": 100 * t_mad,
               "mad": {"edge": int(rec["edge"]), "distal": float(rec["distal"]), "score": float(score), "ambiguity": float(ambiguity)},
               "midpoint": {"edge": int(mid["edge"]), "distal": float(mid["distal"])}}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    m, model = args.model_leaves, None
    if m >= 3:  # (0: no restatement, for a kernel trace of one size alone)
        Dm, _, _ = nj_model.additive_tree(m, seed=m, noise=0.01)
        Jm = lib.tree(ctx, Dm, "nj")
        t0 = time.perf_counter()
        want = root_model.root(Jm, "mad", per=True)
        t_model = time.perf_counter() - t0
        t_dev, _, got = least(lambda: lib.root(ctx, Jm, "mad", per=True), args.reps)
        model = {"n": m, "numpy_s": t_model, "device_s": t_dev,
                 "equal_to_restatement": all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))
                 and lib.root(ctx, Jm, "midpoint").tobytes() == root_model.root(Jm, "midpoint").tobytes()}
        print(json.dumps(model), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_root on nj trees of additive matrices with 1 % noise; every call whole, with its copies, by a host "
                   + "clock, least of %d after a warm-up, one process; place: andi_hip_place (ols), nq = n, same tree" % args.reps,
           "floor": {"pass1_slots_per_visit": PASS1_SLOTS, "pass2_slots_per_visit": PASS2_SLOTS, "pass1_lds_reads": PASS1_LDS,
                     "pass2_lds_reads": PASS2_LDS, "lane_instructions_per_s": LANE_INSTRUCTIONS_PER_S,
                     "counted": "by hand from the ISA of one build (hipcc -S), v_rcp_f64 as 4"},
           "not_measured": "no counters: how the kernels' time above the floor divides between LDS reads, the staging of the "
                           + "tiles and the triangular tail (the kernels' own times: a traced run of its own, "
                           + "profiles/root_kernel_stats_n3085.txt); the batch form (out of scope): -b 100 is 100 calls",
           "rows": rows, "restatement": model}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if model and not model["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
