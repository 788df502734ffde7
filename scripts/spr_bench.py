#!/usr/bin/env python3
"""Balanced subtree pruning and regrafting on the device (andi_hip_refine_spr) beside the interchanges of andi_hip_refine:
the time of the call, of a round, the moves and the length reached, in one process.

The trees: refine_bench's -- additive trees with 10 % multiplicative noise on the distances at --sizes (1000 and 3085)
leaves, joined by andi_hip_tree (nj) -- as they are ("nj") and after n random interchanges ("perturbed": the far start).
Per start and per search ("spr", "bnni"), after one warm-up call at 200 leaves, one run by a host clock around the call,
which is synchronous and includes its copies and one look of the host a round:
  zero      the call with max_moves = 0 and a tolerance nothing passes: one round, the call's fixed part with it;
  search    the call with tol = 1e-9 and max_moves = --max-moves (default 10 n): moves + 1 rounds;
  round     (search - zero) / moves where moves were made: what one more round costs.
The yardsticks of an SPR round: the same tree's round of interchanges, measured here beside it; and the table B, 8 (2n - 3)^2
bytes, written once and read once by k_pairs itself (an entry is the average of two entries a level down), at the copy
ceiling andi_hip_copy_ceiling reports.  At --model-leaves (200; 0: not at all) the NumPy restatement (tests/spr_model.py)
runs on the host and must equal the device bit for bit.  The kernels' own times come from a traced run of its own
(--trace-size N: one warm-up and one call of --trace-moves moves from the perturbed start at N leaves and nothing else,
for rocprofv3 --kernel-trace).
Writes one JSON object to --out (default: profiles/spr_bench.json)."""
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def write(out, noise, ceiling, rows, model):
    res = {"what": "andi_hip_refine_spr beside andi_hip_refine (tol 1e-9) on nj trees of additive matrices with %g %% multiplicative "
                   % (100 * noise)
                   + "noise, as joined and after n random interchanges; every call whole, with its copies and one look of the host "
                   + "a round, by a host clock, one run each after a warm-up at 200 leaves, one process",
           "copy_ceiling_gbps": ceiling,
           "yardsticks": {"bnni_round": "the same tree's round of interchanges, in the same process",
                          "pairs_traffic": "B written once and read once: 2 x 8 (2n - 3)^2 bytes, at the copy ceiling"},
           "not_measured": "no counters; the kernels' own times are a traced run of its own (profiles/spr_kernel_stats.txt, if it "
                           + "is there)",
           "rows": rows, "restatement": model}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 3085])
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--max-moves", type=int, default=0)
    ap.add_argument("--model-leaves", type=int, default=200)
    ap.add_argument("--trace-size", type=int, default=0)
    ap.add_argument("--trace-moves", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spr_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import bme_model
    import nj_model
    import spr_model

    ctx = lib.Context(0)
    searches = {"spr": lambda S, D, **kw: lib.refine_spr(ctx, S, D, **kw), "bnni": lambda S, D, **kw: lib.refine(ctx, S, D, **kw)}
    Dw, _, _ = nj_model.additive_tree(200, seed=200, noise=args.noise)
    Pw = bme_model.perturb(lib.tree(ctx, Dw, "nj"), np.random.default_rng(200), 200)
    for run in searches.values():
        run(Pw, Dw, tol=TOL)  # warm-up: the kernels loaded, the arena grown
    if args.trace_size:
        n = args.trace_size
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=args.noise)
        P = bme_model.perturb(lib.tree(ctx, D, "nj"), np.random.default_rng(n), n)
        K, res = lib.refine_spr(ctx, P, D, tol=TOL, max_moves=args.trace_moves)
        print(json.dumps({"n": n, "moves": int(res["moves"]), "converged": int(res["converged"])}))
        ctx.close()
        return
    ceiling = lib.copy_ceiling(ctx, 1 << 30, 5)
    rows = []
    for n in args.sizes:
        D, _, _ = nj_model.additive_tree(n, seed=n, noise=args.noise)
        E = 2 * n - 3
        J = lib.tree(ctx, D, "nj")
        cap = args.max_moves or 10 * n
        for name, S in {"nj": J, "perturbed": bme_model.perturb(J, np.random.default_rng(n), n)}.items():
            row = {"n": n, "start": name, "edges": E, "max_moves": cap, "pairs_bytes": 8 * E * E,
                   "pairs_traffic_at_copy_ceiling_s": 2 * 8 * E * E / (ceiling * 1e9)}
            for kind, run in searches.items():
                t_zero, _ = timed(lambda: run(S, D, tol=1e300, max_moves=0))
                t, (K, res) = timed(lambda: run(S, D, tol=TOL, max_moves=cap))
                moves = int(res["moves"])
                row[kind] = {"moves": moves, "converged": int(res["converged"]), "search_s": t, "zero_moves_s": t_zero,
                             "round_s": (t - t_zero) / moves if moves else None,
                             "changed": len(bme_model.inner_splits(S) - bme_model.inner_splits(K)),
                             "length_before": float(res["length_before"]), "length_after": float(res["length_after"])}
            if row["spr"]["round_s"] and row["bnni"]["round_s"]:
                row["spr_round_over_bnni_round"] = row["spr"]["round_s"] / row["bnni"]["round_s"]
            row["spr_length_minus_bnni_length"] = row["spr"]["length_after"] - row["bnni"]["length_after"]
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            write(args.out, args.noise, ceiling, rows, None)  # (a run cut short leaves what it measured)
    m, model = args.model_leaves, None
    if m >= 3:  # (0: no restatement)
        Dm, _, _ = nj_model.additive_tree(m, seed=m, noise=args.noise)
        Pm = bme_model.perturb(lib.tree(ctx, Dm, "nj"), np.random.default_rng(m), m)
        t_model, want = timed(lambda: spr_model.refine_spr(Pm, Dm, tol=TOL))
        t_dev, got = timed(lambda: lib.refine_spr(ctx, Pm, Dm, tol=TOL, log=True))
        model = {"n": m, "moves": int(want[1]["moves"]), "numpy_s": t_model, "device_s": t_dev,
                 "equal_to_restatement": all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))}
        print(json.dumps(model), file=sys.stderr)
    ctx.close()
    write(args.out, args.noise, ceiling, rows, model)
    if model and not model["equal_to_restatement"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
