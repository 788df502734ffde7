#!/usr/bin/env python3
"""Placement on the device (andi_hip_place): the time of the call at the size of the project's largest tree.

The tree: a synthetic binary tree of --leaves (3085) leaves, a random joining order, branch lengths in [0.001, 0.01).
The queries: points on random edges of it, their own tree distances to the leaves off by up to 3 %, for 1, 100 and 1000
queries, both methods.  The call is synchronous -- it ends in a synchronise and includes the upload of the tree and the
distances, the table of path lengths (k_sets, k_paths), the weights, k_place, k_choose and the download of the records --
so device events around it (recorded on the default stream, idle before and after) and a host clock measure the same
window; both are recorded, after one warm-up of each shape, as the median of --reps runs with every run beside it.

Beside each time, the two floors of the call, computed from the shapes:
  bytes  the table, (2n - 3) * n * 8 bytes, read once per tile of QT = 4 queries in each of the two passes, over the
         6.3 TB/s a streaming read reaches on this device (a table that fits the 256 MB Infinity Cache can beat this one);
  ops    nq * (2n - 3) * n leaf visits of 10 double operations (5 per pass; none may be fused), over 39.3e12 per second:
         256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz, half of the 78.6 TFLOP/s the data sheet counts with an FMA as two.
And the only other implementation there is: the NumPy restatement (tests/place_model.py) at --model-leaves (300) leaves
and --model-queries (10) queries on the host, whose result the device's must equal bit for bit.
Writes one JSON object to --out (default: profiles/place_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

QT = 4
HBM_BYTES_PER_S = 6.3e12
F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9
OPS_PER_VISIT = 10


def queries(rng, paths, n, nq, noise=0.03):
    H, below, parent, L = paths
    rows = np.empty((nq, n))
    for q in range(nq):
        v = int(rng.integers(2 * n - 3))
        x, p = rng.uniform(0, 1) * L[v], rng.uniform(0, 0.01)
        rows[q] = np.where(below[v], (p + x) + H[v], (p + (L[v] - x)) + H[parent[v]]) * (1.0 + rng.uniform(-noise, noise, n))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=3085)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 100, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--model-leaves", type=int, default=300)
    ap.add_argument("--model-queries", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.json"))
    args = ap.parse_args()
    import torch
    from andi_amd import lib
    import place_model

    ctx = lib.Context(0)
    rng = np.random.default_rng(args.leaves)
    n = args.leaves
    J = place_model.random_tree(rng, n, lambda k: rng.uniform(0.001, 0.01, k))
    paths = place_model.paths(J, n)
    E = 2 * n - 3
    rows = []
    for nq in args.queries:
        D = queries(rng, paths, n, nq)
        for method in ("fm", "ols"):
            lib.place(ctx, J, D, method)  # warm-up of this shape
            events, clock = [], []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                t0 = time.perf_counter()
                P = lib.place(ctx, J, D, method)
                clock.append(time.perf_counter() - t0)
                b.record()
                b.synchronize()
                events.append(a.elapsed_time(b) * 1e-3)
            table = E * n * 8
            row = {"leaves": n, "queries": nq, "method": method, "events_s": statistics.median(events), "events_runs_s": events,
                   "host_clock_s": statistics.median(clock), "host_clock_runs_s": clock, "placed": int((P["edge"] >= 0).sum()),
                   "table_bytes": table, "leaf_visits_per_pass": nq * E * n,
                   "floor_bytes_s": 2 * -(-nq // QT) * table / HBM_BYTES_PER_S,
                   "floor_ops_s": OPS_PER_VISIT * nq * E * n / F64_OPS_PER_S}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    # the restatement, on the host, and that the device agrees with it
    m, mq = args.model_leaves, args.model_queries
    Jm = place_model.random_tree(rng, m, lambda k: rng.uniform(0.001, 0.01, k))
    Dm = queries(rng, place_model.paths(Jm, m), m, mq)
    model = []
    for method in ("fm", "ols"):
        t0 = time.perf_counter()
        want = place_model.place(Jm, Dm, method, per=True)
        t = time.perf_counter() - t0
        got = lib.place(ctx, Jm, Dm, method, per=True)
        row = {"leaves": m, "queries": mq, "method": method, "numpy_s": t,
               "equal_to_restatement": all(g.tobytes() == w.tobytes() for g, w in zip(got, want))}
        model.append(row)
        print(json.dumps(row), file=sys.stderr)
    ctx.close()
    res = {"what": "andi_hip_place on a synthetic tree, queries at their own tree distances off by up to 3 %; the whole "
                   + "synchronous call between device events and by a host clock, median of %d warm runs" % args.reps,
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "f64_ops_per_s": F64_OPS_PER_S, "ops_per_leaf_visit": OPS_PER_VISIT},
           "rows": rows, "restatement": model}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if not all(r["equal_to_restatement"] for r in model):
        sys.exit(1)


if __name__ == "__main__":
    main()
