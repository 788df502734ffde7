#!/usr/bin/env python3
"""The rogue genomes of a bootstrap on the device: andi_hip_nj_transfer_taxa beside andi_hip_nj_transfer on the same records.

Trees: scripts/transfer_bench.py's -- one additive tree per size (tests/nj_model.py, seed = n) and --count copies of its
distances with seeded symmetric noise, joined by andi_hip_nj_batch in chunks of 20 matrices -- once per --noise: at
that script's 1 % every replicate has every branch of the tree and no leaf moves; at 20 % branches are lost and leaves
move.  Timed, in one process: the wall time around the andi_hip_nj_transfer_taxa call (match == dist == NULL, what the
command line asks for) and around the andi_hip_nj_transfer call (per == NULL), a host clock, with the calls' copies in
and out (both end in a synchronise); the least of --reps runs after one warm-up each.  taxa_over_transfer is their ratio: the inner loop is k_transfer's and the
scatter reads each replicate's sets once, so it should be near 1.  Checked at every size: min(dist, depth - 1) is the
transfer index, the moved leaves sum to the counted distances, and at --cutoff 0 the counted pairs are andi_hip_nj_support's
counts.  Writes one JSON object to --out (default: profiles/rogues_bench.json).
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


def least(call, reps):
    call()  # warm-up
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        runs.append(time.perf_counter() - t0)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 3085])
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=float, nargs="*", default=[0.01, 0.2])
    ap.add_argument("--cutoff", type=float, default=0.3)
    ap.add_argument("--commit", help="the commit the numbers are taken on (default: git rev-parse HEAD, if there is one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rogues_bench.json"))
    args = ap.parse_args()
    from andi_amd import lib
    import nj_model

    commit = args.commit
    if not commit:
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True)
        commit = p.stdout.decode().strip() if p.returncode == 0 else "unknown"
    ctx = lib.Context(0)
    rows = []
    for n, noise in [(n, noise) for n in args.sizes for noise in args.noise]:
        D, _, _ = nj_model.additive_tree(n, seed=n)
        rng = np.random.default_rng(n)
        tree = lib.nj(ctx, D)
        parts = []
        for first in range(0, args.count, 20):
            Ds = np.empty((min(20, args.count - first), n, n))
            for k in range(len(Ds)):
                E = np.triu(rng.uniform(-noise, noise, (n, n)), 1)
                Ds[k] = D * (1.0 + E + E.T)
            J, bad = lib.nj_batch(ctx, Ds)
            assert (bad == -1).all()
            parts.append(J)
        J = np.concatenate(parts)
        del Ds, parts
        taxa = least(lambda: lib.nj_transfer_taxa(ctx, tree, J, cutoff=args.cutoff), args.reps)
        transfer = least(lambda: lib.nj_transfer(ctx, tree, J), args.reps)
        moved, pairs, match, dist = lib.nj_transfer_taxa(ctx, tree, J, cutoff=args.cutoff, detail=True)
        depth, total, per = lib.nj_transfer(ctx, tree, J, per=True)
        on = dist <= np.floor(args.cutoff * (depth.astype(np.float64) - 1.0)).astype(np.uint32)[None, :]
        row = {"n": n, "count": args.count, "noise": noise, "cutoff": args.cutoff, "taxa_s": min(taxa), "taxa_runs_s": taxa,
               "transfer_s": min(transfer), "transfer_runs_s": transfer, "taxa_over_transfer": min(taxa) / min(transfer),
               "pairs": pairs, "moved_sum": int(moved.sum()), "leaves_that_move": int((moved != 0).sum()),
               "dist_is_per": bool((np.minimum(dist, depth[None, :] - 1) == per).all()),
               "moved_is_dist": bool(pairs == int(on.sum()) and int(moved.sum()) == int(dist[on].sum()))}
        if args.cutoff == 0.0:
            row["pairs_is_support"] = bool(pairs == int(lib.nj_support(ctx, tree, J).sum()))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    res = {"what": "andi_hip_nj_transfer_taxa (match == dist == NULL) and andi_hip_nj_transfer (per == NULL) on the same "
                   "records in one process: wall time with copies, least of the warm runs; additive trees, replicates with "
                   "noise joined by andi_hip_nj_batch, cutoff %g" % args.cutoff,
           "commit": commit, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    if not all(r["dist_is_per"] and r["moved_is_dist"] and r.get("pairs_is_support", True) for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
