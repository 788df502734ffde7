#!/usr/bin/env python3
"""Tree-likeness scores from all quartets on the device (andi_hip_delta_scores) beside two yardsticks.

Matrices: nj_bench's -- additive trees (tests/nj_model.py: random binary trees, branch lengths in [0.01, 0.1)) with 1 %
seeded noise -- at 1000 and 3085 leaves, nothing missing, so every quartet is used.  Per size, from this one process:
  call_s       the wall time of the call -- a host clock around it; the call ends in a synchronise and includes the H2D copy
               of D (8 n^2 bytes), the cut of the items on the host and the D2H copy of the n records -- the least of --reps
               runs after a warm-up;
  quartets     C(n, 4), which the records must add up to (checked);
  quartets_per_s  quartets / call_s;
  complete_quartets_per_s  yardstick (a): the rates of k_complete_quartets, the kernel with the same access pattern that takes
               a maximum and a difference where this one sorts three sums and divides, read from profiles/complete_bench.json
               (least and most of its rows);
  floor_valu_s yardstick (b): the vector instructions of the inner loop per candidate, counted in the kernel's ISA
               (VALU_PER_CANDIDATE below: 27 FP64 -- 5 add, 6 min/max, 11 of the division, 2 class, 1 compare, ldexp,
               convert -- and 16 of 32 bits; v_rcp_f64 issues at a quarter of the rate and counts 4), at one
               wave-instruction per 4 cycles and SIMD: 1024 SIMDs x 16 lanes at 2.4 GHz;
  mean_delta   the matrix's mean delta, for the record.
The NumPy restatement (tests/delta_model.py) runs at --model-n leaves and must equal the device bit for bit.  Writes one
JSON object to --out (default: stdout).
"""
import argparse
import json
import os
import sys
import time
from math import comb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

# Counted by hand in the ISA of one build of delta.hip (hipcc -S, the l loop of k_delta_quartets): count again when the
# kernel changes.  43 instructions; v_rcp_f64 takes the issue slots of 4.
VALU_PER_CANDIDATE = 43 + 3
LANES_PER_S = 1024 * 16 * 2.4e9


def least(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 3085])
    ap.add_argument("--model-n", type=int, default=96)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    from andi_amd import lib
    import delta_model as dm
    import nj_model

    yard = None
    path = os.path.join(ROOT, "profiles", "complete_bench.json")
    if os.path.exists(path):
        rates = [r["candidates_per_s"] for r in json.load(open(path))["rows"] if r.get("candidates_per_s")]
        yard = [min(rates), max(rates)]

    ctx = lib.Context(0)
    rows = []
    for n in args.sizes:
        D = nj_model.additive_tree(n, seed=n, noise=0.01)[0]
        call_s, runs, rec = least(lambda: lib.delta_scores(ctx, D), args.reps)
        q = comb(n, 4)
        row = {"case": "n = %d, 1 %% noise" % n, "n": n, "quartets": q, "call_s": call_s, "call_runs_s": runs,
               "all_quartets_used": int(rec["quartets"].sum()) == 4 * q, "quartets_per_s": q / call_s,
               "complete_quartets_per_s": yard, "floor_valu_s": VALU_PER_CANDIDATE * q / LANES_PER_S,
               "mean_delta": float(int(rec["sum"].sum()) / (4.0 * q * (1 << 24)))}
        row["call_over_floor_valu"] = call_s / row["floor_valu_s"]
        if yard:
            row["rate_over_complete"] = [row["quartets_per_s"] / y for y in yard]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)

    n = args.model_n
    D = nj_model.additive_tree(n, seed=n, noise=0.01)[0]
    call_s, runs, rec = least(lambda: lib.delta_scores(ctx, D), args.reps)
    t0 = time.perf_counter()
    want = dm.scores(D)
    row = {"case": "n = %d, against NumPy" % n, "n": n, "quartets": comb(n, 4), "call_s": call_s,
           "numpy_s": time.perf_counter() - t0, "equal_to_restatement": rec.tobytes() == want.tobytes()}
    rows.append(row)
    print(json.dumps(row), file=sys.stderr)
    ctx.close()

    res = {"what": "andi_hip_delta_scores on additive trees with 1% noise", "valu_per_candidate": VALU_PER_CANDIDATE,
           "valu_per_candidate_source": "counted by hand in the ISA of the l loop of k_delta_quartets as built when this was "
                                        "run (43 instructions, v_rcp_f64 counted 4); not read from the binary by this script",
           "lanes_per_s": LANES_PER_S, "rows": rows}
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    if not rows[-1]["equal_to_restatement"] or not all(r.get("all_quartets_used", True) for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
