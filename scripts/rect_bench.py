#!/usr/bin/env python3
"""Wall time of the query-versus-reference call (andi_hip_dist_rect) beside the square call it replaces, on one GPU.

  bench: the bench set (29 x 4.9 Mbp star, bench.py's defaults): 28 references + 1 query, against the 29 x 29 square call.
  c4:    3085 references x 2.1 Mbp (d ~ U[1e-3, 1.5e-2], scripts/full_size.py's C4 set) with 1 and with 10 queries
         (the 3085 x 3085 square call is not rerun here: scripts/full_size.py c4 measures it).

Every timed call is run cold once and then warm --reps times; the cross blocks are checked against the square call
(bench) or against the oracle's dist_anchor on sampled entries (c4).  The library's ANDI_E2E_TRACE lines of one warm
call (suffix arrays, index builds, scans of device 0's driver) are captured from the C stderr.  --rect-batch B...
repeats the rectangular calls with ANDI_RECT_BATCH=B (subjects per scan call; a switch of libandihip_test.so only).
Writes one JSON object to --out (default: stdout).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def traced(fn):
    """(fn's result, the library's stderr lines while it ran)"""
    os.environ["ANDI_E2E_TRACE"] = "1"
    from andi_amd import lib
    lib.reload_knobs()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("ANDI_E2E_TRACE", None)
            lib.reload_knobs()
        f.seek(0)
        lines = f.read().decode(errors="replace").splitlines()
    return out, [ln for ln in lines if "trace" in ln]


def timed(fn, reps):
    t0 = time.perf_counter()
    out = fn()
    cold = time.perf_counter() - t0
    warm = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        warm.append(time.perf_counter() - t0)
    return out, cold, warm


def rect_runs(refs, queries, model, reps, batches):
    from andi_amd import lib
    runs = []
    for b in batches:
        if b:
            os.environ["ANDI_RECT_BATCH"] = str(b)
        else:
            os.environ.pop("ANDI_RECT_BATCH", None)
        lib.reload_knobs()
        (MRQ, MQR), cold, warm = timed(lambda: lib.dist_rect(refs, queries, model=model), reps)
        _, trace = traced(lambda: lib.dist_rect(refs, queries, model=model))
        runs.append({"rect_batch": b or "default", "cold_s": cold, "warm_s": warm, "warm_min_s": min(warm) if warm else None,
                     "trace": trace})
    os.environ.pop("ANDI_RECT_BATCH", None)
    lib.reload_knobs()
    return MRQ, MQR, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=("bench", "c4"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 10], help="c4: numbers of queries")
    ap.add_argument("--rect-batch", type=int, nargs="*", default=[0], help="0: the default batch")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from andi_amd import lib, synth
    model = 1
    rec = {"config": a.config, "library": lib.LIB_PATH}
    if a.config == "bench":
        seqs = synth.genome_set_fast(29, 4_900_000, 0.0004, 0.03, seed=1729, threads=a.threads)[0]
        refs, queries = seqs[:28], seqs[28:]
        M, cold, warm = timed(lambda: lib.dist_matrix(seqs, model=model), a.reps)
        rec["square"] = {"shape": "29 x 29", "cold_s": cold, "warm_s": warm, "warm_min_s": min(warm)}
        MRQ, MQR, runs = rect_runs(refs, queries, model, a.reps, a.rect_batch)
        rec["rect"] = {"shape": "28 references x 1 query", "runs": runs,
                       "equal_to_square_blocks": bool((MRQ == M[:28, 28:]).all() and (MQR == M[28:, :28]).all())}
    else:
        from oracle import orc
        t0 = time.perf_counter()
        seqs = synth.genome_set_fast(3085 + max(a.queries), 2_100_000, 1e-3, 1.5e-2, seed=1729, threads=a.threads)[0]
        rec["generate_s"] = time.perf_counter() - t0
        refs = seqs[:3085]
        rec["rect"] = []
        rng = np.random.default_rng(5)
        for nq in a.queries:
            queries = seqs[3085:3085 + nq]
            MRQ, MQR, runs = rect_runs(refs, queries, model, a.reps, a.rect_batch)
            checked = []
            for r, q in zip(rng.integers(0, 3085, 2), rng.integers(0, nq, 2)):
                ok = bool((MRQ[r, q] == orc.OracleEsa(refs[r]).dist_anchor(queries[q], model=model)).all() and
                          (MQR[q, r] == orc.OracleEsa(queries[q]).dist_anchor(refs[r], model=model)).all())
                checked.append({"ref": int(r), "query": int(q), "equal_to_oracle": ok})
            rec["rect"].append({"shape": "3085 references x %d queries" % nq, "runs": runs, "oracle_samples": checked})
    text = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
