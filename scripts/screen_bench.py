#!/usr/bin/env python3
"""What the k-mer sketch screen costs and what it saves, on one GPU: the 3085 references x 2.1 Mbp of scripts/rect_bench.py's
c4 set, with 1 and with 10 queries (andi-hip --reference=... --screen=32 without the ingest).

  sketch:    andi_hip_sketch of the references and of the queries (k = 21, scale = 1000), wall time and its split --
             packing on the host, uploads, the hash kernel's two passes, sort and unique (andi_hip_sketch_timings) --
             and andi_hip_sketch_shared.  The hash kernel must read 0.5 bytes per position; its throughput is reported
             beside the copy ceiling of andi_hip_copy_ceiling (which counts read + written bytes);
  screened:  andi_hip_screen + andi_hip_screen_select(keep) + andi_hip_dist_rect on the kept references;
  plain:     andi_hip_dist_rect on all references, in the same process -- the comparison point, with the parent's figures in
             profiles/rect_c4.json.  The screened table is checked against the plain one's columns.

Every timed call is run cold once and then warm --reps times.  Writes one JSON object to --out (default: stdout).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(fn, reps):
    t0 = time.perf_counter()
    out = fn()
    cold = time.perf_counter() - t0
    warm = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        warm.append(time.perf_counter() - t0)
    return out, {"cold_s": cold, "warm_s": warm, "warm_min_s": min(warm) if warm else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=3085)
    ap.add_argument("--length", type=int, default=2_100_000)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--keep", type=int, default=32)
    ap.add_argument("--kmer", type=int, default=21)
    ap.add_argument("--scale", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-plain", action="store_true", help="skip the unscreened run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import andi_amd
    from andi_amd import lib, synth
    model = lib.M_JC
    rec = {"library": os.path.relpath(lib.LIB_PATH, ROOT), "refs": a.refs, "length": a.length, "keep": a.keep, "kmer": a.kmer, "scale": a.scale}
    t0 = time.perf_counter()
    seqs = synth.genome_set_fast(a.refs + max(a.queries), a.length, 1e-3, 1.5e-2, seed=1729, threads=a.threads)[0]
    rec["generate_s"] = time.perf_counter() - t0
    refs = seqs[:a.refs]
    ctx = andi_amd.Context(0)
    rec["copy_ceiling_gbps"] = lib.copy_ceiling(ctx, 1 << 30, 5)
    positions = sum(len(s) for s in refs)

    def sketch_refs():
        S = andi_amd.sketch(ctx, refs, a.kmer, a.scale)
        t = S.timings()
        sizes = S.sizes.copy()
        S.close()
        return t, sizes

    (split, sizes), wall = timed(sketch_refs, a.reps)
    rec["sketch_refs"] = dict(wall, split_ms=split, positions=positions, hashes=int(sizes.sum()),
                              hash_gbps_of_bytes_it_must_read=0.5 * positions / (split["hash_ms"] * 1e-3) / 1e9)
    rec["runs"] = []
    for nq in a.queries:
        queries = seqs[a.refs:a.refs + nq]
        R = andi_amd.sketch(ctx, refs, a.kmer, a.scale)
        Q, qwall = timed(lambda: andi_amd.sketch(ctx, queries, a.kmer, a.scale), a.reps)
        shared, swall = timed(lambda: andi_amd.sketch_shared(ctx, Q, R), a.reps)
        R.close(), Q.close()

        def screened():
            sh, _, _ = andi_amd.screen(refs, queries, k=a.kmer, scale=a.scale)
            kept, taken = andi_amd.screen_select(sh, a.keep)
            cols = np.nonzero(kept)[0]
            return cols, lib.dist_rect([refs[c] for c in cols], queries, model=model, host_threads=a.threads)

        (cols, (MRQ, MQR)), scr = timed(screened, a.reps)
        run = {"queries": nq, "sketch_queries": qwall, "shared": swall, "kept": int(len(cols)), "screened": scr,
               "shared_equal_to_the_one_call": bool(np.array_equal(shared, andi_amd.screen(refs, queries, k=a.kmer, scale=a.scale)[0]))}
        if not a.no_plain:
            (PRQ, PQR), plain = timed(lambda: lib.dist_rect(refs, queries, model=model, host_threads=a.threads), a.reps)
            run["plain"] = plain
            run["screened_equal_to_plain_columns"] = bool((MRQ == PRQ[cols]).all() and (MQR == PQR[:, cols]).all())
            D = lib.distances_rect(PRQ, PQR, model)
            nearest = np.argsort(np.where(np.isnan(D), np.inf, D), axis=1, kind="stable")[:, :a.keep]
            run["nearest_by_distance_kept"] = [int(np.isin(nearest[q], cols).sum()) for q in range(nq)]
        rec["runs"].append(run)
    ctx.close()
    text = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
