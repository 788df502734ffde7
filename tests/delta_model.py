"""The contract of andi_hip_delta_scores (include/andi_hip.h) in NumPy: tree-likeness scores from all quartets.

Only D[i][j], i < j, is read; it is mirrored.  A pair is known iff its entry is finite.  For every quartet {x, y, u, v} of
distinct genomes whose six distances are known: s1 = d(x,y) + d(u,v), s2 = d(x,u) + d(y,v), s3 = d(x,v) + d(y,u), each one
rounded addition; a >= b >= c the three by value; w = a - c, u = a - b; the quartet is used iff w is finite;
delta = w > 0 ? u / w : 0; t = floor(delta * 2^24).  A genome's record is the number of used quartets that contain it and
the sum of their t."""
import itertools

import numpy as np

DELTA = np.dtype([("sum", "<u8"), ("quartets", "<u8")])
ONE = 1 << 24


def mirrored(D):
    """D as the call reads it: the upper triangle mirrored, a missing pair a NaN, the diagonal 0"""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    v = D[iu].copy()
    v[~np.isfinite(v)] = np.nan
    M = np.zeros((n, n))
    M[iu] = v
    M.T[iu] = v
    return M


def _t(s1, s2, s3):
    """(used, t) of quartets whose sums are the arrays s1, s2, s3 (a NaN where one of the two distances is missing)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        known = ~(np.isnan(s1) | np.isnan(s2) | np.isnan(s3))
        hi, lo = np.maximum(s1, s2), np.minimum(s1, s2)
        a, c = np.maximum(hi, s3), np.minimum(lo, s3)
        b = np.maximum(lo, np.minimum(hi, s3))
        w, u = a - c, a - b
        used = known & np.isfinite(w)
        delta = np.where(used & (w > 0), u / np.where(used & (w > 0), w, 1.0), 0.0)
        t = np.where(used, np.floor(delta * float(ONE)), 0.0).astype(np.uint64)
    return used, t


def _sum(a, b):
    """a + b, a NaN where either is missing (an overflowed sum is an infinity, not a NaN: its quartet is dropped by w)"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = a + b
    return np.where(np.isnan(a) | np.isnan(b), np.nan, s)


def scores(D):
    """the n records, vectorised per pair i < j over the pairs k < l above it"""
    M = mirrored(D)
    n = M.shape[0]
    out = np.zeros(n, DELTA)
    for i in range(n - 3):
        for j in range(i + 1, n - 2):
            if np.isnan(M[i, j]):
                continue
            K = np.arange(j + 1, n)
            ik, jk = M[i, K], M[j, K]
            kl = M[np.ix_(K, K)].copy()
            kl[np.tril_indices(len(K))] = np.nan  # k < l only
            used, t = _t(_sum(M[i, j], kl), _sum(ik[:, None], jk[None, :]), _sum(ik[None, :], jk[:, None]))
            total, count = t.sum(dtype=np.uint64), np.uint64(used.sum())
            out["sum"][i] += total
            out["sum"][j] += total
            out["quartets"][i] += count
            out["quartets"][j] += count
            out["sum"][K] += t.sum(axis=1, dtype=np.uint64) + t.sum(axis=0, dtype=np.uint64)
            out["quartets"][K] += (used.sum(axis=1) + used.sum(axis=0)).astype(np.uint64)
    return out


def quartet(M, x, y, u, v):
    """(used, t) of one quartet on the mirrored matrix M, in plain Python"""
    six = [M[x, y], M[u, v], M[x, u], M[y, v], M[x, v], M[y, u]]
    if not all(np.isfinite(d) for d in six):
        return False, 0
    with np.errstate(over="ignore", invalid="ignore"):
        c, b, a = sorted([six[0] + six[1], six[2] + six[3], six[4] + six[5]])
        w, uu = a - c, a - b
        if not np.isfinite(w):
            return False, 0
        delta = uu / w if w > 0 else 0.0
    return True, int(np.floor(delta * float(ONE)))


def scores_loops(D):
    """the same by the plain four loops of the contract's text"""
    M = mirrored(D)
    n = M.shape[0]
    out = np.zeros(n, DELTA)
    for q in itertools.combinations(range(n), 4):
        used, t = quartet(M, *q)
        if used:
            for x in q:
                out["sum"][x] += np.uint64(t)
                out["quartets"][x] += np.uint64(1)
    return out


def through(D, pairs):
    """(records, seen): the records of the quartets that contain at least one of the given pairs alone, each quartet once, and
    how many such quartets contain each genome, used or not -- for matrices whose every other quartet has three equal sums
    by construction (used, t = 0: it adds C(n - 1, 3) - seen to a genome's count and nothing to its sum)"""
    M = mirrored(D)
    n = M.shape[0]
    parts = []
    for m, (p, q) in enumerate(pairs):
        rest = np.array([x for x in range(n) if x not in (p, q)], np.int64)
        X, Y = np.triu_indices(len(rest), 1)
        X, Y = rest[X], rest[Y]
        again = np.zeros(len(X), bool)  # the quartet holds an earlier pair too: it has been taken
        for e, f in pairs[:m]:
            again |= ((X == e) | (Y == e) | (e in (p, q))) & ((X == f) | (Y == f) | (f in (p, q)))
        parts.append(np.stack([np.full(len(X), p), np.full(len(X), q), X, Y])[:, ~again])
    q0, q1, q2, q3 = np.concatenate(parts, axis=1) if parts else np.zeros((4, 0), np.int64)
    used, t = _t(_sum(M[q0, q1], M[q2, q3]), _sum(M[q0, q2], M[q1, q3]), _sum(M[q0, q3], M[q1, q2]))
    out = np.zeros(n, DELTA)
    seen = np.zeros(n, np.uint64)
    assert len(q0) < 1 << 29  # the weighted counts below are sums of doubles: exact below 2^53
    for q in (q0, q1, q2, q3):
        out["sum"] += np.bincount(q, weights=t.astype(np.float64), minlength=n).astype(np.uint64)
        out["quartets"] += np.bincount(q, weights=used.astype(np.float64), minlength=n).astype(np.uint64)
        seen += np.bincount(q, minlength=n).astype(np.uint64)
    return out, seen


def with_background(D, pairs):
    """the records of a matrix all of whose quartets outside `through(D, pairs)` are used with t = 0"""
    n = np.asarray(D).shape[0]
    out, seen = through(D, pairs)
    out["quartets"] += np.uint64((n - 1) * (n - 2) * (n - 3) // 6) - seen
    return out


def mean(records):
    """a genome's mean delta (NaN with no quartet)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return records["sum"].astype(np.float64) / (records["quartets"].astype(np.float64) * float(ONE))
