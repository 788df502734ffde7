"""NumPy restatement of refitting a tree's branch lengths by least squares (andi_hip_fit and andi_hip_relength,
include/andi_hip.h).  The tree, the edges and h(v, i) are place_model's; the classes of the leaves around an edge, the sums
in the contract's order -- of a (edge, b) over c > b ascending, then over b ascending --, the closed form of the lengths,
the two fits and the record are here.  fit() is vectorised over (edge, b) with a Python loop over c, so a few hundred
leaves take seconds; fit_loops() is the same contract as plain loops over Python floats, for small trees.  What
tests/test_fit_*.py hold the library to."""
import numpy as np

from place_model import paths

METHODS = ("ols",)
FIT = np.dtype([("rss", "<f8"), ("rss_joined", "<f8"), ("tss", "<f8"), ("length", "<f8"), ("length_joined", "<f8"),
                ("worst", "<f8"), ("pairs", "<u8"), ("negative", "<u4"), ("negative_joined", "<u4"), ("worst_b", "<i4"),
                ("worst_c", "<i4")])
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def relength(J, length):
    """the records with la, lb, lc replaced by length[child]"""
    out = np.array(J, copy=True)
    last = len(out) - 1
    for s in range(len(out)):
        out[s]["la"], out[s]["lb"] = length[int(out[s]["a"])], length[int(out[s]["b"])]
        if s == last:
            out[s]["lc"] = length[int(out[s]["c"])]
    return out


def classes(J):
    """(cls, size): cls[v, i] the class 0 ... 3 of leaf i around edge v, size[v, k] the number of leaves of class k"""
    J = np.asarray(J)
    n = len(J) + 2
    E = C = 2 * n - 3
    _, below, parent, _ = paths(J, n)
    cls = np.full((E, n), 3, np.int8)
    final = [int(J[n - 3][k]) for k in "abc"]
    for v in range(E):
        q = int(parent[v])
        if q == C:
            k2 = [x for x in final if x != v][0]
        else:
            k2 = [int(J[q - n][k]) for k in "ab" if int(J[q - n][k]) != v][0]
        k0 = v if v < n else int(J[v - n]["a"])
        cls[v, below[k2]] = 2
        cls[v, below[v]] = 1
        cls[v, below[k0]] = 0
    size = np.stack([(cls == k).sum(1) for k in range(4)], 1).astype(np.int64)
    return cls, size


def _solve(S, size, n):
    """the lengths of the 2n - 3 edges from S[xy][v] (PAIRS' order) and the classes' sizes"""
    with np.errstate(all="ignore"):
        m = {xy: S[k] / (size[:, xy[0]] * size[:, xy[1]]).astype(np.float64) for k, xy in enumerate(PAIRS)}
        n0, n1, n2, n3 = (size[:, k] for k in range(4))
        g = (n1 * n2 + n0 * n3).astype(np.float64) / ((n0 + n1) * (n2 + n3)).astype(np.float64)
        leaf = ((m[0, 2] + m[0, 3]) - m[2, 3]) * 0.5
        inner = ((g * (m[0, 2] + m[1, 3]) + (1.0 - g) * (m[1, 2] + m[0, 3])) - (m[0, 1] + m[2, 3])) * 0.5
    return np.where(np.arange(len(leaf)) < n, leaf, inner)


def lengths(J, D):
    """the refit lengths of the 2n - 3 edges"""
    J = np.asarray(J)
    n = len(J) + 2
    E = 2 * n - 3
    D = np.asarray(D, np.float64)
    cls, size = classes(J)
    s = np.zeros((4, E, n))
    with np.errstate(all="ignore"):
        for c in range(1, n):  # (every (v, b), b < c, takes D[b][c] into the sum of c's class: c ascending)
            d = D[:c, c][None, :]
            for k in range(4):
                s[k][:, :c] += np.where((cls[:, c] == k)[:, None], d, 0.0)
        S = np.zeros((6, E))
        for b in range(n):
            cb = cls[:, b]
            for k, (x, y) in enumerate(PAIRS):
                S[k] = S[k] + np.where(cb == x, s[y][:, b], np.where(cb == y, s[x][:, b], 0.0))
    return _solve(S, size, n)


def residuals(J, D):
    """R[b, c] = D[lo, hi] - p(lo, hi), lo < hi the two leaves, under the records' lengths: symmetric, the diagonal 0"""
    J = np.asarray(J)
    n = len(J) + 2
    E = 2 * n - 3
    H, below, parent, L = paths(J, n)
    with np.errstate(all="ignore"):
        T = np.where(below[:E], H[:E], H[parent])
        P = T[:n] + L[:n, None]  # row b is leaf b's own edge: p(b, c) = h(parent(b), c) + len(b)
        R = np.triu(np.asarray(D, np.float64) - P, 1)
    R = np.where(np.triu(np.ones((n, n), bool), 1), R, 0.0)
    return R + R.T


def _seq_sum(x):
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for a in x:
            s = s + a
    return s


def sums_of_squares(R):
    """(rss, leaf_ss) of the symmetric residuals"""
    n = len(R)
    rows, leaf = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        Q = R * R
        for j in range(n):
            leaf = leaf + np.where(np.arange(n) != j, Q[j], 0.0)
            rows[:j] = rows[:j] + Q[:j, j]
    return _seq_sum(rows), leaf


def total_ss(D):
    n = len(D)
    D = np.asarray(D, np.float64)
    rows = np.zeros(n)
    with np.errstate(all="ignore"):
        for c in range(1, n):
            rows[:c] = rows[:c] + D[:c, c]
        mean = _seq_sum(rows) / np.float64(n * (n - 1) // 2)
        rows = np.zeros(n)
        for c in range(1, n):
            d = D[:c, c] - mean
            rows[:c] = rows[:c] + d * d
    return _seq_sum(rows)


def worst_pair(R):
    """(b, c, r) of the greatest |r|, b < c, the first in (b, c) order, a NaN below every number; (-1, -1, nan) if all are"""
    n = len(R)
    up = np.triu(np.ones((n, n), bool), 1)
    A = np.abs(R)
    key = np.where(up, np.where(np.isnan(A), -1.0, A), -2.0)
    b, c = np.unravel_index(int(np.argmax(key)), key.shape)  # (the first of the greatest, in row-major order)
    if key[b, c] < 0:
        return -1, -1, np.float64("nan")
    return int(b), int(c), R[b, c]


def fit(J, D, method="ols", per=False):
    """(len, record) of the tree J and the matrix D; with per=True also leaf_ss and leaf_ss_joined"""
    assert method in METHODS
    J = np.asarray(J)
    n = len(J) + 2
    E = 2 * n - 3
    D = np.asarray(D, np.float64)
    length = lengths(J, D)
    joined = paths(J, n)[3]
    out = np.zeros(1, FIT)[0]
    Rf, Rj = residuals(relength(J, length), D), residuals(J, D)
    out["rss"], leaf = sums_of_squares(Rf)
    out["rss_joined"], leaf_joined = sums_of_squares(Rj)
    out["tss"] = total_ss(D)
    out["length"], out["length_joined"] = _seq_sum(length), _seq_sum(joined[:E])
    out["negative"], out["negative_joined"] = int((length < 0).sum()), int((joined[:E] < 0).sum())
    out["pairs"] = n * (n - 1) // 2
    out["worst_b"], out["worst_c"], out["worst"] = worst_pair(Rf)
    return (length, out, leaf, leaf_joined) if per else (length, out)


def r2(rec, joined=False):
    """1 - rss / tss; nan when tss is 0"""
    with np.errstate(all="ignore"):
        tss = np.float64(rec["tss"])
        return np.float64("nan") if tss == 0 else 1.0 - np.float64(rec["rss_joined" if joined else "rss"]) / tss


def fit_loops(J, D):
    """The same contract as plain loops: (len, rss, rss_joined, tss, leaf_ss, leaf_ss_joined, (worst_b, worst_c, worst))."""
    J = np.asarray(J)
    n = len(J) + 2
    E = 2 * n - 3
    D = np.asarray(D, np.float64)
    cls, size = classes(J)
    length = np.zeros(E)
    with np.errstate(all="ignore"):
        for v in range(E):
            S = {xy: np.float64(0.0) for xy in PAIRS}
            for b in range(n):
                s = [np.float64(0.0)] * 4
                for c in range(b + 1, n):
                    s[cls[v, c]] = s[cls[v, c]] + D[b, c]
                for x, y in PAIRS:
                    if cls[v, b] == x:
                        S[x, y] = S[x, y] + s[y]
                    elif cls[v, b] == y:
                        S[x, y] = S[x, y] + s[x]
            nk = [int(k) for k in size[v]]
            m = {(x, y): S[x, y] / np.float64(nk[x] * nk[y]) for x, y in PAIRS if nk[x] * nk[y] or v >= n}
            if v < n:
                length[v] = ((m[0, 2] + m[0, 3]) - m[2, 3]) * 0.5
            else:
                g = np.float64(nk[1] * nk[2] + nk[0] * nk[3]) / np.float64((nk[0] + nk[1]) * (nk[2] + nk[3]))
                length[v] = ((g * (m[0, 2] + m[1, 3]) + (1.0 - g) * (m[1, 2] + m[0, 3])) - (m[0, 1] + m[2, 3])) * 0.5

        def one(K):
            H, below, parent, L = paths(K, n)
            rss, leaf = np.float64(0.0), np.zeros(n)
            r = np.zeros((n, n))
            for b in range(n):
                inner = np.float64(0.0)
                for c in range(b + 1, n):
                    r[b, c] = r[c, b] = D[b, c] - (H[parent[b], c] + L[b])
                    inner = inner + r[b, c] * r[b, c]
                rss = rss + inner
            for i in range(n):
                for j in range(n):
                    if j != i:
                        leaf[i] = leaf[i] + r[i, j] * r[i, j]
            return rss, leaf, r

        rss, leaf, r = one(relength(J, length))
        rss_joined, leaf_joined, _ = one(J)
        total = np.float64(0.0)
        for b in range(n):
            inner = np.float64(0.0)
            for c in range(b + 1, n):
                inner = inner + D[b, c]
            total = total + inner
        mean = total / np.float64(n * (n - 1) // 2)
        tss = np.float64(0.0)
        for b in range(n):
            inner = np.float64(0.0)
            for c in range(b + 1, n):
                inner = inner + (D[b, c] - mean) * (D[b, c] - mean)
            tss = tss + inner
    worst = (-1, -1, np.float64("nan"))
    for b in range(n):
        for c in range(b + 1, n):
            if not np.isnan(r[b, c]) and (worst[0] < 0 or abs(r[b, c]) > abs(worst[2])):
                worst = (b, c, r[b, c])
    return length, rss, rss_joined, tss, leaf, leaf_joined, worst
