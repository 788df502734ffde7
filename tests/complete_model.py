"""The contract of andi_hip_complete (include/andi_hip.h) in NumPy: missing distances from quartets.

Only D[i][j], i < j, is read; it is mirrored, the diagonal is +0.0.  A pair is known iff its entry is finite.  Rounds
t = 1, 2, ... read the matrix as it stood at the round's start (Jacobi).  For a missing pair i < j the candidates are the
unordered {k, l}, k != l, both outside {i, j}, with (i,k), (i,l), (j,k), (j,l), (k,l) all known:
c = max(D[i][k] + D[j][l], D[i][l] + D[j][k]) - D[k][l].  With a candidate and the least one m < +inf the pair is filled
with m <= 0 ? +0.0 : m, records its round and the number of candidates, and is known from the next round on.  The rounds
end after one that fills nothing or after max_rounds (0: no limit).  What stays missing is the quiet NaN."""
import numpy as np

FILL = np.dtype([("i", "<u4"), ("j", "<u4"), ("round", "<u4"), ("pad", "<u4"), ("quartets", "<u8"), ("value", "<f8")])
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def mirrored(D):
    """D as the call reads it: the upper triangle mirrored, a missing pair the quiet NaN, the diagonal +0.0"""
    D = np.asarray(D, np.float64)
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    v = D[iu].copy()
    v[~np.isfinite(v)] = QNAN
    M = np.zeros((n, n))
    M[iu] = v
    M.T[iu] = v
    return M


def candidates(M, i, j):
    """the least candidate of the pair (i, j) on the mirrored matrix M and the number of candidates; (None, 0) without one"""
    n = M.shape[0]
    ok = np.isfinite(M[i]) & np.isfinite(M[j])
    ok[i] = ok[j] = False
    K = np.nonzero(ok)[0]
    if len(K) < 2:
        return None, 0
    S = M[i, K][:, None] + M[j, K][None, :]  # S[k, l] = D[i][k] + D[j][l]
    sub = M[np.ix_(K, K)]
    valid = np.triu(np.isfinite(sub), 1)  # k < l, (k, l) known
    count = int(valid.sum())
    if count == 0:
        return None, 0
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.maximum(S, S.T) - sub
    return c[valid].min(), count


def candidates_loops(M, i, j):
    """the same by the plain triple loop of the contract's text"""
    n = M.shape[0]
    best, count = None, 0
    f = np.isfinite
    with np.errstate(over="ignore"):
        for k in range(n):
            for l in range(k + 1, n):
                if k in (i, j) or l in (i, j):
                    continue
                if f(M[i, k]) and f(M[i, l]) and f(M[j, k]) and f(M[j, l]) and f(M[k, l]):
                    c = max(M[i, k] + M[j, l], M[i, l] + M[j, k]) - M[k, l]
                    count += 1
                    if best is None or c < best:
                        best = c
    return best, count


def complete(D, max_rounds=0, cand=candidates):
    """(C, fills): the completed matrix and one FILL record per missing pair of D in row-major order"""
    M = mirrored(D)
    n = M.shape[0]
    I, J = np.nonzero(np.triu(~np.isfinite(M), 1))  # row-major
    fills = np.zeros(len(I), FILL)
    fills["i"], fills["j"], fills["value"] = I, J, QNAN
    t = 0
    while n >= 4 and (max_rounds == 0 or t < max_rounds):
        t += 1
        new = []
        for x in np.nonzero(fills["round"] == 0)[0]:
            m, count = cand(M, int(I[x]), int(J[x]))
            if count and m < np.inf:
                new.append((x, 0.0 if m <= 0.0 else m, count))
        for x, v, count in new:  # the round's fills are committed behind the round
            fills[x]["round"], fills[x]["quartets"], fills[x]["value"] = t, count, v
            M[I[x], J[x]] = M[J[x], I[x]] = v
        if not new:
            break
    return M, fills


# ---- additive matrices with dyadic branch lengths (every sum of the contract is exact on them)
def additive(rng, n, bits=6):
    """the leaf distances of a random binary tree on n leaves whose branch lengths are multiples of 2^-bits in (0, 1]"""
    parent, length = {}, {}
    nodes = list(range(n))
    nxt = n
    rng.shuffle(nodes)
    while len(nodes) > 1:
        a = nodes.pop(int(rng.integers(len(nodes))))
        b = nodes.pop(int(rng.integers(len(nodes))))
        for c in (a, b):
            parent[c] = nxt
            length[c] = float(rng.integers(1, 2 ** bits + 1)) / 2 ** bits
        nodes.append(nxt)
        nxt += 1
    root = nodes[0]

    def path(v):
        out = {v: 0.0}
        d = 0.0
        while v != root:
            d += length[v]
            v = parent[v]
            out[v] = d
        return out

    paths = [path(i) for i in range(n)]
    T = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            T[i, j] = T[j, i] = min(paths[i][v] + paths[j][v] for v in paths[i] if v in paths[j])
    return T


def punch(rng, T, frac):
    """T with a fraction of its pairs missing at random"""
    n = T.shape[0]
    iu = np.triu_indices(n, 1)
    hole = rng.random(len(iu[0])) < frac
    D = T.copy()
    D[iu[0][hole], iu[1][hole]] = np.nan
    D.T[iu[0][hole], iu[1][hole]] = np.nan
    return D


def separated(T, M, i, j):
    """is there a quartet {k, l} with its five distances known in M whose topology (by the true distances T) does not
    put i and j together -- ik|jl or il|jk: the sum d(i,j) + d(k,l) is then one of the two largest"""
    n = T.shape[0]
    f = np.isfinite
    for k in range(n):
        for l in range(k + 1, n):
            if k in (i, j) or l in (i, j):
                continue
            if f(M[i, k]) and f(M[i, l]) and f(M[j, k]) and f(M[j, l]) and f(M[k, l]):
                if T[i, j] + T[k, l] >= max(T[i, k] + T[j, l], T[i, l] + T[j, k]):
                    return True
    return False
