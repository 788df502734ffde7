"""NumPy restatement of distance-based placement on a neighbor-joining tree (andi_hip_place, include/andi_hip.h): the
tree's edges, the path lengths h(v, i), the two passes over the leaves in ascending order with every operation rounded on
its own, the constrained solve and the choice of the edge.  Vectorised over (query, edge); the leaves are a Python loop,
so every sum is the sequential one of the contract.  What tests/test_place_*.py hold the library to."""
import numpy as np

METHODS = {"ols": 0, "fm": 1}
PLACEMENT = np.dtype([("edge", "<i4"), ("used", "<u4"), ("distal", "<f8"), ("pendant", "<f8"), ("err", "<f8")])
INF = float("inf")


def edges(J, n):
    """(parent, length) of the 2n - 3 edges: edge v joins node v to parent[v]; the centre is node 2n - 3"""
    E = 2 * n - 3
    parent = np.full(E, -1, np.int64)
    length = np.zeros(E)
    for s in range(n - 2):
        last = s == n - 3
        node = E if last else n + s
        for c, l in (("a", "la"), ("b", "lb"), ("c", "lc"))[:3 if last else 2]:
            v = int(J[s][c])
            assert 0 <= v < node and parent[v] == -1
            parent[v], length[v] = node, float(J[s][l])
    assert (parent >= 0).all()
    return parent, length


def paths(J, n):
    """(H, below, parent, length): H[v, i] = h(v, i) for the 2n - 2 nodes, below[v, i] iff v lies on i's path to the centre"""
    parent, length = edges(J, n)
    E = 2 * n - 3
    H = np.zeros((E + 1, n))
    below = np.zeros((E + 1, n), bool)
    for i in range(n):
        v, h = i, np.float64(0.0)
        while True:
            H[v, i], below[v, i] = h, True
            if v == E:
                break
            h = h + length[v]
            v = parent[v]
    for c in range(E - 1, -1, -1):
        H[c] = np.where(below[c], H[c], H[parent[c]] + length[c])
    return H, below, parent, length


def _less(a, b):
    """a orders before b: by value, a NaN after every number"""
    return (a < b) | (~np.isnan(a) & np.isnan(b))


def place(J, D, method="fm", per=False):
    """The placements of the rows of D (nq, n) on the tree J (n - 2 records): a PLACEMENT array, and with per=True also
    the (nq, 2n - 3) arrays err, x, p of every edge."""
    J = np.asarray(J)
    n = len(J) + 2
    D = np.ascontiguousarray(D, np.float64).reshape(-1, n)
    nq, E = D.shape[0], 2 * n - 3
    fm = METHODS[method] == 1
    H, below, parent, L = paths(J, n)
    below = below[:E]
    T = np.where(below, H[:E], H[parent])  # the endpoint each leaf is measured from
    Lc = np.where(L > 0, L, 0.0)
    usable = np.isfinite(D)
    with np.errstate(all="ignore"):
        w = 1.0 / (D * D) if fm else np.ones_like(D)
        WA, UA, WB, UB = (np.zeros((nq, E)) for _ in range(4))
        for i in range(n):
            d, ok, wi, b = D[:, i, None], usable[:, i, None], w[:, i, None], below[None, :, i]
            u1 = d - T[None, :, i]
            WA += np.where(ok & b, wi, 0.0)
            UA += np.where(ok & b, wi * u1, 0.0)
            WB += np.where(ok & ~b, wi, 0.0)
            UB += np.where(ok & ~b, wi * (u1 - L[None, :]), 0.0)
        cand = ~((WA == 0.0) | (WB == 0.0))
        s, t, W = UA / WA, UB / WB, WA + WB
        p0, x0 = (s + t) * 0.5, (s - t) * 0.5
        free = (p0 >= 0) & (x0 >= 0) & (x0 <= Lc)
        zero = np.zeros((nq, E))
        LcB = np.broadcast_to(Lc, (nq, E))

        def pos(a):
            return np.where(a > 0, a, 0.0)

        def clamp(a):
            return np.where(a > 0, np.where(a < LcB, a, LcB), 0.0)

        def delta(p, x):
            e, f = (p + x) - s, (p - x) - t
            return WA * (e * e) + WB * (f * f)

        cands = [(pos(((WA * s) + (WB * t)) / W), zero),
                 (pos(((WA * (s - LcB)) + (WB * (t + LcB))) / W), LcB),
                 (zero, clamp(((WA * s) - (WB * t)) / W))]
        p, x = cands[0]
        best = delta(p, x)
        for cp, cx in cands[1:]:
            dl = delta(cp, cx)
            take = _less(dl, best)
            p, x, best = np.where(take, cp, p), np.where(take, cx, x), np.where(take, dl, best)
        p, x = np.where(free, p0, p), np.where(free, x0, x)
        px, pl = p + x, p + (L[None, :] - x)
        err = np.zeros((nq, E))
        for i in range(n):
            d, ok, wi, b = D[:, i, None], usable[:, i, None], w[:, i, None], below[None, :, i]
            r = d - np.where(b, px + T[None, :, i], pl + T[None, :, i])
            err += np.where(ok, wi * (r * r), 0.0)
    err = np.where(cand, err, INF)
    x, p = np.where(cand, x, 0.0), np.where(cand, p, 0.0)
    out = np.zeros(nq, PLACEMENT)
    for q in range(nq):
        out[q]["used"] = int(usable[q].sum())
        at = np.nonzero(usable[q] & (D[q] == 0.0))[0] if fm else []
        if len(at):  # the query IS that leaf
            err[q], x[q], p[q] = INF, 0.0, 0.0
            err[q, at[0]] = 0.0
        key = np.where(np.isnan(err[q]), INF, err[q])
        v = int(np.argmin(key))  # (the first of the least: ties to the smaller edge)
        if key[v] == INF:  # +inf or NaN: nowhere
            out[q]["edge"], out[q]["distal"], out[q]["pendant"], out[q]["err"] = -1, 0.0, 0.0, INF
        else:
            out[q]["edge"], out[q]["distal"], out[q]["pendant"], out[q]["err"] = v, x[q, v], p[q, v], err[q, v]
    return (out, err, x, p) if per else out


def random_tree(rng, n, lengths=None):
    """n - 2 records of the shape andi_hip_nj gives (a random joining order, a < b, x < y < z), lengths from lengths(k)
    (default: uniform in [0.01, 0.1))"""
    from andi_amd.lib import NJ_JOIN
    if lengths is None:
        def lengths(k):
            return rng.uniform(0.01, 0.1, k)
    J = np.zeros(n - 2, NJ_JOIN)
    active = list(range(n))
    for s in range(n - 3):
        i, j = sorted(rng.choice(len(active), 2, replace=False).tolist())
        a, b = active[i], active[j]
        la, lb = lengths(2)
        J[s] = (a, b, -1, 0, la, lb, 0.0)
        del active[j], active[i]
        active.append(n + s)
    la, lb, lc = lengths(3)
    J[n - 3] = (active[0], active[1], active[2], 0, la, lb, lc)
    return J


def caterpillar(n, lengths):
    """leaf 0 and 1 joined, then every next leaf with the node before; lengths: 2n - 3 values in record order"""
    from andi_amd.lib import NJ_JOIN
    J = np.zeros(n - 2, NJ_JOIN)
    it = iter(lengths)
    top = 0
    for s in range(n - 3):
        a, b = (0, 1) if s == 0 else (s + 1, top)
        J[s] = (a, b, -1, 0, next(it), next(it), 0.0)
        top = n + s
    x, y, z = sorted(((0, 1, 2) if n == 3 else (n - 2, n - 1, top)))
    J[n - 3] = (x, y, z, 0, next(it), next(it), next(it))
    return J


def balanced(n, lengths):
    """the active nodes joined in pairs, round after round, until three are left"""
    from andi_amd.lib import NJ_JOIN
    J = np.zeros(n - 2, NJ_JOIN)
    it = iter(lengths)
    active, s = list(range(n)), 0
    while len(active) > 3:
        a, b = active[0], active[1]
        J[s] = (a, b, -1, 0, next(it), next(it), 0.0)
        active = active[2:] + [n + s]
        s += 1
    J[n - 3] = (active[0], active[1], active[2], 0, next(it), next(it), next(it))
    return J


def point_distances(J, n, v, x, p):
    """the tree distances to the n leaves of a point hanging by a branch of length p from edge v, x above its child end"""
    H, below, parent, L = paths(J, n)
    return np.where(below[v], (p + x) + H[v], (p + (L[v] - x)) + H[parent[v]])
