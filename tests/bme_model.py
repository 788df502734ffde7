"""NumPy restatement of refining a tree by balanced nearest-neighbor interchanges (andi_hip_refine, include/andi_hip.h):
the tree rooted at the centre with fixed node ids, the table A of balanced leaf-to-subtree averages, the sums S in the
order of a wavefront's lanes (64 partial sums by c mod 64, then the lanes in order), the six averages around an inner
edge, the gains, the rounds, the balanced lengths and the canonical numbering of the result.  refine() is vectorised over
the leaves (the nodes and the 64-leaf words are Python loops); refine_loops() is the same contract as recursion and
plain loops over Python floats, for small trees; pauplin_length() is Pauplin's formula by brute force over the leaf
pairs.  What tests/test_refine_*.py hold the library to."""
import numpy as np

METHODS = ("bnni",)
REFINE = np.dtype([("length_before", "<f8"), ("length_after", "<f8"), ("moves", "<u8"), ("converged", "<i4"), ("pad", "<i4")])
MOVE = np.dtype([("gain", "<f8"), ("first", "<i4"), ("second", "<i4")])
NJ_JOIN = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"), ("lc", "<f8")])


# ---------------------------------------------------------------- the tree
def start(J):
    """(par, kid) of the records: par[v] for the 2n - 3 non-centre nodes; kid[q - n] the children of inner node q in slot
    order (-1 in the third slot but for the centre C = 2n - 3, which is kid[n - 3])"""
    J = np.asarray(J)
    n = len(J) + 2
    C = 2 * n - 3
    par = np.full(C, -1, np.int64)
    kid = np.full((n - 2, 3), -1, np.int64)
    for s in range(n - 2):
        last = s == n - 3
        node = C if last else n + s
        for k, f in enumerate("abc"[:3 if last else 2]):
            v = int(J[s][f])
            assert 0 <= v < min(n + s, C) and par[v] == -1
            par[v], kid[s][k] = node, v
    assert (par >= 0).all()
    return par, kid


def others(kid, n, q, v):
    """the children of q but v, in slot order"""
    return [int(x) for x in kid[q - n] if x >= 0 and x != v]


def bfs(par, kid, n):
    """(order, lev): the non-centre nodes breadth-first from the centre, children in slot order; lev the edges from C"""
    C = 2 * n - 3
    lev = np.zeros(C + 1, np.int64)
    order = [int(x) for x in kid[n - 3]]
    for x in order:
        lev[x] = 1
    head = 0
    while head < len(order):
        x = order[head]
        head += 1
        if x >= n:
            for y in kid[x - n][:2]:
                lev[y] = lev[x] + 1
                order.append(int(y))
    assert len(order) == C
    return order, lev


def leaf_sets(kid, n, order):
    """below[v, c]: leaf c lies below node v (a leaf lies below itself)"""
    C = 2 * n - 3
    below = np.zeros((C, n), bool)
    below[np.arange(n), np.arange(n)] = True
    for x in reversed(order):
        if x >= n:
            below[x] = below[kid[x - n][0]] | below[kid[x - n][1]]
    return below


def rows(par, kid, n):
    """R[x, k]: the row of A that sum k of node x is taken against (-1: none) -- the sibling, the parent's row, the uncle,
    the grandparent's row; where the parent (grandparent) is C, the other two children of C in slot order instead"""
    C = 2 * n - 3
    R = np.full((C, 4), -1, np.int64)
    for x in range(C):
        p = int(par[x])
        if p == C:
            o = others(kid, n, C, x)
            R[x, :2] = o
            continue
        R[x, 0], R[x, 1] = others(kid, n, p, x)[0], p
        g = int(par[p])
        if g == C:
            R[x, 2:] = others(kid, n, C, p)
        else:
            R[x, 2], R[x, 3] = others(kid, n, g, p)[0], g
    return R


def apply_move(par, kid, n, v, alt):
    """re-hang in place: alternative 0 swaps v's second child with s, 1 the first; returns (outgoing, incoming)"""
    q = int(par[v])
    s = others(kid, n, q, v)[0]
    o = int(kid[v - n][1 - alt])
    kid[v - n][1 - alt] = s
    kq = kid[q - n]
    kq[list(kq).index(s)] = o
    par[s], par[o] = v, q
    return o, s


def canonical(par, kid, length, n):
    """the records of the tree in the output numbering: the centre the final record, children visited in order of their
    least leaf, inner nodes n, n + 1, ... in post-order, a pair record's smaller id first, the final record's ascending"""
    C = 2 * n - 3
    order, _ = bfs(par, kid, n)
    least = np.arange(C + 1)
    for x in reversed(order):
        if x >= n:
            least[x] = min(least[kid[x - n][0]], least[kid[x - n][1]])
    new = np.arange(C + 1)
    J = np.zeros(n - 2, NJ_JOIN)
    nxt = 0
    stack = [(C, 0)]
    while stack:
        x, k = stack.pop()
        ch = sorted((int(y) for y in kid[x - n] if y >= 0), key=lambda y: least[y])
        while k < len(ch) and ch[k] < n:
            k += 1
        if k < len(ch):
            stack.append((x, k + 1))
            stack.append((ch[k], 0))
            continue
        ids = sorted((int(new[y]), float(length[y])) for y in ch)
        if x == C:
            J[n - 3] = (ids[0][0], ids[1][0], ids[2][0], 0, ids[0][1], ids[1][1], ids[2][1])
        else:
            new[x] = n + nxt
            J[nxt] = (ids[0][0], ids[1][0], -1, 0, ids[0][1], ids[1][1], 0.0)
            nxt += 1
    return J


def perturb(J, rng, count, lengths=None):
    """the records after `count` random interchanges (a random inner edge, a random alternative), renumbered"""
    J = np.asarray(J)
    n = len(J) + 2
    par, kid = start(J)
    for _ in range(count if n > 3 else 0):
        apply_move(par, kid, n, int(rng.integers(n, 2 * n - 3)), int(rng.integers(2)))
    return canonical(par, kid, np.full(2 * n - 3, 0.05) if lengths is None else lengths, n)


def mirrored(D):
    D = np.asarray(D, np.float64)
    U = np.triu(D, 1)
    return U + U.T  # (the diagonal +0.0)


# ---------------------------------------------------------------- one round, vectorised over the leaves
def table(Dm, par, kid, n, order, below):
    """A[v, c] for the 2n - 3 non-centre nodes v"""
    C = 2 * n - 3
    A = np.zeros((C, n))
    A[:n] = Dm
    with np.errstate(all="ignore"):
        for x in reversed(order):  # the far side below x: children first
            if x >= n:
                a, b = kid[x - n][:2]
                A[x] = np.where(below[x], A[x], (A[a] + A[b]) * 0.5)
        for v in order:  # the far side above v: parents first
            q = int(par[v])
            o = others(kid, n, q, v)
            val = (A[o[0]] + A[o[1]]) * 0.5 if q == C else (A[o[0]] + A[q]) * 0.5
            A[v] = np.where(below[v], val, A[v])
    return A


def weights(lev, below, n):
    """w[x, c] = 2^-(lev(c) - lev(x)) for c below x, 0 once the exponent passes 1022"""
    e = np.where(below, lev[None, :n] - lev[:len(below), None], 0)
    return np.where(e > 1022, 0.0, np.ldexp(1.0, -np.minimum(e, 1022).astype(np.int64)))


def sums(A, below, lev, R, n):
    """T[x, k] = S(x, R[x, k]): 64 partial sums by c mod 64, c ascending, then the partial sums in order"""
    E = len(A)
    W = (n + 63) // 64
    w = weights(lev, below, n)
    T = np.zeros((E, 4))
    with np.errstate(all="ignore"):
        for k in range(4):
            M = np.zeros((E, W * 64))
            M[:, :n] = np.where(below & (R[:, k] >= 0)[:, None], w * A[np.maximum(R[:, k], 0)], 0.0)
            M = M.reshape(E, W, 64)
            p = np.zeros((E, 64))
            for i in range(W):
                p = p + M[:, i]
            t = np.zeros(E)
            for lane in range(64):
                t = t + p[:, lane]
            T[:, k] = t
    return T


def between(T, R, x, r):
    """S(x, r) from the table of sums"""
    k = list(R[x]).index(r)
    return T[x, k]


def six(T, R, par, kid, n, v):
    """(d_ab, d_as, d_bs, d_au, d_bu, d_su) of the inner edge v"""
    C = 2 * n - 3
    a, b = (int(x) for x in kid[v - n][:2])
    q = int(par[v])
    o = others(kid, n, q, v)
    d_su = between(T, R, o[0], o[1]) if q == C else T[o[0], 1]
    return T[a, 0], T[a, 2], T[b, 2], T[a, 3], T[b, 3], d_su


def gains(T, R, par, kid, n):
    """g[v - n, alternative] of the n - 3 inner edges"""
    g = np.zeros((n - 3, 2))
    with np.errstate(all="ignore"):
        for v in range(n, 2 * n - 3):
            d_ab, d_as, d_bs, d_au, d_bu, d_su = six(T, R, par, kid, n, v)
            g[v - n, 0] = ((d_ab + d_su) - (d_as + d_bu)) * 0.25
            g[v - n, 1] = ((d_ab + d_su) - (d_bs + d_au)) * 0.25
    return g


def lengths(T, R, par, kid, n):
    """the balanced length of every edge"""
    C = 2 * n - 3
    L = np.zeros(C)
    with np.errstate(all="ignore"):
        for v in range(C):
            if v >= n:
                d_ab, d_as, d_bs, d_au, d_bu, d_su = six(T, R, par, kid, n, v)
                L[v] = ((d_as + d_au) + (d_bs + d_bu)) * 0.25 - (d_ab + d_su) * 0.5
                continue
            q = int(par[v])
            o = others(kid, n, q, v)
            d_su = between(T, R, o[0], o[1]) if q == C else T[o[0], 1]
            L[v] = ((T[v, 0] + T[v, 1]) - d_su) * 0.5
    return L


def best(g):
    """(index, gain) of the greatest gain in (v, alternative) order, ties to the first, a NaN below every number"""
    flat = g.ravel()
    if not len(flat):
        return -1, np.float64("nan")
    ok = ~np.isnan(flat)
    if not ok.any():
        return 0, flat[0]
    top = flat[ok].max()
    return int(np.nonzero(ok & (flat == top))[0][0]), top


def seq_sum(x):
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for a in x:
            s = s + a
    return s


def evaluate(Dm, par, kid, n):
    """one round's (T, R, order, below) of the tree as it stands"""
    order, lev = bfs(par, kid, n)
    below = leaf_sets(kid, n, order)
    A = table(Dm, par, kid, n, order, below)
    R = rows(par, kid, n)
    return sums(A, below, lev, R, n), R, below


def _search(J, D, tol, max_moves, evaluate):
    J = np.asarray(J)
    n = len(J) + 2
    assert n >= 3 and tol >= 0
    max_moves = 10 * n if max_moves is None else max_moves
    Dm = mirrored(D)
    par, kid = start(J)
    res = np.zeros(1, REFINE)[0]
    log = []
    first = None
    while True:
        T, R, below = evaluate(Dm, par, kid, n)
        L = lengths(T, R, par, kid, n)
        if first is None:
            first = L
        at, gain = best(gains(T, R, par, kid, n))
        if not gain > tol:
            res["converged"] = 1
            break
        if len(log) >= max_moves:
            res["converged"] = 0
            break
        o, s = apply_move(par, kid, n, n + at // 2, at % 2)
        log.append((gain, int(np.nonzero(below[o])[0][0]), int(np.nonzero(below[s])[0][0])))
    res["length_before"], res["length_after"], res["moves"] = seq_sum(first), seq_sum(L), len(log)
    return canonical(par, kid, L, n), res, np.array(log, MOVE)


def refine(J, D, tol=0.0, max_moves=None):
    """(records, result, log) of the search from the tree J on the matrix D"""
    return _search(J, D, tol, max_moves, evaluate)


# ---------------------------------------------------------------- the same contract as recursion and plain loops
def evaluate_loops(Dm, par, kid, n):
    C = 2 * n - 3
    order, lev = bfs(par, kid, n)
    leaves = {}

    def under(v):
        if v not in leaves:
            leaves[v] = [v] if v < n else sorted(under(int(kid[v - n][0])) + under(int(kid[v - n][1])))
        return leaves[v]

    memo = {}

    def A(v, c):
        if (v, c) not in memo:
            if c not in under(v):
                memo[v, c] = Dm[v, c] if v < n else (A(int(kid[v - n][0]), c) + A(int(kid[v - n][1]), c)) * 0.5
            else:
                q = int(par[v])
                o = others(kid, n, q, v)
                memo[v, c] = (A(o[0], c) + A(o[1], c)) * 0.5 if q == C else (A(o[0], c) + A(q, c)) * 0.5
        return memo[v, c]

    def S(x, r):
        p = [np.float64(0.0)] * 64
        for c in under(x):
            e = int(lev[c] - lev[x])
            w = np.float64(0.0) if e > 1022 else np.float64(2.0) ** -e
            p[c % 64] = p[c % 64] + w * A(r, c)
        t = np.float64(0.0)
        for lane in range(64):
            t = t + p[lane]
        return t

    R = rows(par, kid, n)
    T = np.zeros((C, 4))
    below = np.zeros((C, n), bool)
    with np.errstate(all="ignore"):
        for x in range(C):
            below[x, under(x)] = True
            for k in range(4):
                if R[x, k] >= 0:
                    T[x, k] = S(x, int(R[x, k]))
    return T, R, below


def refine_loops(J, D, tol=0.0, max_moves=None):
    return _search(J, D, tol, max_moves, evaluate_loops)


# ---------------------------------------------------------------- Pauplin's formula
def hops(J):
    """tau[i, j]: the edges on the path between leaves i and j"""
    J = np.asarray(J)
    n = len(J) + 2
    par, _ = start(J)
    C = 2 * n - 3
    up = []
    for i in range(n):
        d, v, seen = 0, i, {}
        while v != C:
            seen[v] = d
            v, d = int(par[v]), d + 1
        seen[C] = d
        up.append(seen)
    tau = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            v, d = j, 0
            while v not in up[i]:
                v, d = int(par[v]), d + 1
            tau[i, j] = tau[j, i] = d + up[i][v]
    return tau


def pauplin_length(J, D):
    """the sum over i < j of 2^(1 - tau(i, j)) D[i][j]"""
    tau = hops(J)
    n = len(tau)
    iu = np.triu_indices(n, 1)
    return float(np.sum(np.ldexp(np.asarray(D, np.float64)[iu], 1 - tau[iu])))


def inner_splits(J):
    """the inner branches of the records as frozensets of leaves, on the side without leaf 0"""
    J = np.asarray(J)
    n = len(J) + 2
    par, kid = start(J)
    below = leaf_sets(kid, n, bfs(par, kid, n)[0])
    out = set()
    for v in range(n, 2 * n - 3):
        s = frozenset(np.nonzero(below[v])[0].tolist())
        out.add(frozenset(range(n)) - s if 0 in s else s)
    return out
