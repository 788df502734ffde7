"""NumPy restatement of refining a tree by balanced subtree pruning and regrafting (andi_hip_refine_spr,
include/andi_hip.h): the tree as three neighbour slots per inner node, rooted at the centre again every round; the table
B of balanced averages between the sides of two edges, built by A's recursion with an edge where the leaf was; the gain
of every (pruned side, target edge) pair with its running value R; the order of the candidates; the move in the slots.
The tree, A, the sums and the balanced lengths are tests/bme_model.py's.  refine_spr() is vectorised over the pruned
sides: a step a -> b of the tree carries, for every pruned side that reaches it, the hops and R so far, and the steps are
taken child-to-parent the deepest first, then parent-to-child from the centre.  refine_spr_loops() is the same contract as
a depth-first walk per pruned side over Python floats, for small trees.  rehung() gives the records after one move, for
the brute-force check against Pauplin's length.  What tests/test_spr_*.py hold the library to."""
import numpy as np

import bme_model as bm

SPR_MOVE = np.dtype([("gain", "<f8"), ("first", "<i4"), ("second", "<i4"), ("hops", "<i4"), ("pad", "<i4")])


# ---------------------------------------------------------------- the tree in slots
def slots_of(J):
    """nb[q - n]: the three neighbours of inner node q -- a, b and the parent for a pair record's node, a, b, c for C"""
    par, kid = bm.start(J)
    n = len(kid) + 2
    nb = kid.copy()
    for q in range(n, 2 * n - 3):
        nb[q - n][2] = par[q]
    return nb


def orient(nb, n):
    """(par, kid) of the slots rooted at C: the children of a node are its neighbours but its parent, in slot order"""
    C = 2 * n - 3
    par = np.full(C, -1, np.int64)
    kid = np.full((n - 2, 3), -1, np.int64)
    kid[n - 3] = nb[n - 3]
    queue = [int(x) for x in nb[n - 3]]
    for x in queue:
        par[x] = C
    for x in queue:
        if x >= n:
            ch = [int(y) for y in nb[x - n] if y != par[x]]
            assert len(ch) == 2
            kid[x - n][:2] = ch
            for y in ch:
                par[y] = x
                queue.append(y)
    assert len(queue) == C
    return par, kid


def beyond(par, kid, n, v, frm):
    """the two neighbours of inner node v but frm"""
    nbrs = [int(x) for x in kid[v - n] if x >= 0] + ([int(par[v])] if v != 2 * n - 3 else [])
    out = [x for x in nbrs if x != frm]
    assert len(out) == 2
    return out


def edge_of(par, n, a, b):
    """the edge between the adjacent nodes a and b: its lower node"""
    return b if b != 2 * n - 3 and par[b] == a else a


def pruned(par, kid, n):
    """the pruned sides in the contract's order: (u, side, x, v0) -- edge u, 0 its lower and 1 its upper side"""
    for u in range(2 * n - 3):
        yield u, 0, u, int(par[u])
        if u >= n:
            yield u, 1, int(par[u]), u


def apply_spr(nb, n, x, v0, q, vk, w):
    """the move in the slots, in place"""
    def slot(i, t):
        return (i - n, list(nb[i - n]).index(t))

    p = [int(y) for y in nb[v0 - n] if y != x and y != q]
    assert len(p) == 1
    p = p[0]
    writes = [(slot(v0, p), vk), (slot(v0, q), w), (slot(vk, w), v0)]
    if p >= n:
        writes.append((slot(p, v0), q))
    if q >= n:
        writes.append((slot(q, v0), p))
    if w >= n:
        writes.append((slot(w, vk), v0))
    assert len({at for at, _ in writes}) == len(writes)
    for at, value in writes:
        nb[at] = value


def rehung(J, x, v0, q, vk, w, length=None):
    """the records after the one move, renumbered"""
    n = len(J) + 2
    nb = slots_of(J)
    apply_spr(nb, n, x, v0, q, vk, w)
    par, kid = orient(nb, n)
    return bm.canonical(par, kid, np.zeros(2 * n - 3) if length is None else length, n)


def least_of_side(below, par, n, a, b):
    """the least leaf on b's side of the edge between the adjacent nodes a and b"""
    if b != 2 * n - 3 and par[b] == a:
        return int(np.nonzero(below[b])[0][0])
    return int(np.nonzero(~below[a])[0][0])


# ---------------------------------------------------------------- B
def ancestors(par, n, order):
    """anc[x, y]: y lies below x or is x, for the 2n - 3 non-centre nodes"""
    C = 2 * n - 3
    anc = np.eye(C, dtype=bool)
    for x in reversed(order):
        if par[x] != C:
            anc[par[x]] |= anc[x]
    return anc


def pairs(A, par, kid, n, order, anc):
    """B[e, f] for all edges: A's recursion with the column f an edge"""
    C = 2 * n - 3
    B = np.zeros((C, C))
    B[:n] = A.T
    with np.errstate(all="ignore"):
        for x in reversed(order):  # the far side below x: children first
            if x >= n:
                a, b = kid[x - n][:2]
                B[x] = np.where(anc[x], B[x], (B[a] + B[b]) * 0.5)
        for v in order:  # the far side above v: parents first
            q = int(par[v])
            o = bm.others(kid, n, q, v)
            val = (B[o[0]] + B[o[1]]) * 0.5 if q == C else (B[o[0]] + B[q]) * 0.5
            B[v] = np.where(anc[v], val, B[v])
    return B


def pairs_loops(A, par, kid, n):
    C = 2 * n - 3

    def has(x, y):
        while y != C and y != x:
            y = int(par[y])
        return y == x

    memo = {}

    def B(e, f):
        if (e, f) not in memo:
            if not has(e, f):
                memo[e, f] = A[f, e] if e < n else (B(int(kid[e - n][0]), f) + B(int(kid[e - n][1]), f)) * 0.5
            else:
                q = int(par[e])
                o = bm.others(kid, n, q, e)
                memo[e, f] = (B(o[0], f) + B(o[1], f)) * 0.5 if q == C else (B(o[0], f) + B(q, f)) * 0.5
        return memo[e, f]

    out = np.zeros((C, C))
    with np.errstate(all="ignore"):
        for e in range(C):
            for f in range(C):
                out[e, f] = B(e, f)
    return out


# ---------------------------------------------------------------- the gains
def _gain(h, dXY0, dXW, dYW, dXZ, dYZ, Bff, R):
    t1 = (0.5 * (1.0 - h)) * (dXY0 - dXZ)
    t2 = 0.5 * dXW - (0.5 * h) * dXZ
    t3 = 0.5 * dYW - (0.5 * h) * dYZ
    t4 = 0.5 * Bff - (0.25 * h) * (dYZ + dXZ)
    return (((t1 + t2) - t3) + t4) - 0.25 * R


def _pow2(k):
    """2^-k, +0.0 once k > 1022"""
    k = np.asarray(k)
    return np.where(k > 1022, 0.0, np.ldexp(1.0, -np.minimum(k, 1022).astype(np.int64)))


def candidates_loops(B, par, kid, n):
    """every candidate by a depth-first walk: a list of (gain, u, side, f, x, v0, q, vk, w, k) in the contract's order"""
    out = []
    with np.errstate(all="ignore"):
        for u, side, x, v0 in pruned(par, kid, n):
            found = []
            o = beyond(par, kid, n, v0, x)
            for q, p in ((o[0], o[1]), (o[1], o[0])):
                ep, e1 = edge_of(par, n, v0, p), edge_of(par, n, v0, q)
                stack = [(q, v0, np.float64(0.0), 0)]
                while stack:
                    v, frm, Rp, k = stack.pop()
                    if v < n:
                        continue
                    k += 1
                    h = np.float64(0.0) if k > 1022 else np.float64(2.0) ** -k
                    a, b = beyond(par, kid, n, v, frm)
                    for w, y in ((a, b), (b, a)):
                        f = edge_of(par, n, v, w)
                        R = 0.5 * Rp + B[u, edge_of(par, n, v, y)]
                        g = _gain(h, B[u, ep], B[u, e1], B[ep, e1], B[u, f], B[ep, f], B[f, f], R)
                        found.append((g, u, side, f, x, v0, q, v, w, k))
                        stack.append((w, v, R, k))
            out += sorted(found, key=lambda c: c[3])
    return out


def candidates(B, par, kid, n, order):
    """the same list, vectorised over the pruned sides s = 2 u + side.  A step a -> b goes by the side it enters,
    t = 2 b (b below a) or 2 a + 1 (b above a); K[t, s], R[t, s]: the hops and the running value with which pruned side s
    evaluates the edge (a, b) as its target (K = 0: (a, b) is the edge the path leaves v0 by; -1: s does not come here);
    EP[t, s], E1[t, s]: the edges of Y0 and W1 of that walk."""
    C = 2 * n - 3
    K = np.full((2 * C, 2 * C), -1, np.int64)
    R = np.zeros((2 * C, 2 * C))
    EP = np.zeros((2 * C, 2 * C), np.int64)
    E1 = np.zeros((2 * C, 2 * C), np.int64)
    ex = np.arange(2 * C) >> 1

    def entered(a, b):
        return 2 * b if b != C and par[b] == a else 2 * a + 1

    steps = [(x, int(par[x])) for x in reversed(order) if x >= n] + [(int(par[x]), x) for x in order]
    with np.errstate(all="ignore"):
        for a, b in steps:  # (a is inner)
            t = entered(a, b)
            c1, c2 = beyond(par, kid, n, a, b)
            for c, y in ((c1, c2), (c2, c1)):
                ey = edge_of(par, n, a, y)
                if c >= n:  # the walks that came to a from c go on
                    tp = entered(c, a)
                    on = K[tp] >= 0
                    K[t, on] = K[tp, on] + 1
                    R[t, on] = 0.5 * R[tp, on] + B[ex[on], ey]
                    EP[t, on], E1[t, on] = EP[tp, on], E1[tp, on]
                s = entered(a, c)  # the side beyond c is pruned: v0 = a, the path leaves by b, Y0 lies beyond y
                K[t, s], R[t, s], EP[t, s], E1[t, s] = 0, 0.0, ey, edge_of(par, n, a, b)
        G = np.full((2 * C, C), np.nan)
        ok = np.zeros((2 * C, C), bool)
        for a, b in steps:
            t = entered(a, b)
            f = edge_of(par, n, a, b)
            on = np.nonzero(K[t] >= 1)[0]
            e, ep, e1 = ex[on], EP[t, on], E1[t, on]
            G[on, f] = _gain(_pow2(K[t, on]), B[e, ep], B[e, e1], B[ep, e1], B[e, f], B[ep, f], B[f, f], R[t, on])
            ok[on, f] = True
    return G, ok, K


def best(G, ok):
    """(s, f) of the greatest gain in (s, f) order, ties to the first, a NaN below every number; None: no candidate"""
    if not ok.any():
        return None
    num = ok & ~np.isnan(G)
    if not num.any():
        s, f = np.argwhere(ok)[0]
        return int(s), int(f)
    top = G[num].max()
    s, f = np.argwhere(num & (G == top))[0]
    return int(s), int(f)


def best_loops(cands):
    top = None
    for c in cands:  # (in the contract's order: on a tie the earlier one stays)
        if top is None or (np.isnan(top[0]) and not np.isnan(c[0])) or c[0] > top[0]:
            top = c
    return top


def move_of(par, kid, n, K, s, f):
    """(x, v0, q, vk, w, k) of the candidate (pruned side s, target edge f)"""
    C = 2 * n - 3
    u, side = s >> 1, s & 1
    x, v0 = (int(par[u]), u) if side else (u, int(par[u]))
    lower, upper = f, int(par[f])
    t = 2 * f if K[2 * f, s] >= 1 else 2 * f + 1  # the target is entered downwards or upwards
    vk, w = (upper, lower) if t == 2 * f else (lower, upper)
    k = int(K[t, s])
    q = [c for c in beyond(par, kid, n, v0, x) if c == vk or _reaches(par, C, v0, c, vk)]
    assert len(q) == 1
    return x, v0, q[0], vk, w, k


def _reaches(par, C, v, c, target):
    """the side of c seen from v holds target"""
    def has(x, y):
        while y != C and y != x:
            y = int(par[y])
        return y == x

    if c != C and par[c] == v:
        return has(c, target)
    return not has(v, target)


# ---------------------------------------------------------------- the search
def _search(J, D, tol, max_moves, loops, trace=None):
    J = np.asarray(J)
    n = len(J) + 2
    assert n >= 3 and tol >= 0
    max_moves = 10 * n if max_moves is None else max_moves
    Dm = bm.mirrored(D)
    nb = slots_of(J)
    res = np.zeros(1, bm.REFINE)[0]
    log = []
    first = None
    while True:
        par, kid = orient(nb, n)
        order, lev = bm.bfs(par, kid, n)
        below = bm.leaf_sets(kid, n, order)
        A = bm.table(Dm, par, kid, n, order, below)
        Rows = bm.rows(par, kid, n)
        T = bm.sums(A, below, lev, Rows, n)
        L = bm.lengths(T, Rows, par, kid, n)
        if first is None:
            first = L
        if loops:
            top = best_loops(candidates_loops(pairs_loops(A, par, kid, n), par, kid, n))
            gain, mv = (top[0], top[4:]) if top is not None else (np.float64("nan"), None)
        else:
            G, ok, K = candidates(pairs(A, par, kid, n, order, ancestors(par, n, order)), par, kid, n, order)
            at = best(G, ok)
            gain, mv = (G[at], move_of(par, kid, n, K, *at)) if at is not None else (np.float64("nan"), None)
        if not gain > tol:
            res["converged"] = 1
            break
        if len(log) >= max_moves:
            res["converged"] = 0
            break
        x, v0, q, vk, w, k = mv
        if trace is not None:
            trace.append((x, v0, q, vk, w, k, par.copy()))
        log.append((gain, least_of_side(below, par, n, v0, x), least_of_side(below, par, n, vk, w), k, 0))
        apply_spr(nb, n, x, v0, q, vk, w)
    res["length_before"], res["length_after"], res["moves"] = bm.seq_sum(first), bm.seq_sum(L), len(log)
    return bm.canonical(par, kid, L, n), res, np.array(log, SPR_MOVE)


def refine_spr(J, D, tol=0.0, max_moves=None, trace=None):
    """(records, result, log) of the search from the tree J on the matrix D; trace: a list that takes every move made as
    (x, v0, q, vk, w, k, par) -- the nodes of the move and the parents of the tree it was made on"""
    return _search(J, D, tol, max_moves, False, trace)


def depth_of(par, n):
    """the edges from the centre to the deepest leaf: what sizes the walk's stacks on the device"""
    C, deepest = 2 * n - 3, 0
    for v in range(n):
        d = 0
        while v != C:
            v, d = int(par[v]), d + 1
        deepest = max(deepest, d)
    return deepest


def kind_of(move, n):
    """what a traced move does with the centre: "at" (v0 = C), "across" (C is one of v1 ... vk), "holds" (X holds C), or
    "" -- the cases in which a move re-orients edges of the rooted tree"""
    x, v0, q, vk, w, k, par = move
    C = 2 * n - 3
    if v0 == C:
        return "at"
    if par[v0] == x:
        return "holds"
    v = vk  # the path v0 ... vk runs up from v0 to its top and down to vk: it holds C if it climbs to it
    while v != C and v != v0:
        v = int(par[v])
    return "across" if v == C else ""


def refine_spr_loops(J, D, tol=0.0, max_moves=None):
    return _search(J, D, tol, max_moves, True)
