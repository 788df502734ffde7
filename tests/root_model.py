"""NumPy restatement of rooting a neighbor-joining tree (andi_hip_root, include/andi_hip.h): minimal ancestor deviation and
the midpoint of the longest path.  The tree, the edges and h(v, i) are place_model's; the near-end distances, the pairs'
path lengths, the two passes with every operation rounded on its own and every sum in the contract's order -- the inner sum
of a (edge, b) over c > b ascending, then over b ascending --, the choice of the edge and the midpoint's walk are here.
Vectorised over the edges; the pairs are a Python loop.  What tests/test_root_*.py hold the library to."""
import numpy as np

from place_model import paths

METHODS = {"mad": 0, "midpoint": 1}
ROOT = np.dtype([("edge", "<i4"), ("pad", "<u4"), ("distal", "<f8"), ("ss", "<f8"), ("pairs", "<u8"), ("ss_second", "<f8"),
                 ("far_b", "<i4"), ("far_c", "<i4")])


class Table:
    """what both methods work from: T[v, i] = t_v(i), below[v, i], parent, L of the 2n - 3 edges, P[b, c] = p(b, c) and
    used[b, c] for b < c"""

    def __init__(self, J):
        J = np.asarray(J)
        n = self.n = len(J) + 2
        E = self.E = 2 * n - 3
        H, below, self.parent, self.L = paths(J, n)
        self.below = below[:E]
        self.T = np.where(self.below, H[:E], H[self.parent])
        with np.errstate(all="ignore"):
            self.P = self.T[:n] + self.L[:n, None]  # row b is leaf b's own edge
            self.used = np.isfinite(self.P) & (self.P > 0) & np.triu(np.ones((n, n), bool), 1)
        self.Lc = np.where(self.L > 0, self.L, 0.0)


def pair_r(t, b, c, x):
    """r of the pair b < c for every edge under the roots at x (E,): the contract's two closed forms"""
    p = t.P[b, c]
    sb, sc = t.below[:, b], t.below[:, c]
    with np.errstate(all="ignore"):
        d = np.where(sb, t.T[:, b] + x, t.T[:, b] + (t.L - x))
        return np.where(sb != sc, (2.0 * d) / p - 1.0, (t.T[:, b] - t.T[:, c]) / p)


def solve_x(t):
    """pass 1: (x, N, W) of every edge"""
    n, E = t.n, t.E
    N, W = np.zeros(E), np.zeros(E)
    with np.errstate(all="ignore"):
        for b in range(n):
            iN, iW = np.zeros(E), np.zeros(E)
            for c in np.nonzero(t.used[b])[0]:
                p = t.P[b, c]
                sb, sc = t.below[:, b], t.below[:, c]
                ta = np.where(sb, t.T[:, b], t.T[:, c])
                iN = np.where(sb != sc, iN + (p - 2.0 * ta) / (p * p), iN)
                iW = np.where(sb != sc, iW + 1.0 / (p * p), iW)
            N, W = N + iN, W + iW
        a = N / (2.0 * W)
        x = np.where(W == 0.0, 0.0, np.where(a > 0, np.where(a < t.Lc, a, t.Lc), 0.0))
    return x, N, W


def sum_ss(t, x):
    """pass 2: SS of every edge under the roots at x"""
    SS = np.zeros(t.E)
    with np.errstate(all="ignore"):
        for b in range(t.n):
            inner = np.zeros(t.E)
            for c in np.nonzero(t.used[b])[0]:
                r = pair_r(t, b, c, x)
                inner = inner + r * r
            SS = SS + inner
    return SS


def _least(ss, skip=-1):
    """the index of the least value, ties to the smaller index, a NaN after every number; skip: an index left out"""
    best = -1
    for v in range(len(ss)):
        if v == skip:
            continue
        if best < 0 or ss[v] < ss[best] or (not np.isnan(ss[v]) and np.isnan(ss[best])):
            best = v
    return best


def farthest(t):
    """(b, c) of the used pair of the greatest p, the first in (b, c) order; (-1, -1) without a used pair"""
    if not t.used.any():
        return -1, -1
    key = np.where(t.used, t.P, -np.inf)
    b, c = np.unravel_index(int(np.argmax(key)), key.shape)  # (the first of the greatest, in row-major order)
    return int(b), int(c)


def midpoint_walk(t, b, c):
    """(edge, distal) of the point p * 0.5 from b on the path to c"""
    C = t.E
    up, v = [], b
    while v != C:
        up.append(v)
        v = int(t.parent[v])
    mine = set(up) | {C}
    down, top = [], c
    while top not in mine:
        down.append(top)
        top = int(t.parent[top])
    rem = t.P[b, c] * 0.5
    for v in up:
        if v == top:
            break
        if rem < t.L[v]:
            return v, rem
        rem = rem - t.L[v]
    for u in reversed(down):
        if rem < t.L[u]:
            return u, t.L[u] - rem
        rem = rem - t.L[u]
    return c, 0.0


def root(J, method="mad", per=False):
    """The ROOT record of the tree J; with per=True (mad) also x and SS of every edge."""
    t = Table(J)
    out = np.zeros(1, ROOT)[0]
    out["pairs"] = int(t.used.sum())
    out["far_b"], out["far_c"] = farthest(t)
    if METHODS[method] == 1:
        if out["far_b"] >= 0:
            out["edge"], out["distal"] = midpoint_walk(t, int(out["far_b"]), int(out["far_c"]))
        return out
    x, _, _ = solve_x(t)
    ss = sum_ss(t, x)
    v = _least(ss)
    out["edge"], out["distal"], out["ss"], out["ss_second"] = v, x[v], ss[v], ss[_least(ss, skip=v)]
    return (out, x, ss) if per else out


def score(rec):
    """(sqrt(ss / pairs), sqrt(ss / ss_second)): MAD's score and the root ambiguity index"""
    with np.errstate(all="ignore"):
        return (np.sqrt(np.float64(rec["ss"]) / np.float64(rec["pairs"])),
                np.sqrt(np.float64(rec["ss"]) / np.float64(rec["ss_second"])))
