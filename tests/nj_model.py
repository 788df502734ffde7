"""NumPy restatement of andi_hip_nj's arithmetic contract (include/andi_hip.h), a Newick formatter and a small Newick
parser: what tests/test_nj_*.py and scripts/nj_bench.py hold the device and the library to."""
import numpy as np

NJ_JOIN = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"),
                    ("lc", "<f8")])


def nj(D):
    """The records andi_hip_nj writes for D (only the upper triangle is read), bit for bit."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    M = np.zeros((n, n))  # diagonal +0.0
    M[iu] = D[iu]
    M.T[iu] = D[iu]
    if n == 2:
        h = M[0, 1] * 0.5
        return np.array([(0, 1, -1, 0, h, h, 0.0)], NJ_JOIN)
    out = np.zeros(n - 2, NJ_JOIN)
    ids = np.arange(n)
    active = np.ones(n, bool)
    for s in range(n - 3):
        r = n - s
        act = np.flatnonzero(active)  # ascending slots
        sub = M[np.ix_(act, act)]
        # R: a sequential sum per column from +0.0 (np.cumsum is sequential, np.sum pairwise); D is symmetric
        R = np.cumsum(np.vstack([np.zeros((1, r)), sub]), axis=0)[-1]
        idl = ids[act]
        x_first = idl[:, None] < idl[None, :]  # row member has the smaller id
        Rx = np.where(x_first, R[:, None], R[None, :])
        Ry = np.where(x_first, R[None, :], R[:, None])
        Q = (np.float64(r - 2) * sub - Rx) - Ry
        Q[np.arange(r), np.arange(r)] = np.inf
        cand = np.argwhere(Q == Q.min())
        lo = np.minimum(idl[cand[:, 0]], idl[cand[:, 1]])
        hi = np.maximum(idl[cand[:, 0]], idl[cand[:, 1]])
        k = np.lexsort((hi, lo))[0]
        pi, pj = cand[k]
        if idl[pi] > idl[pj]:
            pi, pj = pj, pi
        sa, sb = act[pi], act[pj]
        d = M[sa, sb]
        la = d * 0.5 + (R[pi] - R[pj]) / np.float64(2 * (r - 2))
        lb = d - la
        out[s] = (ids[sa], ids[sb], -1, 0, la, lb, 0.0)
        su, so = min(sa, sb), max(sa, sb)
        others = act[(act != sa) & (act != sb)]
        v = ((M[sa, others] + M[sb, others]) - d) * 0.5
        M[su, others] = v
        M[others, su] = v
        M[su, su] = 0.0
        active[so] = False
        ids[su] = n + s
    act = np.flatnonzero(active)
    x, y, z = act[np.argsort(ids[act])]
    xy, xz, yz = M[x, y], M[x, z], M[y, z]
    out[n - 3] = (ids[x], ids[y], ids[z], 0, ((xy + xz) - yz) * 0.5, ((xy + yz) - xz) * 0.5, ((xz + yz) - xy) * 0.5)
    return out


def _leaf(name, truncate):
    if truncate:
        name = name[:10]
    if any(ch in name for ch in " \t()[]':;,"):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(J, names, truncate_names=False):
    """andi_hip_format_newick's text of the records J, built without recursion."""
    n = len(names)
    root = 0 if n == 2 else n - 3
    kids = 2 if n == 2 else 3
    parts = ["("]
    stack = [(root, 0, kids, 0.0)]  # (record, next child, children, own length)
    while stack:
        rec, k, nk, own = stack.pop()
        if k == nk:
            parts.append(")")
            parts.append(";\n" if not stack else ":%.8g" % own)
            continue
        stack.append((rec, k + 1, nk, own))
        if k:
            parts.append(",")
        child = int(J[rec][("a", "b", "c")[k]])
        length = float(J[rec][("la", "lb", "lc")[k]])
        if child < n:
            parts.append(_leaf(names[child], truncate_names) + ":%.8g" % length)
        else:
            stack.append((child - n, 0, 2, length))
            parts.append("(")
    return "".join(parts)


def parse_newick(text):
    """(leaf names, splits, lengths) of a Newick line: every internal edge's split as the frozenset of leaf names on its
    far side from the root; lengths maps a split (a leaf's split is frozenset({name})) to its branch length."""
    text = text.strip()
    assert text.endswith(";")
    pos, stack, leaves, splits, lengths = 0, [], [], set(), {}
    cur = None
    while pos < len(text) - 1:
        ch = text[pos]
        if ch == "(":
            stack.append(set())
            pos += 1
        elif ch == ")":
            cur = frozenset(stack.pop())
            if stack:
                stack[-1] |= cur
                splits.add(cur)
            pos += 1
        elif ch == ",":
            pos += 1
        elif ch == ":":
            end = pos + 1
            while end < len(text) and text[end] not in ",);":
                end += 1
            lengths[cur] = float(text[pos + 1:end])
            pos = end
        else:
            if ch == "'":
                end, name = pos + 1, []
                while True:
                    if text[end] == "'" and text[end + 1:end + 2] == "'":
                        name.append("'")
                        end += 2
                    elif text[end] == "'":
                        end += 1
                        break
                    else:
                        name.append(text[end])
                        end += 1
                name = "".join(name)
            else:
                end = pos
                while text[end] not in ":,()":
                    end += 1
                name = text[pos:end]
            leaves.append(name)
            stack[-1].add(name)
            cur = frozenset([name])
            pos = end
    return leaves, splits, lengths


def unrooted_splits(splits, leaves):
    """splits as unrooted bipartitions: each side normalised to the one without the first leaf; trivial ones dropped"""
    everything = frozenset(leaves)
    first = sorted(leaves)[0]
    out = set()
    for s in splits:
        side = everything - s if first in s else s
        if 1 < len(side) < len(everything) - 1:
            out.add(side)
    return out


def additive_tree(n, seed, noise=0.0):
    """(D, splits, names) of a random binary tree with n leaves and branch lengths in [0.01, 0.1): D the leaves' path
    distances (plus seeded symmetric noise of that relative size), splits the tree's nontrivial bipartitions."""
    rng = np.random.default_rng(seed)
    names = ["L%d" % i for i in range(n)]
    # grow by attaching each new leaf to the middle of a random edge; edges as (child, parent) with length
    parent = {0: -1, 1: -1}  # node -> parent; -1 the root joining leaf 0 and leaf 1
    length = {0: rng.uniform(0.01, 0.1), 1: rng.uniform(0.01, 0.1)}
    nxt = n
    for leaf in range(2, n):
        edges = list(parent.keys())
        e = edges[rng.integers(len(edges))]
        mid = nxt
        nxt += 1
        parent[mid], length[mid] = parent[e], rng.uniform(0.01, 0.1)
        parent[e] = mid
        parent[leaf], length[leaf] = mid, rng.uniform(0.01, 0.1)
    nodes = sorted(parent)  # every node with an edge above it
    col = {v: k for k, v in enumerate(nodes)}
    A = np.zeros((n, len(nodes)))  # A[i, e] = 1: edge e lies on leaf i's path to the root
    below = {}
    for i in range(n):
        v = i
        while v != -1:
            A[i, col[v]] = 1.0
            below.setdefault(v, set()).add(names[i])
            v = parent[v]
    lens = np.array([length[v] for v in nodes])
    S = (A * lens) @ A.T  # the length the two paths share
    depth = np.diag(S).copy()
    D = depth[:, None] + depth[None, :] - 2.0 * S
    D = np.triu(D, 1) + np.triu(D, 1).T
    if noise:
        E = np.triu(rng.uniform(-noise, noise, (n, n)), 1)
        D = D * (1.0 + E + E.T)
    splits = unrooted_splits({frozenset(s) for s in below.values()}, names)
    return D, splits, names


def patristic(J, n):
    """(n, n) path lengths between the leaves of the tree J describes"""
    P = np.zeros((n, n))
    below = {}  # node -> (leaves, their distances from it)

    def side(v, length):
        leaves, dist = below.pop(v) if v >= n else (np.array([v]), np.zeros(1))
        return leaves, dist + length

    recs = [(J[s]["a"], J[s]["b"], J[s]["la"], J[s]["lb"]) for s in range(len(J) - 1)] if n > 2 else []
    for s, (a, b, la, lb) in enumerate(recs):
        (xa, da), (xb, db) = side(a, la), side(b, lb)
        P[np.ix_(xa, xb)] = da[:, None] + db[None, :]
        below[n + s] = (np.r_[xa, xb], np.r_[da, db])
    last = J[len(J) - 1]
    kids = [side(last["a"], last["la"]), side(last["b"], last["lb"])]
    if n > 2:
        kids.append(side(last["c"], last["lc"]))
    for i in range(len(kids)):
        for j in range(i + 1, len(kids)):
            (xa, da), (xb, db) = kids[i], kids[j]
            P[np.ix_(xa, xb)] = da[:, None] + db[None, :]
    return np.maximum(P, P.T)
