"""NumPy restatement of andi_hip_nj's arithmetic contract (include/andi_hip.h), a Newick formatter and a small Newick
parser: what tests/test_nj_*.py and scripts/nj_bench.py hold the device and the library to."""
import numpy as np

NJ_JOIN = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"),
                    ("lc", "<f8")])


def nj(D, steps=None):
    """The records andi_hip_nj writes for D (only the upper triangle is read), bit for bit; with steps=k only the first k
    records (each is a function of the state before its step alone, so a prefix stands on its own).

    The contract's arithmetic, one step at a time.  C holds D by position, positions in ascending slot order; a join
    overwrites the lower slot's row and column and retires the other position (live[p] = False).  Retired positions stay
    in C, unread, until a quarter of C is retired, when C is compacted: no step copies the active block."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    nrec = 1 if n == 2 else n - 2
    steps = nrec if steps is None else min(steps, nrec)
    iu = np.triu_indices(n, 1)
    C = np.zeros((n, n))  # diagonal +0.0
    C[iu] = D[iu]
    C.T[iu] = D[iu]
    out = np.zeros(steps, NJ_JOIN)
    if steps and n == 2:
        h = C[0, 1] * 0.5
        out[0] = (0, 1, -1, 0, h, h, 0.0)
    if steps == 0 or n == 2:
        return out
    ids = np.arange(n)  # ids[p]: the id of the node at position p
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):  # (overflow of finite input: inf and NaN are part of the contract)
        for s in range(min(steps, n - 3)):
            r = n - s
            if len(live) - r > len(live) // 4:
                C, ids, live = C[np.ix_(live, live)], ids[live], live[live]
            # R_x: a sequential sum over the active slots in ascending order from +0.0, one row of C at a time (C is
            # symmetric: row k is column k); entries at retired positions are never read below
            R = np.zeros(len(live))
            for k in np.flatnonzero(live):
                R += C[k]

            def q_rows(p0):
                """Q for rows p0 .. p0+63 (row x, column y: ((r-2) * D[x][y] - R_x) - R_y), and which entries are
                candidates: x and y active and id(x) < id(y), so every active pair once, with x the smaller id"""
                rows = slice(p0, p0 + 64)
                Q = (np.float64(r - 2) * C[rows] - R[rows, None]) - R[None, :]
                pair = live[rows, None] & live[None, :] & (ids[rows, None] < ids[None, :])
                return Q, pair

            # the least Q by value (-0.0 == +0.0); a NaN Q orders after every number
            least = {}  # row block -> its least non-NaN Q
            for p0 in range(0, len(live), 64):
                Q, pair = q_rows(p0)
                num = pair & ~np.isnan(Q)
                if num.any():
                    least[p0] = Q.min(where=num, initial=np.inf)
            if least:
                m = min(least.values())
                px, py = [], []
                for p0 in (p0 for p0, q in least.items() if q == m):
                    Q, pair = q_rows(p0)
                    x, y = np.nonzero(pair & (Q == m))
                    px.append(x + p0)
                    py.append(y)
                px, py = np.concatenate(px), np.concatenate(py)
                k = np.lexsort((ids[py], ids[px]))[0]  # ties: the smaller id(x), then the smaller id(y)
                pa, pb = px[k], py[k]
            else:  # every Q is NaN: the id order alone, so the two smallest ids
                pa, pb = sorted(np.flatnonzero(live), key=lambda p: ids[p])[:2]
            d = C[pa, pb]
            la = d * 0.5 + (R[pa] - R[pb]) / np.float64(2 * (r - 2))
            out[s] = (ids[pa], ids[pb], -1, 0, la, d - la, 0.0)
            pu, po = min(pa, pb), max(pa, pb)  # the new node takes the lower slot, the other retires
            v = ((C[pa] + C[pb]) - d) * 0.5
            v[pu] = 0.0
            C[pu], C[:, pu] = v, v
            ids[pu] = n + s
            live[po] = False
        if steps == n - 2:
            act = np.flatnonzero(live)
            x, y, z = act[np.argsort(ids[act])]  # (r = 3)
            xy, xz, yz = C[x, y], C[x, z], C[y, z]
            out[n - 3] = (ids[x], ids[y], ids[z], 0, ((xy + xz) - yz) * 0.5, ((xy + yz) - xz) * 0.5,
                          ((xz + yz) - xy) * 0.5)
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
