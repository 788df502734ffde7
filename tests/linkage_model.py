"""NumPy restatement of andi_hip_linkage's contract (include/andi_hip.h) and of the host functions on its records -- the
cut into flat clusters, the medoids, the stability over replicates, the Newick text: what tests/test_linkage_*.py and
scripts/linkage_bench.py hold the device and the library to."""
import numpy as np

from nj_model import _leaf

LINK = np.dtype([("a", "<i4"), ("b", "<i4"), ("size", "<u4"), ("pad", "<u4"), ("height", "<f8")])
METHODS = ("single", "complete", "average")


def mapped(D):
    """D as the contract reads it: the upper triangle mirrored, a NaN as +inf, the diagonal +0.0; a -inf is refused."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    up = D[iu].copy()
    up[np.isnan(up)] = np.inf
    if (up == -np.inf).any():
        k = int(np.flatnonzero(up == -np.inf)[0])
        raise ValueError("D[%d][%d] is -inf" % (iu[0][k], iu[1][k]))
    C = np.zeros((n, n))
    C[iu] = up
    C.T[iu] = up
    return C


def linkage(D, method="average", steps=None):
    """The records andi_hip_linkage writes for D, bit for bit; with steps=k only the first k (a record is a function of
    the state before its step alone, so a prefix stands on its own).

    One step at a time on the active block: the least entry of its upper triangle by value, NaN after every number, ties
    to the smaller id(x), then the smaller id(y); the new node's row by the method's rule, every operation a rounded
    NumPy operation of its own."""
    assert method in METHODS
    C = mapped(D)
    n = C.shape[0]
    steps = n - 1 if steps is None else min(steps, n - 1)
    out = np.zeros(steps, LINK)
    ids = np.arange(n)
    size = np.ones(n, np.int64)
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):  # (overflow in the average rule: inf and NaN are part of the contract)
        for s in range(steps):
            pos = np.flatnonzero(live)
            r = len(pos)
            i, j = np.triu_indices(r, 1)
            vals = C[pos[i], pos[j]]
            num = ~np.isnan(vals)
            pick = np.flatnonzero(vals == vals[num].min()) if num.any() else np.arange(len(vals))
            x, y = ids[pos[i[pick]]], ids[pos[j[pick]]]
            lo, hi = np.minimum(x, y), np.maximum(x, y)
            k = np.lexsort((hi, lo))[0]
            pa, pb = pos[i[pick[k]]], pos[j[pick[k]]]
            if ids[pa] > ids[pb]:
                pa, pb = pb, pa  # a: the member of smaller id
            na, nb = size[pa], size[pb]
            out[s] = (ids[pa], ids[pb], na + nb, 0, C[pa, pb])
            ra, rb = C[pa], C[pb]
            if method == "single":
                v = np.where(rb < ra, rb, ra)
            elif method == "complete":
                v = np.where(rb > ra, rb, ra)
            else:
                v = (np.float64(na) * ra + np.float64(nb) * rb) / np.float64(na + nb)
            pu, po = min(pa, pb), max(pa, pb)  # the new node takes the lower slot, the other retires
            v[pu] = 0.0
            C[pu], C[:, pu] = v, v
            ids[pu], size[pu] = n + s, na + nb
            live[po] = False
    return out


def cut(Z, t):
    """andi_hip_linkage_cut: node n + s is closed iff height[s] <= t and each child is a leaf or closed; the clusters are
    the maximal closed nodes and the remaining leaves, numbered by first appearance in ascending leaf id."""
    n = len(Z) + 1
    closed = np.zeros(2 * n - 1, bool)
    closed[:n] = True
    for s in range(n - 1):
        closed[n + s] = bool(Z["height"][s] <= t) and closed[Z["a"][s]] and closed[Z["b"][s]]
    top = np.arange(2 * n - 1)
    for s in range(n - 2, -1, -1):
        if closed[n + s]:
            top[Z["a"][s]] = top[Z["b"][s]] = top[n + s]
    labels, seen = np.zeros(n, np.uint32), {}
    for i in range(n):
        labels[i] = seen.setdefault(int(top[i]), len(seen))
    return labels


def medoids(D, labels):
    """andi_hip_cluster_medoids: per cluster the member with the least sequential sum (ascending id, from +0.0) of the
    mapped distances to the cluster's members; ties to the smaller id, a NaN sum last."""
    C = mapped(D)
    labels = np.asarray(labels)
    out = np.zeros(int(labels.max()) + 1, np.uint32)
    with np.errstate(all="ignore"):
        for c in range(len(out)):
            members = np.flatnonzero(labels == c)
            best = None
            for i in members:
                acc = np.float64(0.0)
                for j in members:
                    acc = acc + C[i, j]
                key = (bool(np.isnan(acc)), 0.0 if np.isnan(acc) else float(acc), int(i))
                if best is None or key < best:
                    best = key
            out[c] = best[2]
    return out


def stability(labels, rep_labels):
    """andi_hip_cluster_stability: for every cluster the number of replicates that have exactly its leaf set as a cluster."""
    labels = np.asarray(labels)
    out = np.zeros(int(labels.max()) + 1, np.uint32)
    for R in np.asarray(rep_labels):
        theirs = {frozenset(np.flatnonzero(R == v).tolist()) for v in np.unique(R)}
        for c in range(len(out)):
            out[c] += frozenset(np.flatnonzero(labels == c).tolist()) in theirs
    return out


def newick(Z, names, truncate_names=False):
    """andi_hip_format_newick_linkage's text, built without recursion; "" where the library refuses a branch length that
    is not finite."""
    n = len(names)
    h = np.r_[np.zeros(n), Z["height"]]
    with np.errstate(all="ignore"):
        for s in range(n - 1):
            if not (np.isfinite(h[n + s] - h[Z["a"][s]]) and np.isfinite(h[n + s] - h[Z["b"][s]])):
                return ""
        parts = ["("]
        stack = [(n - 2, 0, 0.0)]  # (record, next child, own length)
        while stack:
            rec, k, own = stack.pop()
            if k == 2:
                parts.append("):%.8g" % own if stack else ");\n")
                continue
            stack.append((rec, k + 1, own))
            if k:
                parts.append(",")
            child = int(Z[rec][("a", "b")[k]])
            length = float(h[n + rec] - h[child])
            if child < n:
                parts.append(_leaf(names[child], truncate_names) + ":%.8g" % length)
            else:
                stack.append((child - n, 0, length))
                parts.append("(")
    return "".join(parts)
