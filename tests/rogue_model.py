"""Plain Python restatement of the rogue genomes of a bootstrap (andi_hip_nj_transfer_taxa, include/andi_hip.h), twice:
leaf sets as Python ints, and -- the fast statement -- unpacked bits as float32 with H = |A| + |B| - 2 A B^T (sums of at
most n < 2^24 zeros and ones: exact), argmin along the replicate's axis (NumPy's takes the first occurrence: the least t)
and XOR of bit rows.  And the hand-made records the tests feed the library: tests/test_transfer_gpu.py's trees, with a
recipe of eight replicates.  What tests/test_rogues_*.py hold the library to.

For pair record s of the tree and a used replicate k: over the replicate's pair records t, h = |L_s xor L_{k,t}| and d =
min(h, n - h); dist[k][s] is the least d (no cap), match[k][s] the least t that attains it, flip is h > n - h there, and
M(k, s) = L_s xor L_{k,match}, complemented within the n leaves on flip.  The pair is counted iff dist[k][s] <=
floor(cutoff * (depth[s] - 1)); moved[i] counts the counted pairs with leaf i in M, pairs counts the counted pairs."""
import math

import numpy as np

import nj_model
from transfer_model import SKIPPED, _ones, bit_matrix, leaf_sets


def limit(cutoff, depth):
    """one rounded multiplication in doubles, then floor"""
    return int(math.floor(float(cutoff) * float(int(depth) - 1)))


def nearest(a, theirs, n):
    """(d, t, flip): the least distance of the set a among the replicate's sets, the least t that attains it, its side"""
    best = None
    for t, b in enumerate(theirs):
        h = _ones(a ^ b)
        d = min(h, n - h)
        if best is None or d < best[0]:
            best = (d, t, h > n - h)
    return best


def nearest_all(tree, reps, skip=None):
    """per replicate the (d, t, flip) of every set of the tree; None for a skipped one.  It does not depend on the cutoff."""
    n = len(tree) + 2
    mine = leaf_sets(tree, n)
    out = []
    for k, rep in enumerate(reps):
        if skip is not None and skip[k]:
            out.append(None)
            continue
        theirs = leaf_sets(rep, n)
        out.append([nearest(a, theirs, n) for a in mine])
    return out


def taxa(tree, reps, skip=None, cutoff=0.3, near=None):
    """(moved, pairs, match, dist) as lists and an int: the contract in ints.  near: nearest_all's result, if at hand"""
    n = len(tree) + 2
    mine = leaf_sets(tree, n)
    depth = [min(_ones(a), n - _ones(a)) for a in mine]
    full = (1 << n) - 1
    near = nearest_all(tree, reps, skip) if near is None else near
    moved, pairs, match, dist = [0] * n, 0, [], []
    for k, rep in enumerate(reps):
        if near[k] is None:
            match.append([SKIPPED] * len(mine))
            dist.append([SKIPPED] * len(mine))
            continue
        theirs = leaf_sets(rep, n)
        for s, a in enumerate(mine):
            d, t, flip = near[k][s]
            if d <= limit(cutoff, depth[s]):
                pairs += 1
                M = a ^ theirs[t]
                if flip:
                    M = ~M & full
                assert _ones(M) == d
                for i in range(n):
                    moved[i] += M >> i & 1
        match.append([t for _, t, _ in near[k]])
        dist.append([d for d, _, _ in near[k]])
    return moved, pairs, match, dist


def taxa_numpy(tree, reps, skip=None, cutoff=0.3):
    """(moved uint64[n], pairs, match, dist (count, n - 3) uint32): the same contract through one matrix product per replicate"""
    n = len(tree) + 2
    assert n < 1 << 24
    A = bit_matrix(tree, n)
    size = A.sum(1)
    depth = np.minimum(size, n - size)
    lim = np.array([limit(cutoff, d) for d in depth], np.float32)
    moved, pairs = np.zeros(n, np.uint64), 0
    match = np.full((len(reps), len(A)), SKIPPED, np.uint32)
    dist = np.full((len(reps), len(A)), SKIPPED, np.uint32)
    rows = np.arange(len(A))
    for k, rep in enumerate(reps):
        if (skip is not None and skip[k]) or n < 4:
            continue
        B = bit_matrix(rep, n)
        H = size[:, None] + B.sum(1)[None, :] - 2.0 * (A @ B.T)
        Dm = np.minimum(H, n - H)
        t = Dm.argmin(1)  # (the first occurrence of the minimum: the least t)
        d = Dm[rows, t]
        flip = H[rows, t] > n - H[rows, t]
        M = (A != B[t]) ^ flip[:, None]
        on = d <= lim
        assert (M.sum(1) == d).all()
        moved += M[on].sum(0).astype(np.uint64)
        pairs += int(on.sum())
        match[k], dist[k] = t.astype(np.uint32), d.astype(np.uint32)
    return moved, pairs, match, dist


# ------------------------------------------------------------------ hand-made records (as tests/test_transfer_gpu.py makes them)
def records(rows, final):
    J = np.zeros(len(rows) + 1, nj_model.NJ_JOIN)
    for s, (a, b) in enumerate(rows):
        J[s] = (a, b, -1, 0, 0.1, 0.1, 0.0)
    J[len(rows)] = tuple(final) + (0, 0.1, 0.1, 0.1)
    return J


def caterpillar(n, order=None):
    order = list(range(n)) if order is None else order
    rows = [(order[0], order[1])] + [(n + s - 1, order[s + 1]) for s in range(1, n - 3)]
    return records(rows, (order[n - 2], order[n - 1], n + n - 4))


def random_tree(n, seed):
    """random joins; the last pair record's node is the final record's third child"""
    rng = np.random.default_rng(seed)
    nodes, rows = list(range(n)), []
    while len(nodes) > 3:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b, a = nodes.pop(j), nodes.pop(i)
        nodes.append(n + len(rows))
        rows.append((a, b))
    return records(rows, nodes)


def other_final(J, n):
    """the same unrooted tree with another final three (one leaf set turns into its complement)"""
    if n <= 4:
        return J
    K = J.copy()
    x, y, z = (int(J[n - 3][f]) for f in "abc")
    assert z == n + n - 4
    p, q = int(J[n - 4]["a"]), int(J[n - 4]["b"])
    K[n - 4]["a"], K[n - 4]["b"] = x, y
    K[n - 3]["a"], K[n - 3]["b"], K[n - 3]["c"] = p, q, z
    return K


def exchanged(J, n, seed, leaves):
    """J with `leaves` pairs of its leaves exchanged: a tree a few transfers away"""
    rng = np.random.default_rng(seed)
    perm = np.arange(n)
    for _ in range(leaves):
        i, j = rng.choice(n, 2, replace=False)
        perm[[i, j]] = perm[[j, i]]
    return relabelled(J, n, perm)


def relabelled(J, n, perm):
    K = J.copy()
    for f in "abc":
        leaf = (K[f] >= 0) & (K[f] < n)
        K[f][leaf] = perm[K[f][leaf]]
    return K


def swapped(J, n, i, j):
    """J with the leaves i and j exchanged"""
    perm = np.arange(n)
    perm[[i, j]] = j, i
    return relabelled(J, n, perm)


def replicates(n):
    """the tree random_tree(n, n) and eight replicates around it: itself, its other writing, one pair of leaves exchanged,
    an unrelated tree, max(2, n // 16) pairs exchanged, a caterpillar, and the other writings of a one-exchange and of a
    many-exchange tree"""
    tree = random_tree(n, n)
    many = max(2, n // 16)
    return tree, [tree, other_final(tree, n), exchanged(tree, n, 2, 1), random_tree(n, n + 4), exchanged(tree, n, 4, many),
                  caterpillar(n), other_final(exchanged(tree, n, 6, 1), n), other_final(exchanged(tree, n, 7, many), n)]


def ties_and_flips(tree, reps, cutoff):
    """(ties, flips) among the counted pairs with d > 0: those whose least distance two records of the replicate attain
    with different M, and those matched on the far side"""
    n = len(tree) + 2
    mine = leaf_sets(tree, n)
    full = (1 << n) - 1
    ties = flips = 0
    for rep in reps:
        theirs = leaf_sets(rep, n)
        for a in mine:
            d, t, flip = nearest(a, theirs, n)
            depth = min(_ones(a), n - _ones(a))
            if d == 0 or d > limit(cutoff, depth):
                continue
            flips += flip
            Ms = set()
            for b in theirs:
                h = _ones(a ^ b)
                if min(h, n - h) == d:
                    Ms.add(a ^ b if h <= n - h else ~(a ^ b) & full)
            ties += len(Ms) > 1
    return ties, flips
