"""Plain Python restatement of the majority-rule consensus of a bootstrap (andi_hip_nj_splits, andi_hip_consensus,
andi_hip_format_newick_consensus; include/andi_hip.h), on support_model.leaf_sets: the distinct splits numbered by first
appearance through a dict, their frequencies, the strict majority, parents by set containment, the sequential mean
lengths and the Newick text.  What tests/test_consensus_*.py hold the library to."""
import functools

import numpy as np

import nj_model
import support_model

CONS_NODE = np.dtype([("parent", "<i4"), ("support", "<u4"), ("length", "<f8")])
NONE = 0xFFFFFFFF


def splits(reps, skip=None):
    """(ids, freq, sets) as andi_hip_nj_splits gives them: ids (count, n - 3) uint32, freq uint32, sets (nsplits, W) uint64"""
    reps = np.asarray(reps)
    count, n = reps.shape[0], reps.shape[1] + 2
    S, W = max(n - 3, 0), (n + 63) // 64
    ids = np.full((count, S), NONE, np.uint32)
    number, freq, bitsets = {}, [], []
    for k in range(count):
        if skip is not None and skip[k]:
            continue
        for s, bits in enumerate(support_model.leaf_sets(reps[k], n)):
            if bits not in number:
                number[bits] = len(freq)
                freq.append(0)
                bitsets.append(bits)
            ids[k, s] = number[bits]
            freq[number[bits]] += 1
    sets = np.zeros((len(freq), W), np.uint64)
    for i, bits in enumerate(bitsets):
        for w in range(W):
            sets[i, w] = (bits >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return ids, np.array(freq, np.uint32), sets


def _bits(row):
    return sum(int(x) << (64 * w) for w, x in enumerate(row))


def _above(rep, n):
    """the length of the branch above every node of one replicate's records: the la, lb or lc of the record that has it as a child"""
    out = {}
    for t in range(len(rep)):
        for f, g in (("a", "la"), ("b", "lb"), ("c", "lc")):
            v = int(rep[t][f])
            if v >= 0:
                out[v] = rep[t][g]
    return out


def consensus(reps, ids, freq, sets, skip=None, n=None):
    """andi_hip_consensus' nodes: the leaves, the majority splits in ascending id order, the root"""
    reps = np.asarray(reps)
    count = reps.shape[0]
    if n is None:
        n = 2 if reps.shape[1] == 1 and int(reps[0, 0]["c"]) < 0 else reps.shape[1] + 2
    S = max(n - 3, 0)
    use = [k for k in range(count) if skip is None or not skip[k]]
    used = len(use)
    assert used > 0
    major = [i for i in range(len(freq) if S else 0) if 2 * int(freq[i]) > used]
    m = len(major)
    bits = [_bits(sets[i]) for i in major]
    nodes = np.zeros(n + m + 1, CONS_NODE)
    root = n + m

    def parent_of(mine, proper):
        best = None
        for j, other in enumerate(bits):
            if mine & other == mine and (other != mine or not proper):
                if best is None or bin(other).count("1") < bin(bits[best]).count("1"):
                    best = j
        return root if best is None else n + best

    for j in range(m):
        nodes[n + j]["parent"] = parent_of(bits[j], True)
        nodes[n + j]["support"] = freq[major[j]]
    for i in range(n):
        nodes[i]["parent"] = parent_of(1 << i, False)
        nodes[i]["support"] = used
    nodes[root] = (-1, used, 0.0)
    # the lengths: sequential sums from +0.0 in ascending k, as doubles
    lsum = [np.float64(0.0)] * n
    isum = [np.float64(0.0)] * m
    where = {i: j for j, i in enumerate(major)}
    for k in use:
        above = _above(reps[k], n)
        for i in range(n):
            lsum[i] = lsum[i] + np.float64(above[i])
        for s in range(S):
            j = where.get(int(ids[k][s]))
            if j is not None:
                isum[j] = isum[j] + np.float64(above[n + s])
    for i in range(n):
        nodes[i]["length"] = lsum[i] / np.float64(used)
    for j in range(m):
        nodes[n + j]["length"] = isum[j] / np.float64(int(freq[major[j]]))
    return nodes


def newick_consensus(nodes, names, truncate_names=False):
    """andi_hip_format_newick_consensus' text: children in ascending order of their least leaf, inner nodes labelled"""
    n = len(names)
    root = len(nodes) - 1
    least = {}
    kids = {v: [] for v in range(n, root + 1)}
    for leaf in range(n):  # a node is entered at its parent when its least leaf reaches it
        v = leaf
        while v != root and v not in least:
            least[v] = leaf
            kids[int(nodes[v]["parent"])].append(v)
            v = int(nodes[v]["parent"])
    parts = ["("]
    stack = [(root, 0)]
    while stack:
        v, k = stack.pop()
        if k == len(kids[v]):
            parts.append(");\n" if not stack else ")%d:%.8g" % (nodes[v]["support"], nodes[v]["length"]))
            continue
        stack.append((v, k + 1))
        if k:
            parts.append(",")
        c = kids[v][k]
        if c < n:
            parts.append(nj_model._leaf(names[c], truncate_names) + ":%.8g" % nodes[c]["length"])
        else:
            stack.append((c, 0))
            parts.append("(")
    return "".join(parts)


# ------------------------------------------------------------------ hand-made records for the tests
def records(rows, final, lengths=None):
    """n - 3 pair records (a, b) and the final three; branch lengths 0.1, or drawn from the generator `lengths`"""
    J = np.zeros(len(rows) + 1, nj_model.NJ_JOIN)
    for s, (a, b) in enumerate(rows):
        J[s] = (a, b, -1, 0, 0.1, 0.1, 0.0)
    J[len(rows)] = tuple(final) + (0, 0.1, 0.1, 0.1)
    if lengths is not None:
        for f in ("la", "lb"):
            J[f] = lengths.uniform(0.01, 0.2, len(J))
        J["lc"][-1] = lengths.uniform(0.01, 0.2)
    return J


def caterpillar(n, lengths=None):
    return records([(0, 1)] + [(n + s - 1, s + 1) for s in range(1, n - 3)], (n - 2, n - 1, n + n - 4), lengths)


def mirrored_caterpillar(n, lengths=None):
    """the caterpillar built from the other end: the same unrooted tree, every set the complement's side"""
    rows = [(n - 1, n - 2)] + [(n + s - 1, n - 2 - s) for s in range(1, n - 3)]
    return records(rows, (0, 1, n + n - 4), lengths)


def random_tree(n, seed, lengths=None):
    """random joins; the last pair record's node is the final record's third child"""
    rng = np.random.default_rng(seed)
    nodes, rows = list(range(n)), []
    while len(nodes) > 3:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b, a = nodes.pop(j), nodes.pop(i)
        nodes.append(n + len(rows))
        rows.append((a, b))
    return records(rows, nodes, lengths)


def other_final(J, n):
    """the same unrooted tree with another final three: final (x, y, z), z the last pair record (p, q), becomes a pair
    record (x, y) and the final (p, q, that node) -- so one leaf set turns into its complement"""
    K = J.copy()
    x, y, z = (int(J[n - 3][f]) for f in "abc")
    assert z == n + n - 4
    p, q = int(J[n - 4]["a"]), int(J[n - 4]["b"])
    K[n - 4]["a"], K[n - 4]["b"] = x, y
    K[n - 3]["a"], K[n - 3]["b"], K[n - 3]["c"] = p, q, z
    return K


# ------------------------------------------------------------------ trees whose difference lies in the far words of the sets
# A kernel that walks a set's W = ceil(n / 64) words 64 at a time takes its second trip at W > 64, n > 4096.  Two trees
# that differ only where that trip reads are what shows a wrong one: a kernel that dropped the far words would call them equal.
def swap_leaves(J, n, i, j):
    """the same records with leaves i and j exchanged: a set that holds exactly one of them changes in bits i and j only"""
    assert 0 <= i < n and 0 <= j < n and i != j
    K = J.copy()
    for f in "abc":
        was_i, was_j = J[f] == i, J[f] == j
        K[f][was_i], K[f][was_j] = j, i
    return K


def _record_of(J, n, v):
    """(record, field) that has node v as a child"""
    for f in "abc":
        at = np.nonzero(J[f] == v)[0]
        if len(at):
            return int(at[0]), f
    raise AssertionError("node %d is nobody's child" % v)


def far_swap(J, n, i, j):
    """swap_leaves for two leaves of the words a second trip reads (i, j >= 4096) that are not siblings"""
    assert i >= 4096 and j >= 4096 and _record_of(J, n, i)[0] != _record_of(J, n, j)[0]
    return swap_leaves(J, n, i, j)


def near_swap(J, n, i, j):
    """the control: two leaves of word 0 that are not siblings"""
    assert i < 64 and j < 64 and _record_of(J, n, i)[0] != _record_of(J, n, j)[0]
    return swap_leaves(J, n, i, j)


def move_leaf(J, n, x):
    """the same records with leaf x cut off and hung on the edge above another node z: the sets between the two places gain
    or lose bit x and nothing else changes (at n = 4097 leaf 4096 is the only leaf of word 64, so no two can be swapped).
    Record s of x, (y, x), becomes (z, x) -- z an earlier node whose parent is a later record --; y takes the place of
    node n + s where that was a child, and node n + s the place of z."""
    s, f = _record_of(J, n, x)
    assert s < n - 4  # a pair record, and not the last one (other_final wants that node as the final record's third child)
    y = int(J[s]["b" if f == "a" else "a"])
    for z in range(64, n + s):
        t, g = _record_of(J, n, z)
        if z not in (x, y) and s < t:
            break
    else:
        raise AssertionError("no place to hang leaf %d" % x)
    K = J.copy()
    up, h = _record_of(J, n, n + s)
    K[s]["a"], K[s]["b"] = z, x
    K[up][h] = y
    K[t][g] = n + s
    return K


@functools.lru_cache(maxsize=None)
def far_word_case(n):
    """(tree, far, near, edge) for the tests of leaf sets around and past 64 words.  tree = random_tree(n, n); near = two
    leaves of word 0 exchanged; far = a tree that lacks some of tree's splits and has in their place splits that differ from
    them in bits >= edge = 64 * min(64, W - 1) alone: two
    leaves of the second (and, where there is one, the third) trip exchanged; at n = 4097, where leaf 4096 is alone past
    bit 4095, that leaf moved; at n <= 4096, where no word lies past the first trip, two leaves of the last word exchanged.
    What the case says about itself is asserted here, on Python ints, without a device.  (Computed once per n and
    shared: the records are not to be written to.)"""
    W = (n + 63) // 64
    edge = 64 * min(64, W - 1)
    tree = random_tree(n, n)
    if n == 4097:
        far = move_leaf(tree, n, 4096)
    else:
        i, j = edge + 4 if edge + 4 < n - 1 else edge, n - 1
        while _record_of(tree, n, i)[0] == _record_of(tree, n, j)[0]:
            i += 1
        far = far_swap(tree, n, i, j) if edge == 4096 else swap_leaves(tree, n, i, j)
    i, j = 3, 40
    while _record_of(tree, n, i)[0] == _record_of(tree, n, j)[0]:
        j += 1
    near = near_swap(tree, n, i, j)
    low = (1 << edge) - 1
    mine, theirs = support_model.leaf_sets(tree, n), support_model.leaf_sets(far, n)
    lost, gained = set(mine) - set(theirs), set(theirs) - set(mine)
    twin = {b & low: b for b in gained}
    twins = [(a, twin[a & low]) for a in lost if a & low in twin]
    # splits of tree that far lacks, each with a split of far beside it that the far words alone tell from it
    assert twins and all(a != b and (a ^ b) & low == 0 for a, b in twins)
    close = support_model.leaf_sets(near, n)
    assert any(mine[s] != close[s] and (mine[s] ^ close[s]) >> 64 == 0 for s in range(n - 3))  # the control: word 0 alone
    return tree, far, near, edge
