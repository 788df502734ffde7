"""Plain Python restatement of transfer bootstrap support on a neighbor-joining tree (andi_hip_nj_transfer,
andi_hip_format_newick_transfer; include/andi_hip.h), twice: leaf sets as Python ints with bin(a ^ b).count("1"), and
-- the fast statement -- unpacked bits as float32 with H = |A| + |B| - 2 A B^T (sums of at most n < 2^24 zeros and ones:
exact).  The labelled Newick text and a parser that reads the float labels back.  What tests/test_transfer_*.py hold the
library to.

Pair record s (0 <= s < n - 3) of a tree defines the leaf set L_s below node n + s.  h(A, B) = |A xor B| over the n
leaves; the transfer distance is d(A, B) = min(h, n - h).  depth[s] = min(|L_s|, n - |L_s|); the transfer index of
branch s in a replicate is min(depth[s] - 1, min over the replicate's pair records t of d(L_s, L_t)); transfer[s] sums
it over the used replicates; a skipped replicate's row is 0xFFFFFFFF."""
import numpy as np

import nj_model

SKIPPED = 0xFFFFFFFF


def leaf_sets(J, n):
    """The leaf set (an int, bit i = leaf i) below node n + s of every pair record s of the n - 2 records J, as built"""
    below = {}
    out = []
    for s in range(max(n - 3, 0)):
        bits = 0
        for v in (int(J[s]["a"]), int(J[s]["b"])):
            bits |= (1 << v) if v < n else below[v]
        below[n + s] = bits
        out.append(bits)
    return out


def _ones(x):
    return bin(x).count("1")


def transfer(tree, reps, skip=None):
    """(depth, transfer, per) as lists: the contract in ints"""
    n = len(tree) + 2
    mine = leaf_sets(tree, n)
    depth = [min(_ones(a), n - _ones(a)) for a in mine]
    total = [0] * len(mine)
    per = []
    for k, rep in enumerate(reps):
        if skip is not None and skip[k]:
            per.append([SKIPPED] * len(mine))
            continue
        theirs = leaf_sets(rep, n)
        row = []
        for s, a in enumerate(mine):
            best = depth[s] - 1
            for b in theirs:
                h = _ones(a ^ b)
                best = min(best, h, n - h)
            row.append(best)
            total[s] += best
        per.append(row)
    return depth, total, per


def bit_matrix(J, n):
    """(n - 3, n) float32 zeros and ones: row s is L_s"""
    X = np.zeros((max(n - 3, 0), n), np.float32)
    for s in range(max(n - 3, 0)):
        for v in (int(J[s]["a"]), int(J[s]["b"])):
            if v < n:
                X[s, v] = 1
            else:
                X[s] += X[v - n]
    return X


def transfer_numpy(tree, reps, skip=None):
    """(depth, transfer, per) as arrays (uint32, uint64, uint32): the same contract through one matrix product per replicate"""
    n = len(tree) + 2
    assert n < 1 << 24
    A = bit_matrix(tree, n)
    size = A.sum(1)
    depth = np.minimum(size, n - size)
    per = np.full((len(reps), len(A)), SKIPPED, np.uint32)
    for k, rep in enumerate(reps):
        if skip is not None and skip[k]:
            continue
        B = bit_matrix(rep, n)
        H = size[:, None] + B.sum(1)[None, :] - 2.0 * (A @ B.T)
        best = np.minimum(H, n - H).min(1)
        per[k] = np.minimum(best, depth - 1).astype(np.uint32)
    used = [k for k in range(len(reps)) if skip is None or not skip[k]]
    total = per[used].astype(np.uint64).sum(0) if used else np.zeros(len(A), np.uint64)
    return depth.astype(np.uint32), total.astype(np.uint64), per


def label(depth, transfer, used):
    """the label's text: %.6g of 1 - transfer / (used * (depth - 1)) in doubles, each operation rounded"""
    return "%.6g" % (1.0 - float(int(transfer)) / (float(int(used)) * float(int(depth) - 1)))


def newick_transfer(J, depth, transfer, used, names, truncate_names=False):
    """andi_hip_format_newick_transfer's text: nj_model.newick's walk, the label directly behind the ")" of pair record s"""
    n = len(names)
    if used == 0 or depth is None or transfer is None or any(int(depth[s]) < 2 for s in range(max(n - 3, 0))):
        return ""
    root = 0 if n == 2 else n - 3
    kids = 2 if n == 2 else 3
    parts = ["("]
    stack = [(root, 0, kids, 0.0)]  # (record, next child, children, own length)
    while stack:
        rec, k, nk, own = stack.pop()
        if k == nk:
            parts.append(")")
            if stack:
                parts.append(label(depth[rec], transfer[rec], used))
            parts.append(";\n" if not stack else ":%.8g" % own)
            continue
        stack.append((rec, k + 1, nk, own))
        if k:
            parts.append(",")
        child = int(J[rec][("a", "b", "c")[k]])
        length = float(J[rec][("la", "lb", "lc")[k]])
        if child < n:
            parts.append(nj_model._leaf(names[child], truncate_names) + ":%.8g" % length)
        else:
            stack.append((child - n, 0, 2, length))
            parts.append("(")
    return "".join(parts)


def parse_labels(text):
    """(labels, unlabelled) of a labelled Newick line with unquoted leaf names: labels maps every internal node's leaf
    set (a frozenset of names, the side away from the root) to its label as a float; unlabelled lists the internal nodes
    below the root that have none."""
    text = text.strip()
    assert text.endswith(";")
    pos, stack, labels, unlabelled = 0, [], {}, []
    while pos < len(text) - 1:
        ch = text[pos]
        if ch == "(":
            stack.append(set())
            pos += 1
        elif ch == ")":
            cur = frozenset(stack.pop())
            if stack:
                stack[-1] |= cur
            end = pos + 1
            while text[end] not in ":,);":
                end += 1
            if end > pos + 1:
                labels[cur] = float(text[pos + 1:end])
            elif stack:
                unlabelled.append(cur)
            pos = end
        elif ch == ",":
            pos += 1
        elif ch == ":":
            end = pos + 1
            while text[end] not in ",);":
                end += 1
            pos = end
        else:
            end = pos
            while text[end] not in ":,()":
                end += 1
            stack[-1].add(text[pos:end])
            pos = end
    return labels, unlabelled


def strip_labels(text):
    """the line without its inner labels: andi_hip_format_newick's text (unquoted names)"""
    import re
    return re.sub(r"\)[^:,);]+", ")", text)
