"""Plain Python restatement of bootstrap support on a neighbor-joining tree (andi_hip_nj_support,
andi_hip_format_newick_support; include/andi_hip.h): leaf sets as Python ints used as bitsets, built from the records,
brought to the side without leaf 0, counted by set equality; the labelled Newick text and a parser that reads the
labels back.  What tests/test_support_*.py hold the library to."""
import nj_model


def leaf_sets(J, n):
    """The canonical leaf set (an int, bit i = leaf i; the side without leaf 0) of every pair record of the n - 2 records J"""
    everything = (1 << n) - 1
    below = {}
    out = []
    for s in range(max(n - 3, 0)):
        bits = 0
        for v in (int(J[s]["a"]), int(J[s]["b"])):
            bits |= (1 << v) if v < n else below[v]
        below[n + s] = bits
        out.append(everything & ~bits if bits & 1 else bits)
    return out


def support(tree, reps, skip=None):
    """support[s]: the replicates (rows of reps; those with skip[k] left out) whose tree has pair record s's bipartition"""
    n = len(tree) + 2
    mine = leaf_sets(tree, n)
    out = [0] * len(mine)
    for k, rep in enumerate(reps):
        if skip is not None and skip[k]:
            continue
        theirs = set(leaf_sets(rep, n))
        for s, bits in enumerate(mine):
            out[s] += bits in theirs
    return out


def newick_support(J, support, names, truncate_names=False):
    """andi_hip_format_newick_support's text: nj_model.newick's walk, support[s] directly behind the ")" of pair record s"""
    n = len(names)
    root = 0 if n == 2 else n - 3
    kids = 2 if n == 2 else 3
    parts = ["("]
    stack = [(root, 0, kids, 0.0)]  # (record, next child, children, own length)
    while stack:
        rec, k, nk, own = stack.pop()
        if k == nk:
            parts.append(")")
            if stack and support is not None:
                parts.append("%d" % support[rec])
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
    """(labels, unlabelled, lengths) of a labelled Newick line with unquoted leaf names: labels maps every internal
    node's leaf set (a frozenset of names, the side away from the root) to its integer label, unlabelled lists the
    internal nodes without one, lengths maps every node's set (a leaf: frozenset({name})) to its branch length."""
    text = text.strip()
    assert text.endswith(";")
    pos, stack, labels, unlabelled, lengths = 0, [], {}, [], {}
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
            end = pos + 1
            while text[end].isdigit():
                end += 1
            if end > pos + 1:
                labels[cur] = int(text[pos + 1:end])
            elif stack:
                unlabelled.append(cur)
            pos = end
        elif ch == ",":
            pos += 1
        elif ch == ":":
            end = pos + 1
            while text[end] not in ",);":
                end += 1
            lengths[cur] = float(text[pos + 1:end])
            pos = end
        else:
            end = pos
            while text[end] not in ":,()":
                end += 1
            cur = frozenset([text[pos:end]])
            stack[-1].add(text[pos:end])
            pos = end
    return labels, unlabelled, lengths


def canonical(names_set, names):
    """a set of leaf names as the canonical bitset leaf_sets gives (names[i] is leaf i)"""
    index = {name: i for i, name in enumerate(names)}
    bits = 0
    for name in names_set:
        bits |= 1 << index[name]
    return ((1 << len(names)) - 1) & ~bits if bits & 1 else bits
