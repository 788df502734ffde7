"""Rooting without a GPU: the NumPy restatement (tests/root_model.py) against the definition of the ancestor deviations on a
tree that is actually rooted, in exact arithmetic; its x as the minimiser; ultrametric trees, the midpoint, odd trees;
andi_hip_format_newick_rooted read back by a small parser; the new symbols; --help and the usage errors."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import place_model as pm
import root_model as rm
from newick_reader import leafset as _leafset, parse as _parse, splits as _splits
from conftest import ROOT

NEW = ("andi_hip_root", "andi_hip_format_newick_rooted")
CLI = os.path.join(ROOT, "andi_amd", "andi-hip")


def test_declared_exported_and_abi_stays_5():
    from andi_amd import lib
    import andi_amd
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    shipped = C.CDLL(os.path.join(ROOT, "andi_amd", "libandihip.so"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
        assert getattr(L, name) is not None and getattr(shipped, name) is not None
    assert L.andi_hip_abi_version() == 5 and "#define ANDI_HIP_ABI_VERSION 5" in header  # additions only
    assert lib.ROOT.itemsize == 48 and rm.ROOT == lib.ROOT and lib.ROOT_METHODS == rm.METHODS
    assert andi_amd.root is lib.root and andi_amd.newick_rooted is lib.newick_rooted and andi_amd.ROOT is lib.ROOT
    knobs_h = open(os.path.join(ROOT, "andi_amd", "csrc", "knobs.h")).read()
    shipped_list, hooks = knobs_h.split("#define ANDI_KNOB_LIST_HOOKS(X)")
    assert "X(ROOT_GROUP)" in hooks.split("#define ANDI_KNOB_LIST(X)")[0] and "ROOT_GROUP" not in shipped_list


# ---------------------------------------------------------------- the model against the definition
def _dyadic(rng, lo=2, hi=16, unit=64.0):
    return lambda k: rng.integers(lo, hi + 1, k) / unit


class Rooted:
    """the tree J actually rooted at x above the child end of edge v: parent pointers and branch lengths towards the new
    root R; every path sum is taken from the leaf upwards, so with dyadic lengths all of it but the last step is exact"""

    def __init__(self, J, n, v, x):
        parent, L = pm.edges(J, n)
        E = 2 * n - 3
        nbr = {u: [] for u in range(E + 1)}
        for u in range(E):
            if u != v:
                nbr[u].append((int(parent[u]), L[u]))
                nbr[int(parent[u])].append((u, L[u]))
        R = E + 1
        nbr[R] = [(v, x), (int(parent[v]), L[v] - x)]
        nbr[v].append((R, x))
        nbr[int(parent[v])].append((R, L[v] - x))
        self.up = {R: (None, 0.0)}
        todo = [R]
        while todo:
            u = todo.pop()
            for w, l in nbr[u]:
                if w not in self.up:
                    self.up[w] = (u, l)
                    todo.append(w)
        self.R = R

    def chain(self, leaf):
        """the nodes from the leaf up to the root"""
        out, u = [], leaf
        while u is not None:
            out.append(u)
            u = self.up[u][0]
        return out

    def ancestor(self, b, c):
        """the deepest common ancestor of b and c"""
        mine = set(self.chain(b))
        return next(u for u in self.chain(c) if u in mine)

    def dist(self, leaf, anc, number=float):
        """the path length from the leaf up to its ancestor, summed upwards"""
        d, u = number(0), leaf
        while u != anc:
            d = d + number(self.up[u][1])
            u = self.up[u][0]
        return d


def _unrooted_path(J, n, b, c):
    """the path length between two leaves on the tree as it is, exactly"""
    parent, L = pm.edges(J, n)
    up = {}
    d, u = Fraction(0), b
    while u != 2 * n - 3:
        up[u] = d
        d, u = d + Fraction(L[u]), int(parent[u])
    up[u] = d
    d, u = Fraction(0), c
    while u not in up:
        d, u = d + Fraction(L[u]), int(parent[u])
    return d + up[u]


def test_the_models_deviations_are_those_of_a_tree_that_is_rooted_there():
    """For every edge, at the model's x, r of every pair.  A straddling pair's ancestor is the root: the model's
    (2 * d) / p - 1 is the definition's own sequence of operations, so the doubles are equal.  A pair on one side: the
    definition 2 * d(b, anc) / p - 1 in exact arithmetic, rounded once, is the model's (t_b - t_c) / p -- an exact
    difference and one division: this is what guards the closed form."""
    rng = np.random.default_rng(20261021)
    seen = {"straddling": 0, "one side": 0}
    for k in range(36):
        n = 4 + k % 9
        J = pm.random_tree(rng, n, _dyadic(rng))
        t = rm.Table(J)
        x, _, _ = rm.solve_x(t)
        for v in range(t.E):
            tree = Rooted(J, n, v, x[v])
            for b in range(n):
                for c in range(b + 1, n):
                    p = _unrooted_path(J, n, b, c)
                    assert Fraction(t.P[b, c]) == p and t.used[b, c]
                    r = rm.pair_r(t, b, c, x)[v]
                    anc = tree.ancestor(b, c)
                    if anc == tree.R:
                        assert t.below[v, b] != t.below[v, c]
                        want = 2.0 * tree.dist(b, anc) / float(p) - 1.0
                        seen["straddling"] += 1
                    else:
                        assert t.below[v, b] == t.below[v, c]
                        want = float(2 * tree.dist(b, anc, Fraction) / p - 1)
                        assert tree.dist(b, anc, Fraction) + tree.dist(c, anc, Fraction) == p
                        seen["one side"] += 1
                    assert r == want, (n, v, b, c, r, want)
    assert min(seen.values()) > 1000


def test_x_minimises_the_straddling_sum():
    rng = np.random.default_rng(5)
    for k in range(30):
        n = 4 + k % 9
        J = pm.random_tree(rng, n, _dyadic(rng))
        t = rm.Table(J)
        x, _, _ = rm.solve_x(t)
        for v in range(t.E):
            pairs = [(b, c) for b in range(n) for c in range(b + 1, n) if t.below[v, b] != t.below[v, c]]
            ta = [Fraction(t.T[v, b] if t.below[v, b] else t.T[v, c]) for b, c in pairs]
            ps = [Fraction(t.P[b, c]) for b, c in pairs]

            def f(y):
                return sum((2 * (a + y) / p - 1) ** 2 for a, p in zip(ta, ps))

            N = sum((p - 2 * a) / (p * p) for a, p in zip(ta, ps))
            W = sum(1 / (p * p) for p in ps)
            L = Fraction(t.L[v])
            best = min(max(N / (2 * W), Fraction(0)), L)
            for y in [Fraction(0), L, L / 2, best + Fraction(1, 1 << 20), best - Fraction(1, 1 << 20)]:
                if 0 <= y <= L:
                    assert f(best) <= f(y)
            assert abs(Fraction(x[v]) - best) <= Fraction(1, 10 ** 12)


def _ultrametric(rng, n, a, b):
    """(J, edge, x): the records of a random ultrametric tree with heights in 256ths whose root sits x = 2^-b above the
    child end of `edge`; the root's other branch has length 2^-a.  The root's two branches are one edge of J."""
    from andi_amd.lib import NJ_JOIN
    height = {i: 0.0 for i in range(n)}
    active, kids, nxt = list(range(n)), {}, n
    while len(active) > 2:
        i, j = sorted(rng.choice(len(active), 2, replace=False).tolist())
        u, w = active[i], active[j]
        h = max(height[u], height[w]) + float(rng.integers(1, 9)) / 256.0
        del active[j], active[i]
        kids[nxt], height[nxt] = (u, w), h
        active.append(nxt)
        nxt += 1
    A, B = active  # the root's children; A becomes the centre, so it has to be an inner node
    if A < n:
        A, B = B, A
    H = max(height[A] + 2.0 ** -a, height[B] + 2.0 ** -b)  # (dyadic; both branches at least the powers of two)
    # the branch to B is exactly 2^-b iff B decides H; make it so by lifting H's other argument out of the way
    if height[B] + 2.0 ** -b < H:
        return None
    order, ids = [u for u in sorted(kids) if u != A], {i: i for i in range(n)}
    J = np.zeros(n - 2, NJ_JOIN)
    for s, u in enumerate(order):
        l, r = kids[u]
        ids[u] = n + s
        x, y = sorted([(ids[l], height[u] - height[l]), (ids[r], height[u] - height[r])])
        J[s] = (x[0], y[0], -1, 0, x[1], y[1], 0.0)
    l, r = kids[A]
    three = sorted([(ids[l], height[A] - height[l]), (ids[r], height[A] - height[r]), (ids[B], (H - height[A]) + (H - height[B]))])
    J[n - 3] = (three[0][0], three[1][0], three[2][0], 0, three[0][1], three[1][1], three[2][1])
    return J, ids[B], H - height[B]


def _ultrametric_cases(count, seed):
    rng = np.random.default_rng(seed)
    made = 0
    while made < count:
        case = _ultrametric(rng, 4 + made % 14, int(rng.integers(2, 6)), int(rng.integers(2, 6)))
        if case is not None:
            made += 1
            yield case


def test_an_ultrametric_tree_is_rooted_at_its_root():
    for J, edge, x in _ultrametric_cases(40, 11):
        rec, xs, ss = rm.root(J, "mad", per=True)
        assert (rec["edge"], rec["distal"], rec["ss"]) == (edge, x, 0.0) and ss[edge] == 0.0
        assert rec["ss_second"] > 0.0 and rec["pairs"] == (len(J) + 2) * (len(J) + 1) // 2
        score, ambiguity = rm.score(rec)
        assert score == 0.0 and ambiguity == 0.0
        mid = rm.root(J, "midpoint")
        assert (mid["edge"], mid["distal"], mid["ss"], mid["ss_second"]) == (edge, x, 0.0, 0.0)
        assert mid["far_b"] == rec["far_b"] >= 0 and mid["far_c"] == rec["far_c"] > mid["far_b"]


def test_midpoint_follows_one_long_branch_and_mad_does_not():
    """an ultrametric tree one of whose leaves evolved three times as fast: the longest path's midpoint moves onto that
    leaf's side by half of what the branch gained; MAD stays on the true root's edge"""
    checked = 0
    for J, edge, x in _ultrametric_cases(30, 12):
        n = len(J) + 2
        if n < 8:
            continue
        t = rm.Table(J)
        leaf = int(np.nonzero(~t.below[edge, :n])[0][0]) if t.below[edge].sum() > 1 else int(np.nonzero(t.below[edge, :n])[0][0])
        K = J.copy()
        for s in range(n - 2):
            for c, l in (("a", "la"), ("b", "lb"), ("c", "lc")):
                if K[s][c] == leaf and (c != "c" or s == n - 3):
                    K[s][l] = 3.0 * K[s][l]
        mad, mid = rm.root(K, "mad"), rm.root(K, "midpoint")
        assert leaf in (mid["far_b"], mid["far_c"])
        if mad["edge"] == edge:
            assert (mid["edge"], mid["distal"]) != (mad["edge"], mad["distal"])
            checked += 1
    assert checked >= 5


def test_odd_trees_pairs_that_are_not_used():
    rng = np.random.default_rng(13)
    n = 12
    lengths = list(rng.integers(1, 9, 2 * n - 3) / 64.0)
    lengths[7], lengths[9] = 0.0, -3 / 64.0
    it = iter(lengths)
    J = pm.random_tree(rng, n, lambda k: [next(it) for _ in range(k)])
    J[0]["la"], J[0]["lb"] = 0.0, 0.0  # two identical leaves
    exact = {(b, c): _unrooted_path(J, n, b, c) for b in range(n) for c in range(b + 1, n)}
    rec, xs, ss = rm.root(J, "mad", per=True)
    assert exact[(int(J[0]["a"]), int(J[0]["b"]))] == 0
    assert rec["pairs"] == sum(p > 0 for p in exact.values()) < n * (n - 1) // 2
    assert np.isfinite(ss).all() and ((xs >= 0) & (xs <= np.where(pm.edges(J, n)[1] > 0, pm.edges(J, n)[1], 0.0))).all()
    # every pair unusable: SS and x are 0 on every edge and edge 0 is chosen; the midpoint has no pair
    Z = pm.random_tree(rng, 7, lambda k: np.zeros(k))
    rec, xs, ss = rm.root(Z, "mad", per=True)
    assert (rec["edge"], rec["distal"], rec["ss"], rec["ss_second"], rec["pairs"], rec["far_b"], rec["far_c"]) == (0, 0, 0, 0, 0, -1, -1)
    assert not xs.any() and not ss.any()
    assert rm.root(Z, "midpoint").tobytes() == rec.tobytes()


# ---------------------------------------------------------------- andi_hip_format_newick_rooted
def _record_sets(J, n):
    """the leaf set below every node of the records"""
    sets = {i: frozenset([i]) for i in range(n)}
    for s in range(n - 3):
        sets[n + s] = sets[int(J[s]["a"])] | sets[int(J[s]["b"])]
    return sets


def _canon(s, n):
    return s if 0 not in s else frozenset(range(n)) - s


def _check_rooted(J, names, edge, distal, labels):
    from andi_amd import lib
    n = len(names)
    index = {nm: i for i, nm in enumerate(names)}
    parent, L = pm.edges(J, n)
    sets = _record_sets(J, n)
    text = lib.newick_rooted(J, names, edge, distal, labels)
    tree = _parse(text)
    assert len(tree["kids"]) == 2 and tree["label"] == ""
    got = _splits(tree, index, n, {})
    # the root's two branches are the two halves of the edge: the same split twice
    side = _canon(sets[edge], n)
    halves = got.pop(side)
    assert len(halves) == 2
    first, second = tree["kids"]
    assert _leafset(first, index) == sets[edge]  # the child end comes first
    assert first["len"] == "%.8g" % distal and second["len"] == "%.8g" % (L[edge] - distal)
    assert float(first["len"]) + float(second["len"]) == L[edge]
    for half in (first, second):
        want = labels[edge - n] if labels is not None and edge >= n and half["kids"] else ""
        assert half["label"] == (want or "")
    # every other edge once, with its length and its label: unrooting gives the records' tree back
    for v in range(2 * n - 3):
        if v == edge:
            continue
        (length, label), = got.pop(_canon(sets[v], n))
        assert length == "%.8g" % L[v], v
        assert label == ((labels[v - n] or "") if labels is not None and v >= n else ""), v
    assert not got
    # every inner node but the root has two children: the old centre is an ordinary node
    todo = list(tree["kids"])
    while todo:
        node = todo.pop()
        assert len(node["kids"]) in (0, 2)
        todo += node["kids"]
    return text


def _edges_to_try(J, n):
    """a leaf edge, an inner edge next to the old centre, the deepest inner edge, and a leaf edge next to the centre"""
    parent, _ = pm.edges(J, n)
    C = 2 * n - 3
    depth = {C: 0}
    for v in range(C - 1, -1, -1):
        depth[v] = depth[int(parent[v])] + 1
    inner = [v for v in range(n, C)]
    out = [0, max(range(n), key=lambda v: depth[v])]
    out += [v for v in inner if parent[v] == C][:1]
    out += [max(inner, key=lambda v: depth[v])] if inner else []
    out += [v for v in range(n) if parent[v] == C][:1]
    return sorted(set(out))


@pytest.mark.parametrize("shape", ["caterpillar", "balanced", "random"])
def test_rooted_newick_unroots_to_the_records_and_keeps_labels_on_their_edges(shape):
    rng = np.random.default_rng(len(shape))
    for n in (3, 4, 5, 9, 20):
        lengths = rng.integers(2, 17, 2 * n - 3) / 64.0
        it = iter(lengths)
        J = pm.random_tree(rng, n, lambda k: [next(it) for _ in range(k)]) if shape == "random" else getattr(pm, shape)(n, lengths)
        names = ["t%d" % i for i in range(n)]
        labels = ["L%d" % s for s in range(n - 3)]
        if n > 5:
            labels[1] = None  # (an entry may be missing)
        parent, L = pm.edges(J, n)
        for edge in _edges_to_try(J, n):
            for distal in (0.0, L[edge] / 2, L[edge]):
                with_labels = _check_rooted(J, names, edge, distal, labels)
                plain = _check_rooted(J, names, edge, distal, None)
                assert "L" not in plain and (n == 3 or "L" in with_labels)


def test_rooted_newick_on_a_deep_caterpillar_is_not_recursive():
    from andi_amd import lib
    n = 20000
    J = pm.caterpillar(n, np.full(2 * n - 3, 0.5))
    names = ["s%d" % i for i in range(n)]
    text = lib.newick_rooted(J, names, 0, 0.25, None)
    assert text.startswith("(s0:0.25,(s1:0.5,(") and text.count("(") == n - 1 and text.endswith(";\n")
    deep = lib.newick_rooted(J, names, n + 5, 0.25, ["%d" % s for s in range(n - 3)])
    assert deep.count("(") == n - 1 and deep.count(")5:") == 2


def test_rooted_newick_quotes_names_as_the_unrooted_text_does():
    from andi_amd import lib
    rng = np.random.default_rng(3)
    names = ["plain", "has blank", "it's", "a(b)", "c:d;e,f", "0123456789abc"]
    J = pm.random_tree(rng, len(names), _dyadic(rng))
    for truncate in (False, True):
        unrooted = lib.newick(J, names, truncate)
        rooted = lib.newick_rooted(J, names, 2, 0.0, None, truncate)
        leaf = re.compile(r"(?<=[(,])('(?:[^']|'')*'|[^(),:']+):")
        assert sorted(leaf.findall(unrooted)) == sorted(leaf.findall(rooted)) and len(leaf.findall(rooted)) == len(names)
    assert "'it''s'" in rooted and "0123456789:" in rooted and "0123456789a" not in rooted


def test_rooted_newick_refuses_what_it_cannot_walk():
    from andi_amd import lib
    rng = np.random.default_rng(4)
    n = 9
    J = pm.random_tree(rng, n)
    names = ["t%d" % i for i in range(n)]
    assert lib.newick_rooted(J, names, 3, 0.01) != ""
    late = J.copy()
    late[2]["b"] = n + 5  # a child that no earlier record made
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    negative = J.copy()
    negative[1]["a"] = -1
    for bad in (late, twice, negative):
        assert lib.newick_rooted(bad, names, 3, 0.01) == ""
    for edge in (-1, 2 * n - 3):
        assert lib.newick_rooted(J, names, edge, 0.01) == ""
    assert lib.newick_rooted(J, names, 3, float("nan")) == ""
    # the bytes it needs, whatever the cap; a cap too small truncates and terminates
    L = lib.load()
    cn = lib._names(names)
    full = lib.newick_rooted(J, names, 3, 0.01).encode()
    buf = C.create_string_buffer(10)
    assert L.andi_hip_format_newick_rooted(J.ctypes.data, n, cn, 0, 3, 0.01, None, C.cast(buf, C.c_void_p), 10) == len(full)
    assert buf.value == full[:9]
    assert L.andi_hip_format_newick_rooted(J.ctypes.data, n, cn, 0, 3, 0.01, None, None, 0) == len(full)


# ---------------------------------------------------------------- the command line, as far as it goes without a GPU
def _cli(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=60, stdin=subprocess.DEVNULL)


def test_help_names_the_options_and_usage_errors():
    p = _cli(["--help"])
    assert p.returncode == 0
    text = p.stdout.decode()
    assert "--root=METHOD" in text and "--root-report=FILE" in text and "'mad'" in text and "'midpoint'" in text
    assert "goes on requiring an unrooted tree" in text
    p = _cli(["--root=bogus", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "Expected one of 'mad' or 'midpoint' for --root, but 'bogus' was given." in p.stderr.decode()
    p = _cli(["--root-report=/dev/null", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "A root report (--root-report) needs a rooting method" in p.stderr.decode()
