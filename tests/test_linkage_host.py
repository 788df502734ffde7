"""Linkage clustering without a GPU: the new entry points' surface, tests/linkage_model.py against a second, scalar
restatement of the contract and against SciPy, the host functions on the records (andi_hip_linkage_cut,
andi_hip_cluster_medoids, andi_hip_cluster_stability, andi_hip_format_newick_linkage) against the model, the argument
checks of andi_hip_linkage and andi_hip_linkage_batch, and the command line's validation of the new options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import linkage_model as lm
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_linkage", "andi_hip_linkage_batch", "andi_hip_linkage_cut", "andi_hip_cluster_medoids",
       "andi_hip_cluster_stability", "andi_hip_format_newick_linkage")


def test_both_libraries_export_the_linkage_entry_points():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        L = C.CDLL(os.path.join(ROOT, "andi_amd", so))
        for name in NEW:
            assert getattr(L, name) is not None, (so, name)
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
    assert "ANDI_LINK_SINGLE = 0, ANDI_LINK_COMPLETE = 1, ANDI_LINK_AVERAGE = 2" in header
    assert lib.load().andi_hip_abi_version() == 5
    assert lib.LINK.itemsize == 24 and lib.LINK == lm.LINK


# ------------------------------------------------- a second restatement of the contract, one operation at a time
def _linkage_scalar(D, method):
    """include/andi_hip.h's linkage contract with Python floats (IEEE doubles, each operation rounded) and plain loops,
    written from the header's text alone: the records as tuples (a, b, size, height)."""
    n = len(D)
    M = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            v = float(D[i][j])
            M[i][j] = M[j][i] = float("inf") if v != v else v
    node, size, active, out = list(range(n)), [1] * n, list(range(n)), []
    for s in range(n - 1):
        best = None  # (NaN?, value, id(x), id(y), slot x, slot y)
        for i in range(len(active)):
            for j in range(i + 1, len(active)):
                x, y = active[i], active[j]
                if node[x] > node[y]:
                    x, y = y, x
                d = M[x][y]
                nan = d != d
                key = (nan, 0.0 if nan else d + 0.0, node[x], node[y])  # (-0.0 == +0.0 in the comparison)
                if best is None or key < best[:4]:
                    best = key + (x, y)
        a, b = best[4], best[5]
        na, nb = size[a], size[b]
        out.append((node[a], node[b], na + nb, M[a][b]))
        u, o = min(a, b), max(a, b)
        for k in active:
            if k == a or k == b:
                continue
            da, db = M[a][k], M[b][k]
            if method == "single":
                v = db if db < da else da
            elif method == "complete":
                v = db if db > da else da
            else:
                v = (float(na) * da + float(nb) * db) / float(na + nb)
            M[u][k] = M[k][u] = v
        node[u], size[u] = n + s, na + nb
        active.remove(o)
    return out


def _as_records(rows):
    Z = np.zeros(len(rows), lm.LINK)
    for s, (a, b, size, h) in enumerate(rows):
        Z[s] = (a, b, size, 0, h)
    return Z


def _same(got, want):
    """ids and sizes exactly; heights by their bits, except that a NaN only has to be a NaN"""
    for f in ("a", "b", "size"):
        assert (got[f] == want[f]).all(), f
    assert (got["pad"] == 0).all()
    g, w = got["height"], want["height"]
    assert (np.isnan(g) == np.isnan(w)).all()
    ok = ~np.isnan(w)
    assert (g[ok].view(np.uint64) == w[ok].view(np.uint64)).all()


def _cases(seed):
    """random, a lower triangle of garbage, small integers (many ties), duplicated leaves at +0.0 and -0.0, pairs without a
    distance (NaN and +inf), negative values, and entries whose averages overflow to +inf, -inf and NaN"""
    rng = np.random.default_rng(seed)
    for n in (2, 3, 4, 5, 7, 12):
        A = rng.uniform(0.0, 1.0, (n, n))
        yield "random", np.triu(A, 1) + np.triu(A, 1).T
        yield "garbage below", np.triu(A, 1) + np.tril(rng.uniform(-5, 5, (n, n)))
        B = np.triu(rng.integers(0, 3, (n, n)).astype(float), 1)
        yield "small integers", B + B.T
        yield "all ties", np.ones((n, n)) - np.eye(n)
        idx = np.sort(rng.integers(0, max(2, n // 2), n))
        base = rng.uniform(0.0, 1.0, (n, n))
        dup = (base + base.T)[np.ix_(idx, idx)]
        same = idx[:, None] == idx[None, :]
        dup[same] = np.where(rng.integers(0, 2, (n, n)) == 1, -0.0, 0.0)[same]
        yield "duplicated leaves", dup
        G = np.triu(A, 1) + np.triu(A, 1).T
        G[rng.uniform(size=(n, n)) < 0.3] = np.nan
        G[rng.uniform(size=(n, n)) < 0.1] = np.inf
        yield "missing", G
        yield "negative", np.triu(A - 0.5, 1)
        H = rng.choice([1e308, -1e308, 1.7e308, 1.0, np.inf], (n, n))
        yield "overflow", np.triu(H, 1)
    # 0 and 1 join first; their averages with 2 and with 3 overflow to -inf; (2, node) joins at -inf; the last pair is
    # (1 * inf + 2 * -inf) / 3 = NaN
    big = -1.6e308
    yield "overflow", np.array([[0, -1.7e308, big, big], [0, 0, big, big], [0, 0, 0, np.inf], [0, 0, 0, 0]])


def test_the_model_is_the_scalar_restatement():
    seen = set()
    for seed in range(3):
        for name, D in _cases(seed):
            for method in lm.METHODS:
                want = _as_records(_linkage_scalar(D, method))
                _same(lm.linkage(D, method), want)
                if name == "overflow" and method == "average":
                    seen |= {"nan" for v in want["height"] if np.isnan(v)} | {"inf" for v in want["height"] if np.isinf(v)}
    assert seen == {"nan", "inf"}  # (the overflow cases do reach both)


def test_the_single_linkage_tie_a_cache_without_rescans_gets_wrong():
    # leaves 1 and 2 are both nearest to leaf 0 (at 1) and as near to each other; 0 joins 3 first.  Then (1, 2) at 1 comes
    # before (1, node) at 1: the new node has the largest id
    D = np.array([[0, 1, 1, 0.5], [0, 0, 1, 2], [0, 0, 0, 2], [0, 0, 0, 0]], float)
    Z = lm.linkage(D, "single")
    assert [(int(z["a"]), int(z["b"])) for z in Z] == [(0, 3), (1, 2), (4, 5)]
    _same(Z, _as_records(_linkage_scalar(D, "single")))


def test_a_prefix_of_the_model_is_the_whole_run_cut_short():
    rng = np.random.default_rng(12)
    for n in (2, 3, 7, 60):
        A = np.triu(rng.integers(0, 3, (n, n)).astype(float), 1)
        for method in lm.METHODS:
            Z = lm.linkage(A, method)
            for k in sorted({0, 1, n // 3, n - 2, n - 1, n}):
                P = lm.linkage(A, method, steps=k)
                assert P.dtype == Z.dtype and P.tobytes() == Z[:max(k, 0)].tobytes(), (n, k)


# ------------------------------------------------- the model against SciPy
def _partition(labels):
    return {frozenset(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels)}


@pytest.mark.parametrize("n", [5, 64, 200])
def test_the_model_against_scipy(n):
    pytest.importorskip("scipy")
    from scipy.cluster import hierarchy
    from scipy.spatial.distance import squareform
    for seed in (100 * n + 1, 100 * n + 2):
        A = np.random.default_rng(seed).uniform(0.0, 1.0, (n, n))
        D = np.triu(A, 1) + np.triu(A, 1).T
        for method in lm.METHODS:
            Z = lm.linkage(D, method)
            S = hierarchy.linkage(squareform(D, checks=False), method)
            got, want = np.sort(Z["height"]), np.sort(S[:, 2])
            if method == "average":
                rel = np.abs(got - want) / want
                print("average linkage, n = %d, seed %d: largest relative difference of a height %.3g" % (n, seed, rel.max()))
                assert (rel <= 1e-12).all()
            else:
                assert (got.view(np.uint64) == want.view(np.uint64)).all(), (method, seed)
            assert sorted(Z["size"].tolist()) == sorted(S[:, 3].astype(int).tolist())
            for t in (want[:-1] + want[1:]) * 0.5:  # midway between consecutive heights
                assert _partition(lm.cut(Z, t)) == _partition(hierarchy.fcluster(S, t, "distance")), (method, seed, t)


# ------------------------------------------------- andi_hip_linkage_cut
def test_cut_at_every_kind_of_threshold():
    from andi_amd import lib
    rng = np.random.default_rng(3)
    for n in (2, 3, 9, 40):
        A = np.triu(rng.integers(1, 6, (n, n)).astype(float), 1)
        for method in lm.METHODS:
            Z = lm.linkage(A, method)
            h = np.unique(Z["height"])
            ts = [h[0] - 1.0, h[-1] + 1.0, np.inf, 0.0, np.nan] + h.tolist() + ((h[:-1] + h[1:]) * 0.5).tolist()
            for t in ts:
                got = lib.linkage_cut(Z, t)
                assert got.dtype == np.uint32 and (got == lm.cut(Z, t)).all(), (n, method, t)
            assert (lib.linkage_cut(Z, h[0] - 1.0) == np.arange(n)).all()  # below the least height: every leaf alone
            assert (lib.linkage_cut(Z, np.inf) == 0).all() and (lib.linkage_cut(Z, h[-1]) == 0).all()


def test_cut_of_records_with_an_inversion_keeps_the_subtree_whole():
    from andi_amd import lib
    # ((0,1) at 2.0, then (2, node 4) at 1.5 -- an inversion --, then (3, node 5) at 3.0
    Z = _as_records([(0, 1, 2, 2.0), (2, 4, 3, 1.5), (3, 5, 4, 3.0)])
    assert lib.linkage_cut(Z, 1.7).tolist() == [0, 1, 2, 3]  # node 5 is low enough but its child 4 is not closed
    assert lib.linkage_cut(Z, 2.0).tolist() == [0, 0, 0, 1]
    assert lib.linkage_cut(Z, 3.0).tolist() == [0, 0, 0, 0]
    for t in (1.0, 1.5, 1.7, 2.0, 2.5, 3.0):
        assert (lib.linkage_cut(Z, t) == lm.cut(Z, t)).all()
    # labels are numbered by first appearance in ascending leaf id
    Z = _as_records([(2, 3, 2, 1.0), (0, 1, 2, 1.0), (4, 5, 4, 9.0)])
    assert lib.linkage_cut(Z, 1.0).tolist() == [0, 0, 1, 1]
    Z = _as_records([(1, 3, 2, 1.0), (0, 2, 2, 5.0), (4, 5, 4, 9.0)])
    assert lib.linkage_cut(Z, 1.0).tolist() == [0, 1, 2, 1]


def test_cut_refuses_records_that_are_no_tree():
    from andi_amd import lib
    L = lib.load()
    good = _as_records([(0, 1, 2, 1.0), (2, 4, 3, 2.0), (3, 5, 4, 3.0)])
    labels, k = np.zeros(4, np.uint32), C.c_size_t(0)
    assert L.andi_hip_linkage_cut(good.ctypes.data, 4, 5.0, labels.ctypes.data, C.byref(k)) == 0 and k.value == 1
    for s, field, value in [(0, "a", -1), (0, "b", 4), (1, "b", 5), (1, "a", 0), (2, "b", 4), (2, "a", 7), (0, "b", 0)]:
        Z = good.copy()
        Z[field][s] = value  # out of range, a later record's node, a node twice, a child twice in one record
        assert L.andi_hip_linkage_cut(Z.ctypes.data, 4, 5.0, labels.ctypes.data, C.byref(k)) == 1, (s, field, value)
        with pytest.raises(lib.AndiHipError):
            lib.linkage_cut(Z, 5.0)
    assert L.andi_hip_linkage_cut(None, 4, 5.0, labels.ctypes.data, C.byref(k)) == 1
    assert L.andi_hip_linkage_cut(good.ctypes.data, 4, 5.0, None, C.byref(k)) == 1
    assert L.andi_hip_linkage_cut(good.ctypes.data, 4, 5.0, labels.ctypes.data, None) == 1
    assert L.andi_hip_linkage_cut(good.ctypes.data, 1, 5.0, labels.ctypes.data, C.byref(k)) == 1
    assert L.andi_hip_linkage_cut(good.ctypes.data, 65536, 5.0, labels.ctypes.data, C.byref(k)) == 1


def test_cut_of_a_65535_leaf_caterpillar():
    from andi_amd import lib
    n = 65535
    Z = _caterpillar(n)
    labels = lib.linkage_cut(Z, float(n // 2))
    assert (labels[:n // 2 + 1] == 0).all() and (labels[n // 2 + 1:] == np.arange(1, n - n // 2)).all()


def _caterpillar(n):
    """leaf 0 and 1 at height 1, that node and leaf 2 at height 2, ...: the deepest tree there is"""
    Z = np.zeros(n - 1, lm.LINK)
    Z["a"][0], Z["b"][0] = 0, 1
    Z["a"][1:] = np.arange(2, n)
    Z["b"][1:] = n + np.arange(n - 2)
    Z["size"] = np.arange(2, n + 1)
    Z["height"] = np.arange(1, n)
    return Z


# ------------------------------------------------- medoids and stability
def test_medoids_match_the_model():
    from andi_amd import lib
    rng = np.random.default_rng(8)
    for n in (2, 5, 30):
        A = rng.uniform(0.0, 1.0, (n, n))
        D = np.triu(A, 1) + np.tril(rng.uniform(-5, 5, (n, n)))  # (the lower triangle and the diagonal are not read)
        for k in (1, 2, max(n // 3, 1)):
            labels = np.r_[np.arange(k), rng.integers(0, k, n - k)].astype(np.uint32)
            got = lib.cluster_medoids(D, labels)
            assert got.dtype == np.uint32 and (got == lm.medoids(D, labels)).all(), (n, k)
            assert (labels[got] == np.arange(k)).all()


def test_medoids_with_a_missing_distance_and_with_ties():
    from andi_amd import lib
    # cluster 0 = {0, 1, 2, 3}: the pair (0, 3) has no distance, so 0 and 3 have a sum of +inf; 1 and 2 tie at 3.0
    D = np.zeros((6, 6))
    D[0, 1], D[0, 2], D[0, 3], D[1, 2], D[1, 3], D[2, 3] = 1.0, 1.0, np.nan, 1.0, 1.0, 1.0
    D[4, 5] = 7.0
    D[:4, 4:] = 50.0
    labels = np.array([0, 0, 0, 0, 1, 1], np.uint32)
    assert lib.cluster_medoids(D, labels).tolist() == [1, 4] == lm.medoids(D, labels).tolist()
    D[0, 3] = np.inf
    assert lib.cluster_medoids(D, labels).tolist() == [1, 4]
    # every member without a distance to some other: all sums +inf, the smallest id
    D[:4, :4] = np.nan
    assert lib.cluster_medoids(D, labels).tolist() == [0, 4] == lm.medoids(D, labels).tolist()
    # a NaN sum (inf - inf, from a negative overflow) orders last
    E = np.zeros((4, 4))
    E[0, 1], E[0, 2], E[0, 3], E[1, 2], E[1, 3], E[2, 3] = -1.7e308, -1.7e308, np.inf, 1.0, 1.0, 1.0
    lab = np.zeros(4, np.uint32)  # leaf 0: (-inf) + inf = NaN; leaves 1 and 2 tie at -1.7e308
    assert lib.cluster_medoids(E, lab).tolist() == lm.medoids(E, lab).tolist() == [1]
    # bad arguments: a label beyond the clusters, an empty cluster, a -inf
    L = lib.load()
    out = np.zeros(6, np.uint32)
    assert L.andi_hip_cluster_medoids(D.ctypes.data, 6, labels.ctypes.data, 1, out.ctypes.data) == 1
    assert L.andi_hip_cluster_medoids(D.ctypes.data, 6, labels.ctypes.data, 3, out.ctypes.data) == 1
    assert L.andi_hip_cluster_medoids(None, 6, labels.ctypes.data, 2, out.ctypes.data) == 1
    D[1, 2] = -np.inf
    assert L.andi_hip_cluster_medoids(D.ctypes.data, 6, labels.ctypes.data, 2, out.ctypes.data) == 1


def test_stability_matches_the_model_and_adds_up_over_chunks():
    from andi_amd import lib
    rng = np.random.default_rng(21)
    n, count = 24, 17
    labels = np.r_[np.arange(5), rng.integers(0, 5, n - 5)].astype(np.uint32)
    reps = np.zeros((count, n), np.uint32)
    for k in range(count):
        r = labels.copy()
        if k % 3 == 1:  # one cluster split in two
            r[np.flatnonzero(labels == k % 5)[0]] = 5
        elif k % 3 == 2:  # two clusters merged
            r[labels == 1] = 0
        perm = rng.permutation(n)[:int(r.max()) + 1]  # any numbering, labels below n
        reps[k] = perm[r]
    reps[3] = np.arange(n)
    reps[4] = 0
    want = lm.stability(labels, reps)
    got = lib.cluster_stability(labels, reps)
    assert got.dtype == np.uint32 and (got == want).all() and 0 < want.min() and want.max() < count
    for cutpoint in (1, 5, 16):
        parts = lib.cluster_stability(labels, reps[:cutpoint]) + lib.cluster_stability(labels, reps[cutpoint:])
        assert (parts == want).all(), cutpoint
    L = lib.load()
    out = np.zeros(n, np.uint32)
    reps[2, 7] = n  # a replicate's label out of range
    assert L.andi_hip_cluster_stability(labels.ctypes.data, 5, reps.ctypes.data, n, count, out.ctypes.data) == 1
    assert L.andi_hip_cluster_stability(labels.ctypes.data, 4, reps.ctypes.data, n, 2, out.ctypes.data) == 1
    assert L.andi_hip_cluster_stability(None, 5, reps.ctypes.data, n, 2, out.ctypes.data) == 1


# ------------------------------------------------- andi_hip_format_newick_linkage
@pytest.mark.parametrize("n", [2, 3, 4, 50])
def test_newick_matches_the_model(n):
    import nj_model
    from andi_amd import lib
    rng = np.random.default_rng(n)
    names = ["taxon_%d" % i for i in range(n)]
    for method in lm.METHODS:
        Z = lm.linkage(rng.uniform(0.0, 1.0, (n, n)), method)
        text = lib.newick_linkage(Z, names)
        assert text == lm.newick(Z, names) and text.endswith(");\n")
        leaves, _, lengths = nj_model.parse_newick(text)
        assert sorted(leaves) == sorted(names) and text.count("(") == text.count(")") == n - 1
        assert all(v >= 0 for v in lengths.values())
    if n == 2:
        assert lib.newick_linkage(_as_records([(0, 1, 2, 0.25)]), ["a", "b"]) == "(a:0.25,b:0.25);\n"


def test_newick_quotes_truncates_and_keeps_negative_lengths():
    from andi_amd import lib
    names = ["plain", "with blank", "it's", "a:b", "x,y", "(p)", "[q]", "semi;colon", "tab\there", "averyverylongname",
             "long name's quoted"]
    n = len(names)
    Z = lm.linkage(np.random.default_rng(1).uniform(0.1, 1.0, (n, n)), "average")
    for trunc in (False, True):
        assert lib.newick_linkage(Z, names, truncate_names=trunc) == lm.newick(Z, names, truncate_names=trunc)
    text = lib.newick_linkage(Z, names)
    assert "'with blank'" in text and "'it''s'" in text and "plain:" in text and "'tab\there'" in text
    assert "averyveryl:" in lib.newick_linkage(Z, names, truncate_names=True)
    inv = _as_records([(0, 1, 2, 2.0), (2, 4, 3, 1.5), (3, 5, 4, 3.0)])  # an inversion: a negative branch
    assert lib.newick_linkage(inv, list("abcd")) == "(d:3,(c:1.5,(a:2,b:2):-0.5):1.5);\n" == lm.newick(inv, list("abcd"))


def test_newick_return_value_and_a_small_cap():
    from andi_amd import lib
    n = 12
    Z = lm.linkage(np.random.default_rng(3).uniform(0.1, 1.0, (n, n)), "complete")
    names = ["n%d" % i for i in range(n)]
    full = lm.newick(Z, names).encode()
    L = lib.load()
    for cap in (0, 1, 7, len(full), len(full) + 1):
        buf = C.create_string_buffer(b"\x7f" * (cap + 4))
        need = L.andi_hip_format_newick_linkage(Z.ctypes.data, n, lib._names(names), 0, C.cast(buf, C.c_void_p) if cap else None,
                                                cap)
        assert need == len(full), cap
        if cap:
            k = min(len(full), cap - 1)
            assert buf.raw[:k] == full[:k] and buf.raw[k] == 0, cap
            assert buf.raw[cap:cap + 4] == b"\x7f" * 4  # nothing beyond cap


def test_newick_of_a_65535_leaf_caterpillar():
    from andi_amd import lib
    n = 65535
    Z = _caterpillar(n)
    names = ["t%d" % i for i in range(n)]
    text = lib.newick_linkage(Z, names)
    assert text.startswith("(t65534:65534,(t65533:65533,(t65532:65532,")
    assert text.endswith("(t2:2,(t0:1,t1:1):1):1" + "):1" * (n - 4) + ");\n")
    assert text == lm.newick(Z, names) and text.count("(") == n - 1


def test_newick_refuses_a_branch_that_is_not_finite_and_records_that_are_no_tree():
    from andi_amd import lib
    names = list("abcd")
    for h in (np.inf, np.nan, -np.inf):
        for s in range(3):
            Z = _as_records([(0, 1, 2, 1.0), (2, 4, 3, 2.0), (3, 5, 4, 3.0)])
            Z["height"][s] = h
            assert lib.newick_linkage(Z, names) == "" == lm.newick(Z, names), (h, s)
    Z = _as_records([(0, 1, 2, -1.7e308), (2, 4, 3, 1.7e308), (3, 5, 4, 1.7e308)])  # finite heights, a difference that is not
    assert lib.newick_linkage(Z, names) == "" == lm.newick(Z, names)
    Z = _as_records([(0, 1, 2, 1.0), (2, 5, 3, 2.0), (3, 4, 4, 3.0)])  # a node no earlier record made
    assert lib.newick_linkage(Z, names) == ""
    buf = C.create_string_buffer(b"\x7f" * 8)
    assert lib.load().andi_hip_format_newick_linkage(Z.ctypes.data, 4, lib._names(names), 0, C.cast(buf, C.c_void_p), 8) == 0
    assert buf.raw[0] == 0


# ------------------------------------------------- argument checks, before any HIP call
def test_linkage_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((2, 4, 4))
    Z = np.zeros((2, 3), lib.LINK)
    bad = np.zeros(2, np.int64)
    d, z, b = D.ctypes.data, Z.ctypes.data, bad.ctypes.data
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, d, 4, 2, z), (None, None, 4, 2, z), (None, d, 4, 2, None), (None, d, 1, 2, z), (None, d, 0, 2, z),
                 (None, d, 65536, 2, z), (None, d, 4, 3, z), (None, d, 4, -1, z)]:
        assert L.andi_hip_linkage(*args) == 1, args
    for args in [(None, d, 4, 2, 2, z, b), (None, None, 4, 2, 2, z, b), (None, d, 4, 2, 2, None, b), (None, d, 4, 2, 2, z, None),
                 (None, d, 4, 0, 2, z, b), (None, d, 1, 2, 2, z, b), (None, d, 65536, 2, 2, z, b), (None, d, 4, 2, 3, z, b),
                 (None, d, 4, 2, -1, z, b)]:
        assert L.andi_hip_linkage_batch(*args) == 1, args
    with pytest.raises(ValueError):
        lib.linkage(None, D[0], "ward")


# ------------------------------------------------- the command line's validation (no GPU is reached)
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n%s\n" % (name, seq))
    return str(path)


def test_cli_lists_the_new_options():
    p = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    text = p.stdout.decode()
    assert p.returncode == 0
    for option in ("--linkage=METHOD", "--dendrogram=FILE", "--clusters=FILE", "--threshold=T"):
        assert option in text, option


_WITH_REFERENCE = " not available together with --reference or --reference-list."
_NO_MATRICES = " not available together with --trees-only: there are no matrices to cluster."
_REFUSALS = [  # (options beside the two FASTA files, with a reference?, the line on stderr behind "andi-hip: ")
    (["--clusters=C"], False, "Clusters (--clusters) need a threshold: give --threshold=T."),
    (["--threshold=0.05"], False, "A threshold (--threshold) needs somewhere to go: give --clusters=FILE."),
    (["--clusters=C", "--threshold=x"], False, "Expected a finite number of at least 0 for --threshold, but 'x' was given."),
    (["--clusters=C", "--threshold=-0.5"], False,
     "Expected a finite number of at least 0 for --threshold, but '-0.5' was given."),
    (["--clusters=C", "--threshold=inf"], False, "Expected a finite number of at least 0 for --threshold, but 'inf' was given."),
    (["--clusters=C", "--threshold=nan"], False, "Expected a finite number of at least 0 for --threshold, but 'nan' was given."),
    (["--clusters=C", "--threshold=0.1x"], False,
     "Expected a finite number of at least 0 for --threshold, but '0.1x' was given."),
    (["--dendrogram=D", "--linkage=ward"], False,
     "Expected one of 'single', 'complete' or 'average' for --linkage, but 'ward' was given."),
    (["--dendrogram=D"], True, "A dendrogram (--dendrogram) is" + _WITH_REFERENCE),
    (["--clusters=C", "--threshold=0.05"], True, "Clusters (--clusters) are" + _WITH_REFERENCE),
    (["--trees-only", "-b", "3", "--tree=T", "--dendrogram=D"], False, "A dendrogram (--dendrogram) is" + _NO_MATRICES),
    (["--trees-only", "-b", "3", "--tree=T", "--clusters=C", "--threshold=0.05"], False,
     "Clusters (--clusters) are" + _NO_MATRICES),
    (["--trees-only", "-b", "3", "--dendrogram=D"], False, "A dendrogram (--dendrogram) is" + _NO_MATRICES),
]


@pytest.mark.parametrize("options,reference,line", _REFUSALS)
def test_cli_refuses_with_these_words(tmp_path, options, reference, line):
    a = _fasta(tmp_path / "a.fa", "a", "ACGT" * 400)
    b = _fasta(tmp_path / "b.fa", "b", "ACGA" * 400)
    args = [o[:o.index("=") + 1] + str(tmp_path / o[o.index("=") + 1:]) if o[:o.index("=")] in ("--dendrogram", "--clusters", "--tree")
            else o for o in options if "=" in o] + [o for o in options if "=" not in o]
    args += ["--reference=" + a, b] if reference else [a, b]
    p = subprocess.run([CLI] + args, capture_output=True, timeout=60)
    # the whole line and the exit status; nothing printed, no file made (the refusals come before any file is opened)
    assert (p.returncode, p.stdout, p.stderr.decode()) == (1, b"", "andi-hip: " + line + "\n")
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.fa"]
