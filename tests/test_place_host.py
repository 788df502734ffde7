"""Placement on a tree without a GPU: the NumPy restatement (tests/place_model.py) recovers a point put on a tree; the
host functions around andi_hip_place -- andi_hip_parse_newick (the inverse of andi_hip_format_newick),
andi_hip_distances_rect, andi_hip_format_jplace -- and the argument checks that come before any HIP call."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import place_model as pm
import support_model
from conftest import ROOT

NEW = ("andi_hip_place", "andi_hip_distances_rect", "andi_hip_parse_newick", "andi_hip_format_jplace")


def test_declared_exported_and_abi_stays_5():
    from andi_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    shipped = C.CDLL(os.path.join(ROOT, "andi_amd", "libandihip.so"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
        assert getattr(L, name) is not None and getattr(shipped, name) is not None
    assert L.andi_hip_abi_version() == 5  # additions only
    assert lib.PLACEMENT.itemsize == 32 and pm.PLACEMENT == lib.PLACEMENT
    knobs_h = open(os.path.join(ROOT, "andi_amd", "csrc", "knobs.h")).read()
    shipped_list, hooks = knobs_h.split("#define ANDI_KNOB_LIST_HOOKS(X)")
    assert "X(PLACE_GROUP)" in hooks.split("#define ANDI_KNOB_LIST(X)")[0] and "PLACE_GROUP" not in shipped_list


def _sixty_fourths(rng, lo, hi):
    return lambda k: rng.integers(lo, hi + 1, k) / 64.0


def _recovery_cases(count, seed):
    """(J, n, v, x, p): a random binary tree, n from 3 to 19, lengths multiples of 1/64; a point on edge v, x above its
    child end, hanging by p -- both multiples of 1/64; x is 0 or the edge's length in some cases"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = 3 + k % 17
        J = pm.random_tree(rng, n, _sixty_fourths(rng, 2, 16))
        _, L = pm.edges(J, n)
        v = int(rng.integers(2 * n - 3))
        x = float(rng.integers(1, int(L[v] * 64))) / 64.0  # 0 < x < L
        if k % 10 == 7:
            x = 0.0
        if k % 10 == 8:
            x = float(L[v])
        p = float(rng.integers(0 if k % 5 == 0 else 1, 9)) / 64.0
        yield J, n, v, x, p, float(L[v])


def test_the_model_recovers_a_point_on_the_tree():
    for J, n, v, x, p, L in _recovery_cases(200, 20261019):
        d = pm.point_distances(J, n, v, x, p)[None, :]
        ols, fm = pm.place(J, d, "ols")[0], pm.place(J, d, "fm")[0]
        assert ols["used"] == n and fm["used"] == n
        assert ols["pendant"] == p and ols["err"] == 0.0  # all the arithmetic is exact there
        assert abs(fm["pendant"] - p) <= 1e-9 and fm["err"] < 1e-24
        if 0.0 < x < L:
            assert ols["edge"] == v and ols["distal"] == x
            assert fm["edge"] == v and abs(fm["distal"] - x) <= 1e-9
        # else the point is a node that three edges share: any of them, at its end


def test_model_edge_rules():
    rng = np.random.default_rng(5)
    n = 7
    J = pm.random_tree(rng, n)
    d = pm.point_distances(J, n, 3, 0.004, 0.02)
    for method in ("ols", "fm"):
        one = np.full(n, np.nan)
        one[2] = 0.3
        out = pm.place(J, np.stack([one, np.full(n, np.nan), np.full(n, np.inf)]), method)
        assert out["edge"].tolist() == [-1, -1, -1] and out["used"].tolist() == [1, 0, 0]
        assert (out["err"] == np.inf).all() and (out["distal"] == 0).all() and (out["pendant"] == 0).all()
        hole = d.copy()
        hole[4] = np.nan  # the whole side below edge 4
        out, err, x, p = pm.place(J, hole[None, :], method, per=True)
        assert err[0, 4] == np.inf and x[0, 4] == 0 and p[0, 4] == 0 and out[0]["used"] == n - 1 and out[0]["edge"] == 3
    at = d.copy()
    at[5] = 0.0
    at[1] = -0.0
    out, err, x, p = pm.place(J, at[None, :], "fm", per=True)
    assert (out[0]["edge"], out[0]["distal"], out[0]["pendant"], out[0]["err"]) == (1, 0.0, 0.0, 0.0)  # the FIRST such leaf
    assert err[0, 1] == 0.0 and np.isinf(np.delete(err[0], 1)).all() and not x.any() and not p.any()
    assert pm.place(J, at[None, :], "ols")[0]["err"] > 0.0  # no special rule


# ---------------------------------------------------------------- andi_hip_parse_newick
def _edge_lengths(J, n):
    """{canonical leaf set of an edge's child side: its length} of the 2n - 3 edges"""
    everything = (1 << n) - 1
    sets = support_model.leaf_sets(J, n)

    def canonical(v):
        bits = (1 << v) if v < n else sets[v - n]
        return everything & ~bits if bits & 1 else bits

    out = {}
    for s in range(n - 2):
        for c, l in (("a", "la"), ("b", "lb"), ("c", "lc"))[:3 if s == n - 3 else 2]:
            out[canonical(int(J[s][c]))] = float(J[s][l])
    assert len(out) == 2 * n - 3
    return out


@pytest.mark.parametrize("n", [3, 4, 5, 8, 33, 200])
def test_parse_newick_inverts_format_newick(n):
    from andi_amd import lib
    rng = np.random.default_rng(n)
    names = ["L%d" % i for i in range(n)]
    shapes = [pm.random_tree(rng, n), pm.caterpillar(n, rng.uniform(-0.01, 0.1, 2 * n - 3)),
              pm.balanced(n, rng.uniform(0.0, 0.1, 2 * n - 3))]
    for J in shapes:
        J1 = lib.parse_newick(lib.newick(J, names), names)
        want = {k: float("%.8g" % v) for k, v in _edge_lengths(J, n).items()}
        assert _edge_lengths(J1, n) == want  # the splits and the lengths of J
        pairs, last = J1[:n - 3], J1[n - 3]
        assert (pairs["a"] < pairs["b"]).all() and (pairs["c"] == -1).all() and last["a"] < last["b"] < last["c"]
        t = lib.newick(J1, names)
        assert lib.newick(lib.parse_newick(t, names), names) == t  # a fixed point
        # labels behind ")" are not looked at; blanks and line ends between tokens neither
        labelled = lib.newick(J, names, support=rng.integers(0, 100, max(n - 3, 0)))
        spaced = labelled.replace(",", " ,\n ").replace(":", " : ").replace(";", " ;\n\n")
        for text in (labelled, spaced, lib.newick_transfer(J, np.full(max(n - 3, 1), 2), np.ones(max(n - 3, 1)), 3, names)):
            J2 = lib.parse_newick(text, names)
            assert J2.tobytes() == lib.parse_newick(lib.newick(J, names), names).tobytes()


def test_parse_newick_names():
    from andi_amd import lib
    rng = np.random.default_rng(9)
    names = ["a b", "it's", "(x)", "plain", "semi;colon", "a_very_long_name_1", "a_very_long_name_2"]
    n = len(names)
    J = pm.random_tree(rng, n)
    text = lib.newick(J, names)
    assert "'it''s'" in text and "'a b'" in text
    J1 = lib.parse_newick(text, names)
    assert _edge_lengths(J1, n) == {k: float("%.8g" % v) for k, v in _edge_lengths(J, n).items()}
    # truncated, both long names are 'a_very_lon': the text then holds that name twice
    with pytest.raises(lib.AndiHipError, match="duplicate name 'a_very_lon'"):
        lib.parse_newick(lib.newick(J, names, truncate_names=True), names, truncate_names=True)
    short = names[:6]
    Js = pm.random_tree(rng, 6)
    cut = lib.newick(Js, short, truncate_names=True)
    assert "a_very_lon:" in cut
    assert lib.newick(lib.parse_newick(cut, short, truncate_names=True), short, truncate_names=True) == \
        lib.newick(lib.parse_newick(lib.newick(Js, short), short), short, truncate_names=True)
    with pytest.raises(lib.AndiHipError, match="unknown name 'a_very_lon'"):
        lib.parse_newick(cut, short)


@pytest.mark.parametrize("text, message, offset", [
    ("(A:1,B:1);", "the root has 2 subtrees, not three", 8),
    ("((A:1,B:1):1,(C:1,D:1):1);", "the root has 2 subtrees, not three", 24),
    ("(A:1,B:1,C:1,D:1);", "the root has more than three subtrees", 15),
    ("(A:1,B:1,(C:1,D:1,E:1):1);", "an inner node has more than two children", 20),
    ("(A:1,B:1,(C:1):1,D:1);", "an inner node has 1 child, not two", 13),
    ("(A:1,B,C:1);", "missing branch length", 6),
    ("(A:1,B:,C:1);", "missing branch length", 7),
    ("(A:1,(B:1,C:1),D:1);", "missing branch length", 14),
    ("(A:1,B:inf,C:1);", "the branch length is not finite", 7),
    ("(A:1,B:nan,C:1);", "the branch length is not finite", 7),
    ("(A:1,B:1e999,C:1);", "the branch length is not finite", 7),
    ("(A:1,B:1,X:1);", "unknown name 'X'", 9),
    ("(A:1,B:1,:1);", "unknown name ''", 9),
    ("(A:1,B:1,A:1);", "duplicate name 'A'", 9),
    ("(A:1,B:1,C:1);", "missing name 'D'", 14),
    ("(A:1,B:1,(C:1,D:1):1); (", "trailing text behind the tree", 23),
    ("(A:1,B:1,(C:1,D:1):1)", "expected ';' at the end of the tree", 21),
    ("A:1;", "expected '(' at the start of the tree", 0),
    ("(A:1,B:1,('C:1,D:1):1);", "a quoted name does not end", 10),
])
def test_parse_newick_refusals(text, message, offset):
    from andi_amd import lib
    names = ["A", "B", "C", "D"] if "D" in text or "missing name" in message else ["A", "B", "C"]
    if "E:1" in text:
        names = ["A", "B", "C", "D", "E"]
    with pytest.raises(lib.AndiHipError) as e:
        lib.parse_newick(text, names)
    assert str(e.value) == "andi_hip_parse_newick: byte %d: %s" % (offset, message) or \
        (message.startswith("missing name") and "byte %d: " % offset in str(e.value) and str(e.value).endswith(message))
    L = lib.load()
    J = np.zeros(8, lib.NJ_JOIN)
    err = C.create_string_buffer(64)
    cn = (C.c_char_p * 3)(b"A", b"B", b"C")
    assert L.andi_hip_parse_newick(None, cn, 3, 0, J.ctypes.data, err, 64) == 1 and b"bad arguments" in err.value
    assert L.andi_hip_parse_newick(b"(A:1,B:1);", cn, 2, 0, J.ctypes.data, None, 0) == 1


def test_parse_newick_is_not_recursive():
    from andi_amd import lib
    n = 65535
    names = ["s%d" % i for i in range(n)]
    J = pm.caterpillar(n, np.full(2 * n - 3, 0.25))
    t = lib.newick(J, names)
    assert lib.newick(lib.parse_newick(t, names), names) == lib.newick(lib.parse_newick(lib.newick(lib.parse_newick(t, names), names), names), names)


# ---------------------------------------------------------------- andi_hip_distances_rect
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_distances_rect_is_the_square_matrix_cells(model):
    from andi_amd import lib
    rng = np.random.default_rng(40 + model)
    nr, nq = 9, 5
    n = nr + nq
    M = np.zeros((n, n, 17), np.uint32)
    M[:, :, :16] = rng.integers(0, 40, (n, n, 16))
    for k in (0, 5, 10, 15):
        M[:, :, k] += rng.integers(2000, 4000, (n, n)).astype(np.uint32)
    M[:, :, 16] = 20000
    M[nr + 1, 2, :16] = 0  # a pair without homology: a NaN, the same bits from both
    M[2, nr + 1, :16] = 0
    M[nr + 3, 4, :16] = rng.integers(0, 3000, 16)  # saturated: whatever the estimator makes of it
    D = lib.distances(M, model)
    R = lib.distances_rect(M[:nr, nr:], M[nr:, :nr], model)
    assert R.shape == (nq, nr)
    assert (R.view(np.uint64) == D[nr:, :nr].view(np.uint64)).all()
    assert np.isnan(R[1, 2]) and np.isfinite(R[0]).all()
    assert lib.load().andi_hip_distances_rect(None, None, nr, nq, model, R.ctypes.data) == 1


# ---------------------------------------------------------------- andi_hip_format_jplace
def test_format_jplace():
    from andi_amd import lib
    rng = np.random.default_rng(77)
    n = 11
    refs = ["r%d" % i for i in range(n)]
    refs[3], refs[6] = 'quo"te', "back\\slash and blank"
    J = pm.random_tree(rng, n)
    D = np.stack([pm.point_distances(J, n, 4, 0.003, 0.01), np.full(n, np.nan), pm.point_distances(J, n, 15, 0.001, 0.0)])
    D[2] *= 1.0 + rng.uniform(-0.03, 0.03, n)
    queries = ['q "one" \\ end', "unplaced", "tab\there"]
    for method in ("fm", "ols"):
        P = pm.place(J, D, method)
        assert P["edge"][1] == -1 and P["edge"][0] == 4
        text = lib.jplace(J, refs, P, queries, method)
        doc = json.loads(text)
        assert doc["version"] == 3 and doc["metadata"]["method"] == method
        assert doc["fields"] == ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]
        tree = doc["tree"]
        assert sorted(int(k) for k in re.findall(r"\{(\d+)\}", tree)) == list(range(2 * n - 3))  # 0 ... 2n - 4, each once
        assert re.sub(r"\{\d+\}", "", tree) + "\n" == lib.newick(J, refs)  # the walk of format_newick
        # the number behind a leaf's length is the leaf's id: its edge
        for i, name in enumerate(refs):
            if not re.search(r"[ '\"\\]", name):
                assert re.search(r"[(,]%s:[^,(){]+\{%d\}" % (name, i), tree)
        got = doc["placements"]
        assert [g["n"] for g in got] == [[queries[0]], [queries[2]]]  # input order, the unplaced one left out; names round-trip
        for g, q in zip(got, (0, 2)):
            (edge, like, ratio, distal, pendant), = g["p"]
            assert (edge, ratio) == (int(P[q]["edge"]), 1)
            assert (like, distal, pendant) == (P[q]["err"], P[q]["distal"], P[q]["pendant"])  # %.17g: every bit
    # cap: the bytes needed come back whatever the room, the text is cut and NUL-terminated
    L = lib.load()
    rn, qn = lib._names(refs), lib._names(queries)
    need = L.andi_hip_format_jplace(J.ctypes.data, n, rn, 0, P.ctypes.data, 3, qn, 0, None, 0)
    assert need == len(text.encode())
    small = C.create_string_buffer(b"x" * 40, 40)
    assert L.andi_hip_format_jplace(J.ctypes.data, n, rn, 0, P.ctypes.data, 3, qn, 0, C.cast(small, C.c_void_p), 40) == need
    assert small.raw[:39] == text.encode()[:39] and small.raw[39:] == b"\0"
    # truncated names, as the table prints them
    cut = json.loads(lib.jplace(J, refs, P, queries, "ols", truncate_names=True))
    assert cut["placements"][0]["n"] == [queries[0][:10]] and "back\\slash:" in cut["tree"]
    # refused: malformed records, a method that is none
    bad = J.copy()
    bad[0]["a"] = 2 * n
    assert lib.jplace(bad, refs, P, queries) == ""
    assert L.andi_hip_format_jplace(J.ctypes.data, n, rn, 0, P.ctypes.data, 3, qn, 2, None, 0) == 0


def test_place_refuses_bad_arguments_before_any_hip_call():
    from andi_amd import lib
    L = lib.load()
    J = pm.random_tree(np.random.default_rng(1), 5)
    D = np.ones((1, 5))
    out = np.zeros(1, lib.PLACEMENT)
    assert L.andi_hip_place(None, J.ctypes.data, 5, D.ctypes.data, 1, 1, out.ctypes.data, None, None, None) == 1
