"""andi_hip_root on the MI355X: bit-exact to the NumPy restatement (tests/root_model.py) on everything it returns -- the
record, x and SS of every edge --, for both methods, across the tiles of k_root (read from root.hip), on caterpillars,
balanced trees, a BIONJ tree with negative lengths and identical leaves, in forced small groups of leaves; two calls on one
context; its argument checks."""
import os
import re

import numpy as np
import pytest

import place_model as pm
import root_model as rm
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "andi_amd", "csrc", "root.hip")).read()
ET, BT, LT = (int(re.search(r"constexpr int %s = (\d+);" % k, _SRC).group(1)) for k in ("ET", "BT", "LT"))
METHODS = ("mad", "midpoint")


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_record(g, w, what):
    for f in ("edge", "pad", "pairs", "far_b", "far_c"):
        assert g[f] == w[f], (what, f, g, w)
    for f in ("distal", "ss", "ss_second"):
        assert _bits(g[f]) == _bits(w[f]), (what, f, g, w)


def _check(ctx, J, what=""):
    """both methods, everything returned, bit for bit; the MAD results for the caller"""
    from andi_amd import lib
    got, want = lib.root(ctx, J, "mad", per=True), rm.root(J, "mad", per=True)
    _same_record(got[0], want[0], what)
    for g, w, f in zip(got[1:], want[1:], ("x", "ss")):
        bad = np.argwhere(_bits(g) != _bits(w))
        assert not len(bad), (what, f, bad[:4].tolist(), g[bad[0][0]], w[bad[0][0]])
    _same_record(lib.root(ctx, J, "midpoint"), rm.root(J, "midpoint"), what)
    return got


def _sizes():
    edge_tile = sorted({(ET + 3 + d) // 2 for d in (-3, -1, 0, 1, 3)})  # 2n - 3 around ET, both sides of the boundary
    leaf_tile = [LT - 1, LT, LT + 1, LT + 2]
    two_tiles = [2 * LT - 1, 2 * LT, 2 * LT + 1]
    groups = [BT - 1 if BT > 3 else 3, BT, BT + 1, 2 * BT + 1]
    return sorted(set([3, 4, 5] + edge_tile + leaf_tile + two_tiles + groups))


@pytest.mark.parametrize("n", _sizes())
def test_bit_exact_on_random_trees(ctx, n):
    rng = np.random.default_rng(7000 + n)
    _check(ctx, pm.random_tree(rng, n), n)


@pytest.mark.parametrize("shape", ["caterpillar", "balanced"])
@pytest.mark.parametrize("n", [5, LT + 1, 2 * LT + 1])
def test_caterpillars_and_balanced_trees(ctx, shape, n):
    rng = np.random.default_rng(n + len(shape))
    _check(ctx, getattr(pm, shape)(n, rng.uniform(0.01, 0.1, 2 * n - 3)), (shape, n))


def test_a_bionj_tree_of_a_noisy_matrix_with_negative_lengths(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(81)
    n = 90
    J0 = pm.random_tree(rng, n)
    t = rm.Table(J0)
    D = np.triu(t.P, 1)
    D = (D + D.T) * (1.0 + rng.uniform(-0.4, 0.4, (n, n)))
    D = np.triu(D, 1) + np.triu(D, 1).T
    J = lib.tree(ctx, D, "bionj")
    lens = np.concatenate([J["la"], J["lb"], J["lc"][-1:]])
    assert (lens < 0).any()
    _check(ctx, J, "bionj")


def test_identical_leaves_zero_and_negative_edges(ctx):
    rng = np.random.default_rng(82)
    n = LT + 6
    lengths = rng.uniform(0.01, 0.1, 2 * n - 3)
    lengths[rng.choice(2 * n - 3, 12, replace=False)] = 0.0
    lengths[rng.choice(2 * n - 3, 6, replace=False)] = -0.03
    it = iter(lengths)
    J = pm.random_tree(rng, n, lambda k: [next(it) for _ in range(k)])
    J[0]["la"], J[0]["lb"] = 0.0, 0.0  # two identical leaves: p == 0
    got = _check(ctx, J, "odd")
    assert got[0]["pairs"] < n * (n - 1) // 2
    # every pair unusable
    Z = pm.random_tree(rng, 9, lambda k: np.zeros(k))
    got = _check(ctx, Z, "zero")
    assert (got[0]["edge"], got[0]["pairs"], got[0]["far_b"]) == (0, 0, -1) and not got[2].any()


def test_small_groups_of_leaves_give_the_same_bytes(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(83)
    n = 3 * LT + 9
    J = pm.random_tree(rng, n)
    whole = _check(ctx, J, "whole")
    for g in (1, BT + 1, LT + 3):
        with knobs(ROOT_GROUP=g):
            parts = lib.root(ctx, J, "mad", per=True)
        for a, b in zip(whole, parts):
            assert a.tobytes() == b.tobytes(), g


def test_two_calls_on_one_context_with_another_size_between(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(84)
    A, B = pm.random_tree(rng, 70), pm.random_tree(rng, 11)
    first = lib.root(ctx, A, "mad", per=True)
    _check(ctx, B, "between")
    again = lib.root(ctx, A, "mad", per=True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    _same_record(first[0], rm.root(A, "mad"), "first")


def test_bad_arguments_and_records_leave_the_context_usable(ctx):
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(85)
    n = 20
    J = pm.random_tree(rng, n)
    out = np.zeros(1, lib.ROOT)
    px, pss = np.full(2 * n - 3, 7.0), np.full(2 * n - 3, 7.0)

    def call(J=J, n=n, method=0, out=out):
        return L.andi_hip_root(ctx._h, J.ctypes.data if J is not None else None, n, method,
                               out.ctypes.data if out is not None else None, px.ctypes.data, pss.ctypes.data)

    for kw in (dict(J=None), dict(out=None), dict(n=2), dict(n=65536), dict(method=2), dict(method=-1)):
        assert call(**kw) == 1, kw
        assert b"bad arguments" in L.andi_hip_last_error(ctx._h)
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    late = J.copy()
    late[2]["b"] = n + 7           # a child that no earlier record made
    for bad in (twice, late):
        assert call(J=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_root: the tree's records are not those of andi_hip_nj"
    for value in (np.nan, np.inf, -np.inf):
        bad = J.copy()
        bad[7]["lb"] = value
        assert call(J=bad) == 1 and b"record 7 is not finite" in L.andi_hip_last_error(ctx._h)
    assert out.tobytes() == bytes(out.nbytes) and (px == 7.0).all() and (pss == 7.0).all()  # nothing written
    assert call(method=1) == 0 and (px == 7.0).all() and (pss == 7.0).all()  # midpoint leaves the per-edge arrays alone
    _same_record(out[0], rm.root(J, "midpoint"), "midpoint")
    assert call() == 0
    _check(ctx, J, "after")
