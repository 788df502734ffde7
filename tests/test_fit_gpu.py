"""andi_hip_fit on the MI355X: bit-exact to the NumPy restatement (tests/fit_model.py) on everything it returns -- the
lengths, the record, both per-leaf arrays --, across the tiles of k_fit (read from fit.hip), on caterpillars, balanced
trees, a BIONJ tree with negative lengths, odd matrices and sums that overflow, in forced small groups of leaves; two calls
on one context; its argument checks; and the relengthed records under andi_hip_root."""
import os
import re

import numpy as np
import pytest

import fit_model as fm
import place_model as pm
import root_model as rm
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "andi_amd", "csrc", "fit.hip")).read()
ET, BT, LT = (int(re.search(r"constexpr int %s = (\d+);" % k, _SRC).group(1)) for k in ("ET", "BT", "LT"))
INTS = ("pairs", "negative", "negative_joined", "worst_b", "worst_c")
REALS = ("rss", "rss_joined", "tss", "length", "length_joined", "worst")


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _same(g, w, what):
    """the same doubles: bit for bit, a NaN as a NaN"""
    g, w = np.atleast_1d(np.asarray(g, np.float64)), np.atleast_1d(np.asarray(w, np.float64))
    same = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
    bad = np.argwhere(~same)
    assert not len(bad), (what, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _check(ctx, J, D, what=""):
    """everything returned, bit for bit; the results for the caller"""
    from andi_amd import lib
    got, want = lib.fit(ctx, J, D, "ols", per=True), fm.fit(J, D, per=True)
    _same(got[0], want[0], (what, "len"))
    for f in INTS:
        assert got[1][f] == want[1][f], (what, f, got[1], want[1])
    for f in REALS:
        _same(got[1][f], want[1][f], (what, f))
    _same(got[2], want[2], (what, "leaf_ss"))
    _same(got[3], want[3], (what, "leaf_ss_joined"))
    short = lib.fit(ctx, J, D)
    assert len(short) == 2 and short[0].tobytes() == got[0].tobytes() and short[1].tobytes() == got[1].tobytes()
    return got


def _noisy(J, rng, noise=0.3):
    """the tree's own path lengths with multiplicative noise, symmetric"""
    n = len(J) + 2
    P = np.triu(rm.Table(J).P, 1)
    D = P * (1.0 + rng.uniform(-noise, noise, (n, n)))
    return D + D.T


def _sizes():
    edge_tile = sorted({(ET + 3 + d) // 2 for d in (-3, -1, 0, 1, 3)})  # 2n - 3 around ET, both sides of the boundary
    leaf_tile = [LT - 1, LT, LT + 1, LT + 2]
    two_tiles = [2 * LT - 1, 2 * LT, 2 * LT + 1]
    groups = [BT - 1 if BT > 3 else 3, BT, BT + 1, 2 * BT + 1]
    return sorted(set([3, 4, 5] + edge_tile + leaf_tile + two_tiles + groups))


@pytest.mark.parametrize("n", _sizes())
def test_bit_exact_on_random_trees(ctx, n):
    rng = np.random.default_rng(9000 + n)
    J = pm.random_tree(rng, n)
    _check(ctx, J, _noisy(J, rng), n)


@pytest.mark.parametrize("shape", ["caterpillar", "balanced"])
@pytest.mark.parametrize("n", [5, LT + 1, 2 * LT + 1])
def test_caterpillars_and_balanced_trees(ctx, shape, n):
    rng = np.random.default_rng(n + len(shape))
    J = getattr(pm, shape)(n, rng.uniform(0.01, 0.1, 2 * n - 3))
    _check(ctx, J, _noisy(J, rng), (shape, n))


def test_a_bionj_tree_of_a_noisy_matrix_with_negative_lengths(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(81)  # (test_root_gpu.py's matrix: the same construction and seed)
    n = 90
    J0 = pm.random_tree(rng, n)
    t = rm.Table(J0)
    D = np.triu(t.P, 1)
    D = (D + D.T) * (1.0 + rng.uniform(-0.4, 0.4, (n, n)))
    D = np.triu(D, 1) + np.triu(D, 1).T
    J = lib.tree(ctx, D, "bionj")
    lens = np.concatenate([J["la"], J["lb"], J["lc"][-1:]])
    assert (lens < 0).any()
    got = _check(ctx, J, D, "bionj")
    assert got[1]["negative_joined"] == (lens < 0).sum() and got[1]["rss"] <= got[1]["rss_joined"]


def test_zeros_negative_entries_and_identical_leaves(ctx):
    rng = np.random.default_rng(91)
    n = LT + 6
    J = pm.random_tree(rng, n)
    D = _noisy(J, rng)
    for _ in range(40):
        i, j = sorted(rng.choice(n, 2, replace=False).tolist())
        D[i, j] = D[j, i] = (0.0, -0.0, -0.05)[int(rng.integers(3))]
    a, b = int(J[0]["a"]), int(J[0]["b"])  # two identical leaves: the same row, and nothing between them
    D[b, :] = D[a, :]
    D[:, b] = D[:, a]
    D[a, b] = D[b, a] = 0.0
    D[np.arange(n), np.arange(n)] = 0.0
    D = np.triu(D, 1) + np.triu(D, 1).T
    _check(ctx, J, D, "odd")
    lower = np.triu(D, 1) + np.tril(np.full((n, n), np.nan))  # the lower triangle and the diagonal are not read
    from andi_amd import lib
    assert lib.fit(ctx, J, lower)[0].tobytes() == lib.fit(ctx, J, D)[0].tobytes()
    _check(ctx, J, np.zeros((n, n)), "zero")


def test_sums_that_overflow_give_the_models_inf_and_nan(ctx):
    rng = np.random.default_rng(92)
    n = LT + 3
    J = pm.random_tree(rng, n)
    D = _noisy(J, rng)
    D *= 1e307 / D.max()
    with np.errstate(all="ignore"):
        got = _check(ctx, J, D, "huge")
        _check(ctx, J, D * 0.5, "half as huge")  # (fewer of the sums overflow)
    assert not np.isfinite(got[0]).all()
    tiny = pm.random_tree(rng, 5)
    with np.errstate(all="ignore"):
        _check(ctx, tiny, np.full((5, 5), 1.7e308), "every residual")


def test_small_groups_of_leaves_give_the_same_bytes(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(93)
    n = 3 * LT + 9
    J = pm.random_tree(rng, n)
    D = _noisy(J, rng)
    whole = _check(ctx, J, D, "whole")
    for g in (1, BT + 1, LT + 3):
        with knobs(FIT_GROUP=g):
            parts = lib.fit(ctx, J, D, per=True)
        for a, b in zip(whole, parts):
            assert a.tobytes() == b.tobytes(), g


def test_two_calls_on_one_context_with_another_size_between(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(94)
    A, B = pm.random_tree(rng, 70), pm.random_tree(rng, 11)
    DA, DB = _noisy(A, rng), _noisy(B, rng)
    first = lib.fit(ctx, A, DA, per=True)
    _check(ctx, B, DB, "between")
    again = lib.fit(ctx, A, DA, per=True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    _same(first[0], fm.fit(A, DA)[0], "first")


def test_bad_arguments_records_and_entries_leave_the_context_usable(ctx):
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(95)
    n = 20
    J = pm.random_tree(rng, n)
    D = _noisy(J, rng)
    out = np.zeros(1, lib.FIT)
    length, ss, ssj = np.full(2 * n - 3, 7.0), np.full(n, 7.0), np.full(n, 7.0)

    def call(J=J, n=n, D=D, method=0, length=length, out=out):
        p = lambda a: a.ctypes.data if a is not None else None
        return L.andi_hip_fit(ctx._h, p(J), n, p(D), method, p(length), p(out), ss.ctypes.data, ssj.ctypes.data)

    for kw in (dict(J=None), dict(D=None), dict(length=None), dict(out=None), dict(n=2), dict(n=65536), dict(method=1), dict(method=-1)):
        assert call(**kw) == 1, kw
        assert b"andi_hip_fit: bad arguments" in L.andi_hip_last_error(ctx._h)
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    late = J.copy()
    late[2]["b"] = n + 7           # a child that no earlier record made
    for bad in (twice, late):
        assert call(J=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_fit: the tree's records are not those of andi_hip_nj"
    for value in (np.nan, np.inf, -np.inf):
        bad = J.copy()
        bad[7]["lb"] = value
        assert call(J=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_fit: a branch length of the tree's record 7 is not finite"
    for value, text in ((np.nan, b"nan"), (np.inf, b"inf")):
        bad = D.copy()
        bad[11, 3] = value                     # (below the diagonal: not read)
        bad[5, 17] = bad[5, 9] = bad[8, 2 + 8] = value  # the first in row-major order is named
        assert call(D=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_fit: D[5][9] is not finite (" + text + b")"
    assert out.tobytes() == bytes(out.nbytes) and (length == 7.0).all() and (ss == 7.0).all() and (ssj == 7.0).all()  # nothing written
    assert call() == 0 and not (length == 7.0).any() and not (ss == 7.0).any()
    _check(ctx, J, D, "after")


def test_the_relengthed_records_go_through_root(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(96)
    n = LT + 9
    J = pm.random_tree(rng, n)
    D = _noisy(J, rng)
    length, _ = lib.fit(ctx, J, D)
    K = lib.relength(J, length)
    assert K.tobytes() == fm.relength(J, length).tobytes()
    got, want = lib.root(ctx, K, "mad", per=True), rm.root(K, "mad", per=True)
    for f in ("edge", "pairs", "far_b", "far_c"):
        assert got[0][f] == want[0][f], f
    for f in ("distal", "ss", "ss_second"):
        _same(got[0][f], want[0][f], f)
    _same(got[1], want[1], "x")
    _same(got[2], want[2], "ss")
