"""andi_hip_refine on the MI355X: records, result and log bit-exact to the NumPy restatement (tests/bme_model.py) -- on
perturbed random trees across the 64-lane boundary of the sums and the words of the leaf sets, on caterpillars and
balanced trees, a BIONJ tree, a parsed tree, odd matrices, weights past 2^-1022, max_moves = 0; two calls on one context;
the refined records under andi_hip_fit and andi_hip_root; its argument checks."""
import numpy as np
import pytest

import bme_model as bm
import nj_model
import place_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _check(ctx, J, D, what="", tol=1e-12, max_moves=None):
    """records, result and log, bit for bit; the library's for the caller"""
    from andi_amd import lib
    got = lib.refine(ctx, J, D, "bnni", tol=tol, max_moves=max_moves, log=True)
    want = bm.refine(J, D, tol=tol, max_moves=max_moves)
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes(), (what, got[2][:4], want[2][:4])
    assert got[0].tobytes() == want[0].tobytes(), what
    short = lib.refine(ctx, J, D, tol=tol, max_moves=max_moves)
    assert len(short) == 2 and short[0].tobytes() == got[0].tobytes() and short[1].tobytes() == got[1].tobytes()
    return got


def _noisy(n, seed, noise=0.2):
    return nj_model.additive_tree(n, seed, noise)[0]


@pytest.mark.parametrize("n", [4, 5, 8, 63, 64, 65, 129, 130])
def test_bit_exact_on_perturbed_random_trees(ctx, n):
    rng = np.random.default_rng(7000 + n)
    D = _noisy(n, 500 + n)
    J = bm.perturb(nj_model.nj(D), rng, n)
    got = _check(ctx, J, D, n)
    assert got[1]["converged"] == 1 and (n < 8 or got[1]["moves"] > 0)
    assert got[1]["length_after"] <= got[1]["length_before"]


@pytest.mark.parametrize("shape", ["caterpillar", "balanced"])
@pytest.mark.parametrize("n", [5, 65, 129])
def test_caterpillars_and_balanced_trees(ctx, shape, n):
    J = getattr(pm, shape)(n, np.full(2 * n - 3, 0.05))
    _check(ctx, J, _noisy(n, 600 + n), (shape, n))


def test_a_bionj_tree_and_a_parsed_tree(ctx):
    from andi_amd import lib
    n = 90
    D = _noisy(n, 81, 0.4)
    J = lib.tree(ctx, D, "bionj")
    _check(ctx, J, D, "bionj")
    names = ["t%d" % i for i in range(n)]
    rng = np.random.default_rng(82)
    text = lib.newick(bm.perturb(pm.random_tree(rng, n), rng, 5), names)
    _check(ctx, lib.parse_newick(text, names), D, "parsed")


def test_zeros_negative_entries_and_identical_leaves(ctx):
    rng = np.random.default_rng(91)
    n = 70
    D = _noisy(n, 91, 0.3)
    J = bm.perturb(nj_model.nj(D), rng, n)
    for _ in range(40):
        i, j = sorted(rng.choice(n, 2, replace=False).tolist())
        D[i, j] = D[j, i] = (0.0, -0.0, -0.05)[int(rng.integers(3))]
    D[7, :], D[:, 7] = D[3, :], D[:, 3]  # two identical leaves: the same row, and nothing between them
    D[3, 7] = D[7, 3] = 0.0
    D[np.arange(n), np.arange(n)] = 0.0
    D = np.triu(D, 1) + np.triu(D, 1).T
    _check(ctx, J, D, "odd")
    from andi_amd import lib
    lower = np.triu(D, 1) + np.tril(np.full((n, n), np.nan))  # the lower triangle and the diagonal are not read
    assert lib.refine(ctx, J, lower, tol=1e-12)[0].tobytes() == lib.refine(ctx, J, D, tol=1e-12)[0].tobytes()
    got = _check(ctx, J, np.zeros((n, n)), "zero", tol=0.0)
    assert got[1]["moves"] == 0 and got[1]["converged"] == 1
    same = _check(ctx, J, np.full((n, n), 0.25), "equal", tol=0.0)
    assert same[1]["moves"] == 0


def test_a_deep_caterpillar_whose_weights_pass_the_least_normal_number(ctx):
    n = 1100
    J = pm.caterpillar(n, np.full(2 * n - 3, 0.05))
    rng = np.random.default_rng(92)
    D = rng.uniform(0.5, 1.5, (n, n))
    D = np.triu(D, 1) + np.triu(D, 1).T
    got = _check(ctx, J, D, "deep", tol=0.0, max_moves=2)
    assert got[1]["moves"] == 2 and got[1]["converged"] == 0
    par, kid = bm.start(J)
    assert bm.bfs(par, kid, n)[1].max() > 1023  # (some weights are 0)


def test_two_calls_on_one_context_with_another_size_between(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(94)
    DA, DB = _noisy(70, 94), _noisy(11, 95)
    A, B = bm.perturb(nj_model.nj(DA), rng, 70), bm.perturb(nj_model.nj(DB), rng, 11)
    first = lib.refine(ctx, A, DA, tol=1e-12, log=True)
    _check(ctx, B, DB, "between")
    again = lib.refine(ctx, A, DA, tol=1e-12, log=True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert first[0].tobytes() == bm.refine(A, DA, tol=1e-12)[0].tobytes()


def test_no_move_allowed_gives_the_balanced_lengths_of_the_tree_given(ctx):
    rng = np.random.default_rng(96)
    n = 40
    D = _noisy(n, 96)
    J = bm.perturb(nj_model.nj(D), rng, n)
    got = _check(ctx, J, D, "none", tol=0.0, max_moves=0)
    assert got[1]["moves"] == 0 and got[1]["converged"] == 0 and got[1]["length_before"] == got[1]["length_after"]
    assert bm.inner_splits(got[0]) == bm.inner_splits(J)
    three = _check(ctx, pm.random_tree(rng, 3), _noisy(3, 97), "three")
    assert three[1]["moves"] == 0 and three[1]["converged"] == 1


def test_the_refined_records_go_through_fit_and_root(ctx):
    import fit_model as fm
    import root_model as rm
    from andi_amd import lib
    rng = np.random.default_rng(98)
    n = 73
    D = _noisy(n, 98)
    K, res = lib.refine(ctx, bm.perturb(nj_model.nj(D), rng, n), D, tol=1e-12)
    length, rec = lib.fit(ctx, K, D)
    assert length.tobytes() == fm.fit(K, D)[0].tobytes()
    assert rec["length_joined"] == pytest.approx(res["length_after"], rel=1e-12)
    got, want = lib.root(ctx, K, "mad"), rm.root(K, "mad")
    assert got["edge"] == want["edge"] and got["distal"] == want["distal"]
    reps = np.stack([K, K])
    assert (lib.nj_support(ctx, K, reps) == 2).all()


def test_bad_arguments_records_and_entries_leave_the_context_usable(ctx):
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(99)
    n = 20
    D = _noisy(n, 99)
    J = bm.perturb(nj_model.nj(D), rng, n)
    out, res, log = np.zeros(n - 2, lib.NJ_JOIN), np.zeros(1, lib.REFINE), np.zeros(10 * n, lib.REFINE_MOVE)

    def call(J=J, n=n, D=D, method=0, tol=0.0, out=out, res=res):
        p = lambda a: a.ctypes.data if a is not None else None
        return L.andi_hip_refine(ctx._h, p(J), n, p(D), method, tol, 10 * n, p(out), p(res), log.ctypes.data)

    for kw in (dict(J=None), dict(D=None), dict(out=None), dict(res=None), dict(n=2), dict(n=65536), dict(method=1), dict(method=-1),
               dict(tol=-1e-9), dict(tol=float("nan"))):
        assert call(**kw) == 1, kw
        assert b"andi_hip_refine: bad arguments" in L.andi_hip_last_error(ctx._h)
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    late = J.copy()
    late[2]["b"] = n + 7           # a child that no earlier record made
    for bad in (twice, late):
        assert call(J=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_refine: the tree's records are not those of andi_hip_nj"
    for value, text in ((np.nan, b"nan"), (np.inf, b"inf")):
        bad = D.copy()
        bad[11, 3] = value                     # (below the diagonal: not read)
        bad[5, 17] = bad[5, 9] = bad[8, 10] = value  # the first in row-major order is named
        assert call(D=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_refine: D[5][9] is not finite (" + text + b")"
    assert out.tobytes() == bytes(out.nbytes) and res.tobytes() == bytes(res.nbytes) and log.tobytes() == bytes(log.nbytes)
    assert call() == 0 and res[0]["converged"] == 1
    _check(ctx, J, D, "after")
