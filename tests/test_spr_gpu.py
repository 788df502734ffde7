"""andi_hip_refine_spr on the MI355X: records, result and log bit-exact to the NumPy restatement (tests/spr_model.py) --
on the smallest trees (n = 6 has the first move of two hops), across the 64-lane boundary of the tables' columns and the
words of the leaf sets, on a caterpillar (one node a level: the deepest stacks) and a balanced tree, on a search that
deepens its tree sixfold (the stacks grow between rounds), on trees whose
winning move is made at the centre, across it, and on the side that holds it; max_moves = 0, a cap and a tolerance that
end the search, out aliasing tree, a bad matrix; the refined records under andi_hip_fit and andi_hip_root."""
import numpy as np
import pytest

import bme_model as bm
import nj_model
import place_model as pm
import spr_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _check(ctx, J, D, what="", tol=1e-12, max_moves=None, trace=None):
    """records, result and log, bit for bit; the library's for the caller"""
    from andi_amd import lib
    got = lib.refine_spr(ctx, J, D, tol=tol, max_moves=max_moves, log=True)
    want = sm.refine_spr(J, D, tol=tol, max_moves=max_moves, trace=trace)
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes(), (what, got[2][:4], want[2][:4])
    assert got[0].tobytes() == want[0].tobytes(), what
    short = lib.refine_spr(ctx, J, D, tol=tol, max_moves=max_moves)
    assert len(short) == 2 and short[0].tobytes() == got[0].tobytes() and short[1].tobytes() == got[1].tobytes()
    return got


def _noisy(n, seed, noise=0.2):
    return nj_model.additive_tree(n, seed, noise)[0]


@pytest.mark.parametrize("n", [3, 4, 5, 6, 63, 64, 65])
def test_bit_exact_on_perturbed_random_trees(ctx, n):
    rng = np.random.default_rng(7000 + n)
    D = _noisy(n, 500 + n)
    J = bm.perturb(nj_model.nj(D), rng, n)
    got = _check(ctx, J, D, n)
    assert got[1]["converged"] == 1 and (n < 63 or got[1]["moves"] > 0)
    assert got[1]["length_after"] <= got[1]["length_before"]
    assert n < 63 or got[2]["hops"].max() > 1  # (moves no interchange makes)


def test_six_leaves_make_a_move_of_two_hops(ctx):
    n = 6
    J = pm.caterpillar(n, np.full(2 * n - 3, 0.05))
    D = nj_model.additive_tree(n, 3)[0]
    hops = set()
    for seed in range(12):  # the leaves renamed: one of the starts is two hops from the tree of D
        perm = np.random.default_rng(seed).permutation(n)
        got = _check(ctx, J, D[np.ix_(perm, perm)], ("six", seed))
        hops |= set(got[2]["hops"].tolist())
    assert 2 in hops


def test_129_leaves_ten_moves(ctx):
    n = 129
    rng = np.random.default_rng(7129)
    D = _noisy(n, 629)
    got = _check(ctx, bm.perturb(nj_model.nj(D), rng, n), D, n, max_moves=10)
    assert got[1]["moves"] == 10 and got[1]["converged"] == 0


@pytest.mark.parametrize("shape, n, moves", [("caterpillar", 200, 4), ("balanced", 128, 6)])
def test_a_caterpillar_and_a_balanced_tree(ctx, shape, n, moves):
    J = getattr(pm, shape)(n, np.full(2 * n - 3, 0.05))
    got = _check(ctx, J, _noisy(n, 600 + n), (shape, n), max_moves=moves)
    assert got[1]["moves"] == moves


def test_a_search_that_deepens_the_tree_grows_the_stacks(ctx):
    """a balanced tree on a caterpillar's distances: move by move the tree gets deeper, from 5 edges to 31, so the stacks
    sized for the first tree are too short for the later ones and the call has to grow them between rounds"""
    n = 48
    i = np.arange(n)
    D = 2.0 + np.abs(i[:, None] - i[None, :])
    D = D * (1 + 0.05 * np.triu(np.random.default_rng(1).uniform(-1, 1, (n, n)), 1))
    D = np.triu(D, 1) + np.triu(D, 1).T
    J = pm.balanced(n, np.full(2 * n - 3, 0.05))
    trace = []
    got = _check(ctx, J, D, "deepens", tol=1e-9, trace=trace)
    depths = [sm.depth_of(m[6], n) for m in trace] + [sm.depth_of(bm.start(got[0])[0], n)]
    assert depths[0] == 5 and max(depths) > 4 * depths[0] and got[1]["converged"] == 1
    assert len({d for d in depths}) > 8  # (the depth rises in many steps: more than one growth)


@pytest.mark.parametrize("kind, seed", [("across", 0), ("holds", 3), ("at", 20)])
def test_the_winning_move_meets_the_centre(ctx, kind, seed):
    """a first move of two hops or more that is made at C, crosses C, or prunes the side holding C: the rooted tree's edges
    on the path turn round, and the search goes on from the tree it leaves"""
    n = 14
    rng = np.random.default_rng(seed)
    D = _noisy(n, seed)
    J = bm.perturb(nj_model.nj(D), rng, n)
    trace = []
    _check(ctx, J, D, kind, trace=trace)
    assert sm.kind_of(trace[0], n) == kind and trace[0][5] >= 2 and len(trace) > 1


def test_zeros_negative_entries_and_equal_distances(ctx):
    rng = np.random.default_rng(91)
    n = 70
    D = _noisy(n, 91, 0.3)
    J = bm.perturb(nj_model.nj(D), rng, n)
    for _ in range(40):
        i, j = sorted(rng.choice(n, 2, replace=False).tolist())
        D[i, j] = D[j, i] = (0.0, -0.0, -0.05)[int(rng.integers(3))]
    _check(ctx, J, D, "odd", max_moves=12)
    got = _check(ctx, J, np.zeros((n, n)), "zero", tol=0.0)
    assert got[1]["moves"] == 0 and got[1]["converged"] == 1
    assert _check(ctx, J, np.full((n, n), 0.25), "equal", tol=0.0)[1]["moves"] == 0


def test_no_move_allowed_a_cap_and_a_tolerance_end_the_search(ctx):
    rng = np.random.default_rng(96)
    n = 40
    D = _noisy(n, 96)
    J = bm.perturb(nj_model.nj(D), rng, n)
    got = _check(ctx, J, D, "none", tol=0.0, max_moves=0)
    assert got[1]["moves"] == 0 and got[1]["converged"] == 0 and got[1]["length_before"] == got[1]["length_after"]
    assert bm.inner_splits(got[0]) == bm.inner_splits(J)
    full = _check(ctx, J, D, "full")
    assert full[1]["moves"] >= 4 and full[1]["converged"] == 1
    capped = _check(ctx, J, D, "capped", max_moves=3)
    assert capped[1]["moves"] == 3 and capped[1]["converged"] == 0
    assert capped[2].tobytes() == full[2][:3].tobytes()
    gains = full[2]["gain"]
    at = int(np.argmin(gains))  # a tolerance the least gain does not pass: the search stops in front of that move
    stopped = _check(ctx, J, D, "tol", tol=float(gains[at]))
    assert stopped[1]["moves"] == at and stopped[1]["converged"] == 1


def test_out_may_be_the_tree_and_a_bad_matrix_writes_nothing(ctx):
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(99)
    n = 20
    D = _noisy(n, 99)
    J = bm.perturb(nj_model.nj(D), rng, n)
    want = sm.refine_spr(J, D, tol=1e-12)
    out, res, log = np.zeros(n - 2, lib.NJ_JOIN), np.zeros(1, lib.REFINE), np.zeros(10 * n, lib.SPR_MOVE)

    def call(J=J, n=n, D=D, tol=1e-12, out=out, res=res):
        p = lambda a: a.ctypes.data if a is not None else None
        return L.andi_hip_refine_spr(ctx._h, p(J), n, p(D), tol, 10 * n, p(out), p(res), log.ctypes.data)

    for kw in (dict(J=None), dict(D=None), dict(out=None), dict(res=None), dict(n=2), dict(n=65536), dict(tol=-1e-9),
               dict(tol=float("nan"))):
        assert call(**kw) == 1, kw
        assert b"andi_hip_refine_spr: bad arguments" in L.andi_hip_last_error(ctx._h)
    late = J.copy()
    late[2]["b"] = n + 7  # a child that no earlier record made
    assert call(J=late) == 1
    assert L.andi_hip_last_error(ctx._h) == b"andi_hip_refine_spr: the tree's records are not those of andi_hip_nj"
    for value, text in ((np.nan, b"nan"), (np.inf, b"inf")):
        bad = D.copy()
        bad[11, 3] = value                           # (below the diagonal: not read)
        bad[5, 17] = bad[5, 9] = bad[8, 10] = value  # the first in row-major order is named
        assert call(D=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_refine_spr: D[5][9] is not finite (" + text + b")"
    assert out.tobytes() == bytes(out.nbytes) and res.tobytes() == bytes(res.nbytes) and log.tobytes() == bytes(log.nbytes)
    same = J.copy()
    assert call(out=same, J=same) == 0
    assert same.tobytes() == want[0].tobytes() and res[0].tobytes() == want[1].tobytes()
    assert log[:len(want[2])].tobytes() == want[2].tobytes() and log[len(want[2]):].tobytes() == bytes(log[len(want[2]):].nbytes)


def test_the_refined_records_go_through_fit_and_root(ctx):
    import fit_model as fm
    import root_model as rm
    from andi_amd import lib
    rng = np.random.default_rng(98)
    n = 73
    D = _noisy(n, 98)
    K, res = lib.refine_spr(ctx, bm.perturb(nj_model.nj(D), rng, n), D, tol=1e-12)
    assert res["converged"] == 1
    length, rec = lib.fit(ctx, K, D)
    assert length.tobytes() == fm.fit(K, D)[0].tobytes()
    assert rec["length_joined"] == pytest.approx(res["length_after"], rel=1e-12)
    got, want = lib.root(ctx, K, "mad"), rm.root(K, "mad")
    assert got["edge"] == want["edge"] and got["distal"] == want["distal"]
    assert (lib.nj_support(ctx, K, np.stack([K, K])) == 2).all()
    # no interchange is left either: the search by interchanges makes no move from the result
    assert lib.refine(ctx, K, D, tol=1e-12)[1]["moves"] == 0
