"""Refining a tree by balanced subtree pruning and regrafting without a GPU: the NumPy restatement (tests/spr_model.py)
against its own depth-first walk over plain loops, bit for bit; every candidate's gain against the difference of
Pauplin's length by brute force, the moves at the centre, across it and on its side among them; the one-hop candidates
against the interchanges' gains; no move from the tree of an additive matrix; the search recovering the generating tree
from starts n random SPRs away; the new symbol, its argument checks; --help and the usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bme_model as bm
import nj_model
import place_model as pm
import spr_model as sm
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
U = 2.0 ** -53


def _bound(n, D):
    """64 * 2^-53 * n * max D, the bound tests/test_refine_host.py derives for a gain of interchanges against the brute-
    force lengths, with u = 2^-53 and M = max |D|.  It holds here too: an entry of B is an average of distances reached
    through at most 2n - 4 averagings of one rounded addition each (n - 2 for the A it starts from, n - 2 more for the
    second side), so it is within 2 n u M of the exact balanced average.  A gain is a combination of at most six entries
    and R, whose weights add up to less than 3 in absolute value (1/2 + 1/2 + 1/2 + 1/2 + 1/4 R, R < 2M), so it inherits
    less than 6 n u M from them; its own dozen rounded operations on values below 2M add 24 u M, R's k <= n additions of
    halved values 2 n u M; the two brute-force lengths add 2 n u M.  Together below (10 n + 24) u M < 64 n u M."""
    return 64 * U * n * np.abs(D).max()


def _noisy(n, seed, noise=0.3):
    return nj_model.additive_tree(n, seed, noise)[0]


def _splits_of(J, names):
    leaves, splits, _ = nj_model.parse_newick(nj_model.newick(J, names))
    assert sorted(leaves) == sorted(names)
    return nj_model.unrooted_splits(splits, names)


def _round(J, D):
    """(par, kid, order, A, B) of the first round"""
    n = len(J) + 2
    par, kid = sm.orient(sm.slots_of(J), n)
    order, lev = bm.bfs(par, kid, n)
    A = bm.table(bm.mirrored(D), par, kid, n, order, bm.leaf_sets(kid, n, order))
    return par, kid, order, A, sm.pairs(A, par, kid, n, order, sm.ancestors(par, n, order))


def _random_sprs(J, rng, count):
    """the records after `count` random SPRs: a random pruned side, a random target edge of its candidates"""
    n = len(J) + 2
    for _ in range(count):
        par, kid, order, _, _ = _round(J, np.zeros((n, n)))
        _, ok, K = sm.candidates(np.zeros((2 * n - 3, 2 * n - 3)), par, kid, n, order)
        s, f = np.argwhere(ok)[int(rng.integers(ok.sum()))]
        J = sm.rehung(J, *sm.move_of(par, kid, n, K, int(s), int(f))[:5])
    return J


# ---------------------------------------------------------------- the surface
def test_declared_exported_and_abi_stays_5():
    from andi_amd import lib
    import andi_amd
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    shipped = C.CDLL(os.path.join(ROOT, "andi_amd", "libandihip.so"))
    assert re.search(r"\bandi_hip_refine_spr\s*\(", header) and "andi_hip_refine_spr" in lib.SYMBOLS
    assert getattr(L, "andi_hip_refine_spr") is not None and getattr(shipped, "andi_hip_refine_spr") is not None
    assert L.andi_hip_abi_version() == 5 and "#define ANDI_HIP_ABI_VERSION 5" in header  # additions only
    assert "} andi_hip_spr_move; /* 24 bytes */" in header
    assert lib.SPR_MOVE.itemsize == 24 and lib.SPR_MOVE == sm.SPR_MOVE
    assert andi_amd.refine_spr is lib.refine_spr and andi_amd.SPR_MOVE is lib.SPR_MOVE
    assert lib.REFINE_METHODS == ("bnni",)  # (the old names take no new value)


# ---------------------------------------------------------------- 1: the model's two forms
@pytest.mark.parametrize("n", range(3, 15))
def test_the_vectorised_model_is_the_walk_bit_for_bit(n):
    rng = np.random.default_rng(1000 + n)
    D = _noisy(n, 50 + n)
    if n == 7:
        D[1, 4] = D[4, 1] = 0.0
        D[2, 3] = D[3, 2] = -0.02
    J = bm.perturb(pm.random_tree(rng, n), rng, n)
    for kw in (dict(), dict(tol=1e-3, max_moves=2)):
        a, b = sm.refine_spr(J, D, **kw), sm.refine_spr_loops(J, D, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (n, kw)
    par, kid, order, A, B = _round(J, D)
    assert B.tobytes() == sm.pairs_loops(A, par, kid, n).tobytes()
    G, ok, K = sm.candidates(B, par, kid, n, order)
    walk = sm.candidates_loops(B, par, kid, n)
    assert ok.sum() == len(walk) and [(2 * c[1] + c[2], c[3]) for c in walk] == [tuple(at) for at in np.argwhere(ok)]
    for c in walk:
        s = 2 * c[1] + c[2]
        assert G[s, c[3]].tobytes() == np.float64(c[0]).tobytes() and sm.move_of(par, kid, n, K, s, c[3]) == c[4:]


# ---------------------------------------------------------------- 2: every gain is Pauplin's
@pytest.mark.parametrize("n", range(5, 18))
def test_every_gain_is_the_difference_of_pauplins_length(n):
    rng = np.random.default_rng(2000 + n)
    D = _noisy(n, 70 + n)
    J = pm.random_tree(rng, n)
    bound = _bound(n, D)
    par, kid, order, _, B = _round(J, D)
    G, ok, K = sm.candidates(B, par, kid, n, order)
    here = bm.pauplin_length(J, D)
    worst, kinds, most = 0.0, set(), 0
    assert ok.sum() == _candidates(par, kid, n)
    for s, f in np.argwhere(ok):
        mv = sm.move_of(par, kid, n, K, int(s), int(f))
        moved = sm.rehung(J, *mv[:5])
        dev = abs(G[s, f] - (here - bm.pauplin_length(moved, D)))
        worst, most = max(worst, dev), max(most, mv[5])
        kinds.add(sm.kind_of(mv + (par,), n))
        assert dev <= bound, (n, mv, dev, bound)
        if mv[5] > 1:  # (no interchange: the tree's branches change)
            assert bm.inner_splits(moved) != bm.inner_splits(J)
    print("n = %d: %d candidates, up to %d hops, worst deviation %.3g, bound %.3g" % (n, ok.sum(), most, worst, bound))
    assert kinds == {"", "at", "across", "holds"} and most >= 2  # both prune directions, v0 = C, paths through C


def _candidates(par, kid, n):
    """every edge beyond v0 but its own two: all but the edges of X, the pruned edge and those two"""
    E = 2 * n - 3
    size = 2 * bm.leaf_sets(kid, n, bm.bfs(par, kid, n)[0]).sum(1) - 2  # the edges below node u
    return int(sum(E - 3 - size[u] for u in range(E)) + sum(size[u] - 2 for u in range(n, E)))


# ---------------------------------------------------------------- 3: one hop is an interchange
@pytest.mark.parametrize("n", [4, 5, 9, 17])
def test_the_one_hop_candidates_are_the_interchanges(n):
    rng = np.random.default_rng(3000 + n)
    D = _noisy(n, 80 + n)
    J = pm.random_tree(rng, n)
    par, kid, order, _, B = _round(J, D)
    G, ok, K = sm.candidates(B, par, kid, n, order)
    T, R, _ = bm.evaluate(bm.mirrored(D), par, kid, n)
    g = bm.gains(T, R, par, kid, n)
    bound, seen, worst = _bound(n, D), 0, 0.0
    for s, f in np.argwhere(ok):
        x, v0, q, vk, w, k = sm.move_of(par, kid, n, K, int(s), int(f))
        if k != 1:
            continue
        # the interchange across the edge (v0, q): x changes places with the neighbour of q that is not w
        moved = bm.inner_splits(sm.rehung(J, x, v0, q, vk, w))
        v = sm.edge_of(par, n, v0, q)
        same = []
        for alt in (0, 1):
            p2, k2 = par.copy(), kid.copy()
            bm.apply_move(p2, k2, n, v, alt)
            if bm.inner_splits(bm.canonical(p2, k2, np.zeros(2 * n - 3), n)) == moved:
                same.append(alt)
        assert len(same) == 1, (n, s, f)
        worst = max(worst, abs(G[s, f] - g[v - n, same[0]]))
        seen += 1
    print("n = %d: %d one-hop candidates, worst deviation %.3g, bound %.3g" % (n, seen, worst, bound))
    assert seen == 8 * (n - 3) and worst <= bound  # (each interchange is four SPRs; two interchanges an inner edge)


# ---------------------------------------------------------------- 4: an additive matrix
@pytest.mark.parametrize("n", [3, 4, 5, 9, 17, 40])
def test_on_an_additive_matrix_its_tree_is_left_alone(n):
    D, splits, names = nj_model.additive_tree(n, 300 + n)
    J = nj_model.nj(D)
    out, res, log = sm.refine_spr(J, D, tol=_bound(n, D))
    assert res["moves"] == 0 and res["converged"] == 1 and len(log) == 0
    assert _splits_of(out, names) == _splits_of(J, names) == splits
    assert res["length_before"] == res["length_after"]
    assert out.tobytes() == bm.refine(J, D, tol=_bound(n, D))[0].tobytes()  # (the same lengths, the same numbering)


# ---------------------------------------------------------------- 5: recovery
@pytest.mark.parametrize("seed", range(100, 103))
@pytest.mark.parametrize("n", [8, 33, 65])
def test_the_search_recovers_the_generating_tree(n, seed):
    """By Bordewich et al. (2009) any tree but the generating one has an improving interchange on an additive matrix, and
    the interchanges are among the candidates; tol lies far below the least inner branch's gain and far above the noise."""
    D, splits, names = nj_model.additive_tree(n, seed)
    rng = np.random.default_rng(seed)
    J = _random_sprs(nj_model.nj(D), rng, n)
    before = bm.pauplin_length(J, D)
    out, res, log = sm.refine_spr(J, D, tol=2.0 ** -32 * before)
    away = len(splits - _splits_of(J, names))
    print("n = %d seed %d: %d splits away, %d moves, up to %d hops" % (n, seed, away, res["moves"], log["hops"].max() if len(log) else 0))
    assert res["converged"] == 1 and res["moves"] <= away + n
    assert _splits_of(out, names) == splits


# ---------------------------------------------------------------- the argument checks
def test_bad_arguments_are_refused_before_any_hip_call():
    from andi_amd import lib
    L = lib.load()
    n = 5
    J = pm.random_tree(np.random.default_rng(1), n)
    D = np.ones((n, n))
    out, res = np.zeros(n - 2, lib.NJ_JOIN), np.zeros(1, lib.REFINE)
    j, d, o, r = J.ctypes.data, D.ctypes.data, out.ctypes.data, res.ctypes.data
    # with no context nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, j, n, d, 0.0, 10, o, r, None), (None, None, n, d, 0.0, 10, o, r, None),
                 (None, j, 2, d, 0.0, 10, o, r, None), (None, j, 65536, d, 0.0, 10, o, r, None),
                 (None, j, n, d, -1.0, 10, o, r, None), (None, j, n, d, float("nan"), 10, o, r, None)]:
        assert L.andi_hip_refine_spr(*args) == 1, args
    assert out.tobytes() == bytes(out.nbytes) and res.tobytes() == bytes(res.nbytes)
    with pytest.raises(ValueError):
        lib.refine_spr(None, J, D[:-1])
    with pytest.raises(ValueError):
        lib.refine_spr(None, J, D, max_moves=-1)


# ---------------------------------------------------------------- the command line, as far as it goes without a GPU
def _cli(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=60, stdin=subprocess.DEVNULL)


def test_help_names_the_option_and_usage_errors():
    p = _cli(["--help"])
    assert p.returncode == 0
    text = p.stdout.decode()
    assert "--refine-moves=MOVES" in text and "'nni'" in text and "'spr'" in text
    p = _cli(["--refine=bnni", "--refine-moves=bogus", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "Expected one of 'nni' or 'spr' for --refine-moves, but 'bogus' was given." in p.stderr.decode()
    for args in (["--refine-moves=spr"], ["--refine-moves=SPR", "--refine=none"], ["--refine-moves=nni"]):
        p = _cli(args + ["--tree=/dev/null", "x.fa"])
        assert p.returncode == 1 and p.stdout == b""
        assert "The moves of the refinement (--refine-moves) need --refine=bnni." in p.stderr.decode()
    p = _cli(["--refine=Bnni", "--refine-moves=Spr", "--trees-only", "-b", "3", "--tree=/dev/null", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "Trees (--refine=bnni) are not refined together with --trees-only" in p.stderr.decode()
    p = _cli(["--refine=spr", "x.fa"])
    assert p.returncode == 1 and "Expected one of 'none' or 'bnni' for --refine, but 'spr' was given." in p.stderr.decode()
