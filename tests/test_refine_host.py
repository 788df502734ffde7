"""Refining a tree by balanced nearest-neighbor interchanges without a GPU: the NumPy restatement (tests/bme_model.py)
against its own recursion and plain loops, bit for bit; every gain against the difference of Pauplin's length by brute
force; the balanced lengths against that length and against neighbor-joining's on an additive matrix; the search
recovering the generating tree from starts many interchanges away; max_moves, equal distances, the output numbering; the
new symbol, its argument checks; --help and the usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bme_model as bm
import nj_model
import place_model as pm
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
U = 2.0 ** -53


def _bound(n, D):
    """64 * 2^-53 * n * max D.  Where it comes from, with u = 2^-53 and M = max |D|: an A(v, c) is an average of
    distances, so |A| <= M, and it is reached through at most n - 2 averagings of one rounded addition each (the
    halving is exact): its error is below n u M.  A sum S has weights that are powers of two and add up to 1, so the
    products are exact and every partial sum stays below M; a lane makes at most ceil(n / 64) rounded additions and the
    lanes' sums take 64 more: S is within (n + n / 64 + 64) u M of the exact balanced average.  A gain is three rounded
    additions of values below 2M and an exact scaling of four such sums by 1/4: within (n + n / 64 + 66) u M.  The
    brute-force lengths it is compared with are exactly rounded sums (math.fsum of exact terms) of at most n M each, so
    their difference adds 2 n u M: together below (3n + n / 64 + 66) u M, which is below 64 n u M for every n >= 2.  The
    sum of all 2n - 3 lengths is held to the same figure: its worst case is larger (every length carries its own
    error), but the errors do not line up; the measured deviations are printed and were below 2e-15 M everywhere."""
    return 64 * U * n * np.abs(D).max()


def _noisy_tree(n, seed, noise):
    D, splits, names = nj_model.additive_tree(n, seed, noise)
    return D, splits, names


def _splits_of(J, names):
    text = nj_model.newick(J, names)
    leaves, splits, _ = nj_model.parse_newick(text)
    assert sorted(leaves) == sorted(names)
    return nj_model.unrooted_splits(splits, names)


# ---------------------------------------------------------------- 1: the surface
def test_declared_exported_and_abi_stays_5():
    from andi_amd import lib
    import andi_amd
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    shipped = C.CDLL(os.path.join(ROOT, "andi_amd", "libandihip.so"))
    assert re.search(r"\bandi_hip_refine\s*\(", header) and "andi_hip_refine" in lib.SYMBOLS
    assert getattr(L, "andi_hip_refine") is not None and getattr(shipped, "andi_hip_refine") is not None
    assert L.andi_hip_abi_version() == 5 and "#define ANDI_HIP_ABI_VERSION 5" in header  # additions only
    assert "ANDI_REFINE_BNNI = 0" in header and "} andi_hip_refine_result;" in header and "} andi_hip_refine_move;" in header
    assert lib.REFINE.itemsize == 32 and lib.REFINE == bm.REFINE and lib.REFINE_MOVE.itemsize == 16 and lib.REFINE_MOVE == bm.MOVE
    assert lib.REFINE_METHODS == bm.METHODS == ("bnni",) and bm.NJ_JOIN == lib.NJ_JOIN
    assert andi_amd.refine is lib.refine and andi_amd.REFINE is lib.REFINE and andi_amd.REFINE_MOVE is lib.REFINE_MOVE
    makefile = open(os.path.join(ROOT, "andi_amd", "csrc", "Makefile")).read()
    off = [line for line in makefile.splitlines() if line.endswith("HIPFLAGS += -ffp-contract=off")]
    assert len(off) == 1 and "build/refine.o" in off[0].split(":")[0].split()


# ---------------------------------------------------------------- 2: the model's two forms
def _same_result(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), what
    assert a[1].tobytes() == b[1].tobytes(), (what, a[1], b[1])
    assert a[2].tobytes() == b[2].tobytes(), what


@pytest.mark.parametrize("n", range(4, 21))
def test_the_vectorised_model_is_the_recursion_bit_for_bit(n):
    rng = np.random.default_rng(1000 + n)
    D, _, _ = _noisy_tree(n, 50 + n, 0.3)
    if n == 7:
        D[1, 4] = D[4, 1] = 0.0
        D[2, 3] = D[3, 2] = -0.02
    J = bm.perturb(pm.random_tree(rng, n), rng, n)
    _same_result(bm.refine(J, D), bm.refine_loops(J, D), n)
    _same_result(bm.refine(J, D, tol=1e-3, max_moves=2), bm.refine_loops(J, D, tol=1e-3, max_moves=2), (n, "capped"))
    par, kid = bm.start(J)
    a, b = bm.evaluate(bm.mirrored(D), par, kid, n), bm.evaluate_loops(bm.mirrored(D), par, kid, n)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def test_the_lower_triangle_and_the_diagonal_are_not_read():
    rng = np.random.default_rng(5)
    n = 12
    D, _, _ = _noisy_tree(n, 3, 0.3)
    J = bm.perturb(pm.random_tree(rng, n), rng, n)
    other = np.triu(D, 1) + np.tril(rng.uniform(5, 6, (n, n)))
    _same_result(bm.refine(J, D), bm.refine(J, other), "lower")


# ---------------------------------------------------------------- 3: the gains and the lengths are Pauplin's
@pytest.mark.parametrize("n", [5, 6, 9, 17])
def test_every_gain_is_the_difference_of_pauplins_length(n):
    rng = np.random.default_rng(2000 + n)
    D, _, _ = _noisy_tree(n, 70 + n, 0.3)
    J = pm.random_tree(rng, n)
    bound = _bound(n, D)
    par, kid = bm.start(J)
    T, R, _ = bm.evaluate(bm.mirrored(D), par, kid, n)
    g = bm.gains(T, R, par, kid, n)
    L = bm.lengths(T, R, par, kid, n)
    here = bm.pauplin_length(J, D)
    worst = abs(bm.seq_sum(L) - here)
    assert worst <= bound, (n, worst, bound)
    for v in range(n, 2 * n - 3):
        for alt in (0, 1):
            p2, k2 = par.copy(), kid.copy()
            bm.apply_move(p2, k2, n, v, alt)
            moved = bm.canonical(p2, k2, np.zeros(2 * n - 3), n)
            dev = abs(g[v - n, alt] - (here - bm.pauplin_length(moved, D)))
            worst = max(worst, dev)
            assert dev <= bound, (n, v, alt, dev, bound)
    print("n = %d: worst deviation %.3g, bound %.3g" % (n, worst, bound))


# ---------------------------------------------------------------- 4: an additive matrix
@pytest.mark.parametrize("n", [3, 4, 5, 9, 17, 40])
def test_on_an_additive_matrix_the_lengths_are_neighbor_joinings(n):
    D, splits, names = nj_model.additive_tree(n, 300 + n)
    J = nj_model.nj(D)
    out, res, log = bm.refine(J, D, tol=_bound(n, D))
    assert res["moves"] == 0 and res["converged"] == 1 and len(log) == 0
    assert _splits_of(out, names) == _splits_of(J, names) == splits
    # the same tree in two numberings: compare the length of every branch by its split
    def exact(K):
        par, kid = bm.start(K)
        below = bm.leaf_sets(kid, n, bm.bfs(par, kid, n)[0])
        L = pm.edges(K, n)[1]
        out = {}
        for v in range(2 * n - 3):
            s = frozenset(np.nonzero(below[v])[0].tolist())
            out[frozenset(range(n)) - s if 0 in s else s] = L[v]
        return out

    mine, theirs = exact(out), exact(J)
    assert mine.keys() == theirs.keys()
    worst = max(abs(mine[s] - theirs[s]) for s in mine)
    print("n = %d: worst deviation from NJ's lengths %.3g, bound %.3g" % (n, worst, _bound(n, D)))
    assert worst <= _bound(n, D)
    assert res["length_before"] == res["length_after"]


# ---------------------------------------------------------------- 5: recovery
@pytest.mark.parametrize("seed", range(100, 105))
@pytest.mark.parametrize("n", [8, 33, 65])
def test_the_search_recovers_the_generating_tree(n, seed):
    D, splits, names = nj_model.additive_tree(n, seed)
    rng = np.random.default_rng(seed)
    J = bm.perturb(nj_model.nj(D), rng, n)
    before = bm.pauplin_length(J, D)
    out, res, log = bm.refine(J, D, tol=2.0 ** -32 * before)
    print("n = %d seed %d: %d splits away, %d moves" % (n, seed, len(splits - _splits_of(J, names)), res["moves"]))
    assert res["converged"] == 1
    assert _splits_of(out, names) == splits


# ---------------------------------------------------------------- 6, 7: max_moves, equal distances
def test_one_move_allowed_gives_one_move_and_a_shorter_tree():
    n, seed = 33, 100
    D, splits, names = nj_model.additive_tree(n, seed)
    J = bm.perturb(nj_model.nj(D), np.random.default_rng(seed), n)
    out, res, log = bm.refine(J, D, tol=0.0, max_moves=1)
    assert res["moves"] == 1 and res["converged"] == 0 and len(log) == 1 and log[0]["gain"] > 0
    assert bm.pauplin_length(out, D) < bm.pauplin_length(J, D)
    assert res["length_after"] < res["length_before"]
    assert abs((res["length_before"] - res["length_after"]) - log[0]["gain"]) <= 2 * _bound(n, D)
    none = bm.refine(J, D, tol=0.0, max_moves=0)
    assert none[1]["moves"] == 0 and none[1]["converged"] == 0 and none[1]["length_before"] == none[1]["length_after"]
    assert _splits_of(none[0], names) == _splits_of(J, names)


@pytest.mark.parametrize("n", [3, 4, 9, 70])
def test_equal_distances_give_no_move(n):
    rng = np.random.default_rng(n)
    D = np.full((n, n), 0.25) - 0.25 * np.eye(n)
    J = pm.random_tree(rng, n)
    out, res, log = bm.refine(J, D)
    assert res["moves"] == 0 and res["converged"] == 1 and len(log) == 0
    assert bm.inner_splits(out) == bm.inner_splits(J)


# ---------------------------------------------------------------- 8: the output records
@pytest.mark.parametrize("n", [3, 4, 5, 12, 66])
def test_the_output_records_parse_back_and_keep_the_leaves(n):
    from andi_amd import lib
    rng = np.random.default_rng(40 + n)
    D, _, names = _noisy_tree(n, 90 + n, 0.3)
    J = bm.perturb(pm.random_tree(rng, n), rng, n)
    out, res, log = bm.refine(J, D, tol=1e-12)
    text = lib.newick(out, names)
    assert text == nj_model.newick(out, names) and text.endswith(";\n")
    back = lib.parse_newick(text, names)
    assert bm.inner_splits(back) == bm.inner_splits(out)
    leaves, _, _ = nj_model.parse_newick(text)
    assert sorted(leaves) == sorted(names)
    # the numbering: pair records ascending in (a < b), the final record x < y < z, every node a child once
    par, kid = bm.start(out)
    assert (out["a"][:-1] < out["b"][:-1]).all() and out[-1]["a"] < out[-1]["b"] < out[-1]["c"]
    # canonical: numbering the result again changes nothing
    assert bm.canonical(par, kid, pm.edges(out, n)[1], n).tobytes() == out.tobytes()
    for m in log:
        assert 0 <= m["first"] < n and 0 <= m["second"] < n and m["first"] != m["second"] and m["gain"] > 1e-12


# ---------------------------------------------------------------- 9: the argument checks
def test_bad_arguments_are_refused_before_any_hip_call():
    from andi_amd import lib
    L = lib.load()
    n = 5
    J = pm.random_tree(np.random.default_rng(1), n)
    D = np.ones((n, n))
    out, res = np.zeros(n - 2, lib.NJ_JOIN), np.zeros(1, lib.REFINE)
    j, d, o, r = J.ctypes.data, D.ctypes.data, out.ctypes.data, res.ctypes.data
    # with no context nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, j, n, d, 0, 0.0, 10, o, r, None), (None, None, n, d, 0, 0.0, 10, o, r, None),
                 (None, j, 2, d, 0, 0.0, 10, o, r, None), (None, j, 65536, d, 0, 0.0, 10, o, r, None),
                 (None, j, n, d, 1, 0.0, 10, o, r, None), (None, j, n, d, 0, -1.0, 10, o, r, None),
                 (None, j, n, d, 0, float("nan"), 10, o, r, None)]:
        assert L.andi_hip_refine(*args) == 1, args
    assert out.tobytes() == bytes(out.nbytes) and res.tobytes() == bytes(res.nbytes)
    with pytest.raises(ValueError):
        lib.refine(None, J, D, method="spr")
    with pytest.raises(ValueError):
        lib.refine(None, J, D[:-1])
    with pytest.raises(ValueError):
        lib.refine(None, J, D, max_moves=-1)


# ---------------------------------------------------------------- the command line, as far as it goes without a GPU
def _cli(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=60, stdin=subprocess.DEVNULL)


def test_help_names_the_options_and_usage_errors():
    p = _cli(["--help"])
    assert p.returncode == 0
    text = p.stdout.decode()
    assert "--refine=METHOD" in text and "--refine-tol=X" in text and "--refine-report=FILE" in text and "'bnni'" in text
    p = _cli(["--refine=bogus", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "Expected one of 'none' or 'bnni' for --refine, but 'bogus' was given." in p.stderr.decode()
    for spelling in ("bnni", "BNNI"):
        p = _cli(["--refine=" + spelling, "--trees-only", "-b", "3", "--tree=/dev/null", "x.fa"])
        assert p.returncode == 1 and p.stdout == b""
        assert "Trees (--refine=bnni) are not refined together with --trees-only" in p.stderr.decode()
    for args in (["--refine-report=/dev/null"], ["--refine-report=/dev/null", "--refine=none"]):
        p = _cli(args + ["--tree=/dev/null", "x.fa"])
        assert p.returncode == 1 and p.stdout == b""
        assert "A refinement report (--refine-report) needs --refine=bnni." in p.stderr.decode()
    for bad in ("-1", "nan", "x"):
        p = _cli(["--refine=bnni", "--refine-tol=" + bad, "--tree=/dev/null", "x.fa"])
        assert p.returncode == 1 and p.stdout == b""
        assert "--refine-tol" in p.stderr.decode()
