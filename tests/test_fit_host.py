"""Refitting branch lengths without a GPU: the NumPy restatement (tests/fit_model.py) against its own plain loops, bit for
bit, and against LAPACK's least squares on the path design matrix; the refit never explains the matrix worse than the
joined lengths; the per-leaf sums and the worst pair; andi_hip_relength; the new symbols; --help and the usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bionj_model
import fit_model as fm
import nj_model
import place_model as pm
from conftest import ROOT
from newick_reader import parse as _parse, splits as _splits

NEW = ("andi_hip_fit", "andi_hip_relength")
CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
# The model's worst deviation from numpy.linalg.lstsq over the cases of test_the_lengths_are_lapacks_least_squares,
# relative to the largest distance of the case, was 7.31e-15 where this was written (4.57e-15 on the random trees, 3.75e-15
# on the caterpillars, 7.31e-15 on the balanced trees; OpenBLAS, these seeds); both sides are
# reference computations, and 64 times that is allowed for other BLAS builds and seeds.
MEASURED = 7.31e-15
TOL = 64 * MEASURED


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
    assert lib.FIT.itemsize == 72 and fm.FIT == lib.FIT and lib.FIT_METHODS == fm.METHODS == ("ols",)
    assert andi_amd.fit is lib.fit and andi_amd.relength is lib.relength and andi_amd.FIT is lib.FIT
    knobs_h = open(os.path.join(ROOT, "andi_amd", "csrc", "knobs.h")).read()
    shipped_list, hooks = knobs_h.split("#define ANDI_KNOB_LIST_HOOKS(X)")
    assert "X(FIT_GROUP)" in hooks.split("#define ANDI_KNOB_LIST(X)")[0] and "FIT_GROUP" not in shipped_list


# ---------------------------------------------------------------- trees and matrices
def _tree(shape, rng, n, lengths=None):
    lengths = rng.uniform(0.01, 0.1, 2 * n - 3) if lengths is None else lengths
    if shape == "random":
        it = iter(lengths)
        return pm.random_tree(rng, n, lambda k: [next(it) for _ in range(k)])
    return getattr(pm, shape)(n, lengths)


def _design(J, n):
    """(A, pairs): A[pair, v] = 1 iff edge v lies on the path between the pair's leaves"""
    _, below, _, _ = pm.paths(J, n)
    E = 2 * n - 3
    pairs = [(b, c) for b in range(n) for c in range(b + 1, n)]
    return np.array([(below[:E, b] != below[:E, c]).astype(np.float64) for b, c in pairs]), pairs


def _matrix(n, pairs, d):
    D = np.zeros((n, n))
    for (b, c), x in zip(pairs, d):
        D[b, c] = D[c, b] = x
    return D


def _noisy(J, n, rng, noise=0.3):
    A, pairs = _design(J, n)
    d = A @ pm.edges(J, n)[1]
    return _matrix(n, pairs, d * (1.0 + rng.uniform(-noise, noise, len(d)))), A, pairs


SHAPES = ("random", "caterpillar", "balanced")


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("shape", SHAPES)
def test_the_vectorised_model_is_the_plain_loops_bit_for_bit(shape):
    rng = np.random.default_rng(100 + len(shape))
    for n in range(3, 13):
        J = _tree(shape, rng, n)
        D, _, _ = _noisy(J, n, rng)
        if n == 7:
            D[1, 4] = D[4, 1] = 0.0
            D[2, 3] = D[3, 2] = -0.02
        length, rec, leaf, leaf_joined = fm.fit(J, D, per=True)
        l2, rss, rss_joined, tss, leaf2, leaf_joined2, worst = fm.fit_loops(J, D)
        assert length.tobytes() == l2.tobytes(), n
        assert (rec["rss"], rec["rss_joined"], rec["tss"]) == (rss, rss_joined, tss), n
        assert leaf.tobytes() == leaf2.tobytes() and leaf_joined.tobytes() == leaf_joined2.tobytes(), n
        assert (rec["worst_b"], rec["worst_c"], rec["worst"]) == worst, n
        assert rec["pairs"] == n * (n - 1) // 2


def test_the_lower_triangle_and_the_diagonal_are_not_read():
    rng = np.random.default_rng(5)
    n = 9
    J = _tree("random", rng, n)
    D, _, _ = _noisy(J, n, rng)
    other = np.triu(D, 1) + np.tril(rng.uniform(5, 6, (n, n)))
    a, b = fm.fit(J, D, per=True), fm.fit(J, other, per=True)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_lengths_are_lapacks_least_squares(shape):
    """The model's lengths against numpy.linalg.lstsq on the 0/1 path design matrix.  Measured over these cases: a worst
    deviation of 7.31e-15 of the largest distance (MEASURED); the bound is 64 times that, 4.7e-13 (TOL).  The figure of
    this run is printed."""
    rng = np.random.default_rng(200 + len(shape))
    worst = 0.0
    for n in range(3, 41):
        J = _tree(shape, rng, n)
        D, A, pairs = _noisy(J, n, rng)
        want = np.linalg.lstsq(A, np.array([D[b, c] for b, c in pairs]), rcond=None)[0]
        got, rec = fm.fit(J, D)
        dev = np.abs(got - want).max() / D.max()
        worst = max(worst, dev)
        assert dev <= TOL, (n, dev)
        # the refit is the minimum: it never explains the matrix worse than the lengths the tree came with
        assert rec["rss"] <= rec["rss_joined"] * (1 + TOL), n
        res = A @ got - np.array([D[b, c] for b, c in pairs])
        assert rec["rss"] == pytest.approx(float(res @ res), rel=1e-9, abs=1e-24)
    print("worst deviation from lstsq, relative to the largest distance: %.3g" % worst)


@pytest.mark.parametrize("shape", SHAPES)
def test_an_additive_matrix_gives_the_trees_own_lengths_back(shape):
    rng = np.random.default_rng(300 + len(shape))
    for n in (3, 4, 5, 8, 17, 40):
        lengths = rng.integers(2, 17, 2 * n - 3) / 64.0
        J = _tree(shape, rng, n, lengths)
        A, pairs = _design(J, n)
        own = pm.edges(J, n)[1]
        D = _matrix(n, pairs, A @ own)  # (dyadic: every path length is exact)
        got, rec = fm.fit(J, D)
        assert np.abs(got - own).max() <= TOL * D.max(), n
        assert rec["rss"] <= (TOL * D.max()) ** 2 * len(pairs) * n and rec["rss_joined"] == 0.0
        assert rec["negative"] == rec["negative_joined"] == 0
        assert rec["length"] == pytest.approx(own.sum(), rel=1e-12) and rec["length_joined"] == pytest.approx(own.sum(), rel=1e-15)


@pytest.mark.parametrize("builder", ["nj", "bionj"])
def test_the_refit_never_fits_worse_than_the_joined_lengths(builder):
    rng = np.random.default_rng(400 + len(builder))
    for n in (5, 12, 30):
        D, _, _ = _noisy(_tree("random", rng, n), n, rng, 0.4)
        J = nj_model.nj(D) if builder == "nj" else bionj_model.bionj(D)
        length, rec, leaf, leaf_joined = fm.fit(J, D, per=True)
        assert rec["rss"] <= rec["rss_joined"] * (1 + TOL), (n, rec)
        assert 0.0 < fm.r2(rec, joined=True) <= fm.r2(rec) <= 1.0
        # every pair is in two leaves' sums
        assert leaf.sum() == pytest.approx(2 * rec["rss"], rel=1e-12) and leaf_joined.sum() == pytest.approx(2 * rec["rss_joined"], rel=1e-12)
        R = fm.residuals(fm.relength(J, length), D)
        b, c = int(rec["worst_b"]), int(rec["worst_c"])
        assert b < c and abs(R[b, c]) == np.abs(R).max() and rec["worst"] == R[b, c]
        assert rec["negative"] == (length < 0).sum() and rec["length"] == pytest.approx(length.sum(), rel=1e-12)


def test_the_worst_pair_orders_a_nan_below_every_number():
    assert fm.worst_pair(np.array([[0, np.nan, 1.0], [np.nan, 0, -1.0], [1.0, -1.0, 0]]))[:2] == (0, 2)  # (the first of a tie)
    b, c, r = fm.worst_pair(np.full((3, 3), np.nan))
    assert (b, c) == (-1, -1) and np.isnan(r)
    assert fm.worst_pair(np.array([[0, np.nan, np.nan], [np.nan, 0, 0.0], [np.nan, 0.0, 0]]))[:2] == (1, 2)


def test_r2_is_nan_without_variance():
    rec = np.zeros(1, fm.FIT)[0]
    assert np.isnan(fm.r2(rec))


# ---------------------------------------------------------------- andi_hip_relength
@pytest.mark.parametrize("shape", SHAPES)
def test_relength_puts_every_length_on_its_child(shape):
    from andi_amd import lib
    rng = np.random.default_rng(500 + len(shape))
    for n in (3, 4, 5, 9, 20):
        J = _tree(shape, rng, n)
        new = rng.integers(2, 1000, 2 * n - 3) / 1024.0
        new[0] = -0.125  # (negative lengths are kept)
        out = lib.relength(J, new)
        assert out.tobytes() == fm.relength(J, new).tobytes()
        for f in ("a", "b", "c", "pad"):
            assert (out[f] == J[f]).all()
        parent, L = pm.edges(out, n)
        assert (parent == pm.edges(J, n)[0]).all() and L.tobytes() == new.tobytes()
        assert (out["lc"][:-1] == J["lc"][:-1]).all()  # a pair record has no third child: copied
        # the text of the result parses back to the same splits, with the new lengths
        names = ["t%d" % i for i in range(n)]
        index = {nm: i for i, nm in enumerate(names)}
        got = _splits(_parse(lib.newick(out, names)), index, n, {})
        want = _splits(_parse(lib.newick(J, names)), index, n, {})
        assert set(got) == set(want)
        _, below, _, _ = pm.paths(J, n)
        for v in range(2 * n - 3):
            s = frozenset(np.nonzero(below[v])[0].tolist())
            side = s if 0 not in s else frozenset(range(n)) - s
            assert [length for length, _ in got[side]] == ["%.8g" % new[v]], v
        # in place
        same = J.copy()
        assert lib.load().andi_hip_relength(same.ctypes.data, n, new.ctypes.data, same.ctypes.data) == 0
        assert same.tobytes() == out.tobytes()


def test_relength_refuses_what_is_not_a_tree():
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(6)
    n = 9
    J = pm.random_tree(rng, n)
    new = np.full(2 * n - 3, 0.5)
    late = J.copy()
    late[2]["b"] = n + 5  # a child that no earlier record made
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    negative = J.copy()
    negative[1]["a"] = -1
    out = np.zeros(n - 2, lib.NJ_JOIN)
    for bad in (late, twice, negative):
        assert L.andi_hip_relength(bad.ctypes.data, n, new.ctypes.data, out.ctypes.data) == 1
        with pytest.raises(ValueError):
            lib.relength(bad, new)
    assert L.andi_hip_relength(None, n, new.ctypes.data, out.ctypes.data) == 1
    assert L.andi_hip_relength(J.ctypes.data, n, None, out.ctypes.data) == 1
    assert L.andi_hip_relength(J.ctypes.data, n, new.ctypes.data, None) == 1
    assert L.andi_hip_relength(J.ctypes.data, 2, new.ctypes.data, out.ctypes.data) == 1
    assert out.tobytes() == bytes(out.nbytes)  # nothing written
    with pytest.raises(ValueError):
        lib.relength(J, new[:-1])


# ---------------------------------------------------------------- the command line, as far as it goes without a GPU
def _cli(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=60, stdin=subprocess.DEVNULL)


def test_help_names_the_options_and_usage_errors():
    p = _cli(["--help"])
    assert p.returncode == 0
    text = p.stdout.decode()
    assert "--lengths=KIND" in text and "--fit=FILE" in text and "'joined'" in text and "'ols'" in text
    p = _cli(["--lengths=bogus", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "Expected one of 'joined' or 'ols' for --lengths, but 'bogus' was given." in p.stderr.decode()
    for spelling in ("ols", "OLS"):
        p = _cli(["--lengths=" + spelling, "--trees-only", "-b", "3", "--tree=/dev/null", "x.fa"])
        assert p.returncode == 1 and p.stdout == b""
        assert "Branch lengths (--lengths=ols) are not refit together with --trees-only" in p.stderr.decode()
    p = _cli(["--fit=/dev/null", "--reference=r.fa", "x.fa"])
    assert p.returncode == 1 and p.stdout == b""
    assert "A fit report (--fit) is not available together with --reference or --reference-list." in p.stderr.decode()
