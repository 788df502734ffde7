"""andi_hip_nj on the MI355X: bit-exact to the NumPy restatement (tests/nj_model.py) on random matrices and on ties, at
the sizes where the kernels change paths (more than 1024 active nodes, more than 1024 tiles: the 3085-leaf bench tree),
with overflow of finite input, the splits of additive trees and of scanned genomes, non-finite input, determinism, and
andi-hip --tree."""
import os
import subprocess

import numpy as np
import pytest

import nj_model
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _same(got, want):
    for f in ("a", "b", "c", "pad"):
        assert (got[f] == want[f]).all(), f
    for f in ("la", "lb", "lc"):
        assert (got[f].view(np.uint64) == want[f].view(np.uint64)).all(), f


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 64, 257, 1000])
def test_bit_exact_on_random_matrices(ctx, n):
    from andi_amd import lib
    for seed in ((1,) if n == 1000 else (1, 2, 3)):
        rng = np.random.default_rng(1000 * n + seed)
        D = _sym(rng, n)
        if seed == 2:  # the lower triangle and the diagonal are not read
            D = D + np.tril(rng.uniform(-5, 5, (n, n)))
        _same(lib.nj(ctx, D), nj_model.nj(D))


def test_ties(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(5)
    cases = [np.ones((9, 9)) - np.eye(9), 0.25 * (np.ones((40, 40)) - np.eye(40))]
    # duplicated rows: the distance between duplicates is +0.0 or -0.0
    base = _sym(rng, 12)
    idx = np.array([0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 11])
    dup = base[np.ix_(idx, idx)]
    for i in range(len(idx)):
        for j in range(len(idx)):
            if i != j and idx[i] == idx[j]:
                dup[i, j] = -0.0 if (i + j) % 2 else 0.0
    cases.append(dup)
    for n in (6, 23, 70):  # small integers: many exact ties in Q
        cases.append(np.triu(rng.integers(0, 4, (n, n)).astype(float), 1))
        cases[-1] = cases[-1] + cases[-1].T
    for D in cases:
        _same(lib.nj(ctx, D), nj_model.nj(D))


def test_bit_exact_past_1024_active_nodes(ctx):
    # r > 1024 for the first 76 steps: k_nj_rowsum's second pass (base > 0, a partial chunk) and k_nj_join's strided
    # walk of the active list
    from andi_amd import lib
    D = _sym(np.random.default_rng(1100), 1100)
    _same(lib.nj(ctx, D), nj_model.nj(D))


def _children_once(J, n):
    kids = np.concatenate([J["a"], J["b"], J["c"][J["c"] >= 0]])
    assert (np.sort(kids) == np.arange(2 * n - 3)).all()  # every leaf and every joined node but the root, once


def test_the_3085_leaf_bench_tree(ctx):
    # the bench's matrix: more than 1024 tiles of 64 x 64 while r >= 2817 (the first 269 steps), so k_nj_join folds the
    # tile minima with a stride; k_nj_rowsum's third pass while r > 2048
    from andi_amd import lib
    n = 3085
    D, _, names = nj_model.additive_tree(n, seed=n, noise=0.01)
    J = lib.nj(ctx, D)
    _same(J[:269], nj_model.nj(D, steps=269))
    _children_once(J, n)
    leaves, _, _ = nj_model.parse_newick(lib.newick(J, names))
    assert sorted(leaves) == sorted(names)


def test_the_3085_leaf_additive_tree_is_recovered(ctx):
    from andi_amd import lib
    n = 3085
    D, splits, names = nj_model.additive_tree(n, seed=n)
    J = lib.nj(ctx, D)
    _children_once(J, n)
    leaves, got, _ = nj_model.parse_newick(lib.newick(J, names))
    assert len(leaves) == n and nj_model.unrooted_splits(got, names) == splits
    assert np.abs(nj_model.patristic(J, n) - D).max() < 1e-9


def _small_integers(rng, n):
    A = np.triu(rng.integers(0, 4, (n, n)).astype(float), 1)
    return A + A.T


@pytest.mark.parametrize("n", [300, 1100])
def test_ties_of_small_integers(ctx, n):
    from andi_amd import lib
    D = _small_integers(np.random.default_rng(n + 7), n)
    _same(lib.nj(ctx, D), nj_model.nj(D))


def test_ties_with_more_than_1024_tiles(ctx):
    # n = 2900: 1081 tiles at the first step, more than 1024 for the first 84 steps.  Small integers, and equal distances
    # with two pairs at 0: the two least Q tie, one in tile 0, one in tile 1024 (rows 2176..2239, columns 2816..2879),
    # which k_nj_join's thread 0 folds one after the other; after them every Q ties
    from andi_amd import lib
    n = 2900
    D = _small_integers(np.random.default_rng(2900), n)
    _same(lib.nj(ctx, D)[:100], nj_model.nj(D, steps=100))
    E = np.ones((n, n))
    E[0, 1] = E[1, 0] = 0.0
    E[2200, 2850] = E[2850, 2200] = -0.0
    J = lib.nj(ctx, E)
    _same(J[:100], nj_model.nj(E, steps=100))
    assert (J["a"][0], J["b"][0]) == (0, 1) and (J["a"][1], J["b"][1]) == (2200, 2850)


def test_ties_of_duplicated_leaves_in_other_tiles(ctx):
    # leaf k + 150 repeats leaf k (at +0.0 or -0.0 from it): its pairs tie with leaf k's, 150 slots and 2 or 3 tiles away
    from andi_amd import lib
    rng = np.random.default_rng(150)
    base = _sym(rng, 150)
    idx = np.r_[np.arange(150), np.arange(150)]
    D = base[np.ix_(idx, idx)]
    for k in range(150):
        D[k, k + 150] = D[k + 150, k] = -0.0 if k % 2 else 0.0
    _same(lib.nj(ctx, D), nj_model.nj(D))


def _same_overflowed(got, want):
    """ids exactly; lengths by their bits unless NaN (the bits of inf - inf are the platform's, not the contract's)"""
    for f in ("a", "b", "c", "pad"):
        assert (got[f] == want[f]).all(), f
    for f in ("la", "lb", "lc"):
        nan = np.isnan(want[f])
        assert (np.isnan(got[f]) == nan).all(), f
        assert (got[f][~nan].view(np.uint64) == want[f][~nan].view(np.uint64)).all(), f


def test_overflow_of_finite_input(ctx):
    # entries up to the largest double: row sums and (r-2) * D overflow; Q is -inf, +inf or NaN (inf - inf), and a NaN Q
    # orders after every number, NaN against NaN by id
    from andi_amd import lib
    big = 1.7e308
    D = np.zeros((5, 5))
    D[0, 1:] = D[1, 2:] = big
    D[2, 3], D[2, 4], D[3, 4] = 1.0, 2.0, 3.0
    J = lib.nj(ctx, D)
    _same_overflowed(J, nj_model.nj(D))
    assert (J["a"][0], J["b"][0]) == (2, 3)  # Q(2, 3) = -inf; Q(0, 1) = NaN
    seen = set()
    for n in (6, 40, 130):
        rng = np.random.default_rng(n)
        A = rng.uniform(0.0, 1.0, (n, n))
        far = rng.choice(n, max(2, n // 10), replace=False)  # leaves about 1e307 from all others
        A[:, far] = rng.uniform(0.5, 1.5, (n, len(far))) * 1e307
        A[far, :] = A[:, far].T
        A[far[0], far[1]] = A[far[1], far[0]] = big
        D = np.triu(A, 1) + np.triu(A, 1).T
        want = nj_model.nj(D)
        _same_overflowed(lib.nj(ctx, D), want)
        L = np.concatenate([want["la"], want["lb"]])
        seen |= {"nan"} if np.isnan(L).any() else set()
        seen |= {"inf"} if np.isinf(L).any() else set()
        seen |= {"finite"} if np.isfinite(L).any() else set()
    assert seen == {"nan", "inf", "finite"}
    D = np.full((70, 70), big)  # every Q NaN: the id order alone
    J = lib.nj(ctx, D)
    _same_overflowed(J, nj_model.nj(D))
    assert (J["a"][:3] == [0, 2, 4]).all() and (J["b"][:3] == [1, 3, 5]).all()


@pytest.mark.parametrize("n", [100, 500])
def test_additive_trees_are_recovered(ctx, n):
    from andi_amd import lib
    D, splits, names = nj_model.additive_tree(n, seed=n)
    J = lib.nj(ctx, D)
    leaves, got, lengths = nj_model.parse_newick(lib.newick(J, names))
    assert sorted(leaves) == sorted(names)
    assert nj_model.unrooted_splits(got, names) == splits
    # the lengths: the tree's path between any two leaves is their distance
    assert np.abs(nj_model.patristic(J, n) - D).max() < 1e-9
    assert (J["la"] > 0).all() and (J["lb"] > 0).all()


def test_scanned_genomes_give_the_expected_tree(ctx):
    from andi_amd import lib, synth
    seqs, expected = synth.tree_set(12, 200_000, seed=31)
    names = ["g%d" % i for i in range(12)]
    want = nj_model.unrooted_splits(nj_model.parse_newick(lib.newick(lib.nj(ctx, expected), names))[1], names)
    D = lib.distances(lib.dist_matrix(seqs, model=lib.M_JC, host_threads=8), lib.M_JC)
    got = nj_model.unrooted_splits(nj_model.parse_newick(lib.newick(lib.nj(ctx, D), names))[1], names)
    assert got == want
    _same(lib.nj(ctx, D), nj_model.nj(D))


def test_non_finite_input(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(9)
    for bad in (np.nan, np.inf, -np.inf):
        D = _sym(rng, 30)
        D[4, 17] = bad
        D[9, 20] = np.nan
        with pytest.raises(lib.AndiHipError, match=r"D\[4\]\[17\] is not finite"):
            lib.nj(ctx, D)
    D = _sym(rng, 30)
    want = nj_model.nj(D)
    D[np.arange(30), np.arange(30)] = np.nan  # the diagonal and the lower triangle are ignored
    D[20, 3] = np.inf
    D[29, 0] = np.nan
    _same(lib.nj(ctx, D), want)
    with pytest.raises(lib.AndiHipError, match=r"D\[0\]\[1\] is not finite"):
        lib.nj(ctx, np.array([[0.0, np.nan], [1.0, 0.0]]))


def test_determinism(ctx):
    from andi_amd import lib
    D = _sym(np.random.default_rng(11), 300)
    a, b = lib.nj(ctx, D), lib.nj(ctx, D)
    other = lib.Context(0)
    try:
        c = lib.nj(other, D)
    finally:
        other.close()
    assert a.tobytes() == b.tobytes() == c.tobytes()


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.mark.timeout(900)
def test_cli_tree(tmp_path, ctx):
    from andi_amd import lib, synth
    n = 8
    seqs, _ = synth.tree_set(n, 100_000, seed=77)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    env = dict(os.environ, ANDI_HIP_GPUS="1")
    tree = str(tmp_path / "t.nwk")

    def run(args, status=0):
        p = subprocess.run([CLI, "-t", "4"] + args, capture_output=True, timeout=300, env=env)
        assert p.returncode == status, p.stderr.decode()
        return p.stdout, p.stderr

    M = {m: lib.dist_matrix(seqs, model=lib.MODEL_NAMES[m.lower()], host_threads=4) for m in ("JC", "Kimura")}
    for model in ("JC", "Kimura"):
        plain = run(["-m", model] + files)
        with_tree = run(["-m", model, "--tree=" + tree] + files)
        assert with_tree == plain
        lines = open(tree).read().splitlines(keepends=True)
        D = lib.distances(M[model], lib.MODEL_NAMES[model.lower()])
        assert lines == [lib.newick(lib.nj(ctx, D), names)], model
    # -vv prints the matrix of one direction; the tree keeps the averaged distances
    run(["-vv", "--tree=" + tree] + files)
    first = open(tree).read()
    run(["--tree=" + tree] + files)
    assert open(tree).read() == first
    # -b 3: three lines, the first unchanged, each a tree over every leaf
    run(["-b", "3", "--tree=" + tree] + files)
    lines = open(tree).read().splitlines(keepends=True)
    assert len(lines) == 3 and lines[0] == first
    for line in lines:
        leaves, _, _ = nj_model.parse_newick(line)
        assert sorted(leaves) == sorted(names)
    # unrelated sequences (the reference's test/nan.sh): a nan distance, a warning, no line, status 1, the same stdout
    pair = [_fasta(tmp_path / ("%s.fa" % x), x, synth.unrelated(10_000, 40 + k)) for k, x in enumerate(("x", "y"))]
    plain_out, plain_err = run(pair, status=1)
    out, err = run(["--tree=" + tree] + pair, status=1)
    assert b"nan" in out and out == plain_out
    assert err.decode() == plain_err.decode() + "andi-hip: No tree for matrix 1: the distance of 'x' and 'y' is not finite.\n"
    assert open(tree).read() == ""
