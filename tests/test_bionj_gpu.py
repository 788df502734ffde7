"""BIONJ on the MI355X (andi_hip_tree, andi_hip_tree_batch, andi_hip_bootstrap_tree with ANDI_TREE_BIONJ): bit-exact to
the NumPy restatement (tests/bionj_model.py) at the sizes where the kernels change paths, on each of lambda's branches
(inside (0, 1), clamped, halved because vab is 0 or the quotient NaN), with overflow of finite input and non-finite input;
method "nj" equal to the neighbor-joining calls byte for byte; batches, groups and split ranges; determinism; and
andi-hip --tree-method."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bionj_model
import nj_model
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
SEED = 20240917


def _same(got, want):
    for f in ("a", "b", "c", "pad"):
        assert (got[f] == want[f]).all(), f
    for f in ("la", "lb", "lc"):
        assert (got[f].view(np.uint64) == want[f].view(np.uint64)).all(), f


def _same_overflowed(got, want):
    """ids exactly; lengths by their bits unless NaN (the bits of inf - inf are the platform's, not the contract's)"""
    for f in ("a", "b", "c", "pad"):
        assert (got[f] == want[f]).all(), f
    for f in ("la", "lb", "lc"):
        nan = np.isnan(want[f])
        assert (np.isnan(got[f]) == nan).all(), f
        assert (got[f][~nan].view(np.uint64) == want[f][~nan].view(np.uint64)).all(), f


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _small_integers(rng, n):
    A = np.triu(rng.integers(0, 4, (n, n)).astype(float), 1)
    return A + A.T


# ------------------------------------------------------------------ 1, 2: random matrices at the sizes that change paths
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 64, 65, 257, 1000])
def test_bit_exact_on_random_matrices(ctx, n):
    # 2 and 3: the final record alone; 4: one step; 64 and 65: either side of an argmin tile and of a full wavefront of the
    # row chain; 257: the chain's last chunk partly filled
    from andi_amd import lib
    for seed in ((1,) if n == 1000 else (1, 2, 3)):
        rng = np.random.default_rng(1000 * n + seed)
        D = _sym(rng, n)
        if seed == 2:  # the lower triangle and the diagonal are not read
            D = D + np.tril(rng.uniform(-5, 5, (n, n)))
        _same(lib.tree(ctx, D, "bionj"), bionj_model.bionj(D))


def test_bit_exact_past_1024_active_nodes(ctx):
    # r > 1024 for the first 76 steps: the join kernel's strided pass and the row chain's 1024-entry pass take a second trip
    from andi_amd import lib
    D = _sym(np.random.default_rng(1100), 1100)
    _same(lib.tree(ctx, D, "bionj"), bionj_model.bionj(D))


# ------------------------------------------------------------------ 3: lambda's branches, each shown hit by the model
@pytest.mark.parametrize("seed", [0, 3])
def test_lambda_inside_and_clamped(ctx, seed):
    # seed 0: one step is clamped to 0; seed 3: one to 1; 56 steps of each strictly inside (0, 1)
    from andi_amd import lib
    D, _, _ = nj_model.additive_tree(60, seed, 0.15)
    want, lam = bionj_model.bionj(D, lambdas=True)
    free = lam["value"][~lam["halved"]]
    assert (free == (0.0 if seed == 0 else 1.0)).any() and ((free > 0) & (free < 1)).any()
    _same(lib.tree(ctx, D, "bionj"), want)


@pytest.mark.parametrize("n", [6, 23, 70])
def test_lambda_halved_where_vab_is_zero(ctx, n):
    # small integers with zeros off the diagonal: many joins of a pair at variance 0
    from andi_amd import lib
    D = _small_integers(np.random.default_rng(5 + n), n)
    want, lam = bionj_model.bionj(D, lambdas=True)
    assert lam["halved"].any()
    got = lib.tree(ctx, D, "bionj")
    _same(got, want)
    if n > 6:  # the joined ids are not neighbor-joining's: a build that quietly runs NJ fails here
        other = nj_model.nj(D)
        assert (want["a"] != other["a"]).any() or (want["b"] != other["b"]).any()
        assert (got["a"] != other["a"]).any() or (got["b"] != other["b"]).any()


def test_lambda_of_duplicated_leaves(ctx):
    # leaves 3, 3 and 7 once more: distance 0, so vab = 0 at a pair of leaves
    from andi_amd import lib
    base, _, _ = nj_model.additive_tree(20, 2, 0.05)
    idx = np.r_[np.arange(20), 3, 3, 7]
    D = base[np.ix_(idx, idx)]
    want, lam = bionj_model.bionj(D, lambdas=True)
    assert lam["halved"].any()
    got = lib.tree(ctx, D, "bionj")
    _same(got, want)
    assert all(np.isfinite(got[f]).all() for f in ("la", "lb", "lc"))


# ------------------------------------------------------------------ 4: overflow of finite input
@pytest.mark.parametrize("n", [6, 40, 130])
def test_overflow_of_finite_input(ctx, n):
    # entries near 1.5e308: row sums of D and of V overflow, lambda's quotient is inf / inf = NaN (then 1/2) or +-inf
    # (then clamped); NaN and inf in the lengths are part of the contract
    from andi_amd import lib
    rng = np.random.default_rng(n)
    A = rng.uniform(0.0, 1.0, (n, n))
    far = rng.choice(n, max(2, n // 10), replace=False)  # leaves about 1e307 from all others
    A[:, far] = rng.uniform(0.5, 1.5, (n, len(far))) * 1e307
    A[far, :] = A[:, far].T
    A[far[0], far[1]] = A[far[1], far[0]] = 1.5e308
    D = np.triu(A, 1) + np.triu(A, 1).T
    want = bionj_model.bionj(D)
    _same_overflowed(lib.tree(ctx, D, "bionj"), want)
    L = np.concatenate([want["la"], want["lb"]])
    print("n = %d: %d NaN, %d inf, %d finite lengths" % (n, np.isnan(L).sum(), np.isinf(L).sum(), np.isfinite(L).sum()))


def test_overflow_where_every_q_is_nan(ctx):
    from andi_amd import lib
    D = np.full((70, 70), 1.5e308)  # every Q NaN: the id order alone; the row sums of V are inf, lambda's quotient NaN
    want, lam = bionj_model.bionj(D, lambdas=True)
    assert lam["halved"][0] and (want["a"][:3] == [0, 2, 4]).all()
    _same_overflowed(lib.tree(ctx, D, "bionj"), want)


# ------------------------------------------------------------------ 5: non-finite input
def test_non_finite_input(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(9)
    for bad in (np.nan, np.inf, -np.inf):
        D = _sym(rng, 30)
        D[4, 17] = bad
        D[9, 20] = np.nan
        with pytest.raises(lib.AndiHipError, match=r"andi_hip_tree: D\[4\]\[17\] is not finite"):
            lib.tree(ctx, D, "bionj")
    D = _sym(rng, 30)
    want = bionj_model.bionj(D)
    D[np.arange(30), np.arange(30)] = np.nan  # the diagonal and the lower triangle are ignored
    D[20, 3] = np.inf
    _same(lib.tree(ctx, D, "bionj"), want)
    # in a batch the bad matrix is named, its records are zero bytes, and its neighbours are untouched
    n = 33
    Ds = np.stack([_sym(rng, n) for _ in range(5)])
    Ds[2, 7, 31] = np.inf
    Ds[2, 9, 10] = np.nan
    J, bad = lib.tree_batch(ctx, Ds, "bionj")
    assert bad.tolist() == [-1, -1, 7 * n + 31, -1, -1] and J[2].tobytes() == bytes(40 * (n - 2))
    for k in (0, 1, 3, 4):
        _same(J[k], bionj_model.bionj(Ds[k]))


# ------------------------------------------------------------------ 6: method "nj" is the neighbor-joining calls
def _models(seed, n, length=5000, div=(0.02, 0.3)):
    """an (n, n, 17) count matrix of n genomes of about `length` aligned positions at divergences within div"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n, 17), np.uint32)
    off = (np.ones((4, 4)) - np.eye(4)).reshape(-1) / 12
    for i in range(n):
        for j in range(n):
            if i == j:
                M[i, j, 0] = M[i, j, 16] = 1
                continue
            tot = float(M[j, i, :16].sum())
            d = rng.uniform(*div) if i < j else (tot - float(M[j, i, 0:16:5].sum())) / tot
            L = int(length * rng.uniform(0.8, 1.0))
            mism = rng.binomial(L, d)
            M[i, j, :16] = rng.multinomial(mism, off)
            M[i, j, 0:16:5] += rng.multinomial(L - mism, np.full(4, 0.25)).astype(np.uint32)
            M[i, j, 16] = length
    return M


@functools.lru_cache(maxsize=None)
def _models_65():
    return _models(65, 65)


def test_method_nj_is_the_neighbor_joining_calls(ctx):
    from andi_amd import lib
    n = 65
    Ds = np.stack([_sym(np.random.default_rng(650 + k), n) for k in range(4)])
    assert lib.tree(ctx, Ds[0], "nj").tobytes() == lib.nj(ctx, Ds[0]).tobytes() == lib.tree(ctx, Ds[0]).tobytes()
    J, bad = lib.tree_batch(ctx, Ds, "nj")
    wantJ, want_bad = lib.nj_batch(ctx, Ds)
    assert J.tobytes() == wantJ.tobytes() and bad.tolist() == want_bad.tolist()
    assert J[0].tobytes() != lib.tree(ctx, Ds[0], "bionj").tobytes()
    M = _models_65()
    J, bad, D = lib.bootstrap_tree(ctx, M, 4, lib.M_KIMURA, "nj", seed=SEED, distances=True)
    wantJ, want_bad, wantD = lib.bootstrap_nj(ctx, M, 4, lib.M_KIMURA, seed=SEED, distances=True)
    assert J.tobytes() == wantJ.tobytes() and bad.tolist() == want_bad.tolist() and D.tobytes() == wantD.tobytes()
    # a method out of range fails as a bad argument, with a context too
    L = lib.load()
    out = np.zeros(n - 2, lib.NJ_JOIN)
    for method in (-1, 2):
        assert L.andi_hip_tree(ctx._h, Ds[0].ctypes.data, n, method, out.ctypes.data) == 1
        assert b"andi_hip_tree: bad arguments" in L.andi_hip_last_error(ctx._h)


# ------------------------------------------------------------------ 7: batches and groups
def test_batch_is_the_single_call_whatever_the_groups(ctx):
    from andi_amd import lib
    n = 65
    Ds = np.stack([_sym(np.random.default_rng(700 + k), n) for k in range(7)])
    J, bad = lib.tree_batch(ctx, Ds, "bionj")
    assert (bad == -1).all()
    for k in range(7):
        assert J[k].tobytes() == lib.tree(ctx, Ds[k], "bionj").tobytes(), k
    _same(J[6], bionj_model.bionj(Ds[6]))
    with knobs(NJ_GROUP=3):  # groups of 3, 3 and 1
        J3, bad3 = lib.tree_batch(ctx, Ds, "bionj")
    assert J3.tobytes() == J.tobytes() and bad3.tolist() == bad.tolist()


# ------------------------------------------------------------------ 8: draw, estimate and join
@pytest.mark.parametrize("n", [5, 65])
def test_bootstrap_tree_is_tree_batch_on_its_distances(ctx, n):
    from andi_amd import lib
    M = _models_65() if n == 65 else _models(15, n)
    with knobs(NJ_GROUP=3):
        J, bad, D = lib.bootstrap_tree(ctx, M, 7, lib.M_KIMURA, "bionj", seed=SEED, distances=True)
        Ja, bada, Da = lib.bootstrap_tree(ctx, M, 3, lib.M_KIMURA, "bionj", seed=SEED, first=0, distances=True)
        Jb, badb, Db = lib.bootstrap_tree(ctx, M, 4, lib.M_KIMURA, "bionj", seed=SEED, first=3, distances=True)
    assert (bad == -1).all()
    wantJ, want_bad = lib.tree_batch(ctx, D, "bionj")
    assert J.tobytes() == wantJ.tobytes() and bad.tolist() == want_bad.tolist()
    assert np.concatenate([Ja, Jb]).tobytes() == J.tobytes()
    assert np.concatenate([Da, Db]).tobytes() == D.tobytes()
    assert np.concatenate([bada, badb]).tolist() == bad.tolist()
    # the distances are bootstrap_nj's: D receives D alone
    assert D.tobytes() == lib.bootstrap_nj(ctx, M, 7, lib.M_KIMURA, seed=SEED, distances=True)[2].tobytes()
    J2, bad2 = lib.bootstrap_tree(ctx, M, 7, lib.M_KIMURA, "bionj", seed=SEED)  # the default group, without the copy of D
    assert J2.tobytes() == J.tobytes() and bad2.tolist() == bad.tolist()
    _same(J[1], bionj_model.bionj(D[1]))


# ------------------------------------------------------------------ 9: determinism
def test_determinism(ctx):
    from andi_amd import lib
    D = _sym(np.random.default_rng(11), 300)
    a, b = lib.tree(ctx, D, "bionj"), lib.tree(ctx, D, "bionj")
    other = lib.Context(0)
    try:
        c = lib.tree(other, D, "bionj")
    finally:
        other.close()
    assert a.tobytes() == b.tobytes() == c.tobytes()


# ------------------------------------------------------------------ 10: the command line
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


def _table(names, moved, pairs):
    return "#name\tmoved\tindex\n" + "".join(
        "%s\t%d\t%s\n" % (name, int(m), "%.6g" % (int(m) / pairs) if pairs else "0") for name, m in zip(names, moved))


FILES = ("tree", "support", "consensus", "transfer", "rogues")


@pytest.mark.timeout(300)
def test_cli_tree_method(tmp_path, ctx):
    from andi_amd import lib, synth
    n = 8
    seqs, _ = synth.tree_set(n, 5000, seed=9)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))
    env.pop("ANDI_HIP_BOOT_CHUNK", None)

    def run(tag, args):
        paths = {k: str(tmp_path / ("%s_%s" % (tag, k))) for k in FILES}
        given = [k for k in FILES if k == "tree" or "-b" in args]
        p = subprocess.run([CLI, "-t", "4"] + args + ["--%s=%s" % (k, paths[k]) for k in given] + files, capture_output=True,
                           timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout, p.stderr, {k: open(paths[k]).read() for k in given}

    M = lib.dist_matrix(seqs, host_threads=4)
    D = lib.distances(M, lib.M_JC)
    J = lib.tree(ctx, D, "bionj")
    # --tree alone: the model's tree
    out, err, texts = run("point", ["--tree-method=bionj"])
    assert texts["tree"] == nj_model.newick(bionj_model.bionj(D), names) == lib.newick(J, names)
    assert (out, err) == run("plain", [])[:2]  # the matrix on stdout does not depend on the method

    def expected(R, bad):
        skip = (bad >= 0).astype(np.uint8)
        used = int((bad < 0).sum())
        assert used >= 1
        depth, transfer = lib.nj_transfer(ctx, J, R, skip=skip)
        moved, pairs = lib.nj_transfer_taxa(ctx, J, R, skip=skip, cutoff=0.3)
        ids, freq, sets = lib.nj_splits(ctx, R, skip=skip)
        return {"tree": lib.newick(J, names) + "".join(lib.newick(R[k], names) for k in range(len(R)) if bad[k] < 0),
                "support": lib.newick(J, names, support=lib.nj_support(ctx, J, R, skip=skip)),
                "consensus": lib.newick_consensus(lib.consensus(R, ids, freq, sets, skip=skip), names),
                "transfer": lib.newick_transfer(J, depth, transfer, used, names),
                "rogues": _table(names, moved, pairs)}

    # -b 5: four replicates as matrices, joined by tree_batch
    B = lib.bootstrap_range(ctx, M, 0, 4, seed=SEED)
    R, bad = lib.tree_batch(ctx, np.stack([lib.distances(B[k], lib.M_JC) for k in range(4)]), "bionj")
    _, _, texts = run("boot", ["-b", "5", "--tree-method=BioNJ"])
    assert texts == expected(R, bad)
    # ... and without matrices, through bootstrap_tree
    R, bad = lib.bootstrap_tree(ctx, M, 4, lib.M_JC, "bionj", seed=SEED)
    _, _, texts = run("only", ["-b", "5", "--trees-only", "--tree-method=bionj"])
    assert texts == expected(R, bad)
    # --tree-method=nj is a run without the option, byte for byte
    for tag, args in (("a", []), ("b", ["-b", "5"]), ("c", ["-b", "5", "--trees-only"])):
        assert run(tag + "_nj", args + ["--tree-method=nj"]) == run(tag + "_none", args), args
    # without a tree to build the option changes nothing and is no error
    p = subprocess.run([CLI, "-t", "4", "--tree-method=bionj"] + files, capture_output=True, timeout=120, env=env)
    q = subprocess.run([CLI, "-t", "4"] + files, capture_output=True, timeout=120, env=env)
    assert (p.returncode, p.stdout, p.stderr) == (q.returncode, q.stdout, q.stderr) and p.returncode == 0
