"""andi_hip_linkage on the MI355X: bit-exact to the NumPy restatement (tests/linkage_model.py) for the three methods on
random matrices, on ties (where a neighbour cache goes wrong), past 1024 active rows, with pairs without a distance, a
-inf, overflow of the average rule, in batches, on scanned genomes, and andi-hip --dendrogram / --clusters."""
import os
import subprocess

import numpy as np
import pytest

import linkage_model as lm
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
    assert got.shape == want.shape
    for f in ("a", "b", "size", "pad"):
        assert (got[f] == want[f]).all(), f
    assert (got["height"].view(np.uint64) == want["height"].view(np.uint64)).all(), "height"


def _same_but_nan(got, want):
    """a NaN height (inf - inf on the device) only has to be a NaN: its bits are the platform's"""
    for f in ("a", "b", "size", "pad"):
        assert (got[f] == want[f]).all(), f
    g, w = got["height"], want["height"]
    assert (np.isnan(g) == np.isnan(w)).all()
    ok = ~np.isnan(w)
    assert (g[ok].view(np.uint64) == w[ok].view(np.uint64)).all(), "height"


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


@pytest.mark.parametrize("method", lm.METHODS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 257])
def test_bit_exact_on_random_matrices(ctx, n, method):
    from andi_amd import lib
    for seed in (1, 2):
        rng = np.random.default_rng(1000 * n + seed)
        D = _sym(rng, n)
        if seed == 2:  # junk in the lower triangle and on the diagonal: not read
            D = np.triu(D, 1) + np.tril(rng.uniform(-5, 5, (n, n)))
            D[0, 0] = np.nan
        _same(lib.linkage(ctx, D, method), lm.linkage(D, method))


def test_bit_exact_past_1024_active_rows(ctx):
    from andi_amd import lib
    n = 1100
    D = _sym(np.random.default_rng(77), n)
    Z = lib.linkage(ctx, D, "average")
    _same(Z[:100], lm.linkage(D, "average", steps=100))
    # the whole run is a tree over every leaf, its sizes those of its children
    size = np.r_[np.ones(n, np.int64), Z["size"]]
    assert sorted(np.r_[Z["a"], Z["b"]].tolist()) == list(range(2 * n - 2))
    assert (Z["size"] == size[Z["a"]] + size[Z["b"]]).all() and Z["size"][-1] == n
    assert (Z["a"] < Z["b"]).all()


def _tie_cases():
    rng = np.random.default_rng(5)
    cases = [np.ones((9, 9)) - np.eye(9), 0.25 * (np.ones((40, 40)) - np.eye(40))]
    for n in (6, 23, 70):  # small integers: many exact ties
        A = np.triu(rng.integers(0, 4, (n, n)).astype(float), 1)
        cases.append(A + A.T)
    # duplicated rows: the distance between duplicates alternates +0.0 and -0.0
    base = _sym(rng, 12)
    idx = np.array([0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 11])
    dup = base[np.ix_(idx, idx)]
    for i in range(len(idx)):
        for j in range(len(idx)):
            if i != j and idx[i] == idx[j]:
                dup[i, j] = -0.0 if (i + j) % 2 else 0.0
    cases.append(dup)
    # the tie a cache without rescans gets wrong under single linkage (tests/test_linkage_host.py)
    cases.append(np.array([[0, 1, 1, 0.5], [0, 0, 1, 2], [0, 0, 0, 2], [0, 0, 0, 0]], float))
    return cases


@pytest.mark.parametrize("method", lm.METHODS)
def test_ties(ctx, method):
    from andi_amd import lib
    for D in _tie_cases():
        _same(lib.linkage(ctx, D, method), lm.linkage(D, method))


def _two_groups(between):
    rng = np.random.default_rng(14)
    D = _sym(rng, 16, 0.01, 0.2)
    group = np.array([0] * 7 + [1] * 9)[rng.permutation(16)]
    D[group[:, None] != group[None, :]] = between
    return D, group


@pytest.mark.parametrize("method", lm.METHODS)
def test_pairs_without_a_distance(ctx, method):
    from andi_amd import lib
    D, group = _two_groups(np.nan)
    E, _ = _two_groups(np.inf)
    Z = lib.linkage(ctx, D, method)
    _same(Z, lib.linkage(ctx, E, method))
    _same(Z, lm.linkage(D, method))
    assert Z["height"][-1] == np.inf and np.isfinite(Z["height"][:-1]).all()
    for t in (0.0, 0.1, 0.2, 1e300, np.finfo(float).max):  # any finite threshold keeps the groups apart
        labels = lib.linkage_cut(Z, t)
        assert not (labels[group == 0][:, None] == labels[group == 1][None, :]).any(), t
    top = lib.linkage_cut(Z, np.finfo(float).max)
    assert len(set(top.tolist())) == 2 and (top == (group != group[0])).all()
    assert lib.newick_linkage(Z, ["g%d" % i for i in range(16)]) == ""  # (its root's branches are not finite)


def test_minus_inf_fails_names_its_entry_and_writes_nothing(ctx):
    from andi_amd import lib
    D = _sym(np.random.default_rng(9), 30)
    D[4, 17] = -np.inf
    D[9, 20] = -np.inf
    D[2, 3] = np.nan
    with pytest.raises(lib.AndiHipError, match=r"D\[4\]\[17\] is -inf"):
        lib.linkage(ctx, D, "average")
    Z = np.full(29, 0x7f, np.uint8).repeat(24).view(lib.LINK)
    before = Z.tobytes()
    assert lib.load().andi_hip_linkage(ctx._h, D.ctypes.data, 30, 2, Z.ctypes.data) == 1
    assert Z.tobytes() == before
    D[4, 17] = D[9, 20] = 0.5
    D[20, 9] = D[17, 17] = -np.inf  # the lower triangle and the diagonal are not read
    _same(lib.linkage(ctx, D, "complete"), lm.linkage(D, "complete"))


def test_overflow_of_the_average_rule(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(3)
    D = np.full((12, 12), 1e308)
    D[:6, :6] = _sym(rng, 6)
    D[6:, 6:] = _sym(rng, 6)
    Z = lib.linkage(ctx, D, "average")
    _same(Z, lm.linkage(D, "average"))
    assert Z["height"][-1] == np.inf  # ((3 * 1e308 + 3 * 1e308) overflows on the way to the root)
    # and where the overflow goes both ways, inf - inf: a NaN orders after every number
    big = -1.6e308
    E = np.array([[0, -1.7e308, big, big], [0, 0, big, big], [0, 0, 0, np.inf], [0, 0, 0, 0]])
    Z = lib.linkage(ctx, E, "average")
    _same_but_nan(Z, lm.linkage(E, "average"))
    assert np.isnan(Z["height"][-1]) and Z["height"][1] == -np.inf


def test_batch(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(41)
    n = 65
    Ds = np.stack([_sym(rng, n), _sym(rng, n), np.zeros((n, n)), _sym(rng, n), _sym(rng, n)])
    A = np.triu(rng.integers(0, 3, (n, n)).astype(float), 1)
    Ds[2] = A + A.T  # ties
    group = rng.integers(0, 3, n)
    Ds[3][group[:, None] != group[None, :]] = np.nan  # blocks without a distance
    Ds[4][7, 31] = -np.inf
    Ds[4][30, 40] = -np.inf
    for method in lm.METHODS:
        Z, bad = lib.linkage_batch(ctx, Ds, method)
        assert bad.tolist() == [-1, -1, -1, -1, 7 * n + 31]
        for k in range(4):
            _same(Z[k], lib.linkage(ctx, Ds[k], method))
            _same(Z[k], lm.linkage(Ds[k], method))
        assert Z[4].tobytes() == bytes(24 * (n - 1))
        Z2, bad2 = lib.linkage_batch(ctx, Ds, method)
        assert Z2.tobytes() == Z.tobytes() and (bad2 == bad).all()
    # the grouping does not matter (a test hook of the suite's library: groups of two)
    from conftest import knobs
    want, _ = lib.linkage_batch(ctx, Ds, "average")
    with knobs(NJ_GROUP=2):
        got, bad = lib.linkage_batch(ctx, Ds, "average")
    assert got.tobytes() == want.tobytes() and bad.tolist() == [-1, -1, -1, -1, 7 * n + 31]


def test_scanned_genomes_give_the_generating_clades(ctx):
    from andi_amd import lib, synth
    n = 12
    seqs, expected = synth.tree_set(n, 50_000, seed=31)
    D = lib.distances(lib.dist_matrix(seqs, model=lib.M_JC, host_threads=8), lib.M_JC)
    # the clades of the generating tree at the widest gap of its heights, and a threshold in the middle of that gap
    heights = np.unique(expected[np.triu_indices(n, 1)])
    gap = int(np.argmax(heights[1:] / heights[:-1]))
    t = float(np.sqrt(heights[gap] * heights[gap + 1]))
    clades = lm.cut(lm.linkage(expected, "average"), t)
    assert 1 < len(set(clades.tolist())) < n
    for method in lm.METHODS:
        Z = lib.linkage(ctx, D, method)
        _same(Z, lm.linkage(D, method))
        assert (lib.linkage_cut(Z, t) == clades).all(), method


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.mark.timeout(900)
def test_cli_dendrogram_and_clusters(tmp_path, ctx):
    from andi_amd import lib, synth
    n, N, seed, t = 8, 5, 4242, 0.004
    seqs, _ = synth.tree_set(n, 40_000, seed=77)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    base = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(seed))
    dend, clus = str(tmp_path / "d.nwk"), str(tmp_path / "c.tsv")

    def run(args, env=base):
        p = subprocess.run([CLI, "-t", "4"] + args, capture_output=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    M = lib.dist_matrix(seqs, model=lib.M_JC, host_threads=4)
    B = lib.bootstrap_range(ctx, M, 0, N - 1, seed=seed)
    D = lib.distances(M, lib.M_JC)
    Ds = np.stack([lib.distances(B[k], lib.M_JC) for k in range(N - 1)])
    plain = run(["-b", str(N)] + files)
    for method in lm.METHODS:
        Z = lib.linkage(ctx, D, method)
        Zs, bad = lib.linkage_batch(ctx, Ds, method)
        assert (bad == -1).all()
        labels = lib.linkage_cut(Z, t)
        medoid = lib.cluster_medoids(D, labels)
        stab = lib.cluster_stability(labels, np.stack([lib.linkage_cut(Zk, t) for Zk in Zs]))
        want_d = "".join(lib.newick_linkage(z, names) for z in [Z] + list(Zs))
        want_c = "#name\tcluster\trepresentative\tstability\n" + "".join(
            "%s\t%d\t%s\t%d\n" % (names[i], labels[i] + 1, names[medoid[labels[i]]], stab[labels[i]]) for i in range(n))
        assert 1 < len(set(labels.tolist())) < n and want_d.count("\n") == N
        for env in (base, dict(base, ANDI_HIP_BOOT_CHUNK="2")):
            out = run(["-b", str(N), "--linkage=" + method, "--dendrogram=" + dend, "--clusters=" + clus, "--threshold=%r" % t]
                      + files, env)
            assert out == plain
            assert open(dend).read() == want_d, method
            assert open(clus).read() == want_c, method
    # the default is average linkage; without -b there is no fourth column
    run(["--dendrogram=" + dend, "--clusters=" + clus, "--threshold=%r" % t] + files)
    assert open(dend).read() == lib.newick_linkage(lib.linkage(ctx, D, "average"), names)
    labels = lib.linkage_cut(lib.linkage(ctx, D, "average"), t)
    medoid = lib.cluster_medoids(D, labels)
    assert open(clus).read() == "#name\tcluster\trepresentative\n" + "".join(
        "%s\t%d\t%s\n" % (names[i], labels[i] + 1, names[medoid[labels[i]]]) for i in range(n))
    # --tree and --support keep their bytes beside the new options
    tree, sup = str(tmp_path / "t.nwk"), str(tmp_path / "s.nwk")
    out = run(["-b", str(N), "--tree=" + tree, "--support=" + sup] + files)
    assert out == plain
    before = open(tree).read(), open(sup).read()
    out = run(["-b", str(N), "--tree=" + tree, "--support=" + sup, "--dendrogram=" + dend, "--clusters=" + clus, "--threshold=%r" % t]
              + files)
    assert out == plain and (open(tree).read(), open(sup).read()) == before
