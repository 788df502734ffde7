"""Tree-likeness scores from all quartets, what needs no GPU: the contract's NumPy restatement (tests/delta_model.py) equals
its own plain four loops at the contract's edges (missing pairs in each spelling, negative entries, an overflowing sum), is
0 on additive matrices, has the closed form of one perturbed pair on the all-ones matrix, and follows a permutation of the
genomes; the symbol, the argument checks and the command line's option."""
import ctypes as C
import os
import re
import subprocess
from math import comb

import numpy as np
import pytest

import complete_model as cm
import delta_model as dm
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
ONE = 1 << 24


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _set(D, i, j, v):
    D[i, j] = D[j, i] = v


def _same(a, b):
    assert a.dtype == dm.DELTA and b.dtype == dm.DELTA
    assert (a["quartets"] == b["quartets"]).all() and (a["sum"] == b["sum"]).all()


# ------------------------------------------------- the vectorised model is the four loops
@pytest.mark.parametrize("n", range(4, 10))
def test_model_equals_the_four_loops(n):
    rng = np.random.default_rng(n)
    D = _sym(rng, n)
    full = dm.scores(D)
    _same(full, dm.scores_loops(D))
    assert (full["quartets"] == comb(n - 1, 3)).all() and full["sum"].any()
    for miss in (np.nan, np.inf, -np.inf):  # the three spellings of a missing pair: the same records
        H = D.copy()
        _set(H, 0, n - 1, miss)
        _set(H, 1, 2, miss)
        got = dm.scores(H)
        _same(got, dm.scores_loops(H))
        if miss is np.nan:
            first = got
        _same(got, first)
    # genome 0 loses the C(n - 2, 2) quartets with n - 1 and the n - 4 that hold 1 and 2 but not n - 1
    assert first["quartets"][0] == comb(n - 1, 3) - comb(n - 2, 2) - (n - 4)
    N = _sym(rng, n, -1.0, 1.0)  # negative entries are known
    _same(dm.scores(N), dm.scores_loops(N))
    assert (dm.scores(N)["quartets"] == comb(n - 1, 3)).all()
    O = D.copy()
    _set(O, 0, 1, 1e308)  # with (2, 3) at 1e308 too, d(0,1) + d(2,3) overflows: that quartet is not used
    _set(O, 2, 3, 1e308)
    got = dm.scores(O)
    _same(got, dm.scores_loops(O))
    assert got["quartets"][0] == comb(n - 1, 3) - 1 and got["quartets"][3] == comb(n - 1, 3) - 1
    if n > 4:
        assert got["quartets"][4] == comb(n - 1, 3)


def test_one_quartet():
    D = np.zeros((4, 4))
    for (i, j), v in {(0, 1): 1.0, (2, 3): 1.0, (0, 2): 2.0, (1, 3): 1.0, (0, 3): 1.5, (1, 2): 1.0}.items():
        D[i, j] = v  # the upper triangle alone is read
    D[3, 0] = np.nan
    got = dm.scores(D)  # sums 2, 3, 2.5: delta = 0.5
    assert (got["sum"] == ONE // 2).all() and (got["quartets"] == 1).all()
    for n in (2, 3):
        assert dm.scores(np.ones((n, n))).tobytes() == np.zeros(n, dm.DELTA).tobytes()


# ------------------------------------------------- additive distances: delta is 0
@pytest.mark.parametrize("seed", range(4))
def test_additive_matrices_score_zero(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 20))
    got = dm.scores(cm.additive(rng, n))  # dyadic branch lengths: every sum is exact, the two largest are equal
    assert (got["sum"] == 0).all() and (got["quartets"] == comb(n - 1, 3)).all()


# ------------------------------------------------- the all-ones matrix with one pair at 2
@pytest.mark.parametrize("n,p,q", [(6, 0, 1), (9, 2, 7), (13, 12, 4)])
def test_one_long_pair_on_the_all_ones_matrix(n, p, q):
    D = np.ones((n, n))
    _set(D, p, q, 2.0)  # {p, q, x, y}: sums 3, 2, 2: delta = 1
    got = dm.scores(D)
    assert (got["quartets"] == comb(n - 1, 3)).all()
    for x in range(n):
        assert got["sum"][x] == (comb(n - 2, 2) if x in (p, q) else n - 3) * ONE
    _same(dm.with_background(D, [(p, q)]), got)
    r = next(x for x in range(n) if x not in (p, q))
    _set(D, p, r, 1.5)  # {p, q, r, x}: sums 3, 2.5, 2: delta = 0.5
    got = dm.scores(D)
    _same(dm.with_background(D, [(p, q), (p, r)]), got)
    x = next(x for x in range(n) if x not in (p, q, r))
    assert dm.quartet(dm.mirrored(D), p, q, r, x) == (True, ONE // 2)
    _set(D, q, r, np.nan)  # and a missing pair: its quartets are not used
    _same(dm.with_background(D, [(p, q), (p, r), (q, r)]), dm.scores(D))


# ------------------------------------------------- permuting the genomes permutes the records
@pytest.mark.parametrize("seed", range(3))
def test_records_follow_a_permutation(seed):
    rng = np.random.default_rng(50 + seed)
    n = 11
    D = _sym(rng, n)
    _set(D, 1, 5, np.nan)
    _set(D, 0, 9, np.inf)
    got = dm.scores(D)
    perm = rng.permutation(n)
    _same(dm.scores(D[np.ix_(perm, perm)]), got[perm])
    assert int(got["quartets"].sum()) % 4 == 0
    assert 0 < int(got["quartets"].sum()) // 4 < comb(n, 4)
    m = dm.mean(got)
    assert ((m >= 0) & (m <= 1)).all()


# ------------------------------------------------- the C-ABI
def test_symbol_is_declared_and_exported():
    from andi_amd import lib
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    L = lib.load()
    assert re.search(r"^int andi_hip_delta_scores\(andi_hip_ctx \*ctx, const double \*D, size_t n, andi_hip_delta \*out", header, re.M)
    assert hasattr(L, "andi_hip_delta_scores")
    assert "} andi_hip_delta;" in header
    assert re.search(r"#define ANDI_HIP_ABI_VERSION 5\b", header) and L.andi_hip_abi_version() == 5
    assert lib.DELTA.itemsize == 16 and lib.DELTA == dm.DELTA
    import andi_amd
    assert andi_amd.delta_scores is lib.delta_scores and andi_amd.DELTA is lib.DELTA


def test_delta_scores_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((4, 4))
    out = np.zeros(4, lib.DELTA)
    d, o = D.ctypes.data, out.ctypes.data
    # with no context nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, d, 4, o), (None, None, 4, o), (None, d, 4, None), (None, d, 1, o), (None, d, 16385, o), (None, d, 0, o)]:
        assert L.andi_hip_delta_scores(*args) == 1, args
    assert C.sizeof(C.c_uint64) * 2 == lib.DELTA.itemsize


# ------------------------------------------------- the command line's validation (no GPU is reached)
def test_cli_lists_the_new_option():
    p = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and "--delta=FILE" in p.stdout.decode()


@pytest.mark.parametrize("option", ["--reference=g0.fa", "--reference-list=refs.txt"])
def test_cli_refuses_delta_with_references(tmp_path, option):
    files = []
    for k in range(2):
        path = tmp_path / ("g%d.fa" % k)
        path.write_text(">g%d\nACGTACGTTGCA\n" % k)
        files.append(str(path))
    (tmp_path / "refs.txt").write_text("g0.fa\n")
    p = subprocess.run([CLI, "--delta=F", option, files[1]], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.decode().strip() == ("andi-hip: Tree-likeness scores (--delta) are not available together with --reference or "
                                         "--reference-list.")
    assert not os.path.exists(tmp_path / "F")  # refused before a file is opened
