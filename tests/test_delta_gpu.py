"""andi_hip_delta_scores on the MI355X: bit for bit the NumPy restatement (tests/delta_model.py) at the smallest shapes that
reach each path of andi_amd/csrc/delta.hip: no quartet, one, the edges of a wavefront and of the block's stride, the edges
of the LDS chunk in every role (i, j in one chunk, k in the next, l in the third), a row cut into several items by work and
by the cap on an item's partners, an item of a single partner, and the accumulators cleared between calls.

Measured GPU time of each case (the call with its copies, one MI355X; the model's time on the host is not in it):
  test_two_to_five_leaves, test_n_out_of_range...   below 0.1 ms a call
  test_wavefront_edges                   0.6 ms at n = 63 ... 66, 0.7 ms at 129 and 130 (their models: 0.1 and 0.7 s)
  test_chunk_edges                       91 ms at CH - 1 and CH, 133 ms at CH + 1 and CH + 3; three calls each (0.6 - 0.7 s a case)
  test_three_chunks                      1.49 s at 2 CH + 1 = 2049: 7.3e11 quartets at 4.9e11 a second (3.1 s with its model)
  test_items_cut_by_the_cap_on_partners  6 ms at n = 2600: nearly every pair is missing, the blocks only walk their partners
  test_twice_on_one_context              1.0 ms a call at n = 200
The whole module: 8 s.
"""
import os
import re
from math import comb

import numpy as np
import pytest

import delta_model as dm
from conftest import ROOT

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "andi_amd", "csrc", "delta.hip")).read()
CH = int(re.search(r"constexpr int CH = (\d+);", _SRC).group(1))  # the kernel's chunk of columns
JMAX = int(re.search(r"constexpr int JMAX = (\d+);", _SRC).group(1))  # the most partners of one item
MINW = int(re.search(r"constexpr uint64_t MINW = (\d+);", _SRC).group(1))  # an item's least target of quartets
NITEMS = int(re.search(r"constexpr uint64_t NITEMS = (\d+);", _SRC).group(1))  # target = max(MINW, quartets / NITEMS)


def _row_items(n, i):
    """the items of row i as delta.hip's cut_items cuts them: [j0, j1) each"""
    target = max(MINW, comb(n, 4) // NITEMS)
    out, j0, acc = [], i + 1, 0
    for j in range(i + 1, n - 2):
        acc += comb(n - 1 - j, 2)
        if acc >= target or j + 1 - j0 == JMAX or j + 3 == n:
            out.append((j0, j + 1))
            j0, acc = j + 1, 0
    return out


def _sym(rng, n, lo=0.5, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _set(D, i, j, v):
    D[i, j] = D[j, i] = v


def _punch(rng, D, frac):
    n = D.shape[0]
    hole = np.triu(rng.random((n, n)) < frac, 1)
    D[hole | hole.T] = np.nan
    return D


def _equal(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert (got["quartets"] == want["quartets"]).all()
    assert (got["sum"] == want["sum"]).all()
    assert got.tobytes() == want.tobytes()


def _same(ctx, D):
    from andi_amd import lib
    want = dm.scores(D)
    _equal(lib.delta_scores(ctx, D), want)
    return want


# ------------------------------------------------- n = 2 ... 5
def test_two_to_five_leaves(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(5)
    for n in (2, 3):
        assert lib.delta_scores(ctx, _sym(rng, n)).tobytes() == np.zeros(n, dm.DELTA).tobytes()
    D = _sym(rng, 4)
    want = _same(ctx, D)
    assert (want["quartets"] == 1).all() and len(set(want["sum"].tolist())) == 1
    D[np.tril_indices(4)] = np.nan  # only the upper triangle is read
    _equal(lib.delta_scores(ctx, D), want)
    _set(D, 1, 3, -np.inf)
    assert lib.delta_scores(ctx, D).tobytes() == np.zeros(4, dm.DELTA).tobytes()
    D = _sym(rng, 5, -1.0, 1.0)
    want = _same(ctx, D)
    assert (want["quartets"] == 4).all()
    _set(D, 0, 4, np.inf)
    want = _same(ctx, D)
    assert want["quartets"].tolist() == [1, 2, 2, 2, 1]
    _set(D, 0, 4, 1e308)  # a sum that overflows: its quartets are not used either
    _set(D, 1, 2, 1e308)
    assert _same(ctx, D)["quartets"].tolist() == [3, 3, 3, 4, 3]


# ------------------------------------------------- the edges of a lane's stride and of a wavefront's
@pytest.mark.parametrize("n,holes", [(63, True), (64, True), (65, True), (66, True), (66, False), (129, True), (130, True)])
def test_wavefront_edges(ctx, n, holes):
    rng = np.random.default_rng(n)
    D = _sym(rng, n)
    if holes:
        _punch(rng, D, 0.05)
        dead = n // 3
        D[dead, :] = D[:, dead] = np.nan  # a genome without a distance: in no quartet
    want = _same(ctx, D)
    if holes:
        assert want[dead]["quartets"] == 0 and want[dead]["sum"] == 0
        assert 0 < int(want["quartets"].sum()) // 4 < comb(n - 1, 4)
    else:
        assert (want["quartets"] == comb(n - 1, 3)).all()
    assert int(want["quartets"].sum()) % 4 == 0
    if n == 130:
        assert len(_row_items(n, 0)) >= 3  # row 0's partners are the work of at least three blocks


# ------------------------------------------------- the edges of the LDS chunk
def _background(n, long_pairs, missing):
    D = np.ones((n, n))
    for (p, q), v in long_pairs.items():
        _set(D, p, q, v)
    for p, q in missing:
        _set(D, p, q, np.nan)
    return D, dm.with_background(D, list(long_pairs) + list(missing))


@pytest.mark.parametrize("n", [CH - 1, CH, CH + 1, CH + 3])
def test_chunk_edges(ctx, n):
    from andi_amd import lib
    c = min(CH, n - 2)  # the first chunk's end, or (one chunk) two columns before the matrix's
    D, want = _background(n, {(c - 1, c): 2.0, (n - 3, n - 1): 1.5, (0, n - 1): 1.25}, [(c - 2, c + 1), (1, n - 2)])
    assert want["sum"].all() and (want["quartets"] < comb(n - 1, 3)).all()
    _equal(lib.delta_scores(ctx, D), want)
    # noise on every pair: the records follow a permutation of the genomes
    rng = np.random.default_rng(n)
    D = _punch(rng, _sym(rng, n), 0.01)
    perm = rng.permutation(n)
    got = lib.delta_scores(ctx, D)
    _equal(lib.delta_scores(ctx, D[np.ix_(perm, perm)]), got[perm])
    assert int(got["quartets"].sum()) % 4 == 0 and got["sum"].all()
    m = dm.mean(got)
    assert ((m > 0) & (m < 1)).all()


def test_three_chunks(ctx):
    """2 CH + 1 columns: i and j in chunk 0, k in chunk 1, l in chunk 2 (and every other split of a quartet over them)"""
    from andi_amd import lib
    n = 2 * CH + 1
    long_pairs = {(5, 9): 2.0, (3, CH + 476): 1.5, (7, n - 1): 1.25, (CH + 5, n - 1): 1.75}
    D, want = _background(n, long_pairs, [(9, CH + 6), (CH + 76, n - 1)])
    assert want["sum"].all()
    _equal(lib.delta_scores(ctx, D), want)


# ------------------------------------------------- the cap on an item's partners
def test_items_cut_by_the_cap_on_partners(ctx):
    """n so large that rows of little work have more than JMAX partners: such a row's items end at the cap.  All but a few
    genomes have no distance at all, so the quartets are those of the few -- spread over the capped rows, their items' ends
    and the chunks.  The row with JMAX + 1 partners ends in an item of a single j"""
    from andi_amd import lib
    n = 2600
    target = max(MINW, comb(n, 4) // NITEMS)
    capped = [i for i in range(n - 3 - JMAX) if comb(n - 1 - i, 3) - comb(n - 1 - i - JMAX, 3) < target]
    assert len(capped) > 40
    i0, i1 = capped[0], capped[len(capped) // 2]
    assert _row_items(n, i0)[0] == (i0 + 1, i0 + 1 + JMAX) and len(_row_items(n, i0)) >= 2
    one = n - 4 - JMAX
    assert one in capped and _row_items(n, one) == [(one + 1, n - 3), (n - 3, n - 2)]
    keep = sorted({0, 1, 600, one - 1, one, one + 1, one + 500, CH - 1, CH, i0 - 1, i0, i0 + 1, i0 + 2, i1, i1 + 1, i0 + JMAX - 1, i0 + JMAX, i0 + JMAX + 1, i0 + JMAX + 2,
                   i1 + JMAX, i1 + JMAX + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1, n - 3, n - 2, n - 1}
                  | set(range(i1 + 400, i1 + 412)) | set(range(n - 30, n - 24)))
    rng = np.random.default_rng(n)
    S = _punch(rng, _sym(rng, len(keep)), 0.02)
    D = np.full((n, n), np.nan)
    D[np.ix_(keep, keep)] = S
    want = np.zeros(n, dm.DELTA)
    want[keep] = dm.scores(S)
    assert want["quartets"][keep].all()
    _equal(lib.delta_scores(ctx, D), want)


# ------------------------------------------------- the accumulators are cleared
def test_twice_on_one_context(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(77)
    D = _punch(rng, _sym(rng, 200), 0.02)
    first = lib.delta_scores(ctx, D)
    assert first["sum"].all()
    assert lib.delta_scores(ctx, D).tobytes() == first.tobytes()
    E = _sym(rng, 70)
    _same(ctx, E)
    assert lib.delta_scores(ctx, D).tobytes() == first.tobytes()


# ------------------------------------------------- the range of n, behind a real context
def test_n_out_of_range_is_refused_with_the_contexts_error(ctx):
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((4, 4))
    out = np.zeros(4, lib.DELTA)
    out["sum"], out["quartets"] = 7, 9
    before = out.tobytes()
    for args in [(ctx._h, D.ctypes.data, 1, out.ctypes.data), (ctx._h, D.ctypes.data, 0, out.ctypes.data),
                 (ctx._h, D.ctypes.data, 16385, out.ctypes.data), (ctx._h, None, 4, out.ctypes.data),
                 (ctx._h, D.ctypes.data, 4, None)]:
        assert L.andi_hip_delta_scores(*args) == 1, args
        assert b"andi_hip_delta_scores: bad arguments" in L.andi_hip_last_error(ctx._h) and b"2 <= n <= 16384" in L.andi_hip_last_error(ctx._h)
        assert out.tobytes() == before  # nothing was written
    with pytest.raises(lib.AndiHipError):
        lib.delta_scores(ctx, np.zeros((1, 1)))
    _same(ctx, _sym(np.random.default_rng(1), 6))  # the context goes on working
