"""andi_hip_complete on the MI355X: bit for bit the NumPy restatement (tests/complete_model.py) -- the completed matrix as
bytes and every fill with its round and its quartets -- at the smallest shapes that reach each path of
andi_amd/csrc/complete.hip: one candidate, none, the edges of a wavefront, of a block's stride and of the LDS chunk, a
row's partners shared by a block, a second round, a batch under every grouping; and the tree of a completed matrix."""
import os
import re

import numpy as np
import pytest

import complete_model as cm
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "andi_amd", "csrc", "complete.hip")).read()
CH = int(re.search(r"constexpr int CH = (\d+);", _SRC).group(1))  # the kernel's chunk of columns
P = int(re.search(r"constexpr int P = (\d+);", _SRC).group(1))  # the partners of a row that a block serves


def _same(ctx, D, max_rounds=0):
    from andi_amd import lib
    C, fills = lib.complete(ctx, D, max_rounds)
    wC, wfills = cm.complete(D, max_rounds)
    assert fills.dtype == wfills.dtype and fills.shape == wfills.shape
    for f in ("i", "j", "round", "pad", "quartets"):
        assert (fills[f] == wfills[f]).all(), f
    assert fills.tobytes() == wfills.tobytes()
    assert C.tobytes() == wC.tobytes()
    return wC, wfills


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _hole(D, i, j, v=np.nan):
    D[i, j] = D[j, i] = v


# ------------------------------------------------- n = 4
def test_four_leaves():
    from andi_amd import lib
    ctx = lib.Context(0)
    try:
        rng = np.random.default_rng(4)
        D = _sym(rng, 4)
        _hole(D, 0, 1)
        _, fills = _same(ctx, D)
        assert len(fills) == 1 and fills[0]["round"] == 1 and fills[0]["quartets"] == 1
        _hole(D, 2, 3)
        _, fills = _same(ctx, D)
        assert len(fills) == 2 and (fills["round"] == 0).all()
        # nothing missing: the input mirrored, whatever is below the diagonal and on it
        D = np.triu(_sym(rng, 4), 1) + np.tril(rng.uniform(-5, 5, (4, 4)))
        D[1, 0] = np.nan
        C, fills = _same(ctx, D)
        assert len(fills) == 0 and (C == C.T).all() and (np.diag(C) == 0).all()
        for n in (2, 3):  # never a candidate
            D = _sym(rng, n)
            _hole(D, 0, 1)
            _same(ctx, D)
    finally:
        ctx.close()


# ------------------------------------------------- the edges of a wavefront and of the block's stride
@pytest.mark.parametrize("common", [63, 64, 65, 255, 256, 257])
def test_wavefront_and_block_edges(ctx, common):
    n = common + 2
    rng = np.random.default_rng(common)
    D = _sym(rng, n, 0.5, 1.0)
    sprinkle = np.triu(rng.random((n, n)) < 120.0 / (n * n), 1)  # some sixty missing D[k][l]
    sprinkle[:2, :] = False  # rows 0 and 1 know every column: `common` common columns
    D[sprinkle | sprinkle.T] = np.nan
    _hole(D, 0, 1)
    wC, fills = _same(ctx, D)
    first = fills[0]
    assert (first["i"], first["j"], first["round"]) == (0, 1, 1)
    assert first["quartets"] == common * (common - 1) // 2 - int(sprinkle.sum())


# ------------------------------------------------- the edges of the LDS chunk
@pytest.mark.parametrize("n", [CH - 1, CH, CH + 1, CH + 2, CH + 3, 2 * CH, 2 * CH + 1, 2 * CH + 3])
def test_chunk_edges(ctx, n):
    """CH - 1, CH, CH + 1 and 2 CH + 1 common columns are n - 2 of them; the chunks themselves end at multiples of CH"""
    rng = np.random.default_rng(n)
    D = _sym(rng, n, 0.5, 1.0)
    _hole(D, 0, 1)
    _hole(D, 7, n - 1, np.inf)
    c = min(CH, n - 2)
    _hole(D, c - 1, c, -np.inf)  # a pair across the first chunk's end, and a missing D[k][l] of the others
    _, fills = _same(ctx, D)
    assert len(fills) == 3 and (fills["round"] == 1).all()
    assert (fills["quartets"] == (n - 2) * (n - 3) // 2 - 2).all()


# ------------------------------------------------- one row's partners shared by a block
@pytest.mark.parametrize("partners", sorted({1, P - 1, P, P + 1, 2 * P + 1} - {0}))
def test_partners_of_one_row(ctx, partners):
    n = 41
    rng = np.random.default_rng(partners)
    D = _sym(rng, n, 0.5, 1.0)
    row = 3
    js = [5, 6, 9, 17, 18, 19, 30, 38, 40][:partners]
    for q, j in enumerate(js):
        _hole(D, row, j)
        for k in rng.choice([k for k in range(n) if k not in (row, j, 20)], 2 + q, replace=False):
            if k not in js:
                _hole(D, min(j, int(k)), max(j, int(k)))  # partner q knows its own set of columns
    for k in range(n):
        if k != 20:
            _hole(D, 20, k, (np.nan, np.inf, -np.inf)[k % 3])  # a row without a known entry stays missing
    _, fills = _same(ctx, D)
    r20 = fills[(fills["i"] == 20) | (fills["j"] == 20)]
    assert len(r20) == n - 1 and (r20["round"] == 0).all() and (r20["quartets"] == 0).all()
    mine = fills[(fills["i"] == row) & np.isin(fills["j"], js)]
    assert len(mine) == partners and (mine["round"] == 1).all()


# ------------------------------------------------- a second round, a tie, the clamp, the three spellings
def _second_round_case():
    rng = np.random.default_rng(1)  # (three rounds)
    n = 12
    A = np.triu(rng.integers(0, 4, (n, n)).astype(float), 1)
    D = A + A.T
    holes = np.argwhere(np.triu(rng.random((n, n)) < 0.5, 1))
    for x, (i, j) in enumerate(holes):
        _hole(D, i, j, (np.nan, np.inf, -np.inf)[x % 3])
    return D


def test_second_round(ctx):
    D = _second_round_case()
    M = cm.mirrored(D)
    _, fills = _same(ctx, D)
    # what the case is there for, by the model
    assert (fills["round"] >= 2).any() and (fills["round"] == 1).any()
    clamped = tied = 0
    for f in fills[fills["round"] == 1]:
        i, j = int(f["i"]), int(f["j"])
        cands = [max(M[i, k] + M[j, l], M[i, l] + M[j, k]) - M[k, l] for k in range(12) for l in range(k + 1, 12)
                 if not {k, l} & {i, j} and np.isfinite([M[i, k], M[i, l], M[j, k], M[j, l], M[k, l]]).all()]
        assert len(cands) == f["quartets"]
        clamped += min(cands) < 0 and f["value"] == 0 and not np.signbit(f["value"])
        tied += cands.count(min(cands)) >= 2
    assert clamped and tied
    _, fills1 = _same(ctx, D, max_rounds=1)
    assert (fills1["round"] <= 1).all() and (fills1["round"] == 0).sum() > (fills["round"] == 0).sum()
    _same(ctx, D, max_rounds=2)


# ------------------------------------------------- a batch
def _batch():
    n = 33
    rng = np.random.default_rng(8)
    Ds = np.stack([_sym(rng, n, 0.5, 1.0) for _ in range(5)])
    holes = np.triu(rng.random((n, n)) < 0.2, 1)
    Ds[0][holes | holes.T] = np.nan
    # Ds[1] is complete
    Ds[2][:] = np.inf  # unfillable: one known pair
    Ds[2][0, 1] = 0.25
    Ds[3][:] = np.nan  # every pair missing
    holes = np.triu(rng.random((n, n)) < 0.7, 1)  # needs more than one round
    Ds[4][holes | holes.T] = -np.inf
    return Ds


def test_batch_is_the_single_calls_under_every_grouping(ctx):
    from andi_amd import lib
    Ds = _batch()
    n = Ds.shape[1]
    singles = [lib.complete(ctx, D) for D in Ds]
    want = [cm.complete(D) for D in Ds]
    assert max(f["round"].max() for _, f in want if len(f)) >= 2
    for (C, f), (wC, wf) in zip(singles, want):
        assert C.tobytes() == wC.tobytes() and f.tobytes() == wf.tobytes()
    assert len(singles[1][1]) == 0 and (singles[2][1]["round"] == 0).all() and (singles[3][1]["round"] == 0).all()
    assert len(singles[3][1]) == n * (n - 1) // 2

    def check():
        Cs, missing, left = lib.complete_batch(ctx, Ds)
        for k, (C, f) in enumerate(singles):
            assert Cs[k].tobytes() == C.tobytes(), k
            assert missing[k] == len(f) and left[k] == (f["round"] == 0).sum(), k
        Cs1, _, left1 = lib.complete_batch(ctx, Ds, max_rounds=1)
        for k, D in enumerate(Ds):
            C1, f1 = lib.complete(ctx, D, max_rounds=1)
            assert Cs1[k].tobytes() == C1.tobytes() and left1[k] == (f1["round"] == 0).sum(), k

    check()
    for group in (1, 2, 3):
        with knobs(NJ_GROUP=group):
            check()


def test_batch_in_place(ctx):
    from andi_amd import lib
    Ds = _batch()
    want = lib.complete_batch(ctx, Ds)[0]
    buf = Ds.copy()
    missing, left = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    assert lib.load().andi_hip_complete_batch(ctx._h, buf.ctypes.data, Ds.shape[1], 5, 0, buf.ctypes.data, missing.ctypes.data,
                                              left.ctypes.data) == 0
    assert buf.tobytes() == want.tobytes()


def test_fills_up_to_cap(ctx):
    import ctypes as C
    from andi_amd import lib
    D = _batch()[0]
    n = D.shape[0]
    _, want = lib.complete(ctx, D)
    out = np.empty((n, n))
    for cap in (0, 1, len(want) - 1, len(want) + 3):
        fills = np.zeros(cap + 1, lib.FILL)
        fills["pad"] = 77  # (what lies behind cap is not written)
        m, l = C.c_size_t(0), C.c_size_t(0)
        assert lib.load().andi_hip_complete(ctx._h, D.ctypes.data, n, 0, out.ctypes.data, fills.ctypes.data if cap else None, cap,
                                            C.byref(m), C.byref(l)) == 0
        took = min(cap, len(want))
        assert m.value == len(want) and l.value == (want["round"] == 0).sum()
        assert fills[:took].tobytes() == want[:took].tobytes() and (fills[took:]["pad"] == 77).all()


# ------------------------------------------------- end to end: the tree of a completed matrix
def test_tree_of_a_completed_additive_matrix(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(40)
    T = cm.additive(rng, 40)
    D = cm.punch(rng, T, 0.06)
    for i, j in np.argwhere(np.triu(np.isnan(D), 1)):  # a hole that no known quartet separates (a cherry, say) is given back
        if not cm.separated(T, cm.mirrored(D), int(i), int(j)):
            D[i, j] = D[j, i] = T[i, j]
    M = cm.mirrored(D)
    I, J = np.nonzero(np.triu(np.isnan(M), 1))
    assert len(I) >= 20 and all(cm.separated(T, M, int(i), int(j)) for i, j in zip(I, J))
    wC, _ = cm.complete(D)
    assert (wC == T).all()
    C, _ = lib.complete(ctx, D)
    assert C.tobytes() == wC.tobytes()
    for method in ("nj", "bionj"):
        assert lib.tree(ctx, C, method).tobytes() == lib.tree(ctx, T, method).tobytes()
