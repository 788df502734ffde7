"""Bootstrap trees without matrices on the MI355X: andi_hip_bootstrap_range against the stream andi_hip_bootstrap draws,
and andi_hip_bootstrap_nj -- draw, estimate and join on the device -- against the pieces it replaces: its distances bit for
bit the portable estimate (host) of the counts andi_hip_bootstrap draws, doubled; its records bit for bit those of
andi_hip_nj_batch on those distances, across group boundaries and split ranges; bad replicates; arguments."""

import numpy as np
import pytest

import estimate_model as em
from conftest import knobs

pytestmark = pytest.mark.gpu

SEED = 20240917


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _models(seed, n, length=20000, div=(0.02, 0.3)):
    """an (n, n, 17) count matrix of n genomes of about `length` aligned positions at divergences within div; the two
    directions of a pair differ a little, as a scan's do"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n, 17), np.uint32)
    base = np.full(4, 0.25)
    off = (np.ones((4, 4)) - np.eye(4)).reshape(-1) / 12
    for i in range(n):
        for j in range(n):
            if i == j:
                M[i, j, 0] = M[i, j, 16] = 1
                continue
            d = rng.uniform(*div) if i < j else None
            if i > j:
                d = float(M[j, i, :16].sum() - M[j, i, 0:16:5].sum()) / float(M[j, i, :16].sum())
            L = int(length * rng.uniform(0.8, 1.0))
            mism = rng.binomial(L, d)
            M[i, j, :16] = rng.multinomial(mism, off)
            M[i, j, 0:16:5] += rng.multinomial(L - mism, base).astype(np.uint32)
            M[i, j, 16] = length
    return M


def _tiny_pair(M, i, j):
    """pair (i, j) with twelve counts in all: every binomial of its draw takes the waiting-time branch"""
    M[i, j, :16] = M[j, i, :16] = 0
    for a, b in ((i, j), (j, i)):
        M[a, b, 0], M[a, b, 5], M[a, b, 1] = 3, 2, 1
    return M


def _doubled(B):
    """what andi_hip_model_average makes of a mirrored replicate: every count twice (32-bit)"""
    d = B.copy()
    d[..., :16] = B[..., :16] + B[..., :16]
    return d


def _check_distances(D, B, model):
    from andi_amd import lib
    count, n = D.shape[0], D.shape[1]
    want = lib.estimate_portable(_doubled(B), model)  # (count, n, n)
    iu = np.triu_indices(n, 1)
    got_u, want_u = D[:, iu[0], iu[1]], want[:, iu[0], iu[1]]
    ok = em.same_bits(got_u, want_u)
    assert ok.all(), (model, int((~ok).sum()), got_u[~ok][:3], want_u[~ok][:3])
    assert (np.ascontiguousarray(D[:, iu[1], iu[0]]).view(np.uint64) == np.ascontiguousarray(got_u).view(np.uint64)).all()  # mirrored
    k = np.arange(n)
    assert (np.ascontiguousarray(D[:, k, k]).view(np.uint64) == 0).all()  # +0.0
    return got_u


# ------------------------------------------------------------------ ranges of replicates
def test_range_is_a_slice_of_the_stream(ctx):
    from andi_amd import lib
    M = _tiny_pair(_models(1, 6), 1, 4)
    whole = lib.bootstrap(ctx, M, 7, seed=SEED)
    part = lib.bootstrap_range(ctx, M, 3, 4, seed=SEED)
    assert part.shape == (4, 6, 6, 17) and part.tobytes() == whole[3:7].tobytes()
    assert lib.bootstrap_range(ctx, M, 0, 7, seed=SEED).tobytes() == whole.tobytes()
    assert whole[3].tobytes() != whole[4].tobytes()
    # count = 0: nothing is written, nothing fails
    B = np.full((1, 6, 6, 17), 7, np.uint32)
    L = lib.load()
    assert L.andi_hip_bootstrap_range(ctx._h, M.ctypes.data, 6, SEED, 3, 0, B.ctypes.data) == 0
    assert (B == 7).all()
    # first + count must fit 32 bits
    assert L.andi_hip_bootstrap_range(ctx._h, M.ctypes.data, 6, SEED, 2 ** 32 - 1, 1, B.ctypes.data) == 1
    assert b"andi_hip_bootstrap_range" in L.andi_hip_last_error(ctx._h)
    assert (B == 7).all()


# ------------------------------------------------------------------ the distances
@pytest.mark.parametrize("model", range(5))
def test_distances_are_the_portable_estimate_of_the_drawn_counts(ctx, model):
    from andi_amd import lib
    n, count = 6, 40
    M = _tiny_pair(_models(2, n), 0, 3)
    B = lib.bootstrap(ctx, M, count, seed=SEED)
    J, bad, D = lib.bootstrap_nj(ctx, M, count, model, seed=SEED, distances=True)
    assert D.shape == (count, n, n) and J.shape == (count, n - 2) and bad.shape == (count,)
    got = _check_distances(D, B, model)
    tiny = D[:, 0, 3]
    if model != em.M_LOGDET:  # (two nucleotides never occur in the tiny pair: no LogDet distance)
        assert len(set(tiny.tolist())) > 3                   # the tiny pair is drawn anew in every replicate
    assert np.isfinite(got).sum() > got.size // 2            # ... and the test is not about NaN alone


# ------------------------------------------------------------------ the records
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_records_equal_nj_batch_on_the_distances(ctx, n):
    from andi_amd import lib
    M = _models(10 + n, n)
    J, bad, D = lib.bootstrap_nj(ctx, M, 6, em.M_JC, seed=SEED, distances=True)
    _check_distances(D, lib.bootstrap(ctx, M, 6, seed=SEED), em.M_JC)
    wantJ, want_bad = lib.nj_batch(ctx, D)
    assert (bad == -1).all() and bad.tolist() == want_bad.tolist()
    assert J.shape == (6, 1 if n == 2 else n - 2) and J.tobytes() == wantJ.tobytes()
    J2, bad2 = lib.bootstrap_nj(ctx, M, 6, em.M_JC, seed=SEED)  # without the copy of D
    assert J2.tobytes() == J.tobytes() and bad2.tolist() == bad.tolist()


def test_records_across_group_boundaries_and_split_ranges(ctx):
    # n = 65: one past the 64 x 64 argmin tile, 2080 pairs (nine blocks of k_bootstrap_dist); groups of 3, 3 and 1
    from andi_amd import lib
    n = 65
    M = _models(65, n, length=5000)
    B = lib.bootstrap(ctx, M, 7, seed=SEED)
    with knobs(NJ_GROUP=3):
        J, bad, D = lib.bootstrap_nj(ctx, M, 7, em.M_KIMURA, seed=SEED, distances=True)
        Ja, bada, Da = lib.bootstrap_nj(ctx, M, 3, em.M_KIMURA, seed=SEED, first=0, distances=True)
        Jb, badb, Db = lib.bootstrap_nj(ctx, M, 4, em.M_KIMURA, seed=SEED, first=3, distances=True)
    _check_distances(D, B, em.M_KIMURA)
    assert (bad == -1).all()
    wantJ, want_bad = lib.nj_batch(ctx, D)
    assert J.tobytes() == wantJ.tobytes() and bad.tolist() == want_bad.tolist()
    assert np.concatenate([Ja, Jb]).tobytes() == J.tobytes()
    assert np.concatenate([Da, Db]).tobytes() == D.tobytes()
    assert np.concatenate([bada, badb]).tolist() == bad.tolist()
    whole, whole_bad = lib.bootstrap_nj(ctx, M, 7, em.M_KIMURA, seed=SEED)  # the default group: all seven at once
    assert whole.tobytes() == J.tobytes() and whole_bad.tolist() == bad.tolist()
    assert J[0].tobytes() != J[1].tobytes()


# ------------------------------------------------------------------ bad replicates
def test_bad_replicates(ctx):
    from andi_amd import lib
    n, count = 5, 40
    M = _models(5, n)
    # pair (1, 3): 40 counts, 29 of them mismatches -- a replicate with 30 or more (p >= 0.75) has no JC distance
    M[1, 3, :16] = M[3, 1, :16] = 0
    M[1, 3, 0], M[1, 3, 5], M[1, 3, 1], M[1, 3, 6] = 3, 2, 8, 7
    M[3, 1, 10], M[3, 1, 15], M[3, 1, 11], M[3, 1, 2] = 3, 3, 7, 7
    J, bad, D = lib.bootstrap_nj(ctx, M, count, em.M_JC, seed=SEED, distances=True)
    _check_distances(D, lib.bootstrap(ctx, M, count, seed=SEED), em.M_JC)
    good = bad == -1
    assert 0 < good.sum() < count, bad.tolist()  # (each saturates with probability 0.4: all 40 of one kind is below 1e-8)
    iu = np.triu_indices(n, 1)
    for k in range(count):
        nonfinite = ~np.isfinite(D[k][iu])
        if good[k]:
            assert not nonfinite.any()
        else:
            first = int(np.argmax(nonfinite))
            assert nonfinite.any() and bad[k] == iu[0][first] * n + iu[1][first] == 1 * n + 3
            assert J[k].tobytes() == bytes(J[k].nbytes)
    wantJ, want_bad = lib.nj_batch(ctx, D)
    assert want_bad.tolist() == bad.tolist() and J.tobytes() == wantJ.tobytes()
    assert J[good].tobytes() == lib.nj_batch(ctx, D[good])[0].tobytes()


# ------------------------------------------------------------------ arguments
def test_arguments_fail_before_any_work(ctx):
    from andi_amd import lib
    L = lib.load()
    n = 4
    M = _models(4, n)
    J = np.zeros((2, n - 2), lib.NJ_JOIN)
    bad = np.full(2, 99, np.int64)

    def call(ctx_h=ctx._h, M_p=M.ctypes.data, n_=n, model=1, first=0, count=2, J_p=J.ctypes.data, bad_p=bad.ctypes.data):
        return L.andi_hip_bootstrap_nj(ctx_h, M_p, n_, model, SEED, first, count, J_p, bad_p, None)

    for kw in (dict(M_p=None), dict(J_p=None), dict(bad_p=None), dict(count=0), dict(n_=1), dict(n_=65536), dict(model=5),
               dict(model=-1), dict(first=2 ** 32 - 2)):
        L.andi_hip_sync(ctx._h)
        assert call(**kw) == 1, kw
        assert b"andi_hip_bootstrap_nj: bad arguments" in L.andi_hip_last_error(ctx._h), kw
    assert call(ctx_h=None) == 1
    assert (bad == 99).all() and J.tobytes() == bytes(J.nbytes)
    assert call() == 0 and (bad == -1).all()
