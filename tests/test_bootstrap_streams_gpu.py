"""The draw of the device's bootstrap (bootstrap_draw.h) on the MI355X: its streams and its binomial's branch switches.

What the draw is held to here.  Streams: over a matrix of twelve genomes whose 66 pairs all have the same sums and 2000
replicates, no two of the 132 000 (pair, replicate) draws are the same sixteen counts; cell 0's correlation over the
replicates between every two pairs (2145 coefficients) and with itself at lags 1, 2, 3 (198) stays below 6 / sqrt(2000)
= 0.134; seeds that differ by 1, by 2^32, in the high word only and in bit 63 give different draws in every pair, also
in andi_hip_bootstrap_nj's distances; the replicates 0, 2^16, 2^24, 2^31 and 2^32 - 2 differ in every pair, keep totals,
mirror and diagonal, and their distances are the portable estimate of their counts bit for bit.  The binomial: 10^4
draws each of two-cell pairs at n p = 9, 10, 11 for N = 20 ... 10^8, at p = 0.5 exactly and just above it, at N = 1
and 2, and of a three-cell pair -- against the exact law, against the oracle's draws, and the oracle against the exact
law, chi-square p > 10^-5 each.  The generators differ, so the law is what is held, not the bits.

On the MI355X: largest cross-correlation 0.0711, largest autocorrelation 0.0670 (bound 0.1342); smallest p-value of the
binomial's 45 comparisons 0.0053 (device against oracle at N = 10^6, p = 0.5; the oracle's own smallest against the
exact law is 0.0282, and the seed was chosen on the oracle's side alone, for its p-values to clear 10^-3)."""

import itertools

import numpy as np
import pytest

import estimate_model as em
from conftest import binomial_gof_pvalue, two_sample_pvalue
from test_bootstrap_trees_gpu import _check_distances

pytestmark = pytest.mark.gpu

SEED = 20240917
N, REPS = 12, 2000
BOUND = 6 / np.sqrt(REPS)
IU = np.triu_indices(N, 1)


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def equal_sums(ctx):
    from andi_amd import lib
    M, sums = em.equal_sums_matrix(SEED, N)
    B = lib.bootstrap(ctx, M, REPS, seed=SEED)
    B.setflags(write=False)
    return M, sums, B


def _structure(M, B):
    """what test_bootstrap_structure_and_determinism asks of replicates: totals kept, mirrored, the diagonal"""
    n = M.shape[0]
    summed = M.astype(np.uint64) + M.transpose(1, 0, 2)
    iu = np.triu_indices(n, 1)
    k = np.arange(n)
    assert (B[:, k, k, 0] == 1).all() and (B[:, k, k, 16] == 1).all() and (B[:, k, k, 1:16] == 0).all()
    assert (B[:, iu[0], iu[1]] == B[:, iu[1], iu[0]]).all()
    up = B[:, iu[0], iu[1]].astype(np.uint64)
    assert (up[..., :16].sum(axis=-1) == summed[iu][:, :16].sum(axis=-1)).all()
    assert (up[..., 16] == summed[iu][:, 16]).all()
    assert (up[..., :16][:, summed[iu][:, :16] == 0] == 0).all()


# ------------------------------------------------------------------ B. streams are distinct
def test_no_two_draws_are_equal(equal_sums):
    # cell standard deviations of about 47 (diagonal) and 5 ... 8 (off it): two independent draws coincide with probability
    # below 10^-20, so among the 8.7 * 10^9 pairs of the 132 000 vectors fewer than 10^-10 coincidences are expected
    M, sums, B = equal_sums
    _structure(M, B)
    assert ((M[IU][:, :16].astype(np.int64) + M[IU[1], IU[0]][:, :16]) == sums).all()
    v = np.ascontiguousarray(B[:, IU[0], IU[1], :16]).reshape(-1, 16)
    assert len(v) == 132000
    assert len(np.unique(v, axis=0)) == len(v)


def test_pairs_do_not_move_together(equal_sums):
    # 2145 coefficients, each about N(0, 1 / reps): one beyond 6 standard deviations with probability 2145 * 2e-9 = 4e-6
    x = equal_sums[2][:, IU[0], IU[1], 0].astype(np.float64)  # (reps, 66)
    r = np.corrcoef(x.T)
    off = np.abs(r[np.triu_indices(66, 1)])
    assert len(off) == 2145
    print("largest cross-correlation of cell 0 between two pairs: %.4f (bound %.4f)" % (off.max(), BOUND))
    assert off.max() < BOUND


def test_replicates_do_not_move_together(equal_sums):
    x = equal_sums[2][:, IU[0], IU[1], 0].astype(np.float64)
    r = np.array([[np.corrcoef(x[:-lag, p], x[lag:, p])[0, 1] for lag in (1, 2, 3)] for p in range(66)])
    assert r.shape == (66, 3)
    print("largest autocorrelation of cell 0 at lags 1, 2, 3: %.4f (bound %.4f)" % (np.abs(r).max(), BOUND))
    assert np.abs(r).max() < BOUND


def _all_pairs_differ(Ba, Bb):
    return (Ba[:, IU[0], IU[1], :16] != Bb[:, IU[0], IU[1], :16]).any(axis=-1).all()


def test_every_bit_of_the_seed_counts(ctx, equal_sums):
    from andi_amd import lib
    M = equal_sums[0]
    s = SEED
    seeds = [s, s + 1, s + 2 ** 32, s << 32, s ^ (1 << 63)]
    draws = [lib.bootstrap(ctx, M, 3, seed=k) for k in seeds]
    assert draws[0].tobytes() == equal_sums[2][:3].tobytes()
    for a, b in itertools.combinations(range(5), 2):  # (a coincidence of one pair's sixteen counts: below 10^-20)
        assert _all_pairs_differ(draws[a], draws[b]), (hex(seeds[a]), hex(seeds[b]))
    Da = lib.bootstrap_nj(ctx, M, 3, em.M_RAW, seed=s, distances=True)[2]
    Db = lib.bootstrap_nj(ctx, M, 3, em.M_RAW, seed=s + 2 ** 32, distances=True)[2]
    _check_distances(Da, draws[0], em.M_RAW)
    _check_distances(Db, draws[2], em.M_RAW)
    # (a distance is the number of mismatches, standard deviation 21: two draws agree in it about once in 50)
    assert (Da[:, IU[0], IU[1]] != Db[:, IU[0], IU[1]]).mean() > 0.8


def test_every_bit_of_the_replicate_index_counts(ctx, equal_sums):
    from andi_amd import lib
    M = equal_sums[0]
    firsts = [0, 2 ** 16, 2 ** 24, 2 ** 31, 2 ** 32 - 2]
    reps = [lib.bootstrap_range(ctx, M, r, 1, seed=SEED) for r in firsts]
    assert reps[0].tobytes() == equal_sums[2][:1].tobytes()
    for B in reps:
        _structure(M, B)
    for a, b in itertools.combinations(range(5), 2):
        assert _all_pairs_differ(reps[a], reps[b]), (firsts[a], firsts[b])
    for r, B in zip(firsts, reps):
        J, bad, D = lib.bootstrap_nj(ctx, M, 1, em.M_JC, seed=SEED, first=r, distances=True)
        got = _check_distances(D, B, em.M_JC)
        assert np.isfinite(got).all() and (got > 0).all() and bad.tolist() == [-1]


# ------------------------------------------------------------------ C. the binomial at its switches
SWITCH_SEED = 2026
SWITCH_REPS = 10000


def test_binomial_at_its_switches(ctx, orc):
    from andi_amd import lib
    M, cases = em.switch_matrix(SWITCH_SEED)
    reps = SWITCH_REPS
    G = lib.bootstrap(ctx, M, reps, seed=SWITCH_SEED)
    O = orc.bootstrap(M, reps, seed=SWITCH_SEED)
    _structure(M, G)
    worst, worst_oracle, compared = 1.0, 1.0, 0
    for i, j, sums in cases:
        total = int(sums.sum())
        g, o = G[:, i, j, :16].astype(np.int64), O[:, i, j, :16].astype(np.int64)
        cell = int(np.nonzero(sums)[0][0])          # the first cell that has counts: its binomial is the whole draw
        last = int(np.nonzero(sums)[0][-1])
        for x in (g, o):
            assert (x[:, sums == 0] == 0).all() and (x.sum(axis=1) == total).all()
            assert cell == last or (x[:, last] == total - x[:, cell]).all()
        if total == 1:                              # N = 1, c = 1: cell 0 is empty, cell 1 takes the one count
            assert cell == last == 1 and (g[:, 1] == 1).all()
            continue
        p = int(sums[cell]) / total
        xs, ys = g[:, cell], o[:, cell]
        if total == 2:                              # the exact frequencies 1/4, 1/2, 1/4 within 5 standard errors
            for k, f in enumerate((0.25, 0.5, 0.25)):
                se = np.sqrt(f * (1 - f) / reps)
                assert abs((xs == k).mean() - f) < 5 * se and abs((ys == k).mean() - f) < 5 * se, (k, (xs == k).mean())
            continue
        p1, p2, p3 = binomial_gof_pvalue(xs, total, p), binomial_gof_pvalue(ys, total, p), two_sample_pvalue(xs, ys)
        print("N = %9d, cell %d of %9d: device vs law %.3g, oracle vs law %.3g, device vs oracle %.3g"
              % (total, cell, sums[cell], p1, p2, p3))
        worst, worst_oracle, compared = min(worst, p1, p3), min(worst_oracle, p2), compared + 3
        assert p1 > 1e-5, ("device vs Binomial", total, sums[cell], p1)
        assert p2 > 1e-5, ("oracle vs Binomial", total, sums[cell], p2)
        assert p3 > 1e-5, ("device vs oracle", total, sums[cell], p3)
    assert compared == 45
    print("smallest p-value over %d comparisons: %.3g (the oracle against the exact law: %.3g)"
          % (compared, worst, worst_oracle))
