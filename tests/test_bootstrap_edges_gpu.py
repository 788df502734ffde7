"""The device's side of the bootstrap at the estimator's edges and at larger n, on the MI355X.

What the device's portable estimator (andi_estimate.h inside k_bootstrap_dist) is held to here: bit for bit the host's
andi_hip_estimate_portable -- itself the NumPy model bit for bit over 120 000 models -- on forty replicates of
estimate_model.edge_matrix, all five models of evolution: identical genomes (snps == 0: JC and Kimura +0.0 by the bits,
LogDet +0.0 or a few units of 2^-52, never -0.0), the doubled totals 0 2 4 6 8 around nucl <= 3, log(0) at JC's exact
saturation (+inf) and NaN beyond it, Kimura's argument at 0 and below it, LogDet with a nucleotide that never occurs
(-inf - -inf), with a negative determinant and with a determinant of exactly 0, the cancellation of close genomes at
counts of 10^8 and 4 * 10^8.  The test first asserts, on the drawn counts, that the draw reached every one of these
(estimate_model.edge_coverage; tests/test_estimate_portable_host.py asserts the same of the oracle's draw without a GPU).

k_bootstrap_dist's unranking t -> (i, j) (a sqrt estimate and two correcting loops) against k_bootstrap's other formula
at n = 257 and n = 700 (129 and 956 blocks of pairs), with the replicate index through blockIdx.y (the default group)
and through rep0 (ANDI_NJ_GROUP=1)."""

import numpy as np
import pytest

import estimate_model as em
from conftest import knobs
from test_bootstrap_trees_gpu import _check_distances

pytestmark = pytest.mark.gpu

SEED = 20240917


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge(ctx):
    """edge_matrix, its forty replicates as andi_hip_bootstrap draws them, and the proof that they reach the edges"""
    from andi_amd import lib
    M = em.edge_matrix(SEED)
    B = lib.bootstrap(ctx, M, em.EDGE_REPS, seed=SEED)
    fig = em.edge_coverage(B)  # conditions on the drawn counts, asserted before any distance of the device is looked at
    print("coverage of the device's draw:", fig)
    return M, B


@pytest.mark.parametrize("model", range(5))
def test_estimator_at_the_edges(ctx, edge, model):
    from andi_amd import lib
    M, B = edge
    n, count = em.EDGE_N, em.EDGE_REPS
    J, bad, D = lib.bootstrap_nj(ctx, M, count, model, seed=SEED, distances=True)
    assert D.shape == (count, n, n) and bad.shape == (count,)
    got = _check_distances(D, B, model)  # bit for bit; NaN where the host has NaN; mirrored; +0.0 on the diagonal
    # (the records of these replicates, nearly all bad, are not this test's subject) bad[k]: the first pair without a
    # finite distance, or -1
    iu = np.triu_indices(n, 1)
    nonfinite = ~np.isfinite(got)
    for k in range(count):
        want = -1
        if nonfinite[k].any():
            first = int(np.argmax(nonfinite[k]))
            want = int(iu[0][first]) * n + int(iu[1][first])
        assert bad[k] == want, (k, bad[k], want)
    assert (bad != -1).any()


@pytest.mark.parametrize("group", [None, 1])
@pytest.mark.parametrize("n", [257, 700])
def test_unranking_at_larger_n(ctx, n, group):
    from andi_amd import lib
    M = em.models_matrix(n, n)
    B = lib.bootstrap(ctx, M, 2, seed=SEED)
    with knobs(NJ_GROUP=group):
        J, bad, D = lib.bootstrap_nj(ctx, M, 2, em.M_RAW, seed=SEED, distances=True)
    got = _check_distances(D, B, em.M_RAW)
    assert (bad == -1).all() and np.isfinite(got).all()
    assert (got[0] != got[1]).mean() > 0.99  # two replicates, not one twice
