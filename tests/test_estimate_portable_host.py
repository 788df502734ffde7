"""The portable estimator on the host (andi_hip_estimate_portable, andi_amd/csrc/andi_estimate.h): bit for bit the NumPy
restatement of its contract (tests/estimate_model.py), and as close to andi_hip_estimate -- the same formulas on the
host's libm -- as one differing logarithm allows.  No GPU: the device's side of the same text is held to this function
in tests/test_bootstrap_trees_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import estimate_model as em
from conftest import ROOT

# The largest distances measured between the portable estimate and andi_hip_estimate over the sample below (glibc 2.35,
# x86-64): JC 2 ulp, Kimura 1 ulp, LogDet |delta d| = 8.9e-16 (at |d| of 0.5 ... 3; the sample's largest |d| is 10.9),
# andi_log against libm's log 1 ulp.  The tests assert TWICE that, since another machine's libm may round another way.
JC_ULP = 2 * 2
KIMURA_ULP = 2 * 1
LOGDET_ABS = 2 * 8.881784197001252e-16
LOG_ULP = 2 * 1


@pytest.fixture(scope="module")
def sample():
    s = em.sample_models()
    assert len(s) >= 100000
    return s


@pytest.fixture(scope="module")
def libm_estimates(sample):
    """andi_hip_estimate of every model of the sample, per model of evolution (one C call each: a handle of its own with
    plain pointer arguments)"""
    from andi_amd import lib
    lib.load()
    fn = C.CDLL(lib.LIB_PATH).andi_hip_estimate
    fn.restype, fn.argtypes = C.c_double, [C.c_void_p, C.c_int]
    base = sample.ctypes.data
    return {m: np.array([fn(base + 68 * k, m) for k in range(len(sample))]) for m in range(5)}


def test_sample_covers_the_edges(sample):
    c = sample[:, :16].astype(np.uint64)
    total = c.sum(axis=1)
    snps = total - (c[:, 0] + c[:, 5] + c[:, 10] + c[:, 15])
    assert ((snps == 0) & (total > 1000)).sum() >= 1000                        # identical genomes
    for t in range(5):
        assert (total == t).sum() >= 10                                        # totals 0 ... 4
    assert ((4 * snps == 3 * total) & (total > 3)).sum() >= 10                 # JC exactly at saturation
    assert ((4 * snps > 3 * total) & (total > 3)).sum() >= 1000                # ... and beyond
    assert (c.max(axis=1) >= 10 ** 8).sum() >= 1000                            # counts of 10^8


def test_edge_matrix_reaches_the_edges_under_the_oracles_draw(orc):
    """the design of tests/test_bootstrap_edges_gpu.py, verified without a GPU: forty replicates of edge_matrix drawn by
    the oracle -- another generator, the same multinomial law -- meet every coverage condition the GPU test asserts on the
    device's draw, and the host's estimate of them is the NumPy model bit for bit"""
    from andi_amd import lib
    M = em.edge_matrix(20240917)
    assert M.shape == (em.EDGE_N, em.EDGE_N, 17) and M.dtype == np.uint32
    summed = M[..., :16].astype(np.uint64) + M.transpose(1, 0, 2)[..., :16]
    assert summed.max() < 2 ** 31
    B = orc.bootstrap(M, em.EDGE_REPS, seed=20240917)
    fig = em.edge_coverage(B)
    print(fig)
    iu = np.triu_indices(em.EDGE_N, 1)
    m = em.doubled(B[:, iu[0], iu[1]])
    for model in range(5):
        assert em.same_bits(lib.estimate_portable(m, model), em.estimate_portable(m, model)).all(), model


@pytest.mark.parametrize("model", range(5))
def test_portable_estimate_is_the_numpy_model_bit_for_bit(sample, model):
    from andi_amd import lib
    got = lib.estimate_portable(sample, model)
    want = em.estimate_portable(sample, model)
    ok = em.same_bits(got, want)
    assert ok.all(), (int((~ok).sum()), sample[~ok][:3], got[~ok][:3], want[~ok][:3])
    assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("model", range(5))
def test_portable_estimate_against_libm(sample, libm_estimates, model):
    from andi_amd import lib
    got, ref = lib.estimate_portable(sample, model), libm_estimates[model]
    assert (np.isnan(got) == np.isnan(ref)).all()
    assert (np.isinf(got) == np.isinf(ref)).all() and (got[np.isinf(got)] == ref[np.isinf(ref)]).all()
    fin = np.isfinite(got)
    got, ref = got[fin], ref[fin]
    ulp, dist = em.ulp_distance(got, ref), np.abs(got - ref)
    print("model %d: %d finite, %.4f equal, worst %d ulp, worst |delta d| %.3g at |d| = %.3g, largest |d| %.3g"
          % (model, fin.sum(), (ulp == 0).mean(), ulp.max(), dist.max(), abs(ref[dist.argmax()]), np.abs(ref).max()))
    if model in (em.M_RAW, em.M_ANI):  # no logarithm: the same operations
        assert em.same_bits(got, ref).all()
    elif model == em.M_JC:
        assert ulp.max() <= JC_ULP
    elif model == em.M_KIMURA:
        assert ulp.max() <= KIMURA_ULP
    else:  # log(det) - lg/2 cancels for close genomes: a last-bit difference of one log is not small in ulps of d
        assert dist.max() <= LOGDET_ABS


def test_arguments():
    from andi_amd import lib
    L = lib.load()
    m = np.zeros((2, 17), np.uint32)
    out = np.full(2, 7.0)
    assert L.andi_hip_estimate_portable(m.ctypes.data, 2, 5, out.ctypes.data) == 1
    assert L.andi_hip_estimate_portable(m.ctypes.data, 2, -1, out.ctypes.data) == 1
    assert L.andi_hip_estimate_portable(None, 2, 1, out.ctypes.data) == 1
    assert L.andi_hip_estimate_portable(m.ctypes.data, 2, 1, None) == 1
    assert (out == 7.0).all()
    assert L.andi_hip_estimate_portable(None, 0, 1, None) == 0
    assert lib.estimate_portable(np.zeros((3, 4, 17), np.uint32), em.M_JC).shape == (3, 4)


HARNESS = r"""
#include <math.h>
#include <stddef.h>
#include "andi_estimate.h"
void portable_logs(const double *x, size_t n, double *out) { for (size_t k = 0; k < n; k++) out[k] = andi_log(x[k]); }
void libm_logs(const double *x, size_t n, double *out) { for (size_t k = 0; k < n; k++) out[k] = log(x[k]); }
"""


def test_andi_log_alone(tmp_path):
    """the header as strict C99 with gcc, without contraction: andi_log on subnormals, powers of two, 1.0 and its
    neighbours, the special values -- bit for bit the NumPy model, and within LOG_ULP of libm's log"""
    src = tmp_path / "harness.c"
    src.write_text(HARNESS)
    so = tmp_path / "harness.so"
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "andi_amd", "csrc"), str(src), "-o", str(so),
                    "-lm"], check=True)
    H = C.CDLL(str(so))
    x = em.sample_log_arguments()
    got, ref = np.empty_like(x), np.empty_like(x)
    H.portable_logs(C.c_void_p(x.ctypes.data), C.c_size_t(len(x)), C.c_void_p(got.ctypes.data))
    H.libm_logs(C.c_void_p(x.ctypes.data), C.c_size_t(len(x)), C.c_void_p(ref.ctypes.data))
    assert em.same_bits(got, em.andi_log(x)).all()

    def one(v):
        a, r = np.array([v], np.float64), np.empty(1)
        H.portable_logs(C.c_void_p(a.ctypes.data), C.c_size_t(1), C.c_void_p(r.ctypes.data))
        return r[0]
    assert one(1.0) == 0.0 and not np.signbit(one(1.0))
    assert one(0.0) == -np.inf and one(-0.0) == -np.inf and one(np.inf) == np.inf
    assert np.isnan(one(-1.0)) and np.isnan(one(-np.inf)) and np.isnan(one(np.nan)) and np.isnan(one(-5e-324))
    assert abs(one(5e-324) - -744.4400719213812) < 1e-12  # the least subnormal
    assert one(np.nextafter(1.0, 0.0)) < 0.0 < one(np.nextafter(1.0, 2.0))
    assert one(2.0) == 0.6931471805599453 and one(0.5) == -0.6931471805599453  # ln2_hi + ln2_lo: ln 2, rounded

    pos = x > 0
    assert (np.isnan(got) == np.isnan(ref)).all() and (np.isinf(got) == np.isinf(ref)).all()
    fin = pos & np.isfinite(x)
    ulp = em.ulp_distance(got[fin], ref[fin])
    print("andi_log: %d arguments, %.4f equal to libm, worst %d ulp" % (fin.sum(), (ulp == 0).mean(), ulp.max()))
    assert ulp.max() <= LOG_ULP
