"""NumPy restatement of the portable estimator (include/andi_hip.h: andi_hip_estimate_portable and the contract of
andi_log), written from the header.  Elementwise float64 ufuncs round every operation on its own and never fuse a product
into a sum, which is what the contract asks of the C text on the host and on the device.  The tests hold the library to
this, bit for bit."""
import numpy as np

M_RAW, M_JC, M_KIMURA, M_LOGDET, M_ANI = range(5)

_MANT = np.uint64(0x000FFFFFFFFFFFFF)
_ONE = np.uint64(0x3FF0000000000000)
_SQRT2 = 1.4142135623730951
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def andi_log(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    shape = x.shape
    x = x.reshape(-1)
    with np.errstate(all="ignore"):
        sub = (x.view(np.uint64) >> np.uint64(52)) == 0  # (of a positive x: the others are replaced below)
        xs = np.where(sub, x * 18014398509481984.0, x)
        b = np.ascontiguousarray(xs).view(np.uint64)
        k = np.where(sub, -54, 0).astype(np.int64) + ((b >> np.uint64(52)).astype(np.int64) - 1023)
        m = ((b & _MANT) | _ONE).view(np.float64)
        big = m > _SQRT2
        m = np.where(big, m * 0.5, m)
        k = k + big
        f = m - 1.0
        s = f / (2.0 + f)
        z = s * s
        p = np.zeros_like(z)
        for i in range(27, 1, -2):
            p = p * z + 1.0 / i
        hfsq = (0.5 * f) * f
        R = (2.0 * z) * p
        t = s * (hfsq + R)
        dk = k.astype(np.float64)
        r = np.where(k == 0, f - (hfsq - t), dk * _LN2_HI - ((hfsq - (t + dk * _LN2_LO)) - f))
        r = np.where(x == np.inf, np.inf, r)
        r = np.where(x == 0.0, -np.inf, r)
        r = np.where(x > 0.0, r, np.where(x == 0.0, -np.inf, NAN))
    return r.reshape(shape)


def _counts(models):
    c = np.asarray(models, dtype=np.uint32)[..., :16].astype(np.uint64)
    return c.reshape(-1, 16)


def _total(c):
    return c.sum(axis=1, dtype=np.uint64)


def _off_diagonal(c):
    return _total(c) - (c[:, 0] + c[:, 5] + c[:, 10] + c[:, 15])


def _clamp(d):
    with np.errstate(invalid="ignore"):
        return np.where(d <= 0.0, 0.0, d)


def raw(c):
    nucl, snps = _total(c), _off_diagonal(c)
    with np.errstate(all="ignore"):
        return np.where(nucl <= 3, NAN, snps.astype(np.float64) / nucl.astype(np.float64))


def jc(c):
    with np.errstate(all="ignore"):
        return _clamp(-0.75 * andi_log(1.0 - (4.0 / 3.0) * raw(c)))


def kimura(c):
    nucl = _total(c)
    ts = c[:, 2] + c[:, 8] + c[:, 7] + c[:, 13]  # A>G, G>A, C>T, T>C
    tv = _off_diagonal(c) - ts
    with np.errstate(all="ignore"):
        P = ts.astype(np.float64) / nucl.astype(np.float64)
        Q = tv.astype(np.float64) / nucl.astype(np.float64)
        w = 1.0 - 2.0 * P - Q
        return _clamp(-0.25 * andi_log((1.0 - 2.0 * Q) * w * w))


def logdet(c):
    with np.errstate(all="ignore"):
        nucl = _total(c).astype(np.float64)
        P = c.astype(np.float64) / nucl[:, None]
        lg = None
        for f in range(4):
            s = c[:, 4 * f] + c[:, 4 * f + 1] + c[:, 4 * f + 2] + c[:, 4 * f + 3]
            term = andi_log(s.astype(np.float64) / nucl)
            lg = term if lg is None else lg + term
        for g in range(4):
            s = c[:, g] + c[:, 4 + g] + c[:, 8 + g] + c[:, 12 + g]
            lg = lg + andi_log(s.astype(np.float64) / nucl)

        def p(f, g):
            return P[:, 4 * f + g]

        A, C, G, T = range(4)
        det = (p(A, A) * p(C, C) * (p(G, G) * p(T, T) - p(T, G) * p(G, T)) -
               p(A, A) * p(C, G) * (p(G, C) * p(T, T) - p(T, C) * p(G, T)) +
               p(A, A) * p(C, T) * (p(G, C) * p(T, G) - p(T, C) * p(G, G)) -

               p(A, C) * p(C, A) * (p(G, G) * p(T, T) - p(T, G) * p(G, T)) +
               p(A, C) * p(C, G) * (p(G, A) * p(T, T) - p(T, A) * p(G, T)) -
               p(A, C) * p(C, T) * (p(G, A) * p(T, G) - p(T, A) * p(G, G)) +

               p(A, G) * p(C, A) * (p(G, C) * p(T, T) - p(T, C) * p(G, T)) -
               p(A, G) * p(C, C) * (p(G, A) * p(T, T) - p(T, A) * p(G, T)) +
               p(A, G) * p(C, T) * (p(G, A) * p(T, C) - p(T, A) * p(G, C)) -

               p(A, T) * p(C, A) * (p(G, C) * p(T, G) - p(T, C) * p(G, G)) +
               p(A, T) * p(C, C) * (p(G, A) * p(T, G) - p(T, A) * p(G, G)) -
               p(A, T) * p(C, G) * (p(G, A) * p(T, C) - p(T, A) * p(G, C)))
        return _clamp(-0.25 * (andi_log(det) - 0.5 * lg))


def ani(c):
    with np.errstate(all="ignore"):
        return (1.0 - raw(c)) * 100


def estimate_portable(models, model):
    """float64 of shape models.shape[:-1]: the portable estimate of every model (..., 16 or 17) uint32"""
    shape = np.asarray(models).shape[:-1]
    c = _counts(models)
    fn = {M_RAW: raw, M_KIMURA: kimura, M_LOGDET: logdet, M_ANI: ani}.get(model, jc)
    return fn(c).reshape(shape)


def same_bits(a, b):
    """elementwise: the same double, bit for bit, or both NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def ulp_distance(a, b):
    """the number of doubles between a and b (finite, or equal infinities), elementwise, as int64"""
    def order(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 63)) - i, i)
    return np.abs(order(a) - order(b))


def _pairs(rng, N, length, div, gc=0.5, kappa=1.0):
    """N models of `length` aligned positions at divergence `div` (per model), composition gc, ts/tv ratio kappa"""
    base = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
    L = np.asarray(length, dtype=np.int64)
    mism = rng.binomial(L, np.minimum(div, 1.0))
    w = np.ones((4, 4))
    for f, g in ((0, 2), (2, 0), (1, 3), (3, 1)):
        w[f, g] = kappa
    w[np.arange(4), np.arange(4)] = 0
    w = w * base[:, None] * base[None, :]
    c = np.zeros((N, 17), np.uint64)
    c[:, :16] = rng.multinomial(mism, (w / w.sum()).reshape(-1))
    c[:, 0:16:5] += rng.multinomial(L - mism, base).astype(np.uint64)
    c[:, 16] = L
    return c


def sample_models(seed=20240917, size=120000):
    """The seeded sample of the host tests, (N, 17) uint32, N >= 10^5: genome pairs from identical to saturated, the tiny
    totals 0 ... 4 around the nucl <= 3 rule, counts of 10^8, skewed compositions, and random fillings."""
    rng = np.random.default_rng(seed)
    out = []

    def pairs(N, length, div, gc=0.5, kappa=1.0):
        return _pairs(rng, N, length, div, gc, kappa)

    N = size // 12
    ones = np.ones(N)
    out.append(pairs(N, rng.integers(1000, 5_000_000, N), np.zeros(N)))                      # identical genomes
    out.append(pairs(N, rng.integers(1000, 5_000_000, N), 10.0 ** rng.uniform(-6, -2, N)))   # close
    out.append(pairs(N, rng.integers(1000, 5_000_000, N), rng.uniform(0.01, 0.3, N), 0.4, 2.0))
    out.append(pairs(N, rng.integers(1000, 200_000, N), rng.uniform(0.3, 0.74, N), 0.65, 3.0))
    out.append(pairs(N, rng.integers(4, 400, N), rng.uniform(0.7, 0.8, N)))                  # JC around saturation
    out.append(pairs(N, rng.integers(4, 5000, N), rng.uniform(0.75, 1.0, N)))                # ... and beyond
    out.append(pairs(N, 100_000_000 * ones, rng.uniform(0.0, 0.5, N), 0.5, 2.0))             # counts of 10^8
    out.append(pairs(N, 400_000_000 * ones, 10.0 ** rng.uniform(-8, -1, N), 0.3, 1.0))
    out.append(pairs(N, rng.integers(0, 5, N), rng.uniform(0, 1, N)))                        # totals 0 ... 4
    sat = np.zeros((N, 17), np.uint64)                                                       # p == 0.75 exactly and around
    L = rng.integers(1, 100000, N) * 4
    sat[:, 0] = L // 4 + rng.integers(-1, 2, N)
    sat[:, 1] = L - L // 4
    out.append(sat)
    out.append(rng.integers(0, 2 ** 32, (N, 17), dtype=np.uint64))                            # any bits
    few = rng.integers(0, 50, (size - 11 * N, 17)).astype(np.uint64)                          # sparse small counts
    few[rng.random(few.shape) < 0.5] = 0
    out.append(few)
    return np.concatenate(out).astype(np.uint32)


def sample_log_arguments(seed=7):
    """andi_log alone: subnormals, the least and greatest doubles, exact powers of two, 1.0 and its two neighbours, the
    split point of the reduction and its neighbours, the special values, and random arguments over all exponents"""
    rng = np.random.default_rng(seed)
    bits = [0x1, 0x2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000, 0x3FEFFFFFFFFFFFFF,
            0x3FF0000000000001, 0x3FF6A09E667F3BCC, 0x3FF6A09E667F3BCD, 0x3FF6A09E667F3BCE, 0x3FE6A09E667F3BCD,
            0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF0000000000001,
            0xBFF0000000000000, 0x8000000000000001]
    bits += [e << 52 for e in range(1, 2047)]                       # every power of two
    bits += [1 << k for k in range(52)]                             # ... the subnormal ones
    x = np.array(bits, np.uint64).view(np.float64)
    sub = rng.integers(1, 1 << 52, 20000, dtype=np.uint64).view(np.float64)
    anyexp = rng.integers(0, 0x7FF0000000000000, 200000, dtype=np.uint64).view(np.float64)
    near1 = 1.0 + rng.uniform(-0.3, 0.45, 200000)
    unit = rng.uniform(0, 1, 200000)
    return np.concatenate([x, sub, anyexp, near1, unit, unit * 4.0])


# ---------------------------------------------------------------- count matrices for the device's bootstrap
_DIAG = np.array([0, 5, 10, 15])
_TS = np.array([2, 8, 7, 13])                    # A>G, G>A, C>T, T>C
_TV = np.array([1, 3, 4, 6, 9, 11, 12, 14])


def _from_summed(rng, n, S):
    """the (n, n, 17) uint32 count matrix whose pair (i, j), i < j in row-major order, sums over its two directions to
    S[t] ((n (n - 1) / 2, 17)): every count is split between (i, j) and (j, i) at random, as a scan's two directions
    differ; the diagonal is a scan's (counts[0] = seq_len = 1)"""
    iu = np.triu_indices(n, 1)
    S = np.asarray(S).astype(np.int64)
    assert S.shape == (len(iu[0]), 17) and S[:, :16].max() < 2 ** 31
    a = rng.binomial(S, 0.5)
    M = np.zeros((n, n, 17), np.uint32)
    M[iu[0], iu[1]] = a
    M[iu[1], iu[0]] = S - a
    k = np.arange(n)
    M[k, k, 0] = M[k, k, 16] = 1
    return M


def models_matrix(seed, n, length=20000, div=(0.02, 0.3)):
    """an (n, n, 17) count matrix of n genomes of about `length` aligned positions each way at divergences within div,
    built without a Python loop over the pairs (n = 700 is a quarter of a million of them)"""
    rng = np.random.default_rng(seed)
    per = n * (n - 1) // 2
    L = (2 * length * rng.uniform(0.8, 1.0, per)).astype(np.int64)
    return _from_summed(rng, n, _pairs(rng, per, L, rng.uniform(div[0], div[1], per)))


EDGE_N, EDGE_REPS = 48, 40
EDGE_IDENTICAL = 24  # pairs of identical genomes of 1000 counts and more


def _scatter(rng, N, parts):
    """N models: for every (cells, count) of parts, `count` counts (a number, or one per model) thrown at random over
    `cells`"""
    c = np.zeros((N, 17), np.uint64)
    for cells, count in parts:
        cells = np.asarray(cells)
        got = rng.multinomial(np.broadcast_to(np.asarray(count, dtype=np.int64), (N,)), np.full(len(cells), 1.0 / len(cells)))
        for k, cell in enumerate(cells):
            c[:, cell] += got[:, k].astype(np.uint64)
    c[:, 16] = c[:, :16].sum(axis=1)
    return c


def edge_matrix(seed):
    """The (48, 48, 17) uint32 count matrix of tests/test_bootstrap_edges_gpu.py: 1128 pairs, laid out by class in the
    row-major order of the pairs i < j, so that forty bootstrap replicates of it take the portable estimator through
    every edge the host's sample (sample_models) has -- edge_coverage() below states which, and checks a draw for them.

      24 identical genomes     only the four diagonal cells, 1000 ... 5 * 10^6 counts, even and skewed compositions
      40 close genomes         divergence 10^-6 ... 10^-2, up to 5 * 10^6 counts
      24 of 10^8 counts        5 * 10^7 each way, divergences 0 (exactly) ... 0.5, ts/tv ratio 2
       8 of 4 * 10^8 counts    divergence 10^-8 ... 10^-1, composition 0.3: cells above 10^8, the cancellation of close genomes
      30 of total 0 ... 4      six each; the draw keeps the total, so the doubled totals 0 2 4 6 8 straddle nucl <= 3
      12 at JC's saturation    six of total 4 and six of total 8 with three quarters of the counts off the diagonal
      24 around it             40 ... 400 counts at p = 0.7 ... 0.8, and at p = 0.75 ... 1.0 (the last: mismatches only)
       8 + 8 of Kimura's       transversions the majority (1 - 2Q < 0); total 4, two transitions and two matches
                               (1 - 2P - Q == 0 in three draws of eight)
       8 + 8 + 8 of LogDet's   one nucleotide never occurs (log 0 - log 0); two nucleotides swapped (determinant < 0);
                               three rows within two columns (determinant == 0 with every nucleotide present: +inf)
     926 filler                divergence 0.02 ... 0.3, about 2 * 20000 counts

    Every summed cell stays below 2^31, so a doubled draw does not wrap: summed cells of 2^31 and more are the reference's
    own 32-bit wrap (model_average) and truncation at genome sizes that do not exist, and out of scope."""
    rng = np.random.default_rng(seed)
    n = EDGE_N
    per = n * (n - 1) // 2
    S = []
    half = EDGE_IDENTICAL // 2
    L = np.r_[1000, 5_000_000, rng.integers(1000, 5_000_000, EDGE_IDENTICAL - 2)]
    S.append(_pairs(rng, half, L[:half], np.zeros(half)))                                     # identical, even
    S.append(_pairs(rng, half, L[half:], np.zeros(half), 0.2))                                # identical, skewed
    S.append(_pairs(rng, 40, rng.integers(1000, 5_000_000, 40), 10.0 ** rng.uniform(-6, -2, 40)))
    S.append(_pairs(rng, 24, np.full(24, 100_000_000), np.linspace(0.0, 0.5, 24), 0.5, 2.0))
    S.append(_pairs(rng, 8, np.full(8, 400_000_000), 10.0 ** np.linspace(-8, -1, 8), 0.3, 1.0))
    for t in range(5):
        S.append(_pairs(rng, 6, np.full(6, t), rng.uniform(0, 1, 6)))
    S.append(_scatter(rng, 6, [(_DIAG, 1), (np.r_[_TS, _TV], 3)]))
    S.append(_scatter(rng, 6, [(_DIAG, 2), (np.r_[_TS, _TV], 6)]))
    S.append(_pairs(rng, 12, np.linspace(40, 400, 12).astype(np.int64), np.linspace(0.7, 0.8, 12)))
    S.append(_pairs(rng, 12, np.linspace(40, 400, 12).astype(np.int64), np.linspace(0.75, 1.0, 12)))
    T = np.linspace(200, 5000, 8)
    Q = np.linspace(0.6, 0.9, 8)
    tv, ts = (T * Q).astype(np.int64), (T * 0.05).astype(np.int64)
    S.append(_scatter(rng, 8, [(_TV, tv), (_TS, ts), (_DIAG, T.astype(np.int64) - tv - ts)]))
    S.append(_scatter(rng, 8, [(_TS, 2), (_DIAG, 2)]))
    gone = _pairs(rng, 8, rng.integers(1000, 100_000, 8), rng.uniform(0.02, 0.3, 8))
    for k in range(8):
        f = k % 4
        gone[k, 4 * f:4 * f + 4] = 0
        gone[k, f:16:4] = 0
    gone[:, 16] = gone[:, :16].sum(axis=1)
    S.append(gone)
    swapped = np.zeros((8, 17), np.uint64)
    for k, (a, b) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1), (2, 3))):
        T = int(rng.integers(1000, 100_000))
        rest = [f for f in range(4) if f not in (a, b)]
        one = _scatter(rng, 1, [([4 * a + b], 3 * T // 10), ([4 * b + a], 3 * T // 10), ([5 * rest[0]], 3 * T // 20),
                                ([5 * rest[1]], 3 * T // 20), (np.arange(16), T // 10)])
        swapped[k] = one[0]
    S.append(swapped)
    S.append(_scatter(rng, 8, [([c], rng.integers(20, 100, 8)) for c in (0, 1, 4, 5, 8, 9, 14, 15)]))
    special = sum(len(s) for s in S)
    rest = per - special
    S.append(_pairs(rng, rest, (2 * 20000 * rng.uniform(0.8, 1.0, rest)).astype(np.int64), rng.uniform(0.02, 0.3, rest)))
    return _from_summed(rng, n, np.concatenate(S))


def doubled(B):
    """what andi_hip_model_average makes of a mirrored replicate: every count twice (32-bit)"""
    d = np.array(B, dtype=np.uint32)
    d[..., :16] = d[..., :16] + d[..., :16]
    return d


def edge_coverage(B):
    """Asserts that the replicates B ((reps, n, n, 17), drawn from edge_matrix by any exact generator) reach the edges of
    the estimator, and returns the figures.  These are conditions on the drawn counts and on the NumPy model's estimates
    of them, not on any code under test.  Each holds with probability above 1 - 10^-9 under the multinomial law (most of
    them always: the draw keeps a pair's total and leaves an empty cell empty); the arithmetic stands next to it."""
    reps, n = B.shape[:2]
    iu = np.triu_indices(n, 1)
    m = doubled(B[:, iu[0], iu[1]]).reshape(-1, 17)
    c = m[:, :16].astype(np.uint64)
    total, snps = _total(c), _off_diagonal(c)
    d = {k: estimate_portable(m, k) for k in range(5)}
    fig = {}
    # identical genomes: 24 pairs and the first of the 10^8 ones have no mismatch to draw, in every replicate
    ident = (snps == 0) & (total >= 2 * 1000)
    fig["identical"] = int(ident.sum())
    assert fig["identical"] >= 16 * reps
    for k in (M_JC, M_KIMURA):
        assert (d[k][ident].view(np.uint64) == 0).all(), k                     # +0.0, by the bits
    # LogDet's log(det) - lg / 2 is the difference of two rounded sums of logarithms there, each below 16 in size (no
    # nucleotide of these pairs is rarer than 0.05: 8 log 0.05 = -24, halved): +0.0 by the bits where the roundings cancel
    # or leave d below zero (four draws of five), a few units of 2^-52 above it otherwise -- never -0.0, never below zero
    ld = d[M_LOGDET][ident]
    fig["identical, LogDet +0.0"] = int((ld.view(np.uint64) == 0).sum())
    assert 2 * fig["identical, LogDet +0.0"] >= len(ld) and (ld.view(np.uint64) >> np.uint64(63) == 0).all()
    assert ld.max() <= 2.0 ** -48
    # the totals are kept by the draw: always
    for t in (0, 2, 4, 6, 8):
        assert (total == t).any(), t
    # exactly at saturation: a pair of total 4 with three counts off the diagonal draws 3 of 4 off it with probability
    # 4 * 0.75^3 * 0.25 = 0.42; none of 6 * 40 such draws: 0.58^240 < 10^-56 (the pairs of total 8 only add to that)
    fig["saturated"] = int(((4 * snps == 3 * total) & (total > 3)).sum())
    assert fig["saturated"] >= 1
    # beyond it: the pair of 400 mismatches and no match, always; below it: the identical genomes, always
    assert ((4 * snps > 3 * total) & (total > 3)).any() and ((4 * snps < 3 * total) & (total > 3)).any()
    # +inf, NaN, 0.0 of every model with a logarithm.  0.0: the identical genomes, always.  NaN: the pairs of total 0 (JC,
    # Kimura: 0/0), a nucleotide that never occurs (LogDet), always.  +inf: JC at saturation, above; Kimura where a pair
    # of two transitions and two matches draws two and two, 6/16 a draw, none of 8 * 40: (5/8)^320 < 10^-65; LogDet where
    # the pairs with three rows within two columns have no empty row or column -- a row of 40 and more among at most 800
    # counts is empty with probability below (1 - 40/800)^800 < 10^-17, four rows and four columns: 10^-16 a draw.
    for k in (M_JC, M_KIMURA, M_LOGDET):
        fig["inf", k], fig["nan", k] = int((d[k] == np.inf).sum()), int(np.isnan(d[k]).sum())
        assert fig["inf", k] >= 1 and fig["nan", k] >= 1 and (d[k] == 0.0).any(), k
        assert not (d[k] == -np.inf).any() and not (d[k] < 0).any()
    # a third of every model's values finite and not zero: the 926 filler pairs of 1128 are, at 32000 counts and more of
    # which at most 0.3 mismatch (0.75 is more than 150 standard deviations away)
    for k in range(5):
        fig["finite", k] = int((np.isfinite(d[k]) & (d[k] != 0.0)).sum())
        assert 3 * fig["finite", k] >= len(m), k
    # counts of 10^8: the doubled totals of 2 * 10^8, always; doubled cells of 2 * 10^8 and more: cell 0 of the pairs of
    # 4 * 10^8 counts has 0.35 * 0.9 * 4 * 10^8 = 1.26 * 10^8 of them and more, 2600 standard deviations (10^4) above 10^8
    assert (total == 200_000_000).any() and (c >= 200_000_000).any()
    assert int(c.max()) < 2 ** 32 and (2 * B[..., :16].astype(np.uint64)).max() < 2 ** 32  # nothing wrapped
    return fig


def equal_sums_matrix(seed, n=12):
    """an (n, n, 17) count matrix whose pairs all have the SAME sixteen sums -- four diagonal cells near 3000, twelve
    off-diagonal cells of 20 ... 60 -- so that nothing but its stream tells one pair's draw from another's; the split
    between the two directions differs from pair to pair"""
    rng = np.random.default_rng(seed)
    sums = np.zeros(17, np.int64)
    sums[_DIAG] = [3010, 2990, 3020, 2980]
    sums[np.r_[_TS, _TV]] = rng.integers(20, 61, 12)
    sums[16] = sums[:16].sum()
    return _from_summed(rng, n, np.tile(sums, (n * (n - 1) // 2, 1))), sums[:16].copy()


def switch_matrix(seed):
    """The (7, 7, 17) count matrix of the binomial's branch switches and its cases [(i, j, sums)] in the order of the
    pairs.  Two-cell pairs, sums[0] = N - c and sums[1] = c: the first conditional binomial is the whole draw, cell 0 is
    Binomial(N, (N - c) / N), and cell 1 takes what is left without a draw (counts[c] >= mass).
      c = 9, 10, 11 at N = 20, 1000, 10^6, 10^8   n p on both sides of and at the switch from waiting times to BTRS at 10;
                                                  N = 20, c = 10 is p = 0.5 exactly: no flip, BTRS at its smallest n;
                                                  N = 20, c = 9 is p = 0.55: waiting times after a flip
      N = 10^6, c = N / 2 and N / 2 - 1           p = 0.5, and the least p above it
      N = 1 and N = 2, c = 1                      the smallest draws there are
    and one three-cell pair, 7 in cell 1 and 5 in cell 15: leading empty cells and a last cell that takes what is left.
    The four pairs left over are empty."""
    rng = np.random.default_rng(seed)
    cases = [(N, c) for N in (20, 1000, 10 ** 6, 10 ** 8) for c in (9, 10, 11)]
    cases += [(10 ** 6, 500_000), (10 ** 6, 499_999), (1, 1), (2, 1)]
    n = 7
    S = np.zeros((n * (n - 1) // 2, 17), np.int64)
    for t, (N, c) in enumerate(cases):
        S[t, 0], S[t, 1] = N - c, c
    S[len(cases), 1], S[len(cases), 15] = 7, 5
    S[:, 16] = S[:, :16].sum(axis=1)
    iu = np.triu_indices(n, 1)
    M = _from_summed(rng, n, S)
    return M, [(int(iu[0][t]), int(iu[1][t]), S[t, :16].copy()) for t in range(len(cases) + 1)]
