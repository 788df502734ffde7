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


def sample_models(seed=20240917, size=120000):
    """The seeded sample of the host tests, (N, 17) uint32, N >= 10^5: genome pairs from identical to saturated, the tiny
    totals 0 ... 4 around the nucl <= 3 rule, counts of 10^8, skewed compositions, and random fillings."""
    rng = np.random.default_rng(seed)
    out = []

    def pairs(N, length, div, gc=0.5, kappa=1.0):
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
