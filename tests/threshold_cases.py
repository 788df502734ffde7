"""Subjects with a chosen anchor threshold (host only; tests/test_threshold_cases_host.py, tests/test_thresholds_gpu.py).

The anchor threshold of a subject (min_anchor_length, src/sequence.c:296-304) is the smallest x whose shustring
probability reaches 1 - p for the subject's G+C content and 2 len + 1 symbols: it falls as p grows, and for a G+C level
and a length most thresholds from 2 to 33 have an interval of p of their own.  p_for_threshold finds the middle of that
interval (in log p), so the value holds for a copy a few substitutions away as a rule -- and every sequence is asked for
its own p anyway.  Thresholds of 2 to 6 need a skewed G+C (0.1; 0.05 at 100 kbp) and a p near 1, 2 itself a subject of about 1 kbp; from
about 21 on a G+C of 0.3 keeps p above 1e-14."""
import math

import numpy as np

from conftest import rand_dna  # (first: it puts the repository's root on the path)
from andi_amd import lib, synth

# the ladder of tests/test_thresholds_gpu.py: the bounds of the wavefront kernels' range (scan_call.hip: plan_call), the
# powers of two (the smear of the head rule doubles; no remainder step) and remainder steps of 1, 3, 7, 13 and 14
LADDER = (2, 3, 4, 7, 8, 15, 16, 17, 29, 30, 31)

P_LO, P_HI = 1e-14, 1.0 - 1e-12

# G+C levels through rand_dna's alphabet (twenty letters each)
ALPHABETS = {
    0.05: b"A" * 10 + b"T" * 9 + b"C",
    0.1: b"A" * 9 + b"T" * 9 + b"CG",
    0.3: b"A" * 7 + b"T" * 7 + b"CCCGGG",
    0.5: b"ACGT" * 5,
}


def gc(seq: bytes) -> float:
    """calc_gc (src/sequence.c:197-208): G and C over ALL bytes, the separators of joined contigs among them."""
    return (seq.count(b"G") + seq.count(b"C")) / len(seq)


def threshold(seq: bytes, p: float) -> int:
    return int(lib.min_anchor_length(p, gc(seq), 2 * len(seq) + 1))


def p_for_threshold(seq: bytes, t: int):
    """The p in (1e-14, 1 - 1e-12) at the middle (in log p) of the interval that gives `seq` the threshold t; None where
    no p of that range does."""
    g, l = gc(seq), 2 * len(seq) + 1
    f = lambda x: int(lib.min_anchor_length(math.exp(x), g, l))  # falls (weakly) as x grows
    LO, HI = math.log(P_LO), math.log(P_HI)

    def edge(k):  # the smallest x of [LO, HI] with f(x) <= k; None: there is none
        if f(LO) <= k:
            return LO
        if f(HI) > k:
            return None
        lo, hi = LO, HI  # f(lo) > k >= f(hi)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if f(mid) <= k:
                hi = mid
            else:
                lo = mid
        return hi

    x1 = edge(t)
    if x1 is None:
        return None
    x0 = edge(t - 1)  # f == t on [x1, x0)
    if x0 is None:
        x0 = HI
    if not x0 > x1:
        return None
    p = math.exp(0.5 * (x1 + x0))
    if not (P_LO < p < P_HI) or int(lib.min_anchor_length(p, g, l)) != t:
        p = math.exp(x1)
    assert int(lib.min_anchor_length(p, g, l)) == t, (t, p, g, l)
    return p


def gc_level(t: int, length=40000) -> float:
    """thresholds of up to 6: 0.1 (beyond 40 kbp 0.05: at 100 kbp a G+C of 0.1 gives 4 at the least); up to 20: 0.5; beyond: 0.3"""
    return (0.1 if length <= 40000 else 0.05) if t <= 6 else 0.5 if t <= 20 else 0.3


def subject(t: int, length: int, seed: int, level=None):
    """(seq, p): a random sequence of `length` symbols at the G+C level that reaches the threshold t, and the p that
    gives it exactly t."""
    level = gc_level(t, length) if level is None else level
    seq = rand_dna(np.random.default_rng(seed), length, ALPHABETS[level])
    p = p_for_threshold(seq, t)
    assert p is not None, "threshold %d is out of reach for %d symbols at G+C %.1f" % (t, length, level)
    assert threshold(seq, p) == t
    return seq, p


def mutated(seq: bytes, d: float, seed: int, level=0.5) -> bytes:
    """A copy with substitutions at round(d len) random places, the new symbol drawn from the level's alphabet (never the
    old one): uniform substitutions would carry a G+C of 0.1 towards 0.5, and the low thresholds out of reach."""
    rng = np.random.default_rng(seed)
    out = np.frombuffer(seq, np.uint8).copy()
    pos = rng.choice(len(out), size=int(round(d * len(out))), replace=False)
    letters = np.frombuffer(ALPHABETS[level], np.uint8)
    new = rng.choice(letters, len(pos))
    while True:
        same = np.nonzero(new == out[pos])[0]
        if not len(same):
            break
        new[same] = rng.choice(letters, len(same))
    out[pos] = new
    return out.tobytes()


def revcomp(b: bytes) -> bytes:
    return bytes(b[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")))


def base_length(t: int) -> int:
    return 1000 if t == 2 else 40000  # (a threshold of 2 is within reach of subjects of about 1 kbp only)


def genome_set(t: int, seed=0):
    """The set of tests/test_thresholds_gpu.py for the threshold t: ([sequence], [p per sequence]) -- a base, copies 0.5 %,
    3 % and 8 % away, a further copy as joined contigs and one reverse-complemented; every p gives its sequence t."""
    lv = gc_level(t)
    base, _ = subject(t, base_length(t), 1000 * t + seed)
    seqs = [base] + [mutated(base, d, 7 * t + k, lv) for k, d in enumerate((0.005, 0.03, 0.08))]
    seqs.append(synth.join_contigs(mutated(base, 0.01, 7 * t + 4, lv), 4, seed=t))
    seqs.append(revcomp(mutated(base, 0.02, 7 * t + 5, lv)))
    ps = [p_for_threshold(s, t) for s in seqs]
    assert all(p is not None for p in ps), (t, ps)
    return seqs, ps


def long_queries(t: int, seqs):
    """t = 2: queries of 3, 6 and 10 kbp for the subjects of 1 kbp -- their copies one behind the other, further mutated"""
    tile = b"".join(seqs[k % 4] for k in range(10))
    return [mutated(tile[:n], 0.02, 50 + k, gc_level(t)) for k, n in enumerate((3000, 6000, 10000))]


def pool_set(t: int, seed=0):
    """three genomes of 100 kbp for k_pool_cold (segments of 32768 symbols): a base and copies 1 % and 4 % away"""
    lv = gc_level(t, 100000)
    base, _ = subject(t, 100000, 2000 * t + seed)
    seqs = [base, mutated(base, 0.01, 9 * t + 1, lv), mutated(base, 0.04, 9 * t + 2, lv)]
    ps = [p_for_threshold(s, t) for s in seqs]
    assert all(p is not None for p in ps), (t, ps)
    return seqs, ps
