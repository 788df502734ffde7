"""How a segment of pass A by wavefronts starts (andi_amd/csrc/coop_dev.h: coop_segment, mode G's step) against the oracle and the
lane scan, bit for bit.

Where the block of 64 probes has no answer for the chain's position, mode G settles that position alone first -- one probe,
COOP_SOLO_CAP symbols deep; a unique match that reaches the cap is followed to its end by coop_lcp -- and takes the block where
several occurrences match as far as the cap, or after COOP_SOLO_MAX such steps in a row without an anchor.  A segment's first step
is of that kind.  So every case here puts a chosen situation AT A SEGMENT START: the genomes are 100 kbp (40 kbp at the chosen
thresholds), the segment lengths 300 ... 2048 for k_coop_cold (windows of 2, 4 and 5 chunks) and 32768 for k_pool_cold, forced
the way tests/test_pool_limits_gpu.py forces it, and the situation stands at X = 65536 (32768): a segment start of all of them.
Each case first asserts its own precondition on the host -- how often the K-mer at X occurs in the subject's text
RS = revcomp(S) # S, how far each occurrence matches, the threshold -- so that it cannot pass by missing its path."""
import os
import re

import numpy as np
import pytest

import andi_amd
import threshold_cases as tc
from conftest import ROOT, knobs, rand_dna
from oracle import orc
from probe_table_model import natural_k, subject_text

pytestmark = pytest.mark.gpu

L = 100000
X = 65536       # a multiple of 512, 2048 and 32768
X300 = 60000    # a multiple of 300
CLEAN = (55536, 75536)  # no substitution here unless a case puts one: matches of 10 kbp and more around X and X300
NUC = np.frombuffer(b"ACGT", np.uint8)


def _constant(header, name):
    text = open(os.path.join(ROOT, "andi_amd", "csrc", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


CAP, SOLO_MAX, MULTI_MAX = _constant("coop_dev.h", "COOP_SOLO_CAP"), _constant("coop_dev.h", "COOP_SOLO_MAX"), _constant("lane_dev.h", "ANDI_MULTI_MAX")


def test_the_constants_are_the_kernel_s():
    assert 16 < CAP <= 128 and 1 <= SOLO_MAX <= 8 and MULTI_MAX == 32


# ------------------------------------------------------------------ the host's view of a probe
def occurrences(RS: bytes, w: bytes):
    out, k = [], RS.find(w)
    while k >= 0:
        out.append(k)
        k = RS.find(w, k + 1)
    return out


def lcp(q: bytes, p: int, RS: bytes, s: int) -> int:
    """equal nucleotides of q[p:] and RS[s:] from the front (a separator on either side ends the match)"""
    n = min(len(q) - p, len(RS) - s)
    a, b = np.frombuffer(q, np.uint8, n, p), np.frombuffer(RS, np.uint8, n, s)
    bad = np.nonzero((a != b) | ~np.isin(a, NUC))[0]
    return int(bad[0]) if len(bad) else n


def probe(q: bytes, p: int, RS: bytes, K: int):
    """anchor() (src/process.c:113-123) at q[p:]: (occurrences of the K-mer, the longest match, whether one occurrence alone
    attains it, where); an absent K-mer: the longest prefix that occurs"""
    occ = occurrences(RS, q[p:p + K])
    if occ:
        lens = [lcp(q, p, RS, s) for s in occ]
        best = max(lens)
        return len(occ), best, lens.count(best) == 1, occ[lens.index(best)], dict(zip(occ, lens))
    for l in range(K - 1, 0, -1):
        occ = occurrences(RS, q[p:p + l])
        if occ:
            return 0, l, len(occ) == 1, occ[0], {}
    return 0, 0, False, 0, {}


def other(sym: int, *avoid) -> int:
    return next(int(c) for c in NUC if c != sym and c not in avoid)


def plant_unique(arr, at, K, rng, n=None):
    """a K-mer (or n-mer) at `at` that occurs once in RS"""
    n = K if n is None else n
    for _ in range(200):
        arr[at:at + n] = rng.choice(NUC, n)
        if len(occurrences(subject_text(arr.tobytes()), arr[at:at + n].tobytes())) == 1:
            return
    raise AssertionError("no unique %d-mer found" % n)


def make_absent(q, at, RS, K):
    """substitute one of the last symbols of the K-mer at `at` so that it occurs nowhere in RS (the symbols in front of the
    substitution still do: on the diagonal)"""
    for off in (K - 1, K - 2, K - 3):
        old = int(q[at + off])
        for c in NUC:
            if c != old:
                q[at + off] = c
                if not occurrences(RS, q[at:at + K].tobytes()):
                    return
        q[at + off] = old
    raise AssertionError("every K-mer occurs")


def scatter(q, step=997):
    """substitutions every `step` symbols outside CLEAN and outside the first 64 kbp's planted copies (which stand at 3000 + 1500 i)"""
    for x in list(range(3700, CLEAN[0], 1500)) + list(range(CLEAN[1] + 464, len(q) - 100, step)):
        q[x] = other(int(q[x]))


@pytest.fixture(scope="module")
def base():
    """(the subject as an array, K, the threshold at the default p): unique K-mers at every place a case starts from"""
    rng = np.random.default_rng(1212)
    s = np.frombuffer(rand_dna(rng, L), np.uint8).copy()
    K = natural_k(2 * L + 1)
    for at in (1000 - K, X300, X - K, X, X + K):
        plant_unique(s, at, K, rng)
    thr = int(andi_amd.lib.subject_prepare(s.tobytes())[2])
    assert K == 9 and K - 1 < thr < CAP, (K, thr)
    return s, K, thr


# ------------------------------------------------------------------ every path of pass A on one set
def _run(seqs, p, model, segment, **kn):
    with knobs(**kn):
        return andi_amd.dist_matrix(seqs, p_value=p, model=model, segment=segment)


def check(seqs, segments=(2048,), p=0.025, model=andi_amd.M_JC, pool=True):
    seqs = [bytes(s) for s in seqs]
    want = orc.dist_matrix(seqs, p_value=p, model=model, threads=len(seqs))
    lane = _run(seqs, p, model, 0, COOP=0)
    assert (lane == want).all(), ("lane scan", np.argwhere((lane != want).any(axis=2)).tolist())
    for coop in (2, 4, 5):
        for segment in segments:
            got = _run(seqs, p, model, segment, COOP=coop, POOL=0)
            bad = np.argwhere((got != want).any(axis=2))
            assert len(bad) == 0, ("k_coop_cold", coop, segment, bad.tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    if pool and model in (andi_amd.M_RAW, andi_amd.M_JC, andi_amd.M_KIMURA):
        got = _run(seqs, p, model, 32768, COOP=4, POOL=None)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, ("k_pool_cold", bad.tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def test_the_switches_take_their_kernels(base):
    """check()'s switches and segment lengths through andi_hip_scan_rows on a context, whose counters say which kernel a call took:
    k_coop_cold for ANDI_COOP = 2, 4, 5 with ANDI_POOL=0, k_pool_cold for ANDI_COOP=4 on segments of 32768 symbols, neither for
    ANDI_COOP=0 -- so that no case passes because its call fell back to another kernel."""
    s, K, thr = base
    q = s.copy()
    scatter(q)
    seqs = [s.tobytes(), q.tobytes()]
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=2)
    cases = [(dict(COOP=0), 0, 0, 0)]
    cases += [(dict(COOP=coop, POOL=0), segment, 1, 0) for coop in (2, 4, 5) for segment in (300, 512, 2048)]
    cases += [(dict(COOP=4, POOL=None), 32768, 1, 1)]
    for kn, segment, coop_calls, pool_calls in cases:
        with knobs(**kn):
            ctx = andi_amd.Context(0)
            Q = andi_amd.Queries(ctx, seqs)
            esas = [andi_amd.Esa(ctx, x, sa="device") for x in seqs]
            ctx.timings_reset()
            got = andi_amd.scan_rows(ctx, esas, [0, 1], Q, andi_amd.M_JC, segment)
            t = ctx.timings()
            for e in esas:
                e.close()
            Q.close()
            ctx.close()
        assert t["coop_calls"] == coop_calls and t["pool_calls"] == pool_calls and t["routed_calls"] == 0, (kn, segment, t)
        assert (got == want).all(), (kn, segment)


# ------------------------------------------------------------------ a K-mer that occurs once, a long match
@pytest.mark.parametrize("close", [False, True])
def test_unique_kmer_long_match(base, close):
    """The segment start lies inside a match longer than the cap and than several segments; the K-mer occurs once.  Identical
    genomes, and genomes 5e-4 apart; segments of 300 and 2048 symbols."""
    s, K, thr = base
    q = s.copy()
    if close:
        rng = np.random.default_rng(5)
        where = rng.choice(np.concatenate([np.arange(100, CLEAN[0]), np.arange(CLEAN[1], L - 100)]), 50, replace=False)
        q[where] = [other(int(c)) for c in q[where]]
    S, Q = s.tobytes(), q.tobytes()
    RS = subject_text(S)
    for at, seg in ((X300, 300), (X, 2048)):
        n, best, unique, pos, _ = probe(Q, at, RS, K)
        assert n == 1 and unique and pos == L + 1 + at and best >= CLEAN[1] - at > max(CAP, 4 * seg), (at, n, best)
    check([S, Q], segments=(300, 2048))


def test_unique_kmer_long_match_logdet(base):
    s, K, thr = base
    q = s.copy()
    scatter(q)
    n, best, unique, pos, _ = probe(q.tobytes(), X, subject_text(s.tobytes()), K)
    assert n == 1 and unique and best > 4 * 2048
    check([s.tobytes(), q.tobytes()], segments=(512, 2048), model=andi_amd.M_LOGDET)


# ------------------------------------------------------------------ absent K-mers
def _absent_steps(s, K, thr, count):
    """`count` steps from X on whose K-mer is absent, by a substitution among its last symbols: each step's longest match ends at its
    substitution or a little behind it -- short of the threshold --, and the next step stands behind that"""
    q = s.copy()
    scatter(q)
    RS = subject_text(s.tobytes())
    at = X
    for k in range(count):
        make_absent(q, at, RS, K)
        n, best, unique, _, _ = probe(q.tobytes(), at, RS, K)
        assert n == 0 and K - 3 <= best < min(K, thr), (k, n, best)
        at += best + 1
    assert at < X + 400
    n, best, unique, pos, _ = probe(q.tobytes(), at, RS, K)
    assert n >= 1 and unique and best >= thr and pos == L + 1 + at  # the step behind them finds an anchor, on the main diagonal
    return q.tobytes()


def test_absent_kmer_then_an_anchor(base):
    s, K, thr = base
    check([s.tobytes(), _absent_steps(s, K, thr, 1)], segments=(512, 2048))


def test_more_absent_kmers_in_a_row_than_single_steps(base):
    s, K, thr = base
    check([s.tobytes(), _absent_steps(s, K, thr, SOLO_MAX + 4)], segments=(512, 2048))


def test_unrelated_query(base):
    """a query without homology: no step from a segment's start finds an anchor for as long as the host follows it"""
    s, K, thr = base
    u = rand_dna(np.random.default_rng(77), 40000)
    RS = subject_text(s.tobytes())
    for start in (0, 2048, 32768):
        at = start
        for _ in range(SOLO_MAX + 3):
            n, best, unique, _, _ = probe(u, at, RS, K)
            assert not (unique and best >= thr), (start, at)
            at += best + 1
    q = s.copy()
    scatter(q)
    check([s.tobytes(), q.tobytes(), u], segments=(2048,))


# ------------------------------------------------------------------ K-mers that occur several times: a repeat planted in the subject
def _copies(s, src, length, count, q_next):
    """`count` copies of src[:length] at 3000, 4500, ... of s, each followed by a symbol that differs from q_next (the query's symbol
    behind the match) -- and from the symbol behind the original, so that a copy matches `length` symbols and no more"""
    for i in range(count):
        y = 3000 + 1500 * i
        assert y + length < CLEAN[0] - 2000 and length < 700
        s[y:y + length] = src[:length]
        s[y + length] = other(int(q_next))


@pytest.mark.parametrize("count", [2, 3, MULTI_MAX + 2])
def test_repeated_kmer_short_copies(base, count):
    """the K-mer at the segment start occurs 2, 3 and more than MULTI_MAX times; the copies match K + 3 symbols, the diagonal on and on"""
    s0, K, thr = base
    s = s0.copy()
    _copies(s, s[X:X + K + 3].copy(), K + 3, count - 1, s[X + K + 3])
    q = s.copy()
    scatter(q)
    RS = subject_text(s.tobytes())
    n, best, unique, pos, lens = probe(q.tobytes(), X, RS, K)
    assert n == count and unique and pos == L + 1 + X and best > 4 * 2048, (n, best)
    assert sorted(lens.values())[:-1] == [K + 3] * (count - 1)
    check([s.tobytes(), q.tobytes()])


def test_diagonal_is_the_longest_only_beyond_the_cap(base):
    s0, K, thr = base
    s = s0.copy()
    _copies(s, s[X:X + CAP + 20].copy(), CAP + 20, 1, s[X + CAP + 20])
    q = s.copy()
    scatter(q)
    n, best, unique, pos, lens = probe(q.tobytes(), X, subject_text(s.tobytes()), K)
    assert n == 2 and unique and pos == L + 1 + X and sorted(lens.values())[0] == CAP + 20 > CAP, lens
    check([s.tobytes(), q.tobytes()])


def test_two_occurrences_tie_beyond_the_cap(base):
    """both occurrences match CAP + 36 symbols: not unique, no anchor -- the chain steps on"""
    s0, K, thr = base
    n1 = CAP + 36
    s = s0.copy()
    a = int(s[X + n1])
    b = other(a)
    c = other(a, b)
    s[3000:3000 + n1] = s[X:X + n1]
    s[3000 + n1] = b
    q = s.copy()
    scatter(q)
    q[X + n1] = c
    n, best, unique, pos, lens = probe(q.tobytes(), X, subject_text(s.tobytes()), K)
    assert n == 2 and not unique and list(lens.values()) == [n1, n1], lens
    check([s.tobytes(), q.tobytes()])


def test_longest_occurrence_off_the_diagonal(base):
    """the diagonal's occurrence matches CAP + 6 symbols, a copy elsewhere CAP + 26: an anchor off the diagonal at a segment's start"""
    s0, K, thr = base
    s = s0.copy()
    n_d, n_x = CAP + 6, CAP + 26
    c = other(int(s[X + n_d]))
    s[3000:3000 + n_x] = s[X:X + n_x]
    s[3000 + n_d] = c
    s[3000 + n_x] = other(int(s[X + n_x]))
    q = s.copy()
    scatter(q)
    q[X + n_d] = c
    n, best, unique, pos, lens = probe(q.tobytes(), X, subject_text(s.tobytes()), K)
    assert n == 2 and unique and best == n_x and pos == L + 1 + 3000 and lens[L + 1 + X] == n_d, lens
    check([s.tobytes(), q.tobytes()])


# ------------------------------------------------------------------ separators and the query's end
def test_separator_of_the_query_inside_the_kmer(base):
    s, K, thr = base
    q = s.copy()
    scatter(q)
    q[X + 3] = ord("!")
    assert b"!" in q[X:X + K].tobytes() and b"!" not in q[X - 64:X].tobytes()
    check([s.tobytes(), q.tobytes()], segments=(512, 2048))


@pytest.mark.parametrize("where", [40, CAP + 36])
def test_separator_in_the_subject_s_occurrence(base, where):
    """the subject's contig ends `where` symbols behind the segment start (inside the cap, and beyond it: coop_lcp meets it)"""
    s0, K, thr = base
    s = s0.copy()
    q = s.copy()
    scatter(q)
    s[X + where] = ord("!")
    n, best, unique, pos, _ = probe(q.tobytes(), X, subject_text(s.tobytes()), K)
    assert n == 1 and unique and best == where >= thr and pos == L + 1 + X
    check([s.tobytes(), q.tobytes()])


@pytest.mark.parametrize("left", ["K - 4", "40"])
def test_query_ends_behind_the_segment_start(base, left):
    """the last segment shorter than K; a query that ends inside the cap"""
    s, K, thr = base
    left = K - 4 if left == "K - 4" else 40
    assert 0 < left < CAP and (left < K or left > thr)
    q = s.copy()
    scatter(q)
    check([s.tobytes(), q[:X + left].tobytes()])


# ------------------------------------------------------------------ strands
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(b: bytes) -> bytes:
    return b[::-1].translate(_RC)


def test_start_on_reverse_strand_homology(base):
    s, K, thr = base
    S = s.tobytes()
    q = s.copy()
    scatter(q)
    q[X - 5000:X + 5000] = np.frombuffer(_rc(S[X - 5000:X + 5000]), np.uint8)
    n, best, unique, pos, _ = probe(q.tobytes(), X, subject_text(S), K)
    assert n == 1 and unique and best == 5000 and pos < L, (n, best, pos)  # in revcomp(S): in front of '#'
    check([S, q.tobytes()])


def test_start_on_a_match_that_runs_into_the_border(base):
    """the query holds revcomp(S[:3000]), one symbol, S[:3000]: ONE diagonal of RS = revcomp(S) # S, with '#' at the symbol between --
    the match from the segment start ends at '#' after 1000 symbols, and the next step's lucky attempt goes on behind it, on the other strand"""
    s, K, thr = base
    S = s.tobytes()
    q = s.copy()
    scatter(q)
    q[X - 2000:X + 1000] = np.frombuffer(_rc(S[:3000]), np.uint8)
    q[X + 1001:X + 4001] = s[:3000]
    Q, RS = q.tobytes(), subject_text(S)
    n, best, unique, pos, _ = probe(Q, X, RS, K)
    assert n == 1 and unique and best == 1000 and pos == L - 1000 and RS[pos + best:pos + best + 1] == b"#"
    assert lcp(Q, X + 1001, RS, pos + 1001) == 3000
    check([S, Q])


# ------------------------------------------------------------------ thresholds
LT, XT = 40000, 32768


def _threshold_set(t, seed):
    rng = np.random.default_rng(seed)
    s, _ = tc.subject(t, LT, seed)
    s = np.frombuffer(s, np.uint8).copy()
    K = natural_k(2 * LT + 1)
    assert K == 9
    return s, K, rng


def _threshold_check(t, s, q):
    S, Q = s.tobytes(), q.tobytes()
    p = tc.p_for_threshold(S, t)
    assert p is not None and tc.threshold(S, p) == t and tc.threshold(Q, p) == t
    assert int(andi_amd.lib.subject_prepare(S, p)[2]) == t
    check([S, Q], segments=(512, 2048), p=p)


def test_threshold_below_the_table_s_depth():
    """thr = 8 <= K - 1: the K-mer at the segment start is absent, and its first K - 1 symbols occur once -- an anchor of 8 symbols that
    the table's entry alone describes (FINAL)"""
    t = 8
    s, K, rng = _threshold_set(t, 808)
    plant_unique(s, XT, K, rng, n=K - 1)
    q = np.frombuffer(tc.mutated(s.tobytes(), 0.005, 81), np.uint8).copy()
    q[XT - 50:XT + 50] = s[XT - 50:XT + 50]
    RS = subject_text(s.tobytes())
    make_absent(q, XT, RS, K)
    n, best, unique, pos, _ = probe(q.tobytes(), XT, RS, K)
    assert n == 0 and best == K - 1 >= t and unique and pos == LT + 1 + XT, (n, best, unique)
    _threshold_check(t, s, q)


def test_threshold_30():
    """thr = 30: a unique match of 29 symbols at the segment start is no anchor, the one of 400 and more behind it is"""
    t = 30
    s, K, rng = _threshold_set(t, 3030)
    plant_unique(s, XT, K, rng)
    plant_unique(s, XT + 30, K, rng)
    q = np.frombuffer(tc.mutated(s.tobytes(), 0.005, 31, 0.3), np.uint8).copy()
    q[XT - 100:XT + 500] = s[XT - 100:XT + 500]
    q[XT + 29] = other(int(q[XT + 29]))
    RS = subject_text(s.tobytes())
    n, best, unique, pos, _ = probe(q.tobytes(), XT, RS, K)
    assert n == 1 and unique and best == 29 < t
    n, best, unique, pos, _ = probe(q.tobytes(), XT + 30, RS, K)
    assert n == 1 and unique and best >= 470 and pos == LT + 1 + XT + 30
    _threshold_check(t, s, q)


# ------------------------------------------------------------------ a routed call
def test_routed_call_hands_back_the_pair_without_homology_at_its_segment_starts(base):
    """Three genomes 0.2 ... 1 % from the base and a fourth whose every segment start (segments of 2048 symbols) lies in 500 symbols of
    unrelated sequence, in one routed call with the step limit at 16: the fourth's six pairs are handed back to the lane scan through
    route_giveup, the clean pairs stay the wavefront kernel's."""
    s, K, thr = base
    GIVEUP = 16
    rng = np.random.default_rng(99)
    seqs = []
    for d in (0.002, 0.005, 0.01):
        q = s.copy()
        where = rng.choice(L - 200, int(d * L), replace=False) + 100
        q[where] = [other(int(c)) for c in q[where]]
        seqs.append(q.tobytes())
    z = s.copy()
    for m in range(0, L, 2048):
        lo, hi = max(m - 100, 0), min(m + 400, L)
        z[lo:hi] = rng.choice(NUC, hi - lo)
    RS = subject_text(seqs[0])
    for m in (2048, X):  # more steps without an anchor from a segment's start than the limit allows
        at = m
        for _ in range(GIVEUP + 1):
            n, best, unique, _, _ = probe(z.tobytes(), at, RS, K)
            assert not (unique and best >= thr) and at < m + 400
            at += best + 1
    seqs.append(z.tobytes())
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    with knobs(COOP=None, POOL=None, ROUTE_TINY=1, COOP_SEG=2048, COOP_GIVEUP=GIVEUP):
        got = andi_amd.dist_matrix(seqs, model=andi_amd.M_JC)
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, x, sa="device") for x in seqs]
        ctx.timings_reset()
        rows = andi_amd.scan_rows(ctx, esas, list(range(4)), Q)
        t = ctx.timings()
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    print(t)
    assert t["routed_calls"] == 1 and t["coop_calls"] == 1, t
    assert t["coop_fallbacks"] == 6 and t["coop_query_nt"] == 6 * L and t["lane_query_nt"] == 6 * L, t
    assert (got == want).all(), np.argwhere((got != want).any(axis=2)).tolist()
    assert (rows == want).all()
