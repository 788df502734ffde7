"""k_pool_cold (andi_amd/csrc/coop_pool.h) at the limits random substitutions do not reach, against the oracle, bit for bit.

Uniform substitutions put at most about 25 heads into a round of 2048 positions and give stretches of a few positions.
Here the query is the subject itself -- a random genome of 150 kbp at the default p -- with substitutions written by
rule, so that the main diagonal shows what the kernel has a limit for: more than POOL_CHUNK_HEADS = 128 heads in a round,
more than hc = POOL_MW / 64 = 2048 heads in a window, stretches longer than a head's record (POOL_EQ_MAX = 63 positions:
pool_count_equal_coop, the loop from the fourth word on of the bits or-ed in), records with a separator in them, and more
segments than resident wavefronts (the ticket loop).  Every case states its precondition with a NumPy restatement of sweep
S's head rule on the diagonal's mismatches, and runs through k_pool_cold at segments of 32768 and 131072 symbols,
k_coop_cold and the lane scan."""
import os
import re

import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import ROOT, knobs, rand_dna
from oracle import orc

pytestmark = pytest.mark.gpu

N = 150000
REGION = (20000, 120000)  # where the substitutions by rule go: 100 kbp
POOL_CHUNK_HEADS, POOL_HC, POOL_EQ_MAX, ROUND = 128, 2048, 63, 2048


def _pool_constant(name):
    text = open(os.path.join(ROOT, "andi_amd", "csrc", "coop_pool.h")).read()
    return int(re.search(r"\b%s\b(?:\s*=)?\s*(\d+)" % name, text).group(1))  # (#define NAME n / constexpr ... NAME = n)


def test_the_constants_are_the_kernel_s():
    assert _pool_constant("POOL_CHUNK_HEADS") == POOL_CHUNK_HEADS and _pool_constant("POOL_EQ_MAX") == POOL_EQ_MAX
    assert _pool_constant("POOL_MW_POS") // 64 == POOL_HC


@pytest.fixture(scope="module")
def subject():
    s = rand_dna(np.random.default_rng(2024), N)
    return s, int(andi_amd.lib.subject_prepare(s)[2])


def _substitute(s: bytes, positions) -> bytes:
    out = np.frombuffer(s, np.uint8).copy()
    out[positions] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), out[positions])]
    return out.tobytes()


def heads(mm, thr):
    """sweep S's head rule (coop_pool.h: pool_stream) on a diagonal's mismatch bitmap: a mismatch at x with a mismatch among
    x + 1 ... x + thr and none among x - thr ... x - 1"""
    mm = np.asarray(mm, bool)
    c = np.concatenate(([0], np.cumsum(mm)))  # c[k]: mismatches before position k
    n = len(mm)
    x = np.arange(n)
    after = c[np.minimum(x + thr + 1, n)] - c[np.minimum(x + 1, n)]
    before = c[x] - c[np.maximum(x - thr, 0)]
    return mm & (after > 0) & (before == 0)


def _window_counts(h, span, lo, hi):
    """heads in [a, a + span) for every a with lo <= a and a + span <= hi"""
    c = np.concatenate(([0], np.cumsum(h)))
    a = np.arange(lo, hi - span + 1)
    return c[a + span] - c[a]


def _mismatches(s: bytes, q: bytes):
    return np.frombuffer(s, np.uint8) != np.frombuffer(q, np.uint8)


class _Runner:
    """the pair through every path on one context; the oracle's rows once"""

    def __init__(self, seqs):
        self.seqs = seqs
        self.want = orc.dist_matrix(seqs, model=orc.M_JC, threads=len(seqs))

    def run(self, what, segment=0, expect_pool=None, expect_coop=None, **kn):
        with knobs(**kn):
            ctx = andi_amd.Context(0)
            Q = andi_amd.Queries(ctx, self.seqs)
            esas = [andi_amd.Esa(ctx, s, sa="device") for s in self.seqs]
            ctx.timings_reset()
            got = andi_amd.scan_rows(ctx, esas, list(range(len(self.seqs))), Q, andi_amd.M_JC, segment)
            t = ctx.timings()
            for e in esas:
                e.close()
            Q.close()
            ctx.close()
        if expect_pool is not None:
            assert t["pool_calls"] == expect_pool and t["coop_calls"] == expect_coop, (what, t)
        bad = np.argwhere((got != self.want).any(axis=2))
        assert len(bad) == 0, (what, segment, bad.tolist(), got[tuple(bad[0])].tolist(), self.want[tuple(bad[0])].tolist())

    def all_paths(self):
        for segment in (32768, 131072):
            self.run("k_pool_cold", segment, 1, 1, COOP=4, POOL=None)
        self.run("k_coop_cold", 32768, 0, 1, COOP=4, POOL=0)
        self.run("k_coop_cold", 0, 0, 1, COOP=4, POOL=0)
        self.run("lane scan", 0, 0, 0, COOP=0)


LEAD_IN = np.concatenate([np.arange(1000, REGION[0] - 999, 1000), [REGION[0] - 500]])


def _pairs_every(period):
    """pairs of adjacent substitutions every `period` positions of the region -- and single ones every 1000 positions in
    front of it: a window begins behind a lucky anchor only (coop_dev.h: coop_segment), and in the region the chain finds
    next to none, so the window that meets the region's heads is one that began at these"""
    x = np.arange(REGION[0], REGION[1] - 1, period)
    return np.concatenate([LEAD_IN, x, x + 1])


def _check_lead_in(mm, h):
    """the mismatches in front of the region stand alone -- none is a head, behind each a lucky anchor begins --, and the last
    is nearer to the region than the shortest window is long (four rounds)"""
    assert np.array_equal(np.nonzero(mm[:REGION[0]])[0], LEAD_IN) and not h[:REGION[0]].any()
    assert REGION[0] - LEAD_IN[-1] < 4 * ROUND - 32


def test_more_heads_in_a_round_than_the_list_holds(subject):
    """Two adjacent substitutions every thr + 2 positions over 100 kbp: the first of each pair is a head, and every 2048
    consecutive positions of the region hold more than 128 of them, wherever a round begins -- every round of a window
    there drops its heads, and nothing is decided from the round's first head on (f_cap)."""
    s, thr = subject
    assert thr <= 13, thr  # (2048 / (thr + 2) > 128)
    q = _substitute(s, _pairs_every(thr + 2))
    h = heads(_mismatches(s, q), thr)
    _check_lead_in(_mismatches(s, q), h)
    assert h[REGION[0]] and h.sum() == len(range(REGION[0], REGION[1] - 1, thr + 2))
    per_round = _window_counts(h, ROUND, *REGION)
    assert per_round.min() > POOL_CHUNK_HEADS, per_round.min()
    _Runner([s, q]).all_paths()


def test_more_heads_in_a_window_than_it_has_records(subject):
    """The same with a period of 18: no round of 2048 positions overflows the round's list, and every 24 rounds -- the
    shortest first window of a segment -- hold more heads than a window has records for (hc = 2048).  A window that
    overflows ends some 18 rounds in, the next one is 32 rounds long and overflows again."""
    s, thr = subject
    assert thr <= 16, thr  # (the pair before, 17 positions back, must lie outside x - thr ... x - 1)
    q = _substitute(s, _pairs_every(18))
    h = heads(_mismatches(s, q), thr)
    _check_lead_in(_mismatches(s, q), h)
    assert _window_counts(h, ROUND, 0, N).max() <= POOL_CHUNK_HEADS
    assert _window_counts(h, 24 * ROUND, *REGION).min() > POOL_HC
    _Runner([s, q]).all_paths()


STRETCHES = (62, 63, 64, 65, 96, 200)  # positions behind a head up to the landing of its walk: around POOL_EQ_MAX, and far beyond


def _clusters(thr, first, count):
    """(substituted positions, [(head, stretch)]): clusters of a mismatch every 5 positions, the last one `stretch` positions
    behind the head, clean sequence of 2 thr + 240 ... positions between them; every stretch at `count` offsets (so that the
    heads stand at every position of a word of the bits)"""
    pos, where = [], []
    x = first
    for k in range(count):
        for n in STRETCHES:
            pos += list(range(x, x + n, 5)) + [x + n]
            where.append((x, n))
            x += n + 2 * thr + 240 + k  # (the offset of the heads in their words drifts)
    return np.unique(np.array(pos)), where


def _check_clusters(mm, thr, where):
    h = heads(mm, thr)
    assert np.array_equal(np.nonzero(h)[0], np.array([x for x, _ in where]))
    for x, n in where:
        assert mm[x + n] and not mm[x + n + 1:x + n + 1 + 2 * thr].any()  # the walk lands at x + n + 1, on 2 thr equal symbols
        gaps = np.diff(np.nonzero(mm[x:x + n + 1])[0])
        assert gaps.max() <= 5 < thr
    assert {x % 32 for x, _ in where} == set(range(32))


def test_stretches_longer_than_a_record(subject):
    """Stretches of 62, 63 (a walk still counts their equal symbols from its record), 64, 65, 96 and 200 positions (sweep R
    counts them with all lanes -- pool_count_equal_coop -- and ors the bits in beyond the record's three words)."""
    s, thr = subject
    pos, where = _clusters(thr, REGION[0], 40)
    assert where[-1][0] + 200 < REGION[1]
    q = _substitute(s, pos)
    _check_clusters(_mismatches(s, q), thr, where)
    _Runner([s, q]).all_paths()


def test_records_with_a_separator(subject):
    """The same pair, the query cut into contigs ('!' wherever join_contigs puts it) and three separators placed by hand:
    1, 33 and 64 positions behind a head -- in each of the three words a record's 64 positions are cut from (rc.dirty)."""
    s, thr = subject
    pos, where = _clusters(thr, REGION[0], 40)
    q = np.frombuffer(_substitute(s, pos), np.uint8).copy()
    long_ones = [x for x, n in where if n == 200]
    placed = [long_ones[3] + 1, long_ones[11] + 33, long_ones[17] + 64]
    q[placed] = ord("!")
    q = q.tobytes()
    mm = _mismatches(s, q)
    _check_clusters(mm, thr, where)  # (a separator is a mismatch among the stretch's: the heads stay where they were)
    h = heads(mm, thr)
    for at, back in zip(placed, (1, 33, 64)):
        assert q[at] == ord("!") and h[at - back]
    joined = synth.join_contigs(q, 9, seed=3)
    assert joined.count(b"!") == 3 + 8
    _Runner([s, joined]).all_paths()


def _compute_units():
    """the largest GPU's compute units, from the driver's topology (SIMDs / SIMDs per CU)"""
    import glob
    best = 0
    for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            prop = dict(line.split()[:2] for line in open(path) if len(line.split()) >= 2)
        except OSError:  # (a device this process may not use)
            continue
        if int(prop.get("simd_count", 0)) and int(prop.get("simd_per_cu", 0)):
            best = max(best, int(prop["simd_count"]) // int(prop["simd_per_cu"]))
    assert best, "no GPU in /sys/class/kfd/kfd/topology"
    return best


def test_more_segments_than_resident_wavefronts():
    """8 subjects x 1000 queries of 8.2 ... 9 kbp, one segment each: more items than k_pool_cold has persistent wavefronts,
    so every wavefront comes back for tickets.  Rows of subjects 0 and 7 against the oracle, all rows against the lane scan."""
    cus = _compute_units()
    pool_occ = _pool_constant("POOL_OCC")
    rng = np.random.default_rng(31)
    base = synth.base_codes(9000, 17)
    queries = []
    for k in range(1000):
        codes = synth.mutate_codes(base, float(rng.uniform(0.005, 0.02)), 300 + k)
        queries.append(synth.to_bytes(codes[: int(rng.integers(8200, 9001))]))
    subjects = list(range(8))
    segment = 32768
    total_segs = sum((len(q) + segment - 1) // segment for q in queries)
    assert total_segs * len(subjects) > 4 * pool_occ * cus, (total_segs, cus, pool_occ)
    want = {}
    for i in (0, 7):
        O = orc.OracleEsa(queries[i])
        want[i] = orc.scan_row(O, queries, i, orc.M_JC, threads=os.cpu_count() or 1)
        O.close()
    rows = {}
    for name, kn, expect in (("pool", dict(COOP=4, POOL=None), 1), ("lane", dict(COOP=0), 0)):
        with knobs(**kn):
            ctx = andi_amd.Context(0)
            ctx.expect_queries(len(queries) - 1)
            Q = andi_amd.Queries(ctx, queries)
            esas = [andi_amd.Esa(ctx, queries[i]) for i in subjects]  # (suffix arrays from the host: the long extended entries)
            assert name != "pool" or all(e.single_form() == 1 for e in esas)
            ctx.timings_reset()
            rows[name] = andi_amd.scan_rows(ctx, esas, subjects, Q, andi_amd.M_JC, segment)
            t = ctx.timings()
            for e in esas:
                e.close()
            Q.close()
            ctx.close()
        assert t["pool_calls"] == expect and t["coop_calls"] == expect, (name, t)
    for i in (0, 7):
        assert (rows["pool"][i] == want[i]).all(), (i, np.argwhere((rows["pool"][i] != want[i]).any(axis=1))[:6].tolist())
        assert (rows["lane"][i] == want[i]).all(), i
    assert (rows["pool"] == rows["lane"]).all(), np.argwhere((rows["pool"] != rows["lane"]).any(axis=2))[:6].tolist()
