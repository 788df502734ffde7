"""tests/stitch_model.py on the CPU: the reference that tests/test_stitch_slots_gpu.py holds pass B to is pinned to the
oracle, and the inputs that module runs are shown to reach every way a replay settles."""
import collections

import numpy as np
import pytest

from andi_amd import synth
from oracle import orc
from tests import stitch_model as sm

SEGMENTS = (64, 300, 2048)
MODES = ((orc.M_JC, False), (orc.M_LOGDET, True))


@pytest.fixture(scope="module")
def structured():
    """3 x 80 kbp with repeats, indels, inversions and a tenth of unrelated sequence: the smallest set found whose
    replays settle in every way (a clean synth.pair(40000, 0.05) reaches only shortcut, mark and position)"""
    seqs, _ = synth.realistic_set(3, 80000, 0.001, 0.06, seed=41, novel_fraction=0.1)
    return seqs, sm.pairs_of(seqs)


@pytest.mark.parametrize("model,exact", MODES)
def test_chaining_segments_reproduces_the_oracle(structured, model, exact):
    """plain_segment chained segment by segment -- each entered in the state the one before left -- plus the epilogue of
    src/process.c:199-211 is dist_anchor, at every segment length and in both counting modes"""
    seqs, pairs = structured
    want = orc.dist_matrix(seqs, model=model, threads=3)
    for (s, q), P in pairs.items():
        for seg in SEGMENTS:
            got, _ = sm.chain_by_segments(P.counting(exact), seg)
            assert [int(x) for x in got] == [int(x) for x in want[s, q, :16]], (s, q, seg)
            assert int(want[s, q, 16]) == P.qlen


def test_chaining_covers_identical_and_short_sequences():
    """the epilogue's special case (the last anchor is the whole query), and a query shorter than a segment"""
    s = synth.unrelated(3000, 5)
    seqs = [s, s, s[:777]]
    for model, exact in MODES:
        want = orc.dist_matrix(seqs, model=model, threads=1)
        for (a, b), P in sm.pairs_of(seqs).items():
            for seg in (64, 1000):
                got, _ = sm.chain_by_segments(P.counting(exact), seg)
                assert [int(x) for x in got] == [int(x) for x in want[a, b, :16]], (a, b, seg, model)


def _classes(pairs, exact, segs=SEGMENTS):
    """every replay of the set, entered in the state the model assumes for it: class -> count, and the steps by segment length"""
    count, steps = collections.Counter(), {seg: [] for seg in segs}
    for P0 in pairs.values():
        P = P0.counting(exact)
        for seg in segs:
            cold = sm.cold_records(P, seg)
            rows = [sm.exit_row(r) for r in cold]
            for k in range(1, len(cold)):
                cls, n = sm.classify(P, sm.assumed_entry(rows, k, seg, P.qlen), k, seg, cold[k])
                count[cls] += 1
                steps[seg].append(n)
    return count, steps


@pytest.mark.parametrize("exact", [False, True])
def test_every_way_to_settle_has_members(structured, exact):
    _, pairs = structured
    count, steps = _classes(pairs, exact)
    print("classes (exact=%s):" % exact, dict(count), {seg: (sum(n > sm.STITCH_FIRST for n in v), sum(n > sm.STITCH_BUDGET for n in v)) for seg, v in steps.items()})
    for cls in sm.CLASSES:
        if cls == "shortcut" and exact:
            assert count[cls] == 0  # (the even-split models only)
        else:
            assert count[cls] >= 20, (cls, dict(count))
    assert any(n > sm.STITCH_FIRST for n in steps[300]) and any(n > sm.STITCH_BUDGET for n in steps[2048]), "no long replays"


def test_assumed_entry_windows():
    """entry_source and assumed_entry on hand-made exits: the span window of 8, jumped-over segments, memory inherited
    through anchor-free segments and where that stops"""
    seg, qlen = 10, 1000

    def row(p, mem=(0, 0, 0, 0), anchors=1):
        return [p] + list(mem) + [0, anchors, 0]

    # every chain leaves right behind its segment: the source is k - 1
    exits = [row(10 * (k + 1) + 1, (k, k, k, 0)) for k in range(100)]
    assert all(sm.entry_source(exits, k, seg, qlen) == k - 1 for k in range(1, 100))
    # segment 20 leaves at 255: segments 21 .. 24 (ends 220 .. 250) are jumped over, 25 (end 260) is not
    exits[20] = row(255, (7, 7, 7, 1))
    assert [sm.entry_source(exits, k, seg, qlen) for k in (21, 22, 25, 26, 27)] == [20, 20, 20, 25, 26]
    assert sm.assumed_entry(exits, 25, seg, qlen) == (255, 7, 7, 7, 1)
    # ... but only within SPAN_WINDOW segments: one that leaves 12 segments ahead covers the 8 behind it
    exits[40] = row(10 * 53 + 5)
    assert sm.entry_source(exits, 49, seg, qlen) == 40 and sm.entry_source(exits, 50, seg, qlen) == 49
    # anchor-free segments 60 .. 69: memory from 59, position from the segment before
    for k in range(60, 70):
        exits[k] = row(10 * (k + 1) + 3, (1000, 0, 0, 0), anchors=0)
    assert sm.assumed_entry(exits, 70, seg, qlen) == (703, 59, 59, 59, 0)
    assert sm.assumed_entry(exits, 61, seg, qlen) == (613, 59, 59, 59, 0)
    # an unknown anchor count (the group scan) is not zero: nothing is inherited
    exits[69][sm.ANCHORS] = 0xffffffff
    assert sm.assumed_entry(exits, 70, seg, qlen) == (703, 1000, 0, 0, 0)
    # anchor-free from the query's start: segment 0's memory
    for k in range(1, 5):
        exits[k] = row(10 * (k + 1) + 2, (1000, 0, 0, 0), anchors=0)
    exits[0] = row(12, (3, 2, 1, 1), anchors=0)
    assert sm.assumed_entry(exits, 5, seg, qlen) == (52, 3, 2, 1, 1)


def test_exact_counting_differs_where_it_should():
    """the switch is live: on a GC-rich pair the per-nucleotide counts differ from the even split, and both match the oracle"""
    rng = np.random.Generator(np.random.PCG64(3))
    base = rng.choice(np.frombuffer(b"ACGGGC", np.uint8), 20000)
    s = base.tobytes()
    q = base.copy()
    pos = rng.choice(len(q), 200, replace=False)
    q[pos] = np.frombuffer(b"T", np.uint8)[0]
    seqs = [s, q.tobytes()]
    P = sm.pairs_of(seqs)[(0, 1)]
    even, _ = sm.chain_by_segments(P, 300)
    exact, _ = sm.chain_by_segments(P.counting(True), 300)
    assert [int(x) for x in even] == [int(x) for x in orc.dist_matrix(seqs, model=orc.M_JC)[0, 1, :16]]
    assert [int(x) for x in exact] == [int(x) for x in orc.dist_matrix(seqs, model=orc.M_LOGDET)[0, 1, :16]]
    assert list(even) != list(exact)
