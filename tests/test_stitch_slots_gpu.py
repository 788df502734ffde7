"""Pass B of the anchor scan (scan_lane.hip: stitch_one; scan.hip: stitch_segment) held to the sequential chain SLOT BY SLOT.

The contract (tests/stitch_model.py): whatever state T a segment [start, end) was entered in, the counts `owned` and the
state `true_exit` pass B records for it are those of the plain loop of dist_anchor started in T and run while p < end.
Pass C verifies entries only and silently re-stitches what was entered wrongly, so the final 17 words of a pair -- all the
rest of the suite looks at -- do not see a wrong exit, and see a wrong count only if some input drives a segment through
the arithmetic that is wrong.  Here the per-slot records of a call are read back (andi_hip_test_stitch_slots) and compared
word for word with the model; pass A's records and the entries pass B assumes are held to the model the same way, and
the inputs are shown, by count, to reach every way a replay settles and every kind of launch.

The lane scan is forced (ANDI_COOP=0) with an explicit segment length; per-pair segment lengths are out of scope
(stitch_one is the same code there, only the slot of a segment differs).  Every comparison is integer equality."""
import collections
import functools

import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import SHIPPED_LIB, knobs
from oracle import orc
from tests import stitch_model as sm
from tests.coop_model import State

pytestmark = pytest.mark.gpu

SEGMENTS = (64, 300, 2048)
MODES = {"jc": (andi_amd.M_JC, False), "logdet": (andi_amd.M_LOGDET, True)}
STRAGGLERS, LISTED, ON_THEIR_OWN = 12, 8, 3  # restitch_count: ANDI_STRAGGLERS, the first stage's list, ANDI_RESTITCH_ROUNDS


@pytest.fixture(autouse=True)
def _hooks_only():
    if SHIPPED_LIB:
        pytest.skip("andi_hip_test_stitch_slots is a test hook: not in the shipped library")


# ------------------------------------------------------------------ inputs, calls and model records, each made once
@functools.lru_cache(maxsize=None)
def _input(name):
    if name == "structured":  # the smallest set found whose replays settle in every way (tests/test_stitch_model_host.py)
        seqs, _ = synth.realistic_set(3, 80000, 0.001, 0.06, seed=41, novel_fraction=0.1)
    elif name == "copies":  # one match covers far more than 8 segments: the span window, jumped-over segments
        base = synth.base_codes(60000, 17)
        seqs = [synth.to_bytes(base)] + [synth.to_bytes(synth.mutate_codes(base, k / 60000.0, 50 + k, raw=True)) for k in (0, 3, 40)]
    elif name == "island":  # several hundred anchor-free segments in a row: memory inherited backwards through them
        base = synth.base_codes(60000, 19)
        q = synth.to_bytes(synth.mutate_codes(base, 0.01, 20))
        seqs = [synth.to_bytes(base), q[:20000] + synth.unrelated(25000, 21) + q[20000:]]
    elif name == "large":  # the straggler counter past ANDI_STITCH_MANY
        seqs, _ = synth.realistic_set(8, 400000, 0.001, 0.06, seed=41, novel_fraction=0.1)
    return seqs, sm.pairs_of(seqs)


@functools.lru_cache(maxsize=None)
def _oracle(name, model):
    return orc.dist_matrix(_input(name)[0], model=model, threads=4)


_calls = {}


def _call(ctx, name, seg, mode, **env):
    """one scan call of the set through the lane scan (or what env says) at one segment length: its matrix, timings and slots"""
    key = (name, seg, mode, tuple(sorted(env.items())))
    if key not in _calls:
        seqs = _input(name)[0]
        with knobs(COOP=0, **env):
            Q = andi_amd.Queries(ctx, seqs)
            esas = [andi_amd.Esa(ctx, s, sa="device") for s in seqs]
            ctx.timings_reset()
            got = andi_amd.scan_rows(ctx, esas, list(range(len(seqs))), Q, MODES[mode][0], seg)
            t = ctx.timings()
            slots = ctx.stitch_slots()
            for e in esas:
                e.close()
            Q.close()
        assert t["adaptive_calls"] == 0 and t["routed_calls"] == 0 and t["coop_calls"] == 0, t
        assert slots["seg"] == seg and slots["nsub"] == len(seqs)
        qstart = np.concatenate([[0], np.cumsum([(len(s) + seg - 1) // seg for s in seqs])])
        assert slots["total_segs"] == qstart[-1]
        slots["qstart"] = qstart
        _calls[key] = (got, t, slots)
    return _calls[key]


def _base(slots, s, q):
    return s * slots["total_segs"] + int(slots["qstart"][q])


@functools.lru_cache(maxsize=None)
def _cold(name, s, q, seg, exact):
    return sm.cold_records(_input(name)[1][(s, q)].counting(exact), seg)


def _ints(x):
    return [int(v) for v in x]


# ------------------------------------------------------------------ (a) the contract
def _check_contract(name, slots, s, q, seg, exact, classes=None, steps=None):
    """every slot of the pair: owned and true_exit are the plain chain's from the entry that was used"""
    P = _input(name)[1][(s, q)].counting(exact)
    base, segs = _base(slots, s, q), sm.segments(P.qlen, seg)
    used, texit, owned = slots["used_entry"], slots["true_exit"], slots["owned"]
    for k, (start, end) in enumerate(segs):
        T = State() if k == 0 else State(*_ints(used[base + k][:5]))
        want = sm.walk(P, T, end)
        where = (name, s, q, seg, k, T.tup())
        assert _ints(owned[base + k]) == _ints(want.counts), where
        assert tuple(_ints(texit[base + k][:5])) == want.exit, where
        if classes is not None and k >= 1:
            cls, n = sm.classify(P, T.tup(), k, seg, _cold(name, s, q, seg, exact)[k], replay=want)
            classes[cls] += 1
            steps.append(n)


@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("mode", list(MODES))
def test_every_slot_is_the_plain_chain_from_its_entry(ctx, mode, seg):
    got, _, slots = _call(ctx, "structured", seg, mode)
    for (s, q) in _input("structured")[1]:
        _check_contract("structured", slots, s, q, seg, MODES[mode][1])
    assert (got == _oracle("structured", MODES[mode][0])).all()


# ------------------------------------------------------------------ (b) pass A's records
def _check_cold_records(name, slots, s, q, seg, exact):
    base = _base(slots, s, q)
    for k, rec in enumerate(_cold(name, s, q, seg, exact)):
        slot, where = base + k, (name, s, q, seg, k)
        assert tuple(_ints(slots["cold_exit"][slot][:5])) == rec.exit, where
        assert int(slots["cold_exit"][slot][sm.ANCHORS]) == min(rec.anchors, 255), where
        assert _ints(slots["cold_counts"][slot]) == _ints(rec.counts), where
        mark = slots["marks"][slot]
        if rec.first is not None:
            assert tuple(_ints(mark[24:27])) == rec.first, where
        assert (int(mark[5]) != 0) == (rec.mark is not None), where
        if rec.mark is not None:
            assert tuple(_ints(mark[:5])) == rec.mark[0] and _ints(mark[8:24]) == _ints(rec.mark[1]), where


@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("mode", list(MODES))
def test_pass_a_records_are_the_plain_cold_chain(ctx, mode, seg):
    _, _, slots = _call(ctx, "structured", seg, mode)
    for (s, q) in _input("structured")[1]:
        _check_cold_records("structured", slots, s, q, seg, MODES[mode][1])


# ------------------------------------------------------------------ (c) the entries pass B assumes
def _assumed(slots, seqs, s, q, seg):
    """[(slot, the model's assumed entry from the device's cold exits, whether entry_source passed segments over, whether the
    memory was inherited)] of the pair's segments k >= 1"""
    base, nseg = _base(slots, s, q), (len(seqs[q]) + seg - 1) // seg
    rows = slots["cold_exit"][base:base + nseg].tolist()
    out = []
    for k in range(1, nseg):
        j = sm.entry_source(rows, k, seg, len(seqs[q]))
        out.append((base + k, sm.assumed_entry(rows, k, seg, len(seqs[q])), j != k - 1, j != 0 and rows[j][sm.ANCHORS] == 0))
    return out


def _check_assumed(ctx, name, seg, mode="jc", **env):
    got, _, slots = _call(ctx, name, seg, mode, **env)
    seqs, pairs = _input(name)
    jumped = inherited = 0
    for (s, q) in pairs:
        for slot, T, over, inh in _assumed(slots, seqs, s, q, seg):
            assert tuple(_ints(slots["used_entry"][slot][:5])) == T, (name, s, q, seg, slot - _base(slots, s, q))
            jumped += over
            inherited += inh
    assert (got == _oracle(name, MODES[mode][0])).all()  # (pass C's fix-ups take what the rounds would have)
    return jumped, inherited


@pytest.mark.parametrize("seg", SEGMENTS)
def test_entries_are_the_assumed_ones_without_the_rounds(ctx, seg):
    _check_assumed(ctx, "structured", seg, NO_RESTITCH=1)


def test_entries_past_long_matches_use_the_span_window(ctx):
    """a 60 kbp genome against copies with 0, 3 and 40 substitutions, segments of 64: one match covers hundreds of segments"""
    jumped, _ = _check_assumed(ctx, "copies", 64, NO_RESTITCH=1)
    assert jumped > 1000, jumped  # (the identical pair alone: 936 segments behind the first, both ways)
    _, _, slots = _call(ctx, "copies", 64, "jc", NO_RESTITCH=1)
    for pair in ((0, 1), (2, 3), (3, 0)):  # (identical; 3 and 40 substitutions apart)
        _check_contract("copies", slots, pair[0], pair[1], 64, False)


def test_memory_is_inherited_through_an_island(ctx):
    """a query with 25 kbp of unrelated sequence, segments of 64: several hundred anchor-free segments in a row"""
    _, inherited = _check_assumed(ctx, "island", 64, NO_RESTITCH=1)
    assert inherited > 200, inherited  # (the island is 390 segments; chance anchors in it are few)
    _, _, slots = _call(ctx, "island", 64, "jc", NO_RESTITCH=1)
    _check_contract("island", slots, 0, 1, 64, False)


def test_segments_stitched_again_are_those_off_the_assumption(ctx):
    """with the rounds on, the slots whose entry is not the assumed one were stitched again (k_stitch_heads, stitch_stretch);
    the contract holds for them as for all (test_every_slot_...)"""
    _, _, slots = _call(ctx, "structured", 64, "jc")
    seqs, pairs = _input("structured")
    off = [(s, q, slot) for (s, q) in pairs for slot, T, _, _ in _assumed(slots, seqs, s, q, 64) if tuple(_ints(slots["used_entry"][slot][:5])) != T]
    rc = slots["restitch_count"]
    print("slots off the assumed entry:", len(off), "stretches per round:", _ints(rc[:3]), "left on their own:", int(rc[ON_THEIR_OWN]))
    assert len(off) > 0 and int(rc[0]) > 0
    assert len(off) >= int(rc[0])  # (every stretch of the first round begins with a segment entered otherwise than assumed)
    _, _, plain = _call(ctx, "structured", 64, "jc", NO_RESTITCH=1)
    assert _ints(plain["restitch_count"][:3]) == [0, 0, 0]


# ------------------------------------------------------------------ (d) every exit, every kind of launch, by count
@pytest.mark.parametrize("mode", list(MODES))
def test_the_inputs_reach_every_way_to_settle(ctx, mode):
    """the device's own entries of the calls above, classified by the model: at least 20 of each class in either counting
    mode (the shortcut is the even-split models'), and the first stage's list is in use at segments of 2048.  Measured on an
    MI355X: position 3095, own 920, first 1014, met 689, mark 1993 (LogDet 3514), shortcut 1521; 8 replays listed at 2048"""
    exact = MODES[mode][1]
    classes, steps = collections.Counter(), {}
    for seg in SEGMENTS:
        _, _, slots = _call(ctx, "structured", seg, mode)
        steps[seg] = []
        for (s, q) in _input("structured")[1]:
            _check_contract("structured", slots, s, q, seg, exact, classes, steps[seg])
    print("classes (%s):" % mode, dict(classes), "replays past 12 / 48 steps:",
          {seg: (sum(n > sm.STITCH_FIRST for n in v), sum(n > sm.STITCH_BUDGET for n in v)) for seg, v in steps.items()},
          "listed at 2048:", int(_call(ctx, "structured", 2048, mode)[2]["restitch_count"][LISTED]))
    for cls in sm.CLASSES:
        if cls == "shortcut" and exact:
            assert classes[cls] == 0
        else:
            assert classes[cls] >= 20, (cls, dict(classes))
    assert int(_call(ctx, "structured", 2048, mode)[2]["restitch_count"][LISTED]) > 0


def test_a_call_past_the_straggler_threshold(ctx):
    """8 x 400 kbp of the same generator at segments of 300: more than ANDI_STITCH_MANY replays go past ANDI_STITCH_FIRST steps,
    so replays leave early for the list where their wavefront is nearly empty (over_budget's `early`).  Measured on an MI355X:
    the counter reads 9981, the list holds 6273 to 6306 replays (which lanes leave early depends on the order of an atomic)"""
    got, _, slots = _call(ctx, "large", 300, "jc")
    rc = slots["restitch_count"]
    print("stragglers:", int(rc[STRAGGLERS]), "listed:", int(rc[LISTED]), "stretches per round:", _ints(rc[:3]))
    assert int(rc[STRAGGLERS]) >= 4096 + 512
    assert int(rc[LISTED]) > 0
    for pair in ((0, 1), (5, 2)):
        _check_contract("large", slots, pair[0], pair[1], 300, False)
    assert (got == _oracle("large", andi_amd.M_JC)).all()


# ------------------------------------------------------------------ (e) the group scan
@pytest.mark.parametrize("mode", list(MODES))
def test_the_group_scan_keeps_the_contract(ctx, mode):
    """ANDI_FORCE_REFERENCE=1: k_scan_cold, k_scan_stitch and stitch_segment (what pass C's fix-ups run) on the reference's own
    walk; no marks, no anchor counts (so no memory is inherited), no rounds: every entry is the assumed one"""
    got, t, slots = _call(ctx, "structured", 300, mode, FORCE_REFERENCE=1)
    assert t["reference_subjects"] == 3, t
    seqs, pairs = _input("structured")
    exact = MODES[mode][1]
    for (s, q) in pairs:
        base = _base(slots, s, q)
        for k, rec in enumerate(_cold("structured", s, q, 300, exact)):
            assert tuple(_ints(slots["cold_exit"][base + k][:5])) == rec.exit and _ints(slots["cold_counts"][base + k]) == _ints(rec.counts), (s, q, k)
            assert int(slots["cold_exit"][base + k][sm.ANCHORS]) == 0xffffffff
        for slot, T, _, _ in _assumed(slots, seqs, s, q, 300):
            assert tuple(_ints(slots["used_entry"][slot][:5])) == T, (s, q, slot - base)
        _check_contract("structured", slots, s, q, 300, exact)
    assert (got == _oracle("structured", MODES[mode][0])).all()


def test_no_record_after_a_call_of_another_kind(ctx):
    """the hook hands out nothing stale: a context that has not scanned has no record, and a call with per-pair segment
    lengths clears the one before it"""
    seqs = _input("island")[0]
    own = andi_amd.Context(0)
    try:
        with pytest.raises(andi_amd.AndiHipError):
            own.stitch_slots()
        Q = andi_amd.Queries(own, seqs)
        esas = [andi_amd.Esa(own, s, sa="device") for s in seqs]
        with knobs(COOP=0):
            andi_amd.scan_rows(own, esas, [0, 1], Q, andi_amd.M_JC, 300)
            assert own.stitch_slots()["seg"] == 300
        with knobs(COOP=0, FORCE_ADAPTIVE=1):
            own.timings_reset()
            andi_amd.scan_rows(own, esas, [0, 1], Q, andi_amd.M_JC, 0)
            assert own.timings()["adaptive_calls"] == 1
        with pytest.raises(andi_amd.AndiHipError):
            own.stitch_slots()
        for e in esas:
            e.close()
        Q.close()
    finally:
        own.close()
