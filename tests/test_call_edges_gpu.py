"""What a routed scan call enqueues around pass A (andi_amd/csrc/scan_call.hip: launch_routed; profiles/r14_call_edges.md): a lane
layout without a pair launches nothing, pass B's first stage of the wavefront kernel's layout goes right behind that kernel while the
host looks for pairs handed back, and the chain of the pairs handed back still starts from that look.  None of it may change a count:
every call against the oracle, and what was enqueued through a hook of the suite's library (andi_hip_test_call_edges).  Small shapes
as in tests/test_coop_order_gpu.py: ANDI_ROUTE_TINY=1 and ANDI_ROUTE_SMALL=1 make a small call a routed one whose host looks,
ANDI_COOP_SEG=2048 gives a pair dozens of segments."""
import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import knobs, rand_dna
from oracle import orc

pytestmark = pytest.mark.gpu

SMALL = {"ROUTE_TINY": 1, "ROUTE_SMALL": 1, "COOP_SEG": 2048}
ROUNDS = 3  # scan.h: ANDI_RESTITCH_ROUNDS
CLEAN_SEG = 8192  # (probed: segments of 2048 symbols leave 24 chains of this set on their own, 8192 and 32768 none)


def _rows(seqs, **kn):
    """all rows through andi_hip_scan_rows on a context of its own; returns (counts, timings, what the call enqueued, layout b's counters)"""
    subjects = list(range(len(seqs)))
    with knobs(**dict({"COOP": None, "POOL": None}, **kn)):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, seqs[i], sa="device") for i in subjects]
        ctx.timings_reset()
        got = andi_amd.scan_rows(ctx, esas, subjects, Q, model=andi_amd.M_JC)
        t = ctx.timings()
        edges, count_b = ctx.call_edges()
        t["went_ahead"], t["ran_again"] = edges.pop("ahead"), edges.pop("again")  # (the call did not wait for its builds; a raised flag made it run again)
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    return got, t, edges, count_b


@pytest.fixture(scope="module")
def star():
    """six genomes of 300 kbp, 0.05 % ... 2 % from their base: every pair suits the wavefront kernel"""
    base = synth.base_codes(300_000, 5)
    seqs = [synth.to_bytes(synth.mutate_codes(base, d, 10 + k)) for k, d in enumerate((0.0005, 0.001, 0.002, 0.005, 0.01, 0.02))]
    return seqs, orc.dist_matrix(seqs, model=orc.M_JC, threads=4)


# ------------------------------------------------------------------ 1: a clean set -- nothing launched for nothing
def test_clean_set_launches_no_lane_pass_and_no_round(star):
    """Every pair is the wavefront kernel's and no true chain leaves its segment on its own (segments of 8192 symbols: a match of the
    closest pairs is a quarter of one): the lane layout's pass A is not enqueued, nor its passes B and C, nor a round of stitching again for
    the wavefront kernel's layout.  Counts equal the oracle's and those of the same call by lanes alone (ANDI_COOP=0)."""
    seqs, want = star
    got, t, edges, count_b = _rows(seqs, **dict(SMALL, COOP_SEG=CLEAN_SEG))
    assert t["routed_calls"] == 1 and t["coop_query_nt"] > 0 and t["lane_query_nt"] == 0 and t["coop_fallbacks"] == 0, t
    assert t["went_ahead"] and not t["ran_again"], t  # (scanned right behind its builds: it did not wait for them, and no flag was raised)
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:6].tolist()
    assert count_b[ROUNDS] == 0 and count_b[11] == 0, count_b.tolist()  # (no chain left on its own, no pair handed back)
    assert edges == {"lanes": (False, 0), "coop": (True, 0), "back": (False, 0)}, edges
    assert t["fixups"] == 0
    lanes, tl, edges_l, _ = _rows(seqs, COOP=0)
    assert not tl["went_ahead"] and tl["routed_calls"] == 0 and edges_l == {"lanes": (False, 0), "coop": (False, 0), "back": (False, 0)}, (tl, edges_l)
    assert (lanes == got).all()


def test_chains_left_on_their_own_bring_the_rounds_back(star):
    """The same set on segments of 2048 symbols -- as long as a match of its closest pairs: some true chains do not meet their cold chain
    inside their segment, the look behind the first stage sees their number, and the rounds are enqueued (they find nothing to stitch
    again here: the chains' exits were right all the same)."""
    seqs, want = star
    got, t, edges, count_b = _rows(seqs, **SMALL)
    assert t["routed_calls"] == 1 and t["lane_query_nt"] == 0, t
    assert count_b[ROUNDS] > 0, count_b.tolist()
    assert edges == {"lanes": (False, 0), "coop": (True, ROUNDS), "back": (False, 0)}, edges
    assert (got == want).all() and t["fixups"] == 0


# ------------------------------------------------------------------ 2: a structured set -- the rounds still run, and work
def test_structured_set_keeps_its_rounds():
    """Genomes with repeats on both strands, indels and inversions (synth.realistic_set without islands, so that the sampling leaves
    pairs to the wavefront kernel) on segments of 512 symbols: chains of the wavefront kernel's layout leave their segments on their own
    and the first round stitches stretches again (counters [3] and [0]); the lane layout has pairs too and runs beside it.  Matrix equal
    to the oracle's; fixups 0, as the parent commit's (c54d474) for the same call."""
    seqs, _ = synth.realistic_set(4, 200_000, 0.002, 0.03, seed=6, novel_fraction=0.0)
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    got, t, edges, count_b = _rows(seqs, **dict(SMALL, COOP_SEG=512))
    assert t["routed_calls"] == 1 and t["coop_query_nt"] > 0 and t["lane_query_nt"] > 0, t
    assert count_b[ROUNDS] > 0 and count_b[0] > 0, count_b.tolist()
    assert edges == {"lanes": (True, ROUNDS), "coop": (True, ROUNDS), "back": (False, 0)}, edges
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:6].tolist()
    assert t["fixups"] == 0


# ------------------------------------------------------------------ 3: pairs handed back -- their chain starts from the later look
def test_pairs_handed_back_start_from_the_look_behind_the_first_stage():
    """A wavefront gives up after four generic steps (ANDI_COOP_GIVEUP=4, as tests/test_coop_order_gpu.py::
    test_pairs_handed_back_from_listed_wavefronts): the word that says so now reaches the host with the first stage's counters, and
    the second lane layout runs from there -- its pass A, its passes B and C."""
    base = synth.base_codes(60_000, 5)
    seqs = [synth.to_bytes(synth.mutate_codes(base, d, 10 + k)) for k, d in enumerate((0.0005, 0.0005, 0.005, 0.02, 0.05, 0.05))]
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    got, t, edges, count_b = _rows(seqs, COOP_GIVEUP=4, **SMALL)
    assert t["routed_calls"] == 1 and t["coop_fallbacks"] > 0, t
    assert count_b[11] == 1 and edges["back"] == (True, ROUNDS) and edges["coop"][0], (edges, count_b.tolist())
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:6].tolist()


# ------------------------------------------------------------------ 4: a scan right behind its builds does not wait for them
def _separator_spanning_subject(rng):
    """(tests/test_scan_gpu.py) a subject whose 10-mer table entry spans a separator: its index build raises flags[0]"""
    while True:
        c = [bytearray(rand_dna(rng, 3000)) for _ in range(3)]
        w = b"GACCGGA"
        c[0][-7:] = w
        c[1][-7:] = w
        c[1][0:2] = b"TA"
        c[2][0:2] = b"TC"
        seq = b"!".join(bytes(x) for x in c)
        rc = seq[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
        if seq.count(w) == 2 and rc.count(w) == 0:
            return seq


def test_flag_raised_by_a_build_still_in_flight_runs_the_call_again(star):
    """The call writes its descriptors for the probe walk without waiting for the builds queued just before it and looks at their flags
    behind its first look.  One subject raises flags[0]: the call runs again the way it does behind finished builds -- not routed, that
    subject on the reference's walk, counted once -- and equals the oracle."""
    seqs = [s[:60_000] for s in star[0][:4]] + [_separator_spanning_subject(np.random.default_rng(58))]
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    got, t, edges, _ = _rows(seqs, **SMALL)
    assert t["went_ahead"] and t["ran_again"], t  # (the first attempt did go ahead, and the flag stopped it behind its first look)
    assert t["reference_subjects"] == 1 and t["routed_calls"] == 0, t
    assert t["stitch_launches"] == 1, t  # (the discarded layout's timer is not counted: the rerun has one segment length, so only its passes B/C)
    assert edges == {"lanes": (False, 0), "coop": (False, 0), "back": (False, 0)}, edges
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:6].tolist()
    got, t, edges, _ = _rows(seqs[:4], **SMALL)  # without it: routed, the flags looked at and found clear
    assert t["went_ahead"] and not t["ran_again"], t
    assert t["reference_subjects"] == 0 and t["routed_calls"] == 1 and edges["coop"][0], (t, edges)
    assert (got == want[:4, :4]).all()


def test_foreign_byte_in_a_subject_is_refused_in_the_same_words(star):
    """A subject with a byte outside the alphabet, staged with a suffix array of the host's (the device's staging refuses it earlier):
    its index build raises flags[1], and the scan right behind that build fails with the words it had when it waited for the build."""
    seqs = [s[:60_000] for s in star[0][:4]]
    bad = seqs[3][:5000] + b"N" + seqs[3][5000:]
    with knobs(**dict({"COOP": None, "POOL": None}, **SMALL)):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, s, sa="device") for s in seqs[:3]] + [andi_amd.Esa(ctx, bad)]
        with pytest.raises(andi_amd.AndiHipError, match=r"andi_hip_scan_rows: a subject holds a byte outside \{A,C,G,T,!,;,#\}"):
            andi_amd.scan_rows(ctx, esas, [0, 1, 2, -1], Q, model=andi_amd.M_JC)
        assert ctx.timings()["reference_subjects"] == 0
        edges, _ = ctx.call_edges()
        assert edges["ahead"] and edges["again"], edges  # (it went ahead, saw flags[1] behind its first look, and failed in the rerun)
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
