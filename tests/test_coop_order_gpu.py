"""Pass A by wavefronts takes its segments from a LIST (andi_amd/csrc/scan.h: coop_items) in routed calls whose host looks at the
layout: a counting sort of the pairs by cost class on the device (scan_lane.hip: andi_launch_coop_items).  The order of the list must
not change a count: the list heaviest first, lightest first and the grid (the test hook ANDI_COOP_ORDER) against the oracle, and the list itself through a hook of the
suite's library.  Small shapes: ANDI_ROUTE_TINY=1 and ANDI_ROUTE_SMALL=1 make a small call a routed one whose host looks,
ANDI_COOP_SEG=2048 gives a pair dozens of segments."""
import numpy as np
import pytest

import andi_amd
import layout_model
from andi_amd import synth
from conftest import knobs, rand_dna
from oracle import orc

pytestmark = pytest.mark.gpu

ROUTE_COOP = 0x40  # scan.h: ANDI_ROUTE_COOP
SMALL = {"ROUTE_TINY": 1, "ROUTE_SMALL": 1, "COOP_SEG": 2048}
ORDERS = (None, "G", "R")  # the list heaviest first (the default), the grid (no list), the list lightest first


def _rows(seqs, subjects=None, model=andi_amd.M_JC, want_list=False, **kn):
    """rows of `subjects` (all) through andi_hip_scan_rows on a context of its own; returns (counts, timings[, the call's list])"""
    subjects = list(range(len(seqs))) if subjects is None else subjects
    with knobs(**dict({"COOP": None, "POOL": None}, **kn)):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, seqs[i], sa="device") for i in subjects]
        ctx.timings_reset()
        got = andi_amd.scan_rows(ctx, esas, subjects, Q, model=model)
        t = ctx.timings()
        listed = ctx.coop_items() if want_list else None
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    return (got, t, listed) if want_list else (got, t)


def _routed(t):
    assert t["routed_calls"] == 1 and t["coop_query_nt"] > 0, t


def _pairs_of(items, lens, seg, nq):
    """the pair (subject * nq + query) of every item of a list over queries of these lengths"""
    qstart = np.concatenate([[0], np.cumsum((np.asarray(lens) + seg - 1) // seg)])
    sub, wseg = items // qstart[-1], items % qstart[-1]
    return sub * nq + (np.searchsorted(qstart, wseg, side="right") - 1), qstart


def _expected_items(cls, lens, seg, nq):
    qstart = np.concatenate([[0], np.cumsum((np.asarray(lens) + seg - 1) // seg)])
    out = []
    for pair in np.nonzero(cls & ROUTE_COOP)[0]:
        s, q = divmod(int(pair), nq)
        out.append(s * qstart[-1] + np.arange(qstart[q], qstart[q + 1]))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.int64)


# ------------------------------------------------------------------ 1: a star set under every order
@pytest.fixture(scope="module")
def star():
    base = synth.base_codes(60_000, 5)
    # pairs from 0.001 (genomes 0, 1) to 0.1 (genomes 4, 5) apart
    return [synth.to_bytes(synth.mutate_codes(base, d, 10 + k)) for k, d in enumerate((0.0005, 0.0005, 0.005, 0.02, 0.05, 0.05))]


@pytest.mark.parametrize("model", [andi_amd.M_JC, andi_amd.M_KIMURA])
def test_star_set_same_counts_under_every_order(star, model):
    want = orc.dist_matrix(star, model=model, threads=4)
    for order in ORDERS:
        got, t, (items, cls, cost, tsegs) = _rows(star, model=model, want_list=True, COOP_ORDER=order, **SMALL)
        _routed(t)
        assert (got == want).all(), (order, np.argwhere((got != want).any(axis=2))[:6].tolist())
        assert (items is None) == (order == "G"), order
        if items is not None:
            assert (np.sort(items) == _expected_items(cls, [len(s) for s in star], 2048, 6)).all(), order
            exact = layout_model.coop_items(6, 6, [len(s) for s in star], 2048, cls, cost, layout_model.ITEMS_LIGHT if order == "R" else layout_model.ITEMS_HEAVY)
            assert len(items) == len(exact) and (items == exact).all(), order  # (entry by entry: the stable order scan.h promises)
            c = cost[_pairs_of(items.astype(np.int64), [len(s) for s in star], 2048, 6)[0]].astype(int)
            if order is None:
                assert (np.diff(c) <= 0).all() and c[0] > c[-1]
            if order == "R":
                assert (np.diff(c) >= 0).all() and c[0] < c[-1]
    # the pair 0.1 apart is heavier than the pair 0.001 apart (both directions)
    assert min(cost[4 * 6 + 5], cost[5 * 6 + 4]) > max(cost[0 * 6 + 1], cost[1 * 6 + 0]), cost.reshape(6, 6)


# ------------------------------------------------------------------ 2: rows that are not the diagonal
def test_rows_of_two_subjects_leave_out_their_own_queries(star):
    subjects = [4, 1]
    want = np.stack([orc.scan_row(orc.OracleEsa(star[i]), star, i, orc.M_JC, threads=0) for i in subjects])
    for order in (None, "R"):
        got, t, (items, cls, cost, tsegs) = _rows(star, subjects, want_list=True, COOP_ORDER=order, **SMALL)
        _routed(t)
        assert (got == want).all(), order
        pairs, _ = _pairs_of(items.astype(np.int64), [len(s) for s in star], 2048, 6)
        assert len(items) and not np.isin(pairs, [0 * 6 + 4, 1 * 6 + 1]).any()  # (subject row 0 is genome 4, row 1 genome 1)
        assert (np.sort(items) == _expected_items(cls, [len(s) for s in star], 2048, 6)).all()


# ------------------------------------------------------------------ 3, 7: more pairs than a block of the sort takes, and more than 4096
@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(8)
    base = synth.base_codes(14_000, 9)
    seqs = []
    for k in range(70):  # 6 ... 14 kbp, 0.001 ... 0.05 from the base
        codes = synth.mutate_codes(base, float(rng.uniform(0.001, 0.05)), 200 + k)
        seqs.append(synth.to_bytes(codes[: int(rng.integers(6_000, 14_000))]))
    return seqs, orc.dist_matrix(seqs, model=orc.M_JC, threads=4)


@pytest.mark.parametrize("seg", [2048, 8192])
def test_ragged_set_of_4830_pairs_and_its_list(ragged, seg):
    """70 x 69 pairs: the sampling's four-pairs-per-block path, five blocks of the sort, segment counts that differ from pair to pair.
    With segments of 8192 symbols the queries shorter than that are the lane scan's: none of their segments is in the list."""
    seqs, want = ragged
    lens = [len(s) for s in seqs]
    got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, **dict(SMALL, COOP_SEG=seg))
    _routed(t)
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:6].tolist()
    assert tsegs == sum((n + seg - 1) // seg for n in lens)
    # the list: a permutation of exactly the segments of the pairs marked for the wavefront kernel, none of them a self pair
    expect = _expected_items(cls, lens, seg, 70)
    assert len(items) == len(expect) > (4096 if seg == 2048 else 0) and (np.sort(items) == expect).all()
    pairs, _ = _pairs_of(items.astype(np.int64), lens, seg, 70)
    assert (pairs // 70 != pairs % 70).all()
    assert not (cls.reshape(70, 70).diagonal() & ROUTE_COOP).any()
    # classes do not rise along the list; inside a class the pairs stand in slot order, a pair's segments in theirs (scan.h: a stable sort) --
    # entry by entry what tests/layout_model.py makes of the call's final pair_class and pair_cost
    c = cost[pairs].astype(int)
    assert (np.diff(c) <= 0).all() and c[0] > c[-1]
    exact = layout_model.coop_items(70, 70, lens, seg, cls, cost)
    assert len(items) == len(exact) and (items == exact).all(), np.nonzero(items != exact)[0][:8].tolist()
    short = np.asarray(lens) < seg
    if seg == 8192:
        assert short.any() and not short.all() and not short[pairs % 70].any()
    else:
        assert len(np.unique(np.bincount(pairs)[np.unique(pairs)])) > 1  # segment counts differ from pair to pair


def test_launches_of_many_rounds_keep_the_grid(ragged):
    """A call whose wavefront kernel could have more than ANDI_ITEMS_ROUNDS = 8 rounds of the device's resident wavefronts (segments of
    256 symbols: 70 subjects x some 2800 segments, eight rounds of a device of up to 760 CUs) builds no list (scan_call.hip: carve_scratch)."""
    seqs, want = ragged
    got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, **dict(SMALL, COOP_SEG=256))
    _routed(t)
    assert 70 * tsegs > 8 * 760 * 32 and items is None, tsegs
    assert (got == want).all()


# ------------------------------------------------------------------ 4: hand-backs
def test_pairs_handed_back_from_listed_wavefronts(star):
    """A wavefront gives up after four generic steps (ANDI_COOP_GIVEUP=4): the pairs a few per cent apart come back, their other listed
    wavefronts return when they see the mark, and the second lane layout counts them; the closest pairs stay the wavefront kernel's.
    (Genomes with unrelated stretches do not get that far in a call whose host looks: the sampling keeps a 60 kbp genome with one
    island of 5 kbp or more away from the wavefront kernel -- synth.realistic_set(12, 60_000, ..., novel_fraction=0.02) is the lane
    scan's whole, as the second half shows; in small calls that do not look, tests/test_coop_gpu.py hands such pairs back.)"""
    want = orc.dist_matrix(star, model=orc.M_JC, threads=4)
    for order in (None, "R"):
        got, t, (items, cls, cost, tsegs) = _rows(star, want_list=True, COOP_ORDER=order, COOP_GIVEUP=4, **SMALL)
        print("limit of 4, order", order, ":", t)
        _routed(t)
        assert items is not None and len(items) > 0 and t["coop_fallbacks"] > 0, t
        assert (got == want).all(), (order, np.argwhere((got != want).any(axis=2))[:6].tolist())
    seqs, _ = synth.realistic_set(12, 60_000, 0.002, 0.03, seed=6, novel_fraction=0.02)
    got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, COOP_GIVEUP=4, **SMALL)
    assert t["routed_calls"] == 1 and t["coop_query_nt"] == 0 and t["lane_query_nt"] > 0 and items is not None and len(items) == 0, t
    assert (got == orc.dist_matrix(seqs, model=orc.M_JC, threads=4)).all()


# ------------------------------------------------------------------ 5: a subject on the reference's walk
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


def test_subject_on_the_reference_walk_has_no_item(star):
    """A call with a subject in reference mode is not routed at all (scan_call.hip: plan_layout), so it has no list and no item:
    the same call that is routed without that subject keeps the grid with it.  Counts equal the oracle's."""
    flagged = _separator_spanning_subject(np.random.default_rng(58))
    seqs = star[:4] + [flagged]
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, **SMALL)
    assert t["reference_subjects"] == 1 and t["routed_calls"] == 0, t
    assert (got == want).all()
    got, t, (items, cls, cost, tsegs) = _rows(seqs[:4], want_list=True, **SMALL)
    _routed(t)
    assert items is not None and len(items) and (got == want[:4, :4]).all()


# ------------------------------------------------------------------ 6: the pooled kernel from the list
def test_pooled_kernel_keeps_the_grid():
    """A routed call whose wavefront kernel is k_pool_cold builds the list (the choice of the kernel comes with the same look) and does
    not use it: that kernel's calls -- a few subjects, thousands of queries each, alike -- lost by it (profiles/r09_coop_order.md)."""
    base = synth.base_codes(300_000, 5)
    seqs = [synth.to_bytes(synth.mutate_codes(base, d, 10 + k)) for k, d in enumerate((0.0005, 0.005, 0.01, 0.02))]
    want = orc.dist_matrix(seqs, model=orc.M_JC, threads=4)
    for order in (None, "R", "G"):
        got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, COOP_ORDER=order, POOL_MATCH=0, **dict(SMALL, COOP_SEG=32768))
        _routed(t)
        assert t["pool_calls"] == 1, t
        assert items is None
        assert (got == want).all(), (order, np.argwhere((got != want).any(axis=2))[:6].tolist())
    got, t, (items, cls, cost, tsegs) = _rows(seqs, want_list=True, POOL=0, POOL_MATCH=0, **dict(SMALL, COOP_SEG=32768))  # the same call by k_coop_cold
    _routed(t)
    assert t["pool_calls"] == 0 and (got == want).all()
    assert (np.sort(items) == _expected_items(cls, [len(s) for s in seqs], 32768, 4)).all()
