"""The layout of a routed scan call (andi_amd/csrc/scan_lane.hip: andi_launch_pair_layout, andi_launch_coop_items) array by array against
what the parent commit c54d474 wrote for the same inputs: pair_class, pair_cost, pair_waves, pair_wave0, sub_order, coop_items and the
lane layout's sixteen counters at the host's first look.  The oracle cannot see these -- a wrong cost, order or counter changes which
kernel takes a pair and how long the call takes, never a count.  The parent's arrays are tests/golden/pair_layout_c54d474.npz, recorded
on the device from a build of c54d474 to which only the reading hook (andi_hip_test_pair_layout) was added; the inputs are made by
cases() below, by the recorder and by the tests alike.

Calls of exactly 1024 pairs (32 x 32 genomes: the sampling's eight wavefronts per pair, one block of every layout kernel), of 1089
(33 x 33: four wavefronts per pair, two blocks, the sort's three launches) and rows of two subjects only.  Small shapes through the
suite's switches: ANDI_ROUTE_TINY=1, ANDI_ROUTE_SMALL=1, ANDI_COOP_SEG=2048, and ANDI_SEG0=64 so that the lanes' segment lengths are
chosen per pair (pair_wave0 exists) for genomes of 6 ... 14 kbp.

Not compared: k_lane_quad's list (its order is that of atomic additions, on either commit, and pass B overwrites it)."""
import os

import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import GOLDEN, knobs

pytestmark = pytest.mark.gpu

KNOBS = {"ROUTE_TINY": 1, "ROUTE_SMALL": 1, "COOP_SEG": 2048, "SEG0": 64}
FIXTURE = os.path.join(GOLDEN, "pair_layout_c54d474.npz")
ROUTE_COOP = 0x40  # scan.h
ARRAYS = ("pair_class", "pair_cost", "pair_waves", "pair_wave0", "sub_order", "coop_items", "counts")


def _genomes(n):
    """n genomes of 6 ... 14 kbp, 0.1 % ... 9 % from one base -- pairs of the wavefront kernel, soft ones --, every eighth one shorter than
    a segment of that kernel: its pairs as a query are the lane scan's whatever they are like (k_pair_estimate)"""
    rng = np.random.default_rng(14)
    base = synth.base_codes(14_000, 9)
    seqs = []
    for k in range(n):
        codes = synth.mutate_codes(base, float(rng.uniform(0.001, 0.09)), 300 + k)
        length = int(rng.integers(6_000, 14_000))
        seqs.append(synth.to_bytes(codes[: (1_500 + 60 * k) if k % 8 == 7 else length]))
    return seqs


def cases():
    """name -> (genomes, subject rows)"""
    g33 = _genomes(33)
    return {"p1024": (g33[:32], list(range(32))), "p1089": (g33, list(range(33))), "rows2": (g33[:32], [27, 19])}  # (two subjects that have pairs of the wavefront kernel in the 32 x 32 call)


def layout_of(seqs, subjects):
    """the arrays of one routed call's layout, through the suite's hooks, on a context of its own"""
    with knobs(**dict({"COOP": None, "POOL": None}, **KNOBS)):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, seqs[i], sa="device") for i in subjects]
        ctx.timings_reset()
        andi_amd.scan_rows(ctx, esas, subjects, Q, model=andi_amd.M_JC)
        t = ctx.timings()
        items, cls, cost, _ = ctx.coop_items()
        out = ctx.pair_layout()
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    assert t["routed_calls"] == 1, t
    assert items is not None and out["pair_wave0"] is not None and out["counts"] is not None  # a list, per-pair segment lengths, a look
    out.update(pair_class=cls, pair_cost=cost, coop_items=items)
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", ["p1024", "p1089", "rows2"])
def test_layout_arrays_equal_the_parent_commits(golden, name):
    seqs, subjects = cases()[name]
    got = layout_of(seqs, subjects)
    pairs = len(subjects) * len(seqs)
    assert len(got["pair_class"]) == pairs and len(got["pair_wave0"]) == pairs + 1 and len(got["sub_order"]) == len(subjects)
    for arr in ARRAYS:
        want = golden[name + "." + arr]
        assert got[arr].shape == want.shape and (got[arr] == want).all(), (name, arr, np.nonzero(np.asarray(got[arr]) != want)[0][:8].tolist())


def test_fixtures_are_not_trivial(golden):
    """what the comparison above rests on: every case has pairs of the wavefront kernel AND pairs the lane scan keeps, offsets that
    rise, a list as long as its counter says, an order that is a permutation and not the identity, cost classes that differ"""
    for name, (seqs, subjects) in cases().items():
        g = {arr: golden[name + "." + arr] for arr in ARRAYS}
        coop = (g["pair_class"] & ROUTE_COOP) != 0
        assert coop.any() and (g["pair_waves"] > 0).any(), name
        assert not (coop & (g["pair_waves"] > 0)).any(), name  # (a pair of the wavefront kernel has no wavefronts in the lane layout)
        assert (np.diff(g["pair_wave0"].astype(np.int64)) == g["pair_waves"]).all() and g["pair_wave0"][-1] == g["pair_waves"].sum() > 0, name
        assert g["counts"][10] == g["pair_waves"].sum() and g["counts"][7] == len(g["coop_items"]) > 0, (name, g["counts"].tolist())
        assert sorted(g["sub_order"].tolist()) == list(range(len(subjects))), name
        assert len(np.unique(g["pair_cost"])) > 3, name
    assert (golden["p1089.sub_order"] != np.arange(33)).any()
