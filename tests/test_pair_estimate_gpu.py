"""k_pair_estimate's verdicts (andi_amd/csrc/scan_lane.hip) pair by pair against what the parent commit c54d474 wrote for the same inputs:
the class byte and the cost class of every pair of a routed call, as they stand after the call (andi_hip_test_coop_items, a hook the
parent has too).  The parent's arrays are tests/golden/pair_estimate_c54d474.npz (tests/golden/record_parent_layout.py records them from a
build of that commit); the inputs are made by cases() below, by the recorder and by the tests alike.

Query lengths cover the sample counts (16, 32, 64 samples: 9 000, 20 000, 40 000 symbols) and the round counts of the further samples
(1, 2, 4, 8 rounds: below 262 144, then 270 000, 530 000, 1 050 000).  Block shapes: at most 1024 pairs (eight wavefronts per pair),
1025 ... 4096 (four, 36 x 36), more (one wavefront per pair, 65 x 65).  Pair kinds: clean, structured with and without islands, and
far apart (0.08) in a small call that does not look, where the sampling's guess decides."""
import os

import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import GOLDEN, knobs

pytestmark = pytest.mark.gpu

LOOK = {"ROUTE_TINY": 1, "ROUTE_SMALL": 1, "COOP_SEG": 2048}  # a small call routed, its host looks
NOLOOK = {"ROUTE_TINY": 1, "COOP_SEG": 2048}  # a small call routed as small calls are: no look, pairs the sampling cannot judge by guess
FIXTURE = os.path.join(GOLDEN, "pair_estimate_c54d474.npz")
ROUTE_COOP = 0x40  # scan.h
LENGTHS = (9_000, 20_000, 40_000, 270_000, 530_000, 1_050_000)


def _star(lengths, ds, seed):
    base = synth.base_codes(max(lengths), seed)
    return [synth.to_bytes(synth.mutate_codes(base, d, 50 + seed + k)[:n]) for k, (n, d) in enumerate(zip(lengths, ds))]


def cases():
    """name -> (genomes, switches)"""
    rng = np.random.default_rng(3)
    out = {}
    # 49 pairs: every sample and round count.  The genomes are prefixes of one base's descendants, so a query finds its whole length only in
    # a subject at least as long: the longest length twice, for a pair of the wavefront kernel at that query length too.
    out["lengths"] = (_star(LENGTHS + LENGTHS[-1:], (0.001, 0.004, 0.008, 0.012, 0.02, 0.03, 0.002), 1), LOOK)
    out["w4"] = (_star([LENGTHS[k % 3] for k in range(36)], rng.uniform(0.001, 0.06, 36), 2), LOOK)  # 1296 pairs: four wavefronts per pair
    out["many"] = (_star([9_000] * 65, rng.uniform(0.001, 0.06, 65), 3), LOOK)  # 4225 pairs: one wavefront per pair
    out["islands"] = (synth.realistic_set(4, 270_000, 0.002, 0.03, seed=6)[0], LOOK)
    out["structured"] = (synth.realistic_set(4, 270_000, 0.002, 0.03, seed=6, novel_fraction=0.0)[0], LOOK)
    out["far"] = (_star([40_000] * 3, (0.04, 0.04, 0.04), 4), NOLOOK)  # pairs 0.08 apart
    out["far_look"] = (_star([270_000] * 3 + [40_000], (0.04, 0.04, 0.001, 0.001), 5), LOOK)
    return out


def verdicts_of(seqs, switches):
    """(pair_class, pair_cost) of one routed call over all rows, on a context of its own"""
    subjects = list(range(len(seqs)))
    with knobs(**dict({"COOP": None, "POOL": None}, **switches)):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, seqs)
        esas = [andi_amd.Esa(ctx, seqs[i], sa="device") for i in subjects]
        ctx.timings_reset()
        andi_amd.scan_rows(ctx, esas, subjects, Q, model=andi_amd.M_JC)
        t = ctx.timings()
        _, cls, cost, _ = ctx.coop_items()
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    assert t["routed_calls"] == 1 and len(cls) == len(seqs) ** 2, t
    return cls, cost


@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", ["lengths", "w4", "many", "islands", "structured", "far", "far_look"])
def test_verdicts_equal_the_parent_commits(golden, name):
    seqs, switches = cases()[name]
    cls, cost = verdicts_of(seqs, switches)
    for arr, got in (("pair_class", cls), ("pair_cost", cost)):
        want = golden[name + "." + arr]
        assert got.shape == want.shape and (got == want).all(), (name, arr, np.nonzero(got != want)[0][:8].tolist())


def test_every_verdict_occurs_in_the_fixtures(golden):
    """the comparison above is no comparison of zeros: pairs marked for the wavefront kernel in every block shape and at every query
    length; pairs in which the sampling saw unrelated stretches (its mark ANDI_ROUTE_LEFT is cleared by k_pair_route: what is left of it
    is a pair of candidate length that is NOT the wavefront kernel's, in the set with islands) ; pairs it could not judge and marked by
    guess (ANDI_ROUTE_GUESS, cleared likewise: the pairs 0.08 apart are the wavefront kernel's in the call that does not look); cost
    classes that differ"""
    def coop(name):
        n = int(round(len(golden[name + ".pair_class"]) ** 0.5))
        return ((golden[name + ".pair_class"] & ROUTE_COOP) != 0).reshape(n, n)
    for name in ("lengths", "w4", "many", "structured"):
        assert coop(name).any(), name
    assert coop("lengths").any(axis=0).all(), coop("lengths").astype(int).tolist()  # (a pair of the wavefront kernel at every query length)
    off = ~np.eye(4, dtype=bool)
    assert not coop("islands")[off].all(), "LEFT-derived"
    assert coop("far")[~np.eye(3, dtype=bool)].any(), "GUESS-derived"
    for name in ("lengths", "w4", "many"):
        assert len(np.unique(golden[name + ".pair_cost"])) > 3, name
