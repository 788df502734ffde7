"""tests/threshold_cases.py hits every threshold of the ladder at the lengths tests/test_thresholds_gpu.py uses, by the
library's min_anchor_length and by the oracle's subject (no GPU)."""
import pytest

import threshold_cases as tc
from andi_amd import lib
from oracle import orc


@pytest.mark.parametrize("t", tc.LADDER)
def test_genome_set_hits_the_threshold(t):
    seqs, ps = tc.genome_set(t)
    assert len(seqs) == 6 and len(seqs[0]) == (1000 if t == 2 else 40000)
    assert b"!" in seqs[4] and seqs[5] != seqs[0]
    for s, p in zip(seqs, ps):
        assert tc.P_LO < p < tc.P_HI
        assert lib.min_anchor_length(p, tc.gc(s), 2 * len(s) + 1) == t
        assert lib.subject_prepare(s, p)[2] == t
        O = orc.OracleEsa(s, p)
        assert O.threshold == t
        O.close()


@pytest.mark.parametrize("t", [t for t in tc.LADDER if t >= 3])
def test_pool_set_hits_the_threshold(t):
    seqs, ps = tc.pool_set(t)
    assert [len(s) for s in seqs] == [100000] * 3
    for s, p in zip(seqs, ps):
        assert lib.subject_prepare(s, p)[2] == t
        O = orc.OracleEsa(s, p)
        assert O.threshold == t
        O.close()


def test_long_queries_of_the_lower_bound():
    seqs, _ = tc.genome_set(2)
    assert [len(q) for q in tc.long_queries(2, seqs)] == [3000, 6000, 10000]


def test_every_threshold_from_3_to_33_is_within_reach():
    """... at 40 kbp, 2 at 1 kbp only; the interval's edges belong to its neighbours"""
    for t in range(3, 34):
        s, p = tc.subject(t, 40000, 5)
        assert tc.threshold(s, p) == t
    s, p = tc.subject(2, 1000, 5)
    assert tc.threshold(s, p) == 2
    assert tc.p_for_threshold(tc.subject(3, 40000, 5)[0], 2) is None
    assert tc.p_for_threshold(s, 1) is None


def test_p_falls_as_the_threshold_grows():
    s, _ = tc.subject(16, 40000, 9)
    ps = [tc.p_for_threshold(s, t) for t in range(8, 24)]
    assert all(a > b for a, b in zip(ps, ps[1:])), ps
