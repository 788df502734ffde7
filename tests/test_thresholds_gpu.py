"""Pass A at anchor thresholds 2 ... 31 against the oracle, 17 words per ordered pair, bit for bit.

The threshold (min_anchor_length, the user's -p) decides every count; the rest of the suite runs five p-values, which
give thresholds of about 9 to 20.  Here a ladder (tests/threshold_cases.py: LADDER): both bounds of the range plan_call
admits the wavefront kernels for (2 and 30) and the first threshold they refuse (31); powers of two, at which the smear
of the head rule (coop_pool.h: pool_stream, coop_window.h: coop_window) takes no remainder step, and thresholds whose
remainder step is 1, 3, 7, 13 and 14 positions; thresholds below the probe table's depth K on texts of normal size
(coop_probe_codes' branch for K >= thr).  One test per threshold over every path of pass A: the lane scan, k_lane_quad,
k_coop_cold at windows of 2, 4 and 5 chunks, k_pool_cold, the reference's own walk, pass C's fix-ups -- hook-free paths
first, so that the pass over the shipped library (conftest.needs_hooks) runs them before it skips."""
import numpy as np
import pytest

import andi_amd
import threshold_cases as tc
from conftest import knobs
from oracle import orc

pytestmark = pytest.mark.gpu

WAVEFRONT_MAX = 30  # scan_call.hip: plan_call


class _Set:
    """subjects (each at its own p) staged on the device with the queries they meet, and the oracle's rows"""

    def __init__(self, ctx, seqs, ps, extra_queries=()):
        self.ctx, self.seqs, self.ps = ctx, list(seqs), list(ps)
        self.queries = self.seqs + list(extra_queries)
        self.Q = andi_amd.Queries(ctx, self.queries)
        self.esas = [andi_amd.Esa(ctx, s, p, sa="device") for s, p in zip(self.seqs, self.ps)]
        self._want = {}

    def want(self, model):
        if model not in self._want:
            rows = []
            for i, (s, p) in enumerate(zip(self.seqs, self.ps)):
                O = orc.OracleEsa(s, p)
                rows.append(orc.scan_row(O, self.queries, i, model, threads=4))
                O.close()
            self._want[model] = np.stack(rows)
        return self._want[model]

    def rows(self, model=andi_amd.M_JC, segment=0, **kn):
        """(the device's rows, the call's counters) under the switches kn"""
        with knobs(**kn):
            self.ctx.timings_reset()
            got = andi_amd.scan_rows(self.ctx, self.esas, list(range(len(self.esas))), self.Q, model, segment)
            return got, self.ctx.timings()

    def check(self, what, model=andi_amd.M_JC, segment=0, **kn):
        got, t = self.rows(model, segment, **kn)
        want = self.want(model)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (what, kn, segment, bad[:6].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
        return t

    def close(self):
        for e in self.esas:
            e.close()
        self.Q.close()


def _wavefronts(t):
    return 1 if t <= WAVEFRONT_MAX else 0


@pytest.mark.parametrize("t", tc.LADDER)
def test_threshold(ctx, t):
    seqs, ps = tc.genome_set(t)
    S = _Set(ctx, seqs, ps, tc.long_queries(t, seqs) if t == 2 else ())
    try:
        for E in S.esas:
            assert E.threshold == t
        if t <= 8:
            for E in S.esas:
                assert t < E.download_index()[0]  # below the probe table's depth
        exact = (andi_amd.M_LOGDET, andi_amd.M_ANI) if t in (3, 16, 30) else ()
        # ---- the lane scan
        for segment in (0, 1000):
            tm = S.check("lane scan", segment=segment, COOP=0)
            assert tm["coop_calls"] == 0 and tm["pool_calls"] == 0 and tm["reference_subjects"] == 0, tm
        for model in exact:
            S.check("lane scan", model=model, COOP=0)
        # ---- k_coop_cold (t = 31: refused -- the lane scan)
        for coop in (2, 4, 5):
            for segment in (0, 3000):
                tm = S.check("k_coop_cold", segment=segment, COOP=coop, POOL=0)
                assert tm["coop_calls"] == _wavefronts(t) and tm["pool_calls"] == 0, (coop, segment, tm)
            for model in exact:
                tm = S.check("k_coop_cold<EXACT>", model=model, COOP=coop)
                assert tm["coop_calls"] == 1 and tm["pool_calls"] == 0, (coop, model, tm)
        if t in (3, 16, 30):
            for model in (andi_amd.M_KIMURA, andi_amd.M_RAW):
                S.check("lane scan", model=model, COOP=0)
                tm = S.check("k_coop_cold", model=model, COOP=4, POOL=0)
                assert tm["coop_calls"] == 1, tm
        # ---- the engine's own choice: a tiny call, the wavefront kernel for every pair (t = 2: too small a call for it)
        tm = S.check("engine's choice", COOP=None)
        assert tm["routed_calls"] == 0 and tm["coop_calls"] == (_wavefronts(t) if t > 2 else 0), tm
        # ---- the reference's own walk
        tm = S.check("reference walk", COOP=0, FORCE_REFERENCE=1)
        assert tm["reference_subjects"] > 0, tm
        # ---- k_pool_cold: segments of 32768 symbols (t = 2: the subjects of 1 kbp against the queries of up to 10 kbp)
        if t == 2:
            P = S
        else:
            pseqs, pps = tc.pool_set(t)
            P = _Set(ctx, pseqs, pps)
        try:
            for E in P.esas:
                assert E.threshold == t
            tm = P.check("k_pool_cold", segment=32768, COOP=4, POOL=None)
            assert tm["coop_calls"] == _wavefronts(t) and tm["pool_calls"] == _wavefronts(t), tm
            if t in (3, 16, 30):
                for model in (andi_amd.M_KIMURA, andi_amd.M_RAW):
                    tm = P.check("k_pool_cold", model=model, segment=32768, COOP=4, POOL=None)
                    assert tm["pool_calls"] == 1, tm
        finally:
            if P is not S:
                P.close()
        # ---- (test hooks from here on) pass C's fix-ups: no re-stitch rounds in pass B
        tm0 = S.check("lane scan, segments of 300", segment=300, COOP=0)
        tm = S.check("lane scan without re-stitch rounds", segment=300, COOP=0, NO_RESTITCH=1)
        print("threshold %d: fix-ups with the re-stitch rounds %d, without %d" % (t, tm0["fixups"], tm["fixups"]))
        assert tm["fixups"] >= tm0["fixups"], (tm0, tm)  # (what the re-stitch rounds leave to pass C is left to it without them too)
        if t > 2:  # segments of 300 on genomes up to 8 % apart, contigs, the other strand: some cold start lands wrong (t = 2: four segments per kbp of query, none does)
            assert tm["fixups"] > 0, tm
        # ---- k_lane_quad for every pair
        tm = S.check("k_lane_quad", COOP=0, QUAD_MATCH=0, FORCE_ADAPTIVE=1)
        assert tm["adaptive_calls"] == 1 and tm["coop_calls"] == 0, tm
        for model in exact:
            S.check("k_lane_quad", model=model, COOP=0, QUAD_MATCH=0, FORCE_ADAPTIVE=1)
        # ---- routed per pair (t = 31: refused as well)
        if t > 2:
            tm = S.check("routed", COOP=None, ROUTE_TINY=1)
            assert tm["routed_calls"] == _wavefronts(t) and tm["coop_calls"] == _wavefronts(t) and tm["pool_calls"] == 0, tm
    finally:
        S.close()


def test_one_subject_past_the_range_keeps_the_call_from_the_wavefront_kernels(ctx):
    """plan_call looks at every subject of the call: subjects at thresholds 3, 16 and 30 (each with copies of its own
    among the queries) take the wavefront kernel together; a fourth at 31 sends the whole call to the lane scan."""
    seqs, ps = [], []
    for t in (3, 16, 30, 31):
        s, p = tc.subject(t, 40000, 77 + t)
        seqs.append(s), ps.append(p)
    copies = [tc.mutated(s, d, 5 + k, tc.gc_level(t)) for k, (s, t, d) in enumerate(zip(seqs, (3, 16, 30, 31), (0.01, 0.03, 0.06, 0.02)))]
    for n, expect in ((3, 1), (4, 0)):
        S = _Set(ctx, seqs[:n], ps[:n], copies)
        try:
            assert [E.threshold for E in S.esas] == [3, 16, 30, 31][:n]
            tm = S.check("mixed thresholds", COOP=4, POOL=0)
            assert tm["coop_calls"] == expect and tm["pool_calls"] == 0, tm
            tm = S.check("mixed thresholds, pooled", segment=32768, COOP=4, POOL=None)
            assert tm["coop_calls"] == expect and tm["pool_calls"] == expect, tm
            S.check("mixed thresholds, lane scan", COOP=0)
        finally:
            S.close()
