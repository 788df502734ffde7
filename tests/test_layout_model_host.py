"""tests/layout_model.py -- the NumPy model the layout kernels of a routed scan call are held to (tests/test_layout_kernels_gpu.py) -- checked
without a GPU: against what the device wrote for three real calls (tests/golden/pair_layout_c54d474.npz, the inputs of
tests/test_pair_layout_gpu.py::cases()), and on calls of a few pairs whose results are written out here by hand, one per rule of the routing
(andi_amd/csrc/scan_lane.hip: route_pair) and per detail of the orders (andi_amd/csrc/scan.h: sub_order, coop_items)."""
import numpy as np
import pytest

import layout_model as lm
from layout_model import COOP, GUESS, LEFT, POOLCAND, SOFT
from test_pair_layout_gpu import FIXTURE, KNOBS, cases


# ------------------------------------------------------------------ the model against recorded device output
@pytest.fixture(scope="module")
def golden():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def recorded_cases():
    return cases()


@pytest.mark.parametrize("name", ["p1024", "p1089", "rows2"])
def test_model_reproduces_the_recorded_calls(golden, recorded_cases, name):
    seqs, subjects = recorded_cases[name]
    g = {arr: golden[name + "." + arr] for arr in ("pair_class", "pair_cost", "pair_waves", "pair_wave0", "coop_items", "counts")}
    qlen, nsub, nq, seg = [len(s) for s in seqs], len(subjects), len(seqs), KNOBS["COOP_SEG"]
    items = lm.coop_items(nsub, nq, qlen, seg, g["pair_class"], g["pair_cost"])
    assert len(items) == len(g["coop_items"]) > 0 and (items == g["coop_items"]).all(), np.nonzero(items != g["coop_items"])[0][:8].tolist()
    assert (lm.offsets(g["pair_waves"]) == g["pair_wave0"]).all()
    # the two counters the recorded final state determines: the list's length and the wavefronts the lanes keep
    start = lm.qseg_start(qlen, seg)
    coop = np.nonzero(g["pair_class"] & COOP)[0]
    assert g["counts"][lm.COOP_SEGS] == (start[coop % nq + 1] - start[coop % nq]).sum() == len(items)
    assert g["counts"][lm.LANE_WAVES] == g["pair_waves"].sum() == lm.offsets(g["pair_waves"])[-1]
    # (the routing of a final state is the identity but for the rule of small calls, which these calls are not)
    cls, waves, counts, rules = lm.route(nsub, nq, qlen, subjects, g["pair_class"], g["pair_waves"], 0, KNOBS["SEG0"], 3, seg, 0)
    assert (cls == g["pair_class"]).all() and (waves == g["pair_waves"]).all()
    assert counts[lm.COOP_SEGS] == g["counts"][lm.COOP_SEGS] and counts[lm.LANE_WAVES] == g["counts"][lm.LANE_WAVES]


# ------------------------------------------------------------------ hand-made calls
def _route(qlen, self_q, cls, **kw):
    """one subject row per entry of self_q; pair_waves from the classes at seg0 = 64; the wavefront kernel's segments 1000 long"""
    nsub, nq = len(self_q), len(qlen)
    cls = np.asarray(cls)
    waves = lm.waves_of(np.tile(qlen, nsub), 64 << (cls & 3))
    arg = dict(struct_waves=0, max_class=3, route_all_few=0)
    arg.update(kw)
    return lm.route(nsub, nq, qlen, self_q, cls, waves, arg["struct_waves"], 64, arg["max_class"], 1000, arg["route_all_few"]), waves


def _counts(**kw):
    c = np.zeros(16, np.int64)
    for k, v in kw.items():
        c[getattr(lm, k)] = v
    return c.tolist()


def test_soft_pairs_go_back_unless_the_lanes_pairs_are_few_or_the_call_is_small():
    # four queries of 6400 nt: 100 segments of 64, two wavefronts each; seven segments of the wavefront kernel
    given = [COOP | SOFT, COOP, 0, COOP | SOFT]
    (cls, waves, counts, rules), w_in = _route([6400] * 4, [-1], given)
    assert w_in.tolist() == [2, 2, 2, 2]
    # all 8, sparse 6 (the two soft pairs and the hard one): 60 > 8, the lanes' pairs are not few
    assert cls.tolist() == [0, COOP, 0, 0] and waves.tolist() == [2, 0, 2, 2]
    assert counts.tolist() == _counts(ALL_WAVES=8, SPARSE_WAVES=6, HARD_WAVES=2, COOP_SEGS=7, LANE_WAVES=6)
    assert rules["soft_back"] == (2, 0) and rules["take_all"] == (0, 3)
    # a small call keeps them with the wavefront kernel (and takes no more: 20 * 2 > 8)
    (cls, waves, counts, rules), _ = _route([6400] * 4, [-1], given, route_all_few=1)
    assert cls.tolist() == [COOP, COOP, 0, COOP] and waves.tolist() == [0, 0, 2, 0]
    assert counts.tolist() == _counts(ALL_WAVES=8, SPARSE_WAVES=6, HARD_WAVES=2, COOP_SEGS=21, LANE_WAVES=2)
    assert rules["soft_back"] == (0, 2) and rules["take_all"] == (0, 1)
    # one soft pair among twelve: all 24, sparse 2, 20 <= 24: few, it rides along
    (cls, waves, counts, rules), _ = _route([6400] * 12, [-1], [COOP | SOFT] + [COOP] * 11)
    assert cls.tolist() == [COOP] * 12 and waves.tolist() == [0] * 12
    assert counts.tolist() == _counts(ALL_WAVES=24, SPARSE_WAVES=2, COOP_SEGS=84)
    assert rules["soft_back"] == (0, 1)


def test_guessed_pairs_go_back_where_the_call_shows_unrelated_stretches():
    (cls, waves, counts, rules), _ = _route([6400] * 4, [-1], [COOP | GUESS, LEFT, COOP, COOP])
    # all 8, island 2: 40 > 8
    assert cls.tolist() == [0, 0, COOP, COOP] and waves.tolist() == [2, 2, 0, 0]
    assert counts.tolist() == _counts(ALL_WAVES=8, SPARSE_WAVES=2, HARD_WAVES=2, ISLAND_WAVES=2, COOP_SEGS=14, LANE_WAVES=4)
    assert rules["guess_back"] == (1, 0) and rules["bump"] == (0, 2)  # (both suspected pairs are the lanes' now; no structured call)
    (cls, waves, counts, rules), _ = _route([6400] * 4, [-1], [COOP | GUESS, 0, COOP, COOP])
    assert cls.tolist() == [COOP, 0, COOP, COOP] and waves.tolist() == [0, 2, 0, 0] and rules["guess_back"] == (0, 1)


def test_structured_calls_double_the_suspected_pairs_segments():
    # 20 000 nt in class 1: 157 segments of 128, three wavefronts; in class 2: 79 of 256, two.  8192 nt in class 3: 16 of 512.
    qlen, given = [20_000, 8192, 100], [LEFT | 1, GUESS | 3, COOP]
    (cls, waves, counts, rules), w_in = _route(qlen, [-1], given, struct_waves=2)
    assert w_in.tolist() == [3, 1, 1]
    # all 5, 3 * 2 >= 5: the pair below the longest class moves up and is counted anew; the pair in class 3 stays
    assert cls.tolist() == [2, 3, COOP] and waves.tolist() == [2, 1, 0]
    assert counts.tolist() == _counts(STRUCT_WAVES=2, ALL_WAVES=5, SPARSE_WAVES=4, HARD_WAVES=4, ISLAND_WAVES=3, COOP_SEGS=1, LANE_WAVES=3)
    assert rules["bump"] == (1, 1)
    (cls, waves, counts, rules), _ = _route(qlen, [-1], given, struct_waves=2, max_class=1)  # no class above 1
    assert cls.tolist() == [1, 3, COOP] and waves.tolist() == [3, 1, 0] and rules["bump"] == (0, 2)
    (cls, waves, counts, rules), _ = _route(qlen, [-1], given, struct_waves=1)  # 3 * 1 < 5: not a structured call
    assert cls.tolist() == [1, 3, COOP] and waves.tolist() == [3, 1, 0] and rules["bump"] == (0, 2)


def test_small_calls_give_the_wavefront_kernel_every_pair_where_the_lanes_would_have_few():
    # 81 920 nt: 1280 segments of 64, twenty wavefronts, 82 segments of 1000; 100 nt: one wavefront, one segment.  Two rows with their own queries.
    qlen, self_q = [81_920, 81_920, 100], [0, 1]
    given = [0, COOP, POOLCAND, COOP | POOLCAND, 0, COOP]
    (cls, waves, counts, rules), w_in = _route(qlen, self_q, given, route_all_few=1)
    assert w_in.tolist() == [20, 20, 1, 20, 20, 1]  # (the model counts what it is given: a self pair's words are zero in a real call, below)
    given_waves = np.array([0, 20, 1, 20, 0, 1])
    cls, waves, counts, rules = lm.route(2, 3, qlen, self_q, given, given_waves, 0, 64, 3, 1000, 1)
    # all 42, hard 1: 20 <= 42 -- the hard pair goes too (its pool mark is counted), the self pairs do not
    assert cls.tolist() == [0, COOP, COOP, COOP, 0, COOP] and waves.tolist() == [0] * 6
    assert counts.tolist() == _counts(ALL_WAVES=42, SPARSE_WAVES=1, HARD_WAVES=1, COOP_SEGS=166, POOL_SEGS=83)
    assert rules["take_all"] == (1, 2) and rules["pool"] == (2, 2)
    # the same call, not small: the hard pair stays
    cls, waves, counts, rules = lm.route(2, 3, qlen, self_q, given, given_waves, 0, 64, 3, 1000, 0)
    assert cls.tolist() == [0, COOP, 0, COOP, 0, COOP] and waves.tolist() == [0, 0, 1, 0, 0, 0]
    assert counts.tolist() == _counts(ALL_WAVES=42, SPARSE_WAVES=1, HARD_WAVES=1, COOP_SEGS=165, POOL_SEGS=82, LANE_WAVES=1)
    # small, but two hard pairs of twenty wavefronts: 20 * 21 > 42
    cls, waves, counts, rules = lm.route(2, 3, qlen, self_q, [0, 0, 0, COOP, 0, COOP], given_waves, 0, 64, 3, 1000, 1)
    assert cls.tolist() == [0, 0, 0, COOP, 0, COOP] and rules["take_all"] == (0, 4)


def test_subjects_by_falling_cost_ties_by_index():
    assert lm.sub_order([1.0, 2.0, 1.0, 2.0, 0.5]).tolist() == [1, 3, 0, 2, 4]
    assert lm.sub_order(np.zeros(5)).tolist() == [0, 1, 2, 3, 4]
    cost = np.arange(8193, dtype=np.float32)
    assert (lm.sub_order(cost) == np.arange(8193)).all()  # too many to rank: as they come
    assert (lm.sub_order(cost[:8192]) == np.arange(8192)[::-1]).all()


def test_offsets_and_the_quad_list():
    waves, cls = [2, 0, 3, 1, 0], [0x80, 0x80, 1, 0x82, COOP]
    w0 = lm.offsets(waves)
    assert w0.tolist() == [0, 2, 2, 5, 6, 6]
    assert lm.quad_list(cls, waves, w0).tolist() == [0, 1, 5]


def test_list_order_clamped_cost_and_lightest_first():
    # segments of 1000: the queries have 3, 1 and 2 of them, six per subject
    qlen, cls = [2500, 1000, 1001], [COOP] * 6
    cost = [10, 200, 5, 63, 63, 0]  # 200 counts as 63, the heaviest class
    heavy = lm.coop_items(2, 3, qlen, 1000, cls, cost)
    # keys 53, 0, 58, 0, 0, 63: pairs 1, 3, 4 (one class, in slot order), then 0, 2, 5
    assert heavy.tolist() == [3, 6, 7, 8, 9, 0, 1, 2, 4, 5, 10, 11]
    light = lm.coop_items(2, 3, qlen, 1000, cls, cost, lm.ITEMS_LIGHT)
    # keys 10, 63, 5, 63, 63, 0: pairs 5, 2, 0, then 1, 3, 4
    assert light.tolist() == [10, 11, 4, 5, 0, 1, 2, 3, 6, 7, 8, 9]
    some = lm.coop_items(2, 3, qlen, 1000, [0, COOP, 0, 0, 0, COOP | 2], cost)
    assert some.tolist() == [3, 10, 11]
    assert len(lm.coop_items(2, 3, qlen, 1000, [0] * 6, cost)) == 0


def test_a_pair_handed_back_keeps_the_class_it_was_moved_up_to():
    # 163 840 nt: forty wavefronts in class 0, 164 segments of 1000.  4097 nt: 65 segments of 64 -- two wavefronts --, 33 of 128 -- one.
    qlen = [163_840, 4097]
    out = lm.layout(1, 2, qlen, [-1], [COOP, LEFT], [40, 2], pair_cost=[7, 9], sub_cost=[1.0], struct_waves=14, route_all_few=1, route_seg=1000,
                    left=[0, 1])
    # all 42, struct 14: 42 >= 42, the suspected pair moves up to class 1; hard 2: 40 <= 42, the small call's wavefront kernel takes it
    assert out["rules"]["bump"] == (1, 0) and out["rules"]["take_all"] == (1, 0)
    assert out["pair_class"].tolist() == [COOP, COOP | 1] and out["pair_waves"].tolist() == [0, 0] and out["pair_wave0"].tolist() == [0, 0, 0]
    assert out["counts"].tolist() == _counts(STRUCT_WAVES=14, ALL_WAVES=42, SPARSE_WAVES=2, HARD_WAVES=2, ISLAND_WAVES=2, COOP_SEGS=169)
    assert out["items"].tolist() == list(range(164, 169)) + list(range(164))  # (cost 9 before cost 7)
    # handed back: in the second layout with the wavefronts of class 1 (class 0 would be two)
    assert out["pair_class2"].tolist() == [COOP, lm.L2 | 1] and out["pair_waves2"].tolist() == [0, 1] and out["pair_wave02"].tolist() == [0, 0, 1]
    assert out["route_nt"].tolist() == [163_840, 4097, 1]
    # nobody handed back: no pair in the second layout; a lane pair that carries the mark is not one either
    out = lm.layout(1, 2, qlen, [-1], [COOP, 0], [40, 2], pair_cost=[7, 9], route_seg=1000, left=[0, 1])
    assert out["pair_class2"].tolist() == [COOP, LEFT] and out["pair_waves2"].tolist() == [0, 0] and out["route_nt"].tolist() == [163_840, 4097, 0]
    # a self pair is never handed back
    out = lm.layout(1, 2, qlen, [0], [COOP, COOP], [0, 2], pair_cost=[7, 9], route_seg=1000, left=[1, 1])
    assert out["pair_class2"].tolist() == [COOP | LEFT, lm.L2] and out["pair_waves2"].tolist() == [0, 2] and out["route_nt"].tolist() == [0, 4097, 1]
