"""The layout kernels of a routed scan call (andi_amd/csrc/scan_lane.hip: k_pair_totals, k_pair_route, k_sub_order and their one-block twin
k_pair_layout_small; k_pair_block_sums, k_pair_block_offsets, k_pair_offsets; k_items, k_items_scan; k_pair_leftover, k_route_count) ALONE,
through a hook of the suite's library (andi_amd.Context.layout_kernels: arrays of the test's making in, every array those kernels write out),
against the NumPy model tests/layout_model.py -- every array exactly, k_lane_quad's list after sorting (its order is that of atomic additions).

The oracle cannot see most of this: a wrong class, offset or order changes which kernel runs and how long the call takes, never a count.  The
inputs come from a seeded generator (layout_model.draw) at the sizes where these kernels take another path; every test asserts FROM THE MODEL
that the rule or launch shape it is about was reached before it looks at the device.  A call of at most 1024 pairs runs twice, by
k_pair_layout_small and by the kernels of the larger calls: byte for byte the same."""
import functools

import numpy as np
import pytest

import andi_amd
import layout_model as lm
from conftest import SHIPPED_LIB

pytestmark = pytest.mark.gpu

STAGE1 = ("pair_class", "pair_waves", "pair_wave0", "sub_order", "counts", "items")
STAGE2 = ("pair_class2", "pair_waves2", "pair_wave02", "counts2", "route_nt")
DEFAULTS = dict(struct_waves=0, seg0=64, max_class=3, route_seg=2048, route_all_few=0, adaptive=1, items_order=lm.ITEMS_HEAVY, left=None)


@pytest.fixture(scope="module")
def dev():
    if SHIPPED_LIB:
        pytest.skip("andi_hip_test_layout_kernels is a test hook: not in the shipped library")
    c = andi_amd.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if want is not None:
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
        assert (got == want).all(), (what, np.nonzero(got != want)[0][:8].tolist())


def _device(dev, c, opt, allow_small):
    return dev.layout_kernels(c["nsub"], c["nq"], c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"], c["pair_cost"], c["sub_cost"],
                              allow_small=allow_small, **opt)


def _model(c, opt):
    return lm.layout(c["nsub"], c["nq"], c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"], c["pair_cost"], c["sub_cost"], **opt)


def held_to_model(dev, c, want=None, **kw):
    """one call of the hook against the model (want: the model's result where the test has it already), and -- at most 1024 pairs -- once more
    by the kernels of the larger calls against the first; returns (the model's result, the device's)"""
    opt = dict(DEFAULTS, **kw)
    want = _model(c, opt) if want is None else want
    P = c["nsub"] * c["nq"]
    got = _device(dev, c, opt, True)
    assert got["path"] == (1 if P <= 1024 else 2) and got["sort_launches"] == (1 if P <= 1024 else 3), (got["path"], got["sort_launches"])
    assert got["total_segs"] == lm.qseg_start(c["qlen"], opt["route_seg"])[-1]
    for k in STAGE1 + STAGE2:
        if k in STAGE1 or k in ("pair_class2", "route_nt") or opt["left"] is not None:
            _same(got[k], want.get(k), k)
    _same(np.sort(got["quad"]), want["quad"], "quad")
    if P <= 1024:
        twin = _device(dev, c, opt, False)
        assert twin["path"] == 2 and twin["sort_launches"] == 1
        for k in STAGE1 + STAGE2:
            _same(twin[k], got[k], "twin paths: " + k)
        _same(np.sort(twin["quad"]), np.sort(got["quad"]), "twin paths: quad")
    return want, got


@functools.lru_cache(maxsize=4)
def _drawn(nsub, nq, seed, short):
    return lm.draw(nsub, nq, seed, qlen=(100, 5000) if short else (100, 40_000))


# ------------------------------------------------------------------ launch shapes by the number of pairs
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13),  # a wavefront's edge
          1023: (31, 33), 1024: (32, 32),  # the one-block path
          1025: (25, 41), 2048: (32, 64), 2049: (3, 683), 4097: (17, 241),  # 2 to 5 blocks: sums and offsets by three kernels
          16385: (113, 145), 17 * 1024 + 1: (21, 829),  # k_items_scan: 64 x 17 and 64 x 18 entries, two per thread, threads beyond the table
          1025 * 1025: (1025, 1025)}  # k_pair_block_offsets: 1027 block sums, two per thread


@pytest.mark.parametrize("order", [lm.ITEMS_HEAVY, lm.ITEMS_LIGHT], ids=["heavy", "light"])
@pytest.mark.parametrize("adaptive", [1, 0])
@pytest.mark.parametrize("pairs", list(SHAPES))
def test_every_launch_shape(dev, pairs, adaptive, order):
    nsub, nq = SHAPES[pairs]
    assert nsub * nq == pairs
    c = dict(_drawn(nsub, nq, 100 + nsub, pairs > 5000))
    if pairs == 1:  # (the one pair is no self pair, and the wavefront kernel's)
        c = lm.draw(1, 1, 5, diagonal=None, p_cand=1.0, p_island=0.0, p_soft=0.0)
    nblocks = (pairs + 1023) // 1024
    if pairs >= 16385:
        assert lm.COST_CLASSES * nblocks > 1024  # k_items_scan takes more than one entry per thread ...
        assert -(-lm.COST_CLASSES * nblocks // 1024) * 1024 > lm.COST_CLASSES * nblocks  # ... and its last threads lie beyond the table
    if pairs == 1025 * 1025:
        assert nblocks > 1024
    want = _model(c, dict(DEFAULTS, adaptive=adaptive, items_order=order))
    assert len(want["items"]) > 0 and (pairs == 1 or (want["pair_waves"] > 0).any())
    if pairs > 64:  # (cost classes that differ: the two orders are two lists)
        assert (want["items"] != _model(c, dict(DEFAULTS, adaptive=adaptive, items_order=3 - order))["items"]).any()
    if adaptive and pairs > 1:
        assert len(want["quad"]) > 0
    held_to_model(dev, c, want, adaptive=adaptive, items_order=order)


# ------------------------------------------------------------------ the subjects' order
@pytest.mark.parametrize("nsub,nq", [(1, 5), (1024, 1), (1025, 1), (2500, 2), (8192, 2), (8193, 2)])
def test_subjects_order(dev, nsub, nq):
    """one block with a subject per thread (1024 x 1: k_pair_layout_small's copy), the strided loop, the last size that is ranked and the first
    that is not; ties in sub_cost, rows that are not the diagonal"""
    c = lm.draw(nsub, nq, 7 + nsub, diagonal=False, qlen=(100, 9000))
    assert nsub == 1 or ((c["self_q"] < 0).any() and (c["self_q"] >= 0).any())
    assert nsub == 1 or len(np.unique(c["sub_cost"])) < nsub  # ties
    want = _model(c, DEFAULTS)
    if 1 < nsub <= lm.RANKED_SUBJECTS:
        assert (want["sub_order"] != np.arange(nsub)).any() and sorted(want["sub_order"].tolist()) == list(range(nsub))
    else:
        assert (want["sub_order"] == np.arange(nsub)).all()
    held_to_model(dev, c, want)
    # a call without the order (and one without the list) leaves the rest as it is
    got = _device(dev, c, dict(DEFAULTS), True)
    bare = dev.layout_kernels(c["nsub"], c["nq"], c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"], None, None, sub_order=False, listed=False,
                              **{k: v for k, v in DEFAULTS.items() if k != "left"})
    assert bare["sub_order"] is None and bare["items"] is None and bare["sort_launches"] == 0
    for k in ("pair_class", "pair_waves", "pair_wave0", "pair_class2", "route_nt"):
        _same(bare[k], got[k], "without order and list: " + k)
    _same(bare["counts"], got["counts"], "without order and list: counts")


# ------------------------------------------------------------------ every rule of route_pair, fired and not
def _rule_sets():
    """name -> (draw's arguments, the hook's, what the model must say of the rules: rule -> (fired?, left alone?))"""
    few = dict(p_cand=0.99, p_island=0.0, p_soft=0.03)
    return {
        "lanes_not_few": (dict(), dict(), {"soft_back": (True, False), "pool": (True, True), "quad": (True, True)}),
        "lanes_few": (few, dict(), {"soft_back": (False, True)}),
        "guess_dropped": (dict(p_island=0.2, p_guess=0.3), dict(), {"guess_back": (True, False)}),
        "guess_kept": (dict(p_island=0.01, p_guess=0.3), dict(), {"guess_back": (False, True)}),
        "structured_max_class_3": (dict(p_island=0.3), dict(struct_waves="third"), {"bump": (True, True)}),
        "structured_max_class_0": (dict(p_island=0.3, max_class=0), dict(struct_waves="third", max_class=0), {"bump": (False, True)}),
        "not_structured": (dict(p_island=0.3), dict(struct_waves="below"), {"bump": (False, True)}),
        "small_take_all": (dict(p_cand=0.98, p_island=0.0), dict(route_all_few=1), {"take_all": (True, True), "soft_back": (False, True)}),
        "small_not_all": (dict(), dict(route_all_few=1), {"take_all": (False, True), "soft_back": (False, True)}),
    }


@pytest.mark.parametrize("nsub,nq", [(30, 33), (40, 57)], ids=["one_block", "several_kernels"])
@pytest.mark.parametrize("name", list(_rule_sets()))
def test_every_rule_of_the_routing(dev, name, nsub, nq):
    dargs, hargs, expect = _rule_sets()[name]
    c = lm.draw(nsub, nq, 31, **dargs)
    hargs = dict(hargs)
    if "struct_waves" in hargs:  # (a structured call: a third of the wavefronts, rounded up -- or one short of it)
        all_waves = lm.totals(c["pair_class"], c["pair_waves"])["all"]
        hargs["struct_waves"] = -(-all_waves // 3) - (hargs["struct_waves"] == "below")
    want = _model(c, dict(DEFAULTS, **hargs))
    for rule, (fired, spared) in expect.items():
        n_fired, n_spared = want["rules"][rule]
        assert (n_fired > 0) == fired and (not spared or n_spared > 0), (name, rule, want["rules"][rule])
        if fired and not spared:  # the rule holds for the call: it fires for every pair that carries its marks, and others carry none
            assert n_spared == 0 and n_fired < nsub * nq
    assert (want["pair_class"] & lm.COOP).any() and ((want["pair_waves"] > 0).any() or name == "small_take_all")  # (there the lanes keep nothing)
    held_to_model(dev, c, want, **hargs)


# ------------------------------------------------------------------ the list
LIST_QLEN = [100, 800, 900, 6400, 6500, 20_000]  # 1, 8, 9, 64, 65 and 200 segments of 100: a thread's own writes, all lanes' writes, strided


@pytest.mark.parametrize("order", [lm.ITEMS_HEAVY, lm.ITEMS_LIGHT], ids=["heavy", "light"])
@pytest.mark.parametrize("nsub", [40, 400], ids=["one_block", "several_kernels"])
@pytest.mark.parametrize("kind", ["mixed", "none", "all"])
def test_list_entry_by_entry(dev, kind, nsub, order):
    """the stable order scan.h promises -- pairs by cost class, pairs of one class in slot order, a pair's segments in theirs --, queries of one
    segment and of hundreds in one call, a cost beyond the classes, a list of nothing and a list of every pair"""
    rates = {"mixed": dict(), "none": dict(p_cand=0.0), "all": dict(p_cand=1.0, p_island=0.0, p_soft=0.0, diagonal=None)}[kind]
    c = lm.draw(nsub, len(LIST_QLEN), 77, qlen=LIST_QLEN, cost=(0, 8), **rates)  # (few classes: many pairs share one)
    c["pair_cost"][::7] = 200  # beyond the 64 classes: the heaviest
    want = _model(c, dict(DEFAULTS, route_seg=100, items_order=order))
    segs = np.diff(lm.qseg_start(LIST_QLEN, 100))
    assert segs.tolist() == [1, 8, 9, 64, 65, 200]
    n_coop = int(((want["pair_class"] & lm.COOP) != 0).sum())
    assert {"mixed": 0 < n_coop < nsub * 6, "none": n_coop == 0, "all": n_coop == nsub * 6}[kind]
    assert len(want["items"]) == (0 if kind == "none" else segs.sum() * nsub if kind == "all" else len(want["items"]))
    if kind != "none":
        coop = np.nonzero(want["pair_class"] & lm.COOP)[0]
        assert set((coop % 6).tolist()) == set(range(6)) and (c["pair_cost"][coop] == 200).any()
    held_to_model(dev, c, want, route_seg=100, items_order=order)


# ------------------------------------------------------------------ the pairs handed back, and who took what
def _masks(want, rng):
    coop = (want["pair_class"] & lm.COOP) != 0
    P = len(coop)
    return {"none": np.zeros(P, bool), "some": (rng.random(P) < 0.4) | (P == 1), "all": np.ones(P, bool)}, coop


@pytest.mark.parametrize("mask", ["none", "some", "all"])
@pytest.mark.parametrize("nsub,nq", [(1, 1), (15, 17), (16, 16), (1, 257), (17, 241)], ids=["p1", "p255", "p256", "p257", "p4097"])
def test_pairs_handed_back(dev, nsub, nq, mask):
    """k_pair_leftover's and k_route_count's blocks of 256 at their edges: no pair, some and all of the wavefront kernel's pairs handed back (the
    marks fall on lane pairs and self pairs too: those are nobody's to hand back)"""
    c = lm.draw(nsub, nq, 5, diagonal=None, p_cand=1.0, p_island=0.0, p_soft=0.0) if nsub * nq == 1 else lm.draw(nsub, nq, 900 + nq)
    want = _model(c, DEFAULTS)
    masks, coop = _masks(want, np.random.default_rng(3))
    left = masks[mask]
    assert coop.any() and (nsub * nq == 1 or ((left & coop).any() == (mask != "none") and (mask != "some" or (~left & coop).any())))
    for adaptive in (1, 0):
        want = _model(c, dict(DEFAULTS, left=left, adaptive=adaptive))
        assert ((want["pair_class2"] & lm.L2) != 0).sum() == (left & coop & (want["pair_waves2"] > 0)).sum() == want["route_nt"][2]
        assert (want["route_nt"][2] > 0) == (mask != "none")
        held_to_model(dev, c, want, left=left, adaptive=adaptive)


@pytest.mark.parametrize("nsub,nq", [(1, 257), (17, 241)], ids=["p257", "p4097"])
def test_a_pair_handed_back_after_its_class_was_moved_up(dev, nsub, nq):
    """a structured small call: a suspected pair of the lanes moves up a class, the wavefront kernel takes it with every other pair and hands
    it back -- its wavefronts in the second layout are those of the class it was moved up to"""
    c = lm.draw(nsub, nq, 41, diagonal=None, p_cand=1.0, p_island=0.03, p_soft=0.0, max_class=2)  # (the suspected pairs few: the lanes' pairs are)
    all_waves = lm.totals(c["pair_class"], c["pair_waves"])["all"]
    opt = dict(DEFAULTS, struct_waves=all_waves, route_all_few=1)
    want = _model(c, opt)
    moved = (want["pair_class"] & 3) > (c["pair_class"] & 3)
    assert want["rules"]["bump"][0] == moved.sum() > 0 and want["rules"]["take_all"][0] > 0 and ((want["pair_class"][moved] & lm.COOP) != 0).all()
    left = moved.copy()
    left[::3] = True
    want = _model(c, dict(opt, left=left))
    back = (want["pair_class2"] & lm.L2) != 0
    assert back[moved].all() and (back & ~moved).any() and (~back).any()
    assert (want["pair_waves2"][moved] == lm.waves_of(c["qlen"][np.nonzero(moved)[0] % nq], 64 << (want["pair_class"][moved].astype(np.int64) & 3))).all()
    assert (want["pair_waves2"][moved] != c["pair_waves"][moved]).any()  # (not the wavefronts they came with)
    held_to_model(dev, c, want, **dict(opt, left=left))


# ------------------------------------------------------------------ the hook itself
def test_two_calls_on_one_context_give_the_same_bytes(dev):
    c, other = lm.draw(25, 41, 12), lm.draw(40, 57, 13)
    left = np.random.default_rng(1).random(25 * 41) < 0.3
    first = _device(dev, c, dict(DEFAULTS, left=left), True)
    held_to_model(dev, other)
    second = _device(dev, c, dict(DEFAULTS, left=left), True)
    for k in STAGE1 + STAGE2:
        _same(second[k], first[k], k)
    _same(np.sort(second["quad"]), np.sort(first["quad"]), "quad")


def test_bad_arguments_are_refused_and_the_context_stays_usable(dev):
    c = lm.draw(5, 13, 3)
    good = dict(DEFAULTS)

    def call(case=c, **kw):
        return _device(dev, case, dict(good, **kw), True)

    for kw in (dict(seg0=0), dict(seg0=1 << 29), dict(max_class=4), dict(route_seg=0), dict(adaptive=2), dict(route_all_few=2), dict(items_order=0),
               dict(items_order=3)):
        with pytest.raises(andi_amd.AndiHipError):
            call(**kw)
    args = (c["nsub"], c["nq"], c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"])
    with pytest.raises(andi_amd.AndiHipError):  # a list without the pairs' cost classes
        dev.layout_kernels(*args, None, c["sub_cost"])
    with pytest.raises(andi_amd.AndiHipError):  # an order without the subjects' costs
        dev.layout_kernels(*args, c["pair_cost"], None)
    with pytest.raises(andi_amd.AndiHipError):  # nsub * nq does not fit 32 bits
        dev.layout_kernels(1 << 16, 1 << 16, c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"], c["pair_cost"], c["sub_cost"])
    with pytest.raises(andi_amd.AndiHipError):  # no pairs
        dev.layout_kernels(0, 13, c["qlen"], c["self_q"], c["pair_class"], c["pair_waves"], c["pair_cost"], c["sub_cost"])
    long_q = dict(c, qlen=np.full(13, 0xffffffff, np.uint32))
    with pytest.raises(andi_amd.AndiHipError):  # more segments than 32 bits count
        call(long_q, route_seg=1)
    held_to_model(dev, c)
