"""A plain NumPy model of the layout kernels of a routed scan call (andi_amd/csrc/scan_lane.hip: k_pair_totals, k_pair_route, k_sub_order,
k_pair_layout_small, the three kernels of the offsets, k_items / k_items_scan, k_pair_leftover, k_route_count), written from the contracts
in andi_amd/csrc/scan.h and the comments on those kernels -- whole arrays at a time, no threads, blocks or wavefronts.  They are pure
integer functions of what k_pair_estimate leaves behind, so everything here compares exactly; a million pairs take a second or two.

A pair is subject * nq + query.  Its class byte: bits 0-1 the segment length's class (segments of seg0 << class), bit 7 k_lane_quad's pair,
and the routing's bits below.  Used by tests/test_layout_model_host.py (no GPU) and tests/test_layout_kernels_gpu.py."""
import numpy as np

QUAD, COOP, LEFT, SOFT, L2, POOLCAND, GUESS = 0x80, 0x40, 0x20, 0x10, 0x08, 0x08, 0x04  # scan.h: ANDI_ROUTE_*
STRUCT_WAVES, POOL_SEGS, COOP_SEGS, HARD_WAVES, LANE_WAVES, ISLAND_WAVES, QUAD_WAVES, SPARSE_WAVES, ALL_WAVES = 4, 6, 7, 9, 10, 11, 13, 14, 15
COST_CLASSES = 64
ITEMS_HEAVY, ITEMS_LIGHT = 1, 2
RANKED_SUBJECTS = 8192  # more subjects than this are taken as they come
RULES = ("soft_back", "guess_back", "bump", "take_all", "pool", "quad")


def waves_of(qlen, seg):
    """wavefronts of a pair: its segments, 64 to a wavefront"""
    qlen = np.asarray(qlen, np.int64)
    return ((qlen + seg - 1) // seg + 63) // 64


def qseg_start(qlen, seg):
    """the segmentation of the queries at one segment length: where every query's segments start, and (last) their number"""
    return np.concatenate([[0], np.cumsum((np.asarray(qlen, np.int64) + seg - 1) // seg)])


def totals(cls, waves):
    """the four sums the routing decides by: wavefronts of all pairs; of those the lane scan would like (soft, or not marked for the
    wavefront kernel); of those that kernel is no candidate for; of those in which the sampling saw unrelated stretches"""
    cls, waves = np.asarray(cls, np.int64), np.asarray(waves, np.int64)
    coop, soft, left = (cls & COOP) != 0, (cls & SOFT) != 0, (cls & LEFT) != 0
    return {"all": int(waves.sum()), "sparse": int(waves[soft | ~coop].sum()), "hard": int(waves[~coop].sum()), "island": int(waves[left].sum())}


def _pairs(nsub, nq, self_q):
    pair = np.arange(nsub * nq, dtype=np.int64)
    sub, q = pair // nq, pair % nq
    return sub, q, np.asarray(self_q, np.int64)[sub] == q


def route(nsub, nq, qlen, self_q, pair_class, pair_waves, struct_waves, seg0, max_class, route_seg, route_all_few):
    """k_pair_totals and k_pair_route (route_pair): returns (pair_class, pair_waves, counts[16], rules) -- rules[name] = (pairs the rule
    fired for, pairs that met the rule's own marks and were left as they were), for the names in RULES but "quad"."""
    qlen = np.asarray(qlen, np.int64)
    sub, q, is_self = _pairs(nsub, nq, self_q)
    cls, waves = np.asarray(pair_class, np.int64).copy(), np.asarray(pair_waves, np.int64).copy()
    t = totals(cls, waves)
    rules = {}
    # soft pairs go back to the lanes unless the lanes' pairs are few or the call is small
    cand = ((cls & COOP) != 0) & ((cls & SOFT) != 0)
    fire = cand & (not (10 * t["sparse"] <= t["all"])) & (not route_all_few)
    cls[fire] &= ~COOP
    rules["soft_back"] = (int(fire.sum()), int((cand & ~fire).sum()))
    # pairs the sampling could not judge go back where a twentieth of the call shows unrelated stretches
    cand = ((cls & GUESS) != 0) & ((cls & COOP) != 0)
    fire = cand & (20 * t["island"] > t["all"])
    cls[fire] &= ~COOP
    rules["guess_back"] = (int(fire.sum()), int((cand & ~fire).sum()))
    # a call of structured genomes: the suspected pairs of the lanes get segments twice as long
    cand = ((cls & (LEFT | GUESS)) != 0) & ((cls & COOP) == 0)
    fire = cand & ((cls & 3) < max_class) & (3 * struct_waves >= t["all"])
    cls[fire] += 1
    waves[fire] = waves_of(qlen[q[fire]], seg0 << (cls[fire] & 3))
    rules["bump"] = (int(fire.sum()), int((cand & ~fire).sum()))
    pool = (cls & POOLCAND) != 0
    cls &= ~(SOFT | LEFT | GUESS | POOLCAND)
    # small calls: where the lane scan's pairs would be few, the wavefront kernel takes every pair but the self pairs
    cand = (cls & COOP) == 0
    fire = cand & bool(route_all_few) & (20 * t["hard"] <= t["all"]) & ~is_self
    cls[fire] |= COOP
    rules["take_all"] = (int(fire.sum()), int((cand & ~fire).sum()))
    coop = (cls & COOP) != 0
    segs = (qlen[q] + route_seg - 1) // route_seg
    rules["pool"] = (int((coop & pool).sum()), int((coop & ~pool).sum()))
    waves[coop] = 0
    counts = np.zeros(16, np.int64)
    counts[STRUCT_WAVES], counts[ALL_WAVES], counts[SPARSE_WAVES], counts[HARD_WAVES], counts[ISLAND_WAVES] = struct_waves, t["all"], t["sparse"], t["hard"], t["island"]
    counts[COOP_SEGS], counts[POOL_SEGS], counts[LANE_WAVES] = segs[coop].sum(), segs[coop & pool].sum(), waves.sum()
    return cls.astype(np.uint8), waves.astype(np.uint32), counts, rules


def sub_order(sub_cost):
    """the subjects by falling float32 cost, ties by index; as they come from RANKED_SUBJECTS + 1 on"""
    c = np.asarray(sub_cost, np.float32)
    if len(c) > RANKED_SUBJECTS:
        return np.arange(len(c), dtype=np.uint32)
    return np.argsort(-c.astype(np.float64), kind="stable").astype(np.uint32)


def offsets(pair_waves):
    """pair_wave0: the exclusive running sum, the total behind the last pair"""
    return np.concatenate([[0], np.cumsum(np.asarray(pair_waves, np.int64))]).astype(np.uint32)


def _runs(first, n):
    """first[k], first[k] + 1, ..., first[k] + n[k] - 1 for every k, one behind the other"""
    first, n = np.asarray(first, np.int64), np.asarray(n, np.int64)
    begin = np.cumsum(n) - n
    return np.repeat(first - begin, n) + np.arange(int(n.sum()), dtype=np.int64)


def quad_list(pair_class, pair_waves, pair_wave0):
    """k_lane_quad's list, SORTED (on the device its order is that of atomic additions): the wavefronts of every pair with bit 7 that has some"""
    cls, waves = np.asarray(pair_class, np.int64), np.asarray(pair_waves, np.int64)
    on = ((cls & QUAD) != 0) & (waves > 0)
    return np.sort(_runs(np.asarray(pair_wave0, np.int64)[:-1][on], waves[on])).astype(np.uint32)


def coop_items(nsub, nq, qlen, route_seg, pair_class, pair_cost, items_order=ITEMS_HEAVY):
    """scan.h: coop_items -- the segments (subject * total_segs + segment) of the pairs marked for the wavefront kernel, the pairs sorted
    stably by cost class, heaviest first (ITEMS_LIGHT: lightest first), a pair's segments in their order"""
    start = qseg_start(qlen, route_seg)
    pairs = np.nonzero((np.asarray(pair_class, np.int64) & COOP) != 0)[0]
    cost = np.minimum(np.asarray(pair_cost, np.int64)[pairs], COST_CLASSES - 1)
    key = cost if items_order == ITEMS_LIGHT else COST_CLASSES - 1 - cost
    pairs = pairs[np.argsort(key, kind="stable")]
    sub, q = pairs // nq, pairs % nq
    return _runs(sub * start[-1] + start[q], start[q + 1] - start[q]).astype(np.uint32)


def leftover(nsub, nq, qlen, self_q, pair_class, seg0):
    """k_pair_leftover: a pair of the wavefront kernel that was handed back (COOP and LEFT, no self pair) is in the second lane layout (L2),
    with the wavefronts of its own class; every other pair has none there.  Returns (pair_class, the second layout's pair_waves)."""
    sub, q, is_self = _pairs(nsub, nq, self_q)
    cls = np.asarray(pair_class, np.int64).copy()
    back = ((cls & COOP) != 0) & ((cls & LEFT) != 0) & ~is_self
    cls[back] = (cls[back] & ~(COOP | LEFT)) | L2
    waves = np.zeros(nsub * nq, np.int64)
    waves[back] = waves_of(np.asarray(qlen, np.int64)[q[back]], seg0 << (cls[back] & 3))
    return cls.astype(np.uint8), waves.astype(np.uint32)


def route_nt(nsub, nq, qlen, self_q, pair_class):
    """k_route_count: query nucleotides of the wavefront kernel's pairs, of the others, and the pairs handed back; no self pair counts"""
    sub, q, is_self = _pairs(nsub, nq, self_q)
    cls, n = np.asarray(pair_class, np.int64), np.asarray(qlen, np.int64)[q]
    coop = (cls & COOP) != 0
    return np.array([n[coop & ~is_self].sum(), n[~coop & ~is_self].sum(), (((cls & L2) != 0) & ~is_self).sum()], np.uint64)


def layout(nsub, nq, qlen, self_q, pair_class, pair_waves, pair_cost=None, sub_cost=None, *, struct_waves=0, seg0=64, max_class=3, route_seg=2048,
           route_all_few=0, adaptive=1, items_order=ITEMS_HEAVY, left=None):
    """Everything one call of the suite's hook (andi_amd.Context.layout_kernels) returns, under the same names; plus rules (RULES)."""
    cls, waves, counts, rules = route(nsub, nq, qlen, self_q, pair_class, pair_waves, struct_waves, seg0, max_class, route_seg, route_all_few)
    out = {"pair_class": cls, "pair_waves": waves, "pair_wave0": None, "sub_order": None if sub_cost is None else sub_order(sub_cost),
           "quad": np.zeros(0, np.uint32), "items": None, "rules": rules}
    if adaptive:
        out["pair_wave0"] = offsets(waves)
        out["quad"] = quad_list(cls, waves, out["pair_wave0"])
        counts[QUAD_WAVES] = len(out["quad"])
        on = (waves > 0) & ((cls & QUAD) != 0)
        rules["quad"] = (int(on.sum()), int(((waves > 0) & ~on).sum()))
    if pair_cost is not None:
        out["items"] = coop_items(nsub, nq, qlen, route_seg, cls, pair_cost, items_order)
        assert len(out["items"]) == counts[COOP_SEGS]
    out["counts"] = counts.astype(np.uint32)
    cls2 = cls
    if left is not None:
        marked = cls | np.where(np.asarray(left) != 0, LEFT, 0).astype(np.uint8)
        cls2, waves2 = leftover(nsub, nq, qlen, self_q, marked, seg0)
        out["pair_waves2"], out["pair_wave02"], counts2 = waves2, None, np.zeros(16, np.uint32)
        if adaptive:
            out["pair_wave02"] = offsets(waves2)
            out["quad2"] = quad_list(cls2, waves2, out["pair_wave02"])
            counts2[QUAD_WAVES] = len(out["quad2"])
        out["counts2"] = counts2
    out["pair_class2"], out["route_nt"] = cls2, route_nt(nsub, nq, qlen, self_q, cls2)
    return out


def draw(nsub, nq, seed, *, seg0=64, max_class=3, qlen=(100, 40_000), p_cand=0.6, p_island=0.1, p_soft=0.2, p_guess=0.1, p_pool=0.3, p_quad=0.2,
         diagonal=True, cost=(0, 64)):
    """A seeded call as k_pair_estimate could leave it: qlen, self, pair_class (a candidate of the wavefront kernel is marked for it, or --
    unrelated stretches seen -- LEFT; soft, guessed, pool candidates and k_lane_quad's pairs at the given rates; a class of 0 .. max_class),
    pair_cost, pair_waves to match (segments of seg0 << class, 64 to a wavefront), sub_cost with ties; self pairs all zero.  qlen: a range to
    draw from, or the lengths themselves.  diagonal: subject s is query s where there is one; False: rows that are not the diagonal -- about
    half of the subjects have a query of their own, any one; None: no subject has."""
    rng = np.random.default_rng(seed)
    P = nsub * nq
    ql = (rng.integers(qlen[0], qlen[1] + 1, nq) if isinstance(qlen, tuple) else np.asarray(qlen)).astype(np.uint32)
    assert ql.shape == (nq,)
    self_q = np.where(np.arange(nsub) < nq, np.arange(nsub), -1).astype(np.int64)
    if not diagonal:
        self_q = np.where((rng.random(nsub) < 0.5) & (diagonal is not None), rng.integers(0, nq, nsub), -1).astype(np.int64)
    sub, q, is_self = _pairs(nsub, nq, self_q)
    cand, isl = rng.random(P) < p_cand, rng.random(P) < p_island
    cls = rng.integers(0, max_class + 1, P)
    cls |= np.where(cand & ~isl, COOP, 0) | np.where(cand & isl, LEFT, 0) | np.where(cand & (rng.random(P) < p_guess), GUESS, 0)
    cls |= np.where(rng.random(P) < p_soft, SOFT, 0) | np.where(rng.random(P) < p_pool, POOLCAND, 0) | np.where(rng.random(P) < p_quad, QUAD, 0)
    cost = rng.integers(cost[0], cost[1], P)
    waves = waves_of(ql[q], seg0 << (cls & 3))
    cls[is_self], cost[is_self], waves[is_self] = 0, 0, 0
    sub_cost = rng.integers(0, max(2, nsub // 2), nsub).astype(np.float32) * np.float32(0.37)  # (ties: about two subjects per value)
    return {"nsub": nsub, "nq": nq, "qlen": ql, "self_q": self_q, "pair_class": cls.astype(np.uint8), "pair_waves": waves.astype(np.uint32),
            "pair_cost": cost.astype(np.uint8), "sub_cost": sub_cost}
