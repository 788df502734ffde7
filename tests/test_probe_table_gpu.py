"""The probe table of the scan index (esa_build.hip: k_probe_table, k_probe_table_batch) entry by entry against the model
of tests/probe_table_model.py (itself checked on the CPU: tests/test_probe_table_model_host.py): every depth, every form
of the once-occurring entries, suffix arrays from the host and from the device, one subject per launch and many, and the
closed-run flag that sends a subject to the reference's own walk."""
import contextlib
import functools

import numpy as np
import pytest

import probe_table_model as ptm
from conftest import knobs, rand_dna

pytestmark = pytest.mark.gpu

# what decides the form of the once-occurring entries (esa_build.hip: andi_index_single_ext): the switch ANDI_COOP, the
# queries the context expects, and where the suffix array was made -- setting: (ANDI_COOP, queries, form by origin)
SETTINGS = {
    "default": (None, 0, {"host": 0, "device": 2}),
    "coop-off": (0, 0, {"host": 0, "device": 0}),
    "coop-4": (4, 0, {"host": 1, "device": 2}),
    "256-queries": (None, 256, {"host": 1, "device": 2}),
}
DEPTHS = ["natural", 4, 5, 6, 7, 8, 9, 10]
ORIGINS = ("host", "device")


@functools.lru_cache(None)
def _subjects():
    from andi_amd import synth
    rng = np.random.default_rng(33)
    s = {}
    s["tiny"] = b"ACGTTGCA"
    s["homopolymer"] = b"A" * 700
    s["two-letter"] = rand_dna(rng, 2500, b"AC")
    s["repeats"] = rand_dna(rng, 300) * 6 + rand_dna(rng, 200)
    s["joined"] = synth.join_contigs(rand_dna(rng, 3000), 9)
    s["short-contigs"] = b"!".join([b"ACG", b"ACGT", b"AC", b"ACGTA", b"ACG"] * 30)
    s["poly-a-at-separators"] = b";".join([b"GATTACA" + b"A" * k for k in range(0, 30)] * 2)
    s["same-contig-ends"] = b"!".join([rand_dna(rng, 40 + 5 * k) + b"ACGTTGCAACGTAC" for k in range(30)])
    s["random-16-tiles"] = rand_dna(rng, 6000)
    for n in (383, 384, 767, 768):  # RS of 767, 769, 1535, 1537 characters: the gaps fill one or two tiles exactly, or run one or two over
        s["length-%d" % n] = rand_dna(rng, n)
    s["run-lengths"] = ptm.run_lengths_text()[0]
    s["single-ends"] = ptm.single_ends_text()[0]
    s["acgt-x-2000"] = b"ACGT" * 2000
    return s


@functools.lru_cache(None)
def _texts():
    """name -> RS.  RS = revcomp(S) '#' S has an odd length; two texts of 768 and 1536 characters besides (staged as
    prepared texts): their last gap is the first of a block of its own, the one k_probe_table_batch's early return must
    let through."""
    t = {name: ptm.subject_text(seq) for name, seq in _subjects().items()}
    t["text-768"] = t["length-383"] + b"T"
    t["text-1536"] = t["length-767"] + b"!"
    return t


def _batch_order():
    """the shortest and the longest are neighbours: shortest, longest, second shortest, second longest ..."""
    by_len = sorted(_texts(), key=lambda k: len(_texts()[k]))
    out = []
    while by_len:
        out.append(by_len.pop(0))
        if by_len:
            out.append(by_len.pop())
    return out


@functools.lru_cache(None)
def _host_sa(name):
    import andi_amd
    return andi_amd.suffix_array(_texts()[name])


_models = {"K": None}  # the models of one depth at a time (at K = 10 a table's words are 9 MB per subject and form)


def _model(name, K):
    """(kind, x, x_defined, y by form) of every code of the subject at depth K"""
    if _models["K"] != K:
        _models.clear()
        _models["K"] = K
    if name not in _models:
        rs = _texts()[name]
        E = ptm.entries(rs, K)
        assert not (E.kind == 3).any()
        ys = {}
        for form in (0, 1, 2):
            x, ys[form], defined = ptm.table(rs, E, form)
        _models[name] = (E.kind.astype(np.uint8), x, defined, ys, ptm.closed_run_flag(rs))
    return _models[name]


@pytest.fixture(scope="module", autouse=True)
def _models_freed():
    yield
    _models.clear()


def _depth_of(name, depth):
    return ptm.natural_k(len(_texts()[name])) if depth == "natural" else depth


@contextlib.contextmanager
def _setting(ctx, setting, depth):
    coop, queries, forms = SETTINGS[setting]
    with knobs(COOP=coop, DEEP_K=None if depth == "natural" else depth):
        ctx.expect_queries(queries)
        try:
            yield forms
        finally:
            ctx.expect_queries(0)


def _stage(ctx, name, origin):
    import andi_amd
    sa = "device" if origin == "device" else _host_sa(name)
    if name in _subjects():
        E = andi_amd.Esa(ctx, _subjects()[name], sa=sa, build=False)
    else:
        E = andi_amd.Esa(ctx, None, build=False, prepared=(_texts()[name], 0.5, 8, sa))
    assert E.RS == _texts()[name]
    return E


def _check_against_model(E, name, K, form, what):
    kind, x, defined, ys, flag = _model(name, K)
    k, table = E.download_index()
    assert k == K and E.single_form() == form, what
    bad = np.flatnonzero(table[:, 1] != ys[form])
    assert len(bad) == 0, (what, "y of codes", bad[:5], table[bad[:5], 1], ys[form][bad[:5]])
    bad = np.flatnonzero((table[:, 0] != x) & defined)
    assert len(bad) == 0, (what, "x of codes", bad[:5], table[bad[:5], 0], x[bad[:5]])
    assert E.flags()[0] == flag, (what, "closed-run flag")
    return table


def test_subjects_have_the_properties_they_are_built_for():
    """from the texts alone: every kind of entry and every regime of the kernel really occurs"""
    subjects = _subjects()
    facts = ptm.run_lengths_facts(subjects["run-lengths"])
    assert set(ptm.RUN_COUNTS) <= facts["counts"] and facts["longest"] >= 1000
    assert facts["short_at_tile_end"] and facts["long_at_tile_end"]
    facts = ptm.single_ends_facts(subjects["single-ends"])
    assert {0, ord("#"), ord("!"), ord(";")} <= facts["ends_at"] and set(ptm.BEHIND) <= facts["behind"] and facts["far"]
    assert [2 * len(subjects["length-%d" % n]) + 1 - ptm.TILE * t for n, t in ((383, 1), (384, 1), (767, 2), (768, 2))] == [-1, 1, -1, 1]
    kinds = set()
    for name, seq in subjects.items():
        E = ptm.entries(ptm.subject_text(seq), ptm.natural_k(2 * len(seq) + 1))
        kinds |= {(int(k), int(u)) for k, u in zip(E.kind, E.unique)}
    assert kinds == {(ptm.FINAL, 0), (ptm.FINAL, 1), (ptm.SINGLE, -1), (ptm.MULTI, -1)}
    E = ptm.entries(ptm.subject_text(subjects["acgt-x-2000"]), 7)
    assert E.count[E.kind != ptm.FINAL].min() >= 1000  # every K-mer that occurs is a long run


# every setting at the natural depth and at K = 4, 8 and 10; the depths between them with the default switches (form 2 from
# the device's suffix arrays, form 0 from the host's) -- the whole cross product took the module past twice the time of
# tests/test_esa_gpu.py
MATRIX = [(d, s) for d in DEPTHS for s in SETTINGS if s == "default" or d in ("natural", 4, 8, 10)]


@pytest.mark.parametrize("depth,setting", MATRIX, ids=["K-%s-%s" % m for m in MATRIX])
def test_every_entry_single_launch_and_batch(ctx, depth, setting):
    """Every entry of every subject's table and its closed-run flag against the model: the subject alone (k_probe_table),
    suffix array from the host (records by one gather per suffix) and from the device (the sorter's records); and in a
    batch of all subjects (k_probe_table_batch), lengths mixed, host-made and device-made suffix arrays alternating --
    byte for byte the table of the single launch."""
    import andi_amd
    order = _batch_order()
    with _setting(ctx, setting, depth) as forms:
        single = {(name, o): _stage(ctx, name, o) for name in order for o in ORIGINS}
        for E in single.values():
            E.build()
        batches = []
        for flip in (0, 1):  # each subject once with either origin, neighbours of different origin
            batch = {name: _stage(ctx, name, ORIGINS[(k + flip) % 2]) for k, name in enumerate(order)}
            andi_amd.lib.build_indexes(ctx, list(batch.values()))
            batches.append(batch)
    for k, name in enumerate(order):
        K = _depth_of(name, depth)
        tables = {o: _check_against_model(single[name, o], name, K, forms[o], (name, o, "single")) for o in ORIGINS}
        for flip, batch in enumerate(batches):
            o = ORIGINS[(k + flip) % 2]
            k2, table = batch[name].download_index()
            assert k2 == K and batch[name].single_form() == forms[o]
            assert (table == tables[o]).all(), (name, o, "batch != single launch")
            assert batch[name].flags()[0] == _model(name, K)[4]
    for E in list(single.values()) + [E for b in batches for E in b.values()]:
        E.close()


@pytest.mark.parametrize("depth", DEPTHS, ids=["K-%s" % d for d in DEPTHS])
def test_forms_and_origins_agree(ctx, depth):
    """Byte-for-byte equalities between builds of one subject (what catches a wrong record from the sorter or a wrong
    gather): form 0 from a host-made suffix array == form 0 from a device-made one, the whole table, the x of FINAL entries
    that are not unique included; forms 0, 1 and 2 differ only in y of SINGLE entries; form 2's extension is form 1's cut to
    min(4, 16 - K) symbols."""
    built = {}
    for setting, origin in (("coop-off", "host"), ("coop-off", "device"), ("coop-4", "host"), ("coop-4", "device")):
        with _setting(ctx, setting, depth) as forms:
            for name in _texts():
                E = _stage(ctx, name, origin)
                E.build()
                built[name, forms[origin], origin] = E
    for name in _texts():
        K = _depth_of(name, depth)
        t0 = built[name, 0, "host"].download_index()[1]
        assert (built[name, 0, "device"].download_index()[1] == t0).all(), name
        t1, t2 = built[name, 1, "host"].download_index()[1], built[name, 2, "device"].download_index()[1]
        one = (t0[:, 1] & 3) == ptm.SINGLE
        for t in (t1, t2):
            assert (t[:, 0] == t0[:, 0]).all() and (t[~one, 1] == t0[~one, 1]).all() and ((t[one, 1] & 3) == ptm.SINGLE).all(), name
        room = ptm.form_room(2, K)
        n1, e1 = (t1[one, 1] >> 2) & 15, t1[one, 1] >> 6
        n2, e2 = (t2[one, 1] >> 2) & 15, t2[one, 1] >> 6
        assert (n2 == np.minimum(n1, room)).all() and (e2 == (e1 & ((1 << (2 * n2)) - 1))).all(), name
    for E in built.values():
        E.close()


@functools.lru_cache(None)
def _deep_codes(name, K):
    """every code that occurs in the text, its two neighbours, the first and the last code, 200 000 random ones"""
    present = ptm.present_codes(_texts()[name], K)
    rng = np.random.default_rng(K)
    codes = np.concatenate([present, present - 1, present + 1, [0, 4 ** K - 1], rng.integers(0, 4 ** K, 200000)])
    return np.unique(codes[(codes >= 0) & (codes < 4 ** K)])


@pytest.mark.parametrize("K", [11, 12, 13])
def test_deep_tables_by_list_of_codes(ctx, K):
    """K = 11, 12, 13 (tables of 4^K entries from texts of a few hundred characters: nearly every entry an absent code's)
    on two small subjects, by the model's list-of-codes back end: form 2 alone and forms 1 and 2 in one batch at every
    depth, forms 0 and 1 alone at K = 11 (a table of K = 13 is 512 MB to fetch)."""
    import andi_amd
    for name in ("single-ends", "length-384"):
        rs = _texts()[name]
        codes = _deep_codes(name, K)
        E = ptm.entries(rs, K, codes)
        assert {ptm.FINAL, ptm.SINGLE} <= set(E.kind.tolist())
        flag = ptm.closed_run_flag(rs)
        for setting, origin in (("default", "device"), ("coop-4", "batch")) + ((("coop-off", "host"), ("coop-4", "host")) if K == 11 else ()):
            with _setting(ctx, setting, K) as forms:
                if origin == "batch":
                    esas = [_stage(ctx, name, "host"), _stage(ctx, "tiny", "device"), _stage(ctx, name, "device")]
                    andi_amd.lib.build_indexes(ctx, esas)
                    esas = [(esas[0], forms["host"]), (esas[2], forms["device"])]
                else:
                    esas = [(_stage(ctx, name, origin), forms[origin])]
                    esas[0][0].build()
            for G, form in esas:
                k, table = G.download_index()
                x, y, defined = ptm.table(rs, E, form)
                assert k == K and G.single_form() == form
                assert (table[codes, 1] == y).all() and (table[codes, 0] == x)[defined].all(), (name, setting, origin)
                assert G.flags()[0] == flag
                del table
                G.close()


@pytest.mark.parametrize("origin,coop", [("device", None), ("host", 4)])
def test_a_thousand_queries_deepen_the_table_by_one(ctx, origin, coop):
    """expect_queries(1024): natural K + 1 -- byte for byte the table that ANDI_DEEP_K = K + 1 gives without the hint"""
    tables = {}
    try:
        for name in ("single-ends", "joined", "run-lengths", "length-768"):
            K = _depth_of(name, "natural")
            with knobs(COOP=coop):
                ctx.expect_queries(1024)
                E = _stage(ctx, name, origin)
                E.build()
                tables[name] = E.download_index()
                form = E.single_form()
                E.close()
            assert tables[name][0] == K + 1 and form == (2 if origin == "device" else 1)
            ctx.expect_queries(0)
            with knobs(COOP=coop, DEEP_K=K + 1):
                E = _stage(ctx, name, origin)
                E.build()
                k, table = E.download_index()
                assert k == K + 1 and E.single_form() == form
                assert (table == tables[name][1]).all(), name
                _check_against_model(E, name, K + 1, form, (name, origin, "hinted"))
                E.close()
    finally:
        ctx.expect_queries(0)


# ---------------------------------------------------------------- the closed-run flag and the scan behind it
def _tails(rng, w):
    """queries that start with w and go on past the 10-mer table's reach"""
    return [w + bytes(t) + rand_dna(rng, 14) for t in (b"", b"A", b"C", b"G", b"T", b"TA", b"TC", b"AT")]


@pytest.mark.parametrize("K", [5, 6, 7, 8, 9])
def test_closed_runs_switch_to_the_reference_walk(ctx, orc, K):
    """A word w of 1..9 nucleotides whose two occurrences both end a contig ("w!"), in subjects of natural depth K: the
    build's flag equals the model's at the natural depth and at forced shallower ones (below |w| + 1 too), and wherever the
    oracle's cached lookup differs from its uncached one for a query that starts with w -- the reference AS RUN is then
    not the true longest match -- the scan equals the oracle's dist_anchor on queries that contain such words."""
    import andi_amd
    differs = 0
    for wlen in range(1, 10):
        seq, w = ptm.closed_run_subject(wlen, K)
        rs = ptm.subject_text(seq)
        flag = ptm.closed_run_flag(rs)
        assert flag == 1 or wlen == 9
        O = orc.OracleEsa(seq)
        rng = np.random.default_rng(100 * K + wlen)
        tails = _tails(rng, w)
        hit = [q for q in tails if O.get_match(q, True) != O.get_match(q, False)]
        differs += bool(hit)
        plain = seq.replace(b"!", b"")
        queries = [b"".join(rand_dna(rng, 40) + q + plain[s:s + 60] for q in tails for s in rng.integers(0, len(plain) - 60, 3)),
                   plain[:7000]]
        want = [O.dist_anchor(q) for q in queries]
        Q = andi_amd.Queries(ctx, queries)
        for depth in [K] + sorted({4, max(4, wlen), max(4, min(K, wlen + 1))} - {K}):  # (the natural depth first: it needs no test hook)
            for origin in ORIGINS:
                with knobs(DEEP_K=None if depth == K else depth):
                    E = andi_amd.Esa(ctx, seq, sa="device" if origin == "device" else None)
                    assert E.download_index()[0] == depth
                    assert E.flags()[0] == flag, (wlen, depth, origin)
                    if hit:
                        got = andi_amd.scan_rows(ctx, [E], [-1], Q, andi_amd.M_JC, 512)
                        for k in range(len(queries)):
                            assert (got[0, k] == want[k]).all(), (wlen, depth, origin, k)
                    E.close()
        Q.close()
        O.close()
    assert differs >= 6  # (the oracle's two lookups really differ for most word lengths up to 8)
