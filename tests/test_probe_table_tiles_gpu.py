"""k_probe_table's two paths (esa_build.hip: probe_table_block): a tile all of whose staged records are full K-mers runs
straight-line code, every other tile the general code.  Subjects in which both kinds of tile occur, side by side, entry by
entry and with the closed-run flag against the model of tests/probe_table_model.py: forms 0, 1 and 2 of the once-occurring
entries, suffix arrays from the host and from the device, each subject alone (k_probe_table) and in a mixed batch
(k_probe_table_batch, byte for byte the single launch's table).  What a case needs of its subject is asserted from the text
alone (tests/probe_table_tiles.py, checked in tests/test_probe_table_tiles_host.py) before the device is touched."""
import numpy as np
import pytest

import probe_table_model as ptm
import probe_table_tiles as ptt
from conftest import knobs

pytestmark = pytest.mark.gpu

# (ANDI_COOP, form by origin of the suffix array): the two settings give form 0 from both origins, form 1 and form 2
SETTINGS = {"coop-off": (0, {"host": 0, "device": 0}), "coop-4": (4, {"host": 1, "device": 2})}
ORIGINS = ("host", "device")
DEPTHS = ("natural", 8, 10)

_models = {}


@pytest.fixture(scope="module", autouse=True)
def _models_freed():
    yield
    _models.clear()


def _model(name, K):
    if (name, K) not in _models:
        rs = ptt.texts()[name]
        E = ptm.entries(rs, K, sa=ptt.model_sa(name))
        ys = {}
        for form in (0, 1, 2):
            x, ys[form], defined = ptm.table(rs, E, form)
        _models[name, K] = (x, defined, ys, ptm.closed_run_flag(rs))
    return _models[name, K]


def _host_sa(name, _cache={}):
    import andi_amd
    if name not in _cache:
        _cache[name] = andi_amd.suffix_array(ptt.texts()[name])
    return _cache[name]


def _stage(ctx, name, origin):
    import andi_amd
    E = andi_amd.Esa(ctx, ptt.subjects()[name], sa="device" if origin == "device" else _host_sa(name), build=False)
    assert E.RS == ptt.texts()[name]
    return E


def _check_against_model(E, name, K, form, what):
    x, defined, ys, flag = _model(name, K)
    k, table = E.download_index()
    assert k == K and E.single_form() == form, what
    bad = np.flatnonzero(table[:, 1] != ys[form])
    assert len(bad) == 0, (what, "y of codes", bad[:5], table[bad[:5], 1], ys[form][bad[:5]])
    bad = np.flatnonzero((table[:, 0] != x) & defined)
    assert len(bad) == 0, (what, "x of codes", bad[:5], table[bad[:5], 0], x[bad[:5]])
    assert E.flags()[0] == flag, (what, "closed-run flag")
    return table


def _every_entry(ctx, names, depth):
    """the subjects `names` at the given depth: every form and origin alone, and in batches with subjects of other lengths"""
    import andi_amd
    order = []
    for name in names:  # lengths mixed: a text of 17 characters and one of 40 001 between the case's own
        order += [name, "tiny", "halo-1"]
    forced = None if depth == "natural" else ptt.depth_of(names[0], depth)  # (a forced depth holds for every subject of the build)
    K_of = {name: forced or ptt.depth_of(name, "natural") for name in set(order)}
    for setting, (coop, forms) in SETTINGS.items():
        with knobs(COOP=coop, DEEP_K=forced):
            single = {(name, o): _stage(ctx, name, o) for name in set(order) for o in ORIGINS}
            for E in single.values():
                E.build()
            batches = []
            for flip in (0, 1):
                batch = [(name, ORIGINS[(k + flip) % 2]) for k, name in enumerate(order)]
                esas = [_stage(ctx, name, o) for name, o in batch]
                andi_amd.lib.build_indexes(ctx, esas)
                batches.append(list(zip(batch, esas)))
        tables = {(name, o): _check_against_model(E, name, K_of[name], forms[o], (name, depth, setting, o, "single")) for (name, o), E in single.items()}
        for batch in batches:
            for (name, o), E in batch:
                k, table = E.download_index()
                assert k == K_of[name] and E.single_form() == forms[o]
                assert (table == tables[name, o]).all(), (name, depth, setting, o, "batch != single launch")
                assert E.flags()[0] == _model(name, K_of[name])[3]
        for E in list(single.values()) + [E for b in batches for _, E in b]:
            E.close()


@pytest.mark.parametrize("depth", DEPTHS)
def test_both_paths(ctx, depth):
    """random, 40 kbp (RS of 80 001 characters, 105 tiles): at least 60 whole tiles and at least 10 that are not"""
    f = ptt.facts(depth)["random-40k"]
    assert f["tiles"] == 105 and f["whole"] >= 60 and f["tiles"] - f["whole"] >= 10
    _every_entry(ctx, ["random-40k"], depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_alternating_tiles(ctx, depth):
    """The 40 kbp genome as joined contigs.  As 60 contigs, the subject named for this case, it has 120 contig ends and some
    1100 suffixes that start within K characters of one: every one of its 105 tiles stages a short record and NONE is whole
    (asserted), so it cannot alternate; it is built and held to the model as the subject that takes the general path
    throughout.  The alternation is asserted on the same genome as 6 contigs: whole and non-whole tiles follow each other at
    least 20 times along the table (52 times at the natural depth)."""
    f = ptt.facts(depth)
    assert f["joined-60"]["tiles"] == 105 and f["joined-60"]["whole"] == 0
    assert f["joined-6"]["alternations"] >= 20 and f["joined-6"]["whole"] >= 20
    _every_entry(ctx, ["joined-60", "joined-6"], depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_short_record_in_the_halo_alone(ctx, depth):
    """20 kbp texts (seeds found by search, pinned) with a tile whose own 768 records are all full K-mers and whose halo holds
    a short one, at rank r0 - 2, r0 - 1 or r0 + TILE, one subject each: the tile must take the general path (the short
    record bounds what its first or last gap owns, or the uniqueness of an entry beside it)"""
    f = ptt.facts(depth)
    for off in ptt.HALO_SEEDS:
        assert [off] in f["halo%+d" % off]["halo_only"].values(), off
    _every_entry(ctx, ["halo%+d" % off for off in ptt.HALO_SEEDS], depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_long_runs_from_whole_tiles(ctx, depth):
    """Runs of equal K-mers longer than a tile.  With the 5000-fold repeat, whole tiles hold the start of a run that ends in a
    later tile, and gaps whose look-ahead of three records does not show the run's end: the walk and the binary search,
    reached from the straight-line path.  b"ACGT" * 2000 has four K-mers of some 4000 occurrences each, whose runs start
    beside the short records of the text's ends, in tiles that are not whole; its 16 whole tiles lie INSIDE the runs: no gap
    of theirs owns anything and they write no entry at all."""
    f = ptt.facts(depth)
    assert f["repeat-x-5000"]["leaving"] >= 1 and f["repeat-x-5000"]["far"] >= 1
    assert f["acgt-x-2000"]["whole"] >= 10 and f["acgt-x-2000"]["most_entries"] == 0
    _every_entry(ctx, ["acgt-x-2000", "repeat-x-5000"], depth)


def test_deep_table(ctx):
    """a table a symbol deeper than the text asks for (four entries per gap: what a thousand expected queries choose): whole
    tiles with more than PT_RANKED entries, whose entries past that number find their owner by binary search"""
    f = ptt.facts("natural+1")["random-40k"]
    assert f["K"] == 10 and f["past_ranked"] >= 60
    _every_entry(ctx, ["random-40k"], "natural+1")
