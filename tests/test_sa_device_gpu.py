"""The device suffix sorter (andi_amd/csrc/sa_device.hip; api.hip: esa_sort_suffixes) entry for entry against the naive
sort of the suffixes, at the edges of every round: the tails of k_sa_keys0, the tiles of the open-slot selection, the
lengths at which the round-1 key narrows, the special suffixes at every offset, doubling past the text's end, reused
workspaces, two contexts at once, and the records it leaves for k_probe_table.  Texts and model: tests/sa_model.py
(checked on the CPU: tests/test_sa_model_host.py).  Every sa_rounds expectation is sa_model.rounds(text).

Texts are staged as prepared texts (andi_hip_esa_stage_text: a fresh slot per text, the context's workspace reused).
Measured on an MI355X: COST_PER_TEXT below."""
import threading

import numpy as np
import pytest

import sa_model as sm
from conftest import knobs, verify_suffix_array

pytestmark = pytest.mark.gpu

COST_PER_TEXT = "0.2 ms per staged text of up to 8 symbols (slot, upload, sort, download, naive sort: 2273 texts in 0.45 s); the module 3.8 s"


def _stage(ctx, text, sa="device"):
    import andi_amd
    return andi_amd.Esa(ctx, None, build=False, prepared=(text, 0.5, 8, sa))


def _sort(ctx, text):
    """(suffix array, rounds) of one text sorted on the device; sa_builds advanced by one"""
    before = ctx.timings()
    E = _stage(ctx, text)
    got = E.SA
    after = ctx.timings()
    E.close()
    assert after["sa_builds"] - before["sa_builds"] == 1
    return got, int(after["sa_rounds"] - before["sa_rounds"])


def _check(ctx, text, name=None, want=None):
    """the device's suffix array of `text` equals the reference entry for entry; returns the rounds it took"""
    got, rounds = _sort(ctx, text)
    if want is None:
        want = sm.reference_sa(text)
    bad = np.flatnonzero(got != want)
    assert got.shape == want.shape and len(bad) == 0, (name or text[:80], len(text), bad[:5], got[bad[:5]], want[bad[:5]])
    if len(text) > sm.NAIVE_MAX:
        verify_suffix_array(text, got)
    return rounds


def _cgt(text):
    return set(text) <= set(b"CGT")


def test_exhaustive_small_texts(ctx):
    for t in sm.exhaustive_texts():
        _check(ctx, t)


def test_every_length_down_and_up(ctx):
    """70 down to 1, then 1 up to 70: the four tails of k_sa_keys0, n < 16, n < 19, a short text in a workspace a longer
    one has just used"""
    for t in sm.length_ladder():
        _check(ctx, t)


@pytest.mark.parametrize("n", sm.TILE_EDGE_LENGTHS)
def test_tile_edges(ctx, n):
    cases = [c for c in sm.tile_edge_texts() if len(c[1]) == n]
    assert len(cases) == 3
    for name, t, must in cases:
        want = sm.naive_sa(t)
        if must:
            assert sm.straddles_tile(t, want), name
        _check(ctx, t, name, want)


@pytest.mark.parametrize("pair", sm.THRESHOLD_PAIRS + ((262142, 262143),), ids=lambda p: "%d-%d" % p)
def test_key_width_thresholds(ctx, pair):
    shapes = [s for s in sm.threshold_shapes() if s[0] in pair]
    assert len(shapes) == (2 if pair[0] > 100000 else 18)
    for n, L in shapes:
        t = sm.threshold_text(n, L)
        want = sm.reference_sa(t)
        rounds = _check(ctx, t, "shared-%d-%d" % (n, L), want)
        assert rounds == sm.rounds(t, want), (n, L)


def test_periodic_texts_and_the_texts_end(ctx):
    for name, t in sm.periodic_texts():
        want = sm.naive_sa(t)
        rounds = _check(ctx, t, name, want)
        if _cgt(t):
            assert rounds == sm.rounds(t, want), name


def test_separators(ctx):
    open_special = 0
    for name, t in sm.separator_texts():
        rounds = _check(ctx, t, name)
        if name.startswith("copies-") and sm.special_open(t):
            open_special += 1
            assert rounds >= 3, name
    assert open_special >= 1


def test_foreign_bytes_are_refused_and_the_next_sort_is_right(ctx):
    import andi_amd
    for bad, clean in sm.foreign_texts():
        before = ctx.timings()["sa_builds"]
        with pytest.raises(andi_amd.AndiHipError, match="outside"):
            _stage(ctx, bad)
        assert ctx.timings()["sa_builds"] == before
        _check(ctx, clean)


def _mixed_texts(seed, count=20):
    rng = np.random.default_rng(seed)
    lengths = [1, 2, 5, 17, 64, 1023, 1025, 3000, 20000, 70000]
    out = []
    for k in range(count):
        n = lengths[int(rng.integers(0, len(lengths)))]
        kind = k % 4
        t = sm.dna(rng, n) if kind == 0 else sm.dna(rng, n, b"AC") if kind == 1 else b"A" * n if kind == 2 else \
            b"!".join([sm.dna(rng, max(1, n // 7))] * 7)
        out.append(t)
    return out


def test_one_context_sorts_long_short_long(ctx):
    """the workspace is the context's and is never cleared: the special list lies in hv, the counts in grp and rank"""
    import andi_amd
    rng = np.random.default_rng(7800)
    big = sm.dna(rng, 300000)
    want_big = andi_amd.suffix_array(big)
    first, _ = _sort(ctx, big)
    assert (first == want_big).all()
    _check(ctx, b"GATTA")
    _check(ctx, b"A" * 50000)
    _check(ctx, b"C")
    again, _ = _sort(ctx, big)
    assert (again == want_big).all() and (again == first).all()
    verify_suffix_array(big, again)


def test_two_contexts_in_two_threads(ctx):
    import andi_amd
    sets = [_mixed_texts(7901), _mixed_texts(7902)]
    single = [[_sort(ctx, t)[0] for t in texts] for texts in sets]
    for texts, sas in zip(sets, single):
        for t, sa in zip(texts, sas):
            assert (sa == sm.reference_sa(t)).all()
    results, errors = [None, None], []

    def work(k):
        try:
            c = andi_amd.Context(0)
            try:
                results[k] = [_sort(c, t)[0] for t in sets[k]]
            finally:
                c.close()
        except BaseException as e:  # (reported by the test's own thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(2):
        for got, want in zip(results[k], single[k]):
            assert (got == want).all()


def test_records_give_the_tables_the_host_suffix_array_gives(ctx):
    """k_sa_records, k_sa_special_records and record_of in k_sa_apply: with ANDI_COOP=0 the once-occurring entries have
    form 0 whatever made the suffix array, so the probe table built from the sorter's records must equal the one built
    from the host's suffix array and the text -- or, where the build hands the subject to the reference's walk, the flags."""
    import andi_amd
    import probe_table_model as ptm
    seqs = sm.record_sequences()
    assert len(seqs) > 250
    tables = flagged = 0
    with knobs(COOP=0):
        for seq in seqs:
            rs = ptm.subject_text(seq)
            D, H = _stage(ctx, rs), _stage(ctx, rs, andi_amd.suffix_array(rs))
            D.build(), H.build()
            fd, fh = D.flags(), H.flags()
            assert (fd == fh).all(), (seq[:80], fd, fh)
            if not fd[0]:
                assert D.single_form() == 0 and H.single_form() == 0
                (kd, td), (kh, th) = D.download_index(), H.download_index()
                bad = np.flatnonzero((td != th).any(axis=1))
                assert kd == kh and len(bad) == 0, (seq[:80], len(seq), bad[:5], td[bad[:5]], th[bad[:5]])
                tables += 1
            else:
                flagged += 1
            D.close(), H.close()
    assert tables > 200
