"""tests/sa_model.py on the CPU: the naive sort and the host sorter (host_sais.cpp) held to each other, and the constructed
texts shown to be what tests/test_sa_device_gpu.py takes them for."""
import numpy as np
import pytest

import sa_model as sm
from conftest import verify_suffix_array


def _host(text):
    import andi_amd
    return andi_amd.suffix_array(text)


def test_params_at_the_lengths_where_the_key_narrows():
    assert [sm.params(n)[1] for n in (1, 510, 511, 4094, 4095, 32766, 32767, 262142, 262143)] == [16, 16, 15, 15, 14, 14, 13, 13, 12]
    assert sm.params(510) == (9, 16) and sm.params(511) == (10, 15) and sm.params(1) == (2, 16)


def test_naive_sort_on_a_worked_example():
    assert sm.naive_sa(b"TGCAACGT#ACGTTGCA").tolist() == sorted(range(17), key=lambda i: b"TGCAACGT#ACGTTGCA"[i:] + b"\0")
    assert sm.naive_sa(b"AA!A").tolist() == [2, 3, 1, 0]  # !A < A < A!A < AA!A
    assert sm.max_lcp(b"AA!A") == 1 and sm.max_lcp(b"A") == 0 and sm.max_lcp(b"TTTTT") == 4


def test_exhaustive_small_texts_naive_equals_host():
    texts = sm.exhaustive_texts()
    assert len(texts) == 510 + 1364 + 399
    for t in texts:
        assert (_host(t) == sm.naive_sa(t)).all(), t


def test_constructed_cases_naive_equals_host():
    short = 0
    for name, t in sm.constructed_cases():
        if len(t) <= sm.NAIVE_MAX:
            want = sm.naive_sa(t)
            verify_suffix_array(t, want)
            assert (_host(t) == want).all(), name
            short += 1
        else:
            verify_suffix_array(t, _host(t))
    assert short > 600


def test_shared_units_share_exactly_what_they_claim():
    shapes = sm.threshold_shapes()
    assert len(shapes) == 6 * 9 + 2
    for n, L in shapes:
        t = sm.threshold_text(n, L)
        assert len(t) == n and set(t) <= set(b"CGT")
        assert sm.max_lcp(t, _host(t)) == L, (n, L)


def test_rounds_takes_every_value_it_is_meant_to():
    by_shape = {(n, L): sm.rounds(sm.threshold_text(n, L), _host(sm.threshold_text(n, L))) for n, L in sm.threshold_shapes()}
    for (n, L), r in by_shape.items():
        h = 16 + sm.params(n)[1]
        want = 1 if L < 16 else 2 if L < h else 3 if L < 2 * h else 4
        assert r == want, (n, L, r)
    assert set(by_shape.values()) == {1, 2, 3, 4}
    assert by_shape[(510, 31)] == 2 and by_shape[(511, 31)] == 3  # one more symbol of text, one symbol less in the key
    per = dict(sm.periodic_texts())
    assert sm.rounds(per["CGT-period-1-1000"]) == 2 + 6  # 999 shared symbols, h = 16 + 15: 31 * 2^5 = 992 <= 999 < 1984
    assert sm.rounds(per["CGT-period-1-4099"]) >= 4 and sm.rounds(per["CGT-period-33-4099"]) >= 4
    assert sm.rounds(b"CGT") == 1 and sm.rounds(b"T" * 16) == 1 and sm.rounds(b"T" * 17) == 2
    with pytest.raises(AssertionError):
        sm.rounds(b"ACGT")


def test_tile_edge_texts_have_groups_across_a_tile():
    for name, t, must in sm.tile_edge_texts():
        sa = sm.naive_sa(t)
        if must:
            assert sm.straddles_tile(t, sa), name
        g = sm.open_groups0(t, sa)
        if name.startswith("period-2"):  # every slot but those of the last sixteen suffixes is open
            assert (g[:, 1] - g[:, 0] + 1).sum() >= len(t) - 16
        if name.startswith("random-AC-"):
            assert len(g) >= 4
    assert sum(must for _, _, must in sm.tile_edge_texts()) == 6


def test_periodic_texts_cut_their_last_period():
    for name, t in sm.periodic_texts():
        if "-period-" in name and "ends" not in name:
            p = int(name.split("-")[2])
            # (4099 is prime; 1000 is a multiple of 2 and 5 alone: every other period's last copy is cut)
            assert t[p:] == t[:-p] and (p in (1, 2, 5) or len(t) % p) and (p == 1 or 4099 % p)
            assert sm.max_lcp(t) == len(t) - p


def test_ties_at_every_offset_tie_in_round_0():
    for jj in range(16):
        t = sm.ties_at(jj)
        key, where = sm.key0(t)
        P = t[len(t) - jj:]
        behind = (b"!CGTTGC", b"#CGTTGC", b";CGTTGC", b"!TGCCGT", b"A" * 16 + b"C")
        at = [t.index(P + b) for b in behind] + ([len(t) - jj] if jj else [])  # (at jj = 0 the text's end is no suffix)
        assert len(set(at)) == len(at) and len(set(key[at].tolist())) == 1, jj
        assert where[at].tolist() == [jj] * 4 + [16] + [jj] * (jj > 0)
        want = sorted(at, key=lambda i: t[i:])
        assert [t[i + jj:i + jj + 1] for i in want] == ([b""] if jj else []) + [b"!", b"!", b"#", b";", b"A"]


def test_copies_of_a_contig_leave_a_special_suffix_open():
    names = dict(sm.separator_texts())
    shapes = sm.copies_shapes()
    for k in (2, 5, 40):
        syms = {L for kk, L in shapes if kk == k and sm.params(k * L + k - 1)[1] == L}
        syms1 = {L for kk, L in shapes if kk == k and sm.params(k * L + k - 1)[1] + 1 == L}
        assert syms and syms1, k
    open_ = [sm.special_open(names["copies-%d-of-%d" % s]) for s in shapes]
    assert any(open_)
    assert sm.special_open(names["copies-5-of-40"]) and not sm.special_open(names["copies-2-of-3"])
    assert not sm.special_open(sm.ties_at(5))
