"""The model of the probe table (tests/probe_table_model.py) is the judge of tests/test_probe_table_gpu.py: here it is
checked without a GPU -- against a search in plain Python, against the oracle's uncached lookup, its two back ends
against each other -- and the texts the GPU tests build are shown to have the properties they are built for."""
import numpy as np
import pytest

import probe_table_model as ptm
from conftest import rand_dna


def _kmer(code, K):
    return bytes(b"ACGT"[(code >> (2 * (K - 1 - t))) & 3] for t in range(K))


def _naive_entry(rs: bytes, sa, K, code, form):
    """(x or None, y) of one code by str.startswith over all positions"""
    w = _kmer(code, K)
    at = [p for p in range(len(rs)) if rs.startswith(w, p)]
    rank = {int(p): r for r, p in enumerate(sa)}
    if len(at) > 1:
        return min(rank[p] for p in at), 2 | (len(at) - 1) << 8
    if len(at) == 1:
        if form == 0:
            return at[0], 1 | 1 << 2 | K << 8
        cnt = ext = 0
        for j in range({1: 13, 2: min(4, 16 - K)}[form]):
            s = b"ACGT".find(rs[at[0] + K + j:at[0] + K + j + 1])
            if s < 0 or at[0] + K + j >= len(rs):
                break
            cnt, ext = cnt + 1, ext | s << (2 * j)
        return at[0], 1 | cnt << 2 | ext << 6
    for l in range(K - 1, 0, -1):
        at = [p for p in range(len(rs)) if rs.startswith(w[:l], p)]
        if at:
            return (rank[at[0]], 1 << 2 | l << 8) if len(at) == 1 else (None, l << 8)
    return (0, 1 << 2) if len(rs) == 1 else (None, 0)


SMALL_TEXTS = [b"ACGTTGCA#TGCAACGT", b"AAAAAAAAAAAAAAAAAAAAAAAAA", b"GT;ACCA;T#A!TGGT!AC", b"ACGTACGTACGT!ACGTACG;ACGTAC#ACGTA",
               b"TTTTTTTTTTTTTTTTTTTTG#CAAAAAAAAAAAAAAAAAAAA", b"A", b"#", b"CAT!CAT!CAT;ATG;ATG#", b"!;#ACGT#;!"]


def _naive_sa(rs):
    return sorted(range(len(rs)), key=lambda p: rs[p:])


@pytest.mark.parametrize("K", [4, 5, 6])
def test_model_equals_naive_search(K):
    rng = np.random.default_rng(K)
    texts = SMALL_TEXTS + [rand_dna(rng, 40, b"ACGT!;"), rand_dna(rng, 60, b"AC") + b"#" + rand_dna(rng, 30, b"ACG!")]
    for rs in texts:
        sa = _naive_sa(rs)
        assert ptm.suffix_array(rs).tolist() == sa, rs
        every = ptm.entries(rs, K)
        step = 1 if K < 6 else 5  # (4^6 codes by pure Python: every fifth, and the list back end on exactly those)
        codes = np.arange(K % step, 4 ** K, step)
        listed = ptm.entries(rs, K, codes)
        for form in (0, 1, 2):
            xe, ye, de = ptm.table(rs, every, form)
            xl, yl, dl = ptm.table(rs, listed, form)
            assert (ye[codes] == yl).all() and (de[codes] == dl).all() and (xe[codes][dl] == xl[dl]).all()
            for k, c in enumerate(codes):
                x, y = _naive_entry(rs, sa, K, int(c), form)
                assert yl[k] == y and dl[k] == (x is not None), (rs, K, form, c)
                assert x is None or xl[k] == x, (rs, K, form, c)


def _oracle_subjects():
    from andi_amd import synth
    rng = np.random.default_rng(77)
    yield "tiny", b"ACGTTGCA"
    yield "homopolymer", b"A" * 300
    yield "two-letter", rand_dna(rng, 900, b"AC")
    yield "random-400", rand_dna(rng, 400)
    yield "random-3k", rand_dna(rng, 3000)
    yield "repeats", rand_dna(rng, 120) * 6 + rand_dna(rng, 90)
    yield "joined", synth.join_contigs(rand_dna(rng, 2500), 9)
    yield "short-contigs", b"!".join([b"ACG", b"ACGT", b"AC", b"ACGTA", b"ACG"] * 20)
    yield "poly-a-at-separators", b";".join([b"GATTACA" + b"A" * k for k in range(0, 20)] * 2)
    yield "same-contig-ends", b"!".join([rand_dna(rng, 40 + 5 * k) + b"ACGTTGCAACGTAC" for k in range(12)])


@pytest.mark.parametrize("name,seq", list(_oracle_subjects()), ids=[n for n, _ in _oracle_subjects()])
def test_model_equals_oracle_lookup(orc, name, seq):
    """get_match (src/esa.c:615-631, uncached) of every K-mer, K = 4..7: (l, i, j) = the model's match length, whether
    one suffix has it (i == j), and for a K-mer that occurs its count j - i + 1 and first rank i."""
    O = orc.OracleEsa(seq)
    rs = O.RS
    assert rs == ptm.subject_text(seq)
    sa = ptm.suffix_array(rs)
    assert (sa == O.SA).all()
    for K in (4, 5, 6, 7):
        E = ptm.entries(rs, K)
        for c in range(4 ** K):
            l, i, j = O.get_match(_kmer(c, K) + b"N", False)  # ('N' is nowhere in RS: the match ends where the K-mer does)
            if E.kind[c] == ptm.FINAL:
                assert l == E.l[c] and (i == j) == bool(E.unique[c]), (K, c)
                assert not E.unique[c] or i == E.rank[c]
            else:
                assert l == K and j - i + 1 == E.count[c], (K, c)
                assert (sa[i] == E.pos[c]) if E.kind[c] == ptm.SINGLE else (i == E.rank[c]), (K, c)
    O.close()


def test_back_ends_agree_and_deep_lists_stay_small():
    """every code == the list of codes where both apply; K = 13 by list needs no 4^13 arrays (tracemalloc: < 64 MB)"""
    import tracemalloc
    rng = np.random.default_rng(5)
    seq = b"!".join([rand_dna(rng, 700), rand_dna(rng, 300) * 3, b"ACGT" * 100])
    rs = ptm.subject_text(seq)
    for K in (4, 7, 10):
        every = ptm.entries(rs, K)
        codes = np.unique(rng.integers(0, 4 ** K, 5000))
        listed = ptm.entries(rs, K, codes)
        for a, b in zip(every[2:], listed[2:]):
            assert (a[codes] == b).all(), K
    tracemalloc.start()
    codes = rng.integers(0, 4 ** 13, 200000)
    E = ptm.entries(rs, 13, codes)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 64 << 20
    assert (E.kind == ptm.FINAL).mean() > 0.99  # (random 13-mers are not in a text of 5 kbp)
    present = ptm.present_codes(rs, 13)
    assert (ptm.entries(rs, 13, present).kind != ptm.FINAL).all() and len(present) > 1000


def test_closed_run_flag_model():
    from test_scan_gpu import _separator_spanning_subject
    subj = _separator_spanning_subject(np.random.default_rng(57))
    assert ptm.closed_run_flag(ptm.subject_text(subj)) == 1
    first = subj.index(b"GACCGGA!")
    broken = subj[:first + 6] + b"C" + subj[first + 7:]  # one of the two "w!": GACCGGC! -- the contigs' ends share no suffix any more
    assert ptm.closed_run_flag(ptm.subject_text(broken)) == 0
    rng = np.random.default_rng(3)
    for text in (rand_dna(rng, 5000), b"A" * 300, b"ACGT" * 500, b"ACGTTGCA"):
        assert ptm.closed_run_flag(ptm.subject_text(text)) == 0
    # a word's occurrences behind different separators, or one of them at the text's end, close nothing
    assert ptm.closed_run_flag(b"TTG!CCG;AAG") == 0
    assert ptm.closed_run_flag(b"TTG!CCG!AAG") == 0  # ("G": the third occurrence ends the text)
    assert ptm.closed_run_flag(b"TTG!CCG!AAC") == 1
    assert ptm.closed_run_flag(b"ACGTACGTA;T#TACGTACGTA;") == 1  # (the 8-mer CGTACGTA)
    # 9 nucleotides, ACGTACGTT, are beyond the 10-mer table's reach (every shorter suffix of it also occurs in front of an A)
    assert ptm.closed_run_flag(b"ACGTACGTT;C#CGTACGTTA!AACGTACGTT;") == 0


@pytest.mark.parametrize("K", [5, 6, 7, 8, 9])
def test_closed_run_subjects_are_closed(K):
    for wlen in range(1, 10):
        seq, w = ptm.closed_run_subject(wlen, K)
        rs = ptm.subject_text(seq)
        assert ptm.natural_k(len(rs)) == K and len(w) == wlen and rs.count(w + b"!") == 2
        if wlen <= 8:
            assert ptm.closed_run_flag(rs) == 1


def test_texts_have_the_properties_they_are_built_for():
    seq, facts = ptm.run_lengths_text()
    assert set(ptm.RUN_COUNTS) <= facts["counts"] and facts["longest"] >= 1000
    assert facts["short_at_tile_end"] and facts["long_at_tile_end"]
    seq, facts = ptm.single_ends_text()
    assert {0, ord("#"), ord("!"), ord(";")} <= facts["ends_at"] and set(ptm.BEHIND) <= facts["behind"] and facts["far"]
