"""The queries' 2-bit codes are staged once (andi_amd/csrc/scan_lane.hip: k_pack_planes writes them beside the planes; ScanArgs.qcodes)
and the windows of pass A by wavefronts load them instead of making them from the planes for every pair (coop_window.h:
coop_window).  The staged words against numpy, through a hook of the suite's library; the kernel with windows of five chunks
(ANDI_COOP=5) against the oracle and the lane scan (ANDI_COOP=0) on queries whose lengths lie around the edges of a block of 32
symbols, of a chunk of 2048 and of a window of 10240."""
import numpy as np
import pytest

import andi_amd
from andi_amd import synth
from conftest import SHIPPED_LIB, knobs
from oracle import orc

pytestmark = pytest.mark.gpu

LENGTHS = (1, 31, 32, 33, 63, 2047, 2049, 10241)


def _codes_numpy(seq: bytes):
    """what the pack kernels make of a query's place in the pool: symbols A, C, G, T = 0 ... 3, '!' = 4, the NUL behind the
    query and the pool's zero padding = 7 (scan_lane.hip: symbol_of); bits 0 and 1 of symbol k of a half block of 16 at bits
    2k, 2k + 1 of its word"""
    slot = (len(seq) + 1 + 255) // 256 * 256
    sym = np.full(slot, 7, np.uint64)
    b = np.frombuffer(seq, np.uint8)
    lut = np.full(256, 7, np.uint64)
    for ch, v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"!", 4)):
        lut[ch[0]] = v
    sym[:len(b)] = lut[b]
    two = (sym & 3).reshape(-1, 16)
    return (two << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def _pool():
    """queries of the lengths above cut from one genome; the longest with '!' separators (one of them the last symbol of a block, one
    the first), the lengths that are no multiple of 32 end in a ragged block"""
    g = synth.to_bytes(synth.base_codes(12000, 3))
    qs = [g[100 * k:100 * k + n] for k, n in enumerate(LENGTHS)]
    last = bytearray(qs[-1])
    for p in (31, 64, 1000, 2048, 5555, 10239):
        last[p] = ord("!")
    qs[-1] = bytes(last)
    return qs


def test_staged_codes_equal_numpy_and_a_view_shares_them():
    if SHIPPED_LIB:
        pytest.skip("andi_hip_test_query_codes is a test hook: not in the shipped library")
    qs = _pool()
    ctx = andi_amd.Context(0)
    Q = andi_amd.Queries(ctx, qs)
    got = [Q.codes(i) for i in range(len(qs))]
    V = Q.view(2, 5)
    seen = [V.codes(i) for i in range(5)]
    V.close(), Q.close(), ctx.close()
    for i, q in enumerate(qs):
        want = _codes_numpy(q)
        assert got[i].shape == want.shape and (got[i] == want).all(), "query %d of %d symbols: words %s" % (
            i, len(q), np.nonzero(got[i] != want)[0][:8].tolist())
    for i in range(5):
        assert (seen[i] == got[2 + i]).all(), "the view's query %d" % i


def _rows(subjects, queries, model, coop):
    """rows of the subjects (the first of the queries) through andi_hip_scan_rows on a context of its own"""
    with knobs(COOP=coop):
        ctx = andi_amd.Context(0)
        Q = andi_amd.Queries(ctx, queries)
        esas = [andi_amd.Esa(ctx, s, sa="device") for s in subjects]
        got = andi_amd.scan_rows(ctx, esas, list(range(len(subjects))), Q, model=model)
        for e in esas:
            e.close()
        Q.close()
        ctx.close()
    return got


def _oracle_rows(subjects, queries, model):
    rows = []
    for i, s in enumerate(subjects):
        rows.append(orc.scan_row(orc.OracleEsa(s), queries, i, model, threads=2))
    return np.stack(rows)


def _star(joined):
    """three genomes of 25 kbp 0.5 ... 3 % from their base -- as subjects and as queries -- and queries of the lengths above cut from a
    fourth; joined: every genome and the longest query cut into contigs joined by '!' (the window's path that is not clean)"""
    base = synth.base_codes(25000, 21)
    genomes = [synth.to_bytes(synth.mutate_codes(base, d, 40 + k)) for k, d in enumerate((0.005, 0.01, 0.03))]
    other = synth.to_bytes(synth.mutate_codes(base, 0.02, 50))
    cuts = [other[1500 * k + 7:1500 * k + 7 + n] for k, n in enumerate(LENGTHS)]
    if joined:
        genomes = [synth.join_contigs(g, 5, seed=60 + k) for k, g in enumerate(genomes)]
        cuts[-1] = synth.join_contigs(cuts[-1], 4, seed=70)
    return genomes, genomes + cuts


_want = {}


def _want_rows(joined, model):
    if (joined, model) not in _want:
        subjects, queries = _star(joined)
        _want[joined, model] = _oracle_rows(subjects, queries, model)
    return _want[joined, model]


@pytest.mark.parametrize("model", [andi_amd.M_JC, andi_amd.M_KIMURA])
@pytest.mark.parametrize("joined", [False, True])
def test_five_chunk_windows_equal_oracle_and_lane_scan(joined, model):
    subjects, queries = _star(joined)
    want = _want_rows(joined, model)
    lane = _rows(subjects, queries, model, 0)
    assert (lane == want).all(), "lane scan: pairs %s" % np.argwhere((lane != want).any(axis=2))[:8].tolist()
    got = _rows(subjects, queries, model, 5)
    assert (got == want).all(), "windows of five chunks: pairs %s" % np.argwhere((got != want).any(axis=2))[:8].tolist()


def test_query_that_ends_inside_its_first_window():
    """a query shorter than a window of 10240 positions whose last block is ragged: the lanes whose words begin beyond its end keep zero
    codes, the word with its end keeps the padding's bits behind it"""
    base = synth.base_codes(25000, 33)
    subject = synth.to_bytes(base)
    mut = synth.to_bytes(synth.mutate_codes(base, 0.01, 34))
    queries = [subject, mut[3000:3000 + 6007], mut[:2049], mut[9000:9000 + 10241]]
    want = _oracle_rows([subject], queries, orc.M_JC)
    lane = _rows([subject], queries, andi_amd.M_JC, 0)
    got = _rows([subject], queries, andi_amd.M_JC, 5)
    assert (lane == want).all()
    assert (got == lane).all(), "queries %s" % np.argwhere((got != lane).any(axis=2))[:8].tolist()
