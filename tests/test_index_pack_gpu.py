"""The text of a scan index as the build packs it (scan_lane.hip: k_pack_text, k_pack_text_batch -- one pass: 4-bit symbols in
two alignments, N0 and N1, and bit-sliced, P) against a numpy restatement of the three forms; and the builds that run that
kernel, one subject per launch and many, against the restatement, against each other and -- by the scan kernels that read
N0 and N1 and by the one that streams P -- against the oracle."""
import functools

import numpy as np
import pytest

import probe_table_model as ptm
from conftest import SHIPPED_LIB, knobs, rand_dna

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_the_hooks():
    if SHIPPED_LIB:  # (the download of the packed text and the pack kernel alone are hooks of the suite's library)
        pytest.skip("the packed text is read through test hooks: not in the shipped library")


# ---------------------------------------------------------------- the three forms, restated
CODE = np.full(256, 7, np.uint8)  # scan_lane.hip: symbol_of
for _ch, _v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"!", 4), (b";", 5), (b"#", 6)):
    CODE[_ch[0]] = _v
for _c in range(0x41, 256):
    if _c not in b"ACGT":
        CODE[_c] = ((_c & 6) ^ ((_c & 6) >> 1)) >> 1  # what a byte outside the alphabet becomes
INSIDE = set(b"ACGT!;#\0")


def packed_model(text: bytes):
    """(N0, N1, P, foreign) of a text of n characters: n + 1 + 64 symbols (the text, its NUL, 64 bytes of zero padding)
    rounded up to pairs of words for N0 and N1, to blocks of 32 for P.  N0: symbol k in nibble k; N1: symbol k - 1 in
    nibble k, a NUL symbol (7) in nibble 0; P: bit k of word 3 j + b = bit b of symbol 32 j + k."""
    n = len(text)
    symbols = n + 1 + 64
    pairs, blocks = (symbols + 15) // 16, (symbols + 31) // 32
    raw = np.zeros(32 * blocks, np.uint8)
    raw[:n] = np.frombuffer(text, np.uint8)
    sym = CODE[raw]
    s0 = sym[:16 * pairs]
    s1 = np.concatenate(([7], sym[:16 * pairs - 1])).astype(np.uint8)
    N0 = s0[0::2] | (s0[1::2] << 4)
    N1 = s1[0::2] | (s1[1::2] << 4)
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    planes = [(((sym.reshape(blocks, 32) >> b) & 1).astype(np.uint64) * weights).sum(axis=1) for b in range(3)]
    P = np.stack(planes, axis=1).astype(np.uint32).reshape(-1)
    foreign = int(any(c not in INSIDE for c in text[:16 * pairs]))
    return N0, N1, P, foreign


def check_packed(E, text, what, with_n1=True, with_p=True):
    """the subject's N0, N1 and P equal the model's; nothing is written in front of P or behind any of the three"""
    N0, N1, P = E.download_text(beyond=16)
    m0, m1, mp, _ = packed_model(text)
    assert (N0[:-16] == m0).all(), (what, "N0", np.flatnonzero(N0[:-16] != m0)[:5])
    assert (N0[-16:] == 0x77).all(), (what, "behind N0")
    if with_n1:
        assert (N1[:-16] == m1).all(), (what, "N1", np.flatnonzero(N1[:-16] != m1)[:5])
    else:
        assert (N1[:-16] == 0x77).all(), (what, "N1 written")
    assert (N1[-16:] == 0x77).all(), (what, "behind N1")
    assert (P[:3] == 0xffffffff).all(), (what, "the block in front of P")
    if with_p:
        assert (P[3:-4] == mp).all(), (what, "P", np.flatnonzero(P[3:-4] != mp)[:5])
    else:
        assert (P[3:-4] == 0xffffffff).all(), (what, "P written")
    assert (P[-4:] == 0xffffffff).all(), (what, "behind P")


def test_the_model_is_the_host_packer():
    """the restatement's N0 against andi_hip_pack_symbols (the host's packer, itself held to the alphabet table by
    tests/test_host.py), and its N1 and P against their definitions symbol by symbol on one text"""
    from andi_amd import lib
    rng = np.random.default_rng(1)
    text = rand_dna(rng, 70) + b"!;#N-\0" + rand_dna(rng, 23)
    N0, N1, P, foreign = packed_model(text)
    got, bad = lib.pack_symbols(text + bytes(len(N0) * 2 - len(text)))
    assert (got == N0).all() and bad and foreign
    sym = [CODE[c] for c in text] + [7] * (len(N0) * 2 + 32)
    for k in range(len(N0) * 2):
        assert (N0[k // 2] >> (4 * (k & 1))) & 15 == sym[k]
        assert (N1[k // 2] >> (4 * (k & 1))) & 15 == (sym[k - 1] if k else 7)
    for k in range(len(P) // 3 * 32):
        assert [(int(P[3 * (k // 32) + b]) >> (k % 32)) & 1 for b in range(3)] == [(sym[k] >> b) & 1 for b in range(3)]


LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4099]
SPECIAL = [b"!", b";", b"#", b"N", b"-", b"\0"]  # (N: a foreign byte that becomes a nucleotide's symbol; -: one that becomes NUL's)


def _stage_text(ctx, text):
    """any bytes as a subject's text (no table is built from it: the suffix array is a placeholder)"""
    import andi_amd
    return andi_amd.Esa(ctx, None, build=False, prepared=(text, 0.5, 8, np.arange(len(text), dtype=np.int32)))


@pytest.mark.parametrize("n", LENGTHS)
def test_fused_kernel_against_the_model(ctx, n):
    """Texts of n characters, plain and with each of ! ; # a foreign byte and the NUL at the first, the last and a middle
    position: N0, N1 (the nibble every word takes from its predecessor, the first word's from nowhere) and P, the zero
    padding behind the text included; the foreign-byte flag; and the forms that leave N1 or P out."""
    rng = np.random.default_rng(n)
    plain = rand_dna(rng, n)
    texts = [(plain, "plain")]
    for c in SPECIAL:
        for pos in sorted({0, n // 2, n - 1}):
            texts.append((plain[:pos] + c + plain[pos + 1:], "%r at %d" % (c, pos)))
    everywhere = bytearray(plain)  # all of them at once, on both sides of every boundary of 16 and 32 that the text has
    for k, pos in enumerate(p for b in range(0, n + 16, 16) for p in (b - 1, b) if 0 <= p < n):
        everywhere[pos] = SPECIAL[k % len(SPECIAL)][0]
    texts.append((bytes(everywhere), "at every boundary"))
    for text, what in texts:
        E = _stage_text(ctx, text)
        E.pack_text()
        check_packed(E, text, (n, what))
        assert E.flags()[1] == packed_model(text)[3] == int(any(c not in INSIDE for c in text)), (n, what)
        E.close()
    for forms in (0, 1, 2):
        E = _stage_text(ctx, texts[-1][0])
        E.pack_text(forms)
        check_packed(E, texts[-1][0], (n, "forms", forms), with_n1=bool(forms & 1), with_p=bool(forms & 2))
        E.close()


# ---------------------------------------------------------------- the builds that run the kernel
@functools.lru_cache(None)
def _seqs():
    """three subjects whose texts RS = revcomp(S) '#' S have 70 001, 4 099 and 33 characters, a fourth of 12 001, and two
    queries made of mutated pieces of all of them"""
    from andi_amd import synth
    seeds = {"long": (35000, 5), "mid": (2049, 6), "short": (16, 7), "other": (6000, 8)}
    s = {k: synth.to_bytes(synth.base_codes(n, seed)) for k, (n, seed) in seeds.items()}
    mut = {k: synth.to_bytes(synth.mutate_codes(synth.base_codes(n, seed), 0.02, 40 + seed)) for k, (n, seed) in seeds.items()}
    queries = [mut["long"][:20000] + mut["mid"] + mut["short"] + mut["other"][:3000], mut["other"] + mut["long"][15000:] + s["short"]]
    return s, queries


@functools.lru_cache(None)
def _want(name):
    """the oracle's counts of the two queries against a subject"""
    from oracle import orc
    orc.build()
    s, queries = _seqs()
    O = orc.OracleEsa(s[name])
    want = [O.dist_anchor(q) for q in queries]
    O.close()
    return want


def _stage(ctx, name, origin="device"):
    import andi_amd
    return andi_amd.Esa(ctx, _seqs()[0][name], sa="device" if origin == "device" else None, build=False)


def _scan_equals_oracle(ctx, esas, names, Q, coop, what):
    """the two queries against the subjects, by the lane kernels (ANDI_COOP=0: they read N0 and N1) or by the wavefront
    kernel (ANDI_COOP=4: it streams P)"""
    import andi_amd
    with knobs(COOP=coop):
        ctx.timings_reset()
        got = andi_amd.scan_rows(ctx, esas, [-1] * len(esas), Q, andi_amd.M_JC)
        assert ctx.timings()["coop_calls"] == (1 if coop else 0), (what, coop)
    for i, name in enumerate(names):
        for k, want in enumerate(_want(name)):
            assert (got[i, k] == want).all(), (what, coop, name, k)


def _built(ctx, names, origins, coop, depth, Q, what):
    """stage and build the batch, scan right behind the build, and return what the build left: per subject (table, N0,
    N1, P, flags)"""
    import andi_amd
    with knobs(COOP=coop, DEEP_K=depth):
        esas = [_stage(ctx, n, o) for n, o in zip(names, origins)]
        andi_amd.lib.build_indexes(ctx, esas)
    _scan_equals_oracle(ctx, esas, names, Q, coop, what)
    out = []
    for E, name in zip(esas, names):
        check_packed(E, E.RS, (what, name))
        out.append((E.download_index()[1],) + E.download_text() + (E.flags(),))
        E.close()
    return out


PARTS = ("table", "N0", "N1", "P", "flags")


@pytest.mark.parametrize("coop", [0, 4], ids=["lane-kernels", "wavefront-kernel"])
def test_batch_of_unequal_lengths(ctx, coop):
    """Three device-sorted subjects of unequal length in one batch (the grid is sized by the longest), tables nine deep
    and at their natural depths (9, 7 and 4: the shallow ones take the closed-run launch, which reads N0): N0, N1 and P
    equal the model, the scan queued right behind the build equals the oracle, and tables, N0, N1, P and flags are the
    bytes of each subject's single launch.  A batch in which one subject's suffix array came from the host gives the same."""
    import andi_amd
    names = ["long", "mid", "short"]
    Q = andi_amd.Queries(ctx, _seqs()[1])
    for depth in (9, None):
        batch = _built(ctx, names, ["device"] * 3, coop, depth, Q, ("batch", depth))
        mixed = _built(ctx, names, ["device", "host", "device"], coop, depth, Q, ("one host suffix array", depth))
        for k, name in enumerate(names):
            for origin, built in (("device", batch), ("host", mixed)) if k == 1 else (("device", batch), ("device", mixed)):
                with knobs(COOP=coop, DEEP_K=depth):
                    E = _stage(ctx, name, origin)
                    E.build()
                single = (E.download_index()[1],) + E.download_text() + (E.flags(),)
                check_packed(E, E.RS, ("single", name, depth))
                E.close()
                for a, b, part in zip(built[k], single, PARTS):
                    assert (a == b).all(), (name, origin, depth, part, "batch != single launch")
    Q.close()


def test_closed_run_subject_in_a_batch(ctx):
    """A constructed subject whose word w occurs twice, each time in front of a contig's end (tests/test_probe_table_gpu.py),
    its table six deep, beside a subject nine deep: the closed-run launch reads the N0 the pack kernel wrote in front of it
    and raises the flag; the other subject's table is that of its single launch."""
    import andi_amd
    seq, _ = ptm.closed_run_subject(3, 6)
    rs = ptm.subject_text(seq)
    assert ptm.closed_run_flag(rs) == 1
    closed = andi_amd.Esa(ctx, seq, sa="device", build=False)
    other, alone = _stage(ctx, "long"), _stage(ctx, "long")
    andi_amd.lib.build_indexes(ctx, [other, closed])
    assert closed.download_index()[0] == 6 and closed.flags()[0] == 1 and other.flags()[0] == 0
    check_packed(closed, rs, "closed-run subject")
    check_packed(other, other.RS, "beside the closed-run subject")
    alone.build()
    assert (alone.download_index()[1] == other.download_index()[1]).all()
    for E in (closed, other, alone):
        E.close()


def test_build_scan_build_scan_on_one_context():
    """Different batches one after the other on one context of its own (the item buffer is reused): counts equal the
    oracle's every time, by either kind of scan kernel."""
    import andi_amd
    ctx = andi_amd.Context(0)
    Q = andi_amd.Queries(ctx, _seqs()[1])
    try:
        for round_, (names, coop) in enumerate(((["long", "other"], 4), (["other", "mid", "long"], 0), (["mid"], 4), (["long", "other"], 0))):
            with knobs(COOP=coop):
                esas = [_stage(ctx, n) for n in names]
                andi_amd.lib.build_indexes(ctx, esas)
            _scan_equals_oracle(ctx, esas, names, Q, coop, ("round", round_))
            for E in esas:
                assert (E.flags() == 0).all()
                E.close()
    finally:
        Q.close()
        ctx.close()
