"""A model of the device suffix sorter (andi_amd/csrc/sa_device.hip) and the texts that pin its branch points.

The reference of a short text is the naive sort of its suffixes; of a long one the host sorter (andi_amd.suffix_array,
held to the naive sort in tests/test_sa_model_host.py) plus conftest.verify_suffix_array on the device's result.  What
the model restates of the sorter:

  params(n)      (bits, syms): the width of a rank + 1 and the symbols a round-1 key has room for
  key0(text)     the round-0 key of every suffix: sixteen 2-bit codes, zeros from the first symbol on that is no
                 nucleotide (a separator or the text's end -- a "special" suffix)
  rounds(text)   the rounds the sorter must take, for texts over C, G, T without separators only: there the zeros of a
                 special's key (the code of A) equal nothing else, so round 0 leaves the pairs that share 16 symbols,
                 round 1 those that share 16 + syms, and every later round doubles what the groups are sorted by
  special_open(text)   whether a group still open after round 1 holds a special suffix (the next round then counts on
                 syms + 1 sorted symbols, not 16 + syms)

rounds() was written from the kernels' code alone; tests/test_sa_device_gpu.py holds the device's round count to it on
every text over C, G, T.  Outcome of the first comparison on an MI355X: see OUTCOME below.

The builders of the texts the two test modules share are here too; every one is deterministic.
"""
import functools
import itertools

import numpy as np

NAIVE_MAX = 5000  # texts up to this length have the naive sort as their reference
SA_SYMS = 16
TILE = 1024  # slots per block of the open-slot selection (SA_TILE)

OUTCOME = ("the device's sa_rounds equalled rounds() on every C, G, T text of tests/test_sa_device_gpu.py at the first run "
           "(56 texts with a planted unit, 18 periodic ones): neither side was changed")


# ---------------------------------------------------------------- references
def naive_sa(text: bytes):
    """byte order, a suffix before every longer one it is a prefix of: the order of the NUL-terminated text"""
    return np.array(sorted(range(len(text)), key=lambda i: text[i:]), dtype=np.int32)


def reference_sa(text: bytes):
    if len(text) <= NAIVE_MAX:
        return naive_sa(text)
    import andi_amd
    return andi_amd.suffix_array(text)


def params(n):
    """(bits, syms) as andi_sa_device computes them"""
    bits = 1
    while (1 << bits) < n + 2:
        bits += 1
    return bits, min(16, (64 - 7 - bits) // 3)


def lcp_array(text: bytes, sa):
    """lcp[r]: symbols shared by the suffixes at ranks r - 1 and r (Kasai); lcp[0] = 0"""
    n = len(text)
    sa = [int(x) for x in sa]
    rank = [0] * n
    for r, i in enumerate(sa):
        rank[i] = r
    lcp = [0] * n
    h = 0
    for i in range(n):
        r = rank[i]
        if r == 0:
            h = 0
            continue
        j = sa[r - 1]
        while i + h < n and j + h < n and text[i + h] == text[j + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return lcp


def max_lcp(text: bytes, sa=None):
    """the longest prefix two distinct suffixes share"""
    if len(text) < 2:
        return 0
    return max(lcp_array(text, reference_sa(text) if sa is None else sa))


def rounds(text: bytes, sa=None):
    """rounds of the device sorter on a text over C, G, T"""
    assert text and set(text) <= set(b"CGT"), "defined for texts over C, G, T only"
    m = max_lcp(text, sa)
    h = SA_SYMS + params(len(text))[1]
    if m < SA_SYMS:
        return 1
    if m < h:
        return 2
    r = 1
    while h << r <= m:
        r += 1
    return 2 + r


_CODE = np.full(256, 4, np.int64)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k


def key0(text: bytes):
    """(key, jj): the round-0 key of every suffix and where its first non-nucleotide is (16: not among the first 16)"""
    n = len(text)
    t = np.concatenate([_CODE[np.frombuffer(text, np.uint8)], np.full(SA_SYMS, 4, np.int64)])
    key, jj, alive = np.zeros(n, np.int64), np.full(n, SA_SYMS, np.int64), np.ones(n, bool)
    for j in range(SA_SYMS):
        c = t[j:j + n]
        stop = alive & (c == 4)
        jj[stop] = j
        alive &= c != 4
        key = key * 4 + np.where(alive, c, 0)
    return key, jj


def open_groups0(text: bytes, sa):
    """[first, last] slots of the groups of two or more equal round-0 keys, in suffix-array order"""
    k = key0(text)[0][np.asarray(sa, np.int64)]
    same = np.concatenate([[False], k[1:] == k[:-1], [False]])
    first = np.flatnonzero(~same[:-1] & same[1:])
    last = np.flatnonzero(same[:-1] & ~same[1:])
    return np.stack([first, last], axis=1)


def straddles_tile(text: bytes, sa):
    """a tie group of round 0 holds the last slot of one tile of the selection and the first of the next"""
    g = open_groups0(text, sa)
    return bool(len(g)) and bool((g[:, 0] // TILE != g[:, 1] // TILE).any())


def special_open(text: bytes):
    """two special suffixes leave round 1 with equal keys: the same nucleotides up to the same separator and the same
    syms symbols behind it"""
    syms = params(len(text))[1]
    _, jj = key0(text)
    seen = set()
    for i in np.flatnonzero(jj < SA_SYMS).tolist():
        j = int(jj[i])
        if i + j >= len(text):
            continue  # (the text's end: one suffix has it at offset j)
        k = (j, text[i:i + j + 1 + syms])
        if k in seen:
            return True
        seen.add(k)
    return False


# ---------------------------------------------------------------- texts
def dna(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, np.uint8), int(n)).tobytes()


@functools.lru_cache(None)
def exhaustive_texts():
    """every text of 1..8 over AC, 1..5 over AT!# and 1..3 over ACGT!;#: 510 + 1364 + 399"""
    out = []
    for alphabet, longest in ((b"AC", 8), (b"AT!#", 5), (b"ACGT!;#", 3)):
        for n in range(1, longest + 1):
            out += [bytes(t) for t in itertools.product(alphabet, repeat=n)]
    return out


@functools.lru_cache(None)
def length_ladder():
    """lengths 70 down to 1, then 1 up to 70; per length a random text over ACGT, one over AC and the homopolymer"""
    rng = np.random.default_rng(7001)
    out = []
    for n in list(range(70, 0, -1)) + list(range(1, 71)):
        out += [dna(rng, n), dna(rng, n, b"AC"), b"A" * n]
    return out


TILE_EDGE_LENGTHS = (1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)


def _straddling_text(n):
    """random over ACGT with a planted repeat whose tie group of round 0 lies across a tile's end"""
    for seed in range(200):
        rng = np.random.default_rng(7100 + 1000 * n + seed)
        t = bytearray(dna(rng, n))
        sa = naive_sa(bytes(t))
        edge = TILE * int(rng.integers(1, (n - 1) // TILE + 1))  # the first slot of a later tile
        src = int(sa[edge])
        if src + 20 > n:
            continue
        unit = bytes(t[src:src + 20])
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, n - 20))
            if abs(at - src) >= 24:
                t[at:at + 20] = unit
        t = bytes(t)
        if straddles_tile(t, naive_sa(t)):
            return t
    raise AssertionError("no straddling text of length %d" % n)


@functools.lru_cache(None)
def tile_edge_texts():
    """(name, text, must_straddle): must_straddle -- the text was built to have a tie group across a tile's end (the
    random texts over ACGT of more than one tile; the others may have one)"""
    rng = np.random.default_rng(7200)
    out = []
    for n in TILE_EDGE_LENGTHS:
        out.append(("period-2-%d" % n, (b"AC" * n)[:n], False))
        out.append(("random-AC-%d" % n, dna(rng, n, b"AC"), False))
        out.append(("random-ACGT-%d" % n, _straddling_text(n) if n > TILE else dna(rng, n), n > TILE))
    return out


def _no_repeat(rng, n, k):
    """random over C, G, T without a repeated k-mer: the longest prefix two suffixes share is below k"""
    t = rng.integers(0, 3, n)
    w = 3 ** np.arange(k - 1, -1, -1)
    for _ in range(10000):
        code = np.lib.stride_tricks.sliding_window_view(t, k) @ w
        order = np.argsort(code, kind="stable")
        dup = order[1:][code[order[1:]] == code[order[:-1]]]
        if len(dup) == 0:
            return t
        at = dup + rng.integers(0, k, len(dup))
        t[at] = rng.integers(0, 3, len(dup))
    raise AssertionError("no repeat-free text")


def shared_unit_text(n, L, seed=0):
    """n symbols over C, G, T with exactly two copies of a unit of L symbols, other symbols in front of and behind the
    copies, and nothing else that two suffixes share L symbols of: max_lcp == L (checked here, asserted in
    tests/test_sa_model_host.py)"""
    assert 15 <= L and 2 * L + 8 <= n
    k = 8
    while 3 ** k < 8 * n:
        k += 1
    assert k < 15
    for attempt in range(100):
        rng = np.random.default_rng(7300 + 131 * n + 17 * L + 100003 * seed + attempt)
        t = _no_repeat(rng, n, k)
        a = int(rng.integers(1, n - 2 * L - 3))
        b = int(rng.integers(a + L + 1, n - L - 1))
        t[b:b + L] = t[a:a + L]
        if t[b + L] == t[a + L]:
            t[b + L] = (t[b + L] + 1) % 3
        if t[b - 1] == t[a - 1]:
            t[b - 1] = (t[b - 1] + 1) % 3
        text = np.frombuffer(b"CGT", np.uint8)[t].tobytes()
        if max_lcp(text) == L:
            return text
    raise AssertionError("no text of %d symbols with max_lcp %d" % (n, L))


THRESHOLD_PAIRS = ((510, 511), (4094, 4095), (32766, 32767))


def threshold_shapes():
    """(n, L) of the key-width cases: around each length at which syms changes, pairs that agree on 15..17 symbols and
    on h - 1, h, h + 1, 2h - 1, 2h, 2h + 1 with h = 16 + syms(n); at 262142 | 262143 h alone"""
    out = []
    for pair in THRESHOLD_PAIRS:
        for n in pair:
            h = SA_SYMS + params(n)[1]
            out += [(n, L) for L in sorted({15, 16, 17, h - 1, h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1})]
    out += [(n, SA_SYMS + params(n)[1]) for n in (262142, 262143)]
    return out


@functools.lru_cache(None)
def threshold_text(n, L):
    return shared_unit_text(n, L)


def _unit(rng, p, alphabet):
    """a primitive word of p symbols (no shorter period) that uses the alphabet's letters in turn where it can"""
    for _ in range(1000):
        u = (alphabet * p)[:p] if p <= len(alphabet) else dna(rng, p, alphabet)
        if all(u[d:] + u[:d] != u for d in range(1, p)):
            return u
    raise AssertionError


PERIODS = (1, 2, 3, 5, 16, 17, 31, 33)


@functools.lru_cache(None)
def periodic_texts():
    """(name, text): periods over ACGT and over CGT at 1000 and 4099 symbols (4099 is prime, 1000 a multiple of 2 and 5
    alone: elsewhere the last period is cut), and random texts that end in a run or in a periodic stretch"""
    rng = np.random.default_rng(7400)
    out = []
    for alphabet in (b"ACGT", b"CGT"):
        for p in PERIODS:
            u = (b"A" if alphabet == b"ACGT" else b"T") if p == 1 else _unit(rng, p, alphabet)
            for n in (1000, 4099):
                out.append(("%s-period-%d-%d" % (alphabet.decode(), p, n), (u * (n // p + 1))[:n]))
        run = alphabet[:1] if alphabet == b"ACGT" else b"T"
        out.append(("%s-ends-in-run" % alphabet.decode(), dna(rng, 2000, alphabet) + run * 300))
        u = _unit(rng, 17, alphabet)
        out.append(("%s-ends-in-period-17" % alphabet.decode(), dna(rng, 2000, alphabet) + (u * 18)[:300]))
    return out


def _filler(rng, n):
    """random over C, G, T: nothing in it looks like a run of A"""
    return dna(rng, n, b"CGT")


def ties_at(jj, seed=0):
    """One text in which the prefix P of jj nucleotides is followed by !X, #X, ;X, !Y, sixteen A and then C, and (at the
    end) by the text's end: seven suffixes with one round-0 key, which round 1 must order by (jj, separator, behind)."""
    rng = np.random.default_rng(7500 + jj + 97 * seed)
    P = dna(rng, jj, b"CGT")  # (no A: the prefix's own suffixes get keys of their own)
    X, Y = b"CGTTGC", b"TGCCGT"
    parts = [P + b"!" + X, P + b"#" + X, P + b";" + X, P + b"!" + Y, P + b"A" * 16 + b"C"]
    order = rng.permutation(len(parts))
    t = b""
    for k in order:
        t += b"G" + _filler(rng, 30)[:int(rng.integers(20, 30))] + b"T" + parts[k]
    return t + b"!" + _filler(rng, 25) + b"T" + P


def copies_shapes():
    """(copies, contig length) of the texts of k copies of one contig joined by '!': lengths 1, 3, 15, 16, 17, syms,
    syms + 1, 40 and 700, syms that of the whole text"""
    out = []
    for k in (2, 5, 40):
        lengths = {1, 3, 15, 16, 17, 40, 700}
        for plus in (0, 1):
            lengths |= {L for L in range(10, 18) if params(k * L + k - 1)[1] + plus == L}
        out += [(k, L) for L in sorted(lengths)]
    return out


@functools.lru_cache(None)
def separator_texts():
    """(name, text) of the special path's cases"""
    rng = np.random.default_rng(7600)
    out = [("ties-at-%d" % jj, ties_at(jj)) for jj in range(16)]
    f = lambda n: _filler(rng, n)
    out.append(("same-prefix-two-offsets", f(40) + b"TAC!" + f(30) + b"TACAA!" + f(30) + b"TACAAAA!" + f(30) + b"TAC" + b"A" * 20 + f(5)))
    out.append(("same-prefix-two-offsets-at-the-end", f(40) + b"TACAA!" + f(30) + b"TAC"))
    out += [("adjacent-1", b"!!"), ("adjacent-2", b"!#;"), ("adjacent-3", b"A!!A"),
            ("adjacent-in-text", dna(rng, 50) + b"!!" + dna(rng, 20) + b"!#;" + dna(rng, 33) + b";;;;" + dna(rng, 18))]
    for n in range(1, 21):
        out.append(("begins-with-separator-%d" % n, (b"!" + dna(rng, n))[:n]))
        out.append(("ends-with-separator-%d" % n, (dna(rng, n) + b"!")[-n:]))
        out.append(("both-ends-%d" % n, b"#" + dna(rng, max(0, n - 2)) + b";" if n > 1 else b";"))
        out.append(("only-one-separator-%d" % n, b"!" * n))
        out.append(("only-separators-%d" % n, dna(rng, n, b"!#;")))
    for k, L in copies_shapes():
        out.append(("copies-%d-of-%d" % (k, L), b"!".join([dna(rng, L)] * k)))
    seps = [b"!", b"#", b";"]
    out.append(("short-mixed-contigs", b"".join(dna(rng, rng.integers(1, 16), b"AC" if c % 3 else b"ACGT") + seps[int(rng.integers(0, 3))]
                                                 for c in range(300))))
    out.append(("short-contigs-one-separator", b"!".join(dna(rng, rng.integers(1, 16), b"AC" if c % 3 else b"ACGT") for c in range(300))))
    return out


FOREIGN = (b"N", b"a", b"\x01", b"\xff")


def foreign_texts():
    """(text, following clean text): a byte outside the alphabet at 0, at n - 1 for each n mod 4, in the middle"""
    rng = np.random.default_rng(7700)
    out = []
    for k, bad in enumerate(FOREIGN):
        for n in (40, 41, 42, 43):
            out.append(dna(rng, n - 1) + bad)
        n = 37 + k
        out.append(bad + dna(rng, n - 1))
        out.append(dna(rng, n // 2) + bad + dna(rng, n - 1 - n // 2))
    out.append(dna(rng, 3000) + b"N" + dna(rng, 2000))
    return [(t, dna(rng, len(t) - 3)) for t in out]


def record_sequences():
    """the sequences among the texts of the length ladder, the tile edges and the separator cases: nucleotides and '!'"""
    seen, out = set(), []
    texts = length_ladder()[210:] + [t for _, t, _ in tile_edge_texts()] + [t for _, t in separator_texts()]
    for t in texts:
        if set(t) <= set(b"ACGT!") and t not in seen:
            seen.add(t)
            out.append(t)
    return out


def constructed_cases():
    """(name, text) of every constructed case, the long ones included"""
    out = [("ladder-%d" % k, t) for k, t in enumerate(length_ladder())]
    out += [(name, t) for name, t, _ in tile_edge_texts()]
    out += [("shared-%d-%d" % (n, L), threshold_text(n, L)) for n, L in threshold_shapes()]
    out += periodic_texts() + separator_texts()
    return out
