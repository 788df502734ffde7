"""The probe table of the scan index (andi_amd/csrc/andi_dev.h: DEEP_*; esa_build.hip: k_probe_table) restated from the
text alone, in NumPy: what tests/test_probe_table_*.py and tests/test_esa_gpu.py hold the device to.

For a K-mer w (a code of 2 K bits, first character most significant, A C G T = 0 1 2 3) the table says what the true
longest match of a query that starts with w is, as far as w alone decides it:

  SINGLE  w occurs once in RS      x = its position; y by the entry's form (table)
  MULTI   w occurs c > 1 times     x = the suffix-array rank of its first suffix, y = 2 | (c - 1) << 8
  FINAL   w does not occur         y = unique << 2 | l << 8: l < K the length of w's longest prefix that occurs, unique:
                                   exactly one suffix starts with that prefix -- and x = that suffix's rank where unique
                                   (the scan reads x of a FINAL entry nowhere else: it is not part of the contract there)

Two back ends make the same Entries: `entries(rs, K)` for EVERY code (np.bincount per prefix length: K <= 10, the arrays
have 4^K cells) and `entries(rs, K, codes)` for a list of codes at any K <= 13 (a sorted array of the text's valid l-mers
per prefix length and np.searchsorted: memory O(n + codes)).  The suffix array is the model's own (prefix doubling)."""
from collections import namedtuple

import numpy as np

FINAL, SINGLE, MULTI = 0, 1, 2
MAX_ALL_CODES_K = 10
MAX_K = 13

Entries = namedtuple("Entries", "K codes kind count l unique pos rank")
Entries.__doc__ = """per code: kind; count = occurrences of the K-mer; FINAL: l and unique, rank = rank of the one suffix
(where unique, else -1); SINGLE: pos = the position; MULTI: rank = the first rank.  Fields that do not apply are -1."""

_CODE = np.full(256, 4, np.int64)
_CODE[list(b"ACGT")] = [0, 1, 2, 3]


def suffix_array(rs: bytes):
    """suffix array of rs in unsigned byte order, a suffix that is a prefix of another first (prefix doubling)"""
    t = np.frombuffer(rs, np.uint8).astype(np.int64)
    n = len(t)
    rank = t + 1  # (0: beyond the text)
    h = 1
    while True:
        nxt = np.zeros(n, np.int64)
        if h < n:
            nxt[:n - h] = rank[h:]
        key = rank * (int(rank.max()) + 2) + nxt
        order = np.argsort(key, kind="stable")
        sk = key[order]
        new = np.empty(n, np.int64)
        new[order] = np.concatenate([[0], np.cumsum(sk[1:] != sk[:-1])]) + 1
        rank = new
        if int(rank.max()) == n or h >= n:
            return order.astype(np.int64)
        h *= 2


def _prefixes(rs: bytes, K):
    """per l = 1..K: (ok, pref): positions with at least l leading nucleotides, and their l-mer codes"""
    t = np.concatenate([_CODE[np.frombuffer(rs, np.uint8)], np.full(K, 4, np.int64)])
    n = len(rs)
    ok, pref = np.ones(n, bool), np.zeros(n, np.int64)
    for l in range(1, K + 1):
        s = t[l - 1:l - 1 + n]
        ok = ok & (s < 4)
        pref = pref * 4 + np.minimum(s, 3)
        yield l, ok, pref


def entries(rs: bytes, K, codes=None, sa=None):
    """Entries of the K-mers `codes` (None: every one, K <= 10) of the text rs (the subject's RS)."""
    assert 1 <= K <= MAX_K
    n = len(rs)
    sa = suffix_array(rs) if sa is None else np.asarray(sa, np.int64)
    rank_of = np.empty(n, np.int64)
    rank_of[sa] = np.arange(n)
    every = codes is None
    if every:
        assert K <= MAX_ALL_CODES_K, "all-code arrays only up to K = 10"
        codes = np.arange(4 ** K, dtype=np.int64)
    else:
        codes = np.asarray(codes, np.int64)
        assert ((codes >= 0) & (codes < 4 ** K)).all()
    # the longest prefix that occurs (l = 0: the empty one, shared by all n suffixes), its count, the least rank among its suffixes
    m = 1 if every else len(codes)
    best_l, best_cnt, best_rank = np.zeros(m, np.int64), np.full(m, n, np.int64), np.zeros(m, np.int64)
    for l, ok, pref in _prefixes(rs, K):
        p = np.nonzero(ok)[0]
        if every:  # cell c of length l: from its parent c >> 2, then its own occurrences
            best_l, best_cnt, best_rank = (np.repeat(a, 4) for a in (best_l, best_cnt, best_rank))
            cnt = np.bincount(pref[p], minlength=4 ** l)
            first = np.full(4 ** l, n, np.int64)
            np.minimum.at(first, pref[p], rank_of[p])
        else:
            c = codes >> (2 * (K - l))
            p = p[np.argsort(rank_of[p], kind="stable")]  # in suffix-array order, then by code: the first of a code has its least rank
            o = np.argsort(pref[p], kind="stable")
            vals, ranks = pref[p][o], rank_of[p][o]
            lo, hi = np.searchsorted(vals, c, "left"), np.searchsorted(vals, c, "right")
            cnt = hi - lo
            first = np.concatenate([ranks, [n]])[lo]
        hit = cnt > 0
        best_l[hit], best_cnt[hit], best_rank[hit] = l, cnt[hit], first[hit]
        if l == K:
            count = cnt
    kind = np.where(count == 0, FINAL, np.where(count == 1, SINGLE, MULTI))
    fin, one, many = kind == FINAL, kind == SINGLE, kind == MULTI
    unique = np.where(fin, (best_cnt == 1).astype(np.int64), -1)
    return Entries(K=K, codes=codes, kind=kind, count=count, l=np.where(fin, best_l, -1), unique=unique,
                   pos=np.where(one, sa[np.minimum(best_rank, n - 1)], -1),
                   rank=np.where(many | (fin & (unique == 1)), best_rank, -1))


def present_codes(rs: bytes, K):
    """the codes of the K-mers that occur in rs, ascending"""
    for l, ok, pref in _prefixes(rs, K):
        pass
    return np.unique(pref[ok])


def behind(rs: bytes, pos, K, room):
    """(count, ext): the nucleotides behind the K-mers at `pos`, up to `room` of them and up to the first symbol that is
    none (a separator, '#', the text's end), and their 2-bit codes, the first in the low bits"""
    pos = np.asarray(pos, np.int64)
    t = np.concatenate([_CODE[np.frombuffer(rs, np.uint8)], np.full(K + room + 1, 4, np.int64)])
    cnt, ext, alive = np.zeros(len(pos), np.int64), np.zeros(len(pos), np.int64), np.ones(len(pos), bool)
    for j in range(room):
        s = t[pos + K + j]
        alive = alive & (s < 4)
        cnt += alive
        ext |= np.where(alive, s, 0) << (2 * j)
    return cnt, ext


def form_room(form, K):
    """symbols an entry of the given form holds behind its K-mer (andi_dev.h: EsaDev.deep_ext)"""
    return {0: 0, 1: 13, 2: min(4, 16 - K)}[form]


def table(rs: bytes, E: Entries, form):
    """(x, y, x_defined): the table's words for E's codes with SINGLE entries of the given form (0 plain, 1 extended,
    2 short extended); x_defined: x is part of the contract"""
    K = E.K
    x, y = np.zeros(len(E.codes), np.int64), np.zeros(len(E.codes), np.int64)
    fin, one, many = E.kind == FINAL, E.kind == SINGLE, E.kind == MULTI
    y[fin] = FINAL | (E.unique[fin] << 2) | (E.l[fin] << 8)  # bits 3..7 zero
    x[fin] = np.maximum(E.rank[fin], 0)
    y[many] = MULTI | ((E.count[many] - 1) << 8)  # bits 2..7 zero
    x[many] = E.rank[many]
    x[one] = E.pos[one]
    if form == 0:
        y[one] = SINGLE | (1 << 2) | (K << 8)
    else:
        cnt, ext = behind(rs, E.pos[one], K, form_room(form, K))
        y[one] = SINGLE | (cnt << 2) | (ext << 6)
    return x.astype(np.uint32), y.astype(np.uint32), ~fin | (E.unique == 1)


def closed_run_flag(rs: bytes):
    """flags[0] of the index build: 1 if some word of 1..8 nucleotides occurs at least twice in rs
    and every occurrence is followed by the same contig separator, '!' or ';' -- the superset of the texts on which the
    reference's 10-mer table differs from the true longest match that the build detects."""
    nxt = np.concatenate([np.frombuffer(rs, np.uint8), np.zeros(9, np.uint8)])
    for l, ok, pref in _prefixes(rs, 8):
        p = np.nonzero(ok)[0]
        follower = nxt[p + l]
        total = np.bincount(pref[p], minlength=4 ** l)
        for sep in b"!;":
            same = np.bincount(pref[p][follower == sep], minlength=4 ** l)
            if ((total >= 2) & (same == total)).any():
                return 1
    return 0


# ---------------------------------------------------------------- texts with the properties the tests need
_RC = bytes.maketrans(b"ACGT!", b"TGCA;")


def subject_text(seq: bytes):
    """RS = revcomp(S) '#' S (src/sequence.c:143-219; the contig separator '!' becomes ';' on the reverse strand)"""
    return seq[::-1].translate(_RC) + b"#" + seq


def natural_k(n):
    """the table's depth for a text of n characters: the smallest K with 4^K >= n, within 4..13 (api.hip: pick_deep_k)"""
    K = 4
    while K < MAX_K and 4 ** K < n:
        K += 1
    return K


def _dna(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, np.uint8), int(n)).tobytes()


RUN_COUNTS = (1, 2, 3, 4, 5, 16, 17, 18, 19)  # around k_probe_table's look-ahead of three records and its walk to 16
TILE = 768  # suffix-array gaps per block of k_probe_table (PT_TILE)


def run_lengths_text():
    """A sequence whose K-mers (natural K) occur exactly 1, 2, 3, 4, 5, 16, 17, 18, 19 and >= 1000 times: units repeated
    that often between random spacers and a tandem repeat; seeds are tried until a run of 2..5 and a run of 16..19 start
    in the last three gaps of a tile.  Returns (seq, facts), facts = what was found (run_lengths_facts)."""
    for seed in range(1000, 1400):
        rng = np.random.default_rng(seed)
        parts = []
        for c in RUN_COUNTS:
            unit = _dna(rng, 14)
            for _ in range(c):
                parts += [unit, _dna(rng, rng.integers(6, 12))]
        parts.append(_dna(rng, 5) * 1010)
        seq = b"".join(parts)
        facts = run_lengths_facts(seq)
        if set(RUN_COUNTS) <= facts["counts"] and facts["longest"] >= 1000 and facts["short_at_tile_end"] and facts["long_at_tile_end"]:
            return seq, facts
    raise AssertionError("no seed gives the run lengths at a tile's end")


def run_lengths_facts(seq: bytes):
    rs = subject_text(seq)
    E = entries(rs, natural_k(len(rs)))
    many = E.kind == MULTI
    at_end = many & (E.rank % TILE >= TILE - 3)
    return {"counts": set(np.unique(E.count).tolist()), "longest": int(E.count.max()),
            "short_at_tile_end": bool((at_end & (E.count <= 5)).any()),
            "long_at_tile_end": bool((at_end & (E.count >= 16) & (E.count <= 19)).any())}


BEHIND = (1, 3, 4, 12, 13)  # where form 2's count (min(4, 16 - K)) and form 1's (13) saturate


def single_ends_text():
    """Joined contigs whose once-occurring K-mers (natural K) include one that ends exactly at the end of RS, at the '#',
    at a '!' and at a ';', and ones with exactly 1, 3, 4, 12, 13 and >= 14 nucleotides behind them before a symbol that is
    none.  Returns (seq, facts), facts = single_ends_facts(seq)."""
    for seed in range(2000, 2400):
        rng = np.random.default_rng(seed)
        seq = b"!".join(_dna(rng, rng.integers(25, 60)) for _ in range(10))
        facts = single_ends_facts(seq)
        if {0, ord("#"), ord("!"), ord(";")} <= facts["ends_at"] and set(BEHIND) <= facts["behind"] and facts["far"]:
            return seq, facts
    raise AssertionError("no seed gives every end")


def single_ends_facts(seq: bytes):
    rs = subject_text(seq)
    K = natural_k(len(rs))
    E = entries(rs, K)
    pos = E.pos[E.kind == SINGLE]
    cnt, _ = behind(rs, pos, K, 15)
    stop = np.frombuffer(rs + bytes(K + 16), np.uint8)[pos + K + cnt]  # (a count of 15: whatever is there)
    return {"ends_at": set(stop[cnt == 0].tolist()), "behind": set(cnt[(cnt < 14) & (stop != 0)].tolist()),
            "far": bool((cnt >= 14).any())}


def closed_run_subject(wlen, K, seed=0):
    """Three joined contigs, natural depth K (5..9), with a word w of wlen nucleotides that occurs exactly twice in RS,
    both times at a contig's end: a closed run "w!".  Returns (seq, w).  (w holds the text's only G -- and, from three
    nucleotides on, a C behind it, so that its reverse complement needs a G as well.)"""
    total = {5: 340, 6: 1500, 7: 6000, 8: 20000, 9: 35000}[K]
    rng = np.random.default_rng(7000 + 100 * K + wlen + 10007 * seed)
    while True:
        if wlen <= 2:
            alphabet, w = b"AT", (b"G", b"GA")[wlen - 1]
        else:
            alphabet, w = b"ACT", b"GC" + _dna(rng, wlen - 2, b"ACT")
        lens = [total // 2, total // 3, total - total // 2 - total // 3]
        c = [bytearray(_dna(rng, n, alphabet)) for n in lens]
        c[0][-wlen:] = w
        c[1][-wlen:] = w
        seq = b"!".join(bytes(x) for x in c)
        rs = subject_text(seq)
        at = [p for p in range(len(rs)) if rs.startswith(w, p)]
        if len(at) == 2 and all(rs[p + wlen:p + wlen + 1] == b"!" for p in at) and natural_k(len(rs)) == K:
            return seq, w
