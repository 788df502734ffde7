"""Which tiles of k_probe_table (esa_build.hip: probe_table_block) are WHOLE, from the text alone, in NumPy, and the subjects
that tests/test_probe_table_tiles_gpu.py builds: what it asserts about them before it touches the device is computed here.

A block takes TILE suffix-array gaps r0 .. r0 + TILE - 1 and stages the records of the suffixes r0 - 2 .. r0 + TILE (two
before its own, one behind: the halo).  The tile is whole when r0 >= 2, r0 + TILE < n and every one of those TILE + 3
suffixes starts with K nucleotides; then the block runs its straight-line code, otherwise the general code.  Both must
write the same table."""
import functools

import numpy as np

import probe_table_model as ptm

TILE = ptm.TILE
RANKED = 4096  # PT_RANKED: entries of a block whose owners are found by rank


def by_rank(rs: bytes, sa, K):
    """(full, code) per suffix-array rank: the suffix starts with K nucleotides; their 2-bit code (garbage where not)"""
    for l, ok, pref in ptm._prefixes(rs, K):
        pass
    sa = np.asarray(sa, np.int64)
    return ok[sa], pref[sa]


def n_tiles(n):
    return (n + TILE) // TILE  # gaps 0 .. n


def whole_tiles(rs: bytes, sa, K, tile=TILE):
    """bool per tile: the block takes the straight-line path"""
    n = len(rs)
    full, _ = by_rank(rs, sa, K)
    short_before = np.concatenate([[0], np.cumsum(~full)])  # short records among the ranks below r
    r0 = np.arange((n + tile) // tile, dtype=np.int64) * tile
    inside = (r0 >= 2) & (r0 + tile < n)
    lo, hi = np.clip(r0 - 2, 0, n), np.clip(r0 + tile + 1, 0, n)
    return inside & (short_before[hi] == short_before[lo])


def halo_only_tiles(rs: bytes, sa, K, tile=TILE):
    """{tile: offsets} of the tiles inside the text whose own `tile` records are all full and whose halo is not: offsets
    among -2, -1 and `tile` (the ranks r0 - 2, r0 - 1, r0 + tile) of the short records"""
    n = len(rs)
    full, _ = by_rank(rs, sa, K)
    out = {}
    for b in range(1, (n + tile) // tile):
        r0 = b * tile
        if r0 + tile < n and full[r0:r0 + tile].all():
            short = [o for o in (-2, -1, tile) if not full[r0 + o]]
            if short:
                out[b] = short
    return out


def alternations(whole):
    """how often whole and non-whole tiles follow each other along the table"""
    w = np.asarray(whole, bool)
    return int((w[1:] != w[:-1]).sum())


def tile_entries(rs: bytes, sa, K, tile=TILE):
    """entries of the table that each WHOLE tile writes (0 for the others): from behind the K-mer of suffix r0 - 1 up to the
    K-mer of suffix r0 + tile - 1"""
    whole = whole_tiles(rs, sa, K, tile)
    _, code = by_rank(rs, sa, K)
    out = np.zeros(len(whole), np.int64)
    for b in np.flatnonzero(whole):
        out[b] = code[b * tile + tile - 1] - code[b * tile - 1]
    return out


def far_runs(rs: bytes, sa, K, tile=TILE):
    """the whole tiles in which a run of equal K-mers starts whose end the three records behind the gap do not show: more
    than three suffixes follow with the same K-mer, or the look-ahead leaves the staged records (the last two gaps of a
    tile) -- the kernel's `more` branch, reached from the straight-line path"""
    whole = whole_tiles(rs, sa, K, tile)
    n = len(rs)
    full, code = by_rank(rs, sa, K)
    key = np.where(full, code, -1 - np.arange(n))  # (short records equal nothing)
    head = np.concatenate([[True], key[1:] != key[:-1]])
    ahead3 = np.zeros(n, bool)
    ahead3[:n - 3] = key[3:] == key[:n - 3]  # records are sorted: the third one behind equal means all three are
    out = []
    for b in np.flatnonzero(whole):
        r0 = b * tile
        r = np.arange(r0, r0 + tile)
        if (head[r] & (ahead3[r] | (r - r0 + 5 >= tile + 3))).any():
            out.append(int(b))
    return out


def leaving_runs(rs: bytes, sa, K, tile=TILE):
    """the whole tiles in which a run of equal K-mers starts that ends in a later tile"""
    whole = whole_tiles(rs, sa, K, tile)
    _, code = by_rank(rs, sa, K)
    out = []
    for b in np.flatnonzero(whole):
        r0 = b * tile
        c = code[r0 + tile - 1]
        if code[r0 + tile] == c and code[r0 - 1] != c:  # (r0 + tile's record is full: the tile is whole)
            out.append(int(b))
    return out


# ---------------------------------------------------------------- the subjects
# seeds of 20 kbp random genomes (rng = default_rng(seed), ptm._dna(rng, 20000)) whose table of natural depth has a tile
# with a short record in the halo alone, at exactly one rank of it (the first seeds of 0, 1, 2 ... for which
# halo_only_tiles says so)
HALO_SEEDS = {-2: 83, -1: 3, TILE: 21}  # offset of the short record -> seed


@functools.lru_cache(None)
def subjects():
    """name -> sequence"""
    from andi_amd import synth
    s = {}
    s["random-40k"] = ptm._dna(np.random.default_rng(4001), 40000)
    s["joined-60"] = synth.join_contigs(s["random-40k"], 60)  # (120 contig ends, some 1100 short records: no tile of its 105 is whole)
    s["joined-6"] = synth.join_contigs(s["random-40k"], 6)  # (12 contig ends: about half of the tiles are whole)
    for off, seed in HALO_SEEDS.items():
        s["halo%+d" % off] = ptm._dna(np.random.default_rng(seed), 20000)
    s["acgt-x-2000"] = b"ACGT" * 2000
    rng = np.random.default_rng(4002)
    s["repeat-x-5000"] = ptm._dna(rng, 3000) + ptm._dna(rng, 7) * 5000 + ptm._dna(rng, 3000)
    s["tiny"] = b"ACGTTGCA"
    return s


@functools.lru_cache(None)
def texts():
    return {name: ptm.subject_text(seq) for name, seq in subjects().items()}


@functools.lru_cache(None)
def model_sa(name):
    return ptm.suffix_array(texts()[name])


def depth_of(name, depth):
    return ptm.natural_k(len(texts()[name])) + (depth == "natural+1") if isinstance(depth, str) else depth


@functools.lru_cache(None)
def facts(depth="natural"):
    """name -> what the tiles of the subject's table of the given depth ("natural", "natural+1" or a number) are like"""
    out = {}
    for name, rs in texts().items():
        sa, K = model_sa(name), depth_of(name, depth)
        whole = whole_tiles(rs, sa, K)
        entries = tile_entries(rs, sa, K)
        out[name] = {"K": K, "tiles": len(whole), "whole": int(whole.sum()), "alternations": alternations(whole),
                     "halo_only": halo_only_tiles(rs, sa, K), "far": len(far_runs(rs, sa, K)), "leaving": len(leaving_runs(rs, sa, K)),
                     "most_entries": int(entries.max()), "past_ranked": int((entries > RANKED).sum())}
    return out
