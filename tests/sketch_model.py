"""The contract of the k-mer sketch screen (include/andi_hip.h: andi_hip_sketch, andi_hip_sketch_shared,
andi_hip_screen_select, and the lines of andi-hip's --screen-report) in NumPy.  All integers.

sketch_loop() is the same contract as a plain loop over the windows in Python integers; tests/test_sketch_host.py holds
the two against each other."""
import numpy as np

M64 = (1 << 64) - 1
_CODE = np.full(256, 4, np.uint8)
for _c, _v in zip(b"ACGT", range(4)):
    _CODE[_c] = _v


def fmix64(h):
    """MurmurHash3's 64-bit finaliser on a uint64 array (arithmetic mod 2^64)."""
    h = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def sketch(seq: bytes, k: int, scale: int):
    """The ascending uint64 array of the kept hashes of seq (bytes over A C G T !), each once."""
    assert 4 <= k <= 32 and scale >= 1
    code = _CODE[np.frombuffer(bytes(seq), np.uint8)]
    n = len(code)
    if n < k:
        return np.zeros(0, np.uint64)
    w = n - k + 1
    f = np.zeros(w, np.uint64)
    r = np.zeros(w, np.uint64)
    bad = np.zeros(w, bool)
    for j in range(k):  # symbol j of every window: 2(k - 1 - j) bits up in f; its complement 2j bits up in r
        c = code[j:j + w]
        bad |= c > 3
        c = (c & 3).astype(np.uint64)
        f |= c << np.uint64(2 * (k - 1 - j))
        r |= (np.uint64(3) - c) << np.uint64(2 * j)
    h = fmix64(np.minimum(f, r)[~bad])
    return np.unique(h[h <= np.uint64(M64 // scale)])


def sketch_loop(seq: bytes, k: int, scale: int):
    """The same, window by window in Python integers."""
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    val = {65: 0, 67: 1, 71: 2, 84: 3}
    out = set()
    seq = bytes(seq)
    for i in range(len(seq) - k + 1):
        win = seq[i:i + k]
        if any(c not in val for c in win):
            continue
        f = r = 0
        for c in win:
            f = f << 2 | val[c]
        for c in reversed(win):
            r = r << 2 | val[comp[c]]
        h = min(f, r)
        h ^= h >> 33
        h = h * 0xff51afd7ed558ccd & M64
        h ^= h >> 33
        h = h * 0xc4ceb9fe1a85ec53 & M64
        h ^= h >> 33
        if h <= M64 // scale:
            out.add(h)
    return np.array(sorted(out), np.uint64)


def revcomp(seq: bytes) -> bytes:
    return bytes(seq)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def shared(A, B):
    """The number of hashes in both sketches."""
    return int(np.intersect1d(A, B, assume_unique=True).size)


def shared_matrix(As, Bs):
    return np.array([[shared(a, b) for b in Bs] for a in As], np.uint32).reshape(len(As), len(Bs))


def select(sh, keep, min_shared=1):
    """(kept, taken): every query (row) takes references in the order (shared descending, index ascending), the first
    `keep` whose count is >= max(1, min_shared)."""
    sh = np.asarray(sh, np.uint32)
    nq, nr = sh.shape
    kept, taken = np.zeros(nr, bool), np.zeros(nq, np.uint32)
    floor = max(1, int(min_shared))
    for q in range(nq):
        order = sorted(range(nr), key=lambda r: (-int(sh[q, r]), r))
        mine = [r for r in order if sh[q, r] >= floor][:keep]
        kept[mine] = True
        taken[q] = len(mine)
    return kept, taken


REPORT_HEADER = "#query\treference\tshared\tquery_hashes\treference_hashes\tcontainment\tkept\n"


def report(sh, query_names, ref_names, query_sizes, ref_sizes, kept):
    """The text of --screen-report: one line per pair with shared >= 1, query-major, references in input order."""
    lines = [REPORT_HEADER]
    for q, qn in enumerate(query_names):
        for r, rn in enumerate(ref_names):
            if sh[q][r] >= 1:
                lines.append("%s\t%s\t%d\t%d\t%d\t%.6f\t%d\n" % (qn, rn, sh[q][r], query_sizes[q], ref_sizes[r],
                                                               float(sh[q][r]) / float(query_sizes[q]), int(kept[r])))
    return "".join(lines)
