"""The k-mer sketch screen on the device (andi_amd/csrc/sketch.hip) against its contract in NumPy (tests/sketch_model.py):
sketches at every window shape the hash kernel can meet, the shared counts through LDS and through global memory, at the
sketch sizes where k_shared's launch changes and against more sketches than its wavefronts take in one trip, the one call, and andi-hip --screen.  Every device result must be EQUAL to the model's."""
import json
import os
import subprocess

import numpy as np
import pytest

import sketch_model as sm
from conftest import ROOT, knobs, rand_dna

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
P = 64                 # sketch.hip: window end positions of a thread of k_hash
WAVE = 64 * P          # ... of a wavefront
BLOCK = 256 * P        # ... of a block (HASH_BLOCK = 256 threads)
SORT_WHOLE = 1 << 16   # a slice with more hashes than this is sorted by a device-wide sort of its own
SHAPES = [(4, 1), (15, 16), (21, 1), (21, 1000), (31, 4), (32, 1), (32, 7)]


def _with_bangs(seq, at):
    b = bytearray(seq)
    for i in at:
        b[i] = ord("!")
    return bytes(b)


def _sequences(k):
    """The set of one sketch call: the lengths around k, a thread's, a wavefront's and a block's span (many of them odd, so
    that later sequences start on an odd nibble), separators at those boundaries, repeats, an empty sequence."""
    rng = np.random.default_rng(1000 + k)
    seqs = [rand_dna(rng, n) for n in (1, k - 1, k, k + 1, P - 1, P, P + 1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1)]
    long = rand_dna(rng, BLOCK + 3 * P + 5)
    for edge in (P, WAVE, BLOCK):  # '!' just before, just behind and on both sides of the boundary
        seqs += [_with_bangs(long, [edge - 1]), _with_bangs(long, [edge]), _with_bangs(long, [edge - 1, edge])]
    seqs.append(_with_bangs(long, list(range(P - 3, P + 4)) + list(range(WAVE - k, WAVE)) + [0, len(long) - 1]))  # runs
    seqs.append(_with_bangs(long, range(k - 1, len(long), k)))  # no window at all: a '!' in every one
    seqs += [b"!" * 101, b"", b"AC" * 3000, b"A" * 5001, b"ACGT!ACGTA", rand_dna(rng, 777, b"ACGT!")]
    return seqs


def _model(seqs, k, scale):
    return [sm.sketch(s, k, scale) for s in seqs]


def _assert_sketches(S, want):
    assert len(S) == len(want)
    assert S.sizes.tolist() == [len(w) for w in want]
    for i, w in enumerate(want):
        got = S.hashes(i)
        assert got.dtype == np.uint64 and np.array_equal(got, w), "sketch %d" % i


@pytest.fixture(scope="module")
def cases():
    """sequences and the model's sketches, once per shape"""
    out = {}
    for k, scale in SHAPES:
        seqs = _sequences(k)
        out[k, scale] = (seqs, _model(seqs, k, scale))
    return out


@pytest.mark.parametrize("k,scale", SHAPES)
def test_sketches_equal_the_model(ctx, cases, k, scale):
    import andi_amd
    seqs, want = cases[k, scale]
    S = andi_amd.sketch(ctx, seqs, k, scale)
    _assert_sketches(S, want)
    if scale == 1:  # the repeats: thousands of survivors, one or two hashes
        assert S.sizes[seqs.index(b"A" * 5001)] == 1 and 1 <= S.sizes[seqs.index(b"AC" * 3000)] <= 2
    S.close()


def test_sketches_do_not_depend_on_the_batching(ctx, cases):
    """ANDI_SKETCH_BATCH=1: every sequence is a batch of its own, so a batch boundary falls between any two sequences;
    3000 packed bytes: batches of several short sequences and of one long one.  (One test, so that a run against the
    shipped library, which has no hooks, skips one.)"""
    import andi_amd
    for k, scale in SHAPES:
        seqs, want = cases[k, scale]
        for batch in (1, 3000):
            with knobs(SKETCH_BATCH=batch):
                S = andi_amd.sketch(ctx, seqs, k, scale)
                _assert_sketches(S, want)
                S.close()


def test_a_slice_longer_than_the_segmented_sort_takes(ctx):
    import andi_amd
    rng = np.random.default_rng(5)
    seqs = [rand_dna(rng, 999), rand_dna(rng, SORT_WHOLE + 4001), rand_dna(rng, 1001), rand_dna(rng, SORT_WHOLE + 20)]
    want = _model(seqs, 21, 1)
    assert len(want[1]) > SORT_WHOLE and len(want[3]) <= SORT_WHOLE + 1
    S = andi_amd.sketch(ctx, seqs, 21, 1)
    _assert_sketches(S, want)
    S.close()


def test_a_scale_that_empties_every_sketch(ctx, cases):
    import andi_amd
    seqs = [s for s in cases[21, 1][0] if s != b"A" * 5001]  # (without the run of A: its code is 0 and fmix64(0) = 0, kept at any scale)
    assert not any(len(w) for w in _model(seqs, 21, sm.M64))
    S = andi_amd.sketch(ctx, seqs, 21, sm.M64)  # kept iff h <= 1
    assert not S.sizes.any() and all(len(S.hashes(i)) == 0 for i in range(len(S)))
    A = andi_amd.sketch_shared(ctx, S, S)
    assert A.shape == (len(seqs), len(seqs)) and not A.any()
    S.close()


# ---------------------------------------------------------------- shared counts
K16 = 16


def _kmer_pool():
    """distinct random 16-mers in ascending order of their hash"""
    rng = np.random.default_rng(77)
    kmers = sorted({rand_dna(rng, K16) for _ in range(700)}, key=lambda m: int(sm.sketch(m, K16, 1)[0]))
    hashes = [int(sm.sketch(m, K16, 1)[0]) for m in kmers]
    assert len(set(hashes)) == len(hashes)
    return kmers


def _kmer_sets():
    """Sequences whose sketches (k = 16, scale = 1) are chosen sets of hashes: 16-mers joined by '!', one window each.
    pool: distinct random 16-mers in ascending order of their hash."""
    kmers = _kmer_pool()
    join = lambda idx: b"!".join(kmers[i] for i in idx)
    n = len(kmers)
    sets = {
        "one": [5], "s63": range(100, 163), "s64": range(100, 164), "s65": range(100, 165), "copy65": range(100, 165),
        "disjoint": range(300, 420), "empty": [],
        "first_a": [0] + list(range(11, 200, 2)), "first_b": [0] + list(range(12, 200, 2)),     # share only their first hash
        "last_a": list(range(201, 400, 2)) + [n - 1], "last_b": list(range(202, 400, 2)) + [n - 1],  # ... only their last
        "big": range(0, n, 1), "s200": range(50, 250),
    }
    names = list(sets)
    return names, [join(sets[m]) for m in names]


@pytest.fixture(scope="module")
def kmer_sets():
    names, seqs = _kmer_sets()
    want = _model(seqs, K16, 1)
    return names, seqs, want, sm.shared_matrix(want, want)


def test_shared_counts_equal_the_model(ctx, kmer_sets):
    import andi_amd
    names, seqs, want, M = kmer_sets
    at = {m: i for i, m in enumerate(names)}
    # what the inputs are: identical, disjoint, an empty side, only the first / only the last hash in common, the sizes
    assert [len(want[at[m]]) for m in ("one", "s63", "s64", "s65", "empty")] == [1, 63, 64, 65, 0]
    assert M[at["s65"], at["copy65"]] == 65 and M[at["disjoint"], at["s65"]] == 0 and not M[at["empty"]].any()
    assert M[at["first_a"], at["first_b"]] == 1 and want[at["first_a"]][0] == want[at["first_b"]][0]
    assert M[at["last_a"], at["last_b"]] == 1 and want[at["last_a"]][-1] == want[at["last_b"]][-1]
    S = andi_amd.sketch(ctx, seqs, K16, 1)
    _assert_sketches(S, want)
    T = andi_amd.sketch(ctx, seqs[::-1], K16, 1)
    same = andi_amd.sketch_shared(ctx, S, S)  # a == b
    assert same.dtype == np.uint32 and np.array_equal(same, M)
    cross = andi_amd.sketch_shared(ctx, S, T)
    assert np.array_equal(cross, M[:, ::-1])
    sub = andi_amd.sketch(ctx, seqs[:3], K16, 1)
    assert np.array_equal(andi_amd.sketch_shared(ctx, sub, S), M[:3]) and np.array_equal(andi_amd.sketch_shared(ctx, S, sub), M[:, :3])
    for X in (S, T, sub):
        X.close()


def test_shared_counts_through_lds_and_through_global_memory(ctx, kmer_sets):
    """ANDI_SKETCH_LDS=64: the sketches of 63 and 64 hashes are staged, those of 65 and more are searched where they lie;
    without the hook every one is staged.  Equal numbers."""
    import andi_amd
    names, seqs, want, M = kmer_sets
    S = andi_amd.sketch(ctx, seqs, K16, 1)
    free = andi_amd.sketch_shared(ctx, S, S)
    with knobs(SKETCH_LDS=64):
        forced = andi_amd.sketch_shared(ctx, S, S)
    with knobs(SKETCH_LDS=1):  # (only the sketch of one hash is staged)
        forced1 = andi_amd.sketch_shared(ctx, S, S)
    assert np.array_equal(free, M) and np.array_equal(forced, M) and np.array_equal(forced1, M)
    S.close()


# ---------------------------------------------------------------- k_shared: the sizes at which its launch changes
LDS_64K = 65536 // 8   # hashes: up to here the launch takes its dynamic LDS without asking for the attribute
LDS_MAX = 20000        # sketch.hip: SKETCH_LDS_MAX, the longest sketch that is staged (160 000 bytes)
STAGED_SIZES = [100, LDS_64K, LDS_64K + 1, LDS_MAX, LDS_MAX + 1, 25000]


def _prefix_with(seq, size):
    """the shortest prefix of seq whose model sketch (k = 16, scale = 1) has exactly `size` hashes: a base more adds at
    most one hash, so the sizes of the prefixes pass through every number on their way up"""
    lo, hi = 0, len(seq)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(sm.sketch(seq[:mid], K16, 1)) < size:
            lo = mid + 1
        else:
            hi = mid
    return seq[:lo]


def _mutated(rng, seq, rate):
    b = np.frombuffer(seq, np.uint8).copy()
    at = np.nonzero(rng.random(len(b)) < rate)[0]
    b[at] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), b[at])]
    return b.tobytes()


def _sized_sketches():
    """(A, B, the model's sketches of both): A has sketches of exactly STAGED_SIZES hashes (prefixes of one random
    sequence, so each holds the ones before it) and an empty one; B has the same, prefixes of an unrelated sequence, and
    copies of three of A's with a base in 50 changed -- counts that are full, zero and in between."""
    rng = np.random.default_rng(160000)
    seq, other = rand_dna(rng, 26_000), rand_dna(rng, 26_000)
    A = [_prefix_with(seq, s) for s in STAGED_SIZES] + [b""]
    B = A + [other[:5000], other] + [_mutated(rng, A[i], 0.02) for i in (1, 2, 5)]
    wa, wb = _model(A, K16, 1), _model(B, K16, 1)
    assert [len(w) for w in wa] == STAGED_SIZES + [0]
    M = sm.shared_matrix(wa, wb)
    assert M[:6, :6].tolist() == [[min(a, b) for b in STAGED_SIZES] for a in STAGED_SIZES] and not M[:, 6:9].any()
    for col, i in zip((9, 10, 11), (1, 2, 5)):  # a changed base takes up to 16 windows with it: some hashes stay, not all
        assert 0 < M[0, col] < 100 and STAGED_SIZES[i] // 4 < M[i, col] < STAGED_SIZES[i]
    return A, B, wa, wb


@pytest.fixture(scope="module")
def sized_sketches():
    return _sized_sketches()


def _assert_shared(ctx, S, T, want_s, want_t):
    import andi_amd
    got = andi_amd.sketch_shared(ctx, S, T)
    assert got.dtype == np.uint32 and np.array_equal(got, sm.shared_matrix(want_s, want_t))


def test_shared_counts_at_the_sizes_where_the_launch_changes(ctx, sized_sketches):
    """The first set's longest staged sketch decides k_shared's launch: up to 8192 hashes it takes 65 536 bytes of dynamic
    LDS as it is; from 8193 on it asks for the attribute first; with 20000 it takes all 160 000 bytes, and in that same
    launch the sketches of 20001 and 25000 hashes are searched in global memory.  In this order, so that a process that
    runs this test first meets the launches in ascending order of what they ask for."""
    import andi_amd
    A, B, wa, wb = sized_sketches
    SB = andi_amd.sketch(ctx, B, K16, 1)
    _assert_sketches(SB, wb)
    for upto in (LDS_64K, LDS_64K + 1, 25000):
        keep = [i for i, w in enumerate(wa) if len(w) <= upto]
        SA = andi_amd.sketch(ctx, [A[i] for i in keep], K16, 1)
        part = [wa[i] for i in keep]
        assert max(len(w) for w in part) == upto
        _assert_sketches(SA, part)
        _assert_shared(ctx, SA, SB, part, wb)
        _assert_shared(ctx, SA, SA, part, part)
        if upto == 25000:
            _assert_shared(ctx, SB, SA, wb, part)
        SA.close()
    SB.close()


def test_shared_counts_of_long_sketches_forced_through_global_memory(ctx, sized_sketches):
    """ANDI_SKETCH_LDS=64: none of these sketches but the empty one is staged.  Equal numbers."""
    import andi_amd
    A, B, wa, wb = sized_sketches
    SA, SB = andi_amd.sketch(ctx, A, K16, 1), andi_amd.sketch(ctx, B, K16, 1)
    with knobs(SKETCH_LDS=64):
        _assert_shared(ctx, SA, SB, wa, wb)
        _assert_shared(ctx, SB, SA, wb, wa)
    SA.close(), SB.close()


def _many_sketches(nb):
    """(A, B, the model's sketches of both, the model's counts): B has nb sketches of 1 to 70 16-mers of the pool, A five --
    65 hashes, the whole pool, one hash, none, 200.  k_shared gives a block's four wavefronts the sketches b = 4 * group +
    wave of B and then every 256th from there (64 groups), so b >= 256 is the loop's second trip and b >= 512 its third;
    nb = 256 is the last size with one.  An empty sketch sits in the second trip at b = 258."""
    kmers = _kmer_pool()
    rng = np.random.default_rng(nb)
    join = lambda idx: b"!".join(kmers[i] for i in idx)
    A = [join(range(100, 165)), join(range(len(kmers))), join([5]), b"", join(range(50, 250))]
    B = [join(rng.choice(len(kmers), int(rng.integers(1, 71)), replace=False)) for _ in range(nb)]
    if nb > 258:
        B[258] = b""
    wa, wb = _model(A, K16, 1), _model(B, K16, 1)
    M = sm.shared_matrix(wa, wb)
    assert [len(w) for w in wa] == [65, len(kmers), 1, 0, 200] and all(1 <= len(w) <= 70 for b, w in enumerate(wb) if b != 258)
    assert M[1].tolist() == [len(w) for w in wb] and M[:, -1].any() and not M[3].any()  # the last column is live
    assert 0 < M[0].sum() < M[1].sum() and 0 < M[4].sum() < M[1].sum() and (M[0] != M[4]).any()
    if nb > 256:  # ... and so is the first of the second trip
        assert M[:, 256].any() and (nb <= 258 or not M[:, 258].any())
    return A, B, wa, wb, M


@pytest.mark.parametrize("nb", [256, 257, 261, 600])
def test_shared_counts_against_more_sketches_than_one_trip_takes(ctx, nb):
    import andi_amd
    A, B, wa, wb, M = _many_sketches(nb)
    SA, SB = andi_amd.sketch(ctx, A, K16, 1), andi_amd.sketch(ctx, B, K16, 1)
    _assert_sketches(SB, wb)
    assert np.array_equal(andi_amd.sketch_shared(ctx, SA, SB), M)
    assert np.array_equal(andi_amd.sketch_shared(ctx, SB, SA), M.T)
    SA.close(), SB.close()


def test_sketch_sets_of_another_k_or_scale_are_refused(ctx):
    import andi_amd
    seqs = [b"ACGTTGCAACGTAGCTAGCTAGGATCGATCGTAGCTAGCATCGAT"]
    A, B, C_ = andi_amd.sketch(ctx, seqs, 15, 1), andi_amd.sketch(ctx, seqs, 16, 1), andi_amd.sketch(ctx, seqs, 15, 2)
    for other in (B, C_):
        with pytest.raises(andi_amd.AndiHipError, match="differ"):
            andi_amd.sketch_shared(ctx, A, other)
    assert andi_amd.sketch_shared(ctx, A, A).tolist() == [[len(sm.sketch(seqs[0], 15, 1))]]
    with pytest.raises(andi_amd.AndiHipError, match="alphabet"):
        andi_amd.sketch(ctx, [b"ACGTNACGTACGTACGTACGTACGT"], 15, 1)
    for X in (A, B, C_):
        X.close()


# ---------------------------------------------------------------- the one call, the command line
def _family():
    """One base of 20 kbp; references at d = 0.01, 0.03, 0.1, 0.3 and three unrelated genomes; the query at d = 0.005.  With
    these seeds the model (k = 15, scale = 16) gives a query sketch of 1252 hashes and shared counts 978, 779, 249, 15, 0, 0, 0."""
    from andi_amd import synth
    base = synth.base_codes(20_000, 7)
    refs = [synth.to_bytes(synth.mutate_codes(base, d, 11 + i)) for i, d in enumerate((0.01, 0.03, 0.1, 0.3))]
    refs += [synth.unrelated(20_000, 200 + i) for i in range(3)]
    query = synth.to_bytes(synth.mutate_codes(base, 0.005, 99))
    return refs, [query]


@pytest.fixture(scope="module")
def family():
    refs, queries = _family()
    R, Q = _model(refs, 15, 16), _model(queries, 15, 16)
    return refs, queries, R, Q, sm.shared_matrix(Q, R)


def test_screen_end_to_end(family):
    import andi_amd
    refs, queries, R, Q, M = family
    # a statement about the input: the model's order is strict over the related references and zero on the unrelated ones
    row = M[0].tolist()
    print("query sketch:", len(Q[0]), "shared:", row)
    assert row[0] > row[1] > row[2] > row[3] > 0 and row[4:] == [0, 0, 0]
    shared, rs, qs = andi_amd.screen(refs, queries, k=15, scale=16)
    assert np.array_equal(shared, M) and rs.tolist() == [len(x) for x in R] and qs.tolist() == [len(x) for x in Q]
    kept, taken = andi_amd.screen_select(shared, 3)
    assert kept.tolist() == [True, True, True, False, False, False, False] and taken.tolist() == [3]
    want_kept, want_taken = sm.select(M, 3)
    assert np.array_equal(kept, want_kept) and np.array_equal(taken, want_taken)


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), 70):
            f.write(seq[i:i + 70].decode() + "\n")
    return str(path)


def test_cli_screen(tmp_path, ctx, family):
    from andi_amd import lib
    refs, queries, R, Q, M = family
    from andi_amd import synth
    queries = queries + [synth.to_bytes(synth.mutate_codes(synth.base_codes(20_000, 7), 0.02, 55))]
    Q = Q + _model(queries[1:], 15, 16)
    M = sm.shared_matrix(Q, R)
    rnames, qnames = ["ref%d" % i for i in range(len(refs))], ["new_a", "new_b"]
    rfile = str(tmp_path / "refs.fa")
    with open(rfile, "w") as f:
        for n, s in zip(rnames, refs):
            f.write(open(_fasta(tmp_path / "one.fa", n, s)).read())
    qfiles = [_fasta(tmp_path / ("q%d.fa" % i), qnames[i], s) for i, s in enumerate(queries)]
    env = dict(os.environ, ANDI_HIP_GPUS="1")
    sk = ["--screen-kmer=15", "--screen-scale=16"]

    def run(args, ok=True):
        p = subprocess.run([CLI, "-t", "4"] + args, capture_output=True, timeout=300, env=env)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout, p.stderr.decode()

    # --screen=2: as a plain --reference run on the file of the two references the model selects
    kept, taken = sm.select(M, 2)
    assert kept.tolist() == [True, True] + [False] * 5 and taken.tolist() == [2, 2]
    two = str(tmp_path / "two.fa")
    with open(two, "w") as f:
        for n, s, k in zip(rnames, refs, kept):
            if k:
                f.write(open(_fasta(tmp_path / "one.fa", n, s)).read())
    for extra in ([], ["-v"], ["-m", "kimura", "--truncate-names"]):
        plain, plain_err = run(extra + ["--reference=" + two] + qfiles)
        report = str(tmp_path / "report.tsv")
        got, got_err = run(extra + ["--reference=" + rfile, "--screen=2", "--screen-report=" + report] + sk + qfiles)
        assert got == plain
        if "-v" in extra:
            assert got_err == "andi-hip: The screen kept 2 of 7 references.\n" + plain_err
        else:
            assert got_err == plain_err
        assert open(report).read() == sm.report(M, qnames, rnames, [len(x) for x in Q], [len(x) for x in R], kept)
    # a floor no reference reaches for the second query: a soft warning that names it, the table of the other's choice
    floor = int(M[1].max()) + 1
    assert M[0].max() >= floor
    got, got_err = run(["--reference=" + rfile, "--screen=1", "--screen-min=%d" % floor] + sk + qfiles, ok=False)
    assert "The screen kept no reference for 'new_b'" in got_err and got.startswith(b"2 1\n")
    # a screen that keeps nothing: an error, no table
    got, got_err = run(["--reference=" + rfile, "--screen=3", "--screen-min=100000"] + sk + qfiles, ok=False)
    assert got == b"" and "The screen kept no reference" in got_err

    # with a backbone (a tree needs a distance for every pair: references that are all related): every reference stays a
    # leaf, the references that were not kept are columns without a distance
    seqs, _ = synth.tree_set(8, 20_000, seed=91)
    refs, queries = seqs[:6], seqs[6:]
    rnames = rnames[:6]
    rfiles = [_fasta(tmp_path / ("r%d.fa" % i), rnames[i], s) for i, s in enumerate(refs)]
    qfiles = [_fasta(tmp_path / ("p%d.fa" % i), qnames[i], s) for i, s in enumerate(queries)]
    ref_args = ["--reference=" + f for f in rfiles]
    tree, out = str(tmp_path / "backbone.nwk"), str(tmp_path / "out.jplace")
    run(["--tree=" + tree] + rfiles)
    kept2, _ = sm.select(sm.shared_matrix(_model(queries, 15, 16), _model(refs, 15, 16)), 2)
    cols = np.nonzero(kept2)[0]
    assert 2 <= len(cols) < len(refs)
    got, _ = run(ref_args + ["--screen=2", "--backbone=" + tree, "--place=" + out] + sk + qfiles)
    MRQ, MQR = lib.dist_rect([refs[c] for c in cols], queries, model=lib.M_JC, host_threads=4)
    D = np.full((len(queries), len(refs)), np.nan)
    D[:, cols] = lib.distances_rect(MRQ, MQR, lib.M_JC)
    J = lib.parse_newick(open(tree).read(), rnames)
    Pl = lib.place(ctx, J, D, "fm")
    text = open(out).read()
    doc = json.loads(text)
    assert text == lib.jplace(J, rnames, Pl, qnames, "fm")
    assert [p["n"] for p in doc["placements"]] == [[qnames[q]] for q in range(len(queries)) if Pl["edge"][q] >= 0]
    assert got == run(["--reference=" + rfiles[c] for c in cols] + qfiles)[0] and got.startswith(b"2 %d\n" % len(cols))
