"""The k-mer sketch screen without a GPU: the NumPy restatement of the contract (tests/sketch_model.py) against a plain loop
over the windows; andi_hip_screen_select against the model; the argument checks that come before any HIP call; the
refusals of andi-hip's --screen options."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sketch_model as sm
from conftest import ROOT, rand_dna

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_sketch", "andi_hip_sketch_count", "andi_hip_sketch_sizes", "andi_hip_sketch_download", "andi_hip_sketch_free",
       "andi_hip_sketch_timings", "andi_hip_sketch_shared", "andi_hip_screen_select", "andi_hip_screen")
KS = (4, 5, 21, 31, 32)


def test_declared_exported_and_abi_stays_5():
    from andi_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    shipped = C.CDLL(os.path.join(ROOT, "andi_amd", "libandihip.so"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
        assert getattr(L, name) is not None and getattr(shipped, name) is not None
    assert L.andi_hip_abi_version() == 5  # additions only
    knobs_h = open(os.path.join(ROOT, "andi_amd", "csrc", "knobs.h")).read()
    shipped_list, hooks = knobs_h.split("#define ANDI_KNOB_LIST_HOOKS(X)")
    hooks = hooks.split("#define ANDI_KNOB_LIST(X)")[0]
    assert "X(SKETCH_BATCH)" in hooks and "X(SKETCH_LDS)" in hooks and "SKETCH" not in shipped_list
    assert len(re.findall(r"X\(\w+\)", shipped_list.split("#define ANDI_KNOB_LIST_SHIPPED(X)")[1])) == 7


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("k", KS)
def test_model_equals_the_loop_over_windows(k):
    rng = np.random.default_rng(k)
    for trial in range(40):
        n = int(rng.integers(0, 6 * k))
        s = rand_dna(rng, n, [b"ACGT", b"ACGT" * 6 + b"!", b"AC", b"A"][trial % 4])
        for scale in (1, 2, 7):
            got, want = sm.sketch(s, k, scale), sm.sketch_loop(s, k, scale)
            assert got.dtype == np.uint64 and np.array_equal(got, want)
            assert (np.diff(got.astype(object)) > 0).all()  # ascending, each once
    if k >= 21:  # (a short k meets the window of A only, whose hash is 0: kept at any scale)
        assert len(sm.sketch(rand_dna(rng, 300), k, sm.M64)) == 0


def test_model_facts():
    assert len(sm.sketch(b"AC" * 500, 21, 1)) == 2
    assert len(sm.sketch(b"ACGT!ACGTA", 4, 1)) == 2
    assert sm.fmix64(np.array([0, 1], np.uint64)).tolist() == [0, 0xb456bcfc34c2cb2c]  # MurmurHash3's finaliser
    assert sm.sketch(b"A" * 40, 32, sm.M64).tolist() == [0]  # the code of a run of A is 0, and fmix64(0) = 0: kept at any scale


@pytest.mark.parametrize("k", (4, 16, 21, 31, 32))
def test_a_sequence_and_its_reverse_complement_have_one_sketch(k):
    rng = np.random.default_rng(100 + k)
    for n in (k, k + 1, 500):
        s = rand_dna(rng, n)
        for scale in (1, 3):
            assert np.array_equal(sm.sketch(s, k, scale), sm.sketch(sm.revcomp(s), k, scale))
    s = rand_dna(rng, 400, b"ACGT" * 20 + b"!")
    assert np.array_equal(sm.sketch(s, k, 1), sm.sketch(sm.revcomp(s), k, 1))  # ('!' stays '!')


@pytest.mark.parametrize("k", (4, 16, 32))
def test_palindromic_windows(k):
    """a window that is its own reverse complement (even k only): f == r, one hash like any other"""
    rng = np.random.default_rng(k)
    half = rand_dna(rng, k // 2)
    pal = half + sm.revcomp(half)
    assert sm.revcomp(pal) == pal
    got = sm.sketch(pal, k, 1)
    assert len(got) == 1 and np.array_equal(got, sm.sketch_loop(pal, k, 1))
    both = pal + b"!" + pal
    assert np.array_equal(sm.sketch(both, k, 1), got)


@pytest.mark.parametrize("k", KS)
def test_a_separator_at_every_position(k):
    rng = np.random.default_rng(7 * k)
    s = rand_dna(rng, 2 * k)
    assert len(sm.sketch(s, k, 1)) == len(set(sm.sketch_loop(s, k, 1).tolist())) <= k + 1
    for at in range(2 * k):
        t = s[:at] + b"!" + s[at + 1:]
        got = sm.sketch(t, k, 1)
        assert np.array_equal(got, sm.sketch_loop(t, k, 1))
        windows = max(0, at - k + 1) + max(0, 2 * k - at - k)  # those that end before it plus those that start behind it
        assert len(got) <= windows and (windows > 0 or len(got) == 0)


@pytest.mark.parametrize("k", KS)
def test_lengths_around_k(k):
    rng = np.random.default_rng(3 * k)
    for n, windows in ((k - 1, 0), (k, 1), (k + 1, 2)):
        s = rand_dna(rng, n)
        got = sm.sketch(s, k, 1)
        assert np.array_equal(got, sm.sketch_loop(s, k, 1)) and (len(got) == windows or (windows == 2 and len(got) == 1))
    assert len(sm.sketch(b"", k, 1)) == 0


# ---------------------------------------------------------------- andi_hip_screen_select
def _select_cases():
    rng = np.random.default_rng(11)
    for trial in range(60):
        nq, nr = int(rng.integers(1, 7)), int(rng.integers(1, 40))
        yield rng.integers(0, 50, (nq, nr)).astype(np.uint32), int(rng.integers(1, nr + 3)), int(rng.integers(0, 30))
    ties = np.array([[5, 9, 5, 9, 5, 0, 9], [1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0]], np.uint32)
    for keep in (1, 2, 3, 4, 6, 7, 8, 100):
        for floor in (0, 1, 5, 6, 9, 10):
            yield ties, keep, floor
    big = np.array([[0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 3]], np.uint32)
    yield big, 2, 0
    yield big, 3, 0xFFFFFFFF
    yield np.zeros((4, 9), np.uint32), 3, 0


def test_screen_select_equals_the_model():
    from andi_amd import lib
    for sh, keep, floor in _select_cases():
        kept, taken = lib.screen_select(sh, keep, floor)
        want_kept, want_taken = sm.select(sh, keep, floor)
        assert kept.dtype == bool and np.array_equal(kept, want_kept), (sh, keep, floor)
        assert taken.dtype == np.uint32 and np.array_equal(taken, want_taken)
    # ties go to the smaller index; a floor above every count keeps nothing; an all-zero row takes nothing at floor 0 either
    sh = np.array([[5, 9, 5, 9, 5, 0, 9]], np.uint32)
    assert lib.screen_select(sh, 4)[0].tolist() == [True, True, False, True, False, False, True]
    assert not lib.screen_select(sh, 7, 10)[0].any() and lib.screen_select(sh, 100)[1].tolist() == [6]
    assert lib.screen_select(np.zeros((2, 3), np.uint32), 3, 0)[1].tolist() == [0, 0]
    # taken may be NULL
    kept = np.zeros(7, np.uint8)
    assert lib.load().andi_hip_screen_select(sh.ctypes.data, 1, 7, 2, 1, kept.ctypes.data, None) == 0 and kept.tolist() == [0, 1, 0, 1, 0, 0, 0]


def test_refusals_before_any_hip_call():
    from andi_amd import lib
    L = lib.load()
    sh, kept, taken = np.ones((2, 3), np.uint32), np.zeros(3, np.uint8), np.zeros(2, np.uint32)
    assert L.andi_hip_screen_select(None, 2, 3, 1, 1, kept.ctypes.data, taken.ctypes.data) == 1
    assert L.andi_hip_screen_select(sh.ctypes.data, 2, 3, 1, 1, None, taken.ctypes.data) == 1
    assert L.andi_hip_screen_select(sh.ctypes.data, 0, 3, 1, 1, kept.ctypes.data, None) == 1
    assert L.andi_hip_screen_select(sh.ctypes.data, 2, 0, 1, 1, kept.ctypes.data, None) == 1
    seqs = lib._seq_array([b"ACGTACGTACGTACGTACGTACGTACGT"])
    out = C.c_void_p()
    assert L.andi_hip_sketch(None, seqs, 1, 21, 1000, C.byref(out)) == 1 and not out.value
    assert L.andi_hip_sketch_count(None) == 0
    buf = np.zeros(4, np.uint64)
    assert L.andi_hip_sketch_sizes(None, None, buf.ctypes.data) == 1
    assert L.andi_hip_sketch_download(None, None, 0, buf.ctypes.data) == 1
    assert L.andi_hip_sketch_timings(None, buf.ctypes.data) == 1
    assert L.andi_hip_sketch_shared(None, None, None, buf.ctypes.data) == 1
    L.andi_hip_sketch_free(None, None)  # (nothing to free: no call)
    err = C.create_string_buffer(512)
    shared, sizes = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    for refs, nr, queries, nq, k, scale, dev, dst in ((None, 1, seqs, 1, 21, 1000, 0, shared), (seqs, 1, None, 1, 21, 1000, 0, shared),
                                                      (seqs, 0, seqs, 1, 21, 1000, 0, shared), (seqs, 1, seqs, 0, 21, 1000, 0, shared),
                                                      (seqs, 1, seqs, 1, 3, 1000, 0, shared), (seqs, 1, seqs, 1, 33, 1000, 0, shared),
                                                      (seqs, 1, seqs, 1, 21, 0, 0, shared), (seqs, 1, seqs, 1, 21, 1000, -1, shared),
                                                      (seqs, 1, seqs, 1, 21, 1000, 0, None)):
        err.value = b""
        rc = L.andi_hip_screen(refs, nr, queries, nq, k, scale, dev, dst.ctypes.data if dst is not None else None, sizes.ctypes.data,
                               sizes.ctypes.data, err, len(err))
        assert rc == 1 and err.value.startswith(b"andi_hip_screen: bad arguments")
    with pytest.raises(lib.AndiHipError, match="bad arguments"):
        lib.screen([b"ACGT"], [], k=21)


# ---------------------------------------------------------------- the command line
def test_cli_refusals_and_help(tmp_path):
    ref, q = str(tmp_path / "r.fa"), str(tmp_path / "q.fa")
    for path, name in ((ref, "r"), (q, "q")):
        with open(path, "w") as f:
            f.write(">%s\nACGTACGTAGCTAGCTAGCATCGATCGATCGATCAGCTAGCTAGCTAGC\n" % name)

    def run(args):
        p = subprocess.run([CLI] + args, capture_output=True, timeout=60, stdin=subprocess.DEVNULL)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    R = "--reference=" + ref
    for args, message in (
            (["--screen=2", ref, q], "A screen (--screen) needs references to choose from"),
            ([R, "--screen=0", q], "Expected a positive number of references to keep for --screen, but '0' was given."),
            ([R, "--screen=two", q], "Expected a positive number of references to keep for --screen, but 'two' was given."),
            ([R, "--screen=-1", q], "Expected a positive number of references to keep for --screen, but '-1' was given."),
            ([R, "--screen=2", "--screen-kmer=3", q], "Expected a k-mer length of 4 to 32 for --screen-kmer, but '3' was given."),
            ([R, "--screen=2", "--screen-kmer=33", q], "Expected a k-mer length of 4 to 32 for --screen-kmer, but '33' was given."),
            ([R, "--screen=2", "--screen-kmer=x", q], "Expected a k-mer length of 4 to 32 for --screen-kmer, but 'x' was given."),
            ([R, "--screen=2", "--screen-scale=0", q], "Expected a positive integer for --screen-scale, but '0' was given."),
            ([R, "--screen=2", "--screen-scale=1.5", q], "Expected a positive integer for --screen-scale, but '1.5' was given."),
            ([R, "--screen=2", "--screen-min=0", q], "Expected a positive integer for --screen-min, but '0' was given."),
            ([R, "--screen=2", "--screen-min=many", q], "Expected a positive integer for --screen-min, but 'many' was given."),
            ([R, "--screen-kmer=21", q], "need a screen: give --screen=K."),
            ([R, "--screen-scale=10", q], "need a screen: give --screen=K."),
            ([R, "--screen-min=2", q], "need a screen: give --screen=K."),
            ([R, "--screen-report=" + str(tmp_path / "rep.tsv"), q], "need a screen: give --screen=K."),
    ):
        rc, out, err = run(args)
        assert rc == 1 and out == "" and message in err, (args, err)
    assert not os.path.exists(tmp_path / "rep.tsv")  # (refused before any file is opened)
    rc, out, err = run(["--help"])
    assert rc == 0 and err == ""
    for option in ("--screen=K", "--screen-kmer=INT", "--screen-scale=INT", "--screen-min=INT", "--screen-report=FILE"):
        assert option in out
    assert out.count("sourmash's default") == 2


# ---------------------------------------------------------------- the host function under the sanitizers
def test_screen_select_stand_alone_under_the_sanitizers(tmp_path):
    """scripts/asan_screen_host.c: andi_hip_screen_select in a program of its own (its own main, no Python, no GPU)"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "asan_screen_host")
    subprocess.run([cc, "-std=gnu99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "asan_screen_host.c"),
                    os.path.join(ROOT, "andi_amd", "csrc", "host_screen.c"), "-o", exe], check=True, timeout=120)
    p = subprocess.run([exe], capture_output=True, timeout=120)
    assert p.returncode == 0 and b"clean" in p.stdout, p.stderr.decode()
