"""The query-versus-reference mode without a GPU: its C-ABI surface, argument checks that fail before any HIP call, the
table formatter (andi_hip_format_distances_rect) against a restatement in Python and against the square formatter's cells,
and the command line's --reference options."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_dist_rect", "andi_hip_queries_view", "andi_hip_format_distances_rect")


def test_both_libraries_export_the_rect_entry_points():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        L = C.CDLL(os.path.join(ROOT, "andi_amd", so))
        for name in NEW:
            assert getattr(L, name) is not None, (so, name)
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
    assert lib.load().andi_hip_abi_version() == 5


def _rect_raw(MRQ, MQR, refs, nr, queries, nq):
    from andi_amd import lib
    err = C.create_string_buffer(512)
    o = lib.Opts()
    lib.load().andi_hip_default_opts(C.byref(o))
    rc = lib.load().andi_hip_dist_rect(MRQ, MQR, refs, nr, queries, nq, C.byref(o), err, len(err))
    return rc, err.value.decode()


def test_bad_arguments_fail_through_errbuf_before_any_device_call():
    from andi_amd import lib
    good = lib._seq_array([b"ACGTACGTAC", b"ACGTACGTAA"])
    m = (lib.Model * 4)()
    p = C.cast(m, C.c_void_p)
    for args in [(None, p, good, 1, good, 1), (p, None, good, 1, good, 1), (p, p, None, 1, good, 1),
                 (p, p, good, 1, None, 1), (p, p, good, 0, good, 1), (p, p, good, 1, good, 0)]:
        rc, msg = _rect_raw(*args)
        assert rc == 1 and msg == "andi_hip_dist_rect: bad arguments", (args, msg)
    empty = lib._seq_array([b"ACGT", b""])
    rc, msg = _rect_raw(p, p, good, 2, empty, 2)
    assert rc == 1 and msg == "query 1 is empty"
    rc, msg = _rect_raw(p, p, empty, 2, good, 2)
    assert rc == 1 and msg == "reference 1 is empty"
    huge = lib._seq_array([b"ACGT"])
    huge[0].len = (2 ** 31 - 2) // 2 + 1  # (never read: the length alone is refused)
    rc, msg = _rect_raw(p, p, good, 1, huge, 1)
    assert rc == 1 and msg.startswith("query 0 is too long. The technical limit is")
    with pytest.raises(lib.AndiHipError, match="query 0 is empty"):
        lib.dist_rect([b"ACGTACGT"], [b""])
    with pytest.raises(lib.AndiHipError, match="bad arguments"):
        lib.dist_rect([], [b"ACGTACGT"])


# ---------------------------------------------------------------- the formatter
def _models(rng, shape, kind="close"):
    """random models: 'close' (diagonal heavy, d of a few per cent), 'tiny' (d < 0.001), 'nan' (no matching counts:
    JC fails), 'thin' (coverage < 0.2)"""
    M = np.zeros(shape + (17,), np.uint32)
    diag = [0, 5, 10, 15]
    M[..., diag] = rng.integers(20000, 40000, shape + (4,))
    off = [k for k in range(16) if k not in diag]
    if kind == "close":
        M[..., off] = rng.integers(30, 400, shape + (12,))
    elif kind == "tiny":
        M[..., off] = 0
        M[..., 1] = rng.integers(1, 5, shape)
    elif kind == "nan":
        M[..., diag] = 0
        M[..., off] = rng.integers(100, 200, shape + (12,))
    M[..., 16] = M[..., :16].sum(-1)
    if kind == "thin":
        M[..., off] = rng.integers(30, 400, shape + (12,))
        M[..., 16] = M[..., :16].sum(-1) * 7
    return M


def _restated(MRQ, MQR, rnames, qnames, model, extra_verbose, truncate, warnings=True):
    """the format of include/andi_hip.h: andi_hip_format_distances_rect, restated"""
    from andi_amd import lib
    nr, nq = len(rnames), len(qnames)

    def avg(a, b):
        return (a.astype(np.uint64) + b).astype(np.uint32)

    D = np.zeros((nq, nr))
    warn = []
    for q in range(nq):
        for r in range(nr):
            qr, rq = MQR[q, r], MRQ[r, q]
            d = D[q, r] = lib.estimate(qr if extra_verbose else avg(qr, rq), model)
            if not warnings:
                continue
            if np.isnan(d):
                warn.append("For the two sequences '%s' and '%s' the distance computation failed and is reported as "
                            "nan. Please refer to the documentation for further details." % (qnames[q], rnames[r]))
            up = lib.estimate(rq if extra_verbose else avg(qr, rq), model)
            if not np.isnan(up):
                c1, c2 = lib.coverage(rq), lib.coverage(qr)
                if c1 < 0.2 or c2 < 0.2:
                    warn.append("For the two sequences '%s' and '%s' very little homology was found (%f and %f, "
                                "respectively)." % (rnames[r], qnames[q], c1, c2))
    sci = bool(((D > 0) & (D < 0.001)).any())

    def f(x):  # (printf writes a NaN's sign: glibc's "-nan")
        if np.isnan(x):
            return " -nan" if np.signbit(x) else " nan"
        return (" %1.4e" if sci else " %1.4f") % x
    out = "%d %d\n" % (nq, nr) + " " * 10 + "".join(" " + (n[:10] if truncate else n) for n in rnames) + "\n"
    for q in range(nq):
        out += ("%-10.10s" if truncate else "%-10s") % qnames[q] + "".join(f(x) for x in D[q]) + "\n"
    return out, warn, sci


@pytest.mark.parametrize("kind,model,extra_verbose,truncate", [
    ("close", 1, False, False),   # plain
    ("tiny", 1, False, False),    # scientific
    ("close", 2, False, True),    # truncated names (Kimura)
    ("nan", 1, False, False),     # NaN warnings
    ("thin", 3, False, False),    # low-coverage warnings (LogDet)
    ("close", 4, True, False),    # extra_verbose: MQR alone (ANI)
    ("thin", 1, True, True),
])
def test_rect_formatter_matches_its_restatement(kind, model, extra_verbose, truncate):
    from andi_amd import lib
    rng = np.random.default_rng(zlib.crc32(repr((kind, model, extra_verbose, truncate)).encode()))
    nr, nq = 5, 3
    MRQ, MQR = _models(rng, (nr, nq)), _models(rng, (nq, nr))
    # one pair of the chosen kind in each direction, the rest ordinary ("thin": all of them)
    if kind == "thin":
        MRQ, MQR = _models(rng, (nr, nq), "thin"), _models(rng, (nq, nr), "thin")
    elif kind != "close":
        MRQ[2, 1] = _models(rng, (1,), kind)[0]
        MQR[1, 2] = _models(rng, (1,), kind)[0]
    rnames = ["ref_%d_long_name" % k if truncate else "r%d" % k for k in range(nr)]
    qnames = ["query_%d_long_name" % k if truncate else "q%d" % k for k in range(nq)]
    text, warn, flags = lib.format_distances_rect(MRQ, MQR, rnames, qnames, model, extra_verbose, truncate)
    want, want_warn, sci = _restated(MRQ, MQR, rnames, qnames, model, extra_verbose, truncate)
    assert text == want
    assert warn.splitlines() == want_warn
    assert sci == (kind == "tiny")
    assert flags == (1 if any("nan" in w for w in want_warn) else 0) | (2 if any("homology" in w for w in want_warn) else 0)
    if kind == "nan":
        assert flags & 1
    if kind == "thin":
        assert flags & 2
    text2, warn2, flags2 = lib.format_distances_rect(MRQ, MQR, rnames, qnames, model, extra_verbose, truncate, warnings=False)
    assert text2 == text and warn2 == "" and flags2 == 0


@pytest.mark.parametrize("sci", [False, True])
@pytest.mark.parametrize("extra_verbose", [False, True])
def test_rect_cells_are_the_square_formatters_cells(sci, extra_verbose):
    """On a random matrix of refs ++ queries, every cell of the rectangular table is the string the square formatter
    prints for that pair (the %f / %e switch forced alike: a tiny distance in a cross block, or none anywhere)."""
    from andi_amd import lib
    rng = np.random.default_rng(11 + sci + 2 * extra_verbose)
    nr, nq = 6, 4
    n = nr + nq
    M = _models(rng, (n, n))
    if sci:
        M[1, nr + 2] = M[nr + 2, 1] = _models(rng, (1,), "tiny")[0]
    MRQ, MQR = M[:nr, nr:].copy(), M[nr:, :nr].copy()
    names = ["s%d" % k for k in range(n)]
    square, _, _ = lib.format_distances(M, names, 1, extra_verbose)
    rect, _, _ = lib.format_distances_rect(MRQ, MQR, names[:nr], names[nr:], 1, extra_verbose)
    srows = [line.split() for line in square.splitlines()[1:]]
    rlines = rect.splitlines()
    assert rlines[0] == "%d %d" % (nq, nr) and rlines[1].split() == names[:nr]
    rrows = [line.split() for line in rlines[2:]]
    assert len(rrows) == nq
    for q in range(nq):
        assert rrows[q][0] == names[nr + q]
        assert rrows[q][1:] == srows[nr + q][1:nr + 1], q
    assert ("e-" in rect) == sci


# ---------------------------------------------------------------- the command line
def _run(args, stdin=b""):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _fa(path, name, seq=b"ACGTACGTACGTTTGA"):
    path.write_text(">%s\n%s\n" % (name, seq.decode()))
    return str(path)


def test_cli_reference_options_without_a_gpu(tmp_path):
    rc, out, err = _run(["--help"])
    assert rc == 0 and out.startswith("Usage: andi-hip [OPTIONS...] FILES...")
    assert "--reference=FILE" in out and "--reference-list=FILE" in out
    a, b = _fa(tmp_path / "a.fa", "A"), _fa(tmp_path / "b.fa", "B")
    rc, out, err = _run(["-b", "3", "--reference=" + a, b])
    assert rc == 1 and out == "" and "Bootstrapping (-b) is not available together with --reference" in err
    rc, out, err = _run(["--reference-list=" + str(tmp_path / "missing.txt"), b])
    assert rc == 1 and out == ""
    assert "missing.txt: No such file or directory" in err and "No reference sequences given" in err
    lst = tmp_path / "refs.txt"
    lst.write_text(a + "\n")
    rc, out, err = _run(["--reference-list=" + str(lst), str(tmp_path / "nothere.fa")])
    assert rc == 1 and "nothere.fa" in err and "No query sequences given" in err
