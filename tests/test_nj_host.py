"""Neighbor-joining trees without a GPU: the distances as doubles (andi_hip_distances) against the PHYLIP formatter's
cells, the Newick formatter (andi_hip_format_newick) against tests/nj_model.py, andi_hip_nj's argument checks, the
command line's --tree option, and tests/nj_model.py itself against a second, scalar restatement of the contract."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nj_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_distances", "andi_hip_nj", "andi_hip_format_newick")


def _matrix(rng, n, low=2000):
    M = np.zeros((n, n, 17), np.uint32)
    for i in range(n):
        for j in range(n):
            if i == j:
                M[i, j, 0] = M[i, j, 16] = 9
                continue
            total = int(rng.integers(low, 3_000_000))
            p = rng.dirichlet(np.r_[np.full(4, 40.0), np.full(12, 0.6)])
            c = rng.multinomial(total, p)
            M[i, j, [0, 5, 10, 15]] = c[:4]
            M[i, j, [1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]] = c[4:]
            M[i, j, 16] = total + int(rng.integers(0, 1000))
    return M


def test_both_libraries_export_the_tree_entry_points():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        L = C.CDLL(os.path.join(ROOT, "andi_amd", so))
        for name in NEW:
            assert getattr(L, name) is not None, (so, name)
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
    assert lib.load().andi_hip_abi_version() == 5


@pytest.mark.parametrize("model", range(5))
def test_distances_are_the_printed_cells(model):
    from andi_amd import lib
    rng = np.random.default_rng(100 + model)
    n = 9
    M = _matrix(rng, n)
    M[2, 5, :] = 0  # a pair without anchors: nan from both directions' sum ...
    M[5, 2, :] = 0
    M[5, 2, 16] = M[2, 5, 16] = 1000
    D = lib.distances(M, model)
    text, _, _ = lib.format_distances(M, ["s%d" % i for i in range(n)], model, warnings=False)
    rows = text.splitlines()[1:]
    sci = "e" in rows[0].split()[1]
    for i in range(n):
        cells = rows[i].split()[1:]
        for j in range(n):
            if np.isnan(D[i, j]):  # (C prints a NaN with its sign bit as -nan)
                assert cells[j] in ("nan", "-nan"), (model, i, j)
            else:
                assert (("%1.4e" if sci else "%1.4f") % D[i, j]) == cells[j], (model, i, j)
    assert np.isnan(D[2, 5]) and np.isnan(D[5, 2])  # ... where the matrix says nan
    assert (D.view(np.uint64) == D.T.view(np.uint64)).all()
    assert (np.diag(D).view(np.uint64) == 0).all()  # +0.0, not -0.0


def test_distances_of_a_larger_matrix_match_the_estimate_per_pair():
    from andi_amd import lib
    rng = np.random.default_rng(7)
    n = 150  # (several formatter threads)
    M = _matrix(rng, n)
    D = lib.distances(M, lib.M_KIMURA)
    for i, j in [(0, 1), (3, 149), (77, 12), (148, 149)]:
        avg = M[i, j].astype(np.uint64) + M[j, i]
        assert D[i, j] == lib.estimate(avg.astype(np.uint32), lib.M_KIMURA)
    assert (D.view(np.uint64) == D.T.view(np.uint64)).all()


@pytest.mark.parametrize("n", [2, 3, 4, 50])
def test_newick_matches_the_model(n):
    from andi_amd import lib
    rng = np.random.default_rng(n)
    D = rng.uniform(0.0, 1.0, (n, n))
    J = nj_model.nj(D)
    names = ["taxon_%d" % i for i in range(n)]
    text = lib.newick(J, names)
    assert text == nj_model.newick(J, names)
    leaves, splits, _ = nj_model.parse_newick(text)
    assert sorted(leaves) == sorted(names) and text.endswith(";\n")
    assert text.count("(") == text.count(")") == max(n - 2, 1)


def test_newick_quotes_and_truncates_names():
    from andi_amd import lib
    names = ["plain", "with blank", "it's", "a:b", "x,y", "(p)", "[q]", "semi;colon", "tab\there", "averyverylongname",
             "long name's quoted"]
    n = len(names)
    J = nj_model.nj(np.random.default_rng(1).uniform(0.1, 1.0, (n, n)))
    for trunc in (False, True):
        text = lib.newick(J, names, truncate_names=trunc)
        assert text == nj_model.newick(J, names, truncate_names=trunc), trunc
        leaves, _, _ = nj_model.parse_newick(text)
        want = [s[:10] for s in names] if trunc else names
        assert sorted(leaves) == sorted(want)
    text = lib.newick(J, names)
    assert "'with blank'" in text and "'it''s'" in text and "plain:" in text and "'tab\there'" in text
    assert "averyveryl:" in lib.newick(J, names, truncate_names=True)


def test_newick_return_value_and_a_small_cap():
    from andi_amd import lib
    n = 12
    J = nj_model.nj(np.random.default_rng(3).uniform(0.1, 1.0, (n, n)))
    names = ["n%d" % i for i in range(n)]
    full = nj_model.newick(J, names).encode()
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    L = lib.load()
    for cap in (0, 1, 7, len(full), len(full) + 1):
        buf = C.create_string_buffer(b"\x7f" * (cap + 4))
        need = L.andi_hip_format_newick(Jc.ctypes.data, n, lib._names(names), 0, C.cast(buf, C.c_void_p) if cap else None,
                                        cap)
        assert need == len(full), cap
        if cap:
            k = min(len(full), cap - 1)
            assert buf.raw[:k] == full[:k] and buf.raw[k] == 0, cap
            assert buf.raw[cap:cap + 4] == b"\x7f" * 4  # nothing beyond cap


def test_newick_of_a_65535_leaf_caterpillar():
    from andi_amd import lib
    n = 65535
    J = np.zeros(n - 2, lib.NJ_JOIN)
    # join leaf 0 and 1, then that node with leaf 2, ... : the deepest possible tree
    J["a"][0], J["b"][0] = 0, 1
    J["a"][1:n - 3] = n + np.arange(n - 4)
    J["b"][1:n - 3] = np.arange(2, n - 2)
    J["la"], J["lb"] = 0.5, 0.25
    J[n - 3] = (n - 2, n - 1, n + n - 4, 0, 0.125, 0.125, 0.125)
    names = ["t%d" % i for i in range(n)]
    text = lib.newick(J, names)
    assert text.startswith("(t65533:0.125,t65534:0.125," + "(" * (n - 3) + "t0:0.5,t1:0.25):0.5,t2:0.25):0.5,t3:0.25)")
    assert text.endswith(",t65532:0.25):0.125);\n")
    assert text == nj_model.newick(J, names)
    assert text.count("(") == n - 2


def test_newick_refuses_records_that_are_no_tree():
    from andi_amd import lib
    J = nj_model.nj(np.random.default_rng(4).uniform(0.1, 1.0, (5, 5)))
    J["a"][0] = 5 + 1  # a node no earlier record made
    assert lib.newick(J, ["a", "b", "c", "d", "e"]) == ""


def test_nj_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((4, 4))
    J = np.zeros(4, lib.NJ_JOIN)
    assert L.andi_hip_nj(None, D.ctypes.data, 4, J.ctypes.data) == 1
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, None, 4, J.ctypes.data), (None, D.ctypes.data, 4, None), (None, D.ctypes.data, 1, J.ctypes.data),
                 (None, D.ctypes.data, 0, J.ctypes.data), (None, D.ctypes.data, 65536, J.ctypes.data)]:
        assert L.andi_hip_nj(*args) == 1, args


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n%s\n" % (name, seq))
    return str(path)


def test_cli_lists_the_tree_option():
    p = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and "--tree=FILE" in p.stdout.decode()


def test_cli_refuses_a_tree_of_the_reference_table(tmp_path):
    a = _fasta(tmp_path / "a.fa", "a", "ACGT" * 400)
    b = _fasta(tmp_path / "b.fa", "b", "ACGA" * 400)
    for ref in ("--reference=" + a, "--reference-list=" + str(tmp_path / "list")):
        p = subprocess.run([CLI, "--tree=" + str(tmp_path / "t.nwk"), ref, b], capture_output=True, timeout=60)
        assert p.returncode == 1 and "--tree" in p.stderr.decode() and p.stdout == b""
    # -b with --reference keeps its own message
    p = subprocess.run([CLI, "-b", "2", "--reference=" + a, b], capture_output=True, timeout=60)
    assert p.returncode == 1
    assert "Bootstrapping (-b) is not available together with --reference" in p.stderr.decode()


_WITH_REFERENCE = " not available together with --reference or --reference-list."
_NEEDS_B = " bootstrap matrices: give -b N with N of at least 2."
_REFUSALS = [  # (options beside the two FASTA files, with a reference?, the line on stderr behind "andi-hip: ")
    (["-b", "2"], True, "Bootstrapping (-b) is" + _WITH_REFERENCE),
    (["--tree=T"], True, "A tree (--tree) is" + _WITH_REFERENCE),
    (["--support=S"], True, "Support values (--support) are" + _WITH_REFERENCE),
    (["--support=S"], False, "Support values (--support) need" + _NEEDS_B),
    (["--consensus=C"], True, "A consensus tree (--consensus) is" + _WITH_REFERENCE),
    (["--consensus=C"], False, "A consensus tree (--consensus) needs" + _NEEDS_B),
    (["--transfer=X"], True, "Transfer support (--transfer) is" + _WITH_REFERENCE),
    (["--transfer=X"], False, "Transfer support (--transfer) needs" + _NEEDS_B),
    (["--trees-only", "--tree=T"], False,
     "Trees without matrices (--trees-only) need bootstrap replicates: give -b N with N of at least 2."),
    (["--trees-only", "-b", "2"], False, "Trees without matrices (--trees-only) need somewhere to go: give at least one of "
                                         "--tree, --support, --consensus, --transfer."),
    # more than one violation: the first of the order above is the one reported
    (["--support=S", "--consensus=C"], True, "Support values (--support) are" + _WITH_REFERENCE),
    (["--consensus=C", "--support=S"], False, "Support values (--support) need" + _NEEDS_B),
    (["-b", "2", "--transfer=X", "--tree=T"], True, "Bootstrapping (-b) is" + _WITH_REFERENCE),
    (["--transfer=X", "--tree=T"], True, "A tree (--tree) is" + _WITH_REFERENCE),
    (["--trees-only", "--transfer=X"], False, "Transfer support (--transfer) needs" + _NEEDS_B),
]


@pytest.mark.parametrize("options,reference,line", _REFUSALS)
def test_cli_refuses_with_these_words_and_in_this_order(tmp_path, options, reference, line):
    a = _fasta(tmp_path / "a.fa", "a", "ACGT" * 400)
    b = _fasta(tmp_path / "b.fa", "b", "ACGA" * 400)
    args = [o[:o.index("=") + 1] + str(tmp_path / o[o.index("=") + 1:]) if "=" in o else o for o in options]
    args += ["--reference=" + a, b] if reference else [a, b]
    p = subprocess.run([CLI] + args, capture_output=True, timeout=60)
    # the whole line and the exit status; nothing printed, no file made (the refusals come before any file is opened)
    assert (p.returncode, p.stdout, p.stderr.decode()) == (1, b"", "andi-hip: " + line + "\n")
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.fa"]


def test_cli_fails_on_an_unwritable_tree_file(tmp_path):
    a = _fasta(tmp_path / "a.fa", "a", "ACGT" * 400)
    b = _fasta(tmp_path / "b.fa", "b", "ACGA" * 400)
    bad = str(tmp_path / "no" / "such" / "dir" / "t.nwk")
    p = subprocess.run([CLI, "--tree=" + bad, a, b], capture_output=True, timeout=60)
    err = p.stderr.decode()
    assert p.returncode == 1 and bad in err and p.stdout == b""
    assert "Comparing" not in err and "sequence" not in err  # (reported before any sequence is read)


# ------------------------------------------------- a second restatement of andi_hip_nj's contract, one operation at a time
def _nj_scalar(D):
    """include/andi_hip.h's neighbor-joining contract with Python floats (IEEE doubles, each operation rounded) and plain
    loops, written from the header's text alone: the records as tuples (a, b, c, la, lb, lc)."""
    n = len(D)
    M = [[0.0] * n for _ in range(n)]  # by slot; only D[i][j], i < j, is read; the diagonal is +0.0
    for i in range(n):
        for j in range(i + 1, n):
            M[i][j] = M[j][i] = float(D[i][j])
    if n == 2:
        return [(0, 1, -1, M[0][1] * 0.5, M[0][1] * 0.5, 0.0)]
    node = list(range(n))  # node[slot]: the id in that slot
    active = list(range(n))  # ascending slots
    out = []
    for s in range(n - 3):
        r = len(active)
        R = {}
        for x in active:
            acc = 0.0
            for k in active:
                acc = acc + M[x][k]
            R[x] = acc
        best = None  # (NaN?, Q, id(x), id(y), slot x, slot y)
        for i in range(r):
            for j in range(i + 1, r):
                x, y = active[i], active[j]
                if node[x] > node[y]:
                    x, y = y, x
                q = (float(r - 2) * M[x][y] - R[x]) - R[y]
                nan = q != q
                key = (nan, 0.0 if nan else q, node[x], node[y])  # (-0.0 == +0.0 in the comparison)
                if best is None or key < best[:4]:
                    best = key + (x, y)
        a, b = best[4], best[5]
        d = M[a][b]
        la = d * 0.5 + (R[a] - R[b]) / float(2 * (r - 2))
        out.append((node[a], node[b], -1, la, d - la, 0.0))
        u, o = min(a, b), max(a, b)
        for k in active:
            if k != a and k != b:
                M[u][k] = M[k][u] = ((M[a][k] + M[b][k]) - d) * 0.5
        M[u][u] = 0.0
        node[u] = n + s
        active.remove(o)
    x, y, z = sorted(active, key=lambda k: node[k])
    xy, xz, yz = M[x][y], M[x][z], M[y][z]
    out.append((node[x], node[y], node[z], ((xy + xz) - yz) * 0.5, ((xy + yz) - xz) * 0.5, ((xz + yz) - xy) * 0.5))
    return out


def _same_records(got, want):
    """ids exactly; lengths by their bits, except that a NaN only has to be a NaN (its bits are the platform's)"""
    for f in ("a", "b", "c"):
        assert (got[f] == want[f]).all(), f
    assert (got["pad"] == 0).all()
    for f in ("la", "lb", "lc"):
        g, w = got[f], want[f]
        assert (np.isnan(g) == np.isnan(w)).all(), f
        ok = ~np.isnan(w)
        assert (g[ok].view(np.uint64) == w[ok].view(np.uint64)).all(), f


def _as_records(rows):
    J = np.zeros(len(rows), nj_model.NJ_JOIN)
    for s, (a, b, c, la, lb, lc) in enumerate(rows):
        J[s] = (a, b, c, 0, la, lb, lc)
    return J


def _cases(seed):
    """(name, D): random, small integers (many exact ties in Q), duplicated leaves at +0.0 and -0.0, a lower triangle and
    diagonal of garbage, and entries near the largest double, whose Q overflow to +-inf and NaN"""
    rng = np.random.default_rng(seed)
    for n in (2, 3, 4, 5, 6, 9, 17, 31, 40):
        A = rng.uniform(0.0, 1.0, (n, n))
        yield "random", np.triu(A, 1) + np.triu(A, 1).T
        yield "garbage below", np.triu(A, 1) + np.tril(rng.uniform(-5, 5, (n, n)))
        B = np.triu(rng.integers(0, 4, (n, n)).astype(float), 1)
        yield "small integers", B + B.T
        idx = np.sort(rng.integers(0, max(2, n // 2), n))
        base = rng.uniform(0.0, 1.0, (n, n))
        dup = (base + base.T)[np.ix_(idx, idx)]
        same = idx[:, None] == idx[None, :]
        dup[same] = np.where(rng.integers(0, 2, (n, n)) == 1, -0.0, 0.0)[same]
        yield "duplicated leaves", dup
        yield "near overflow", _overflowing(rng, n)


def _overflowing(rng, n):
    """finite entries, some of them near the largest double: row sums and (r-2) * D overflow to inf, inf - inf is NaN"""
    A = rng.uniform(0.0, 1.0, (n, n)) * 1e307
    A[rng.uniform(size=(n, n)) < 0.5] = rng.uniform(0.0, 1.0) * 10.0 ** rng.integers(0, 300)
    A[:, rng.integers(0, n)] = 1.7e308
    return np.triu(A, 1) + np.triu(A, 1).T


def test_the_model_is_the_scalar_restatement():
    overflowed = set()
    for seed in range(4):
        for name, D in _cases(seed):
            want = _as_records(_nj_scalar(D))
            _same_records(nj_model.nj(D), want)
            if name == "near overflow":
                overflowed |= {"nan" for v in want["la"] if np.isnan(v)} | {"inf" for v in want["la"] if np.isinf(v)}
    assert overflowed == {"nan", "inf"}  # (the overflow cases do reach both)


def test_nan_q_orders_after_every_number_then_by_id():
    # r = 5, Q = (3 D - R_x) - R_y.  Leaves 0 and 1 are 1.7e308 from everything, so every row sum is inf: a pair with 0
    # or 1 has Q = (inf - inf) - inf = NaN, a pair of 2, 3, 4 has Q = (3 D - inf) - inf = -inf.  NaN orders last.
    big = 1.7e308
    D = np.array([[0, big, big, big, big],
                  [0, 0, big, big, big],
                  [0, 0, 0, 1, 2],
                  [0, 0, 0, 0, 3],
                  [0, 0, 0, 0, 0]], float)
    J = nj_model.nj(D)
    _same_records(J, _as_records(_nj_scalar(D)))
    assert (J["a"][0], J["b"][0]) == (2, 3)
    # every Q NaN: the smallest pair of ids
    D = np.full((6, 6), big)
    J = nj_model.nj(D)
    _same_records(J, _as_records(_nj_scalar(D)))
    assert (J["a"][0], J["b"][0]) == (0, 1) and np.isnan(J["la"][0])


def test_a_prefix_of_the_model_is_the_whole_run_cut_short():
    rng = np.random.default_rng(12)
    for n in (2, 3, 4, 7, 60, 130):
        A = np.triu(rng.integers(0, 3, (n, n)).astype(float), 1)
        J = nj_model.nj(A + A.T)
        for k in sorted({0, 1, n // 3, max(n - 3, 0), n - 2, n}):
            P = nj_model.nj(A + A.T, steps=k)
            assert P.dtype == J.dtype and P.tobytes() == J[:k].tobytes(), (n, k)
