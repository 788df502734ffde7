"""Bootstrap support without a GPU: the three entry points' declarations, the labelled Newick formatter
(andi_hip_format_newick_support) against tests/support_model.py, the argument checks of andi_hip_nj_batch and
andi_hip_nj_support, and the command line's refusals of --support."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nj_model
import support_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_nj_batch", "andi_hip_nj_support", "andi_hip_format_newick_support")


def test_both_libraries_export_the_support_entry_points():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        L = C.CDLL(os.path.join(ROOT, "andi_amd", so))
        for name in NEW:
            assert getattr(L, name) is not None, (so, name)
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
    assert lib.load().andi_hip_abi_version() == 5
    assert "#define ANDI_HIP_ABI_VERSION 5\n" in header
    import andi_amd
    assert andi_amd.nj_batch is lib.nj_batch and andi_amd.nj_support is lib.nj_support


def _tree(n, seed):
    return nj_model.nj(np.random.default_rng(seed).uniform(0.1, 1.0, (n, n)))


def _counts(n, seed):
    sup = np.random.default_rng(seed).integers(0, 101, max(n - 3, 0)).astype(np.uint32)
    if len(sup) > 1:
        sup[0], sup[-1] = 0, 4294967295  # (the ends of the range)
    return sup


@pytest.mark.parametrize("n", [2, 3, 4, 5, 40])
def test_labelled_newick_matches_the_model(n):
    from andi_amd import lib
    J, sup = _tree(n, n), _counts(n, n)
    names = ["taxon_%d" % i for i in range(n)]
    text = lib.newick(J, names, support=sup)
    assert text == support_model.newick_support(J, sup, names)
    labels, unlabelled, lengths = support_model.parse_labels(text)
    sets = support_model.leaf_sets(J, n)
    assert len(labels) == max(n - 3, 0) and unlabelled == []  # every pair record's node, and not the final record
    assert sorted((support_model.canonical(k, names), v) for k, v in labels.items()) == sorted(zip(sets, map(int, sup)))
    # the text without the labels is andi_hip_format_newick's
    assert re.sub(r"\)\d+", ")", text) == lib.newick(J, names) == nj_model.newick(J, names)
    # no support: the same bytes as andi_hip_format_newick
    L = lib.load()
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    plain, none = C.create_string_buffer(4096), C.create_string_buffer(4096)
    a = L.andi_hip_format_newick(Jc.ctypes.data, n, lib._names(names), 0, C.cast(plain, C.c_void_p), 4096)
    b = L.andi_hip_format_newick_support(Jc.ctypes.data, None, n, lib._names(names), 0, C.cast(none, C.c_void_p), 4096)
    assert a == b and plain.raw == none.raw


def test_labelled_newick_quotes_and_truncates_names():
    from andi_amd import lib
    names = ["plain", "with blank", "it's", "a:b", "x,y", "(p)", "[q]", "semi;colon", "tab\there", "averyverylongname",
             "long name's quoted"]
    n = len(names)
    J, sup = _tree(n, 1), _counts(n, 1)
    for trunc in (False, True):
        text = lib.newick(J, names, truncate_names=trunc, support=sup)
        assert text == support_model.newick_support(J, sup, names, truncate_names=trunc), trunc
        assert text != lib.newick(J, names, truncate_names=trunc)
    assert "'it''s'" in lib.newick(J, names, support=sup) and "averyveryl:" in lib.newick(J, names, True, support=sup)


def test_labelled_newick_return_value_and_every_cap():
    from andi_amd import lib
    n = 7
    J, sup = _tree(n, 3), _counts(n, 3)
    names = ["n%d" % i for i in range(n)]
    full = support_model.newick_support(J, sup, names).encode()
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    L = lib.load()
    for cap in range(0, len(full) + 2):
        buf = C.create_string_buffer(b"\x7f" * (cap + 4))
        need = L.andi_hip_format_newick_support(Jc.ctypes.data, sup.ctypes.data, n, lib._names(names), 0,
                                                C.cast(buf, C.c_void_p) if cap else None, cap)
        assert need == len(full), cap
        if cap:
            k = min(len(full), cap - 1)
            assert buf.raw[:k] == full[:k] and buf.raw[k] == 0, cap
            assert buf.raw[cap:cap + 4] == b"\x7f" * 4  # nothing beyond cap


def _caterpillar(n):
    """join leaf 0 and 1, then that node with leaf 2, ...: the deepest tree of n leaves"""
    J = np.zeros(n - 2, nj_model.NJ_JOIN)
    J["a"][0], J["b"][0] = 0, 1
    J["a"][1:n - 3] = n + np.arange(n - 4)
    J["b"][1:n - 3] = np.arange(2, n - 2)
    J["la"], J["lb"] = 0.5, 0.25
    J[n - 3] = (n - 2, n - 1, n + n - 4, 0, 0.125, 0.125, 0.125)
    return J


def test_labelled_newick_of_a_65535_leaf_caterpillar():
    from andi_amd import lib
    n = 65535
    J = _caterpillar(n)
    sup = (np.arange(n - 3) % 101).astype(np.uint32)
    names = ["t%d" % i for i in range(n)]
    text = lib.newick(J, names, support=sup)
    assert text.startswith("(t65533:0.125,t65534:0.125," + "(" * (n - 3) + "t0:0.5,t1:0.25)0:0.5,t2:0.25)1:0.5,t3:0.25)2")
    assert text.endswith(",t65532:0.25)%d:0.125);\n" % ((n - 4) % 101))
    assert text == support_model.newick_support(J, sup, names)


def test_labelled_newick_refuses_records_that_are_no_tree():
    from andi_amd import lib
    J = _tree(5, 4)
    J["a"][0] = 5 + 1  # a node no earlier record made
    L = lib.load()
    sup = np.array([1, 2], np.uint32)
    buf = C.create_string_buffer(b"\x7f" * 64)
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    need = L.andi_hip_format_newick_support(Jc.ctypes.data, sup.ctypes.data, 5, lib._names(list("abcde")), 0,
                                            C.cast(buf, C.c_void_p), 64)
    assert need == 0 and buf.raw[0] == 0
    assert lib.newick(J, list("abcde"), support=sup) == ""


def test_model_counts_unordered_bipartitions():
    # ((0,1),2,(3,4)) joined in two orders, with two final records: the same two branches
    A = np.zeros(3, nj_model.NJ_JOIN)
    A["a"], A["b"], A["c"] = [0, 3, 2], [1, 4, 5], [-1, -1, 6]
    B = np.zeros(3, nj_model.NJ_JOIN)
    B["a"], B["b"], B["c"] = [0, 2, 3], [1, 5, 4], [-1, -1, 6]
    assert sorted(support_model.leaf_sets(A, 5)) == sorted(support_model.leaf_sets(B, 5)) == [0b11000, 0b11100]
    assert support_model.support(A, [B]) == [1, 1] and support_model.support(B, [A, A], skip=[0, 1]) == [1, 1]


def test_batch_and_support_reject_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((2, 4, 4))
    J = np.zeros((2, 2), lib.NJ_JOIN)
    bad = np.zeros(2, np.int64)
    sup = np.zeros(1, np.uint32)
    d, j, b, s = D.ctypes.data, J.ctypes.data, bad.ctypes.data, sup.ctypes.data
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, d, 4, 2, j, b), (None, None, 4, 2, j, b), (None, d, 4, 2, None, b), (None, d, 4, 2, j, None),
                 (None, d, 4, 0, j, b), (None, d, 1, 2, j, b), (None, d, 0, 2, j, b), (None, d, 65536, 2, j, b)]:
        assert L.andi_hip_nj_batch(*args) == 1, args
    for args in [(None, j, j, 4, 2, None, s), (None, None, j, 4, 2, None, s), (None, j, None, 4, 2, None, s),
                 (None, j, j, 4, 2, None, None), (None, j, j, 4, 0, None, s), (None, j, j, 1, 2, None, s),
                 (None, j, j, 0, 2, None, s), (None, j, j, 65536, 2, None, s), (None, j, j, 3, 2, None, s)]:
        assert L.andi_hip_nj_support(*args) == 1, args


def _run(args, stdin=b""):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _fa(path, name, seq=b"ACGTACGTACGTTTGA"):
    path.write_text(">%s\n%s\n" % (name, seq.decode()))
    return str(path)


def test_cli_refuses_support_without_bootstrap_and_with_a_reference(tmp_path):
    rc, out, err = _run(["--help"])
    assert rc == 0 and "--support=FILE" in out
    a, b = _fa(tmp_path / "a.fa", "A"), _fa(tmp_path / "b.fa", "B")
    sup = tmp_path / "s.nwk"
    # these refusals come before any sequence is read, any file is made and any device call
    rc, out, err = _run(["--support=" + str(sup), a, b])
    assert rc == 1 and out == "" and "--support" in err and "-b" in err and not sup.exists()
    rc, out, err = _run(["-b", "1", "--support=" + str(sup), a, b])  # (one matrix: no replicate)
    assert rc == 1 and out == "" and "--support" in err and not sup.exists()
    for ref in ("--reference=" + a, "--reference-list=" + str(tmp_path / "list")):
        rc, out, err = _run(["--support=" + str(sup), ref, b])
        assert rc == 1 and out == "" and "--support" in err and "--reference" in err and not sup.exists()
    assert "Comparing" not in err
