"""Transfer bootstrap support without a GPU: the two entry points' declarations, the two statements of the contract in
tests/transfer_model.py against each other, the labelled Newick formatter (andi_hip_format_newick_transfer) against the
model, the argument checks of andi_hip_nj_transfer, and the command line's refusals of --transfer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nj_model
import transfer_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_nj_transfer", "andi_hip_format_newick_transfer")


def test_both_libraries_export_the_transfer_entry_points():
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
    assert andi_amd.nj_transfer is lib.nj_transfer and andi_amd.newick_transfer is lib.newick_transfer


def _sym(rng, n):
    A = rng.uniform(0.1, 1.0, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _noisy(D, rng, size):
    E = np.triu(rng.uniform(-size, size, D.shape), 1)
    return D * (1.0 + E + E.T)


def test_the_two_statements_of_the_model_agree():
    # the tree itself, a lightly and a heavily perturbed matrix: all three regimes of the transfer index
    exact = capped = between = 0
    for n in range(4, 141):
        rng = np.random.default_rng(n)
        D = _sym(rng, n)
        tree = nj_model.nj(D)
        reps = [tree, nj_model.nj(_noisy(D, rng, 0.02)), nj_model.nj(_noisy(D, rng, 0.5))]
        depth, total, per = transfer_model.transfer(tree, reps)
        d2, t2, p2 = transfer_model.transfer_numpy(tree, reps)
        assert d2.dtype == np.uint32 and t2.dtype == np.uint64 and p2.dtype == np.uint32
        assert depth == d2.tolist() and total == t2.tolist() and per == p2.tolist(), n
        assert min(depth) >= 2 and per[0] == [0] * (n - 3)
        for row in per[1:]:
            for s, v in enumerate(row):
                exact += v == 0
                capped += v == depth[s] - 1 and v > 0
                between += 0 < v < depth[s] - 1
    assert exact > 0 and capped > 0 and between > 0, (exact, capped, between)
    # a skipped replicate
    depth, total, per = transfer_model.transfer(tree, reps, skip=[0, 1, 0])
    d2, t2, p2 = transfer_model.transfer_numpy(tree, reps, skip=[0, 1, 0])
    assert per[1] == [transfer_model.SKIPPED] * (n - 3) and per == p2.tolist() and total == t2.tolist()
    assert t2.tolist() == transfer_model.transfer(tree, [reps[0], reps[2]])[1]


def _caterpillar(n, order=None):
    """join order[0] and order[1], then that node with order[2], ...: the deepest tree of n leaves"""
    order = list(range(n)) if order is None else order
    J = np.zeros(n - 2, nj_model.NJ_JOIN)
    J["la"], J["lb"] = 0.5, 0.25
    J[0] = (order[0], order[1], -1, 0, 0.5, 0.25, 0.0)
    for s in range(1, n - 3):
        J[s] = (n + s - 1, order[s + 1], -1, 0, 0.5, 0.25, 0.0)
    J[n - 3] = (order[n - 2], order[n - 1], n + n - 4, 0, 0.125, 0.125, 0.125)
    return J


def test_model_hand_case_pins_the_cap():
    # the caterpillar 0 ... 7 against the caterpillar 0, 2, 3, 4, 5, 6, 7, 1: branch {0, 1} is 2 away from {0, 2} (and
    # from every other branch), but a leaf branch of the replicate is 1 away
    tree, rep = _caterpillar(8), _caterpillar(8, [0, 2, 3, 4, 5, 6, 7, 1])
    depth, total, per = transfer_model.transfer(tree, [rep])
    assert depth == [2, 3, 4, 3, 2] and per == [[1, 1, 1, 1, 1]] and total == [1, 1, 1, 1, 1]
    a = transfer_model.leaf_sets(tree, 8)[0]
    assert min(min(bin(a ^ b).count("1"), 8 - bin(a ^ b).count("1")) for b in transfer_model.leaf_sets(rep, 8)) == 2
    assert [x.tolist() for x in transfer_model.transfer_numpy(tree, [rep])] == [depth, total, per]


def _tree(n, seed):
    return nj_model.nj(np.random.default_rng(seed).uniform(0.1, 1.0, (n, n)))


def _values(J, n, seed, used):
    """depth as the tree has it, and sums that give the labels 0 and 1 and one that needs six digits"""
    sets = transfer_model.leaf_sets(J, n)
    depth = np.array([min(bin(a).count("1"), n - bin(a).count("1")) for a in sets], np.uint32)
    rng = np.random.default_rng(seed)
    total = np.array([int(rng.integers(0, used * (int(d) - 1) + 1)) for d in depth], np.uint64)
    if len(total) > 0:
        total[0] = 0  # label 1
    if len(total) > 1:
        total[-1] = used * (int(depth[-1]) - 1)  # label 0
    if len(total) > 2:
        total[1] = 1  # 1 - 1 / (used * (depth - 1)): six digits with used = 777
    return depth, total


@pytest.mark.parametrize("n", [2, 3, 4, 5, 40])
def test_transfer_newick_matches_the_model(n):
    from andi_amd import lib
    used = 777
    J = _tree(n, n)
    depth, total = _values(J, n, n, used)
    names = ["taxon_%d" % i for i in range(n)]
    text = lib.newick_transfer(J, depth, total, used, names)
    assert text == transfer_model.newick_transfer(J, depth, total, used, names) and text.endswith(";\n")
    labels, unlabelled = transfer_model.parse_labels(text)
    assert len(labels) == max(n - 3, 0) and unlabelled == []  # every pair record's node, and not the final record
    assert all(0.0 <= v <= 1.0 for v in labels.values())
    if n >= 5:
        assert ")1:" in text and ")0:" in text
    if n == 40:
        want = "%.6g" % (1.0 - 1.0 / (777.0 * float(int(depth[1]) - 1)))
        assert len(want) == 8 and ")" + want + ":" in text  # 0.99xxxx
    # the text without the labels is andi_hip_format_newick's
    assert transfer_model.strip_labels(text) == lib.newick(J, names) == nj_model.newick(J, names)


def test_transfer_newick_quotes_and_truncates_names():
    from andi_amd import lib
    names = ["plain", "with blank", "it's", "a:b", "x,y", "(p)", "[q]", "semi;colon", "tab\there", "averyverylongname",
             "long name's quoted"]
    n = len(names)
    J = _tree(n, 1)
    depth, total = _values(J, n, 1, 9)
    for trunc in (False, True):
        text = lib.newick_transfer(J, depth, total, 9, names, truncate_names=trunc)
        assert text == transfer_model.newick_transfer(J, depth, total, 9, names, truncate_names=trunc), trunc
        assert text != lib.newick(J, names, truncate_names=trunc)
    assert "'it''s'" in lib.newick_transfer(J, depth, total, 9, names)
    assert "averyveryl:" in lib.newick_transfer(J, depth, total, 9, names, True)


def test_transfer_newick_return_value_and_every_cap():
    from andi_amd import lib
    n = 7
    J = _tree(n, 3)
    depth, total = _values(J, n, 3, 100)
    names = ["n%d" % i for i in range(n)]
    full = transfer_model.newick_transfer(J, depth, total, 100, names).encode()
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    L = lib.load()
    for cap in range(0, len(full) + 2):
        buf = C.create_string_buffer(b"\x7f" * (cap + 4))
        need = L.andi_hip_format_newick_transfer(Jc.ctypes.data, depth.ctypes.data, total.ctypes.data, 100, n,
                                                 lib._names(names), 0, C.cast(buf, C.c_void_p) if cap else None, cap)
        assert need == len(full), cap
        if cap:
            k = min(len(full), cap - 1)
            assert buf.raw[:k] == full[:k] and buf.raw[k] == 0, cap
            assert buf.raw[cap:cap + 4] == b"\x7f" * 4  # nothing beyond cap


def test_transfer_newick_refusals():
    from andi_amd import lib
    n = 6
    J = _tree(n, 4)
    depth, total = _values(J, n, 4, 10)
    names = list("abcdef")
    L = lib.load()
    Jc = np.ascontiguousarray(J, dtype=lib.NJ_JOIN)
    cn = lib._names(names)

    def call(d, t, used, joins=Jc):
        buf = C.create_string_buffer(b"\x7f" * 256)
        need = L.andi_hip_format_newick_transfer(joins.ctypes.data, d, t, used, n, cn, 0, C.cast(buf, C.c_void_p), 256)
        return need, buf.raw[0]

    assert call(depth.ctypes.data, total.ctypes.data, 10)[0] > 0
    assert call(depth.ctypes.data, total.ctypes.data, 0) == (0, 0)  # no replicate was summed
    assert call(None, total.ctypes.data, 10) == (0, 0) and call(depth.ctypes.data, None, 10) == (0, 0)
    shallow = depth.copy()
    shallow[1] = 1  # a leaf's branch: no transfer index is defined
    assert call(shallow.ctypes.data, total.ctypes.data, 10) == (0, 0)
    assert lib.newick_transfer(J, shallow, total, 10, names) == "" and lib.newick_transfer(J, depth, total, 0, names) == ""
    bad = Jc.copy()
    bad["a"][0] = n + 1  # a node no earlier record made
    assert call(depth.ctypes.data, total.ctypes.data, 10, bad) == (0, 0)


def test_transfer_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    J = np.zeros((2, 2), lib.NJ_JOIN)
    depth, total, per = np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(2, np.uint32)
    j, d, t, p = J.ctypes.data, depth.ctypes.data, total.ctypes.data, per.ctypes.data
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, j, j, 4, 2, None, d, t, p), (None, None, j, 4, 2, None, d, t, p), (None, j, None, 4, 2, None, d, t, p),
                 (None, j, j, 4, 2, None, None, t, p), (None, j, j, 4, 2, None, d, None, p), (None, j, j, 4, 2, None, d, t, None),
                 (None, j, j, 4, 0, None, d, t, p), (None, j, j, 1, 2, None, d, t, p), (None, j, j, 0, 2, None, d, t, p),
                 (None, j, j, 65536, 2, None, d, t, p), (None, j, j, 3, 2, None, d, t, p)]:
        assert L.andi_hip_nj_transfer(*args) == 1, args
    assert depth[0] == 0 and total[0] == 0 and not per.any()


def _run(args, stdin=b""):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _fa(path, name, seq=b"ACGTACGTACGTTTGA"):
    path.write_text(">%s\n%s\n" % (name, seq.decode()))
    return str(path)


def test_cli_refuses_transfer_without_bootstrap_and_with_a_reference(tmp_path):
    rc, out, err = _run(["--help"])
    assert rc == 0 and "--transfer=FILE" in out
    a, b = _fa(tmp_path / "a.fa", "A"), _fa(tmp_path / "b.fa", "B")
    tr = tmp_path / "t.nwk"
    # these refusals come before any sequence is read, any file is made and any device call
    rc, out, err = _run(["--transfer=" + str(tr), a, b])
    assert rc == 1 and out == "" and "--transfer" in err and "-b" in err and not tr.exists()
    rc, out, err = _run(["-b", "1", "--transfer=" + str(tr), a, b])  # (one matrix: no replicate)
    assert rc == 1 and out == "" and "--transfer" in err and not tr.exists()
    for ref in ("--reference=" + a, "--reference-list=" + str(tmp_path / "list")):
        rc, out, err = _run(["--transfer=" + str(tr), ref, b])
        assert rc == 1 and out == "" and "--transfer" in err and "--reference" in err and not tr.exists()
    assert "Comparing" not in err
