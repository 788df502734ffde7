"""The majority-rule consensus tree without a GPU: the three entry points' declarations, andi_hip_consensus and
andi_hip_format_newick_consensus against tests/consensus_model.py (driven with the model's ids, freq and sets), the
argument checks of andi_hip_nj_splits, and the command line's refusals of --consensus."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_model as cm
import nj_model
import support_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_nj_splits", "andi_hip_consensus", "andi_hip_format_newick_consensus")


def test_both_libraries_export_the_consensus_entry_points():
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
    assert lib.CONS_NODE.itemsize == 16 and lib.CONS_NODE == cm.CONS_NODE
    import andi_amd
    assert andi_amd.nj_splits is lib.nj_splits and andi_amd.consensus is lib.consensus
    assert andi_amd.newick_consensus is lib.newick_consensus
    knobs_h = open(os.path.join(ROOT, "andi_amd", "csrc", "knobs.h")).read()
    shipped, hooks = knobs_h.split("#define ANDI_KNOB_LIST_HOOKS(X)")
    assert "X(SPLIT_HASH_BITS)" in hooks.split("#define ANDI_KNOB_LIST(X)")[0] and "SPLIT_HASH_BITS" not in shipped


def _names(n):
    return ["t%d" % i for i in range(n)]


def _both(reps, skip=None, names=None, n=None):
    """the library's nodes and text from the model's splits; both must be the model's, byte for byte"""
    from andi_amd import lib
    reps = np.stack(reps)
    if n is None:
        n = reps.shape[1] + 2
    ids, freq, sets = cm.splits(reps, skip) if n > 3 else (np.zeros((len(reps), 0), np.uint32), np.zeros(0, np.uint32),
                                                           np.zeros((0, 1), np.uint64))
    nodes = lib.consensus(reps, ids, freq, sets, skip, n=n)
    want = cm.consensus(reps, ids, freq, sets, skip, n=n)
    assert nodes.dtype == cm.CONS_NODE and nodes.tobytes() == want.tobytes()
    names = names or _names(n)
    text = lib.newick_consensus(nodes, names)
    assert text == cm.newick_consensus(want, names)
    assert text.endswith(";\n") and text.count("\n") == 1
    return nodes, text, (ids, freq, sets)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 12])
@pytest.mark.parametrize("count", [1, 4])
def test_copies_of_one_tree_give_that_tree(n, count):
    J = nj_model.nj(np.random.default_rng(n).uniform(0.1, 1.0, (n, n)))
    nodes, text, _ = _both([J] * count, n=n)
    assert len(nodes) == n + max(n - 3, 0) + 1 and tuple(nodes[-1]) == (-1, count, 0.0)
    labels, unlabelled, lengths = support_model.parse_labels(text)
    names = _names(n)
    assert unlabelled == [] and len(labels) == max(n - 3, 0) and set(labels.values()) <= {count}
    assert sorted(support_model.canonical(k, names) for k in labels) == sorted(support_model.leaf_sets(J, n))
    # the mean of count equal lengths: the tree's own branch lengths, leaf by leaf
    _, _, own = support_model.parse_labels(nj_model.newick(J, names))
    for i, name in enumerate(names):
        assert lengths[frozenset([name])] == pytest.approx(own[frozenset([name])], rel=1e-7)
    assert text.startswith("(t0:")  # leaf 0 comes first at the root


def test_a_split_in_exactly_half_of_the_replicates_stays_out():
    A = cm.records([(0, 1), (3, 4)], (2, 5, 6))
    B = cm.records([(0, 2), (3, 4)], (1, 5, 6))
    nodes, text, (ids, freq, sets) = _both([A, A, B, B])
    assert freq.tolist() == [2, 4, 2]  # {2,3,4} (the side of (0,1) without leaf 0), {3,4}, {1,3,4}
    assert len(nodes) == 5 + 1 + 1 and nodes[5]["support"] == 4
    labels, _, _ = support_model.parse_labels(text)
    assert labels == {frozenset(["t3", "t4"]): 4}
    nodes, text, _ = _both([A, A, A, B, B])  # three of five: in
    assert support_model.parse_labels(text)[0] == {frozenset(["t3", "t4"]): 5, frozenset(["t2", "t3", "t4"]): 3}


def test_of_two_conflicting_resolutions_only_the_majority_one_enters():
    rng = np.random.default_rng(3)
    A = [cm.records([(1, 2), (3, 4), (6, 7)], (0, 5, 8), rng) for _ in range(3)]  # ((1,2),(3,4)) and 5
    B = [cm.records([(1, 2), (3, 4), (7, 5)], (0, 6, 8), rng) for _ in range(4)]  # (1,2) and ((3,4),5)
    nodes, text, (ids, freq, sets) = _both([A[0], B[0], A[1], B[1], B[2], A[2], B[3]])
    assert freq.tolist() == [7, 7, 3, 4]
    labels, _, lengths = support_model.parse_labels(text)
    assert labels == {frozenset(["t1", "t2"]): 7, frozenset(["t3", "t4"]): 7, frozenset(["t3", "t4", "t5"]): 4}
    # the mean over the four replicates that have the branch, summed in their order (the branch above node n + 2 = 8 is
    # the final record's third)
    want = np.float64(0.0)
    for J in B:
        want = want + J["lc"][3]
    assert lengths[frozenset(["t3", "t4", "t5"])] == float("%.8g" % (want / np.float64(4)))


def test_a_star_where_no_split_reaches_a_majority():
    reps = [cm.records([(0, 1)], (2, 3, 4)), cm.records([(0, 2)], (1, 3, 4)), cm.records([(0, 3)], (1, 2, 4))]
    nodes, text, (ids, freq, sets) = _both(reps)
    assert freq.tolist() == [1, 1, 1] and len(nodes) == 5 and (nodes["parent"][:4] == 4).all()
    assert text == "(t0:0.1,t1:0.1,t2:0.1,t3:0.1);\n"


def test_skipped_replicates_do_not_count():
    rng = np.random.default_rng(5)
    n = 9
    T = [cm.random_tree(n, 1, rng), cm.random_tree(n, 2, rng)]
    garbage = T[0].copy()
    garbage["a"] = 99999
    reps = [T[0], garbage, T[1], cm.other_final(T[0], n), T[0]]
    skip = [0, 1, 0, 0, 0]
    nodes, text, (ids, freq, sets) = _both(reps, skip)
    assert (ids[1] == cm.NONE).all() and nodes[-1]["support"] == 4
    kept, _, _ = _both([reps[k] for k in (0, 2, 3, 4)])
    assert nodes.tobytes() == kept.tobytes()


def test_names_that_need_quoting_and_truncation():
    from andi_amd import lib
    names = ["plain", "with blank", "it's", "a:b", "x,y", "(p)", "[q]", "semi;colon", "tab\there", "averyverylongname",
             "long name's quoted"]
    n = len(names)
    rng = np.random.default_rng(8)
    reps = np.stack([cm.random_tree(n, 4, rng), cm.random_tree(n, 4, rng), cm.random_tree(n, 5, rng)])
    ids, freq, sets = cm.splits(reps)
    nodes = lib.consensus(reps, ids, freq, sets)
    for trunc in (False, True):
        text = lib.newick_consensus(nodes, names, truncate_names=trunc)
        assert text == cm.newick_consensus(nodes, names, truncate_names=trunc), trunc
    assert "'it''s':" in lib.newick_consensus(nodes, names) and "averyveryl:" in lib.newick_consensus(nodes, names, True)


def test_noisy_replicates_nodes_and_text_equal_the_model():
    n, count = 14, 9
    D, _, _ = nj_model.additive_tree(n, seed=2)
    rng = np.random.default_rng(3)
    reps = []
    for _ in range(count):
        E = np.triu(rng.uniform(-0.3, 0.3, (n, n)), 1)
        reps.append(nj_model.nj(D * (1.0 + E + E.T)))
    nodes, text, (ids, freq, sets) = _both(reps)
    m = len(nodes) - n - 1
    assert 0 < m < len(freq)  # some splits are lost to the noise, not all
    labels, _, _ = support_model.parse_labels(text)
    assert all(2 * v > count for v in labels.values()) and len(labels) == m


def test_return_value_and_every_cap():
    from andi_amd import lib
    n = 7
    rng = np.random.default_rng(1)
    reps = np.stack([cm.random_tree(n, 3, rng)] * 2)
    ids, freq, sets = cm.splits(reps)
    nodes = lib.consensus(reps, ids, freq, sets)
    names = _names(n)
    full = cm.newick_consensus(nodes, names).encode()
    L = lib.load()
    for cap in range(0, len(full) + 2):
        buf = C.create_string_buffer(b"\x7f" * (cap + 4))
        need = L.andi_hip_format_newick_consensus(nodes.ctypes.data, n, len(nodes) - n - 1, lib._names(names), 0,
                                                  C.cast(buf, C.c_void_p) if cap else None, cap)
        assert need == len(full), cap
        if cap:
            k = min(len(full), cap - 1)
            assert buf.raw[:k] == full[:k] and buf.raw[k] == 0, cap
            assert buf.raw[cap:cap + 4] == b"\x7f" * 4  # nothing beyond cap


def test_a_65535_leaf_caterpillar_through_the_formatter():
    from andi_amd import lib
    n = 65535
    m = n - 3
    nodes = np.zeros(n + m + 1, cm.CONS_NODE)
    root = n + m
    nodes["parent"][0] = nodes["parent"][1] = nodes["parent"][n] = root  # the root: leaf 0, leaf 1, the first inner node
    nodes["parent"][2:n - 2] = n + np.arange(m - 1)                     # inner node j: leaf j + 2 and inner node j + 1
    nodes["parent"][n + 1:root] = n + np.arange(m - 1)
    nodes["parent"][n - 2] = nodes["parent"][n - 1] = root - 1            # the last one: the last two leaves
    nodes["parent"][root] = -1
    nodes["support"][:n], nodes["support"][n:root], nodes["support"][root] = 100, 51 + np.arange(m) % 50, 100
    nodes["length"][:root] = 0.125
    names = _names(n)
    text = lib.newick_consensus(nodes, names)
    assert text.startswith("(t0:0.125,t1:0.125,(t2:0.125,(t3:0.125,(t4:0.125,")
    assert text.endswith("t65533:0.125,t65534:0.125)%d:0.125)%d:0.125" % (51 + (m - 1) % 50, 51 + (m - 2) % 50)
                         + "".join(")%d:0.125" % (51 + j % 50) for j in range(m - 3, -1, -1)) + ");\n")
    assert text == cm.newick_consensus(nodes, names)


# ------------------------------------------------------------------ malformed input, rule by rule
def _good_nodes():
    # ((t1,t2)3,(t3,t4)2) under a root with t0: leaves 0..4, inner 5 = {1,2}, 6 = {3,4}, 7 = {1,2,3,4}, root 8
    nodes = np.zeros(9, cm.CONS_NODE)
    nodes["parent"] = [8, 5, 5, 6, 6, 7, 7, 8, -1]
    nodes["support"] = [3, 3, 3, 3, 3, 3, 2, 3, 3]
    nodes["length"] = 0.5
    return nodes


def test_the_formatter_refuses_malformed_nodes():
    from andi_amd import lib
    names = _names(5)
    assert lib.newick_consensus(_good_nodes(), names) == \
        "(t0:0.5,((t1:0.5,t2:0.5)3:0.5,(t3:0.5,t4:0.5)2:0.5)3:0.5);\n"
    bad = {}
    bad["a parent that is a leaf"] = (1, 0)
    bad["a parent out of range"] = (1, 9)
    bad["a negative parent"] = (2, -1)
    bad["a root with a parent"] = (8, 7)
    bad["a cycle"] = (7, 5)             # 5 -> 7 -> 5, away from the root
    bad["an inner node that is its own parent"] = (6, 6)
    bad["an inner node with one child"] = (4, 5)
    bad["an inner node without a child"] = (5, 8)  # (then 7 has one child)
    for what, (node, parent) in bad.items():
        nodes = _good_nodes()
        nodes["parent"][node] = parent
        L = lib.load()
        buf = C.create_string_buffer(b"\x7f" * 64)
        need = L.andi_hip_format_newick_consensus(nodes.ctypes.data, 5, 3, lib._names(names), 0, C.cast(buf, C.c_void_p), 64)
        assert need == 0 and buf.raw[0] == 0, what
        assert lib.newick_consensus(nodes, names) == "", what
    assert lib.newick_consensus(_good_nodes()[:5], names) == ""  # (no root)
    # a cycle that leaves every node its two children: t0 and t1 under the root, (t2,t3) and (t4,t5) each other's parent
    nodes = np.zeros(9, cm.CONS_NODE)
    nodes["parent"] = [8, 8, 6, 6, 7, 7, 7, 6, -1]
    assert lib.newick_consensus(nodes, _names(6)) == ""
    nodes["parent"][7] = 8
    assert lib.newick_consensus(nodes, _names(6)) == "(t0:0,t1:0,((t2:0,t3:0)0:0,t4:0,t5:0)0:0);\n"


def _consensus_rc(reps, n, ids, freq, sets, skip=None):
    from andi_amd import lib
    reps = np.ascontiguousarray(reps, lib.NJ_JOIN)
    ids, freq, sets = (np.ascontiguousarray(x, t) for x, t in ((ids, np.uint32), (freq, np.uint32), (sets, np.uint64)))
    nodes = np.zeros(max(2 * n - 2, 3), lib.CONS_NODE)
    m = C.c_size_t(0)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    return lib.load().andi_hip_consensus(reps.ctypes.data, n, len(reps), skip.ctypes.data if skip is not None else None,
                                         ids.ctypes.data, len(freq), freq.ctypes.data, sets.ctypes.data, nodes.ctypes.data,
                                         C.byref(m))


def test_consensus_refuses_inconsistent_arguments():
    from andi_amd import lib
    n = 6
    reps = np.stack([cm.random_tree(n, 1), cm.random_tree(n, 1), cm.random_tree(n, 2)])
    ids, freq, sets = cm.splits(reps)
    assert _consensus_rc(reps, n, ids, freq, sets) == 0
    assert _consensus_rc(reps, n, ids, freq, sets, skip=[1, 1, 1]) == 1  # nothing used
    late = ids.copy()
    late[0, 1] = len(freq)  # an id past the splits
    assert _consensus_rc(reps, n, late, freq, sets) == 1
    none = ids.copy()
    none[1, 0] = cm.NONE  # a used replicate without an id ...
    assert _consensus_rc(reps, n, none, freq, sets) == 1
    assert _consensus_rc(reps, n, none, freq, sets, skip=[0, 1, 0]) == 1  # (... and skipped, the frequencies are off)
    more = freq.copy()
    more[0] += 1  # a frequency the ids do not bear out
    assert _consensus_rc(reps, n, ids, more, sets) == 1
    twice = reps.copy()
    twice["b"][0][1] = twice["b"][0][0]  # a node that is a child twice
    assert _consensus_rc(twice, n, ids, freq, sets) == 1
    far = reps.copy()
    far["a"][2][0] = 2 * n  # a child that is no node
    assert _consensus_rc(far, n, ids, freq, sets) == 1
    for word in (0b000111, 0b1000110, 0b000100, 0b111110):  # leaf 0 in the set, a leaf past n, a single leaf, all but leaf 0
        wrong = sets.copy()
        wrong[0, 0] = word
        assert _consensus_rc(reps, n, ids, freq, wrong) == 1, bin(word)
    # majority sets that are not laminar: {1,2} and {2,3}, each in both of two replicates
    A = cm.records([(1, 2), (3, 4)], (0, 5, 6))
    two = np.stack([A, A])
    ids2, freq2, sets2 = cm.splits(two)
    assert sets2[:, 0].tolist() == [0b00110, 0b11000] and _consensus_rc(two, 5, ids2, freq2, sets2) == 0
    sets2[1, 0] = 0b01100
    assert _consensus_rc(two, 5, ids2, freq2, sets2) == 1
    with pytest.raises(lib.AndiHipError):
        lib.consensus(two, ids2, freq2, sets2)
    # NULL pointers, n and count out of range
    L = lib.load()
    r, i, f, s = two.ctypes.data, ids2.ctypes.data, freq2.ctypes.data, sets2.ctypes.data
    nodes = np.zeros(8, lib.CONS_NODE)
    m = C.c_size_t(0)
    nd, mp = nodes.ctypes.data, C.byref(m)
    for args in [(None, 5, 2, None, i, 2, f, s, nd, mp), (r, 5, 2, None, None, 2, f, s, nd, mp),
                 (r, 5, 2, None, i, 2, None, s, nd, mp), (r, 5, 2, None, i, 2, f, None, nd, mp),
                 (r, 5, 2, None, i, 2, f, s, None, mp), (r, 5, 2, None, i, 2, f, s, nd, None),
                 (r, 5, 0, None, i, 2, f, s, nd, mp), (r, 1, 2, None, i, 2, f, s, nd, mp),
                 (r, 65536, 2, None, i, 2, f, s, nd, mp), (r, 5, 2, None, i, 0, f, s, nd, mp)]:
        assert L.andi_hip_consensus(*args) == 1, args


def test_splits_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    J = np.zeros((2, 2), lib.NJ_JOIN)
    ids = np.zeros(2, np.uint32)
    nsplits, pf, ps = C.c_size_t(7), C.c_void_p(), C.c_void_p()
    j, i, ns, f, s = J.ctypes.data, ids.ctypes.data, C.byref(nsplits), C.byref(pf), C.byref(ps)
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, j, 4, 2, None, i, ns, f, s), (None, None, 4, 2, None, i, ns, f, s), (None, j, 4, 2, None, None, ns, f, s),
                 (None, j, 4, 2, None, i, None, f, s), (None, j, 4, 2, None, i, ns, None, s), (None, j, 4, 2, None, i, ns, f, None),
                 (None, j, 4, 0, None, i, ns, f, s), (None, j, 1, 2, None, i, ns, f, s), (None, j, 0, 2, None, i, ns, f, s),
                 (None, j, 65536, 2, None, i, ns, f, s), (None, j, 3, 2, None, i, ns, f, s)]:
        assert L.andi_hip_nj_splits(*args) == 1, args
    assert not pf.value and not ps.value


def _run(args, stdin=b""):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _fa(path, name, seq=b"ACGTACGTACGTTTGA"):
    path.write_text(">%s\n%s\n" % (name, seq.decode()))
    return str(path)


def test_cli_refuses_consensus_without_bootstrap_and_with_a_reference(tmp_path):
    rc, out, err = _run(["--help"])
    assert rc == 0 and "--consensus=FILE" in out and "--support=FILE" in out
    a, b = _fa(tmp_path / "a.fa", "A"), _fa(tmp_path / "b.fa", "B")
    con = tmp_path / "c.nwk"
    # these refusals come before any sequence is read, any file is made and any device call
    rc, out, err = _run(["--consensus=" + str(con), a, b])
    assert rc == 1 and out == "" and "--consensus" in err and "-b" in err and not con.exists()
    rc, out, err = _run(["-b", "1", "--consensus=" + str(con), a, b])  # (one matrix: no replicate)
    assert rc == 1 and out == "" and "--consensus" in err and not con.exists()
    for ref in ("--reference=" + a, "--reference-list=" + str(tmp_path / "list")):
        rc, out, err = _run(["--consensus=" + str(con), ref, b])
        assert rc == 1 and out == "" and "--consensus" in err and "--reference" in err and not con.exists()
    assert "Comparing" not in err
