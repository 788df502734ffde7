"""BIONJ without a GPU: the new entry points' surface and argument checks, tests/bionj_model.py against a second, scalar
restatement written from Gascuel's paper (explicit sums over k != a, b, Python floats, dictionaries), additive trees
recovered by the model, and the command line's --tree-method."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bionj_model
import nj_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = ("andi_hip_tree", "andi_hip_tree_batch", "andi_hip_bootstrap_tree")


def test_both_libraries_export_the_tree_entry_points():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        L = C.CDLL(os.path.join(ROOT, "andi_amd", so))
        for name in NEW:
            assert getattr(L, name) is not None, (so, name)
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SYMBOLS
    assert re.search(r"#define\s+ANDI_TREE_NJ\s+0\b", header) and re.search(r"#define\s+ANDI_TREE_BIONJ\s+1\b", header)
    assert lib.TREE_METHODS == {"nj": 0, "bionj": 1}
    assert lib.load().andi_hip_abi_version() == 5


def test_tree_calls_reject_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    D = np.zeros((2, 4, 4))
    J = np.zeros((2, 2), lib.NJ_JOIN)
    M = np.zeros((4, 4, 17), np.uint32)
    bad = np.zeros(2, np.int64)
    d, j, b, m = D.ctypes.data, J.ctypes.data, bad.ctypes.data, M.ctypes.data
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, d, 4, 1, j), (None, None, 4, 1, j), (None, d, 4, 1, None), (None, d, 1, 1, j), (None, d, 65536, 1, j),
                 (None, d, 4, -1, j), (None, d, 4, 2, j)]:
        assert L.andi_hip_tree(*args) == 1, args
    for args in [(None, d, 4, 2, 1, j, b), (None, None, 4, 2, 1, j, b), (None, d, 4, 2, 1, None, b), (None, d, 4, 2, 1, j, None),
                 (None, d, 4, 0, 1, j, b), (None, d, 1, 2, 1, j, b), (None, d, 65536, 2, 1, j, b), (None, d, 4, 2, -1, j, b),
                 (None, d, 4, 2, 2, j, b)]:
        assert L.andi_hip_tree_batch(*args) == 1, args
    for args in [(None, m, 4, 1, 1, 0, 0, 2, j, b, None), (None, None, 4, 1, 1, 0, 0, 2, j, b, None),
                 (None, m, 4, 1, 1, 0, 0, 2, None, b, None), (None, m, 4, 1, 1, 0, 0, 2, j, None, None),
                 (None, m, 4, 1, 1, 0, 0, 0, j, b, None), (None, m, 1, 1, 1, 0, 0, 2, j, b, None),
                 (None, m, 65536, 1, 1, 0, 0, 2, j, b, None), (None, m, 4, 1, -1, 0, 0, 2, j, b, None),
                 (None, m, 4, 1, 2, 0, 0, 2, j, b, None), (None, m, 4, 5, 1, 0, 0, 2, j, b, None)]:
        assert L.andi_hip_bootstrap_tree(*args) == 1, args
    for call in (lambda: lib.tree(None, D[0], "upgma"), lambda: lib.tree_batch(None, D, "NJ"),
                 lambda: lib.bootstrap_tree(None, M, 2, method=1)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------- a second restatement, from the paper
def _bionj_scalar(D):
    """BIONJ as Gascuel (1997) states it, on dictionaries keyed by node id, one Python float operation at a time: the
    NJ criterion and branch lengths, lambda = 1/2 + sum over k != a, b of (V_bk - V_ak) / (2 (r - 2) V_ab) held to
    [0, 1] (1/2 where V_ab is 0), and the two reduction formulas.  Records as tuples (a, b, c, la, lb, lc)."""
    n = len(D)
    d = {(i, j): float(D[min(i, j)][max(i, j)]) for i in range(n) for j in range(n) if i != j}
    v = dict(d)
    nodes, out = list(range(n)), []
    for s in range(n - 3):
        r = len(nodes)
        S = {x: sum(d[x, k] for k in nodes if k != x) for x in nodes}
        best = None
        for i, x in enumerate(nodes):
            for y in nodes[i + 1:]:
                key = ((r - 2) * d[x, y] - S[x] - S[y], x, y)
                if best is None or key < best:
                    best = key
        _, a, b = best
        dab, vab = d[a, b], v[a, b]
        la = dab / 2 + (S[a] - S[b]) / (2 * (r - 2))
        lb = dab - la
        out.append((a, b, -1, la, lb, 0.0))
        if vab == 0.0:
            lam = 0.5
        else:
            lam = 0.5 + sum(v[b, k] - v[a, k] for k in nodes if k not in (a, b)) / (2 * (r - 2) * vab)
            lam = min(1.0, max(0.0, lam))
        u = n + s
        for k in nodes:
            if k in (a, b):
                continue
            d[u, k] = d[k, u] = lam * (d[a, k] - la) + (1 - lam) * (d[b, k] - lb)
            v[u, k] = v[k, u] = lam * v[a, k] + (1 - lam) * v[b, k] - lam * (1 - lam) * vab
        nodes = [k for k in nodes if k not in (a, b)] + [u]  # (ids ascend: u is the largest)
    x, y, z = nodes
    out.append((x, y, z, (d[x, y] + d[x, z] - d[y, z]) / 2, (d[x, y] + d[y, z] - d[x, z]) / 2,
                (d[x, z] + d[y, z] - d[x, y]) / 2))
    return out


def _records(rows):
    J = np.zeros(len(rows), nj_model.NJ_JOIN)
    for s, (a, b, c, la, lb, lc) in enumerate(rows):
        J[s] = (a, b, c, 0, la, lb, lc)
    return J


def _splits(J, names):
    return nj_model.unrooted_splits(nj_model.parse_newick(nj_model.newick(J, names))[1], names)


@pytest.mark.parametrize("n", [12, 40])
def test_the_model_is_the_scalar_restatement(n):
    worst = 0.0
    for seed in range(6):
        D, _, names = nj_model.additive_tree(n, seed, 0.05)
        got, want = bionj_model.bionj(D), _records(_bionj_scalar(D))
        assert _splits(got, names) == _splits(want, names), seed
        # the step at r = 4 is left out: with four nodes the complementary pairs tie in Q in exact arithmetic, so rounding
        # picks, and the final record follows that pick
        head = slice(0, n - 4)
        for f in ("a", "b", "c"):
            assert (got[f][head] == want[f][head]).all(), (seed, f)
        for f in ("la", "lb"):
            diff = np.abs(got[f][head] - want[f][head]).max()
            worst = max(worst, diff)
            assert diff <= 1e-12, (seed, f, diff)
    print("n = %d: the largest difference of a length %.3g" % (n, worst))


@pytest.mark.parametrize("n", [40, 60])
def test_the_model_recovers_additive_trees(n):
    found = total = 0
    for seed in range(6):
        D, splits, names = nj_model.additive_tree(n, seed, 0.0)
        got = _splits(bionj_model.bionj(D), names)
        found, total = found + len(got & splits), total + len(splits)
        assert got == splits, seed
    assert found == total == 6 * (n - 3)


def test_the_model_reports_its_lambdas_and_a_prefix_stands_alone():
    D, _, _ = nj_model.additive_tree(30, 4, 0.1)
    J, lam = bionj_model.bionj(D, lambdas=True)
    assert len(J) == 28 and len(lam) == 27 and ((lam["value"] >= 0) & (lam["value"] <= 1)).all()
    assert J.tobytes() == bionj_model.bionj(D).tobytes()
    for k in (0, 1, 9, 27, 28):
        P, pl = bionj_model.bionj(D, steps=k, lambdas=True)
        assert P.tobytes() == J[:k].tobytes() and pl.tobytes() == lam[:min(k, 27)].tobytes(), k
    # n = 2 and 3: no pair join, no lambda; their records are neighbor-joining's
    for n in (2, 3):
        E = np.triu(np.random.default_rng(n).uniform(0.1, 1.0, (n, n)), 1)
        J, lam = bionj_model.bionj(E, lambdas=True)
        assert len(lam) == 0 and J.tobytes() == nj_model.nj(E).tobytes()
    # at the first step V = D, so a matrix of equal distances has equal row sums: lambda is exactly 1/2, and not by the
    # vab == 0 rule
    _, lam = bionj_model.bionj(np.ones((6, 6)), steps=1, lambdas=True)
    assert lam["value"][0] == 0.5 and not lam["halved"][0]


# ------------------------------------------------- the command line's validation (no GPU is reached)
def test_cli_lists_the_option():
    p = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0 and "--tree-method=" in p.stdout.decode()


@pytest.mark.parametrize("value", ["upgma", "", "bionj2"])
def test_cli_refuses_another_method(tmp_path, value):
    paths = []
    for name, seq in (("a", "ACGT" * 400), ("b", "ACGA" * 400)):
        paths.append(str(tmp_path / (name + ".fa")))
        with open(paths[-1], "w") as f:
            f.write(">%s\n%s\n" % (name, seq))
    p = subprocess.run([CLI, "--tree-method=" + value, "--tree=" + str(tmp_path / "t")] + paths, capture_output=True, timeout=60)
    line = "andi-hip: Expected one of 'nj' or 'bionj' for --tree-method, but '%s' was given.\n" % value
    assert (p.returncode, p.stdout, p.stderr.decode()) == (1, b"", line)
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.fa"]
