"""Missing distances from quartets, what needs no GPU: the contract's NumPy restatement (tests/complete_model.py) has the
properties the header states, on additive trees with dyadic branch lengths where every sum is exact; its edges (two rounds,
n = 2, 3, 4, the clamp, the three spellings of a missing pair); the symbols, the argument checks and the command line's
options."""
import os
import re
import subprocess

import numpy as np
import pytest

import complete_model as cm
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ------------------------------------------------- the two properties of the header
@pytest.mark.parametrize("seed", range(12))
def test_round_one_is_never_too_small_and_exact_behind_a_separating_quartet(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(8, 25))
    T = cm.additive(rng, n)
    D = cm.punch(rng, T, float(rng.uniform(0.2, 0.5)))
    M = cm.mirrored(D)
    C, fills = cm.complete(D)
    assert len(fills) == int(np.isnan(np.triu(D, 1)).sum())
    for f in fills:
        i, j = int(f["i"]), int(f["j"])
        assert _bits(C[i, j]) == _bits(C[j, i]) == _bits(f["value"])
        assert (f["round"] == 0) == np.isnan(f["value"])
        if f["round"] == 1:
            assert f["value"] >= T[i, j]
            if cm.separated(T, M, i, j):
                assert f["value"] == T[i, j]
            else:
                assert f["value"] > T[i, j]  # every known quartet puts i with j: the bound is slack by twice the inner branch
    known = np.isfinite(M)
    assert (_bits(C[known]) == _bits(M[known])).all()  # a measured entry is never revised


def test_most_fills_are_exact():
    rng = np.random.default_rng(7)
    total = exact = 0
    for _ in range(20):
        T = cm.additive(rng, int(rng.integers(8, 25)))
        _, fills = cm.complete(cm.punch(rng, T, float(rng.uniform(0.2, 0.5))))
        total += len(fills)
        exact += int((fills["value"] == T[fills["i"], fills["j"]]).sum())
    assert total > 400 and exact >= 0.75 * total, (exact, total)


def test_round_two_can_be_too_small():
    """a filled over-estimate is subtracted as d(k, l): ((0,1),2),(3,(4,5)) with unit branches"""
    T = np.array([[0, 2, 3, 5, 6, 6], [2, 0, 3, 5, 6, 6], [3, 3, 0, 4, 5, 5], [5, 5, 4, 0, 3, 3], [6, 6, 5, 3, 0, 2],
                  [6, 6, 5, 3, 2, 0]], float)
    rng = np.random.default_rng(3)
    low = 0
    for _ in range(300):
        D = cm.punch(rng, T, 0.45)
        _, fills = cm.complete(D)
        late = fills[fills["round"] >= 2]
        low += int((late["value"] < T[late["i"], late["j"]]).sum())
        first = fills[fills["round"] == 1]
        assert (first["value"] >= T[first["i"], first["j"]]).all()
    assert low > 0


def test_vectorised_step_is_the_triple_loop():
    rng = np.random.default_rng(11)
    for n in (4, 5, 9, 14):
        A = rng.uniform(-1.0, 2.0, (n, n))
        D = cm.punch(rng, np.triu(A, 1) + np.triu(A, 1).T, 0.35)
        C1, f1 = cm.complete(D)
        C2, f2 = cm.complete(D, cand=cm.candidates_loops)
        assert C1.tobytes() == C2.tobytes() and f1.tobytes() == f2.tobytes()


# ------------------------------------------------- edges
def two_round_case():
    """n = 6: (0,1) has the one quartet {2,3} in round 1; (0,4) needs (0,1) and gets it in round 2 from {1,5}"""
    nan = np.nan
    D = np.zeros((6, 6))
    D[0, 1], D[0, 2], D[0, 3], D[0, 4], D[0, 5] = nan, 3.0, 4.0, nan, 2.5
    D[1, 2], D[1, 3], D[1, 4], D[1, 5] = 2.0, 3.0, 1.5, 2.0
    D[2, 3], D[2, 4], D[2, 5] = 1.0, nan, nan
    D[3, 4], D[3, 5] = nan, nan
    D[4, 5] = 1.25
    return D


def test_two_rounds_and_max_rounds():
    D = two_round_case()
    C, fills = cm.complete(D)
    by = {(int(f["i"]), int(f["j"])): f for f in fills}
    assert by[(0, 1)]["round"] == 1 and by[(0, 1)]["quartets"] == 1
    assert by[(0, 1)]["value"] == max(3.0 + 3.0, 4.0 + 2.0) - 1.0 == 5.0
    assert by[(0, 4)]["round"] == 2 and by[(0, 4)]["quartets"] == 1
    assert by[(0, 4)]["value"] == max(5.0 + 1.25, 2.5 + 1.5) - 2.0
    C1, fills1 = cm.complete(D, max_rounds=1)
    assert np.isnan(C1[0, 4]) and C1[0, 1] == 5.0
    assert {int(r) for r in fills1["round"]} <= {0, 1}
    assert (fills1["round"] == 1).sum() == (fills["round"] == 1).sum()


def test_small_n():
    for n in (2, 3):
        D = np.full((n, n), np.nan)
        D[0, n - 1] = 1.0
        C, fills = cm.complete(D)
        assert len(fills) == n * (n - 1) // 2 - 1 and (fills["round"] == 0).all()
        assert C[0, n - 1] == C[n - 1, 0] == 1.0 and (np.diag(C) == 0).all()
        assert (_bits(C[np.isnan(C)]) == 0x7ff8000000000000).all()
    D = np.array([[0, np.nan, 1, 2], [0, 0, 3, 4], [0, 0, 0, 5], [0, 0, 0, 0]], float)
    C, fills = cm.complete(D)
    assert len(fills) == 1 and fills[0]["quartets"] == 1 and fills[0]["round"] == 1
    assert C[0, 1] == C[1, 0] == max(1.0 + 4.0, 2.0 + 3.0) - 5.0 == 0.0
    D[2, 3] = np.nan  # (0,1) and (2,3): each is the other's only (k, l)
    C, fills = cm.complete(D)
    assert len(fills) == 2 and (fills["round"] == 0).all() and np.isnan(C[0, 1]) and np.isnan(C[2, 3])


def test_clamp():
    D = np.array([[0, np.nan, 1, 1], [0, 0, 1, 1], [0, 0, 0, 5], [0, 0, 0, 0]], float)  # 2 - 5 < 0
    C, fills = cm.complete(D)
    assert _bits(fills["value"])[0] == 0 and _bits(C[0, 1]) == 0 and _bits(C[1, 0]) == 0
    D[2, 3] = 2.0  # exactly zero, from 2 - 2; and -0.0 cannot come out
    D[0, 2] = D[0, 3] = D[1, 2] = D[1, 3] = 1.0
    assert _bits(cm.complete(D)[1]["value"])[0] == 0


def test_infinities_are_missing_and_negatives_are_known():
    base = np.array([[0, 0, 1, 2], [0, 0, 3, 4], [0, 0, 0, -5], [0, 0, 0, 0]], float)
    outs = []
    for miss in (np.nan, np.inf, -np.inf):
        D = base.copy()
        D[0, 1] = miss
        outs.append(cm.complete(D))
    for C, fills in outs:
        assert C.tobytes() == outs[0][0].tobytes() and fills.tobytes() == outs[0][1].tobytes()
    assert outs[0][0][0, 1] == 5.0 - (-5.0) and outs[0][0][2, 3] == -5.0
    for miss in (np.inf, -np.inf):  # as an operand: no candidate
        D = base.copy()
        D[0, 1], D[2, 3] = np.nan, miss
        C, fills = cm.complete(D)
        assert (fills["round"] == 0).all() and len(fills) == 2
        assert (_bits(C[[0, 2], [1, 3]]) == 0x7ff8000000000000).all()


# ------------------------------------------------- the C-ABI
def test_symbols_are_declared_and_exported():
    from andi_amd import lib
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    L = lib.load()
    for name in ("andi_hip_complete", "andi_hip_complete_batch"):
        assert re.search(r"^int %s\(andi_hip_ctx \*ctx, const double \*D, size_t n" % name, header, re.M), name
        assert hasattr(L, name)
    assert "} andi_hip_fill;" in header
    assert re.search(r"#define ANDI_HIP_ABI_VERSION 5\b", header) and L.andi_hip_abi_version() == 5
    assert lib.FILL.itemsize == 32 and lib.FILL == cm.FILL
    import andi_amd
    assert andi_amd.complete is lib.complete and andi_amd.complete_batch is lib.complete_batch


def test_complete_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    import ctypes as C
    L = lib.load()
    D = np.zeros((2, 4, 4))
    out = np.zeros((2, 4, 4))
    fills = np.zeros(6, lib.FILL)
    m, l = C.c_size_t(0), C.c_size_t(0)
    mm, ll = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    d, c, f = D.ctypes.data, out.ctypes.data, fills.ctypes.data
    # with no context nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, d, 4, 0, c, f, 6, C.byref(m), C.byref(l)), (None, None, 4, 0, c, f, 6, C.byref(m), C.byref(l)),
                 (None, d, 1, 0, c, f, 6, C.byref(m), C.byref(l)), (None, d, 65536, 0, c, f, 6, C.byref(m), C.byref(l)),
                 (None, d, 4, 0, c, None, 6, C.byref(m), C.byref(l)), (None, d, 4, 0, None, f, 6, C.byref(m), C.byref(l))]:
        assert L.andi_hip_complete(*args) == 1, args
    for args in [(None, d, 4, 2, 0, c, mm.ctypes.data, ll.ctypes.data), (None, d, 4, 0, 0, c, mm.ctypes.data, ll.ctypes.data),
                 (None, d, 1, 2, 0, c, mm.ctypes.data, ll.ctypes.data), (None, d, 65536, 2, 0, c, mm.ctypes.data, ll.ctypes.data),
                 (None, d, 4, 2, 0, None, mm.ctypes.data, ll.ctypes.data), (None, d, 4, 2, 0, c, None, ll.ctypes.data)]:
        assert L.andi_hip_complete_batch(*args) == 1, args


# ------------------------------------------------- the command line's validation (no GPU is reached)
def test_cli_lists_the_new_options():
    p = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    text = p.stdout.decode()
    assert p.returncode == 0
    for option in ("--complete ", "--complete-report=FILE"):
        assert option in text, option


@pytest.mark.parametrize("option", ["--complete", "--complete-report=R"])
def test_cli_refuses_complete_with_trees_only(tmp_path, option):
    files = []
    for k in range(2):
        path = tmp_path / ("g%d.fa" % k)
        path.write_text(">g%d\nACGTACGTTGCA\n" % k)
        files.append(str(path))
    p = subprocess.run([CLI, option, "--trees-only", "-b", "3", "--tree=T"] + files, capture_output=True, timeout=60,
                       cwd=str(tmp_path))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.decode().strip() == ("andi-hip: Missing distances (--complete) are not derived together with --trees-only: "
                                         "the bootstrap matrices stay on the GPU.")
    assert not os.path.exists(tmp_path / "T") and not os.path.exists(tmp_path / "R")  # refused before a file is opened
