"""The rogue genomes of a bootstrap without a GPU: the entry point's declarations, the two statements of the contract in
tests/rogue_model.py against each other and against tests/transfer_model.py through the relations the header states, the
argument checks of andi_hip_nj_transfer_taxa, and the command line's refusals of --rogues and --rogue-cutoff."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import nj_model
import rogue_model
import transfer_model
from conftest import ROOT

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NEW = "andi_hip_nj_transfer_taxa"
CUTOFFS = (0.0, 0.3, 1.0)


def test_both_libraries_export_the_entry_point():
    from andi_amd import lib
    for so in ("libandihip.so", "libandihip_test.so"):
        assert getattr(C.CDLL(os.path.join(ROOT, "andi_amd", so)), NEW) is not None, so
    header = open(os.path.join(ROOT, "include", "andi_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % NEW, header) and NEW in lib.SYMBOLS
    assert lib.load().andi_hip_abi_version() == 5
    assert "#define ANDI_HIP_ABI_VERSION 5\n" in header
    import andi_amd
    assert andi_amd.nj_transfer_taxa is lib.nj_transfer_taxa


def _sym(rng, n):
    A = rng.uniform(0.1, 1.0, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _noisy(D, rng, size):
    E = np.triu(rng.uniform(-size, size, D.shape), 1)
    return D * (1.0 + E + E.T)


def _nj_case(n):
    """the tree of a random matrix and those of the matrix itself, lightly and heavily perturbed (test_transfer_host.py's)"""
    rng = np.random.default_rng(n)
    D = _sym(rng, n)
    tree = nj_model.nj(D)
    return tree, [tree, nj_model.nj(_noisy(D, rng, 0.02)), nj_model.nj(_noisy(D, rng, 0.5))]


def test_the_two_statements_of_the_model_agree_and_the_relations_hold():
    counted_far = uncounted = 0
    for n in range(4, 141):
        tree, reps = _nj_case(n)
        depth, total, per = transfer_model.transfer(tree, reps)
        near = rogue_model.nearest_all(tree, reps)
        support = [sum(row[s] == 0 for row in per) for s in range(n - 3)]
        for cutoff in CUTOFFS:
            moved, pairs, match, dist = rogue_model.taxa(tree, reps, cutoff=cutoff, near=near)
            m2, p2, t2, d2 = rogue_model.taxa_numpy(tree, reps, cutoff=cutoff)
            assert m2.dtype == np.uint64 and t2.dtype == np.uint32 and d2.dtype == np.uint32
            assert moved == m2.tolist() and pairs == p2 and match == t2.tolist() and dist == d2.tolist(), (n, cutoff)
            # min(dist, depth - 1) is the transfer index
            assert [[min(d, depth[s] - 1) for s, d in enumerate(row)] for row in dist] == per, n
            # the moved leaves of the counted pairs are dist of them each
            on = [[d <= rogue_model.limit(cutoff, depth[s]) for s, d in enumerate(row)] for row in dist]
            assert pairs == sum(map(sum, on))
            assert sum(moved) == sum(d for row, o in zip(dist, on) for d, c in zip(row, o) if c), (n, cutoff)
            assert all(0 <= t < n - 3 for row in match for t in row)
            if cutoff == 0.0:
                assert not any(moved) and pairs == sum(support), n
            else:
                counted_far += sum(d > 0 for row, o in zip(dist, on) for d, c in zip(row, o) if c)
            uncounted += sum(not c for o in on for c in o)
        assert dist[0] == [0] * (n - 3)
    assert counted_far > 0 and uncounted > 0
    # a skipped replicate, and chunks that add up (n = 140)
    skip = [0, 1, 0]
    moved, pairs, match, dist = rogue_model.taxa(tree, reps, skip, 1.0)
    m2, p2, t2, d2 = rogue_model.taxa_numpy(tree, reps, skip, 1.0)
    assert match[1] == dist[1] == [rogue_model.SKIPPED] * (n - 3)
    assert moved == m2.tolist() and pairs == p2 and match == t2.tolist() and dist == d2.tolist()
    ma, pa, _, _ = rogue_model.taxa(tree, reps[:1], cutoff=1.0)
    mb, pb, _, _ = rogue_model.taxa(tree, reps[2:], cutoff=1.0)
    assert [a + b for a, b in zip(ma, mb)] == moved and pa + pb == pairs
    # fewer than four leaves: no branch
    assert rogue_model.taxa(tree[:1], [tree[:1]]) == ([0, 0, 0], 0, [[]], [[]])
    m3, p3, t3, d3 = rogue_model.taxa_numpy(tree[:1], [tree[:1]])
    assert m3.tolist() == [0, 0, 0] and p3 == 0 and t3.shape == d3.shape == (1, 0)


def test_the_recipe_of_replicates_has_ties_and_far_sides():
    # what tests/test_rogues_gpu.py relies on, at its smallest sizes
    for n in (8, 63, 65):
        tree, reps = rogue_model.replicates(n)
        assert len(reps) == 8
        ties, flips = rogue_model.ties_and_flips(tree, reps, 1.0)
        assert ties > 0 and flips > 0, (n, ties, flips)


def test_rejects_bad_arguments_without_a_device_call():
    from andi_amd import lib
    L = lib.load()
    J = np.zeros((2, 2), lib.NJ_JOIN)
    moved, pairs = np.full(4, 7, np.uint64), np.full(1, 7, np.uint64)
    match, dist = np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    j, m, p, t, d = J.ctypes.data, moved.ctypes.data, pairs.ctypes.data, match.ctypes.data, dist.ctypes.data
    nan, inf = float("nan"), float("inf")
    # with no context, nothing else is looked at; the other checks come before any HIP call too
    for args in [(None, j, j, 4, 2, None, 0.3, m, p, t, d), (None, None, j, 4, 2, None, 0.3, m, p, t, d),
                 (None, j, None, 4, 2, None, 0.3, m, p, t, d), (None, j, j, 4, 2, None, 0.3, None, p, t, d),
                 (None, j, j, 4, 2, None, 0.3, m, None, t, d), (None, j, j, 4, 0, None, 0.3, m, p, t, d),
                 (None, j, j, 1, 2, None, 0.3, m, p, t, d), (None, j, j, 0, 2, None, 0.3, m, p, t, d),
                 (None, j, j, 65536, 2, None, 0.3, m, p, t, d), (None, j, j, 4, 2, None, nan, m, p, t, d),
                 (None, j, j, 4, 2, None, -0.5, m, p, t, d), (None, j, j, 4, 2, None, 1.5, m, p, t, d),
                 (None, j, j, 4, 2, None, inf, m, p, t, d), (None, j, j, 3, 2, None, 0.3, m, p, None, None)]:
        assert L.andi_hip_nj_transfer_taxa(*args) == 1, args
    assert (moved == 7).all() and pairs[0] == 7 and (match == 7).all() and (dist == 7).all()


def _run(args, stdin=b""):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _fa(path, name, seq=b"ACGTACGTACGTTTGA"):
    path.write_text(">%s\n%s\n" % (name, seq.decode()))
    return str(path)


WITH_REFERENCE = " not available together with --reference or --reference-list."
NEEDS_B = " bootstrap matrices: give -b N with N of at least 2."


def test_cli_refusals_of_rogues_and_its_cutoff(tmp_path):
    rc, out, err = _run(["--help"])
    assert rc == 0 and "--rogues=FILE" in out and "--rogue-cutoff=X" in out
    a, b = _fa(tmp_path / "a.fa", "A"), _fa(tmp_path / "b.fa", "B")
    rg = tmp_path / "r.tsv"
    # these refusals come before any sequence is read, any file is made and any device call
    for ref in ("--reference=" + a, "--reference-list=" + str(tmp_path / "list")):
        rc, out, err = _run(["--rogues=" + str(rg), ref, b])
        assert rc == 1 and out == "" and err.endswith(": Rogue genomes (--rogues) are" + WITH_REFERENCE + "\n") and not rg.exists()
    for pre in ([], ["-b", "1"]):  # (one matrix: no replicate)
        rc, out, err = _run(pre + ["--rogues=" + str(rg), a, b])
        assert rc == 1 and out == "" and err.endswith(": Rogue genomes (--rogues) need" + NEEDS_B + "\n") and not rg.exists()
    rc, out, err = _run(["-b", "3", "--rogue-cutoff=0.5", a, b])
    assert rc == 1 and out == ""
    assert err.endswith(": A cutoff (--rogue-cutoff) needs somewhere to go: give --rogues=FILE.\n")
    for bad in ("x", "", "0.5x", "nan", "-0.1", "1.01", "inf"):
        rc, out, err = _run(["-b", "3", "--rogues=" + str(rg), "--rogue-cutoff=" + bad, a, b])
        assert rc == 1 and out == "" and "--rogue-cutoff" in err and "'%s'" % bad in err and not rg.exists(), bad
    # the refusals that were there come first, and --rogues is not one of the files --trees-only asks for
    tr = tmp_path / "t.nwk"
    rc, out, err = _run(["--transfer=" + str(tr), "--rogues=" + str(rg), a, b])
    assert rc == 1 and "Transfer support (--transfer) needs" in err and not tr.exists() and not rg.exists()
    rc, out, err = _run(["-b", "3", "--trees-only", "--rogues=" + str(rg), a, b])
    assert rc == 1 and out == "" and "(--trees-only) need somewhere to go" in err and not rg.exists()
    assert "Comparing" not in err
