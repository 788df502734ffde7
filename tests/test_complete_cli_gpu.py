"""andi-hip --complete end to end on the MI355X: six genomes of which four pairs have no distance -- two pairs of genomes
from unrelated bases, and two genomes that carry both bases, the one quartet of every hole.  Without the option the tree is
refused; with it stdout is unchanged, the tree is the one the Python layer builds from the completed matrix, the report
names the four fills, and the bootstrap matrices' trees are written likewise."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
HOLES = [(0, 2), (0, 3), (1, 2), (1, 3)]


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    from andi_amd import lib, synth
    mut = lambda base, d, seed: synth.mutate_codes(base, d, seed, raw=True)
    P, Q = synth.base_codes(20000, 11), synth.base_codes(20000, 12)
    codes = [mut(P, 0.02, 1), mut(P, 0.03, 2), mut(Q, 0.02, 3), mut(Q, 0.03, 4),
             np.concatenate([mut(P, 0.01, 5), mut(Q, 0.01, 6)]), np.concatenate([mut(P, 0.04, 7), mut(Q, 0.04, 8)])]
    seqs = [synth.to_bytes(c) for c in codes]
    names = ["g%d" % k for k in range(6)]
    d = tmp_path_factory.mktemp("genomes")
    files = [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    M = lib.dist_matrix(seqs, host_threads=4)
    D = lib.distances(M, lib.M_JC)
    missing = [(int(i), int(j)) for i, j in np.argwhere(np.triu(~np.isfinite(D), 1))]
    assert missing == HOLES, missing  # the recipe: exactly these four, each with the one quartet {4, 5}
    # (every other pair has a distance, of about 0.03 to 0.07)
    return names, files, D


def _run(files, args, env=None):
    e = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED="4711")
    e.pop("ANDI_HIP_BOOT_CHUNK", None)
    e.update(env or {})
    return subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=e)


def test_tree_of_the_completed_matrix_and_the_report(ctx, tmp_path, genomes):
    from andi_amd import lib
    names, files, D = genomes
    plain = _run(files, ["--tree=%s" % (tmp_path / "plain.nwk")])
    assert plain.returncode == 1  # (a nan was printed)
    assert any(l.endswith("No tree for matrix 1: the distance of 'g0' and 'g2' is not finite.") for l in plain.stderr.decode().splitlines())
    assert open(tmp_path / "plain.nwk").read() == ""
    C, fills = lib.complete(ctx, D)
    assert [(int(f["i"]), int(f["j"])) for f in fills] == HOLES
    assert (fills["round"] == 1).all() and (fills["quartets"] == 1).all() and np.isfinite(C).all()
    for method in ("nj", "bionj"):
        tree, report = tmp_path / ("%s.nwk" % method), tmp_path / ("%s.tsv" % method)
        p = _run(files, ["--tree=%s" % tree, "--complete-report=%s" % report, "--tree-method=%s" % method])
        assert p.returncode == 1 and p.stdout == plain.stdout  # stdout is not touched: the nan is still printed
        err = p.stderr.decode()
        assert err.count("Matrix 1: 4 of 4 missing distances were derived from quartets (--complete).") == 1
        assert "No tree" not in err
        assert open(tree).read() == lib.newick(lib.tree(ctx, C, method), names)
        lines = open(report).read().splitlines()
        assert lines[0] == "#first\tsecond\tdistance\tround\tquartets"
        assert lines[1:] == ["g%d\tg%d\t%.8g\t1\t1" % (f["i"], f["j"], f["value"]) for f in fills]
    # --complete alone: the same tree, no report
    p = _run(files, ["--tree=%s" % (tmp_path / "c.nwk"), "--complete"])
    assert p.stdout == plain.stdout and open(tmp_path / "c.nwk").read() == open(tmp_path / "nj.nwk").read()


@pytest.mark.parametrize("method", ["nj", "bionj"])
@pytest.mark.parametrize("with_support", [False, True])
def test_bootstrap_matrices_are_completed(tmp_path, genomes, method, with_support):
    """-b 3: the point estimate's line and one per bootstrap matrix -- or, for one that could not be completed, the refusal in
    its place; with --support the replicates go through one andi_hip_complete_batch call"""
    names, files, D = genomes
    tree = tmp_path / "b.nwk"
    args = ["-b", "3", "--tree=%s" % tree, "--complete", "--tree-method=%s" % method]
    if with_support:
        args.append("--support=%s" % (tmp_path / "s.nwk"))
    p = _run(files, args)
    plain = _run(files, ["-b", "3"])
    assert p.stdout == plain.stdout
    err = p.stderr.decode()
    lines = open(tree).read().splitlines()
    refused = [l for l in err.splitlines() if "No tree for matrix" in l]
    assert all(l.endswith("is not finite and could not be derived.") for l in refused)
    assert len(lines) + len(refused) == 3 and len(lines) >= 1
    assert all(l.startswith("(") and l.endswith(";") and all(nm in l for nm in names) for l in lines)
    assert err.count("Matrix 1: 4 of 4 missing distances were derived from quartets (--complete).") == 1
    assert err.count("missing distances were derived from quartets (--complete).") >= len(lines)
    if with_support:
        assert open(tmp_path / "s.nwk").read().count(";") == 1
