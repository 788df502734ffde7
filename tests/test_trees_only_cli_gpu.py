"""andi-hip -b N --trees-only end to end on the MI355X: the replicates' trees without their matrices, against the same trees
built in Python from andi_hip_bootstrap_nj; and -b N in bounded memory: chunks of replicates (ANDI_HIP_BOOT_CHUNK) change
neither stdout nor any of the four tree files."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
SEED = 4711
FILES = ("tree", "support", "consensus", "transfer")


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    from andi_amd import synth
    n = 8
    seqs, _ = synth.tree_set(n, 5000, seed=9)
    names = ["g%d" % k for k in range(n)]
    d = tmp_path_factory.mktemp("genomes")
    return seqs, names, [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]


def _run(files, args, env=None, ok=True):
    e = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))
    e.pop("ANDI_HIP_BOOT_CHUNK", None)
    e.update(env or {})
    p = subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=e)
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p


def _outputs(d, tag):
    return {k: str(d / ("%s_%s.nwk" % (tag, k))) for k in FILES}


def _args(paths):
    return ["--%s=%s" % (k, v) for k, v in paths.items()]


@pytest.mark.timeout(300)
def test_trees_only(tmp_path, genomes):
    from andi_amd import lib
    seqs, names, files = genomes
    n = len(names)
    point = _run(files, []).stdout
    paths = _outputs(tmp_path, "only")
    p = _run(files, ["-b", "6", "--trees-only"] + _args(paths))
    assert p.stdout == point  # the point estimate's matrix, and no other
    # the same trees from the library: five replicates of the stream of that seed
    ctx = lib.Context(0)
    try:
        M = lib.dist_matrix(seqs, host_threads=4)
        J = lib.nj(ctx, lib.distances(M, lib.M_JC))
        R, bad = lib.bootstrap_nj(ctx, M, 5, lib.M_JC, seed=SEED)
        skip = (bad >= 0).astype(np.uint8)
        support = lib.nj_support(ctx, J, R, skip=skip)
        depth, transfer = lib.nj_transfer(ctx, J, R, skip=skip)
    finally:
        ctx.close()
    usable = int((bad < 0).sum())
    assert usable >= 1
    assert open(paths["support"]).read() == lib.newick(J, names, support=support)
    assert open(paths["transfer"]).read() == lib.newick_transfer(J, depth, transfer, usable, names)
    lines = open(paths["tree"]).read().splitlines(keepends=True)
    assert len(lines) == 1 + usable
    assert lines[0] == lib.newick(J, names)
    assert lines[1:] == [lib.newick(R[k], names) for k in range(5) if bad[k] < 0]
    cons = open(paths["consensus"]).read()
    assert cons.endswith(");\n") and cons.count("\n") == 1 and all(name in cons for name in names)
    # --tree alone takes the same path
    alone = str(tmp_path / "alone.nwk")
    p = _run(files, ["-b", "6", "--trees-only", "--tree=" + alone])
    assert p.stdout == point and open(alone).read().splitlines(keepends=True) == lines


def test_trees_only_usage_errors(tmp_path, genomes):
    _, _, files = genomes
    p = _run(files, ["--trees-only", "--tree=" + str(tmp_path / "t.nwk")], ok=False)
    assert p.returncode != 0 and b"--trees-only" in p.stderr and p.stdout == b""
    p = _run(files, ["-b", "6", "--trees-only"], ok=False)
    assert p.returncode != 0 and b"--trees-only" in p.stderr and p.stdout == b""


@pytest.mark.timeout(300)
def test_chunks_of_replicates_change_nothing(tmp_path, genomes):
    _, _, files = genomes
    a, b = _outputs(tmp_path, "whole"), _outputs(tmp_path, "chunks")
    whole = _run(files, ["-b", "6"] + _args(a))
    chunks = _run(files, ["-b", "6"] + _args(b), env={"ANDI_HIP_BOOT_CHUNK": "2"})
    assert chunks.stdout == whole.stdout and whole.stdout.count(b"\n") == 6 * (len(files) + 1)
    for k in FILES:
        assert open(a[k]).read() == open(b[k]).read(), k
        assert open(a[k]).read().endswith(";\n")
    assert len(open(a["tree"]).read().splitlines()) >= 2
