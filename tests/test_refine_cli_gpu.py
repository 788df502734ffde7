"""andi-hip --refine=bnni end to end on the MI355X: without the option and with --refine=none every file keeps its bytes;
with bnni every line of --tree is the model's refined records of its own matrix, the report is the model's numbers, the
support counts are taken on the refined trees; the refusals."""
import os
import subprocess

import numpy as np
import pytest

import bme_model as bm
import nj_model
import support_model
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
N = 9
SEED = 11
TOL = 1e-9


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """a small synthetic set, its matrix, and the matrices of -b 3 under the seed"""
    from andi_amd import lib, synth
    d = tmp_path_factory.mktemp("refine_cli")
    seqs, _ = synth.tree_set(N, 20_000, seed=5)
    names = ["g%d" % k for k in range(N)]
    files = [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    M = lib.dist_matrix(seqs, host_threads=4)
    c = lib.Context(0)
    try:
        B = lib.bootstrap_range(c, M, 0, 2, seed=SEED)
    finally:
        c.close()
    Ds = [lib.distances(M, lib.M_JC)] + [lib.distances(b, lib.M_JC) for b in B]
    assert all(np.isfinite(D).all() for D in Ds)
    return names, files, Ds


def _run(args, files):
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))  # (the same bootstrap matrices in every run)
    env.pop("ANDI_HIP_BOOT_CHUNK", None)
    p = subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=env)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _model(ctx, D, method="nj"):
    """(the library's joined records, the model's refined records, result, log) of the matrix D"""
    from andi_amd import lib
    J = lib.tree(ctx, D, method)
    return (J,) + bm.refine(J, D, tol=TOL, max_moves=10 * len(D))


KINDS = ("tree", "support", "transfer", "consensus", "rogues")


def test_none_and_no_option_are_the_same_bytes(tmp_path, genomes):
    names, files, _ = genomes
    a = {k: str(tmp_path / ("a_%s" % k)) for k in KINDS}
    b = {k: str(tmp_path / ("b_%s" % k)) for k in KINDS}
    rc0, out0, err0 = _run(["-b", "3", "--root=mad", "--lengths=ols"] + ["--%s=%s" % kv for kv in a.items()], files)
    rc1, out1, err1 = _run(["-b", "3", "--root=mad", "--lengths=ols", "--refine=None"] + ["--%s=%s" % kv for kv in b.items()], files)
    assert (rc0, out0, err0) == (rc1, out1, err1) and rc0 == 0, (err0, err1)
    for k in KINDS:
        assert open(a[k]).read() == open(b[k]).read() != "", k
    # without a tree output the option does nothing
    rc2, out2, err2 = _run(["--refine=bnni"], files)
    rc3, out3, err3 = _run([], files)
    assert (rc2, out2, err2) == (rc3, out3, err3) and rc2 == 0


@pytest.mark.parametrize("method", ["nj", "bionj"])
def test_every_line_of_tree_is_the_models_refined_tree(ctx, tmp_path, genomes, method):
    names, files, Ds = genomes
    tree, plain = str(tmp_path / "t.nwk"), str(tmp_path / "p.nwk")
    rc, out, err = _run(["-b", "3", "--tree=" + tree, "--refine=BNNI", "--tree-method=" + method], files)
    rc0, out0, err0 = _run(["-b", "3", "--tree=" + plain, "--tree-method=" + method], files)
    assert (rc, rc0) == (0, 0) and out == out0 and err == err0, (err, err0)
    lines, joined = open(tree).readlines(), open(plain).readlines()
    assert len(lines) == len(joined) == 3
    for k, D in enumerate(Ds):
        J, K, _, _ = _model(ctx, D, method)
        assert joined[k] == nj_model.newick(J, names) and lines[k] == nj_model.newick(K, names), k
        assert lines[k] != joined[k]  # (the balanced lengths, at the least)


def test_the_report_is_the_models_numbers(ctx, tmp_path, genomes):
    names, files, Ds = genomes
    tree, report = str(tmp_path / "t.nwk"), str(tmp_path / "r.tsv")
    J, K, res, log = _model(ctx, Ds[0])
    for extra in ([], ["--refine-tol=1e-9", "-b", "3", "--support=" + str(tmp_path / "s.nwk")]):
        rc, out, err = _run(["--tree=" + tree, "--refine=bnni", "--refine-report=" + report] + extra, files)
        assert rc == 0, err
        changed = len(bm.inner_splits(J) - bm.inner_splits(K))
        want = ["#method\tmoves\tconverged\tlength_before\tlength_after\tchanged",
                "bnni\t%d\t%d\t%.8g\t%.8g\t%d" % (res["moves"], res["converged"], res["length_before"], res["length_after"], changed),
                "#move\tgain\tfirst\tsecond"]
        want += ["%d\t%.8g\t%s\t%s" % (k + 1, m["gain"], names[m["first"]], names[m["second"]]) for k, m in enumerate(log)]
        assert open(report).read() == "\n".join(want) + "\n"
    # a tolerance nothing passes: no move, the joined tree's branches with balanced lengths
    rc, out, err = _run(["--tree=" + tree, "--refine=bnni", "--refine-tol=1e9", "--refine-report=" + report], files)
    assert rc == 0 and open(report).read().splitlines()[1].split("\t")[1:3] == ["0", "1"]
    assert open(tree).read() == nj_model.newick(bm.refine(J, Ds[0], tol=1e9)[0], names)


def test_support_counts_are_taken_on_the_refined_trees(ctx, tmp_path, genomes):
    names, files, Ds = genomes
    support, tree = str(tmp_path / "s.nwk"), str(tmp_path / "t.nwk")
    rc, out, err = _run(["-b", "3", "--refine=bnni", "--support=" + support, "--tree=" + tree], files)
    assert rc == 0, err
    K = [_model(ctx, D)[1] for D in Ds]
    counts = support_model.support(K[0], np.stack(K[1:]))
    assert open(support).read() == support_model.newick_support(K[0], counts, names)
    assert open(tree).readlines() == [nj_model.newick(k, names) for k in K]


def test_the_refusals(tmp_path, genomes):
    names, files, _ = genomes
    tree = "--tree=" + str(tmp_path / "t.nwk")
    rc, out, err = _run(["--refine=bnni", "--trees-only", "-b", "3", tree], files)
    assert rc == 1 and out == b"" and "Trees (--refine=bnni) are not refined together with --trees-only" in err
    rc, out, err = _run(["--refine-report=" + str(tmp_path / "r.tsv"), tree], files)
    assert rc == 1 and out == b"" and "A refinement report (--refine-report) needs --refine=bnni." in err
    rc, out, err = _run(["--refine=spr", tree], files)
    assert rc == 1 and out == b"" and "Expected one of 'none' or 'bnni' for --refine, but 'spr' was given." in err
