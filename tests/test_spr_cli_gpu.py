"""andi-hip --refine=bnni --refine-moves=spr end to end on the MI355X: every line of --tree is the model's SPR-refined
records of its own matrix (the point estimate and the -b 3 replicates), the report is the model's numbers under its own
headers; --refine-moves=nni and no option write the files of --refine=bnni alone; the usage errors."""
import os
import subprocess

import numpy as np
import pytest

import nj_model
import spr_model as sm
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
    d = tmp_path_factory.mktemp("spr_cli")
    seqs, _ = synth.tree_set(N, 20_000, seed=5)
    names = ["g%d" % k for k in range(N)]
    files = [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    M = lib.dist_matrix(seqs, host_threads=4)
    c = lib.Context(0)
    try:
        B = lib.bootstrap_range(c, M, 0, 2, seed=SEED)
        Ds = [lib.distances(M, lib.M_JC)] + [lib.distances(b, lib.M_JC) for b in B]
        Js = [lib.tree(c, D, "nj") for D in Ds]
    finally:
        c.close()
    assert all(np.isfinite(D).all() for D in Ds)
    return names, files, Ds, Js


def _run(args, files):
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))  # (the same bootstrap matrices in every run)
    env.pop("ANDI_HIP_BOOT_CHUNK", None)
    p = subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def test_every_line_of_tree_and_the_report_are_the_models(tmp_path, genomes):
    names, files, Ds, Js = genomes
    tree, plain, report = str(tmp_path / "t.nwk"), str(tmp_path / "p.nwk"), str(tmp_path / "r.tsv")
    rc, out, err = _run(["-b", "3", "--tree=" + tree, "--refine=bnni", "--refine-moves=SPR", "--refine-report=" + report], files)
    rc0, out0, err0 = _run(["-b", "3", "--tree=" + plain], files)
    assert (rc, rc0) == (0, 0) and out == out0 and err == err0, (err, err0)
    lines, joined = open(tree).readlines(), open(plain).readlines()
    assert len(lines) == len(joined) == 3
    want = [sm.refine_spr(J, D, tol=TOL, max_moves=10 * N) for J, D in zip(Js, Ds)]
    for k in range(3):
        assert joined[k] == nj_model.newick(Js[k], names) and lines[k] == nj_model.newick(want[k][0], names), k
        assert lines[k] != joined[k]  # (the balanced lengths, at the least)
    K, res, log = want[0]
    import bme_model as bm
    changed = len(bm.inner_splits(Js[0]) - bm.inner_splits(K))
    text = ["#method\tmoves\tconverged\tlength_before\tlength_after\tchanged",
            "bspr\t%d\t%d\t%.8g\t%.8g\t%d" % (res["moves"], res["converged"], res["length_before"], res["length_after"], changed),
            "#move\tgain\tfirst\tsecond\thops"]
    text += ["%d\t%.8g\t%s\t%s\t%d" % (k + 1, m["gain"], names[m["first"]], names[m["second"]], m["hops"]) for k, m in enumerate(log)]
    assert open(report).read() == "\n".join(text) + "\n"


def test_a_tolerance_nothing_passes_leaves_the_joined_branches(tmp_path, genomes):
    names, files, Ds, Js = genomes
    tree, report = str(tmp_path / "t.nwk"), str(tmp_path / "r.tsv")
    rc, out, err = _run(["--tree=" + tree, "--refine=bnni", "--refine-moves=spr", "--refine-tol=1e9", "--refine-report=" + report], files)
    assert rc == 0, err
    assert open(report).read().splitlines()[1].split("\t")[:3] == ["bspr", "0", "1"]
    assert open(tree).read() == nj_model.newick(sm.refine_spr(Js[0], Ds[0], tol=1e9)[0], names)


def test_nni_and_no_option_are_the_bytes_of_bnni_alone(tmp_path, genomes):
    names, files, _, _ = genomes
    kinds = ("tree", "support", "refine-report")
    runs = []
    for tag, extra in (("a", []), ("b", ["--refine-moves=nni"]), ("c", ["--refine-moves=NNI"])):
        paths = {k: str(tmp_path / ("%s_%s" % (tag, k))) for k in kinds}
        rc, out, err = _run(["-b", "3", "--refine=bnni"] + extra + ["--%s=%s" % kv for kv in paths.items()], files)
        assert rc == 0, err
        runs.append((out, err) + tuple(open(paths[k]).read() for k in kinds))
    assert runs[0] == runs[1] == runs[2] and all(runs[0][2:])
    assert runs[0][4].splitlines()[1].startswith("bnni\t") and runs[0][4].splitlines()[2] == "#move\tgain\tfirst\tsecond"


def test_the_usage_errors(tmp_path, genomes):
    names, files, _, _ = genomes
    tree = "--tree=" + str(tmp_path / "t.nwk")
    rc, out, err = _run(["--refine=bnni", "--refine-moves=tbr", tree], files)
    assert rc == 1 and out == b"" and "Expected one of 'nni' or 'spr' for --refine-moves, but 'tbr' was given." in err
    for extra in ([], ["--refine=none"]):
        for moves in ("spr", "nni"):
            rc, out, err = _run(["--refine-moves=" + moves, tree] + extra, files)
            assert rc == 1 and out == b"" and "The moves of the refinement (--refine-moves) need --refine=bnni." in err
    rc, out, err = _run(["--refine=bnni", "--refine-moves=spr", "--trees-only", "-b", "3", tree], files)
    assert rc == 1 and out == b"" and "Trees (--refine=bnni) are not refined together with --trees-only" in err
    rc, out, err = _run(["--refine=spr", tree], files)
    assert rc == 1 and out == b"" and "Expected one of 'none' or 'bnni' for --refine, but 'spr' was given." in err
