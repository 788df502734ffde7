"""andi-hip --lengths=ols and --fit=FILE end to end on the MI355X: every line of --tree, --support and --transfer carries the
least-squares lengths of its own matrix (the library's, on the same records), before --root roots it and after --complete
fills the matrix; the report is the call's numbers; stdout, the consensus tree and runs without the options keep their
bytes; the refusals."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from newick_reader import parse, splits

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
N = 7
SEED = 11
HEADER = ("#method\tpairs\trss\trss_joined\ttss\tr2\tr2_joined\tlength\tlength_joined\tnegative\tnegative_joined\tworst_first\t"
          "worst_second\tworst_residual")


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """the tiny genomes of test_root_cli_gpu.py, their matrix, and the matrices of -b 3 under the seed"""
    from andi_amd import lib, synth
    d = tmp_path_factory.mktemp("fit_cli")
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


@pytest.fixture(scope="module")
def holes(tmp_path_factory):
    """test_complete_cli_gpu.py's six genomes: four pairs without a distance, each with one quartet"""
    from andi_amd import lib, synth
    mut = lambda base, d, seed: synth.mutate_codes(base, d, seed, raw=True)
    P, Q = synth.base_codes(20000, 11), synth.base_codes(20000, 12)
    codes = [mut(P, 0.02, 1), mut(P, 0.03, 2), mut(Q, 0.02, 3), mut(Q, 0.03, 4),
             np.concatenate([mut(P, 0.01, 5), mut(Q, 0.01, 6)]), np.concatenate([mut(P, 0.04, 7), mut(Q, 0.04, 8)])]
    seqs = [synth.to_bytes(c) for c in codes]
    names = ["g%d" % k for k in range(6)]
    d = tmp_path_factory.mktemp("fit_holes")
    files = [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    D = lib.distances(lib.dist_matrix(seqs, host_threads=4), lib.M_JC)
    assert not np.isfinite(D[0, 2])
    return names, files, D


def _run(args, files):
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))  # (the same bootstrap matrices in every run)
    env.pop("ANDI_HIP_BOOT_CHUNK", None)
    p = subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def _refit(ctx, D, method="nj"):
    """(J, the relengthed records, the call's results) of the matrix D"""
    from andi_amd import lib
    J = lib.tree(ctx, D, method)
    res = lib.fit(ctx, J, D, "ols", per=True)
    return J, lib.relength(J, res[0]), res


def _g(x):
    return "nan" if np.isnan(x) else "%.8g" % x


def _report(names, res):
    _, rec, ss, ssj = res
    with np.errstate(all="ignore"):
        r2 = [float("nan") if rec["tss"] == 0 else 1.0 - rec[k] / rec["tss"] for k in ("rss", "rss_joined")]
    row = ["ols", "%d" % rec["pairs"], _g(rec["rss"]), _g(rec["rss_joined"]), _g(rec["tss"]), _g(r2[0]), _g(r2[1]), _g(rec["length"]),
           _g(rec["length_joined"]), "%d" % rec["negative"], "%d" % rec["negative_joined"], names[rec["worst_b"]],
           names[rec["worst_c"]], _g(rec["worst"])]
    lines = [HEADER, "\t".join(row), "#name\tss\tss_joined"]
    lines += ["%s\t%s\t%s" % (names[i], _g(ss[i]), _g(ssj[i])) for i in range(len(names))]
    return "\n".join(lines) + "\n"


def _labels_and_lengths(line, names):
    index = {nm: i for i, nm in enumerate(names)}
    got = splits(parse(line), index, len(names), {})
    return {s: v[0][1] for s, v in got.items()}, {s: v[0][0] for s, v in got.items()}


@pytest.mark.parametrize("method", ["nj", "bionj"])
def test_every_line_of_tree_carries_its_own_matrixs_lengths(ctx, tmp_path, genomes, method):
    from andi_amd import lib
    names, files, Ds = genomes
    tree, plain = str(tmp_path / "t.nwk"), str(tmp_path / "p.nwk")
    rc, out, err = _run(["-b", "3", "--tree=" + tree, "--lengths=ols", "--tree-method=" + method], files)
    rc0, out0, err0 = _run(["-b", "3", "--tree=" + plain, "--tree-method=" + method], files)
    assert (rc, rc0) == (0, 0) and out == out0 and err == err0, (err, err0)
    lines, joined = open(tree).readlines(), open(plain).readlines()
    assert len(lines) == len(joined) == 3
    for k, D in enumerate(Ds):
        J, K, _ = _refit(ctx, D, method)
        assert joined[k] == lib.newick(J, names) and lines[k] == lib.newick(K, names), k
        assert lines[k] != joined[k]


@pytest.mark.parametrize("root", ["mad", "midpoint"])
def test_the_refit_comes_before_the_root(ctx, tmp_path, genomes, root):
    from andi_amd import lib
    names, files, Ds = genomes
    tree, report = str(tmp_path / "t.nwk"), str(tmp_path / "r.tsv")
    rc, out, err = _run(["--tree=" + tree, "--lengths=OLS", "--root=" + root, "--root-report=" + report], files)
    assert rc == 0, err
    _, K, _ = _refit(ctx, Ds[0])
    rec = lib.root(ctx, K, root)
    assert open(tree).read() == lib.newick_rooted(K, names, rec["edge"], rec["distal"])
    row = open(report).read().splitlines()[1].split("\t")
    assert (row[0], int(row[1]), row[2]) == (root, rec["edge"], "%.8g" % rec["distal"])


def test_support_and_transfer_keep_their_labels_and_take_the_lengths(ctx, tmp_path, genomes):
    from andi_amd import lib
    names, files, Ds = genomes
    kinds = ("tree", "support", "transfer", "consensus")
    a = {k: str(tmp_path / ("a_%s.nwk" % k)) for k in kinds}
    b = {k: str(tmp_path / ("b_%s.nwk" % k)) for k in kinds}
    rc0, out0, err0 = _run(["-b", "3"] + ["--%s=%s" % kv for kv in a.items()], files)
    rc1, out1, err1 = _run(["-b", "3", "--lengths=ols"] + ["--%s=%s" % kv for kv in b.items()], files)
    assert (rc0, rc1) == (0, 0) and out0 == out1 and err0 == err1, (err0, err1)
    assert open(a["consensus"]).read() == open(b["consensus"]).read()  # the consensus tree has no matrix: untouched
    J, K, _ = _refit(ctx, Ds[0])
    reps = np.stack([lib.tree(ctx, D, "nj") for D in Ds[1:]])
    support = lib.nj_support(ctx, J, reps)
    assert open(a["support"]).read() == lib.newick(J, names, support=support)
    assert open(b["support"]).read() == lib.newick(K, names, support=support)
    depth, transfer = lib.nj_transfer(ctx, J, reps)
    assert open(a["transfer"]).read() == lib.newick_transfer(J, depth, transfer, 2, names)
    assert open(b["transfer"]).read() == lib.newick_transfer(K, depth, transfer, 2, names)
    want_lengths = _labels_and_lengths(lib.newick(K, names), names)[1]
    for k in ("support", "transfer"):
        la, _ = _labels_and_lengths(open(a[k]).read(), names)
        lb, lengths = _labels_and_lengths(open(b[k]).read(), names)
        assert la == lb and any(la.values()) and lengths == want_lengths
    # with the replicates' lines: each from its own matrix, the same records the counts were taken on
    lines = open(b["tree"]).readlines()
    assert lines == [lib.newick(_refit(ctx, D)[1], names) for D in Ds]


def test_with_complete_the_fit_uses_the_completed_matrix(ctx, tmp_path, holes):
    from andi_amd import lib
    names, files, D = holes
    tree, report = str(tmp_path / "t.nwk"), str(tmp_path / "f.tsv")
    rc, out, err = _run(["--tree=" + tree, "--lengths=ols", "--complete", "--fit=" + report], files)
    rc0, out0, err0 = _run(["--complete", "--tree=" + str(tmp_path / "p.nwk")], files)
    assert rc == rc0 == 1 and out == out0 and err == err0  # (a nan was printed; the fills are named once)
    Cm, _ = lib.complete(ctx, D)
    J, K, res = _refit(ctx, Cm)
    assert open(tree).read() == lib.newick(K, names)
    assert open(report).read() == _report(names, res)
    # without --complete there is no tree to refit and no report
    rc, out, err = _run(["--tree=" + tree, "--lengths=ols", "--fit=" + report], files)
    assert rc == 1 and open(tree).read() == "" and open(report).read() == ""
    assert "No fit report: the distance of 'g0' and 'g2' is not finite." in err
    assert "No tree for matrix 1: the distance of 'g0' and 'g2' is not finite." in err


def test_the_report_is_the_calls_numbers(ctx, tmp_path, genomes):
    names, files, Ds = genomes
    alone, beside, tree = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv"), str(tmp_path / "t.nwk")
    rc0, out0, err0 = _run([], files)
    rc, out, err = _run(["--fit=" + alone], files)
    assert (rc, out, err) == (rc0, out0, err0) and rc == 0
    want = _report(names, _refit(ctx, Ds[0])[2])
    assert open(alone).read() == want
    rc, out, err = _run(["--fit=" + beside, "--tree=" + tree, "-b", "3", "--trees-only"], files)
    assert rc == 0 and open(beside).read() == want and len(open(tree).readlines()) == 3
    rc, out, err = _run(["--fit=" + beside, "--tree-method=bionj", "--lengths=ols"], files)
    assert rc == 0 and out == out0 and open(beside).read() == _report(names, _refit(ctx, Ds[0], "bionj")[2])


def test_joined_and_no_option_are_the_same_bytes(tmp_path, genomes):
    names, files, _ = genomes
    kinds = ("tree", "support", "transfer", "consensus")
    a = {k: str(tmp_path / ("a_%s.nwk" % k)) for k in kinds}
    b = {k: str(tmp_path / ("b_%s.nwk" % k)) for k in kinds}
    rc0, out0, err0 = _run(["-b", "3", "--root=mad"] + ["--%s=%s" % kv for kv in a.items()], files)
    rc1, out1, err1 = _run(["-b", "3", "--root=mad", "--lengths=Joined"] + ["--%s=%s" % kv for kv in b.items()], files)
    assert (rc0, out0, err0) == (rc1, out1, err1) and rc0 == 0
    for k in kinds:
        assert open(a[k]).read() == open(b[k]).read() != "", k
    # without a tree output the option does nothing
    rc2, out2, err2 = _run(["--lengths=ols"], files)
    rc3, out3, err3 = _run([], files)
    assert (rc2, out2, err2) == (rc3, out3, err3) and rc2 == 0


def test_the_refusals(tmp_path, genomes):
    names, files, _ = genomes
    rc, out, err = _run(["--lengths=ols", "--trees-only", "-b", "3", "--tree=" + str(tmp_path / "t.nwk")], files)
    assert rc == 1 and out == b"" and "Branch lengths (--lengths=ols) are not refit together with --trees-only" in err
    rc, out, err = _run(["--lengths=wls", "--tree=" + str(tmp_path / "t.nwk")], files)
    assert rc == 1 and out == b"" and "Expected one of 'joined' or 'ols' for --lengths, but 'wls' was given." in err
    rc, out, err = _run(["--fit=" + str(tmp_path / "f.tsv"), "--reference=" + files[0]], files[1:])
    assert rc == 1 and out == b"" and "A fit report (--fit) is not available together with --reference or --reference-list." in err
