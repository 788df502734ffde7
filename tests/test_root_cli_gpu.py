"""andi-hip --root=METHOD end to end on the MI355X: stdout and the exit status keep their bytes; every line of --tree is
rooted and unroots to the line of the run without; the labels of --support and --transfer stay on their branches; -b's
replicates and --trees-only; --root-report against andi_amd.root on the same records."""
import math
import os
import subprocess

import pytest

import root_model as rm
from conftest import ROOT
from newick_reader import parse, splits

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
N = 7


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    from andi_amd import synth
    d = tmp_path_factory.mktemp("root_cli")
    seqs, _ = synth.tree_set(N, 20_000, seed=5)
    names = ["g%d" % k for k in range(N)]
    return names, [_fasta(d / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)], seqs


def _run(args, files):
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED="11")  # (the same bootstrap matrices in every run)
    p = subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def _unrooted(line, names):
    """(splits of the line with the root's two branches merged, the root's two branches): {side: (length, label)}"""
    index = {nm: i for i, nm in enumerate(names)}
    tree = parse(line)
    got = splits(tree, index, len(names), {})
    if len(tree["kids"]) == 3:
        return {s: (float(v[0][0]), v[0][1]) for s, v in got.items()}, None
    assert len(tree["kids"]) == 2
    out, halves = {}, None
    for s, v in got.items():
        if len(v) == 2:  # the two halves of the root's edge
            assert halves is None and len({lab for _, lab in v if lab}) <= 1  # (an inner end carries the edge's label)
            halves = (float(v[0][0]), float(v[1][0]))
            out[s] = (halves[0] + halves[1], v[0][1] or v[1][1])
        else:
            (length, label), = v
            out[s] = (float(length), label)
    assert halves is not None
    return out, halves


def _unit(v):
    """one unit of the eighth significant digit of v"""
    return 0.0 if v == 0 else 10.0 ** (math.floor(math.log10(abs(v))) - 7)


def _same_tree(rooted_line, plain_line, names):
    """the rooted line is rooted, and unrooted it is the plain line: the splits, the labels, the lengths as %.8g prints them"""
    got, halves = _unrooted(rooted_line, names)
    want, none = _unrooted(plain_line, names)
    assert halves is not None and none is None
    assert set(got) == set(want)
    for s in want:
        assert got[s][1] == want[s][1], s
        if got[s][0] == halves[0] + halves[1]:
            # the root's edge: three numbers printed to eight significant digits, each within half a unit of its last one
            assert abs(got[s][0] - want[s][0]) <= 0.5 * (_unit(want[s][0]) + _unit(halves[0]) + _unit(halves[1])) * (1 + 1e-9), s
        else:
            assert got[s][0] == want[s][0], s  # the same text
    return halves


@pytest.mark.parametrize("method", ["mad", "midpoint", "MAD"])
def test_tree_support_and_transfer_are_rooted_and_nothing_else_changes(tmp_path, genomes, method):
    names, files, _ = genomes
    plain = {k: str(tmp_path / ("plain_%s.nwk" % k)) for k in ("tree", "support", "transfer", "consensus")}
    rooted = {k: str(tmp_path / ("rooted_%s.nwk" % k)) for k in ("tree", "support", "transfer", "consensus")}
    report = str(tmp_path / "root.tsv")
    args = lambda o: ["-b", "5"] + ["--%s=%s" % kv for kv in o.items()]
    rc0, out0, err0 = _run(args(plain), files)
    rc1, out1, err1 = _run(args(rooted) + ["--root=" + method, "--root-report=" + report], files)
    assert (rc0, rc1) == (0, 0), (err0, err1)
    assert out1 == out0 and err1 == err0  # stdout, the warnings and the exit status keep their bytes
    assert open(rooted["consensus"]).read() == open(plain["consensus"]).read()  # the consensus tree is not rooted
    lines0, lines1 = open(plain["tree"]).readlines(), open(rooted["tree"]).readlines()
    assert len(lines0) == len(lines1) == 5  # the point estimate and four replicates, each with its own root
    for a, b in zip(lines1, lines0):
        _same_tree(a, b, names)
    for k in ("support", "transfer"):
        (a,), (b,) = open(rooted[k]).readlines(), open(plain[k]).readlines()
        _same_tree(a, b, names)
        assert any(lab for _, lab in _unrooted(b, names)[0].values())
    # the report: the point estimate's root is where the first line of --tree has it
    header, row = open(report).read().splitlines()
    assert header == "#method\tedge\tdistal\tlength\tscore\tambiguity\tpairs"
    got = row.split("\t")
    assert got[0] == method.lower() and int(got[6]) == N * (N - 1) // 2
    halves = _same_tree(lines1[0], lines0[0], names)
    assert float(got[2]) == pytest.approx(halves[0], rel=1e-6, abs=1e-12)
    assert float(got[3]) == pytest.approx(halves[0] + halves[1], rel=1e-6)
    if method.lower() == "mad":
        assert 0.0 <= float(got[4]) < 1.0 and 0.0 <= float(got[5]) <= 1.0
    else:
        assert got[4] == "nan" and got[5] == "nan"


def test_the_report_is_the_library_on_the_same_records(tmp_path, genomes):
    """the same records: those andi_amd.tree gives for the distances the run printed from"""
    from andi_amd import lib
    names, files, seqs = genomes
    tree, report = str(tmp_path / "t.nwk"), str(tmp_path / "r.tsv")
    rc, out, err = _run(["--tree=" + tree, "--root=mad", "--root-report=" + report], files)
    assert rc == 0, err
    M = lib.dist_matrix(seqs, host_threads=4)
    ctx = lib.Context(0)
    try:
        J = lib.tree(ctx, lib.distances(M, lib.M_JC), "nj")
        rec = lib.root(ctx, J, "mad")
    finally:
        ctx.close()
    score, ambiguity = rm.score(rec)
    parent_len = {int(J[s][c]): float(J[s][l]) for s in range(N - 2) for c, l in (("a", "la"), ("b", "lb"), ("c", "lc"))
                  if c != "c" or s == N - 3}
    want = "mad\t%d\t%.8g\t%.8g\t%.8g\t%.8g\t%d" % (rec["edge"], rec["distal"], parent_len[int(rec["edge"])], score, ambiguity,
                                                 rec["pairs"])
    assert open(report).read() == "#method\tedge\tdistal\tlength\tscore\tambiguity\tpairs\n" + want + "\n"
    assert open(tree).read() == lib.newick_rooted(J, names, rec["edge"], rec["distal"])


def test_trees_only_bionj_and_complete(tmp_path, genomes):
    names, files, _ = genomes
    for extra in (["--trees-only"], ["--tree-method=bionj"], ["--complete"]):
        a, b = str(tmp_path / "a.nwk"), str(tmp_path / "b.nwk")
        sa, sb = str(tmp_path / "sa.nwk"), str(tmp_path / "sb.nwk")
        rc0, out0, err0 = _run(["-b", "4", "--tree=" + a, "--support=" + sa] + extra, files)
        rc1, out1, err1 = _run(["-b", "4", "--tree=" + b, "--support=" + sb, "--root=midpoint"] + extra, files)
        assert (rc0, rc1) == (0, 0) and out0 == out1 and err0 == err1, (extra, err0, err1)
        la, lb = open(a).readlines(), open(b).readlines()
        assert len(la) == len(lb) >= 3
        for x, y in zip(lb, la):
            _same_tree(x, y, names)
        _same_tree(open(sb).read(), open(sa).read(), names)


def test_without_a_tree_output_the_option_does_nothing(tmp_path, genomes):
    names, files, _ = genomes
    rc0, out0, err0 = _run([], files)
    rc1, out1, err1 = _run(["--root=mad"], files)
    assert (rc0, out0, err0) == (rc1, out1, err1) and rc0 == 0
