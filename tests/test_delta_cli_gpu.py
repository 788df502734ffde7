"""andi-hip --delta end to end on the MI355X: six short genomes, two of them from an unrelated base so that some pairs have
no distance.  The file's lines are the NumPy restatement (tests/delta_model.py) of the same run's distances, formatted by
the option's rule; stdout, the tree of --complete and the scores themselves do not depend on one another."""
import os
import subprocess

import numpy as np
import pytest

import delta_model as dm
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
NAMES = ["g%d_a_name_beyond_ten" % k for k in range(6)]  # longer than the ten characters of --truncate-names


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
    P, Q = synth.base_codes(20000, 21), synth.base_codes(20000, 22)
    codes = [mut(P, 0.02, 1), mut(P, 0.03, 2), mut(P, 0.05, 3), np.concatenate([mut(P, 0.01, 5), mut(Q, 0.01, 6)]),
             np.concatenate([mut(P, 0.04, 7), mut(Q, 0.04, 8)]), mut(Q, 0.02, 4)]
    seqs = [synth.to_bytes(c) for c in codes]
    d = tmp_path_factory.mktemp("genomes")
    files = [_fasta(d / ("g%d.fa" % k), NAMES[k], s) for k, s in enumerate(seqs)]
    D = lib.distances(lib.dist_matrix(seqs, host_threads=4), lib.M_JC)
    missing = [(int(i), int(j)) for i, j in np.argwhere(np.triu(~np.isfinite(D), 1))]
    assert missing == [(0, 5), (1, 5), (2, 5)], missing  # the recipe: the last genome shares nothing with the first three
    return files, D


def _lines(D, names):
    rec = dm.scores(D)
    out = ["#name\tdelta\tquartets"]
    for name, r in zip(names, rec):
        q, s = int(r["quartets"]), int(r["sum"])
        out.append("%s\t%s\t%d" % (name, "%.6f" % (s / (q * float(1 << 24))) if q else "nan", q))
    Q, S = int(rec["quartets"].sum()), int(rec["sum"].sum())
    out.append("#mean\t%s\t%d" % ("%.6f" % (S / (Q * float(1 << 24))) if Q else "nan", Q // 4))
    return out


def _run(files, args):
    e = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED="4711")
    e.pop("ANDI_HIP_BOOT_CHUNK", None)
    return subprocess.run([CLI, "-t", "4"] + args + files, capture_output=True, timeout=120, env=e)


def test_the_file_is_the_model_of_the_printed_distances(tmp_path, genomes):
    files, D = genomes
    want = _lines(D, NAMES)
    assert want[-1].endswith("\t5") and "nan" not in want[-1]  # of the 15 quartets, the 5 without the last genome are used
    assert want[6].endswith("\tnan\t0")
    plain = _run(files, [])
    p = _run(files, ["--delta=%s" % (tmp_path / "d.tsv")])
    assert p.returncode == plain.returncode and p.stdout == plain.stdout
    assert open(tmp_path / "d.tsv").read().splitlines() == want
    # with -b: the point estimate alone is scored
    plain = _run(files, ["-b", "3"])
    p = _run(files, ["-b", "3", "--delta=%s" % (tmp_path / "b.tsv")])
    assert p.stdout == plain.stdout and open(tmp_path / "b.tsv").read().splitlines() == want


def test_complete_does_not_change_the_scores_nor_they_the_tree(tmp_path, genomes):
    files, D = genomes
    base = _run(files, ["--complete", "--tree=%s" % (tmp_path / "t0.nwk")])
    p = _run(files, ["--complete", "--tree=%s" % (tmp_path / "t1.nwk"), "--delta=%s" % (tmp_path / "d.tsv")])
    assert p.stdout == base.stdout and p.returncode == base.returncode
    tree = open(tmp_path / "t1.nwk").read()
    assert tree == open(tmp_path / "t0.nwk").read() and tree.startswith("(") and tree.count(";") == 1
    assert open(tmp_path / "d.tsv").read().splitlines() == _lines(D, NAMES)


def test_names_are_cut_as_the_matrix_cuts_them(tmp_path, genomes):
    files, D = genomes
    p = _run(files, ["--truncate-names", "--delta=%s" % (tmp_path / "d.tsv")])
    printed = [l.split()[0] for l in p.stdout.decode().splitlines()[1:]]
    assert printed == [nm[:10] for nm in NAMES]
    assert open(tmp_path / "d.tsv").read().splitlines() == _lines(D, printed)
