"""The query-versus-reference mode on the device: andi_hip_dist_rect's two cross blocks are those of andi_hip_dist_matrix
over refs ++ queries, bit for bit, on every path of the seam; a few entries against the oracle's dist_anchor; growing a
matrix from its pieces; scans over a column view of a staged set; the command line's --reference table."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")


def _cross_blocks_equal(refs, queries, model=1, **kw):
    from andi_amd import lib
    nr = len(refs)
    M = lib.dist_matrix(list(refs) + list(queries), model=model, host_threads=8)
    MRQ, MQR = lib.dist_rect(refs, queries, model=model, host_threads=8, **kw)
    assert MRQ.shape == (nr, len(queries), 17) and MQR.shape == (len(queries), nr, 17)
    assert (MRQ == M[:nr, nr:]).all()
    assert (MQR == M[nr:, :nr]).all()
    assert lib.last_gather() == "direct"
    return M, MRQ, MQR


@pytest.fixture(scope="module")
def star():
    from andi_amd import synth
    return synth.genome_set(9, 60000, 0.002, 0.06, seed=31)[0]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", [1, 3, 4])  # JC, LogDet, ANI
def test_star_set_every_shape(star, model):
    _cross_blocks_equal(star[:6], star[6:], model)   # nr > nq
    _cross_blocks_equal(star[:2], star[2:], model)   # nq > nr
    _cross_blocks_equal(star[:8], star[8:], model)   # nq = 1
    _cross_blocks_equal(star[:1], star[1:], model)   # nr = 1


@pytest.mark.timeout(600)
def test_tree_realistic_and_joined_contigs():
    from andi_amd import synth
    tree = synth.tree_set(8, 50000, seed=5)
    tree = tree[0] if isinstance(tree, tuple) else tree
    _cross_blocks_equal(tree[:5], tree[5:], 1)
    real = synth.realistic_set(7, 60000, 0.005, 0.05, seed=8)[0]
    _cross_blocks_equal(real[:4], real[4:], 3)
    joined = synth.realistic_set(6, 50000, 0.005, 0.05, seed=9, contigs=5)[0]
    assert all(b"!" in s for s in joined)
    _cross_blocks_equal(joined[:2], joined[2:], 1)
    _cross_blocks_equal(joined[:3], joined[3:], 4)


@pytest.mark.timeout(600)
def test_a_sequence_in_both_sets_is_scanned_not_the_diagonal(star):
    refs, queries = star[:4], [star[2], star[7]]
    M, MRQ, MQR = _cross_blocks_equal(refs, queries, 1)
    # the pair (refs[2], queries[0]) is a real scan of the sequence against itself: its whole length, no mismatch
    n = len(star[2])
    for m in (MRQ[2, 0], MQR[0, 2]):
        assert m[16] == n and m[[0, 5, 10, 15]].sum() == n and m[:16].sum() == n
        assert not (m[0] == 9 and m[16] == 9)  # (not the diagonal placeholder, src/dist_hack.h:61-64)


@pytest.mark.timeout(600)
def test_low_memory_sa_on_host_and_two_contexts_on_one_device(star):
    _cross_blocks_equal(star[:5], star[5:], 1, low_memory=True)
    _cross_blocks_equal(star[:5], star[5:], 3, sa_on_host=True)
    _cross_blocks_equal(star[:5], star[5:], 1, devices=[0, 0])
    _cross_blocks_equal(star[:1], star[1:3], 1, devices=[0, 0])  # (a device without reference rows)


@pytest.mark.timeout(900)
def test_a_call_routed_per_pair():
    """1 Mbp genomes: a batch of 8 query rows against 10 references is 8 x 10 Mbp of query symbols x subjects, above the
    2^25 from which pass A is routed per pair (scan_call.hip: ANDI_ROUTE_TINY_NT)."""
    from andi_amd import synth
    seqs = synth.genome_set(18, 1_000_000, 0.002, 0.03, seed=41)[0]
    assert 8 * 10 * 1_000_000 > 2 ** 25
    _cross_blocks_equal(seqs[:10], seqs[10:], 1)


@pytest.mark.timeout(600)
def test_entries_against_the_oracle(star, orc):
    from andi_amd import lib
    refs, queries = star[:4], star[4:7]
    for model in (1, 3):
        MRQ, MQR = lib.dist_rect(refs, queries, model=model)
        for r, q in ((0, 0), (3, 2), (1, 1)):
            assert (MRQ[r, q] == orc.OracleEsa(refs[r]).dist_anchor(queries[q], model=model)).all(), (model, r, q)
            assert (MQR[q, r] == orc.OracleEsa(queries[q]).dist_anchor(refs[r], model=model)).all(), (model, q, r)


@pytest.mark.timeout(600)
def test_growing_a_matrix_from_its_pieces(star):
    from andi_amd import lib
    old, new = star[:6], star[6:]
    no = len(old)
    whole = lib.dist_matrix(old + new)
    OO = lib.dist_matrix(old)
    MRQ, MQR = lib.dist_rect(old, new)
    NN = lib.dist_matrix(new)
    grown = np.zeros_like(whole)
    grown[:no, :no], grown[:no, no:], grown[no:, :no], grown[no:, no:] = OO, MRQ, MQR, NN
    assert (grown == whole).all()


@pytest.mark.timeout(600)
def test_progress_counts_both_blocks(star):
    from andi_amd import lib
    seen = []
    lib.dist_rect(star[:3], star[3:5], progress=lambda done, total: seen.append((done, total)))
    assert seen and all(t == 2 * 3 * 2 for _, t in seen) and seen[-1][0] == 12


@pytest.mark.timeout(600)
def test_scan_over_a_view_equals_the_columns_of_the_whole_set(ctx, star):
    import andi_amd
    from andi_amd import lib
    subjects = [andi_amd.Esa(ctx, s, sa="device") for s in star[:3]]
    Q = andi_amd.Queries(ctx, star)
    whole = andi_amd.scan_rows(ctx, subjects, [-1, -1, -1], Q, andi_amd.M_JC)
    for a, k in ((3, 4), (0, 2), (8, 1), (1, 8)):
        V = Q.view(a, k)
        assert len(V) == k
        got = andi_amd.scan_rows(ctx, subjects, [-1, -1, -1], V, andi_amd.M_JC)
        assert (got == whole[:, a:a + k]).all(), (a, k)
        V.close()
    # a view of the ranges the square call's rows would scan, with the diagonal: self indexes the view
    V = Q.view(2, 5)
    got = andi_amd.scan_rows(ctx, subjects, [-1, -1, 0], V, andi_amd.M_LOGDET)
    want = andi_amd.scan_rows(ctx, subjects, [-1, -1, 2], Q, andi_amd.M_LOGDET)
    assert (got[:, 1:] == want[:, 3:7]).all() and (got[:2, 0] == want[:2, 2]).all() and (got[2, 0] == want[2, 2]).all()
    V.close()
    with pytest.raises(lib.AndiHipError):
        Q.view(8, 2)
    Q.close()
    for e in subjects:
        e.close()


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.mark.timeout(600)
def test_cli_reference_table_is_a_slice_of_the_square_run(tmp_path, star):
    files = [_fasta(tmp_path / ("g%d.fa" % k), "g%d" % k, s) for k, s in enumerate(star[:7])]
    nr = 4
    env = dict(os.environ, ANDI_HIP_GPUS="1")

    def run(args):
        p = subprocess.run([CLI] + args, capture_output=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.decode()

    for model in ("JC", "LogDet"):
        sq = run(["-v", "-m", model, "-t", "4"] + files).splitlines()
        rect = run(["-v", "-m", model, "-t", "4"] + ["--reference=" + f for f in files[:nr]] + files[nr:]).splitlines()
        n, nq = 7, 3
        assert sq[0] == "7" and rect[0] == "%d %d" % (nq, nr) and rect[1].split() == ["g0", "g1", "g2", "g3"]
        srows = [line.split() for line in sq[1:1 + n]]
        for q in range(nq):
            row = rect[2 + q].split()
            assert row[0] == "g%d" % (nr + q) and row[1:] == srows[nr + q][1:nr + 1], (model, q)
        # the coverage blocks: nq rows of nr values, the slice of the square run's
        sc = sq.index("Coverage:")
        rc = rect.index("Coverage:")
        for q in range(nq):
            assert rect[rc + 1 + q].split() == sq[sc + 1 + nr + q].split()[:nr], (model, q)
