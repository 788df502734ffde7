"""Transfer bootstrap support on the MI355X: andi_hip_nj_transfer against tests/transfer_model.py on hand-made records at
the set-word edges, the tile edges of k_transfer, past one chunk of words and past 64 words; the hand case that pins the cap; equal
topologies; the zero-count cross-check against andi_hip_nj_support on neighbor-joining output; skip, bad records, groups
and chunked calls; and andi-hip -b N --transfer=FILE end to end."""
import os
import subprocess

import numpy as np
import pytest

import consensus_model as cm
import nj_model
import support_model
import transfer_model
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
SKIPPED = transfer_model.SKIPPED


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ hand-made records
def _records(rows, final):
    J = np.zeros(len(rows) + 1, nj_model.NJ_JOIN)
    for s, (a, b) in enumerate(rows):
        J[s] = (a, b, -1, 0, 0.1, 0.1, 0.0)
    J[len(rows)] = tuple(final) + (0, 0.1, 0.1, 0.1)
    return J


def _caterpillar(n, order=None):
    order = list(range(n)) if order is None else order
    rows = [(order[0], order[1])] + [(n + s - 1, order[s + 1]) for s in range(1, n - 3)]
    return _records(rows, (order[n - 2], order[n - 1], n + n - 4))


def _random_tree(n, seed):
    """random joins; the last pair record's node is the final record's third child"""
    rng = np.random.default_rng(seed)
    nodes, rows = list(range(n)), []
    while len(nodes) > 3:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b, a = nodes.pop(j), nodes.pop(i)
        nodes.append(n + len(rows))
        rows.append((a, b))
    return _records(rows, nodes)


def _other_final(J, n):
    """the same unrooted tree with another final three (one leaf set turns into its complement)"""
    K = J.copy()
    x, y, z = (int(J[n - 3][f]) for f in "abc")
    assert z == n + n - 4
    p, q = int(J[n - 4]["a"]), int(J[n - 4]["b"])
    K[n - 4]["a"], K[n - 4]["b"] = x, y
    K[n - 3]["a"], K[n - 3]["b"], K[n - 3]["c"] = p, q, z
    return K


def _moved(J, n, seed, leaves):
    """J with `leaves` of its leaves exchanged with others: a tree a few transfers away"""
    rng = np.random.default_rng(seed)
    perm = np.arange(n)
    for _ in range(leaves):
        i, j = rng.choice(n, 2, replace=False)
        perm[[i, j]] = perm[[j, i]]
    K = J.copy()
    for f in "abc":
        leaf = (K[f] >= 0) & (K[f] < n)
        K[f][leaf] = perm[K[f][leaf]]
    return K


def _replicates(n, count):
    """the tree and count replicates around it: itself, its other writing, near trees, unrelated ones, a caterpillar"""
    tree = _random_tree(n, n)
    kinds = [lambda k: tree, lambda k: _other_final(tree, n) if n > 4 else tree, lambda k: _moved(tree, n, k, 1),
             lambda k: _random_tree(n, n + 1 + k), lambda k: _moved(tree, n, k, max(2, n // 16)), lambda k: _caterpillar(n)]
    return tree, [kinds[k % len(kinds)](k) for k in range(count)]


def _check(ctx, tree, reps, skip=None, numpy=False):
    from andi_amd import lib
    depth, total, per = lib.nj_transfer(ctx, tree, np.stack(reps), skip, per=True)
    assert depth.dtype == np.uint32 and total.dtype == np.uint64 and per.dtype == np.uint32
    want = (transfer_model.transfer_numpy if numpy else transfer_model.transfer)(tree, reps, skip)
    assert depth.tolist() == list(want[0])
    assert per.tolist() == [list(r) for r in want[2]]
    assert total.tolist() == list(want[1])
    d2, t2 = lib.nj_transfer(ctx, tree, np.stack(reps), skip)  # per == NULL: the same sums
    assert d2.tolist() == depth.tolist() and t2.tolist() == total.tolist()
    return depth, total, per


# k_transfer's tiles are TS = TT = 128 sets (of the tree and of the replicate: both dimensions are n - 3), so n - 3 = 127,
# 128, 129 is n = 130, 131, 132; a chunk is WC = 8 words, so W goes from 8 to 9 -- a second chunk, of one word -- at
# n = 513 (checked with the NumPy statement below)
@pytest.mark.parametrize("n", [4, 5, 6, 8, 63, 64, 65, 127, 128, 129, 130, 131, 132, 259, 260])
def test_transfer_matches_the_model(ctx, n):
    tree, reps = _replicates(n, 6)
    depth, total, per = _check(ctx, tree, reps)
    assert (per[0] == 0).all() and (per[1] == 0).all()
    if n >= 63:  # all three regimes occur
        cap = depth[None, :] - 1
        assert (per[2:] == 0).any() and ((per[2:] == cap) & (per[2:] > 0)).any() and ((per[2:] > 0) & (per[2:] < cap)).any()


def test_transfer_300_leaves_5_replicates(ctx):
    tree, reps = _replicates(300, 5)
    _check(ctx, tree, reps)


@pytest.mark.parametrize("n,count", [(513, 3), (1100, 2)])
def test_transfer_past_one_chunk_of_words(ctx, n, count):
    tree = _random_tree(n, n)
    reps = [_moved(tree, n, 1, n // 16), _random_tree(n, n + 1), tree][:count]
    depth, total, per = _check(ctx, tree, reps, numpy=True)
    assert (per[0] > 0).any() and (per[0] == 0).any()


def _far_word_case(n):
    """(tree, replicates, the model's result) for sets of 64, 65 and 66 words: consensus_model.far_word_case's tree, the
    tree `far` that differs from it in the far words alone, and `near` (two leaves of word 0 exchanged) in its other
    writing.  What the input is, from the model: the branches far lacks are at distance 2 from far's nearest branch where
    two leaves were exchanged and 1 where one was moved (n = 4097) -- all of it past bit 4095 (at n = 4096: in word 63),
    so a kernel that dropped those words would give 0."""
    tree, far, near, edge = cm.far_word_case(n)
    reps = [far, _other_final(near, n)]
    want = transfer_model.transfer_numpy(tree, reps)
    depth, total, per = want
    mine, theirs = support_model.leaf_sets(tree, n), set(support_model.leaf_sets(far, n))
    lost = [s for s in range(n - 3) if mine[s] not in theirs]
    away = 1 if n == 4097 else 2
    assert lost and (per[0][lost] > 0).all() and (per[0][lost] == away).any() and per[0].sum() == per[0][lost].sum()
    assert (per[1] > 0).any() and (per[1][lost] == 0).any()  # the control loses other branches
    return tree, reps, want


# W = 64: the last size at which k_depth's lanes take one trip and k_transfer 8 chunks; 65: a ninth chunk of one word, and
# that word holds bit 4096 alone; 66: a ninth chunk of two.  The NumPy statement takes 2 s per size on the host (float32
# products of 4158 x 4161 zeros and ones: sums below 2^24, exact); the device's part is a few milliseconds.
@pytest.mark.parametrize("n", [4096, 4097, 4161])
def test_transfer_past_64_words_of_a_set(ctx, n):
    from andi_amd import lib
    tree, reps, want = _far_word_case(n)
    depth, total, per = lib.nj_transfer(ctx, tree, np.stack(reps), per=True)
    assert depth.tolist() == want[0].tolist() and per.tolist() == want[2].tolist() and total.tolist() == want[1].tolist()
    d2, t2 = lib.nj_transfer(ctx, tree, np.stack(reps))  # per == NULL: the same sums
    assert d2.tolist() == depth.tolist() and t2.tolist() == total.tolist()


def test_transfer_hand_case_pins_the_cap(ctx):
    # branch {0, 1} is 2 away from every branch of the replicate; one of its leaf branches is 1 away
    tree, rep = _caterpillar(8), _caterpillar(8, [0, 2, 3, 4, 5, 6, 7, 1])
    depth, total, per = _check(ctx, tree, [rep])
    assert depth.tolist() == [2, 3, 4, 3, 2] and per.tolist() == [[1, 1, 1, 1, 1]] and total.tolist() == [1, 1, 1, 1, 1]


def test_transfer_of_equal_topologies_is_zero(ctx):
    from andi_amd import lib
    n = 70
    tree = _random_tree(n, 3)
    depth, total, per = _check(ctx, tree, [tree, _other_final(tree, n), tree])
    assert not per.any() and not total.any() and depth.min() >= 2
    # one topology joined in different orders by neighbor-joining itself
    n, count = 60, 4
    D, _, _ = nj_model.additive_tree(n, seed=3)
    J = lib.nj(ctx, D)
    rng = np.random.default_rng(4)
    Ds = []
    for _ in range(count):
        K = J.copy()
        for f in ("la", "lb", "lc"):
            K[f] = rng.uniform(0.01, 0.1, len(K))
        Ds.append(nj_model.patristic(K, n))
    reps, bad = lib.nj_batch(ctx, np.stack(Ds))
    assert (bad == -1).all() and len({tuple(zip(r["a"].tolist(), r["b"].tolist())) for r in reps}) > 1
    depth, total, per = lib.nj_transfer(ctx, J, reps, per=True)
    assert not per.any() and not total.any()


@pytest.mark.parametrize("n,count", [(65, 12), (200, 8)])
def test_zero_transfer_index_is_bootstrap_support(ctx, n, count):
    from andi_amd import lib
    D, _, _ = nj_model.additive_tree(n, seed=n)
    rng = np.random.default_rng(n + 1)
    Ds = []
    for _ in range(count):
        E = np.triu(rng.uniform(-0.15, 0.15, (n, n)), 1)
        Ds.append(D * (1.0 + E + E.T))
    tree = lib.nj(ctx, D)
    reps, bad = lib.nj_batch(ctx, np.stack(Ds))
    assert (bad == -1).all()
    skip = np.zeros(count, np.uint8)
    skip[1] = 1
    for sk in (None, skip):
        depth, total, per = lib.nj_transfer(ctx, tree, reps, sk, per=True)
        support = lib.nj_support(ctx, tree, reps, sk)
        assert (per == 0).sum(0).tolist() == support.tolist()
        assert 0 < support.sum() < (count - (sk is not None)) * (n - 3)  # some branches are lost to the noise, not all
        want = transfer_model.transfer_numpy(tree, list(reps), sk)
        assert per.tolist() == want[2].tolist() and total.tolist() == want[1].tolist() and depth.tolist() == want[0].tolist()


def test_transfer_skip(ctx):
    from andi_amd import lib
    n = 40
    tree, reps = _replicates(n, 6)
    depth, total, per = _check(ctx, tree, reps, skip=[0, 1, 0, 1, 0, 0])
    assert (per[1] == SKIPPED).all() and (per[3] == SKIPPED).all()
    d2, t2, p2 = _check(ctx, tree, [reps[0], reps[2], reps[4], reps[5]])
    assert total.tolist() == t2.tolist() and per[[0, 2, 4, 5]].tolist() == p2.tolist()
    # a skipped replicate's records are not looked at; a used one's are
    garbage = reps[3].copy()
    garbage["a"] = 99999
    d3, t3, p3 = lib.nj_transfer(ctx, tree, np.stack(reps[:3] + [garbage] + reps[4:]), [0, 1, 0, 1, 0, 0], per=True)
    assert t3.tolist() == total.tolist() and p3.tolist() == per.tolist()
    with pytest.raises(lib.AndiHipError, match="replicate 3 are not those of andi_hip_nj"):
        lib.nj_transfer(ctx, tree, np.stack(reps[:3] + [garbage] + reps[4:]), [0, 1, 0, 0, 0, 0])
    with pytest.raises(lib.AndiHipError, match="not those of andi_hip_nj"):
        lib.nj_transfer(ctx, garbage, np.stack(reps))
    # every replicate skipped: zeros, the depths all the same
    d4, t4, p4 = lib.nj_transfer(ctx, tree, np.stack(reps), [1] * 6, per=True)
    assert d4.tolist() == depth.tolist() and not t4.any() and (p4 == SKIPPED).all()
    # n = 3: nothing to write
    d5, t5, p5 = lib.nj_transfer(ctx, tree[:1], np.stack([tree[:1]]), per=True)
    assert d5.size == 0 and t5.size == 0 and p5.shape == (1, 0)


def test_transfer_in_chunks_adds_up(ctx):
    from andi_amd import lib
    n = 65
    tree, reps = _replicates(n, 5)
    depth, total, per = _check(ctx, tree, reps)
    da, ta, pa = lib.nj_transfer(ctx, tree, np.stack(reps[:3]), per=True)
    db, tb, pb = lib.nj_transfer(ctx, tree, np.stack(reps[3:]), per=True)
    assert da.tolist() == db.tolist() == depth.tolist()
    assert (ta + tb).tolist() == total.tolist() and np.concatenate([pa, pb]).tolist() == per.tolist()


def test_transfer_across_a_group_boundary(ctx):
    n = 65
    tree, reps = _replicates(n, 5)
    skip = [0, 0, 0, 1, 0]
    depth, total, per = _check(ctx, tree, reps, skip)
    with knobs(NJ_GROUP=2):  # groups of 2 and 2 of the four used replicates
        d2, t2, p2 = _check(ctx, tree, reps, skip)
    assert d2.tolist() == depth.tolist() and t2.tolist() == total.tolist() and p2.tolist() == per.tolist()


# ------------------------------------------------------------------ end to end
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.mark.timeout(300)
def test_cli_transfer(tmp_path):
    from andi_amd import synth
    n = 6
    seqs, _ = synth.tree_set(n, 20_000, seed=5)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED="11")  # (the same bootstrap matrices in every run)
    paths = {k: tmp_path / (k + ".nwk") for k in ("f", "s", "s2", "f2")}

    def run(args):
        p = subprocess.run([CLI, "-t", "4", "-b", "6"] + args + files, capture_output=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    plain = run(["--support=" + str(paths["s"])])
    assert run(["--transfer=" + str(paths["f"]), "--support=" + str(paths["s2"])]) == plain  # stdout keeps its bytes
    assert paths["s2"].read_bytes() == paths["s"].read_bytes()
    text = paths["f"].read_text()
    assert text.endswith(";\n") and text.count("\n") == 1
    tbe, unlabelled = transfer_model.parse_labels(text)
    counts, _, _ = support_model.parse_labels(paths["s"].read_text())
    assert unlabelled == [] and set(tbe) == set(counts) and len(tbe) == n - 3
    assert transfer_model.strip_labels(text) == transfer_model.strip_labels(paths["s"].read_text())
    used = 5  # -b 6: six matrices, five of them replicates
    for side, v in tbe.items():
        assert 0.0 <= v <= 1.0
        # a replicate that has the branch adds 0 and any other at most depth - 1, so TBE >= c / used; the label is that
        # number rounded to six significant digits
        assert v >= counts[side] / used - 1e-6, (side, v, counts[side])
    # --transfer alone writes the same line
    assert run(["--transfer=" + str(paths["f2"])]) == plain
    assert paths["f2"].read_bytes() == paths["f"].read_bytes()
