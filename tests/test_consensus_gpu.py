"""The distinct splits of a bootstrap on the MI355X: andi_hip_nj_splits against tests/consensus_model.py -- ids by first
appearance, frequencies and sets, all equal -- on hand-made records (the canonical side, the set-word edges, skip, a
2000-leaf caterpillar against its mirror image) and on andi_hip_nj_batch's output; against andi_hip_nj_support; with
the hash cut short so that collisions are the normal case; on sets of more than 64 words, with and without the hash; across a group boundary; and andi-hip -b N --consensus=FILE
end to end."""
import functools
import os
import subprocess

import numpy as np
import pytest

import consensus_model as cm
import nj_model
import support_model
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _splits(ctx, reps, skip=None):
    from andi_amd import lib
    ids, freq, sets = lib.nj_splits(ctx, np.stack(reps), skip)
    n = len(reps[0]) + 2
    assert ids.dtype == np.uint32 and freq.dtype == np.uint32 and sets.dtype == np.uint64
    assert ids.shape == (len(reps), n - 3) and sets.shape == (len(freq), (n + 63) // 64)
    return ids, freq, sets


def _same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check(ctx, reps, skip=None):
    got = _splits(ctx, reps, skip)
    want = cm.splits(np.stack(reps), skip)
    assert got[0].tolist() == want[0].tolist()
    assert got[1].tolist() == want[1].tolist()
    assert got[2].tolist() == want[2].tolist()
    return got


def _hand_made(n, count):
    tree = cm.random_tree(n, n)
    reps = [tree, cm.random_tree(n, n + 1), cm.other_final(tree, n), cm.caterpillar(n), cm.mirrored_caterpillar(n), tree,
            cm.random_tree(n, n + 2)]
    return {1: reps[:1], 2: [reps[0], reps[2]], 7: reps}[count]


# ------------------------------------------------------------------ exactness and first-appearance order
@pytest.mark.parametrize("count", [1, 2, 7])
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 129])
def test_splits_of_hand_made_records_equal_the_model(ctx, n, count):
    ids, freq, sets = _check(ctx, _hand_made(n, count))
    assert ids[0].tolist() == list(range(n - 3))  # the first replicate's splits come first, in its records' order
    if count > 1:
        assert sorted(ids[1 if count == 2 else 2].tolist()) == list(range(n - 3))  # the same tree with another final three
    if count == 7 and n > 4:
        assert len(freq) >= n - 3 and freq[:n - 3].min() >= 3 and (ids[5] == ids[0]).all()
        assert sorted(ids[3].tolist()) == sorted(ids[4].tolist())  # the caterpillar and its mirror image


def test_a_set_with_leaf_0_and_its_complement_are_one_split(ctx):
    # ((0,1),2,(3,4)) written in two ways: {0,1} and {2,3,4}, and {3,4} in both
    A = cm.records([(0, 1), (3, 4)], (2, 5, 6))
    B = cm.records([(3, 4), (2, 5)], (0, 1, 6))
    ids, freq, sets = _check(ctx, [A, B])
    assert ids.tolist() == [[0, 1], [1, 0]] and freq.tolist() == [2, 2] and sets[:, 0].tolist() == [0b11100, 0b11000]
    ids, freq, sets = _check(ctx, [cm.records([(0, 1)], (2, 3, 4)), cm.records([(2, 3)], (0, 1, 4))])  # four leaves
    assert ids.tolist() == [[0], [0]] and freq.tolist() == [2] and sets.tolist() == [[0b1100]]


def _redrawn(J, n, rng):
    """an additive matrix of J's topology with branch lengths drawn anew"""
    K = J.copy()
    for f in ("la", "lb", "lc"):
        K[f] = rng.uniform(0.01, 0.1, len(K))
    return nj_model.patristic(K, n)


def test_one_topology_joined_in_different_orders_has_the_same_ids(ctx):
    from andi_amd import lib
    n, count = 60, 6
    D, _, _ = nj_model.additive_tree(n, seed=3)
    tree = lib.nj(ctx, D)
    rng = np.random.default_rng(4)
    reps, bad = lib.nj_batch(ctx, np.stack([_redrawn(tree, n, rng) for _ in range(count)]))
    assert (bad == -1).all()
    assert len({tuple(zip(r["a"].tolist(), r["b"].tolist())) for r in reps}) > 1  # the joins do come in different orders
    ids, freq, sets = _check(ctx, list(reps))
    assert len(freq) == n - 3 and (freq == count).all()
    assert all(sorted(row.tolist()) == list(range(n - 3)) for row in ids) and len({tuple(r.tolist()) for r in ids}) > 1


def test_skipped_replicates_are_not_looked_at(ctx):
    n = 40
    tree = cm.random_tree(n, 1)
    garbage = tree.copy()
    garbage["a"] = 99999
    reps = [garbage, cm.random_tree(n, 2), tree, garbage, cm.other_final(tree, n), cm.random_tree(n, 3)]
    skip = [1, 0, 0, 1, 0, 0]
    ids, freq, sets = _check(ctx, reps, skip)
    assert (ids[0] == cm.NONE).all() and (ids[3] == cm.NONE).all() and ids[1].tolist() == list(range(n - 3))
    kept = _splits(ctx, [reps[k] for k in (1, 2, 4, 5)])
    assert _same((ids[[1, 2, 4, 5]], freq, sets), kept)
    ids, freq, sets = _check(ctx, reps[:2], [1, 1])  # nothing left: no split
    assert len(freq) == 0 and (ids == cm.NONE).all()
    from andi_amd import lib
    with pytest.raises(lib.AndiHipError, match="replicate 3 are not those of andi_hip_nj"):
        lib.nj_splits(ctx, np.stack(reps), [1, 0, 0, 0, 0, 0])
    assert lib.nj_splits(ctx, np.stack([tree[:1]]))[1].tolist() == []  # n = 3: nothing to find


def test_a_2000_leaf_caterpillar_and_its_mirror_image(ctx):
    n = 2000
    cat, mirror = cm.caterpillar(n), cm.mirrored_caterpillar(n)
    ids, freq, sets = _check(ctx, [cat, mirror, cat])
    assert len(freq) == n - 3 and (freq == 3).all()
    assert ids[1].tolist() == list(range(n - 4, -1, -1)) and (ids[2] == ids[0]).all()


# ------------------------------------------------------------------ nj_batch's output, and the merged kernels
@pytest.fixture(scope="module")
def noisy(ctx):
    """{n: 20 replicate trees of a noisy additive matrix} from andi_hip_nj_batch"""
    from andi_amd import lib
    out = {}
    for n in (29, 130):
        D, _, _ = nj_model.additive_tree(n, seed=n)
        rng = np.random.default_rng(n + 1)
        Ds = []
        for _ in range(20):
            E = np.triu(rng.uniform(-0.15, 0.15, (n, n)), 1)
            Ds.append(D * (1.0 + E + E.T))
        reps, bad = lib.nj_batch(ctx, np.stack(Ds))
        assert (bad == -1).all()
        out[n] = reps
    return out


@pytest.mark.parametrize("n", [29, 130])
def test_splits_of_noisy_replicates_equal_the_model_and_agree_with_support(ctx, noisy, n):
    from andi_amd import lib
    reps = noisy[n]
    ids, freq, sets = _check(ctx, list(reps))
    assert n - 3 < len(freq) < 20 * (n - 3)  # some branches are lost to the noise, not all
    for k in range(len(reps)):
        assert freq[ids[k]].tolist() == lib.nj_support(ctx, reps[k], reps).tolist(), k
    # and the consensus tree of it: every label a majority, the text the model's
    nodes = lib.consensus(reps, ids, freq, sets)
    assert nodes.tobytes() == cm.consensus(reps, ids, freq, sets).tobytes()
    names = ["t%d" % i for i in range(n)]
    text = lib.newick_consensus(nodes, names)
    assert text == cm.newick_consensus(nodes, names)
    labels, unlabelled, lengths = support_model.parse_labels(text)
    assert unlabelled == [] and len(labels) == len(nodes) - n - 1 > 0 and all(2 * v > 20 for v in labels.values())
    assert sum(len(k) == 1 for k in lengths) == n


# ------------------------------------------------------------------ collisions and groups
def _collision_sets():
    a = [cm.random_tree(12, 1), cm.random_tree(12, 2), cm.other_final(cm.random_tree(12, 1), 12), cm.caterpillar(12),
         cm.random_tree(12, 2), cm.mirrored_caterpillar(12)]
    t = cm.random_tree(65, 9)
    b = [t, cm.random_tree(65, 10), cm.other_final(t, 65), cm.caterpillar(65), t]
    return a, b


@pytest.mark.parametrize("bits", [0, 2])
def test_the_result_does_not_depend_on_the_hash(ctx, bits):
    for reps in _collision_sets():
        want = _check(ctx, reps)
        with knobs(SPLIT_HASH_BITS=bits):  # all sets, or a quarter of them, in one run of equal hashes
            assert _same(_check(ctx, reps), want)
        with knobs(SPLIT_HASH_BITS=bits, NJ_GROUP=2):  # ... and the table's entries too
            assert _same(_check(ctx, reps), want)


@functools.lru_cache(maxsize=None)
def _far_word_case(n):
    """(replicates, the model's splits) for sets of 64, 65, 66 and 129 words, once per n (the model takes 0.3 s at n = 4161
    and 1.4 s at n = 8193 on the host, nearly all of it the words of the distinct sets).  What the input is: the splits
    the replicate `far` lacks and the ones it has in their place are distinct entries of the model's table, some pair of
    them equal in every bit below the far words (consensus_model.far_word_case asserts that there is one), and far's other
    writing -- one set built as its complement -- has far's splits, id for id."""
    tree, far, near, edge = cm.far_word_case(n)
    reps = [tree, far, near, cm.other_final(tree, n), cm.other_final(far, n), cm.caterpillar(n)]
    ids, freq, sets = want = cm.splits(np.stack(reps))
    lost = sorted(set(ids[0].tolist()) - set(ids[1].tolist()))
    new = sorted(set(ids[1].tolist()) - set(ids[0].tolist()))
    words = min(64, sets.shape[1] - 1)
    assert lost and new and any((sets[a, :words] == sets[b, :words]).all() for a in lost for b in new)
    assert ids[4].tolist() == ids[1].tolist() and reps[4].tobytes() != reps[1].tobytes()
    return reps, want


@pytest.mark.parametrize("n", [4096, 4097, 4161, 8193])
def test_splits_past_64_words_of_a_set(ctx, n):
    """k_sets' second block, k_hash's and k_append's second (third) trip, the last word's mask in that trip: the table's
    sets, ids and frequencies equal the model's where two replicates differ in the far words alone."""
    reps, want = _far_word_case(n)
    assert _same(_splits(ctx, reps), want)


@pytest.mark.parametrize("n", [4096, 4097, 4161, 8193])
def test_splits_past_64_words_when_every_hash_collides(ctx, n):
    """ANDI_SPLIT_HASH_BITS=0: every set lies in one run of equal keys, so only wave_same's walk over all W words -- its
    second trip from word 64 on -- keeps the far-swapped sets apart, in k_class and, with ANDI_NJ_GROUP=2 (three groups),
    against the table in k_lookup.  (The model is not run again, so 8193 leaves cost only the device's time here.)"""
    reps, want = _far_word_case(n)
    with knobs(SPLIT_HASH_BITS=0):
        assert _same(_splits(ctx, reps), want)
    with knobs(SPLIT_HASH_BITS=0, NJ_GROUP=2):
        assert _same(_splits(ctx, reps), want)


def test_splits_across_a_group_boundary(ctx):
    _, reps = _collision_sets()
    skip = [0, 0, 0, 1, 0]
    want = _check(ctx, reps, skip)
    for group in (2, 1):
        with knobs(NJ_GROUP=group):
            assert _same(_check(ctx, reps, skip), want)


# ------------------------------------------------------------------ end to end
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


@pytest.mark.timeout(300)
def test_cli_consensus(tmp_path):
    from andi_amd import synth
    n = 6
    seqs, _ = synth.tree_set(n, 20_000, seed=5)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    env = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED="11")  # (the same bootstrap matrices in every run)
    paths = {k: tmp_path / (k + ".nwk") for k in ("c", "t", "s", "c2", "t2", "s2")}

    def run(args):
        p = subprocess.run([CLI, "-t", "4", "-b", "6"] + args + files, capture_output=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    plain = run([])
    assert run(["--consensus=" + str(paths["c"])]) == plain  # stdout is what it is without the option
    text = paths["c"].read_text()
    assert text.endswith(";\n") and text.count("\n") == 1
    labels, unlabelled, lengths = support_model.parse_labels(text)
    assert unlabelled == [] and {k for k in lengths if len(k) == 1} == {frozenset([x]) for x in names}
    assert all(2 * v > 5 for v in labels.values())
    # --tree and --support are what they are without --consensus, and the consensus what it is alone
    run(["--tree=" + str(paths["t"]), "--support=" + str(paths["s"])])
    assert run(["--tree=" + str(paths["t2"]), "--support=" + str(paths["s2"]), "--consensus=" + str(paths["c2"])]) == plain
    assert paths["t2"].read_bytes() == paths["t"].read_bytes() and paths["s2"].read_bytes() == paths["s"].read_bytes()
    assert paths["c2"].read_bytes() == paths["c"].read_bytes()
    # every label is the number of replicate lines of --tree that have the branch, and every majority branch is there
    lines = paths["t"].read_text().splitlines()
    assert len(lines) == 6
    everything = frozenset(names)
    count = {}
    for line in lines[1:]:
        for side in nj_model.parse_newick(line + "\n")[1]:
            side = everything - side if names[0] in side else side
            if 1 < len(side) < n - 1:
                count[side] = count.get(side, 0) + 1
    assert labels == {side: c for side, c in count.items() if 2 * c > 5}
