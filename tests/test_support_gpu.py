"""Bootstrap support on the MI355X: andi_hip_nj_batch bit for bit against andi_hip_nj per matrix (and tests/nj_model.py)
at the tile edges, past 1024 active nodes, on ties, with bad matrices and across a group boundary; andi_hip_nj_support
against tests/support_model.py on hand-made records (the canonical side, the set-word edges, a 2000-leaf caterpillar,
sets of more than 64 words, skip) and on neighbor-joining output; and andi-hip -b N --support=FILE end to end."""
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


def _sym(rng, n, lo=0.0, hi=1.0):
    A = rng.uniform(lo, hi, (n, n))
    return np.triu(A, 1) + np.triu(A, 1).T


def _singles(ctx, Ds):
    from andi_amd import lib
    return np.stack([lib.nj(ctx, D) for D in Ds])


# ------------------------------------------------------------------ the batch against single calls
@pytest.mark.parametrize("count", [1, 2, 7])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 129])
def test_batch_equals_single_calls_and_the_model(ctx, n, count):
    from andi_amd import lib
    rng = np.random.default_rng(100 * n + count)
    Ds = np.stack([_sym(rng, n) for _ in range(count)])
    if count > 1:  # the lower triangle and the diagonal are not read
        Ds[1] = Ds[1] + np.tril(rng.uniform(-5, 5, (n, n)))
    J, bad = lib.nj_batch(ctx, Ds)
    assert J.shape == (count, 1 if n == 2 else n - 2) and (bad == -1).all()
    assert J.tobytes() == _singles(ctx, Ds).tobytes()
    assert J.tobytes() == np.stack([nj_model.nj(D) for D in Ds]).tobytes()


def test_batch_past_1024_active_nodes(ctx):
    # r > 1024 for the first steps: k_nj_rowsum's second pass and k_nj_join's strided loops, per replicate
    from andi_amd import lib
    rng = np.random.default_rng(1030)
    Ds = np.stack([_sym(rng, 1030) for _ in range(3)])
    J, bad = lib.nj_batch(ctx, Ds)
    assert (bad == -1).all() and J.tobytes() == _singles(ctx, Ds).tobytes()


def test_batch_with_ties_and_equal_matrices(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(6)
    n = 70
    Ds = np.stack([np.triu(rng.integers(0, 4, (n, n)).astype(float), 1) for _ in range(5)])  # ties everywhere
    Ds = Ds + Ds.transpose(0, 2, 1)
    J, bad = lib.nj_batch(ctx, Ds)
    assert (bad == -1).all() and J.tobytes() == _singles(ctx, Ds).tobytes()
    assert J.tobytes() == np.stack([nj_model.nj(D) for D in Ds]).tobytes()
    same = np.stack([_sym(rng, 66)] * 4)
    J, bad = lib.nj_batch(ctx, same)
    assert (bad == -1).all() and all(J[k].tobytes() == J[0].tobytes() for k in range(4))
    assert J[0].tobytes() == lib.nj(ctx, same[0]).tobytes()


def test_batch_with_bad_matrices(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(7)
    n = 20
    Ds = np.stack([_sym(rng, n) for _ in range(5)])
    Ds[2, 1, 3] = np.nan
    Ds[2, 9, 12] = np.inf  # (a later one: the first counts)
    Ds[4, 0, 1] = np.inf
    Ds[0, 5, 2] = np.nan   # the lower triangle is not read
    J, bad = lib.nj_batch(ctx, Ds)
    assert bad.tolist() == [-1, -1, 1 * n + 3, -1, 1]
    for k in (2, 4):
        assert J[k].tobytes() == bytes(J[k].nbytes)
    for k in (0, 1, 3):
        assert J[k].tobytes() == lib.nj(ctx, Ds[k]).tobytes()
    # every matrix bad
    J, bad = lib.nj_batch(ctx, Ds[[2, 4]])
    assert bad.tolist() == [n + 3, 1] and J.tobytes() == bytes(J.nbytes)


def test_batch_across_a_group_boundary(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(8)
    Ds = np.stack([_sym(rng, 65) for _ in range(5)])
    Ds[3, 2, 64] = np.nan
    want, want_bad = lib.nj_batch(ctx, Ds)
    with knobs(NJ_GROUP=2):  # groups of 2, 2 and 1
        J, bad = lib.nj_batch(ctx, Ds)
    assert bad.tolist() == want_bad.tolist() == [-1, -1, -1, 2 * 65 + 64, -1]
    assert J.tobytes() == want.tobytes()
    good = [0, 1, 2, 4]
    assert J[good].tobytes() == _singles(ctx, Ds[good]).tobytes()


# ------------------------------------------------------------------ support on hand-made records
def _records(rows, final):
    J = np.zeros(len(rows) + 1, nj_model.NJ_JOIN)
    for s, (a, b) in enumerate(rows):
        J[s] = (a, b, -1, 0, 0.1, 0.1, 0.0)
    J[len(rows)] = tuple(final) + (0, 0.1, 0.1, 0.1)
    return J


def _caterpillar(n):
    return _records([(0, 1)] + [(n + s - 1, s + 1) for s in range(1, n - 3)], (n - 2, n - 1, n + n - 4))


def _balanced(n):
    queue, rows = list(range(n)), []
    while len(queue) > 3:
        a, b = queue.pop(0), queue.pop(0)
        queue.append(n + len(rows))
        rows.append((a, b))
    return _records(rows, queue)


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
    """the same unrooted tree with another final three: final (x, y, z), z the last pair record (p, q), becomes a pair
    record (x, y) and the final (p, q, that node) -- so one leaf set turns into its complement"""
    K = J.copy()
    x, y, z = (int(J[n - 3][f]) for f in "abc")
    assert z == n + n - 4
    p, q = int(J[n - 4]["a"]), int(J[n - 4]["b"])
    K[n - 4]["a"], K[n - 4]["b"] = x, y
    K[n - 3]["a"], K[n - 3]["b"], K[n - 3]["c"] = p, q, z
    return K


def _check(ctx, tree, reps, skip=None):
    from andi_amd import lib
    got = lib.nj_support(ctx, tree, np.stack(reps), skip)
    assert got.dtype == np.uint32 and got.tolist() == support_model.support(tree, reps, skip)
    return got.tolist()


def test_support_counts_unordered_bipartitions(ctx):
    # ((0,1),2,(3,4)) written in two ways; without the canonical side {0,1,2} and {3,4} would not meet
    A = _records([(0, 1), (3, 4)], (2, 5, 6))
    B = _records([(0, 1), (2, 5)], (3, 4, 6))
    assert _check(ctx, A, [B]) == [1, 1]
    assert _check(ctx, B, [A]) == [1, 1]
    assert _check(ctx, A, [A, B, B]) == [3, 3]
    C = _records([(0, 2), (3, 4)], (1, 5, 6))  # another tree: only {3,4} is shared
    assert _check(ctx, A, [C, B]) == [1, 2]
    assert _check(ctx, _records([(0, 1)], (2, 3, 4)), [_records([(2, 3)], (0, 1, 4))]) == [1]  # four leaves, one branch


def test_support_of_a_2000_leaf_caterpillar(ctx):
    n = 2000
    cat, bal = _caterpillar(n), _balanced(n)
    assert _check(ctx, cat, [cat]) == [1] * (n - 3)
    got = _check(ctx, cat, [bal, cat, bal])
    assert got[0] == 3 and min(got) == 1  # (the cherry (0,1) is in both trees)
    assert sum(_check(ctx, bal, [cat])) < n - 3


@pytest.mark.parametrize("n", [33, 64, 65, 129])
def test_support_at_the_set_word_edges(ctx, n):
    tree = _random_tree(n, n)
    reps = [tree, _other_final(tree, n), _random_tree(n, n + 1), _caterpillar(n), _other_final(_caterpillar(n), n)]
    assert _check(ctx, tree, reps)[-1] >= 2
    assert _check(ctx, _caterpillar(n), reps) [0] >= 2
    assert _check(ctx, _other_final(tree, n), [tree]) == [1] * (n - 3)


def _far_word_case(n):
    """(tree, far, replicates) for sets of 64, 65, 66 and 129 words.  The replicate `far` differs from the tree in the far
    words alone (consensus_model.far_word_case, asserted there on Python ints); what follows from it, from the model: far
    lacks some of the tree's splits, the control `near` (two leaves of word 0 exchanged) lacks others, so among the
    replicates a split far lacks counts 3 (or 2), one near lacks 4, every other 5."""
    tree, far, near, edge = cm.far_word_case(n)
    assert tree.tobytes() == _random_tree(n, n).tobytes()
    reps = [tree, far, near, _other_final(tree, n), _other_final(far, n), _caterpillar(n)]
    of_far, of_near = support_model.support(tree, [far]), support_model.support(tree, [near])
    assert 0 in of_far and 0 in of_near and of_far != of_near and support_model.support(tree, [tree]) == [1] * (n - 3)
    want = support_model.support(tree, reps)
    assert max(want) == 5 and 3 in want and 4 in want and all((v <= 3) == (f == 0) for v, f in zip(want, of_far))
    return tree, far, reps


@pytest.mark.parametrize("n", [4096, 4097, 4161, 8193])
def test_support_past_64_words_of_a_set(ctx, n):
    """W = 64, 65, 66, 129 words: k_sets' second block, the second (third) trip of k_hash's lane-strided loop, k_match past
    word 63, and canonical_word's mask on a last word that lies in that trip (n = 4097: bit 0 of word 64 alone).  A
    count that ignored the far words would be 5 where the model says 3."""
    tree, far, reps = _far_word_case(n)
    _check(ctx, tree, reps)
    # the complement's side: in _other_final(far) one set is built as the other side, so its canonical side is taken
    # through the last word's mask; every split of far is found in it and the other way round
    assert _check(ctx, far, [_other_final(far, n)]) == [1] * (n - 3)
    assert _check(ctx, _other_final(far, n), [far, tree]) == [1 + v for v in support_model.support(_other_final(far, n), [tree])]


def test_support_skip_and_a_single_replicate(ctx):
    n = 40
    tree = _random_tree(n, 1)
    reps = [_random_tree(n, 2), tree, _other_final(tree, n), _random_tree(n, 3)]
    assert _check(ctx, tree, reps[:1]) == support_model.support(tree, reps[:1])
    assert _check(ctx, tree, reps, skip=[0, 1, 0, 1]) == _check(ctx, tree, [reps[0], reps[2]])
    assert _check(ctx, tree, reps, skip=[1, 1, 1, 1]) == [0] * (n - 3)
    garbage = reps[0].copy()
    garbage["a"] = 99999  # a skipped replicate's records are not looked at
    assert _check(ctx, tree, [tree, garbage], skip=[0, 1]) == [1] * (n - 3)


def test_support_refuses_records_that_are_no_tree(ctx):
    from andi_amd import lib
    n = 12
    tree = _random_tree(n, 5)
    twice = tree.copy()
    twice["b"][3] = twice["b"][2]  # a node that is a child twice (and one that is none)
    late = tree.copy()
    late["a"][0] = n + 4  # a node no earlier record made
    for bad in (twice, late):
        with pytest.raises(lib.AndiHipError, match="not those of andi_hip_nj"):
            lib.nj_support(ctx, tree, np.stack([tree, bad]))
        with pytest.raises(lib.AndiHipError, match="not those of andi_hip_nj"):
            lib.nj_support(ctx, bad, np.stack([tree]))
    assert lib.nj_support(ctx, tree[:1], np.stack([tree[:1]])).tolist() == []  # n = 3: nothing to count


def test_support_across_a_group_boundary(ctx):
    n = 65
    tree = _random_tree(n, 9)
    reps = [tree, _random_tree(n, 10), _other_final(tree, n), _caterpillar(n), tree]
    want = _check(ctx, tree, reps, skip=[0, 0, 0, 1, 0])
    with knobs(NJ_GROUP=2):
        assert _check(ctx, tree, reps, skip=[0, 0, 0, 1, 0]) == want


# ------------------------------------------------------------------ support on neighbor-joining output
def _redrawn(J, n, rng):
    """an additive matrix of J's topology with branch lengths drawn anew"""
    K = J.copy()
    for f in ("la", "lb", "lc"):
        K[f] = rng.uniform(0.01, 0.1, len(K))
    return nj_model.patristic(K, n)


def test_support_of_one_topology_joined_in_different_orders(ctx):
    from andi_amd import lib
    n, count = 60, 6
    D, _, _ = nj_model.additive_tree(n, seed=3)
    tree = lib.nj(ctx, D)
    rng = np.random.default_rng(4)
    reps, bad = lib.nj_batch(ctx, np.stack([_redrawn(tree, n, rng) for _ in range(count)]))
    assert (bad == -1).all()
    orders = {tuple(zip(r["a"].tolist(), r["b"].tolist())) for r in reps}
    assert len(orders) > 1  # the joins do come in different orders
    assert lib.nj_support(ctx, tree, reps).tolist() == [count] * (n - 3)


def test_support_of_noisy_replicates_matches_the_model(ctx):
    from andi_amd import lib
    n, count = 100, 20
    D, _, _ = nj_model.additive_tree(n, seed=5)
    rng = np.random.default_rng(6)
    Ds = []
    for _ in range(count):
        E = np.triu(rng.uniform(-0.15, 0.15, (n, n)), 1)
        Ds.append(D * (1.0 + E + E.T))
    tree = lib.nj(ctx, D)
    reps, bad = lib.nj_batch(ctx, np.stack(Ds))
    got = lib.nj_support(ctx, tree, reps).tolist()
    assert got == support_model.support(tree, list(reps))
    assert 0 < sum(got) < count * (n - 3)  # some branches are lost to the noise, not all


# ------------------------------------------------------------------ end to end
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


def _matrices(stdout):
    """the PHYLIP matrices of andi-hip's stdout, as lists of lines"""
    lines = stdout.decode().splitlines()
    out, pos = [], 0
    while pos < len(lines) and lines[pos].strip().isdigit():
        n = int(lines[pos])
        out.append(lines[pos:pos + n + 1])
        pos += n + 1
    assert pos == len(lines)
    return out


@pytest.mark.timeout(300)
def test_cli_support(tmp_path):
    from andi_amd import synth
    n = 4
    seqs, _ = synth.tree_set(n, 30_000, seed=5)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]
    env = dict(os.environ, ANDI_HIP_GPUS="1")
    sup, tree = tmp_path / "s.nwk", tmp_path / "t.nwk"

    def run(args):
        p = subprocess.run([CLI, "-t", "4", "-b", "5"] + args + files, capture_output=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    plain = _matrices(run([]))
    out = _matrices(run(["--support=" + str(sup), "--tree=" + str(tree)]))
    # stdout is what it is without --support (the bootstrap is seeded from the clock: the first matrix, the number of them)
    assert len(out) == len(plain) == 5 and out[0] == plain[0]
    lines = tree.read_text().splitlines()
    text = sup.read_text()
    assert len(lines) == 5 and text.endswith(";\n") and text.count("\n") == 1  # -b 5: five matrices, four of them replicates
    labels, unlabelled, lengths = support_model.parse_labels(text)
    _, _, plain_lengths = support_model.parse_labels(lines[0])
    assert lengths == plain_lengths and len(lengths) == n + (n - 3)  # the topology and lengths of --tree's first line
    assert len(labels) == n - 3 and unlabelled == []
    # every label is the number of replicate lines that have the branch
    everything = frozenset(names)
    for side, label in labels.items():
        have = 0
        for line in lines[1:]:
            splits = nj_model.parse_newick(line + "\n")[1]
            have += side in splits or (everything - side) in splits
        assert label == have, (side, label, have)
    # --support alone writes the same kind of line, and --tree alone is unchanged by this option
    run(["--support=" + str(sup)])
    assert set(support_model.parse_labels(sup.read_text())[2]) == set(lengths)
