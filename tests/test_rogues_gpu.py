"""The rogue genomes of a bootstrap on the MI355X: andi_hip_nj_transfer_taxa against tests/rogue_model.py on hand-made
records at the set-word edges, the tile edges of k_nearest, past one chunk of words and past 64 words; the hand case that
pins the tie rule; a planted rogue; the relations to andi_hip_nj_transfer and andi_hip_nj_support; skip, bad records,
groups and chunked calls; and andi-hip -b N --rogues=FILE end to end."""
import os
import subprocess

import numpy as np
import pytest

import consensus_model as cm
import rogue_model as rm
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
SKIPPED = rm.SKIPPED
CUTOFFS = (0.0, 0.3, 1.0)


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _check(ctx, tree, reps, want, skip=None, cutoff=0.3):
    """the library's (moved, pairs, match, dist) are the model's `want`; the call without the detail gives the same sums"""
    from andi_amd import lib
    moved, pairs, match, dist = lib.nj_transfer_taxa(ctx, tree, np.stack(reps), skip, cutoff, detail=True)
    assert moved.dtype == np.uint64 and match.dtype == np.uint32 and dist.dtype == np.uint32 and isinstance(pairs, int)
    assert dist.tolist() == [list(r) for r in want[3]]
    assert match.tolist() == [list(r) for r in want[2]]
    assert moved.tolist() == list(want[0]) and pairs == want[1]
    m2, p2 = lib.nj_transfer_taxa(ctx, tree, np.stack(reps), skip, cutoff)  # match == dist == NULL
    assert m2.tolist() == moved.tolist() and p2 == pairs
    return moved, pairs, match, dist


_near = {}


def _case(n):
    """the recipe's tree and replicates at n leaves and the model's nearest records (shared by the cutoffs)"""
    if n not in _near:
        tree, reps = rm.replicates(n)
        _near[n] = (tree, reps, rm.nearest_all(tree, reps))
    return _near[n]


# k_nearest's tiles are 128 sets of the tree and of the replicate (both dimensions are n - 3), so n - 3 = 127, 128, 129 is
# n = 130, 131, 132; k_moved takes a replicate's pairs 64 at a time (a second trip from n = 68); a set's last word is full
# at n = 64 and 128
@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("n", [4, 5, 6, 8, 63, 64, 65, 127, 128, 129, 130, 131, 132, 259, 260])
def test_taxa_match_the_model(ctx, n, cutoff):
    from andi_amd import lib
    tree, reps, near = _case(n)
    want = rm.taxa(tree, reps, cutoff=cutoff, near=near)
    if n >= 8 and cutoff == 1.0:  # the tie rule and the complement (with the last word's mask) decide counted pairs
        ties, flips = rm.ties_and_flips(tree, reps, cutoff)
        assert ties > 0 and flips > 0
    moved, pairs, match, dist = _check(ctx, tree, reps, want, cutoff=cutoff)
    depth, _, per = lib.nj_transfer(ctx, tree, np.stack(reps), per=True)
    assert np.minimum(dist, depth[None, :] - 1).tolist() == per.tolist()
    on = dist <= np.array([rm.limit(cutoff, d) for d in depth])[None, :]
    assert pairs == int(on.sum()) and int(moved.sum()) == int(dist[on].sum())
    if cutoff == 0.0:
        assert not moved.any() and pairs == int(lib.nj_support(ctx, tree, np.stack(reps)).sum())


# a chunk is 8 words, so W goes from 8 to 9 -- a second chunk of k_nearest, of one word, and a second block of k_moved's
# words -- at n = 513
@pytest.mark.parametrize("n,count", [(513, 3), (1100, 2)])
def test_taxa_past_one_chunk_of_words(ctx, n, count):
    tree = rm.random_tree(n, n)
    reps = [rm.other_final(rm.exchanged(tree, n, 1, n // 16), n), rm.random_tree(n, n + 1), tree][:count]
    want = rm.taxa_numpy(tree, reps, cutoff=1.0)
    assert want[0][512:].any() and want[1] > 0
    moved, pairs, match, dist = _check(ctx, tree, reps, want, cutoff=1.0)
    assert (dist[0] > 0).any() and (dist[0] == 0).any()


# W = 64: the last size at which k_limit's lanes take one trip and k_nearest 8 chunks; 65: a ninth chunk of one word, a
# second trip of k_limit's lane 0, and that word holds bit 4096 alone.  At cutoff 1 no limit of this case hangs on leaf
# 4096; at 0.5 one does, so that cutoff is run as well
@pytest.mark.parametrize("n,cutoff", [(4096, 1.0), (4097, 1.0), (4097, 0.5)])
def test_taxa_past_64_words_of_a_set(ctx, n, cutoff):
    from transfer_model import bit_matrix
    tree, far, near, edge = cm.far_word_case(n)
    # from the model: the leaves that far moves lie in the far words alone (at n = 4096: in word 63)
    alone = rm.taxa_numpy(tree, [far], cutoff=cutoff)
    assert alone[0][edge:].any() and not alone[0][:edge].any() and alone[1] > 0
    reps = [far, rm.other_final(near, n)]
    want = rm.taxa_numpy(tree, reps, cutoff=cutoff)
    assert want[0][:64].any()  # the control moves leaves of word 0
    if cutoff == 0.5:  # depths counted without the word past the first 64 would count other pairs
        low = bit_matrix(tree, n)[:, :4096].sum(1)
        short = np.array([rm.limit(cutoff, d) for d in np.minimum(low, n - low)])
        assert int((want[3] <= short[None, :]).sum()) != want[1]
    _check(ctx, tree, reps, want, cutoff=cutoff)


def test_taxa_hand_case_pins_the_tie(ctx):
    # the caterpillar 0 ... 7 against a replicate with the leaf sets {0, 5}, {0, 2, 5}, {6, 7}, {1, 3}, {0, 1, 2, 3, 5}.
    # Branch {0, 1, 2} (s = 1, depth 3, so counted up to 2) is 2 away from the replicate's {0, 2, 5} (t = 1: the leaves 1
    # and 5 move) and from its {0, 1, 2, 3, 5} (t = 4: the leaves 3 and 5): the least t is 1, and moved[1] = 1, moved[3] =
    # 0 say so.  Branch {0, 1} (s = 0) is tied as well, between t = 0 and t = 3, but at depth 2 a distance of 2 does not
    # count.  {0, 1, 2, 3} is 1 from t = 4, {0 ... 4} is 1 from t = 2 = {6, 7} on its far side (flip), {0 ... 5} is {6, 7}.
    tree = rm.caterpillar(8)
    rep = rm.records([(0, 5), (2, 8), (6, 7), (1, 3), (9, 11)], (4, 10, 12))
    want = rm.taxa(tree, [rep], cutoff=1.0)
    assert want == ([0, 1, 0, 0, 0, 3, 0, 0], 4, [[0, 1, 4, 2, 2]], [[2, 2, 1, 1, 0]])
    ties, _ = rm.ties_and_flips(tree, [rep], 1.0)
    assert ties > 0
    moved, pairs, match, dist = _check(ctx, tree, [rep], want, cutoff=1.0)
    assert match.tolist() == [[0, 1, 4, 2, 2]] and moved.tolist() == [0, 1, 0, 0, 0, 3, 0, 0] and pairs == 4


@pytest.mark.parametrize("cutoff,first,second", [(0.3, 46, 10), (1.0, 63, 13)])
def test_a_planted_rogue_stands_out(ctx, cutoff, first, second):
    n = 130
    tree = rm.random_tree(n, n)
    reps = [rm.swapped(tree, n, 7, other) for other in (10, 20, 30, 40, 50, 60)]
    want = rm.taxa_numpy(tree, reps, cutoff=cutoff)
    order = np.sort(want[0])[::-1]
    assert int(want[0].argmax()) == 7 and (int(order[0]), int(order[1])) == (first, second) and first > 2 * second
    moved, _, _, _ = _check(ctx, tree, reps, want, cutoff=cutoff)
    assert int(moved.argmax()) == 7 and int(moved[7]) > 2 * int(np.sort(moved)[-2])


def test_taxa_skip(ctx):
    from andi_amd import lib
    n = 40
    tree, reps = rm.replicates(n)
    skip = [0, 1, 0, 1, 0, 0, 0, 1]
    want = rm.taxa(tree, reps, skip, 1.0)
    moved, pairs, match, dist = _check(ctx, tree, reps, want, skip, 1.0)
    assert (match[[1, 3, 7]] == SKIPPED).all() and (dist[[1, 3, 7]] == SKIPPED).all() and pairs > 0 and moved.any()
    # a skipped replicate's records are not looked at; a used one's are
    garbage = reps[3].copy()
    garbage["a"] = 99999
    m3, p3, t3, d3 = lib.nj_transfer_taxa(ctx, tree, np.stack(reps[:3] + [garbage] + reps[4:]), skip, 1.0, detail=True)
    assert m3.tolist() == moved.tolist() and p3 == pairs and t3.tolist() == match.tolist() and d3.tolist() == dist.tolist()
    with pytest.raises(lib.AndiHipError, match="replicate 3 are not those of andi_hip_nj"):
        lib.nj_transfer_taxa(ctx, tree, np.stack(reps[:3] + [garbage] + reps[4:]), [0, 1, 0, 0, 0, 0, 0, 1], 1.0)
    with pytest.raises(lib.AndiHipError, match="not those of andi_hip_nj"):
        lib.nj_transfer_taxa(ctx, garbage, np.stack(reps))
    # every replicate skipped: zeros, and the rows say so
    m4, p4, t4, d4 = lib.nj_transfer_taxa(ctx, tree, np.stack(reps), [1] * 8, 1.0, detail=True)
    assert not m4.any() and p4 == 0 and (t4 == SKIPPED).all() and (d4 == SKIPPED).all() and t4.shape == (8, n - 3)
    # n = 3: zeros, nothing else to write
    m5, p5, t5, d5 = lib.nj_transfer_taxa(ctx, tree[:1], np.stack([tree[:1]]), detail=True)
    assert m5.tolist() == [0, 0, 0] and p5 == 0 and t5.shape == d5.shape == (1, 0)
    # a cutoff outside [0, 1] is refused
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(lib.AndiHipError, match="bad arguments"):
            lib.nj_transfer_taxa(ctx, tree, np.stack(reps), cutoff=bad)


def test_taxa_in_chunks_add_up(ctx):
    from andi_amd import lib
    n = 65
    tree, reps, near = _case(n)
    moved, pairs, match, dist = _check(ctx, tree, reps, rm.taxa(tree, reps, cutoff=1.0, near=near), cutoff=1.0)
    ma, pa, ta, da = lib.nj_transfer_taxa(ctx, tree, np.stack(reps[:3]), cutoff=1.0, detail=True)
    mb, pb, tb, db = lib.nj_transfer_taxa(ctx, tree, np.stack(reps[3:]), cutoff=1.0, detail=True)
    assert (ma + mb).tolist() == moved.tolist() and pa + pb == pairs and 0 < pa < pairs
    assert np.concatenate([ta, tb]).tolist() == match.tolist() and np.concatenate([da, db]).tolist() == dist.tolist()


def test_taxa_across_a_group_boundary(ctx):
    n = 65
    tree, reps, _ = _case(n)
    skip = [0, 0, 0, 1, 0, 0, 0, 0]
    want = rm.taxa(tree, reps, skip, 1.0)
    _check(ctx, tree, reps, want, skip, 1.0)
    with knobs(NJ_GROUP=2):  # groups of 2, 2, 2 and 1 of the seven used replicates
        _check(ctx, tree, reps, want, skip, 1.0)


# ------------------------------------------------------------------ end to end
SEED = 7  # with these genomes: a genome that moves in three pairs, one in one, and a pair past the cutoff


def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


def _table(names, moved, pairs):
    return "#name\tmoved\tindex\n" + "".join(
        "%s\t%d\t%s\n" % (name, int(m), "%.6g" % (int(m) / pairs) if pairs else "0") for name, m in zip(names, moved))


@pytest.mark.timeout(300)
def test_cli_rogues(tmp_path):
    from andi_amd import lib, synth
    n = 8
    seqs, _ = synth.tree_set(n, 5000, seed=2)
    names = ["g%d" % k for k in range(n)]
    files = [_fasta(tmp_path / ("%s.fa" % names[k]), names[k], s) for k, s in enumerate(seqs)]

    def run(args, env=None):
        e = dict(os.environ, ANDI_HIP_GPUS="1", ANDI_HIP_SEED=str(SEED))
        e.pop("ANDI_HIP_BOOT_CHUNK", None)
        e.update(env or {})
        p = subprocess.run([CLI, "-t", "4", "-b", "6"] + args + files, capture_output=True, timeout=120, env=e)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    t = {k: str(tmp_path / (k + ".nwk")) for k in ("plain", "only", "full", "chunks")}
    r = {k: str(tmp_path / (k + ".tsv")) for k in ("only", "full", "chunks", "alone")}
    plain = run(["--trees-only", "--transfer=" + t["plain"]])
    assert run(["--trees-only", "--transfer=" + t["only"], "--rogues=" + r["only"], "--rogue-cutoff=1"]) == plain
    assert open(t["only"]).read() == open(t["plain"]).read()  # stdout and the other file keep their bytes
    ctx = lib.Context(0)
    try:
        M = lib.dist_matrix(seqs, host_threads=4)
        J = lib.nj(ctx, lib.distances(M, lib.M_JC))
        R, bad = lib.bootstrap_nj(ctx, M, 5, lib.M_JC, seed=SEED)
        moved, pairs = lib.nj_transfer_taxa(ctx, J, R, skip=(bad >= 0).astype(np.uint8), cutoff=1.0)
    finally:
        ctx.close()
    assert moved.tolist() == [0, 0, 0, 0, 0, 1, 3, 0] and pairs == 24  # (what the seed was chosen for)
    text = open(r["only"]).read()
    assert text == _table(names, moved, pairs)
    # the replicates as matrices: the same table, whole and in chunks of two
    whole = run(["--transfer=" + t["full"], "--rogues=" + r["full"], "--rogue-cutoff=1"])
    assert open(r["full"]).read() == text and whole.count(b"\n") == 6 * (n + 1)
    assert run(["--transfer=" + t["chunks"], "--rogues=" + r["chunks"], "--rogue-cutoff=1"], {"ANDI_HIP_BOOT_CHUNK": "2"}) == whole
    assert open(r["chunks"]).read() == text and open(t["chunks"]).read() == open(t["full"]).read()
    # --rogues alone joins the replicates too
    assert run(["--rogues=" + r["alone"], "--rogue-cutoff=1"]) == whole and open(r["alone"]).read() == text
