"""andi_hip_place on the MI355X: bit-exact to the NumPy restatement (tests/place_model.py) on everything it returns, for
both methods, across the tiles of k_place, on rows with pairs without a distance, on odd trees, on a tree of 4097 leaves, in forced small groups of
queries; its argument checks; and andi-hip --reference --backbone --place."""
import json
import os
import subprocess

import numpy as np
import pytest

import place_model as pm
from conftest import ROOT, knobs

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "andi_amd", "andi-hip")
LEAF_TILE, EDGE_TILE, QUERY_TILE = 64, 64, 4  # place.hip: LT, ET, QT
METHODS = ("ols", "fm")


@pytest.fixture(scope="module")
def ctx():
    from andi_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, nan_bits=True):
    """everything place returns, bit for bit (nan_bits=False: a NaN only has to be a NaN, its bits are the platform's)"""
    for g, w, what in zip(got, want, ("records", "err", "x", "p")):
        assert g.shape == w.shape, what
        if what == "records":
            assert (g["edge"] == w["edge"]).all() and (g["used"] == w["used"]).all(), what
            pairs = [(g[f], w[f], f) for f in ("distal", "pendant", "err")]
        else:
            pairs = [(g, w, what)]
        for a, b, f in pairs:
            if not nan_bits:
                assert (np.isnan(a) == np.isnan(b)).all(), f
                a, b = np.where(np.isnan(b), 0.0, a), np.where(np.isnan(b), 0.0, b)
            bad = np.argwhere(_bits(a) != _bits(b))
            assert not len(bad), (f, bad[:4].tolist(), np.asarray(a)[tuple(bad[0])], np.asarray(b)[tuple(bad[0])])


def _queries(rng, J, n, nq, noise=0.03):
    """rows of distances: points on random edges, their tree distances off by a few percent; every third row plain noise"""
    _, L = pm.edges(J, n)
    rows = []
    for q in range(nq):
        v = int(rng.integers(2 * n - 3))
        d = pm.point_distances(J, n, v, rng.uniform(0, 1) * abs(L[v]), rng.uniform(0, 0.05))
        rows.append(rng.uniform(0.01, 0.3, n) if q % 3 == 2 else d * (1.0 + rng.uniform(-noise, noise, n)))
    return np.stack(rows)


def _check(ctx, J, D, **kw):
    from andi_amd import lib
    for method in METHODS:
        _same(lib.place(ctx, J, D, method, per=True), pm.place(J, D, method, per=True), **kw)


@pytest.mark.parametrize("nq", [1, 2, 7])
@pytest.mark.parametrize("n", [3, 4, 5, 17, 63, 64, 65, 130])
def test_bit_exact_on_random_trees(ctx, n, nq):
    rng = np.random.default_rng(100 * n + nq)
    J = pm.random_tree(rng, n)
    _check(ctx, J, _queries(rng, J, n, nq))


@pytest.mark.parametrize("n, nq, what", [
    (LEAF_TILE + 1, 3, "one leaf more than a leaf tile"),
    ((EDGE_TILE + 1 + 3) // 2, 3, "2n - 3 = one edge more than an edge tile"),
    (9, QUERY_TILE + 1, "one query more than a query tile"),
    (600, 33, "many tiles of each kind"),
])
def test_bit_exact_across_tiles(ctx, n, nq, what):
    assert what != "2n - 3 = one edge more than an edge tile" or 2 * n - 3 == EDGE_TILE + 1
    rng = np.random.default_rng(n + nq)
    J = pm.random_tree(rng, n)
    _check(ctx, J, _queries(rng, J, n, nq))


def test_rows_with_pairs_without_a_distance(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(11)
    n = 70
    J = pm.random_tree(rng, n)
    D = _queries(rng, J, n, 8, noise=0.01)
    D[0, [3, 40, 69]] = np.nan
    D[1, [0, 64, 65]] = np.inf
    D[1, 7] = -np.inf
    D[2, :] = np.nan
    D[2, 66] = 0.25        # one usable leaf
    D[3, :] = np.nan       # none
    D[4, :] = np.inf
    D[5, 12] = np.nan      # the whole side below edge 12: that edge is no candidate
    pair = next(s for s in range(n - 3) if J[s]["a"] < n and J[s]["b"] < n)
    D[6, [J[pair]["a"], J[pair]["b"]]] = np.nan  # ... and below an inner edge
    _check(ctx, J, D)
    for method in METHODS:
        out, err, x, p = lib.place(ctx, J, D, method, per=True)
        assert out["edge"][2:5].tolist() == [-1, -1, -1] and out["used"][:5].tolist() == [n - 3, n - 4, 1, 0, 0]
        assert (out["err"][2:5] == np.inf).all() and not out["distal"][2:5].any() and not out["pendant"][2:5].any()
        assert np.isinf(err[2:5]).all()
        assert err[5, 12] == np.inf and x[5, 12] == 0 and p[5, 12] == 0 and out["edge"][5] >= 0
        assert err[6, n + pair] == np.inf and err[6, J[pair]["a"]] == np.inf and out["edge"][6] >= 0
        assert (out["edge"][[0, 1, 7]] >= 0).all() and np.isfinite(out["err"][[0, 1, 7]]).all()


def test_a_distance_of_zero(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(12)
    n = 66
    J = pm.random_tree(rng, n)
    D = _queries(rng, J, n, 5)
    D[0, 65] = 0.0
    D[1, [9, 30]] = 0.0, -0.0   # the first such leaf
    D[2, 30] = -0.0
    D[3, 5] = 0.0
    D[3, [0, 1, 2]] = np.nan
    _check(ctx, J, D)  # (OLS has no special rule; under FM nothing of the row's sums is kept where the rule holds)
    out, err, x, p = lib.place(ctx, J, D, "fm", per=True)
    assert out["edge"][:4].tolist() == [65, 9, 30, 5] and out["used"][:4].tolist() == [n, n, n, n - 3]
    for q in range(4):
        assert (out["distal"][q], out["pendant"][q], out["err"][q]) == (0.0, 0.0, 0.0)
        assert err[q, out["edge"][q]] == 0.0 and np.isinf(np.delete(err[q], out["edge"][q])).all()
        assert not x[q].any() and not p[q].any()
    assert (lib.place(ctx, J, D, "ols")["err"][:4] > 0).all()


@pytest.mark.parametrize("shape", ["caterpillar", "balanced", "random"])
def test_negative_and_zero_branch_lengths(ctx, shape):
    rng = np.random.default_rng(13)
    n = 67
    lengths = rng.uniform(-0.02, 0.1, 2 * n - 3)
    lengths[rng.choice(2 * n - 3, 20, replace=False)] = 0.0
    lengths[5] = -0.0
    if shape == "random":
        it = iter(lengths)
        J = pm.random_tree(rng, n, lambda k: [next(it) for _ in range(k)])
    else:
        J = getattr(pm, shape)(n, lengths)
    D = np.abs(_queries(rng, J, n, 6))
    _check(ctx, J, D)


def test_small_groups_of_queries_give_the_same_bytes(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(14)
    n, nq = 40, 11
    J = pm.random_tree(rng, n)
    D = _queries(rng, J, n, nq)
    D[4, 3] = np.nan
    for method in METHODS:
        whole = lib.place(ctx, J, D, method, per=True)
        for g in (1, 3, QUERY_TILE + 1):
            with knobs(PLACE_GROUP=g):
                parts = lib.place(ctx, J, D, method, per=True)
            for a, b in zip(whole, parts):
                assert a.tobytes() == b.tobytes(), (method, g)
        _same(whole, pm.place(J, D, method, per=True))


def test_exact_recovery_under_ols(ctx):
    from andi_amd import lib
    rng = np.random.default_rng(15)
    for k in range(12):
        n = 3 + (5 * k) % 17
        J = pm.random_tree(rng, n, lambda m: rng.integers(2, 17, m) / 64.0)
        _, L = pm.edges(J, n)
        v = int(rng.integers(2 * n - 3))
        x, p = float(rng.integers(1, int(L[v] * 64))) / 64.0, float(rng.integers(0, 9)) / 64.0
        out = lib.place(ctx, J, pm.point_distances(J, n, v, x, p)[None, :], "ols")[0]
        assert (out["edge"], out["distal"], out["pendant"], out["err"], out["used"]) == (v, x, p, 0.0, n)


def test_a_tree_whose_leaf_sets_have_65_words(ctx):
    """n = 4097: W = 65, so k_sets runs a second block, and k_paths and k_place ask child_word for word (tile) 64 -- the
    one that holds leaf 4096 alone.  (a) Exact recovery under OLS with lengths in 64ths (every sum exact, as in
    test_exact_recovery_under_ols) of points on the edges of leaf 4096, of leaf 70 and of the inner node above leaf 4096,
    whose set holds that leaf: a wrong bit 4096 puts the leaf on the wrong side of the edge and the error is no longer 0.
    (b) Two noisy queries under FM, bit for bit against the model, every edge.  The table T is 268 MB on the device; the
    host's part dominates: the model's path lengths take 0.6 s and its two queries 6 s (measured; hence FM only and two
    queries), the device's calls a small fraction of that."""
    from andi_amd import lib
    n = 4097
    rng = np.random.default_rng(n)
    J = pm.random_tree(rng, n, lambda m: rng.integers(2, 17, m) / 64.0)
    H, below, parent, L = pm.paths(J, n)
    E = 2 * n - 3

    def point(v, x, p):  # (place_model.point_distances, on the paths computed once)
        return np.where(below[v], (p + x) + H[v], (p + (L[v] - x)) + H[parent[v]])

    above = int(parent[4096])
    assert above < E and below[above, 4096] and below[above].sum() >= 2 and not below[70, 4096]
    want = [(4096, 1 / 64.0, 3 / 64.0), (70, 1 / 64.0, 0.0), (above, (L[above] * 64 - 1) / 64.0, 5 / 64.0)]
    out = lib.place(ctx, J, np.stack([point(*w) for w in want]), "ols")
    for q, (v, x, p) in enumerate(want):
        assert (out["edge"][q], out["distal"][q], out["pendant"][q], out["err"][q], out["used"][q]) == (v, x, p, 0.0, n), q
    # (b)
    D = np.stack([point(above, 0.5 * L[above], 0.02), point(int(rng.integers(E)), 0.0, 0.03)])
    D = D * (1.0 + rng.uniform(-0.03, 0.03, D.shape))
    got, model = lib.place(ctx, J, D, "fm", per=True), pm.place(J, D, "fm", per=True)
    _same(got, model)
    assert (model[0]["edge"] >= 0).all() and np.isfinite(model[1]).all()


def test_bad_arguments_and_records_leave_the_context_usable(ctx):
    from andi_amd import lib
    L = lib.load()
    rng = np.random.default_rng(16)
    n = 20
    J = pm.random_tree(rng, n)
    D = _queries(rng, J, n, 2)
    out = np.zeros(2, lib.PLACEMENT)

    def call(J=J, n=n, D=D, nq=2, method=1, out=out):
        return L.andi_hip_place(ctx._h, J.ctypes.data if J is not None else None, n, D.ctypes.data if D is not None else None,
                                nq, method, out.ctypes.data if out is not None else None, None, None, None)

    for kw in (dict(J=None), dict(D=None), dict(out=None), dict(nq=0), dict(n=2), dict(n=65536), dict(method=2), dict(method=-1)):
        assert call(**kw) == 1, kw
        assert b"bad arguments" in L.andi_hip_last_error(ctx._h)
    twice = J.copy()
    twice[5]["a"] = twice[4]["a"]  # a node that is a child twice
    late = J.copy()
    late[2]["b"] = n + 7           # a child that no earlier record made
    for bad in (twice, late):
        assert call(J=bad) == 1
        assert L.andi_hip_last_error(ctx._h) == b"andi_hip_place: the tree's records are not those of andi_hip_nj"
    for value in (np.nan, np.inf, -np.inf):
        bad = J.copy()
        bad[7]["lb"] = value
        assert call(J=bad) == 1 and b"record 7 is not finite" in L.andi_hip_last_error(ctx._h)
    ignored = J.copy()
    ignored[3]["lc"] = np.nan  # (a pair record has no third child)
    assert call(J=ignored) == 0
    assert not out.tobytes() == bytes(out.nbytes)
    _same(lib.place(ctx, J, D, "fm", per=True), pm.place(J, D, "fm", per=True))


# ---------------------------------------------------------------- the command line
def _fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for k in range(0, len(seq), 70):
            f.write(seq[k:k + 70].decode() + "\n")
    return str(path)


def test_cli_place(tmp_path, ctx):
    from andi_amd import lib, synth
    nr, k = 6, 4
    seqs, _ = synth.tree_set(nr + 2, 20_000, seed=91)
    refs, queries = seqs[:nr], [seqs[nr], seqs[nr + 1], seqs[k]]  # the last query is a copy of reference k
    rnames, qnames = ["ref%d" % i for i in range(nr)], ["new_a", 'new"b\\', "copy_of_%d" % k]
    rfiles = [_fasta(tmp_path / ("r%d.fa" % i), rnames[i], s) for i, s in enumerate(refs)]
    qfiles = [_fasta(tmp_path / ("q%d.fa" % i), qnames[i], s) for i, s in enumerate(queries)]
    env = dict(os.environ, ANDI_HIP_GPUS="1")
    tree, out = str(tmp_path / "backbone.nwk"), str(tmp_path / "out.jplace")

    def run(args, ok=True):
        p = subprocess.run([CLI, "-t", "4"] + args, capture_output=True, timeout=300, env=env)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout, p.stderr.decode()

    run(["--tree=" + tree] + rfiles)
    ref_args = ["--reference=" + f for f in rfiles]
    plain, plain_err = run(ref_args + qfiles)
    MRQ, MQR = lib.dist_rect(refs, queries, model=lib.M_JC, host_threads=4)
    D = lib.distances_rect(MRQ, MQR, lib.M_JC)
    J = lib.parse_newick(open(tree).read(), rnames)
    for method, args in (("fm", []), ("ols", ["--place-method=ols"]), ("fm", ["--place-method=FM"])):
        got, got_err = run(ref_args + ["--backbone=" + tree, "--place=" + out] + args + qfiles)
        assert got == plain and got_err == plain_err  # stdout and the warnings keep their bytes
        P = lib.place(ctx, J, D, method)
        text = open(out).read()
        assert text == lib.jplace(J, rnames, P, qnames, method)
        doc = json.loads(text)
        assert [p["n"] for p in doc["placements"]] == [[q] for q in qnames]
        if method == "fm":  # the copy is at distance 0.0 from its original: on that leaf's edge, at the leaf
            assert doc["placements"][2]["p"] == [[k, 0.0, 1, 0.0, 0.0]]
    # -v's coverage block keeps its bytes too
    assert run(["-v"] + ref_args + ["--backbone=" + tree, "--place=" + out] + qfiles)[0] == run(["-v"] + ref_args + qfiles)[0]
    # a query without a distance to any reference: a soft warning that names it, the others are placed
    alien = _fasta(tmp_path / "alien.fa", "alien", synth.unrelated(20_000, 5))
    p = subprocess.run([CLI, "-t", "4"] + ref_args + ["--backbone=" + tree, "--place=" + out, alien, qfiles[0]],
                       capture_output=True, timeout=300, env=env)
    Da = lib.distances_rect(*lib.dist_rect(refs, [synth.unrelated(20_000, 5), queries[0]], model=lib.M_JC, host_threads=4), lib.M_JC)
    Pa = lib.place(ctx, J, Da, "fm")
    assert Pa["edge"][0] == -1 and Pa["used"][0] < 2 and Pa["edge"][1] >= 0
    assert p.returncode == 1 and "No placement for 'alien': only %d of its distances" % Pa["used"][0] in p.stderr.decode()
    assert open(out).read() == lib.jplace(J, rnames, Pa, ["alien", "new_a"], "fm")
    assert [q["n"] for q in json.loads(open(out).read())["placements"]] == [["new_a"]]
    # refusals
    for args, message in (
            (["--place=" + out, "--backbone=" + tree] + rfiles, "Placement (--place) needs references to place on"),
            (ref_args + ["--place=" + out] + qfiles, "Placement (--place) needs the tree of the references: give --backbone=FILE."),
            (ref_args + ["--backbone=" + tree] + qfiles, "A backbone tree (--backbone) needs somewhere to go: give --place=FILE."),
            (ref_args + ["--backbone=" + tree, "--place=" + out, "--place-method=wls"] + qfiles,
             "Expected one of 'fm' or 'ols' for --place-method, but 'wls' was given."),
            (ref_args[:2] + ["--backbone=" + tree, "--place=" + out] + qfiles, "needs a tree: give at least three references"),
            (ref_args[:5] + ["--backbone=" + tree, "--place=" + out] + qfiles, "backbone.nwk: andi_hip_parse_newick: byte"),
            (ref_args + ["--backbone=" + tree, "--place=" + out, "--tree=" + tree] + qfiles,
             "A tree (--tree) is not available together with --reference or --reference-list."),
    ):
        stdout, stderr = run(args, ok=False)
        assert message in stderr and stdout == b"", args
    stdout, stderr = run(ref_args[:5] + ["--backbone=" + tree, "--place=" + out] + qfiles, ok=False)
    assert "unknown name 'ref5'" in stderr  # a backbone whose leaves are not the references: the parser's message
