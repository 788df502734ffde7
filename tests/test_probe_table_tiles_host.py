"""tests/probe_table_tiles.py on the CPU: the classifier of whole tiles against a plain loop over the tiles, and the
properties of the subjects that tests/test_probe_table_tiles_gpu.py relies on (seeds pinned there)."""
import numpy as np
import pytest

import probe_table_model as ptm
import probe_table_tiles as ptt


def _whole_by_loop(rs, sa, K, tile):
    """a tile is whole when it lies inside the text and each of the tile + 3 suffixes it stages starts with K nucleotides"""
    n = len(rs)
    out = []
    for b in range((n + tile) // tile):
        r0 = b * tile
        ok = r0 >= 2 and r0 + tile < n
        if ok:
            for r in range(r0 - 2, r0 + tile + 1):
                p = int(sa[r])
                word = rs[p:p + K]
                if len(word) < K or any(c not in b"ACGT" for c in word):
                    ok = False
                    break
        out.append(ok)
    return np.array(out, bool)


@pytest.mark.parametrize("name,K,tile", [("halo-2", 8, ptt.TILE), ("joined-6", 9, ptt.TILE), ("acgt-x-2000", 7, ptt.TILE),
                                         ("halo-1", 6, 64), ("tiny", 4, 4)])
def test_classifier_equals_the_loop(name, K, tile):
    rs, sa = ptt.texts()[name], ptt.model_sa(name)
    want = _whole_by_loop(rs, sa, K, tile)
    got = ptt.whole_tiles(rs, sa, K, tile)
    assert got.dtype == bool and (got == want).all()
    assert not got[0] and not got[-1]  # the text's first and last tile never are
    if name != "tiny":
        assert got.any() and not got.all()


def test_subjects_have_the_properties_the_gpu_cases_assert():
    facts = ptt.facts()
    assert facts["random-40k"]["tiles"] == 105 and len(ptt.texts()["random-40k"]) == 80001
    for depth in ("natural", 8, 10):
        f = ptt.facts(depth)
        assert f["random-40k"]["whole"] >= 60 and f["random-40k"]["tiles"] - f["random-40k"]["whole"] >= 10
        assert f["joined-6"]["alternations"] >= 20
        assert f["joined-60"]["whole"] == 0  # (see test_probe_table_tiles_gpu.test_alternating_tiles)
        assert f["repeat-x-5000"]["leaving"] >= 1 and f["repeat-x-5000"]["far"] >= 1
        assert f["acgt-x-2000"]["whole"] >= 10 and f["acgt-x-2000"]["most_entries"] == 0
    for off in ptt.HALO_SEEDS:
        assert [off] in facts["halo%+d" % off]["halo_only"].values()
    assert ptt.facts("natural+1")["random-40k"]["past_ranked"] >= 60
