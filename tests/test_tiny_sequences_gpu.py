"""The one-call seam on ragged tiny sequences: subjects written from the resident queries (k_rs_from_query), thresholds
from the device's G+C counts (k_gc_counts), the suffix sorter and the index build in slots sized for the longest text --
so every text but one lands in a slot that is too large for it.  Bit-exact against the oracle."""
import numpy as np
import pytest

from conftest import knobs

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


def _sequences():
    """cut from two bases 2 % apart, in turn, at offsets that overlap; three carry a '!', one is all G, one all A"""
    from andi_amd import synth
    base = synth.base_codes(1200, 51)
    two = [synth.to_bytes(base), synth.to_bytes(synth.mutate_codes(base, 0.02, 52))]
    seqs = []
    for k, n in enumerate(LENGTHS):
        at = (13 * k) % 40 if n < 1000 else 0
        s = two[k % 2][at:at + n]
        if n in (9, 65, 257):
            s = s[:n // 3] + b"!" + s[n // 3 + 1:]
        if n == 4:
            s = b"G" * n
        if n == 16:
            s = b"A" * n
        assert len(s) == n
        seqs.append(s)
    assert sum(b"!" in s for s in seqs) == 3
    return seqs


@pytest.fixture(scope="module")
def tiny(orc):
    import andi_amd
    seqs = _sequences()
    return seqs, {m: orc.dist_matrix(seqs, model=m, threads=0) for m in (andi_amd.M_JC, andi_amd.M_LOGDET)}


def _compare(got, want, what):
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, "pairs (subject, query)", bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("model", ["jc", "logdet"])
def test_tiny_sequences_through_the_seam(tiny, model):
    import andi_amd
    seqs, want = tiny
    m = {"jc": andi_amd.M_JC, "logdet": andi_amd.M_LOGDET}[model]
    assert want[m][-1].any()  # (matches exist)
    _compare(andi_amd.dist_matrix(seqs, model=m, host_threads=2), want[m], "the engine's choice")
    with knobs(COOP=0):
        _compare(andi_amd.dist_matrix(seqs, model=m, host_threads=2), want[m], "ANDI_COOP=0")
    _compare(andi_amd.dist_matrix(seqs, model=m, host_threads=2, sa_on_host=True), want[m], "sa_on_host")
