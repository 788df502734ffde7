"""CPU model of pass B of the anchor scan (andi_amd/csrc/scan_lane.hip: stitch_one; scan.hip: stitch_segment) and of the
entries it assumes (scan_dev.h: entry_source, assumed_entry), TEST INFRASTRUCTURE ONLY.

Pass B's contract is exact.  A segment [start, end) of a query, entered by the true chain in state T, gets from pass B
the counts `owned` and the state `true_exit`; both must be what the plain loop of dist_anchor (src/process.c:153-197)
produces when it starts in T and runs while p < end -- coop_model.plain_segment(P, T, end) -- whether or not T was the
right entry (pass C verifies entries only, and re-stitches a segment whose entry was wrong: a wrong exit or a wrong
count behind a right entry is what nothing else sees).  The kernel gets there by six shortcuts past the plain loop; this
file says, from the model alone, which of them a replay is a case of (classify), so that a test can tell that its
inputs reach them all.

Rows of states are the device's ChainState words: p, lastS, lastQ, lastLen, lwra, pad[0], pad[1] (in a cold exit: the
anchors the cold chain found, capped at 255; 0xffffffff: not recorded), pad[2].
"""
import numpy as np

from oracle import orc
from tests import coop_model as cm
from tests.coop_model import State, cold_state, plain_step

SPAN_WINDOW = 8  # ANDI_SPAN_WINDOW
MEMORY_WINDOW = 4096  # ANDI_MEMORY_WINDOW
STITCH_FIRST = 12  # ANDI_STITCH_FIRST
STITCH_BUDGET = 48  # ANDI_STITCH_BUDGET
ANCHORS = 6  # the word of a cold exit's row that holds its anchor count

CLASSES = ("shortcut", "first", "mark", "met", "position", "own")


class Pair(cm.Pair):
    """coop_model.Pair that remembers what the lookups answered: the chains of a pair's segments, cold and true, at
    every segment length and in both counting modes, ask at the same positions over and over"""

    def __init__(self, subject, query, p_value=0.025, esa=None, exact=False):
        super().__init__(subject, query, p_value, esa, exact)
        self._probe, self._lcp = {}, {}

    def probe(self, p):
        r = self._probe.get(p)
        if r is None:
            r = self._probe[p] = super().probe(p)
        return r

    def lcp(self, p, s, maxlen):
        key = (p, s, maxlen)
        r = self._lcp.get(key)
        if r is None:
            r = self._lcp[key] = super().lcp(p, s, maxlen)
        return r

    def counting(self, exact):
        """the same pair (and its remembered lookups) under the other way of counting an anchor"""
        if exact == self.exact:
            return self
        other = object.__new__(Pair)
        other.__dict__.update(self.__dict__)
        other.exact = exact
        return other


def pairs_of(seqs, p_value=0.025):
    """{(s, q): Pair} of all ordered pairs of a set, one enhanced suffix array per subject"""
    out = {}
    for s, subject in enumerate(seqs):
        E = orc.OracleEsa(subject, p_value)
        for q, query in enumerate(seqs):
            if q != s:
                out[(s, q)] = Pair(subject, query, p_value, esa=E)
    return out


def segments(qlen, seg):
    return [(k * seg, min((k + 1) * seg, qlen)) for k in range((qlen + seg - 1) // seg)]


def walk(P, st0, end):
    """plain_segment that also keeps the loop-top states the chain was in, the first one included"""
    st, rec = st0.copy(), cm.Record()
    states = [st.tup()]
    while st.p < end:
        plain_step(P, st, rec)
        states.append(st.tup())
    rec.exit = st.tup()
    rec.states = states
    return rec


def cold_records(P, seg):
    """what pass A leaves of every segment of the pair: the plain loop from the initial state (segment 0) or from the
    cold state at the segment's start"""
    return [walk(P, State() if k == 0 else cold_state(start, P.n), end) for k, (start, end) in enumerate(segments(P.qlen, seg))]


def exit_row(rec, unknown=False):
    """a cold record's exit as the device's ChainState words (unknown: the group scan does not count its anchors)"""
    return list(rec.exit) + [0, 0xffffffff if unknown else min(rec.anchors, 255), 0]


def epilogue(P, st, counts):
    """src/process.c:199-211, on the state the chain left the query in"""
    if st.lastLen >= P.qlen:
        cm.count_anchor(P, counts, 0, P.qlen)
    elif st.lwra or st.lastLen >= 2 * P.thr:
        cm.count_anchor(P, counts, st.lastQ, st.lastLen)


def chain_by_segments(P, seg):
    """dist_anchor as pass B's contract has it: segment after segment, each entered in the state the one before was
    left in; returns the 16 counts and the exits"""
    st, total, exits = State(), np.zeros(16, np.int64), []
    for start, end in segments(P.qlen, seg):
        rec = cm.plain_segment(P, st, end)
        total += rec.counts
        st = State(*rec.exit)
        exits.append(rec.exit)
    epilogue(P, st, total)
    return total, exits


# ------------------------------------------------------------------ the entries pass B assumes (scan_dev.h)
def entry_source(cold_exits, k, seg, qlen):
    """the segment whose cold exit is taken for the true chain's entry into segment k >= 1: k - 1, unless one of the
    SPAN_WINDOW segments before a segment leaves beyond that segment's end -- such segments are jumped over"""
    j = k - 1
    while j >= 1:
        end_j = min((j + 1) * seg, qlen)
        if not any(cold_exits[j - back][0] >= end_j for back in range(1, min(SPAN_WINDOW, j) + 1)):
            break
        j -= 1
    return j


def assumed_entry(cold_exits, k, seg, qlen):
    """the state pass B lets the true chain enter segment k >= 1 in, five words: the position of entry_source's cold exit,
    and its memory -- unless that cold chain found no anchor: then the memory of the nearest segment before it (by
    entry_source, MEMORY_WINDOW hops at most) whose cold chain found one, or of segment 0"""
    j = entry_source(cold_exits, k, seg, qlen)
    T = [int(x) for x in cold_exits[j][:5]]
    if int(cold_exits[j][ANCHORS]) != 0 or j == 0:
        return tuple(T)
    for _ in range(MEMORY_WINDOW):
        j = entry_source(cold_exits, j, seg, qlen)
        if int(cold_exits[j][ANCHORS]) != 0 or j == 0:
            T[1:5] = [int(x) for x in cold_exits[j][1:5]]
            break
    return tuple(T)


# ------------------------------------------------------------------ the ways a replay settles
def classify(P, T, k, seg, cold, replay=None):
    """(class, chain steps of the true chain before the replay settles) of the true chain that enters segment k >= 1 in
    state T (five words), from the model alone; `cold` is the segment's cold record with its states (walk).

    shortcut  scan_lane.hip:880-883: T stands right behind an anchor that ends where the cold chain's first anchor
              ends, on its diagonal, inside the segment, and the cold chain has a mark; the even-split models only
    first     the chain from T passes through the state right behind the cold chain's first anchor (inside the segment)
    mark      ... through the mark's state (right behind the cold chain's second anchor)
    met       ... through some other state of the cold chain
    position  it leaves at the cold exit's position with a memory of its own
    own       it leaves elsewhere
    Equal states have equal futures, so the first state of the cold chain that the true chain is in decides.  The
    steps are the true chain's alone: the kernel also counts those of the cold chain it replays beside it."""
    start, end = k * seg, min((k + 1) * seg, P.qlen)
    T = tuple(int(x) for x in T[:5])
    p, lastS, lastQ, lastLen, _ = T
    if not P.exact and cold.mark is not None:
        fq, fs, fl = cold.first
        if p == fq + fl + 1 and lastQ + lastLen == fq + fl and lastS + lastLen == fs + fl and p < end:
            return "shortcut", 0
    rep = replay if replay is not None else walk(P, State(*T), end)
    MF = None
    if cold.first is not None and cold.first[0] + cold.first[2] + 1 < end:
        MF = (cold.first[0] + cold.first[2] + 1, cold.first[1], cold.first[0], cold.first[2], 0)
    MK = cold.mark[0] if cold.mark is not None else None
    others = set(cold.states)
    for steps, s in enumerate(rep.states):
        if s == MF:
            return "first", steps
        if s == MK:
            return "mark", steps
        if s in others:
            return "met", steps
    steps = len(rep.states) - 1
    return ("position" if rep.exit[0] == cold.exit[0] else "own"), steps
