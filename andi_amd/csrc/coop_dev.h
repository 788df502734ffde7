// coop_dev.h -- pass A with one wavefront per chain (scan_coop.hip): what mode W (coop_window.h) and mode P (coop_pool.h) share.
// In dependency order: constants, the diagnostics' counters, the W_* flags, the wavefront's helpers, Chain; coop_lcp, the counting of gaps
// and anchors, the probes; coop_note_anchor and coop_account; the texts bit-sliced and the substitutions counted without a loop; the walks'
// verdicts; coop_segment, the driver of one segment -- mode G's step, the step limit of routed calls and what pass B reads are written here
// and nowhere else.
#pragma once
#include "lane_chain.h"
#include "knobs.h"

namespace {

constexpr uint32_t COOP_KCAP = 12; // stretches of a window that are counted nowhere (more: the window ends before the next one)
// (routed calls hand a pair back when one of its segments needs more generic steps than ScanArgs.route_giveup -- 1024: long stretches without homology that the sampling missed (clean sets: <= 45 steps; an island of 20 kbp: some 1500).  Grinding through them instead -- the limit at 16384 -- took the structured set's pass A from 9.4 to 28 ms for 9 of its 812 pairs, and its passes B/C from 6.9 to 15 ms: their true chains cross the islands on long segments, one lane each)
constexpr uint32_t COOP_TRIAL_LCP = 16;  // routed calls: a match followed through more rounds of 2048 symbols than this is longer than its segment
constexpr uint32_t COOP_PARK = 16; // parked lanes (their probe needs lane_probe) that are served together
constexpr uint32_t COOP_MAX_X = 3;  // anchors off the window's diagonal a walk follows before it gives up
constexpr uint32_t NOPOS = 0xffffffffu;
// Mode G where the block of probes has no answer for the chain's position: that position alone first, by one lane and COOP_SOLO_CAP symbols deep
// (a unique match that reaches the cap is finished by coop_lcp; several that reach it: the block).  After COOP_SOLO_MAX such steps in a row
// without an anchor the chain is in a stretch without homology, and the block of 64 probes takes over until the next anchor.
// Neither changes a result.  Measured (profiles/r12_cold_start.md): caps of 32, 64 and 128 are level; with 2 steps in a row the bench set is
// where it is with 1, and a routed call of 12 x 1 Mbp, whose pairs up to 6 % apart start most segments on a probe that finds no anchor, loses 5 %.
#ifndef COOP_SOLO_CAP
#define COOP_SOLO_CAP 64u
#endif
#ifndef COOP_SOLO_MAX
#define COOP_SOLO_MAX 1u
#endif

// -DANDI_COOP_STATS: how the kernel's work splits (diagnostic builds only; ANDI_COOP_STATS=1 prints)
#ifdef ANDI_COOP_STATS
__device__ unsigned long long g_coop_stats[28];
#define CSTAT(k, v)                                                              \
	do {                                                                         \
		if (__lane_id() == 0) atomicAdd(&g_coop_stats[k], (unsigned long long)(v)); \
	} while (0)
// wave-cycles (s_memtime) spent per phase: TICK(t) starts the clock, TOCK(t, phase) charges the time since to `phase`
// (slots 0 ... 6: the window's phases, 7: the segment's loop as a whole, 8 ...: mode G's parts and what lies around the loop)
__device__ unsigned long long g_coop_cycles[16];
#define TICK(t) unsigned long long t = __builtin_readcyclecounter()
#define TOCK(t, ph)                                                                        \
	do {                                                                                   \
		const unsigned long long now_ = __builtin_readcyclecounter();                      \
		if (__lane_id() == 0) atomicAdd(&g_coop_cycles[ph], now_ - t);                     \
		t = now_;                                                                          \
	} while (0)
#else
#define CSTAT(k, v) ((void)0)
#define TICK(t) ((void)0)
#define TOCK(t, ph) ((void)0)
#endif
#ifdef ANDI_COOP_STATS
__device__ unsigned int g_coop_max[4];
__device__ unsigned long long g_coop_trip_lanes[2][8]; // trips by lanes at work: 0, 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64 (plain trips, service trips)
#endif
enum { PH_G, PH_STREAM, PH_HEADS, PH_WALKS, PH_HOPS, PH_STRETCH, PH_FINAL, PH_LOOP, PH_G_LCP, PH_G_BLOCK, PH_G_SOLO, PH_G_SOLO_LCP, PH_G_NOTES, PH_PROLOGUE, PH_EPILOGUE };
enum { CS_SEGMENTS, CS_G_STEPS, CS_BLOCKS, CS_LCP, CS_WINDOWS, CS_MOVED, CS_HEADS, CS_TRIPS, CS_LANE_STEPS, CS_PROBES, CS_ONPATH,
	   CS_HOPS, CS_G_GAPS, CS_COVERED, CS_DROPPED, CS_X, CS_LCP_ROUNDS, CS_NODES, CS_SERVICE, CS_SERVICE_LANES, CS_WHY_PRE, CS_WHY_MULTI, CS_WHY_LONG, CS_WHY_OTHER,
	   CS_G_FIRST, CS_SOLO, CS_SOLO_LCP, CS_SOLO_BLOCK };

// how a head's walk ended
enum : uint32_t { W_OK = 1, W_OPEN = 2, W_EXIT = 3, W_BREAK = 4, W_STATUS = 7u, W_HADX = 8u, W_LUCKY = 16u, W_NX_SHIFT = 8, W_ONPATH = 1u << 12 };

__device__ __forceinline__ uint32_t uni(uint32_t v) { // a wave-uniform value: into a scalar register
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// the lanes of the wavefront exchange data through LDS: order this lane's accesses around the hand-over
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void lds_or(uint32_t *p, uint32_t v) {
	(void)__hip_atomic_fetch_or((lds_u32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}


// inclusive prefix sums / prefix maxima over the 64 lanes in six DPP steps (shifts by 1, 2, 4, 8 inside the rows of 16 lanes, then
// lane 15 of a row into the next row, lane 31 into the upper half; lanes without a source take 0: the identity of both for unsigned
// values) -- six vector instructions where six __shfl_up were six LDS-crossbar round trips with their address arithmetic
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1 and 3
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2 and 3
	return v;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
	uint32_t o;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false), v = o > v ? o : v;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false), v = o > v ? o : v;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false), v = o > v ? o : v;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false), v = o > v ? o : v;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false), v = o > v ? o : v;
	o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false), v = o > v ? o : v;
	return v;
}

// Lane l's value for a wave-uniform l: v_readlane; the value of the lane below / above (lane 0 / 63: its own): one DPP move.
// (__shfl and its kin are ds_bpermute: a trip through the LDS crossbar each.)
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t l) {
	return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)uni(l));
}
__device__ __forceinline__ uint32_t lane_below(uint32_t v) {
	return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false); // wave_shr:1
}
__device__ __forceinline__ uint32_t lane_above(uint32_t v) {
	return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false); // wave_shl:1
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { // (all lanes active) the sum over the wavefront, wave-uniform
	return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(v), 63);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
	for (int d = 32; d; d >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
		v = o < v ? o : v;
	}
	return v;
}

// 8 nibble flags (bit 4k + 3 of a word: symbols k differ) -> 8 bits
__device__ __forceinline__ uint32_t squeeze8(uint32_t x) {
	x = (x >> 3) & ONES;
	x = (x | (x >> 3)) & 0x03030303u;
	x = (x | (x >> 6)) & 0x000f000fu;
	return (x | (x >> 12)) & 0xffu;
}

__device__ __forceinline__ uint32_t squeeze32(const uint4 &d) {
	return squeeze8(d.x) | (squeeze8(d.y) << 8) | (squeeze8(d.z) << 16) | (squeeze8(d.w) << 24);
}

// 32 symbols of the subject from offset sa on (any sa >= -32; at and beyond the text's end: NUL, the padding's symbol)
__device__ __forceinline__ uint4 ld_subject_guarded(const PairCtx &c, int64_t sa) {
	if (sa >= (int64_t)c.E.n) return make_uint4(0x77777777u, 0x77777777u, 0x77777777u, 0x77777777u);
	return ld_subject(c, (int32_t)sa);
}

struct Chain { // the chain of the wavefront: everything wave-uniform
	ChainState st;
	uint32_t quarter, rest; // model_count_equal's split (src/model.c:247-253), folded into the histogram at the end
	uint32_t anchors;
	uint32_t marked; // the mark behind the 2nd anchor has been written
	uint32_t blk_base; // the block of probes in LDS answers positions blk_base ... blk_base + 63 (NOPOS: none)
	uint32_t stuck;    // the last window ended at a head whose walk gave up (W_BREAK: the chain leaves the diagonal there): the next step is mode G's --
					   // a window opened at that head again would stream, walk all its heads and not move (one such window per contig end, round 6)
	uint32_t solo;     // mode G steps in a row that settled their position alone and found no anchor (COOP_SOLO_MAX)
};

// lcp(Q + p, S + s, maxlen) (src/process.c:59-65) with all lanes: 2048 symbols per round trip
// (max_rounds: give up after that many round trips and return NOPOS)
__device__ __forceinline__ uint32_t coop_lcp(const PairCtx &c, uint32_t p, uint32_t s, uint32_t maxlen, uint32_t max_rounds = ~0u) {
	const uint32_t lane = __lane_id(), pe = p & ~1u, skip = p & 1u;
	const int64_t dg = (int64_t)s - (int64_t)p;
	CSTAT(CS_LCP, 1);
	for (uint32_t base = 0;; base += 64 * WNT) {
		const uint32_t x0 = pe + base + WNT * lane;
		CSTAT(CS_LCP_ROUNDS, 1);
		uint32_t f = 0; // first differing symbol of the lane's piece (a piece at or beyond the query's end: at once)
		if (x0 < c.qlen) {
			const uint4 d = neq32(ld_query(c, x0), ld_subject_guarded(c, (int64_t)x0 + dg));
			f = first_from(d, base == 0 && lane == 0 ? skip : 0u);
		}
		const uint64_t hit = __ballot(f < WNT);
		if (hit) {
			const uint32_t l = (uint32_t)__builtin_ctzll(hit);
			const uint32_t fl = lane_read(f, l);
			const uint32_t len = uni(pe + base + WNT * l + fl - p);
			return len < maxlen ? len : maxlen;
		}
		if (base + 64 * WNT - skip >= maxlen) return maxlen;
		if (base / (64 * WNT) + 1 >= max_rounds) return NOPOS;
	}
}

// model_count (src/model.c:309-337) of Q[q..q+len) against S[s..s+len) with all lanes
__device__ __forceinline__ void coop_count_gap(const PairCtx &c, lds_u32 *hist, uint32_t q, uint32_t s, uint32_t len) {
	const uint32_t lane = __lane_id(), qe = q & ~1u, end = q + len;
	const int64_t dg = (int64_t)s - (int64_t)q;
	for (uint32_t base = qe; base < end; base += 64 * WNT) {
		const uint32_t x0 = base + WNT * lane;
		if (x0 >= end) continue;
		const uint4 qv = ld_query(c, x0), sv = ld_subject_guarded(c, (int64_t)x0 + dg);
		const uint32_t lo = q > x0 ? q - x0 : 0u, hi = end - x0 < WNT ? end - x0 : WNT;
		for (uint32_t j = lo >> 3; 8 * j < hi; ++j) {
			const uint32_t a = lo > 8 * j ? lo - 8 * j : 0u, b = hi - 8 * j < 8 ? hi - 8 * j : 8u;
			const uint32_t qw = pick(qv, j), sw = pick(sv, j), dw = neq8(qw, sw) >> 3;
			const uint32_t ok = symbol_range(a, b) & ~(qw >> 2) & ~(sw >> 2); // both nucleotides, src/model.c:318-320
			const uint32_t eq = ok & ~dw, b0 = qw, b1 = qw >> 1;
			if (eq) {
				lds_add(&hist[0], (uint32_t)__builtin_popcount(eq & ~(b0 | b1)));
				lds_add(&hist[5], (uint32_t)__builtin_popcount(eq & b0 & ~b1));
				lds_add(&hist[10], (uint32_t)__builtin_popcount(eq & b1 & ~b0));
				lds_add(&hist[15], (uint32_t)__builtin_popcount(eq & b0 & b1));
			}
			for (uint32_t ne = ok & dw; ne; ne &= ne - 1) {
				const uint32_t k = (uint32_t)__builtin_ctz(ne);
				lds_add(&hist[(((sw >> k) & 3u) << 2) | ((qw >> k) & 3u)], 1u);
			}
		}
	}
}

// model_count_equal for LogDet and ANI (src/model.c:256-278): the nucleotides of the anchor Q[q..q+len), with all lanes
// (add = false: an anchor that was counted and should not have been is taken back)
__device__ __forceinline__ void coop_count_anchor(const PairCtx &c, lds_u32 *hist, uint32_t q, uint32_t len, bool add = true) {
	const uint32_t lane = __lane_id(), qe = q & ~1u, end = q + len;
	uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
	for (uint32_t base = qe; base < end; base += 64 * WNT) {
		const uint32_t x0 = base + WNT * lane;
		if (x0 >= end) continue;
		const uint4 qv = ld_query(c, x0);
		const uint32_t lo = q > x0 ? q - x0 : 0u, hi = end - x0 < WNT ? end - x0 : WNT;
		for (uint32_t j = lo >> 3; 8 * j < hi; ++j) {
			const uint32_t a = lo > 8 * j ? lo - 8 * j : 0u, b = hi - 8 * j < 8 ? hi - 8 * j : 8u;
			const uint32_t qw = pick(qv, j), ok = symbol_range(a, b) & ~(qw >> 2), b0 = qw, b1 = qw >> 1;
			n0 += (uint32_t)__builtin_popcount(ok & ~(b0 | b1)), n1 += (uint32_t)__builtin_popcount(ok & b0 & ~b1);
			n2 += (uint32_t)__builtin_popcount(ok & b1 & ~b0), n3 += (uint32_t)__builtin_popcount(ok & b0 & b1);
		}
	}
	n0 = wave_sum(n0), n1 = wave_sum(n1), n2 = wave_sum(n2), n3 = wave_sum(n3);
	if (lane == 0) {
		if (add) lds_add(&hist[0], n0), lds_add(&hist[5], n1), lds_add(&hist[10], n2), lds_add(&hist[15], n3);
		else lds_add(&hist[0], 0u - n0), lds_add(&hist[5], 0u - n1), lds_add(&hist[10], 0u - n2), lds_add(&hist[15], 0u - n3);
	}
}

// 8 nibbles -> 8 x 2 bits, first symbol in the low bits (the symbols must be nucleotides)
__device__ __forceinline__ uint32_t squeeze_codes(uint32_t x) {
	x &= 0x33333333u;
	x = (x | (x >> 2)) & 0x0f0f0f0fu;
	x = (x | (x >> 4)) & 0x00ff00ffu;
	return (x | (x >> 8)) & 0x0000ffffu;
}

// anchor() (src/process.c:113-123) for a walk's position p inside the window, the part that ONE dependent load
// answers: the K-mer and the symbols behind it come from the window's 2-bit codes in LDS (no load of the query), the
// table's entry settles an absent K-mer, and one that occurs once unless the match is longer than the 13 nucleotides
// its extended entry carries.  Returns false for everything else -- K-mers with several occurrences, long matches,
// windows with separators: the lane then waits until enough lanes of its wavefront need lane_probe, and they take it
// together (a path one lane in ten takes is otherwise executed on nine trips in ten).
// (on_diag: the K-mer occurs once, at p + dg -- on the window's diagonal: the match is the run of equal symbols the bits show)
// (multi_x, multi_n, multi_q: the K-mer occurs multi_n <= 4 times, at SA[multi_x ...]; multi_q = the 16 symbols behind it)
// (the part behind the query symbols: lo = the 16 symbols from p on as 2-bit codes, first in the low bits; hi = the next 16)
__device__ __forceinline__ bool coop_probe_codes(const PairCtx &c, uint32_t p, uint32_t sd, uint32_t lo, uint32_t hi, Probe &r, bool &on_diag,
												 uint32_t &multi_x, uint32_t &multi_n, uint32_t &multi_q) {
	const EsaG &E = c.E;
	const uint32_t K = (uint32_t)E.deepK, qrem = c.qlen - p;
#ifdef ANDI_COOP_STATS
#define WHY(k) atomicAdd(&g_coop_stats[k], 1ull)
#else
#define WHY(k) ((void)0)
#endif
	uint32_t y = __brev(lo); // first symbol on top, the bits of a pair swapped
	y = ((y & 0x55555555u) << 1) | ((y >> 1) & 0x55555555u);
	const uint32_t code = y >> (32 - 2 * K);
	const uint32_t behind = (uint32_t)((((uint64_t)hi << 32) | lo) >> (2 * K)); // the 16 symbols behind the K-mer
	const uint64_t raw = ld_u64_unaligned((g_u8p)(E.deep + code));
	const uint32_t x = (uint32_t)raw, ty = (uint32_t)(raw >> 32), kind = ty & 3u;
	if (kind == DEEP_FINAL) {
		r.len = ty >> 8, r.unique = (ty >> 2) & 1u, r.pos = 0;
		return !(r.unique && r.len >= (uint32_t)E.thr); // (only texts so short that K >= thr: the position is one more load)
	}
	if (kind != DEEP_SINGLE) {
		if (kind == DEEP_MULTI) WHY(CS_WHY_MULTI); else WHY(CS_WHY_OTHER);
		if (kind == DEEP_MULTI && (ty >> 8) < 4) multi_x = x, multi_n = (ty >> 8) + 1, multi_q = behind;
		return false;
	}
	if (x == p + sd) {
		on_diag = true;
		return true;
	}
	if (!E.deep_ext) { // (plain entries: the occurrence has to be looked at -- with the parked lanes, its position is known)
		multi_x = x, multi_n = 0x80000001u, multi_q = behind;
		return false;
	}
	const uint32_t nval = (ty >> 2) & 15u, ext = ty >> 6;
	const uint32_t diff = (behind ^ ext) & 0x03ffffffu;
	const uint32_t m = diff ? (uint32_t)__builtin_ctz(diff) >> 1 : 16u; // first differing nucleotide
	const uint32_t lim = nval < qrem - K ? nval : qrem - K;
	// how many symbols an entry can hold at all: 13 in the long form, what the sorter's keys had behind the K-mer in the
	// short one (andi_dev.h); an entry that holds fewer says that the text has no nucleotide there
	const uint32_t room = E.deep_ext == 2 ? (16u - K < 4u ? 16u - K : 4u) : 13u;
	r.unique = true, r.pos = x;
	if (m < lim) {
		r.len = K + m; // settled by the entry
	} else if (K + lim >= qrem) {
		r.len = qrem; // the query ends inside the match
	} else if (lim == nval && nval < room) {
		r.len = K + lim; // the text has a separator (or its end) there, the query a nucleotide
	} else {
		WHY(CS_WHY_LONG);
		return false; // all that could be compared matches: the occurrence has to be followed
	}
	return true;
}

// lane_probe with a window of its own, for the walks' rare probes that nothing shorter answers (0.4 % of them: window edges,
// separators, matches deeper than 16 symbols off the diagonal)
// (as a real call -- noinline -- the walks' loop shrinks from 4400 to 1500 instructions, but the call's register convention costs more
// than the code's size: k_coop_cold 4.12 -> 4.32 ms, k_pool_cold 4.37 -> 5.07; profiles/r07_pool/readlane.txt)
__device__ __forceinline__ Probe coop_generic_probe(const PairCtx &c, uint32_t pp) {
	LWin w;
	w.q0 = EMPTY, w.dg = NO_DIAG;
	return lane_probe(c, pp, w);
}

// The probe of a parked lane whose K-mer occurs n <= 4 times (at SA[x ...]): the longest match is the best of the
// occurrences' own matches, unique iff one attains it (as lane_probe).  The occurrence on the window's diagonal, if
// there is one, is the run of equal symbols the bits show (*diag_run; *diag_seen: a mismatch of the window ends it);
// the others are compared 16 symbols deep, two per round trip.  false: a match goes deeper than that -- lane_probe's.
// The probe of a K-mer that occurs n <= 4 times (at SA[x ...]) from what the device sorter left beside the suffix array
// (EsaDev.R2): the nucleotides behind every occurrence's K-mer, `room` of them -- ONE load of eight bytes where the suffix
// array's entries and the text behind each of them were three or more.  An occurrence whose symbols differ from the query's
// within them (or whose text ends there) is settled; the diagonal's occurrence (there is one iff the diagonal's run is at
// least K long) is the run the bits show.  false: something is left open -- an occurrence off the diagonal that matches all
// `room` symbols (one in 256) -- or the records are not there: coop_probe_multi's long way.
__device__ __forceinline__ bool coop_probe_r2(const PairCtx &c, uint32_t p, uint32_t sd, uint32_t x, uint32_t n, uint32_t behind,
											  uint32_t diag_run, bool diag_seen, Probe &r, bool &on_diag_long) {
	const EsaG &E = c.E;
	const uint32_t K = (uint32_t)E.deepK, qrem = c.qlen - p;
	on_diag_long = false;
	if (!E.R2 || (n & 0x80000000u) || K + 4 > qrem) return false;
	{
		const uint32_t room = 16u - K < 4u ? 16u - K : 4u;
		const uint64_t w = ld_u64_unaligned((g_u8p)(E.R2 + x));
		const bool diag_in = diag_run >= K; // the K-mer at p occurs on the diagonal: one of these occurrences
		uint32_t open_n = 0, bestLen = 0, bestCnt = 0, bestIdx = 0;
		for (uint32_t i = 0; i < n; ++i) {
			const uint32_t e16 = (uint32_t)(w >> (16 * i)) & 0xffffu, nval = e16 >> 8;
			const uint32_t diff = (behind ^ e16) & ((1u << (2 * nval)) - 1u);
			const uint32_t m = diff ? (uint32_t)__builtin_ctz(diff) >> 1 : nval;
			if (m == nval && nval == room) {
				++open_n; // matches as far as the record goes
				continue;
			}
			const uint32_t len = K + m; // a mismatch, or the text has no nucleotide there (m == nval < room)
			if (len > bestLen) bestLen = len, bestCnt = 1, bestIdx = i;
			else if (len == bestLen) ++bestCnt;
		}
		const bool diag_open = diag_in && (diag_run >= K + room || !diag_seen);
		if (open_n == (diag_open ? 1u : 0u)) { // nothing open but the diagonal's own occurrence
			if (diag_open) { // ... which beats every settled one
				r.unique = true, r.pos = p + sd;
				r.len = diag_seen ? diag_run : 0x40000000u;
				on_diag_long = !diag_seen;
				return true;
			}
			r.len = bestLen, r.unique = bestCnt == 1;
			if (diag_in && bestLen == diag_run && bestCnt == 1) {
				r.pos = p + sd; // the one occurrence of that length is the diagonal's
			} else {
				r.pos = (r.unique && bestLen >= (uint32_t)E.thr) ? (uint32_t)E.SA[x + bestIdx] : 0u; // (an anchor off the diagonal: rare)
			}
			return true;
		}
	}
	return false;
}

template <bool USE_R2 = true>
__device__ __forceinline__ bool coop_probe_multi(const PairCtx &c, uint32_t p, uint32_t sd, uint32_t x, uint32_t n, uint32_t behind,
												 uint32_t diag_run, bool diag_seen, Probe &r, bool &on_diag_long) {
	const EsaG &E = c.E;
	const uint32_t K = (uint32_t)E.deepK, qrem = c.qlen - p;
	on_diag_long = false;
	if (USE_R2 && coop_probe_r2(c, p, sd, x, n, behind, diag_run, diag_seen, r, on_diag_long)) return true;
	uint4 pos4 = make_uint4(x, 0, 0, 0); // (n & 0x80000000: x is the one occurrence's position itself)
	if (!(n & 0x80000000u)) pos4 = ld_u128_unaligned((g_u8p)(E.SA + x)); // (SA is padded by eight entries)
	n &= 0x7fffffffu;
	uint32_t bestLen = 0, bestCnt = 0, bestPos = 0;
	bool deep = false;
	for (uint32_t i = 0; i < n; i += 2) { // two occurrences per round trip
		const uint32_t pa = i == 0 ? pos4.x : pos4.z, pb = i == 0 ? pos4.y : pos4.w;
		const uint4 sa = ld_subject(c, (int32_t)(pa + K));
		uint4 sb = sa;
		if (i + 1 < n) sb = ld_subject(c, (int32_t)(pb + K));
		for (uint32_t h = 0; h < 2 && i + h < n; ++h) {
			const uint4 sv = h ? sb : sa;
			const uint32_t ps = h ? pb : pa;
			uint32_t len;
			if (ps == p + sd) { // the diagonal's occurrence
				len = diag_run;
				if (!diag_seen) len = 0x40000000u, on_diag_long = true; // (longer than anything 16 symbols can show)
			} else {
				const uint32_t bad_lo = sv.x & 0x44444444u, bad_hi = sv.y & 0x44444444u; // separators, the text's end
				const uint32_t stop = bad_lo ? (uint32_t)__builtin_ctz(bad_lo) >> 2 : (bad_hi ? 8u + ((uint32_t)__builtin_ctz(bad_hi) >> 2) : 16u);
				const uint32_t diff = behind ^ (squeeze_codes(sv.x) | (squeeze_codes(sv.y) << 16));
				uint32_t m = diff ? (uint32_t)__builtin_ctz(diff) >> 1 : 16u;
				if (stop < m) m = stop;
				if (m >= 16 && K + 16 < qrem) deep = true;
				len = K + m;
				if (len > qrem) len = qrem;
			}
			if (len > bestLen)
				bestLen = len, bestCnt = 1, bestPos = ps;
			else if (len == bestLen)
				++bestCnt;
		}
	}
	r.len = bestLen, r.unique = bestCnt == 1, r.pos = bestPos;
	return !deep;
}

// the record of an anchor (scan.h: the cold chain's first anchor, the state and counts right after its second)
template <class LDS>
__device__ __forceinline__ void coop_note_anchor(const ScanArgs &a, size_t slot, Chain &ch, const LDS &L) {
	const uint32_t lane = __lane_id();
	ColdMark *m = a.marks + slot * ANDI_COLD_MARKS;
	++ch.anchors;
	if (ch.anchors == 1 && lane == 0) *(uint4 *)m->first = make_uint4(ch.st.lastQ, ch.st.lastS, ch.st.lastLen, 0);
	if (ch.anchors == 2) {
		ch.marked = 1;
		if (lane == 0) {
			ChainState ms = ch.st;
			ms.pad[0] = 1, ms.pad[1] = ms.pad[2] = 0;
			m->st = ms;
		}
		if (lane < 16) {
			uint32_t v = L.hist[lane];
			if (lane == 0 || lane == 5 || lane == 10 || lane == 15) v += ch.quarter;
			if (lane == 15) v += ch.rest;
			m->counts[lane] = v;
		}
	}
}

// What an anchor at subject offset curS found at query offset st.p does to the counts (src/process.c:157-190)
template <bool EXACT, class LDS>
__device__ __forceinline__ void coop_account(const PairCtx &c, Chain &ch, LDS &L, uint32_t curS) {
	ChainState &st = ch.st;
	const uint32_t endS = st.lastS + st.lastLen, endQ = st.lastQ + st.lastLen;
	auto count_last = [&]() { // model_count_equal of the last anchor
		if constexpr (EXACT) coop_count_anchor(c, (lds_u32 *)L.hist, st.lastQ, st.lastLen);
		else ch.quarter += st.lastLen >> 2, ch.rest += st.lastLen & 3u;
	};
	if (curS > endS && st.p - endQ == curS - endS && (curS < c.border) == (st.lastS < c.border)) {
		count_last();
		coop_count_gap(c, (lds_u32 *)L.hist, endQ, endS, st.p - endQ);
		CSTAT(CS_G_GAPS, 1);
		st.lwra = 1;
	} else {
		if (st.lwra || st.lastLen >= 2 * c.thr) count_last();
		st.lwra = 0;
	}
}

// substitutions of Q[q..q+len) against S[s..s+len) taken back from the counts (all lanes, 32 positions each; what sweep S counted of
// a stretch that is counted nowhere)
__device__ __forceinline__ void pool_uncount_coop(const PairCtx &c, lds_u32 *hist, uint32_t q, uint32_t s, uint32_t len) {
	const uint32_t lane = __lane_id(), qe = q & ~1u, end = q + len;
	const int64_t dg = (int64_t)s - (int64_t)q;
	for (uint32_t base = qe; base < end; base += 64 * WNT) {
		const uint32_t x0 = base + WNT * lane;
		if (x0 >= end) continue;
		const uint4 qv = ld_query(c, x0), sv = ld_subject_guarded(c, (int64_t)x0 + dg);
		const uint32_t lo = q > x0 ? q - x0 : 0u, hi = end - x0 < WNT ? end - x0 : WNT;
		for (uint32_t j = lo >> 3; 8 * j < hi; ++j) {
			const uint32_t a = lo > 8 * j ? lo - 8 * j : 0u, b = hi - 8 * j < 8 ? hi - 8 * j : 8u;
			const uint32_t qw = pick(qv, j), sw = pick(sv, j), dw = neq8(qw, sw) >> 3;
			for (uint32_t ne = symbol_range(a, b) & ~(qw >> 2) & ~(sw >> 2) & dw; ne; ne &= ne - 1) {
				const uint32_t k = (uint32_t)__builtin_ctz(ne);
				lds_add(&hist[(((sw >> k) & 3u) << 2) | ((qw >> k) & 3u)], 0u - 1u);
			}
		}
	}
}

// the equal nucleotides of Q[q..q+len) against S[s..s+len) into the diagonal cells (all lanes, 32 positions each; a stretch longer
// than its head's record)
__device__ __forceinline__ void pool_count_equal_coop(const PairCtx &c, uint32_t q, uint32_t s, uint32_t len, uint32_t &n0, uint32_t &n1, uint32_t &n2, uint32_t &n3) {
	const uint32_t lane = __lane_id(), qe = q & ~1u, end = q + len;
	const int64_t dg = (int64_t)s - (int64_t)q;
	for (uint32_t base = qe; base < end; base += 64 * WNT) {
		const uint32_t x0 = base + WNT * lane;
		if (x0 >= end) continue;
		const uint4 qv = ld_query(c, x0), sv = ld_subject_guarded(c, (int64_t)x0 + dg);
		const uint32_t lo = q > x0 ? q - x0 : 0u, hi = end - x0 < WNT ? end - x0 : WNT;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const uint32_t a = lo > 8 * j ? (lo - 8 * j < 8 ? lo - 8 * j : 8u) : 0u, b = hi > 8 * j ? (hi - 8 * j < 8 ? hi - 8 * j : 8u) : 0u;
			if (a >= b) continue;
			const uint32_t qw = pick(qv, j), sw = pick(sv, j), dw = neq8(qw, sw) >> 3;
			const uint32_t eq = symbol_range(a, b) & ~(qw >> 2) & ~(sw >> 2) & ~dw, b0 = qw, b1 = qw >> 1;
			n0 += (uint32_t)__builtin_popcount(eq & ~(b0 | b1)), n1 += (uint32_t)__builtin_popcount(eq & b0 & ~b1);
			n2 += (uint32_t)__builtin_popcount(eq & b1 & ~b0), n3 += (uint32_t)__builtin_popcount(eq & b0 & b1);
		}
	}
}

// The texts bit-sliced (andi_dev.h: EsaDev.P): 32 symbols of the query from x0 (a multiple of 32) / of the subject from any offset s
// (>= -32; at and beyond the text's end: NUL, all ones) as bit 0, 1, 2 of the symbols
struct Planes {
	uint32_t b0, b1, b2;
};
__device__ __forceinline__ Planes ld_query_planes(const PairCtx &c, uint32_t x0) {
	const g_u32p p = c.Qp + 3 * (x0 >> 5);
	Planes r;
	r.b0 = p[0], r.b1 = p[1], r.b2 = p[2];
	return r;
}
__device__ __forceinline__ Planes ld_subject_planes(const PairCtx &c, int64_t s) {
	Planes r;
	r.b0 = r.b1 = r.b2 = ~0u;
	if (s >= (int64_t)c.E.n) return r;
	const int32_t blk = (int32_t)(s >> 5);
	const uint32_t sh = (uint32_t)s & 31u;
	const g_u32p p = c.E.P + 3 * blk; // (blk >= -1: a block of padding lies in front)
	const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], n0 = p[3], n1 = p[4], n2 = p[5];
	r.b0 = __builtin_amdgcn_alignbit(n0, a0, sh), r.b1 = __builtin_amdgcn_alignbit(n1, a1, sh), r.b2 = __builtin_amdgcn_alignbit(n2, a2, sh);
	return r;
}
// The same two fetches as the words come from memory -- no use of a loaded value, so that the loads of round t + 1 stay in flight
// while round t is worked on (ld_subject_planes shifts its words at once: the wait for them then stands right behind the loads,
// and sweep S paid the stream's whole latency every round; round 6) -- and what turns them into planes.
// (aligned(4): the words lie at 4-byte multiples only -- three per block of 32 symbols)
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4), aligned(4)));
struct RawPlanes { // (whole registers tuples as the loads deliver them: taken apart only where they are used -- a struct of nine words was
	u32x3_t q;     // copied word by word at the loop's head, with the wait for the loads in front of the copies)
	u32x4_t a;     // subject block: planes 0, 1, 2 and plane 0 of the next block
	u32x2_t n;     // planes 1, 2 of the next block
};
__device__ __forceinline__ void ld_raw_planes(const PairCtx &c, uint32_t x0, int64_t s, RawPlanes &r) {
	r.q = *(const __attribute__((address_space(1))) u32x3_t *)(c.Qp + 3 * (x0 >> 5));
	r.a = (u32x4_t)(~0u), r.n = (u32x2_t)(~0u); // (at and beyond the text's end: NUL, all ones)
	if (s < (int64_t)c.E.n) {
		const g_u32p p = c.E.P + 3 * (int32_t)(s >> 5); // (block >= -1: a block of padding lies in front)
		r.a = *(const __attribute__((address_space(1))) u32x4_t *)p;
		r.n = *(const __attribute__((address_space(1))) u32x2_t *)(p + 4);
	}
}
__device__ __forceinline__ void planes_of(const RawPlanes &r, uint32_t sh, Planes &q, Planes &s) {
	q.b0 = r.q.x, q.b1 = r.q.y, q.b2 = r.q.z;
	s.b0 = __builtin_amdgcn_alignbit(r.a.w, r.a.x, sh), s.b1 = __builtin_amdgcn_alignbit(r.n.x, r.a.y, sh), s.b2 = __builtin_amdgcn_alignbit(r.n.y, r.a.z, sh);
}
// the substitutions among the positions `mm` (query symbol != subject symbol, both nucleotides) by kind, into twelve counters:
// kind k = 3 * (query nucleotide) + (rank of the subject's among the three others) -- no loop over the mismatches, no LDS
struct SubstAcc {
	uint32_t n[12];
};
__device__ __forceinline__ void subst_count(SubstAcc &acc, uint32_t mm, const Planes &q, const Planes &s) {
	const uint32_t qA = mm & ~q.b1 & ~q.b0, qC = mm & ~q.b1 & q.b0, qG = mm & q.b1 & ~q.b0, qT = mm & q.b1 & q.b0;
	const uint32_t sA = ~s.b1 & ~s.b0, sC = ~s.b1 & s.b0, sG = s.b1 & ~s.b0, sT = s.b1 & s.b0;
	acc.n[0] += (uint32_t)__builtin_popcount(qA & sC), acc.n[1] += (uint32_t)__builtin_popcount(qA & sG), acc.n[2] += (uint32_t)__builtin_popcount(qA & sT);
	acc.n[3] += (uint32_t)__builtin_popcount(qC & sA), acc.n[4] += (uint32_t)__builtin_popcount(qC & sG), acc.n[5] += (uint32_t)__builtin_popcount(qC & sT);
	acc.n[6] += (uint32_t)__builtin_popcount(qG & sA), acc.n[7] += (uint32_t)__builtin_popcount(qG & sC), acc.n[8] += (uint32_t)__builtin_popcount(qG & sT);
	acc.n[9] += (uint32_t)__builtin_popcount(qT & sA), acc.n[10] += (uint32_t)__builtin_popcount(qT & sC), acc.n[11] += (uint32_t)__builtin_popcount(qT & sG);
}
// the counters of all lanes into the 4 x 4 counts (cell = subject nucleotide << 2 | query nucleotide, src/model.c:309-337), added or taken back
__device__ __forceinline__ void subst_flush(const SubstAcc &acc, lds_u32 *hist, bool add) {
	const uint32_t lane = __lane_id();
#pragma unroll
	for (int k = 0; k < 12; ++k) {
		const uint32_t qn = (uint32_t)k / 3, r = (uint32_t)k % 3, sn = r + (r >= qn ? 1u : 0u);
		const uint32_t v = wave_sum(acc.n[k]);
		if (lane == 0 && v) lds_add(&hist[(sn << 2) | qn], add ? v : 0u - v);
	}
}

// 16 bits -> the even bits of a word (bit k to bit 2k)
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
	x &= 0xffffu;
	x = (x | (x << 8)) & 0x00ff00ffu;
	x = (x | (x << 4)) & 0x0f0f0f0fu;
	x = (x | (x << 2)) & 0x33333333u;
	return (x | (x << 1)) & 0x55555555u;
}

// ------------------------------------------------------------------ the walks' verdicts (mode W's sweep W; mode P's keeps the same as text of its own, coop_pool.h)
// A walk from the head at e stands at p and has found an anchor there on the window's diagonal (subject position p + sd); Xl, nX: the
// last anchor it met off the diagonal (0: none) and how many.  It lands there (`lucky`: where the anchor ends is settled later) unless
// the anchor lies on the other strand than the one before the head -- a right anchor only on the same strand, src/process.c:162 -- or
// the anchor off the diagonal is counted by itself
__device__ __forceinline__ uint32_t walk_on_diag(const PairCtx &c, uint32_t sd, uint32_t e, uint32_t p, uint32_t Xl, uint32_t nX, bool lucky) {
	const bool same_side = (p + sd < c.border) == (e + sd <= c.border);
	return (!same_side || (Xl && Xl >= 2 * c.thr)) ? W_BREAK : (W_OK | (lucky ? W_LUCKY : 0u) | (Xl ? W_HADX : 0u) | (nX << W_NX_SHIFT));
}

// What a step's outcome does to its walk: on with the next position, or the head's result (res: how it ended, ra: where it landed, rlen: the
// length of the anchor it landed on).  have: pr is the probe's answer for p; (Xq, Xs, Xl): the last anchor off the diagonal
__device__ __forceinline__ void walk_settle(const PairCtx &c, uint32_t sd, uint32_t e, uint32_t &p, uint32_t &Xq, uint32_t &Xs, uint32_t &Xl, uint32_t &nX,
											uint32_t &res, uint32_t &ra, uint32_t &rlen, const Probe &pr, bool have) {
	const uint32_t thr = c.thr;
	if (!res && have) {
		if (pr.unique && pr.len >= thr) {
			if (pr.pos == p + sd) { // on the diagonal
				res = walk_on_diag(c, sd, e, p, Xl, nX, rlen == NOPOS);
				if (res != W_BREAK) ra = p, rlen = rlen == NOPOS ? 0u : pr.len;
			} else {
				const uint32_t endS = Xs + Xl, endQ = Xq + Xl;
				if (Xl && ((pr.pos > endS && p - endQ == pr.pos - endS && (pr.pos < c.border) == (Xs < c.border)) || Xl >= 2 * thr))
					res = W_BREAK; // a right anchor off the diagonal (its gap is not in the window), or an anchor that is counted by itself
				else if (++nX > COOP_MAX_X)
					res = W_BREAK;
				else
					Xq = p, Xs = pr.pos, Xl = pr.len;
			}
		}
		if (!res) p += pr.len + 1;
	}
	if ((res & W_LUCKY) && (ra + sd < c.border) != (e + sd <= c.border)) res = W_BREAK; // (where a lucky anchor was seen: the strands again)
}

// ------------------------------------------------------------------ one segment
// The cold chain of segment wseg of subject sub: mode G until the chain has a diagonal, windows while it stays on it, then what pass B
// reads.  `win` is the mode's way with windows (coop_window.h: WindowsLds, coop_pool.h: WindowsPool), a plain struct:
//   win.begin(ch)                  the chain has a diagonal: a run of windows begins
//   win.window(a, c, ch, L, end)   one window; true if the chain moved.  The loop around it -- while the chain moves, the pair has not been
//                                  handed back and the chain is not stuck -- is here, once: with the policy returning from inside a loop of
//                                  its own k_coop_cold spilled three to seven more registers (profiles/r11_coop_segment.md)
//   Windows::COUNTS_EQUAL          win.same[4] holds equal pairs the windows found in gaps, by nucleotide: added to the counts at the end
// (both modes synchronise alike: the wave_sync() at the top was mode P's alone, the one at the end stands in front of the diagnostics)
template <bool EXACT, class LDS, class Windows>
__device__ __forceinline__ void coop_segment(const ScanArgs &a, LDS &L, uint32_t sub, uint32_t wseg, Windows &win) {
	if (a.subjects[sub].mode != ANDI_MODE_PROBE) return;
	const uint32_t qidx = uni(a.seg2query[wseg]);
	if (a.self[sub] == (int64_t)qidx) return;
	const uint32_t seg_in_q = wseg - uni(a.qseg_start[qidx]);
	PairCtx c = make_ctx(a, sub, qidx);
	const uint32_t start = seg_in_q * a.seg, end = start + a.seg < c.qlen ? start + a.seg : c.qlen;
	auto slot_of = [&]() { return (size_t)sub * a.total_segs + wseg; }; // (formed where it is used: not held through the loop)
	const uint32_t n = (uint32_t)c.E.n, thr = c.thr;

	// a routed call (scan.h): the pairs k_pair_estimate marked for this kernel; a wavefront that meets what the kernel is slow
	// at hands its PAIR back to the lane scan -- a mark all the pair's wavefronts look at
	const uint32_t lane = __lane_id();
	uint8_t *route = a.route ? a.pair_class + (size_t)sub * a.nq + qidx : nullptr;
	auto give_up = [&]() {
		if (lane == 0) a.restitch_count[ANDI_ROUTE_ANY_LEFT] = 1;
		if (lane == 0) __hip_atomic_store(route, (uint8_t)(__hip_atomic_load(route, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | ANDI_ROUTE_LEFT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	};
	auto given_up = [&]() { return route && (uni(__hip_atomic_load(route, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & (ANDI_ROUTE_COOP | ANDI_ROUTE_LEFT)) != ANDI_ROUTE_COOP; };
	TICK(tpro);
	if (given_up()) return;
	wave_sync();
	if (lane < 16) L.hist[lane] = 0;
	Chain ch;
	ch.st = seg_in_q == 0 ? initial_state() : cold_state(start, n);
	ch.quarter = ch.rest = ch.anchors = ch.marked = 0, ch.blk_base = NOPOS, ch.stuck = 0, ch.solo = 0;
	ChainState &st = ch.st;
	wave_sync();

	CSTAT(CS_SEGMENTS, 1);
	TOCK(tpro, PH_PROLOGUE);
	TICK(tall);
	uint32_t my_g = 0;
	while (st.p < end) {
		CSTAT(CS_G_STEPS, 1);
		CSTAT(CS_G_FIRST, my_g == 0);
		++my_g;
		if (route) {
			if (my_g > a.route_giveup + (a.seg >> 12)) return give_up(); // (a few more per window the segment holds)
			if (given_up()) return;
		}
		// ---- one step of mode G (src/process.c:153-197)
		TICK(tg);
		bool found = false, lucky = false;
		uint32_t curS = 0, curLen = 0;
		// The step follows at most one diagonal with all lanes (tryS: where st.p lies on it; NOPOS: none) -- the last anchor's (lucky_anchor),
		// or that of the one occurrence a probe of st.p alone found (`probed`).  Without an answer for st.p in the block, st.p alone comes first
		// (COOP_SOLO_CAP symbols deep, as k_lane_cold's own probe, scan_lane.hip; every lane takes the same probe, which costs the wavefront what
		// one lane's would and needs no mask of its own -- with lane 0 alone k_coop_cold<5, false> spilled one register more): at a segment's
		// start in homologous sequence the answer is a unique long match, and the chain jumps past what the probes of the 63 positions
		// behind it would have found, each followed to its end -- the wavefront executes the union of what its lanes do.  The 64
		// probes of the next 64 positions at once (the chain then hops through the answers) where that is of no use: several occurrences match
		// as far as the cap, or the last COOP_SOLO_MAX such steps found no anchor.  ONE place where the wavefront follows a diagonal and ONE
		// where it probes, whichever way the step takes.
		// The loop's trips, two at the most -- a trip ends the step (break) or says what the next one does (continue):
		//   1. the lucky attempt, if one applies (tryS); an anchor ends the step.  Else the probe: from the block if it answers st.p; of st.p alone
		//      (`alone`), which ends the step unless its match reaches the cap; or the block of 64 made now, which ends it.
		//   2. behind a probe of st.p alone that reached the cap -- one occurrence did: tryS is its diagonal, coop_lcp follows it and ends the step
		//      (`probed`); several did: `alone` is off, and the trip makes the block and ends the step.
		// (Every lane of a probe of st.p alone runs lane_probe whole, sa_range_match included: a separator inside the K-mer, fewer than K symbols
		// left of the query and K-mers with more than MULTI_MAX occurrences are not held back for the block -- a capped probe is exact below the
		// cap whichever way lane_probe takes, and such steps are rare; profiles/r12_cold_start.md.)
		uint32_t tryS = lucky_applies(st, n, thr) ? st.lastS + (st.p - st.lastQ) : NOPOS;
		bool probed = false, alone = ch.solo < COOP_SOLO_MAX; // alone: this step may probe st.p by itself (ch.solo counts such steps in a row)
		for (;;) {
			if (tryS != NOPOS) {
				curS = tryS;
				curLen = coop_lcp(c, st.p, curS, c.qlen - st.p, route ? COOP_TRIAL_LCP : ~0u);
				if (curLen == NOPOS) return give_up();
				found = curLen >= thr;
				if (probed) {
					TOCK(tg, PH_G_SOLO_LCP);
					break; // the probe's one occurrence, followed to its end
				}
				TOCK(tg, PH_G_LCP);
				lucky = found;
				if (found) break;
				tryS = NOPOS;
			}
			const bool answered = ch.blk_base != NOPOS && st.p >= ch.blk_base && st.p - ch.blk_base < 64;
			if (answered) alone = false;
			if (!answered) {
				const uint32_t p = st.p + (alone ? 0u : lane);
				Probe pr;
				pr.len = 0, pr.pos = 0, pr.unique = false;
				if (p < c.qlen) {
					LWin w;
					w.q0 = EMPTY, w.dg = NO_DIAG;
					pr = lane_probe(c, p, w, alone ? COOP_SOLO_CAP : ~0u);
				}
				if (alone) {
					CSTAT(CS_SOLO, 1);
					++ch.solo;
					curLen = uni(pr.len), curS = uni(pr.pos);
					const bool uq = uni(pr.unique ? 1u : 0u) != 0;
					TOCK(tg, PH_G_SOLO);
					if (curLen >= COOP_SOLO_CAP && COOP_SOLO_CAP < c.qlen - st.p) {
						if (uq) { // the one occurrence that matches that far: its match to its end, with all lanes
							CSTAT(CS_SOLO_LCP, 1);
							tryS = curS, probed = true;
						} else { // several do: the whole answer is the block's
							CSTAT(CS_SOLO_BLOCK, 1);
							alone = false;
						}
						continue;
					}
					found = uq && curLen >= thr;
					break;
				}
				CSTAT(CS_BLOCKS, 1); // the next 64 positions' answers at once
				wave_sync();
				L.pl[lane] = pr.len | (pr.unique ? 0x80000000u : 0u), L.pp[lane] = pr.pos;
				ch.blk_base = st.p;
				wave_sync();
				TOCK(tg, PH_G_BLOCK);
			}
			const uint32_t v = uni(L.pl[st.p - ch.blk_base]);
			curLen = v & 0x7fffffffu, curS = uni(L.pp[st.p - ch.blk_base]);
			found = (v >> 31) && curLen >= thr;
			break;
		}
		if (found) {
			ch.solo = 0;
			coop_account<EXACT>(c, ch, L, curS);
			st.lastS = curS, st.lastQ = st.p, st.lastLen = curLen;
		}
		st.p += curLen + 1;
		if (found) {
			wave_sync();
			coop_note_anchor(a, slot_of(), ch, L);
		}
		TOCK(tg, PH_G_NOTES);
		// ---- windows one after the other while the chain stays canonical on the diagonal and moves
		if (found && lucky) {
			win.begin(ch);
			while (st.p < end && st.lastQ + st.lastLen < c.qlen && win.window(a, c, ch, L, end)) {
				if (given_up()) return;
				if (ch.stuck) break; // (the chain stands at a head whose walk gave up: mode G's step, not another window at the same place)
			}
		}
	}

	TOCK(tall, PH_LOOP);
	TICK(tepi);
	wave_sync();
#ifdef ANDI_COOP_STATS
	if (lane == 0) atomicMax(&g_coop_max[0], my_g);
#endif
	(void)my_g;
	// ---- what pass B reads (scan.h)
	const size_t slot = slot_of();
	if (lane == 0) {
		ColdMark *m = a.marks + slot * ANDI_COLD_MARKS;
		if (!ch.marked) m->st.pad[0] = 0; // unused mark
		ChainState out = st;
		out.pad[0] = 0, out.pad[1] = ch.anchors < 255 ? ch.anchors : 255, out.pad[2] = 0;
		a.cold_exit[slot] = out;
		a.exit_p[slot] = st.p;
	}
	if (lane < 16) {
		uint32_t v = L.hist[lane];
		if (lane == 0 || lane == 5 || lane == 10 || lane == 15) v += ch.quarter;
		if (lane == 15) v += ch.rest;
		if constexpr (Windows::COUNTS_EQUAL) v += lane == 0 ? win.same[0] : lane == 5 ? win.same[1] : lane == 10 ? win.same[2] : lane == 15 ? win.same[3] : 0u;
		a.cold_counts[slot * 16 + lane] = v;
	}
	TOCK(tepi, PH_EPILOGUE);
}

} // namespace
