// coop_window.h -- pass A with one wavefront per chain, the window in LDS (mode W; scan_coop.hip's first comment describes it).
// On top of coop_dev.h alone: the window's memory, its bits' lookups, the walks' probe from the codes in LDS, coop_window, and WindowsLds,
// which hands coop_window to the segment driver.
#pragma once
#include "coop_dev.h"

namespace {

// (LDS bounds the window at eight wavefronts per SIMD: 5120 bytes each.  Five chunks with 112 heads are 5108 bytes; fewer heads per chunk
// cost more than the longer window gains -- at four chunks 16 per chunk: + 4 %, 20: + 1 %, 32: - 0.5 %; at five 100 heads drop 6 % of
// them (a dropped head ends its window), 112 with the list of stretches counted nowhere at 12 instead of 32: - 2 %; profiles/r07_coop/README.md)
#define COOP_HCAP (NCH <= 2 ? 64u : NCH == 5 ? 112u : 24u * NCH) /* heads of a window that are walked (more: the window ends at the first one dropped) */
template <int NCH>
struct CoopLds {
	uint32_t mbits[64 * NCH + 4]; // mismatch bits of the window, bit (x - wbase); the words behind it stay 0: nothing known there
	union {
		uint32_t q2[128 * NCH + 4]; // the window's query symbols as 2-bit codes, 16 per word, symbol k of a word at bits 2k, 2k + 1: for the walks;
		uint32_t ebits[64 * NCH];   // once they are done: the stretches behind the heads the chain came by, [head, landing): counted as gaps -- except
	};
	uint32_t kpos[COOP_KCAP];     // those that start at one of these positions (the walk met anchors off the diagonal): counted nowhere
	uint32_t nhadx;               // walks of the window that ended that way (at most COOP_KCAP: the others give up)
	union {
		struct {
			uint32_t hend[COOP_HCAP]; // from the walk: length of the anchor it landed on (W_LUCKY: not known yet); then: where that anchor ends
			uint16_t ha[COOP_HCAP];   // landing position of the head's walk - wbase
			uint16_t hflag[COOP_HCAP];
			uint16_t hpos[COOP_HCAP]; // the head's position - wbase
		};
		struct {
			uint32_t pl[64], pp[64]; // mode G (no window open): the block of probes, length | unique << 31, position
		};
	};
	uint32_t hist[16];
};


// first mismatch bit of the window at or after position x (x >= wbase), NOPOS if the window shows none
template <int NCH>
__device__ __forceinline__ uint32_t coop_next_mismatch(const CoopLds<NCH> &L, uint32_t wbase, uint32_t x) {
	const uint32_t lane = __lane_id(), o = x - wbase;
	for (uint32_t w0 = o >> 5; w0 < 64 * NCH; w0 += 64) {
		const uint32_t w = w0 + lane;
		uint32_t v = w < 64 * NCH ? L.mbits[w] : 0u;
		if (w == (o >> 5)) v &= ~0u << (o & 31u);
		const uint64_t hit = __ballot(v != 0);
		if (hit) {
			const uint32_t l = (uint32_t)__builtin_ctzll(hit);
			const uint32_t vl = lane_read(v, l);
			return uni(wbase + 32 * (w0 + l) + (uint32_t)__builtin_ctz(vl));
		}
	}
	return NOPOS;
}

// last mismatch bit of the window before position x (x > wbase), NOPOS if none
template <int NCH>
__device__ __forceinline__ uint32_t coop_prev_mismatch(const CoopLds<NCH> &L, uint32_t wbase, uint32_t x) {
	const uint32_t lane = __lane_id(), o = x - wbase; // bits 0 .. o - 1
	if (o == 0) return NOPOS;
	const uint32_t top = (o - 1) >> 5;
	for (int32_t w0 = (int32_t)top; w0 >= 0; w0 -= 64) {
		const int32_t w = w0 - (int32_t)lane;
		uint32_t v = w >= 0 && w < 64 * NCH ? L.mbits[w] : 0u;
		if (w == (int32_t)top && ((o - 1) & 31u) != 31u) v &= (2u << ((o - 1) & 31u)) - 1u;
		const uint64_t hit = __ballot(v != 0);
		if (hit) {
			const uint32_t l = (uint32_t)__builtin_ctzll(hit);
			const uint32_t vl = lane_read(v, l);
			return uni(wbase + 32 * (uint32_t)(w0 - (int32_t)l) + 31u - (uint32_t)__builtin_clz(vl));
		}
	}
	return NOPOS;
}

template <int NCH>
__device__ __forceinline__ bool coop_probe_fast(const PairCtx &c, const CoopLds<NCH> &L, uint32_t wbase, bool clean, uint32_t p, uint32_t sd, Probe &r, bool &on_diag,
												uint32_t &multi_x, uint32_t &multi_n, uint32_t &multi_q) {
	on_diag = false, multi_n = 0;
	const uint32_t o = p - wbase;
	// (a window with a separator -- joined contigs: every probe of it goes the long way.  Per-word flags in LDS were built and measured
	// in round 6: 1 % faster on genomes of 100 contigs, 1.7 % slower on whole ones -- profiles/r07_pool/join_ab.txt; k_pool_cold, whose
	// windows are sixteen times as long, keeps a flag per head's record)
	if (!(clean && o + 32 <= 2048 * NCH && p + 32 <= c.qlen)) {
		WHY(CS_WHY_PRE);
		return false;
	}
	const uint32_t j = o >> 4, sh = 2 * (o & 15u);
	const uint32_t w0 = L.q2[j], w1 = L.q2[j + 1], w2 = L.q2[j + 2];
	return coop_probe_codes(c, p, sd, __builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh), r, on_diag, multi_x, multi_n, multi_q);
}


// The twelve counters of all lanes into the 4 x 4 counts in LDS (cell = subject nucleotide << 2 | query nucleotide, src/model.c:309-337), added or
// taken back.  A window of mode W has at most 32 NCH <= 256 mismatches per lane and kind: two counters to a register, six sums over the lanes;
// the sums go to lanes 0 ... 11, which add them to their cells in ONE instruction (subst_flush's conditional add per counter by lane 0 cost as
// much as its scans; every lane adding its own counters to the twelve cells -- 64 adds to one address each -- took the kernel from 3.7 to 4.3 ms).
__device__ __forceinline__ void subst_flush_pairs(const SubstAcc &acc, lds_u32 *hist, bool add) {
	const uint32_t lane = __lane_id();
	uint32_t w = 0; // lane k < 6: the sums of counters k (low half) and k + 6 (high half)
#pragma unroll
	for (int k = 0; k < 6; ++k) {
		const uint32_t sum = wave_sum(acc.n[k] | (acc.n[k + 6] << 16));
		w = lane == (uint32_t)k ? sum : w;
	}
	const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x116, 0xf, 0xf, false); // row_shr:6: lane k + 6 sees lane k's
	const uint32_t v = lane < 6 ? w & 0xffffu : up >> 16;
	const uint32_t qn = lane / 3, r = lane - 3 * qn, sn = r + (r >= qn ? 1u : 0u);
	if (lane < 12 && v) lds_add(&hist[(sn << 2) | qn], add ? v : 0u - v);
}

// A wave-uniform value as a value of its own from here on: the register allocator weighs it by the loop that follows, not by the whole kernel
// (an empty statement; nothing is emitted for it but the copy)
template <class T>
__device__ __forceinline__ T own_sgpr(T x) {
	asm volatile("" : "+s"(x));
	return x;
}

// ------------------------------------------------------------------ mode W
// The chain stands at a canonical state of diagonal dg: st.p = e0 + 1 behind the anchor [lastQ, e0), e0 a mismatch
// of the diagonal.  Returns true if the chain moved; st is a genuine loop-top state either way.
template <int NCH, bool EXACT>
__device__ __forceinline__ bool coop_window(const ScanArgs &a, const PairCtx &c, Chain &ch, CoopLds<NCH> &L, uint32_t end) {
	static_assert(64 * 32 * NCH < 65536 && 2048 * NCH <= 65536, "two 16-bit sums to a register (subst_flush_pairs, the stretches' equal symbols); offsets into a window are 16 bits");
	const uint32_t lane = __lane_id(), thr = c.thr, n = (uint32_t)c.E.n;
	ChainState &st = ch.st;
	const int64_t dg = (int64_t)st.lastS - (int64_t)st.lastQ;
	const uint32_t sd = st.lastS - st.lastQ; // subject position of window position x: x + sd (x + dg >= lastS >= 0: 32 bits do)
	const uint32_t e0 = st.lastQ + st.lastLen;
	const uint32_t wbase = e0 & ~31u;
	constexpr uint32_t W = 2048 * NCH;

	TICK(tph);
	// ---- the bits: position x of the window against subject position x + dg; the query's symbols as 2-bit codes
	uint32_t dirty = 0; // a query symbol of the window that is no nucleotide ('!' of joined contigs): the walks then read the query itself
	lds_u32 *hist = (lds_u32 *)L.hist;
	// RAW / JC / Kimura (round 6): the texts are streamed BIT-SLICED (EsaDev.P, ScanArgs.qplanes: three words per 32 symbols), as k_pool_cold's
	// sweep S does -- the mismatch bits are three instructions per word, and every mismatch of the window is counted as a single-position gap
	// at once, by kind, without a loop (subst_count): what the chain turns out not to reach, and the stretches that are counted nowhere, are
	// taken back below.  Until then the counting pass fetched both texts a second time for every word with a mismatch and every stretch's lane
	// walked its text symbol by symbol: 22 % of the kernel (profiles/r07_coop/README.md).  LogDet / ANI keep the 4-bit stream.
	// the mismatches of [from, end of the window) out of the counts again
	auto take_back = [&](uint32_t from) {
		if constexpr (!EXACT) {
			if ((from - wbase) / 2048u >= (uint32_t)NCH) return;
			SubstAcc acc;
#pragma unroll
			for (int k = 0; k < 12; ++k) acc.n[k] = 0;
			for (uint32_t t = (from - wbase) / 2048u; t < (uint32_t)NCH; ++t) {
				const uint32_t x0 = wbase + 2048 * t + WNT * lane;
				if (x0 >= c.qlen || x0 + WNT <= from) continue;
				const Planes qv = ld_query_planes(c, x0), sv = ld_subject_planes(c, (int64_t)x0 + dg);
				uint32_t mc = ((qv.b0 ^ sv.b0) | (qv.b1 ^ sv.b1) | (qv.b2 ^ sv.b2)) & ~(qv.b2 | sv.b2);
				if (c.qlen - x0 < WNT) mc &= ~(~0u << (c.qlen - x0));
				if (from > x0) mc &= ~0u << (from - x0);
				subst_count(acc, mc, qv, sv);
			}
			subst_flush_pairs(acc, hist, false);
		}
	};
	if constexpr (!EXACT) {
		SubstAcc acc;
#pragma unroll
		for (int k = 0; k < 12; ++k) acc.n[k] = 0;
		const uint32_t sh = (uint32_t)((int64_t)(wbase + WNT * lane) + dg) & 31u; // (a lane's subject offset keeps its low five bits from chunk to chunk; from the
		// kernel's own dg, not the loop's copy below: that cost the kernel 12 more bytes of scratch and doubled its lane moves)
		// The loop's wave-uniform values as values of its own (own_sgpr): the kernel's are spilled to lanes of a register, and every iteration read
		// the query's length, its two pointers and the diagonal back from there, nine lane moves per chunk.
		const uint32_t qlen = own_sgpr(c.qlen);
		const g_u32p Qp = own_sgpr(c.Qp), Qc = own_sgpr(c.Qc), Sp = own_sgpr(c.E.P);
		const int64_t dgw = own_sgpr(dg), sn = own_sgpr((int64_t)c.E.n);
		// (wbase = e0 & ~31: the window's first word alone holds positions before e0, which are none of the window's business)
		uint32_t keep = lane == 0 ? ~0u << (e0 - wbase) : ~0u;
		// (not unrolled: by two, every iteration ended with thirteen moves of the twelve counters and `dirty` back to the registers the loop's
		// head expects; unrolled in full, the kernel's scratch grows from 56 to 128 bytes per lane -- profiles/r10_coop_valu.md)
#pragma unroll 1
		for (int ck = 0; ck < NCH; ++ck) {
			const uint32_t x0 = wbase + 2048 * ck + WNT * lane;
			uint32_t m = ~0u, mc = 0; // positions at and beyond the query's end: lcp() stops there; mc: the mismatches that are counted
			uint2 codes = make_uint2(0, 0);
			if (x0 < qlen) {
				// (the codes' load issued with the planes': behind them it would wait a second round trip)
				const u32x2_t cv = *(const __attribute__((address_space(1))) u32x2_t *)(Qc + 2 * (x0 >> 5));
				RawPlanes raw;
				raw.q = *(const __attribute__((address_space(1))) u32x3_t *)(Qp + 3 * (x0 >> 5));
				raw.a = (u32x4_t)(~0u), raw.n = (u32x2_t)(~0u); // (at and beyond the text's end: NUL, all ones)
				const int64_t s = (int64_t)x0 + dgw;
				if (s < sn) {
					const g_u32p p = Sp + 3 * (int32_t)(s >> 5); // (block >= -1: a block of padding lies in front)
					raw.a = *(const __attribute__((address_space(1))) u32x4_t *)p;
					raw.n = *(const __attribute__((address_space(1))) u32x2_t *)(p + 4);
				}
				Planes qv, sv;
				planes_of(raw, sh, qv, sv);
				codes = make_uint2(cv.x, cv.y);
				m = (qv.b0 ^ sv.b0) | (qv.b1 ^ sv.b1) | (qv.b2 ^ sv.b2);
				mc = m & ~(qv.b2 | sv.b2); // both nucleotides (src/model.c:318-320)
				uint32_t inq = ~0u;
				if (qlen - x0 < WNT) inq = ~(~0u << (qlen - x0)), m |= ~inq, mc &= inq;
				dirty |= qv.b2 & inq;
				subst_count(acc, mc & keep, qv, sv);
			}
			L.mbits[64 * ck + lane] = m & keep;
			*(uint2 *)&L.q2[2 * (64 * ck + lane)] = codes;
			keep = ~0u;
		}
		subst_flush_pairs(acc, hist, true);
	} else {
	// (the loads of chunk ck + 1 issued before chunk ck is worked on measured no gain: 4.10 against 4.08 ms, three more spilled registers;
	// profiles/r07_pool/coop_stream_pipeline_ab.txt.  k_pool_cold's sweep S, where the stream is most of the work, keeps its pipeline.)
#pragma unroll 2
	for (int ck = 0; ck < NCH; ++ck) {
		const uint32_t x0 = wbase + 2048 * ck + WNT * lane;
		uint32_t m = ~0u; // positions at and beyond the query's end: lcp() stops there
		uint2 codes = make_uint2(0, 0);
		if (x0 < c.qlen) {
			const uint4 qv = ld_query(c, x0), sv = ld_subject_guarded(c, (int64_t)x0 + dg);
			m = squeeze32(neq32(qv, sv));
			codes = make_uint2(squeeze_codes(qv.x) | (squeeze_codes(qv.y) << 16), squeeze_codes(qv.z) | (squeeze_codes(qv.w) << 16));
			if (c.qlen - x0 < WNT) m |= ~0u << (c.qlen - x0);
			dirty |= (qv.x | qv.y | qv.z | qv.w) & 0x44444444u; // bit 2 of a symbol: no nucleotide (the padding behind the query's end too: its last window's walks read the query itself)
		}
		if (x0 <= e0 && e0 - x0 < WNT) m &= ~0u << (e0 - x0); // (what lies before the anchor is none of the window's business)
		if (x0 + WNT <= e0) m = 0;
		L.mbits[64 * ck + lane] = m;
		*(uint2 *)&L.q2[2 * (64 * ck + lane)] = codes;
	}
	}
	const bool clean = !__any(dirty != 0);
	if (lane < 4) L.q2[128 * NCH + lane] = 0;
	if (lane == 0) L.nhadx = 0;
	if (lane < 4) L.mbits[64 * NCH + lane] = 0;
	ch.blk_base = NOPOS; // (mode G's block of probes lies where the heads are about to be listed)
	ch.stuck = 0;
	wave_sync();

	TOCK(tph, PH_STREAM);
	// ---- heads: a mismatch with fewer than thr equal symbols behind it and at least thr before it.  Lane l looks
	// at the NCH words of positions 32 NCH l ...; a word together with its neighbours, thr < 32
	uint32_t hmask[NCH], nh = 0;
#pragma unroll
	for (int j = 0; j < NCH; ++j) {
		const uint32_t w = NCH * lane + j;
		const uint32_t cur = L.mbits[w], nxt = L.mbits[w + 1], prv = w ? L.mbits[w - 1] : 0u;
		// a mismatch among the next thr positions / among the thr positions before: the bits smeared over thr - 1 more positions (doubling,
		// then the remainder) -- on 32-bit words with funnel shifts, as k_pool_cold's sweep S does it (64-bit shifts and ors: twice the instructions)
		uint32_t soon = __builtin_amdgcn_alignbit(nxt, cur, 1), sn = nxt >> 1;   // bit x: position x + 1
		uint32_t before = __builtin_amdgcn_alignbit(cur, prv, 31), bp = prv << 1; // bit x: position x - 1
		uint32_t have = 1;
		while (2 * have <= thr) {
			soon |= __builtin_amdgcn_alignbit(sn, soon, have), sn |= sn >> have;
			before |= __builtin_amdgcn_alignbit(before, bp, 32 - have), bp |= bp << have;
			have *= 2;
		}
		if (have < thr) {
			const uint32_t r = thr - have;
			soon |= __builtin_amdgcn_alignbit(sn, soon, r);
			before |= __builtin_amdgcn_alignbit(before, bp, 32 - r);
		}
		uint32_t live = ~0u; // a chain that stands behind position x >= end - 1 has left the segment
		const uint32_t x0 = wbase + 32 * w;
		if (x0 + 1 >= end) live = 0;
		else if (end - 1 - x0 < 32) live = (1u << (end - 1 - x0)) - 1u;
		hmask[j] = cur & soon & ~before & live;
		nh += (uint32_t)__builtin_popcount(hmask[j]);
	}
	uint32_t hbase = wave_scan_add(nh); // (inclusive; made exclusive below)
	const uint32_t nheads_all = lane_read(hbase, 63);
	hbase -= nh;
	uint32_t dropped = NOPOS; // the first head beyond the list's capacity: nothing is decided from there on
#pragma unroll
	for (int j = 0; j < NCH; ++j)
		for (uint32_t hm = hmask[j]; hm; hm &= hm - 1) {
			const uint32_t off = 32 * (NCH * lane + j) + (uint32_t)__builtin_ctz(hm);
			if (hbase < COOP_HCAP)
				L.hpos[hbase] = (uint16_t)off;
			else if (dropped == NOPOS)
				dropped = wbase + off;
			++hbase;
		}
	const uint32_t nheads = nheads_all < COOP_HCAP ? nheads_all : COOP_HCAP;
	CSTAT(CS_WINDOWS, 1);
	CSTAT(CS_HEADS, nheads);
	CSTAT(CS_DROPPED, nheads_all - nheads);
	const uint32_t f_cap = nheads_all > COOP_HCAP ? uni(wave_min(dropped)) : NOPOS;
	wave_sync();

	TOCK(tph, PH_HEADS);
	// ---- the walks, one lane each; a lane that is done takes the next head.  A lane whose probe needs more than the
	// table's entry is parked; the parked lanes take lane_probe together once there are enough of them (or nothing else
	// is left to do).
	{
		uint32_t hk = NOPOS, e = 0, p = 0, Xq = 0, Xs = 0, Xl = 0, nX = 0, next_head = 0;
		uint32_t mx = 0, mn = 0, mq = 0; // a parked lane's K-mer, if it occurs a few times: first suffix-array index, occurrences, the 16 symbols behind it
		bool parked = false;
		// equal symbols from p on along the diagonal as far as 32 bits of the window show; seen: a mismatch of the window ends them
		auto run_ahead = [&](uint32_t pp, bool &seen) {
			const uint32_t o = pp - wbase, wi = o >> 5;
			const uint32_t lo = L.mbits[wi], hi = L.mbits[wi + 1];
			const uint32_t v = (o & 31u) ? (lo >> (o & 31u)) | (hi << (32u - (o & 31u))) : lo;
			const uint32_t r = v ? (uint32_t)__builtin_ctz(v) : 32u;
			seen = v != 0 && o + r < W;
			return r;
		};
		auto generic_probe = [&](uint32_t pp) { return coop_generic_probe(c, pp); };
		// a step's outcome (walk_settle); a head's result goes to its place in LDS
		auto settle = [&](uint32_t res, uint32_t ra, uint32_t rlen, const Probe &pr, bool have) {
			walk_settle(c, sd, e, p, Xq, Xs, Xl, nX, res, ra, rlen, pr, have);
			if (res) {
				if ((res & W_STATUS) == W_OK && (res & W_HADX) && atomicAdd(&L.nhadx, 1u) >= COOP_KCAP) res = W_BREAK; // (the list of such stretches is full)
				L.ha[hk] = (uint16_t)(ra - wbase), L.hend[hk] = rlen, L.hflag[hk] = (uint16_t)res;
				hk = NOPOS;
			}
		};
		// The parked lanes' turn -- coop_probe_multi, lane_probe: most of this loop's code -- stands in FRONT of the loop of the ordinary trips, not
		// inside it (two loops, the inner one small): 3.52 -> 3.36 ms on the bench set.
		bool due = false;
		for (;;) {
			if (due) {
				due = false;
				if (hk != NOPOS && parked) {
					uint32_t res = 0, ra = 0, rlen = 0;
					Probe pr;
					pr.len = 0, pr.pos = 0, pr.unique = false;
					bool have = false; // pr is the answer for p
					bool long_diag = false;
					if (mn) {
						bool seen;
						const uint32_t r = run_ahead(p, seen);
						have = coop_probe_multi(c, p, sd, mx, mn, mq, r, seen, pr, long_diag);
					}
					if (!have) pr = generic_probe(p), long_diag = false;
					have = true, parked = false;
#ifdef ANDI_COOP_STATS
					atomicAdd(&g_coop_stats[CS_PROBES], 1ull);
#endif
					if (long_diag && pr.unique) { // the diagonal's occurrence is the longest, longer than the bits at hand show
						if (wbase + W - p >= 32) {
							res = walk_on_diag(c, sd, e, p, Xl, nX, true);
							ra = p;
						} else {
							pr = generic_probe(p); // (the window's end)
						}
					}
					settle(res, ra, rlen, pr, have);
				}
			}
			for (;;) {
				const uint64_t idle = __ballot(hk == NOPOS);
				if (idle && next_head < nheads) {
					const uint32_t my = next_head + (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
					if (hk == NOPOS && my < nheads) hk = my, e = wbase + L.hpos[my], p = e + 1, Xl = 0, nX = 0, parked = false;
					next_head += (uint32_t)__builtin_popcountll(idle);
				}
				const uint64_t busy = __ballot(hk != NOPOS), waiting = __ballot(hk != NOPOS && parked);
				if (!busy) break;
				// the parked lanes' turn?
				// (... or no head is left to take: served only when nothing else was left, a parked lane's remaining steps ran alone behind all the others)
				const bool service = waiting && ((uint32_t)__builtin_popcountll(waiting) >= COOP_PARK || waiting == busy || next_head >= nheads);
#ifdef ANDI_COOP_STATS
				if (lane == (uint32_t)__builtin_ctzll(__ballot(1))) {
					const uint32_t nb = (uint32_t)__builtin_popcountll(service ? waiting : busy & ~waiting); // lanes at work in this trip
					atomicAdd(&g_coop_trip_lanes[service ? 1 : 0][nb ? 32 - __builtin_clz(nb) : 0], 1ull);
					atomicAdd(&g_coop_stats[service ? CS_SERVICE : CS_TRIPS], 1ull);
					atomicAdd(&g_coop_stats[service ? CS_SERVICE_LANES : CS_LANE_STEPS], (unsigned long long)__builtin_popcountll(service ? waiting : busy & ~waiting));
				}
#endif
				if (service) {
					due = true;
					break;
				}
				if (hk == NOPOS || parked) continue;
				uint32_t res = 0, ra = 0, rlen = 0;
				Probe pr;
				pr.len = 0, pr.pos = 0, pr.unique = false;
				bool have = false; // pr is the answer for p
				// ---- a lane that is not parked: the step's conditions as values, few branches (a wavefront executes every
				// branch some lane takes, and keeps the books of the execution mask for each: the nested form of this cost
				// 230 vector and 260 scalar instructions per trip)
				const uint32_t o = p - wbase;
				const bool inwin = p < end && o < W;
				bool seen;
				const uint32_t r = run_ahead(inwin ? p : wbase, seen); // equal symbols from p on along the diagonal
				const uint32_t left = W - (inwin ? o : 0u);             // positions of the window from p on
				const bool near = Xl == 0 && p + sd < n && p - e <= thr; // lucky_anchor applies on the diagonal: the bits answer
				const bool run_ok = seen ? r >= thr : left >= thr;      // an anchor (not seen: thr equal symbols and more, its end is settled later)
				res = !inwin ? (Xl ? W_BREAK : (p >= end ? W_EXIT : W_OPEN)) // (the walk has left the segment / the window)
					  : (near && run_ok) ? (W_OK | W_LUCKY)
					  : (near && !seen && left < thr) ? W_OPEN : 0u;
				ra = p;
				if (inwin && !res && o + 32 > W) res = Xl ? W_BREAK : W_OPEN; // (a probe in the window's last 32 symbols would be lane_probe's, by one lane: the chain stops at this head instead, the next window opens there)
				if (inwin && Xl) { // lucky_anchor on the diagonal of the anchor off the window's: compare (rare)
					const uint32_t adv = p - Xq;
					if (Xs + adv < n && adv - Xl <= thr) {
						const uint32_t qa = p & ~1u;
						const uint4 d = neq32(ld_query(c, qa), ld_subject_guarded(c, (int64_t)qa + ((int64_t)Xs - (int64_t)Xq)));
						uint32_t l = first_from(d, p & 1u) - (p & 1u);
						if (l > c.qlen - p) l = c.qlen - p;
						if (l >= thr) res = W_BREAK; // the chain really changes its diagonal: not this window's business
					}
				}
				if (inwin && !res) { // the probe (the lucky attempt has failed or does not apply: it is not repeated)
					bool on_diag;
					have = coop_probe_fast<NCH>(c, L, wbase, clean, p, sd, pr, on_diag, mx, mn, mq);
					if (!have && mn) { // a K-mer with a few occurrences: the sorter's records settle it as a rule -- no wait for the parked lanes' turn
						bool long_diag;
						if (coop_probe_r2(c, p, sd, mx, mn, mq, r, seen, pr, long_diag)) {
							have = true;
							if (long_diag && pr.unique) { // the diagonal's occurrence is the longest, longer than the bits at hand show
								if (wbase + W - p >= 32) {
									res = walk_on_diag(c, sd, e, p, Xl, nX, true);
								} else {
									have = false; // (the window's end: lane_probe's)
								}
							}
						}
					}
					if (on_diag) { // the K-mer's one occurrence is the diagonal's: the bits know the match
						pr.unique = true, pr.pos = p + sd, pr.len = r;
						if (!seen && left < 32) have = false; // (the window's end: lane_probe follows the occurrence)
						else if (!seen) rlen = NOPOS;         // longer than the bits at hand show: an anchor (thr < 32) whose end is settled later
					}
					parked = !have;
#ifdef ANDI_COOP_STATS
					if (have) atomicAdd(&g_coop_stats[CS_PROBES], 1ull);
#endif
				}
				settle(res, ra, rlen, pr, have);
			}
			if (!due) break;
		}
	}
	wave_sync();

	TOCK(tph, PH_WALKS);
	if constexpr (EXACT)
		for (uint32_t jw = 0; jw < (uint32_t)NCH; ++jw) L.ebits[NCH * lane + jw] = 0; // (the walks are done with the query codes that lay there)
	// ---- the chain hops from head to head; between them every mismatch is followed by a lucky anchor.
	// Nearly every head is on the chain's path and is followed by the next one: the lanes work out, head by head,
	// where its walk's anchor ends and whether anything is unusual about it (the next head lies inside the walk's
	// span; the walk did not land; a position at which the window's knowledge ends comes first); the chain is then
	// followed from one unusual head to the next with ballots -- a few trips per window, not one per head.
	uint32_t F = coop_prev_mismatch(L, wbase, wbase + W); // behind the last mismatch nothing is known
	const uint32_t last_mm = F;
	if (f_cap < F) F = f_cap;
	{
		const int64_t b = (int64_t)c.border - dg; // '#': the next anchor lies on the other strand, no right anchor (src/process.c:162)
		if (b >= (int64_t)e0 && b < (int64_t)F) F = (uint32_t)b;
		if (end - 1 < F) { // a chain that stands behind a position >= end - 1 has left the segment
			const uint32_t fe = coop_next_mismatch(L, wbase, end - 1 > e0 ? end - 1 : e0);
			if (fe != NOPOS && fe < F) F = fe;
		}
	}
	if (e0 >= F) {
		take_back(e0);
		wave_sync();
		return false;
	}
	uint32_t cur = e0, kcur = 0, hop = NOPOS; // hop: the last head the chain hopped from
	bool done = false;
	for (uint32_t base = 0; base < nheads && !done; base += 64) {
		const uint32_t k = base + lane;
		const bool valid = k < nheads;
		const uint32_t pos = valid ? wbase + L.hpos[k] : NOPOS, fl = valid ? L.hflag[k] : 0u;
		uint32_t endk = NOPOS; // where the anchor the walk landed on ends: the chain's next stand
		if ((fl & W_STATUS) == W_OK) {
			const uint32_t la = wbase + L.ha[k];
			if (fl & W_LUCKY) {
				const uint32_t o = la - wbase;
				uint32_t wi = o >> 5, v = L.mbits[wi] & (~0u << (o & 31u));
				while (v == 0 && wi + 1 < 64 * NCH) v = L.mbits[++wi];
				if (v) endk = wbase + 32 * wi + (uint32_t)__builtin_ctz(v);
			} else {
				endk = la + L.hend[k];
			}
		}
		const bool hop_ok = endk != NOPOS;
		uint32_t nxtpos = lane_above(pos);
		if (lane == 63) nxtpos = k + 1 < nheads ? wbase + L.hpos[k + 1] : NOPOS;
		const bool unusual = valid && (!hop_ok || pos >= F || nxtpos < endk || endk >= F);
		bool onpath = false;
		if (kcur < base) kcur = base;
		{ // heads the chain has jumped over already
			const uint64_t at = __ballot(valid && pos >= cur);
			const uint32_t first = at ? (uint32_t)__builtin_ctzll(at) : 64u;
			if (base + first > kcur) kcur = base + first;
		}
		while (!done && kcur < base + 64 && kcur < nheads) {
			CSTAT(CS_HOPS, 1);
			const uint32_t lo = kcur - base;
			const uint64_t ev = __ballot(unusual) & (~0ull << lo);
			const uint32_t j = ev ? (uint32_t)__builtin_ctzll(ev) : 64u; // every head before it: hopped, on to the next
			if (lane >= lo && lane < j && valid) onpath = true;
			if (j > lo) {
				const uint32_t last = (j < 64 ? j : 64u) - 1u;
				const uint32_t lastv = nheads - base - 1u < last ? nheads - base - 1u : last;
				hop = base + lastv, cur = lane_read(endk, lastv);
			}
			if (j >= 64) {
				kcur = base + 64;
				break;
			}
			const uint32_t pj = lane_read(pos, j), ej = lane_read(endk, j);
			if (pj >= F) { // the chain reaches a position where the window's knowledge ends before this head
				cur = F, done = true;
			} else if (ej == NOPOS) { // its walk did not land (or where the anchor ends is not in the window): the chain stops at the head
				cur = pj, done = true;
				if ((lane_read(fl, j) & W_STATUS) == W_BREAK) ch.stuck = 1;
			} else { // hopped; the chain stands where the anchor ends
				if (lane == j) onpath = true;
				hop = base + j, cur = ej;
				if (ej >= F) {
					done = true;
				} else {
					const uint64_t at = __ballot(valid && pos >= ej) & (~0ull << j);
					kcur = base + (at ? (uint32_t)__builtin_ctzll(at) : 64u);
				}
			}
		}
		if (valid) {
			L.hend[k] = endk;
			if (onpath) L.hflag[k] = (uint16_t)(fl | W_ONPATH);
		}
#ifdef ANDI_COOP_STATS
		{
			const uint64_t on = __ballot(onpath), ox = __ballot(onpath && (fl & W_HADX));
			CSTAT(CS_ONPATH, __builtin_popcountll(on));
			CSTAT(CS_X, __builtin_popcountll(ox));
		}
#endif
	}
	if (!done) cur = F; // past the last head: lucky anchors up to where the window's knowledge ends
	if (cur == e0) {
		take_back(e0);
		wave_sync();
		return false;
	}
	// What the chain did not reach is taken back.  As a rule it stands at the window's LAST mismatch (cur: the next window's e0): that one
	// mismatch, by one lane -- its query symbol from the codes in LDS (still there), the subject's by one load; anything else: take_back, below
	bool taken_back = false;
	if constexpr (!EXACT) {
		if (cur == last_mm && cur < c.qlen && clean) {
			if (lane == 0) {
				const uint32_t o = cur - wbase, qn = (L.q2[o >> 4] >> (2 * (o & 15u))) & 3u;
				const uint32_t sn = ld_subject_guarded(c, (int64_t)cur + dg).x & 15u;
				if (!(sn & 4u)) lds_add(&hist[((sn & 3u) << 2) | qn], 0u - 1u); // (counted only if both are nucleotides)
			}
			taken_back = true;
		}
	}
	CSTAT(CS_MOVED, 1);
	CSTAT(CS_COVERED, cur - e0);
	wave_sync();
	// the anchor that ends at cur: the one the last hop landed on, or the one behind the mismatch before cur
	uint32_t aQ, lw = 1;
	if (hop != NOPOS && uni(L.hend[hop]) == cur) {
		aQ = wbase + uni(L.ha[hop]), lw = (uni(L.hflag[hop]) & W_HADX) ? 0u : 1u;
	} else {
		aQ = coop_prev_mismatch(L, wbase, cur) + 1;
	}
	// Heads whose walk met anchors off the diagonal (rare): nothing pairs up across such a stretch; the anchor
	// before the head is counted only if it was a right anchor itself or is long (src/process.c:176-186)
	uint32_t extra_anchors = 0, kn = 0; // kn: stretches counted nowhere, listed in L.kpos
	for (uint32_t base = 0; base < nheads; base += 64) {
		const uint32_t k = base + lane;
		const uint32_t fl = k < nheads ? L.hflag[k] : 0u;
		for (uint64_t bx = __ballot((fl & W_ONPATH) && (fl & W_HADX)); bx; bx &= bx - 1) {
			const uint32_t kk = base + (uint32_t)__builtin_ctzll(bx);
			const uint32_t pk = wbase + uni(L.hpos[kk]);
			uint32_t a_before = NOPOS, lw_before = 1;
			if (pk == e0) {
				a_before = st.lastQ, lw_before = st.lwra;
			} else {
				for (uint32_t b2 = 0; b2 < nheads && a_before == NOPOS; b2 += 64) { // a hop that landed right before this head?
					const uint32_t k2 = b2 + lane;
					const bool m = k2 < nheads && (L.hflag[k2] & W_ONPATH) && L.hend[k2] == pk;
					const uint64_t bm = __ballot(m);
					if (bm) {
						const uint32_t kp = b2 + (uint32_t)__builtin_ctzll(bm);
						a_before = wbase + uni(L.ha[kp]), lw_before = (uni(L.hflag[kp]) & W_HADX) ? 0u : 1u;
					}
				}
				if (a_before == NOPOS) a_before = coop_prev_mismatch(L, wbase, pk) + 1;
			}
			if constexpr (EXACT) { // (the counting pass below counts every anchor's nucleotides: this one is taken back if it does not count)
				if (!(lw_before || pk - a_before >= 2 * thr)) coop_count_anchor(c, (lds_u32 *)L.hist, a_before, pk - a_before, false);
			} else {
				if (lw_before || pk - a_before >= 2 * thr) ch.quarter += (pk - a_before) >> 2, ch.rest += (pk - a_before) & 3u;
			}
			extra_anchors += (uni(L.hflag[kk]) >> W_NX_SHIFT) & 7u;
			if (lane == 0) L.kpos[kn] = pk;
			++kn;
			if constexpr (!EXACT) // (the stretch is counted nowhere: its mismatches were, with all the window's)
				pool_uncount_coop(c, hist, pk, (uint32_t)((int64_t)pk + dg), wbase + uni(L.ha[kk]) - pk);
		}
	}
	wave_sync();

	TOCK(tph, PH_HOPS);
	// ---- the stretches behind the heads the chain came by: gap positions (ebits), unless listed in kpos (counted nowhere);
	// their symbols are counted here, by the lane of the head (model_count, src/model.c:309-337)
	if constexpr (!EXACT) {
		// the mismatches were counted with all the window's: what is left of a stretch (head, landing) are its EQUAL symbols, by nucleotide -- from
		// the window's bits and the query's codes, both still in LDS (the codes lie where the stretches' bits are about to be written); a window
		// with a separator ('!' = '!' is no pair of nucleotides) reads the texts instead
		uint32_t eq0 = 0, eq1 = 0, eq2 = 0, eq3 = 0;
		uint32_t tt = 0, t0 = 0, t1 = 0, t01 = 0; // equal symbols in all: whose code has bit 0, bit 1, both
		for (uint32_t b = 0; b < nheads; b += 64) {
			const uint32_t i = b + lane;
			const uint32_t fl = i < nheads ? L.hflag[i] : 0u;
			const bool ord = (fl & W_ONPATH) && !(fl & W_HADX);
			const uint32_t o0 = ord ? L.hpos[i] + 1u : 0u, o1 = ord ? L.ha[i] : 0u; // [o0, o1): behind the head's own mismatch
			if (clean) {
				for (uint32_t wd = o0 >> 5; 32 * wd < o1; ++wd) {
					uint32_t rm = ~0u;
					if (wd == (o0 >> 5)) rm &= ~0u << (o0 & 31u);
					if (32 * wd + 32 > o1) rm &= (1u << (o1 & 31u)) - 1u;
					const uint32_t eq = ~L.mbits[wd] & rm, c0 = L.q2[2 * wd], c1 = L.q2[2 * wd + 1];
					const uint32_t lo = spread16(eq), hi = spread16(eq >> 16); // (a position's bit where its code's low bit lies)
					const uint32_t l0 = lo & c0, l1 = lo & (c0 >> 1), h0 = hi & c1, h1 = hi & (c1 >> 1);
					tt += (uint32_t)__builtin_popcount(eq);
					t0 += (uint32_t)__builtin_popcount(l0) + (uint32_t)__builtin_popcount(h0);
					t1 += (uint32_t)__builtin_popcount(l1) + (uint32_t)__builtin_popcount(h1);
					t01 += (uint32_t)__builtin_popcount(l0 & l1) + (uint32_t)__builtin_popcount(h0 & h1);
				}
			} else {
				for (uint64_t sl = __ballot(ord && o1 > o0); sl; sl &= sl - 1) {
					const uint32_t l = (uint32_t)__builtin_ctzll(sl);
					const uint32_t q0 = wbase + lane_read(o0, l), ln = lane_read(o1, l) - lane_read(o0, l);
					pool_count_equal_coop(c, q0, (uint32_t)((int64_t)q0 + dg), ln, eq0, eq1, eq2, eq3);
				}
			}
		}
		eq0 += tt - t0 - t1 + t01, eq1 += t0 - t01, eq2 += t1 - t01, eq3 += t01; // (A: neither bit, C: bit 0 alone, G: bit 1 alone, T: both)
		{
			const uint32_t v0 = wave_sum(eq0 | (eq2 << 16)), v1 = wave_sum(eq1 | (eq3 << 16)); // (the stretches of a window are disjoint: fewer than 2048 NCH <= 16384 symbols in all -- two sums to a register)
			if (lane == 0) lds_add(&hist[0], v0 & 0xffffu), lds_add(&hist[5], v1 & 0xffffu), lds_add(&hist[10], v0 >> 16), lds_add(&hist[15], v1 >> 16);
		}
		wave_sync();
		for (uint32_t jw = 0; jw < (uint32_t)NCH; ++jw) L.ebits[NCH * lane + jw] = 0; // (the query's codes that lay there are done with)
		wave_sync();
		for (uint32_t b = 0; b < nheads; b += 64) {
			const uint32_t i = b + lane;
			const uint32_t fl = i < nheads ? L.hflag[i] : 0u;
			if (!(fl & W_ONPATH)) continue;
			const uint32_t o0 = L.hpos[i], o1 = L.ha[i]; // [o0, o1)
			for (uint32_t wd = o0 >> 5; 32 * wd < o1; ++wd) {
				uint32_t m = ~0u;
				if (wd == (o0 >> 5)) m &= ~0u << (o0 & 31u);
				if (32 * wd + 32 > o1) m &= (1u << (o1 & 31u)) - 1u;
				lds_or(&L.ebits[wd], m);
			}
		}
	} else
	{
		Tally tl;
		tl.hist = (lds_u32 *)L.hist, tl.hs = 1, tl.quarter = tl.rest = 0;
		tl.same[0] = tl.same[1] = tl.same[2] = tl.same[3] = 0;
		LWin w;
		w.q0 = EMPTY, w.dg = NO_DIAG;
		for (uint32_t b = 0; b < nheads; b += 64) {
			const uint32_t i = b + lane;
			const uint32_t fl = i < nheads ? L.hflag[i] : 0u;
			if (!(fl & W_ONPATH)) continue;
			const uint32_t o0 = L.hpos[i], o1 = L.ha[i]; // [o0, o1)
			uint32_t *dst = L.ebits;
			for (uint32_t wd = o0 >> 5; 32 * wd < o1; ++wd) {
				uint32_t m = ~0u;
				if (wd == (o0 >> 5)) m &= ~0u << (o0 & 31u);
				if (32 * wd + 32 > o1) m &= (1u << (o1 & 31u)) - 1u;
				lds_or(&dst[wd], m);
			}
			if (!(fl & W_HADX)) lane_count_gap(w, c, tl, wbase + o0, (uint32_t)((int64_t)(wbase + o0) + dg), o1 - o0);
		}
	}
	wave_sync();

	TOCK(tph, PH_STRETCH);
	// ---- the mismatches behind which a lucky anchor follows at once (all that are in no such stretch), and the
	// anchors: one ends at every position that starts a gap.  Positions e0 ... cur - 1; lane l takes the NCH words of
	// positions 32 NCH l ... (what lies before its first word comes from one scan over the lanes).
	uint32_t q_acc = 0, r_acc = 0, n_acc = 0, x_acc[4] = {0, 0, 0, 0};
	auto in_range = [&](uint32_t x0) { // the positions e0 ... cur - 1 of the word that starts at x0
		uint32_t rm = ~0u;
		if (x0 + WNT <= e0 || x0 >= cur) rm = 0;
		if (rm && e0 > x0) rm &= ~0u << (e0 - x0);
		if (rm && cur - x0 < WNT) rm &= (1u << (cur - x0)) - 1u;
		return rm;
	};
	uint32_t before = 0; // (the last position in no anchor before the lane's words) + 2; 0: none
	for (uint32_t jw = 0; jw < (uint32_t)NCH; ++jw) {
		const uint32_t w = NCH * lane + jw, x0 = wbase + 32 * w;
		const uint32_t u = (L.mbits[w] | L.ebits[w]) & in_range(x0);
		if (u) before = x0 + 31u - (uint32_t)__builtin_clz(u) + 2u;
	}
	{
		const uint32_t scan = wave_scan_max(before);
		before = lane_below(scan);
		if (lane == 0 || before < st.lastQ + 1u) before = st.lastQ + 1u; // (the anchor before e0 starts at lastQ: lastQ - 1 is the position before it)
	}
	uint32_t prev_top = 0; // the last position of the word before is in no anchor (what lies before e0 is the anchor)
	{
		const uint32_t w = NCH * lane;
		if (w && wbase + 32 * w > e0) prev_top = ((L.mbits[w - 1] | L.ebits[w - 1]) & in_range(wbase + 32 * (w - 1))) >> 31;
	}
	// LogDet / ANI: the nucleotides of every anchor that ends at a gap start of [e0, cur) -- the positions from the start of
	// the anchor before e0 up to aQ that are in no gap (the part of that anchor that lies before the window: at once)
	auto anchor_range = [&](uint32_t x0) { // the positions lastQ ... aQ - 1 of the word that starts at x0
		uint32_t rm = ~0u;
		if (x0 + WNT <= st.lastQ || x0 >= aQ) rm = 0;
		if (rm && st.lastQ > x0) rm &= ~0u << (st.lastQ - x0);
		if (rm && aQ - x0 < WNT) rm &= (1u << (aQ - x0)) - 1u;
		return rm;
	};
	if constexpr (EXACT)
		if (st.lastQ < wbase) coop_count_anchor(c, (lds_u32 *)L.hist, st.lastQ, (aQ < wbase ? aQ : wbase) - st.lastQ);
	auto fetch = [&](uint32_t jw, uint4 &qv, uint4 &sv) { // the symbols of a word that has single mismatches (or, LogDet / ANI, anchors) to count
		const uint32_t w = NCH * lane + jw;
		uint32_t x0 = wbase + 32 * w;
		qv = sv = make_uint4(0, 0, 0, 0);
		if constexpr (!EXACT) return; // (every mismatch was counted when the window was streamed)
		// (five chunks: the word's position as a value of this fetch alone -- an empty statement, as own_sgpr's.  Its range masks are otherwise
		// shared with the loop's of the next iteration and live across this one: k_coop_cold<5, true> then spills 23 registers, not 15;
		// with two and four chunks the shared masks are the cheaper: profiles/r11_coop_segment.md)
		if constexpr (NCH == 5) asm volatile("" : "+v"(x0));
		if (jw >= (uint32_t)NCH) return;
		const bool singles = (L.mbits[w] & ~L.ebits[w] & in_range(x0)) != 0;
		if (singles || (EXACT && anchor_range(x0))) qv = ld_query(c, x0);
		if (singles) sv = ld_subject_guarded(c, (int64_t)x0 + dg);
	};
	uint4 qnext, snext;
	fetch(0, qnext, snext);
	for (uint32_t jw = 0; jw < (uint32_t)NCH; ++jw) {
		const uint32_t w = NCH * lane + jw, x0 = wbase + 32 * w;
		const uint4 qv = qnext, sv = snext;
		fetch(jw + 1, qnext, snext); // (in flight while this word is counted)
		const uint32_t rm = in_range(x0), m = L.mbits[w] & rm, eb = L.ebits[w] & rm, u = m | eb;
		uint32_t gs = u & ~((u << 1) | prev_top); // gap starts: a position in no anchor whose predecessor is in one
		n_acc += (uint32_t)__builtin_popcount(gs);
		for (; gs; gs &= gs - 1) {
			const uint32_t b = (uint32_t)__builtin_ctz(gs), below = u & ((1u << b) - 1u);
			const uint32_t pv = below ? x0 + 31u - (uint32_t)__builtin_clz(below) : before - 2u; // the last position before x0 + b in no anchor
			const uint32_t len = x0 + b - 1u - pv; // (pv may be lastQ - 1 = -1: unsigned wrap is fine)
			// (the anchor before a stretch that is counted nowhere: the hop above has dealt with it, src/process.c:176-186)
			bool nowhere = false;
			for (uint32_t t = 0; t < kn; ++t) nowhere |= L.kpos[t] == x0 + b;
			if (!EXACT && !nowhere) q_acc += len >> 2, r_acc += len & 3u;
		}
		if constexpr (EXACT) { // this word's positions inside anchors, by nucleotide
			const uint32_t am = anchor_range(x0) & ~u;
			for (uint32_t j = 0; j < 4 && am; ++j) {
				uint32_t t = (am >> (8 * j)) & 0xffu; // 8 positions -> bit 4k of a word
				if (!t) continue;
				t = (t | (t << 12)) & 0x000f000fu, t = (t | (t << 6)) & 0x03030303u, t = (t | (t << 3)) & ONES;
				const uint32_t qw = pick(qv, j), ok = t & ~(qw >> 2), b0 = qw, b1 = qw >> 1;
				x_acc[0] += (uint32_t)__builtin_popcount(ok & ~(b0 | b1)), x_acc[1] += (uint32_t)__builtin_popcount(ok & b0 & ~b1);
				x_acc[2] += (uint32_t)__builtin_popcount(ok & b1 & ~b0), x_acc[3] += (uint32_t)__builtin_popcount(ok & b0 & b1);
			}
		}
		if (u) before = x0 + 31u - (uint32_t)__builtin_clz(u) + 2u;
		prev_top = u >> 31;
		for (uint32_t singles = EXACT ? m & ~eb : 0u; singles; singles &= singles - 1) { // mismatches in no head's stretch: single-position gaps
			const uint32_t b = (uint32_t)__builtin_ctz(singles), sh = 4 * (b & 7u);
			const uint32_t qn = (pick(qv, b >> 3) >> sh) & 15u, sn = (pick(sv, b >> 3) >> sh) & 15u;
			if (!((qn | sn) & 4u)) lds_add((lds_u32 *)&L.hist[((sn & 3u) << 2) | (qn & 3u)], 1u);
		}
	}
	TOCK(tph, PH_FINAL);
	ch.quarter += wave_sum(q_acc), ch.rest += wave_sum(r_acc);
	if constexpr (EXACT) {
		for (int k = 0; k < 4; ++k) {
			const uint32_t v = wave_sum(x_acc[k]);
			if (lane == 0) lds_add((lds_u32 *)&L.hist[5 * k], v);
		}
	}
	ch.anchors += wave_sum(n_acc) + extra_anchors;
	{
		const uint32_t nodes = wave_sum(n_acc);
		(void)nodes;
		CSTAT(CS_NODES, nodes);
	}
	if (!taken_back) take_back(cur); // (the mismatches the chain did not reach)
	st.p = cur + 1, st.lastS = (uint32_t)((int64_t)aQ + dg), st.lastQ = aQ, st.lastLen = cur - aQ, st.lwra = lw;
	return true;
}

// coop_segment's windows in mode W
template <int NCH, bool EXACT>
struct WindowsLds {
	static constexpr bool COUNTS_EQUAL = false; // (the stretches' equal symbols go to the counts in LDS, window by window)
	__device__ __forceinline__ void begin(const Chain &) {}
	__device__ __forceinline__ bool window(const ScanArgs &a, const PairCtx &c, Chain &ch, CoopLds<NCH> &L, uint32_t end) { return coop_window<NCH, EXACT>(a, c, ch, L, end); }
};

} // namespace
