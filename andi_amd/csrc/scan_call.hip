// scan_call.hip — andi_hip_scan_rows (include/andi_hip.h): one scan call over a batch of subjects against the staged
// queries -- the choice of path, the segmentation of the queries, the scratch and the launches of passes A, B and C.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "api_internal.h"

// segment length when the caller passes 0: short enough that one scan launch has
// several hundred thousand chains, long enough that stitching stays a few per cent
#define ANDI_MIN_SEGMENT 4096u
#define ANDI_MAX_SEGMENT 65536u
#define ANDI_TARGET_CHAINS (1u << 22) /* at most about this many chains per call (308 bytes of scratch each) */
#define ANDI_MIN_CHAINS (1u << 19)    /* and long segments only while the call keeps this many */
// per-pair segment lengths: classes seg/2, seg, 2 seg, 4 seg of the call's length, as long as the scratch they
// need (whole wavefronts per pair) stays a fraction of the device's memory
#define ANDI_ADAPTIVE_MAX_PAIRS (1u << 22)
#define ANDI_ROUTE_MIN_NT (1u << 18) /* query symbols x subjects from which pass A of a call is routed per pair */
#define ANDI_ROUTE_TINY_NT (1u << 25) /* ... below which it is not routed but takes pass A by wavefronts for every pair */
#define ANDI_ROUTE_SMALL_NT (1ull << 30) /* ... below which pass A by wavefronts takes a millisecond or less: a few pairs left to the lane scan would take longer (k_pair_route) */

static int ensure_segmentation(andi_hip_ctx *ctx, andi_hip_queries *q, uint32_t seg, bool coop = false) {
	uint32_t &have = coop ? q->c_seg : q->seg, &total_out = coop ? q->c_total_segs : q->total_segs;
	uint32_t *&d_start = coop ? q->c_qseg_start : q->d_qseg_start, *&d_s2q = coop ? q->c_seg2query : q->d_seg2query;
	if (have == seg && d_start) return 0;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	(void)andi_arena::dev_free(d_start);
	(void)andi_arena::dev_free(d_s2q);
	d_start = d_s2q = nullptr;
	std::vector<uint32_t> start(q->nq + 1);
	uint64_t total = 0;
	for (size_t i = 0; i < q->nq; ++i) {
		start[i] = (uint32_t)total;
		total += (q->len[i] + (uint64_t)seg - 1) / seg;
		if (total >= UINT32_MAX) {
			ctx->err = "too many scan segments; raise opts.segment";
			return 1;
		}
	}
	start[q->nq] = (uint32_t)total;
	std::vector<uint32_t> s2q((size_t)total);
	for (size_t i = 0; i < q->nq; ++i)
		for (uint32_t w = start[i]; w < start[i + 1]; ++w) s2q[w] = (uint32_t)i;
	HIP_TRY(ctx, dmalloc(&d_start, q->nq + 1));
	HIP_TRY(ctx, dmalloc(&d_s2q, (size_t)total));
	HIP_TRY(ctx, hipMemcpy(d_start, start.data(), (q->nq + 1) * 4, hipMemcpyHostToDevice));
	HIP_TRY(ctx, hipMemcpy(d_s2q, s2q.data(), (size_t)total * 4, hipMemcpyHostToDevice));
	have = seg;
	total_out = (uint32_t)total;
	return 0;
}

namespace {

// a knob's integer value where it lies in [lo, hi]; dflt where it is unset or out of range
int knob_int(AndiKnob k, int lo, int hi, int dflt) {
	const char *v = andi_knob(k);
	return v && atoi(v) >= lo && atoi(v) <= hi ? atoi(v) : dflt;
}

// Everything a scan call decides: which path it takes, its segment lengths and the scalar arguments of its kernels.
// plan_call fixes the path from the call's shape and the knobs; plan_layout, once the subjects' flags are known, whether the
// lane scan takes per-pair segment lengths.
struct ScanPlan {
	bool routed = false;        // pass A routed per pair: the wavefront kernel's layout b beside the lane scan's a (scan.h)
	int coop = 0;               // pass A by wavefronts for every pair (ANDI_COOP=n, tiny calls)
	bool want_adaptive = false; // per-pair segment lengths, unless a subject takes the reference's walk or the scratch says no
	bool adaptive = false;
	uint32_t segment = 0;   // the call's segment length
	uint32_t coop_seg = 0;  // the wavefront kernel's in a routed call
	uint32_t seg0 = 0;      // per-pair segment lengths: the shortest class
	uint32_t max_class = 0;
	uint64_t max_waves = 0; // per-pair segment lengths: wavefronts if every pair had the shortest segments (the grid)
	uint32_t seg_factor = 0, quad_min_match = 0, knock = 0, pool_match = 0, route_all_few = 0, route_giveup = 0;
	uint32_t items_order = ANDI_ITEMS_HEAVY; // the order of the wavefront kernel's segments (scan.h: coop_items)
	uint32_t longest_q = 0, reduce_threads = 0, coop_reduce_threads = 0; // (the lane layouts', layout b's)
	int exact_equal = 0;
	bool force_reference = false, force_adaptive = false;
};

// pass C: 64 threads per pair where no query has more than 64 segments, else the lane scan's block
uint32_t reduce_threads(uint32_t longest_q, uint32_t seg) { return (longest_q + seg - 1) / seg <= 64 ? 64u : 0u; }

ScanPlan plan_call(andi_hip_esa *const *subjects, size_t nsub, const andi_hip_queries *q, int model, uint32_t segment) {
	ScanPlan P;
	P.force_reference = andi_knob(KNOB_FORCE_REFERENCE) != nullptr;
	P.force_adaptive = andi_knob(KNOB_FORCE_ADAPTIVE) != nullptr;
	const bool uniform = andi_knob(KNOB_UNIFORM_SEGMENTS) != nullptr;
	// segment == 0: the engine chooses.  With the lane scan and a moderate number of pairs
	// the segment length is chosen per pair (scan_lane.hip: k_pair_estimate); otherwise one
	// length for the call.
	// Pass A with one wavefront per chain (scan_coop.hip) for the models that split an anchor's length evenly and
	// thresholds a 32-symbol window can decide.  ANDI_COOP=n: the call's pass A, one (long) segment length for the call.
	// Unset: large calls are ROUTED PER PAIR (scan.h) -- the pairs whose sampled matches suit that kernel take it, on a
	// segmentation of its own; the others, and the pairs it hands back, take the lane scan; passes B and C run per layout.
	const int coop_mode = andi_coop_enabled();
	int coop_ok = coop_mode != 0 && !P.force_reference;
	for (size_t s = 0; s < nsub && coop_ok; ++s)
		if (!subjects[s] || subjects[s]->thr < 2 || subjects[s]->thr > 30) coop_ok = 0;
	const uint64_t call_nt = q->total_nt * (uint64_t)nsub;
	const bool engine = coop_ok && coop_mode < 0 && segment == 0 && call_nt >= ANDI_ROUTE_MIN_NT && !uniform && !P.force_adaptive;
	// TINY calls (less than two rounds of wavefronts on 2048-symbol segments): that kernel for every pair, without the
	// sampling -- whatever a pair is like, a wavefront's chain over 2048 symbols is no longer than a lane's over 4096, and
	// the device has the wavefronts to spare (structured genomes 3 x 1 Mbp ... 5 x 1.3 Mbp: 2.1 ... 3.3 ms by wavefronts,
	// 2.65 ... 3.4 by lanes; clean ones 3 x 1 Mbp: 0.34 against 0.54 routed, 0.96 by lanes)
	const int tiny_log = knob_int(KNOB_ROUTE_TINY, 1, 62, 0); // (tests, experiments: log2 of that size; 1: no call is tiny, small ones are routed)
	bool tiny = engine && call_nt < (tiny_log ? 1ull << tiny_log : ANDI_ROUTE_TINY_NT);
	// A wavefront needs far fewer chains in flight than a lane, and every segment costs it a cold start of a dozen
	// dependent round trips: segments as long as leave the device four rounds of wavefronts (24576), 32768 ... 524288
	// symbols (measured: bench set 5.57 / 5.39 / 5.31 / 5.34 ms at 32768 / 65536 / 131072 / 262144, C4 shape 38.6 / 33.5 /
	// 32.6 / 32.6 / 35.4 / 44.0 ms at 32768 / 131072 / 262144 / 524288 / 2^20 / 2^21 -- whole queries: pairs differ too much)
	// Small calls: shorter segments still, as long as the device has one round of wavefronts (2048 symbols at least) --
	// 3 x 1 Mbp (BASELINE's configs[0]): pass A 0.10 ms by wavefronts against 0.66 ms by lanes; 100 x 30 kbp 0.94 against
	// 2.35 ms per call (profiles/r05_small_calls.txt).
	uint32_t coop_seg = 524288;
	while (coop_seg > 32768 && call_nt / coop_seg < 24576) coop_seg /= 2;
	while (coop_seg > 2048 && call_nt / coop_seg < 12000u) coop_seg /= 2; // (8 x 1 Mbp: 0.38 ms at 4096 -- 15 600 wavefronts --, 0.46 at 2048; 12 x 1 Mbp: 0.65 at 8192 -- 17 600 --, 0.74 at 4096)
	P.coop_seg = coop_seg = (uint32_t)knob_int(KNOB_COOP_SEG, 64, INT32_MAX, (int)coop_seg); // experiments
	// (the smallest calls -- a few launches' worth of work -- keep the lane scan: routing costs them the sampling kernel
	// and two looks of the host at the device)
	bool routed = engine && nsub * q->nq <= ANDI_ADAPTIVE_MAX_PAIRS;
	if (routed || tiny) { // (queries shorter than the wavefront kernel takes -- k_pair_estimate -- are the lane scan's: where they are most of the call, all of it)
		uint64_t cand_nt = 0;
		for (size_t i = 0; i < q->nq; ++i)
			if (q->len[i] >= std::min(coop_seg, ANDI_ROUTE_MIN_QLEN)) cand_nt += q->len[i];
		if (2 * cand_nt < q->total_nt) routed = tiny = false;
	}
	P.routed = routed && !tiny;
	P.coop = coop_ok && (coop_mode > 0 || tiny);
	P.want_adaptive = !P.coop && segment == 0 && nsub * q->nq <= ANDI_ADAPTIVE_MAX_PAIRS && !uniform;
	if (segment == 0 && P.coop) segment = coop_seg;
	if (segment == 0) {
		segment = ANDI_MIN_SEGMENT;
		while (segment < ANDI_MAX_SEGMENT && call_nt / segment > ANDI_TARGET_CHAINS) segment *= 2;
	}
	P.segment = segment;
	P.seg0 = (uint32_t)knob_int(KNOB_SEG0, 64, INT32_MAX, (int)(segment / 2)); // classes: 1/2, 1, 2, 4 times the call's segment length (experiments: the shortest)
	P.seg_factor = (uint32_t)knob_int(KNOB_SEG_FACTOR, 1, INT32_MAX, 16); // measured best of 8/16/32 with seg0 = 2048
	P.quad_min_match = (uint32_t)knob_int(KNOB_QUAD_MATCH, INT32_MIN, INT32_MAX, 128); // experiments: mean match length from which a pair goes to k_lane_quad (0: all, -1: none)
	P.knock = (uint32_t)knob_int(KNOB_KNOCK, INT32_MIN, INT32_MAX, 0);
	P.pool_match = (uint32_t)knob_int(KNOB_POOL_MATCH, 0, INT32_MAX, 48); // (experiments: mean sampled match from which a routed pair's wavefront kernel is k_pool_cold)
	const int small_log = knob_int(KNOB_ROUTE_SMALL, 1, 62, 0); // (experiments: log2 of the size below which a call is small)
	P.route_all_few = call_nt < (small_log ? 1ull << small_log : ANDI_ROUTE_SMALL_NT) ? 1u : 0u;
	// (tests: hand pairs back early, so that the second lane layout runs; small calls route pairs the sampling cannot judge: a lower limit)
	P.route_giveup = (uint32_t)knob_int(KNOB_COOP_GIVEUP, 1, INT32_MAX, P.route_all_few ? 256 : 1024);
	// (tests, measurements: ANDI_COOP_ORDER=G the grid -- no list --, R the list lightest first, the worst case; profiles/r09_coop_order.md)
	if (const char *o = andi_knob(KNOB_COOP_ORDER)) P.items_order = o[0] == 'G' ? ANDI_ITEMS_GRID : o[0] == 'R' ? ANDI_ITEMS_LIGHT : ANDI_ITEMS_HEAVY;
	for (size_t i = 0; i < q->nq; ++i) P.longest_q = std::max(P.longest_q, (uint32_t)q->len[i]);
	P.coop_reduce_threads = reduce_threads(P.longest_q, coop_seg);
	P.exact_equal = (model == ANDI_M_LOGDET || model == ANDI_M_ANI) ? 1 : 0; // src/model.c:247
	return P;
}

// the rest of the plan, from the subjects' walks: any_reference (a subject on the reference's walk), the pairs' query
// nucleotides nt, h_self the subjects' own queries
void plan_layout(andi_hip_ctx *ctx, ScanPlan &P, const int64_t *h_self, size_t nsub, const andi_hip_queries *q,
				 int any_reference, uint64_t nt) {
	if (any_reference) P.routed = false;
	P.adaptive = P.want_adaptive && !any_reference;
	if (P.adaptive) {
		for (size_t s = 0; s < nsub; ++s)
			for (size_t i = 0; i < q->nq; ++i) {
				if (h_self[s] == (int64_t)i) continue;
				P.max_waves += ((q->len[i] + (uint64_t)P.seg0 - 1) / P.seg0 + 63) / 64;
			}
		// a pair occupies whole wavefronts: with queries of a few segments most lanes would idle, and the
		// scratch must stay a fraction of the device's memory -- one segment length for the call then
		uint64_t used = 0;
		for (size_t i = 0; i < q->nq; ++i) used += (q->len[i] + (uint64_t)P.seg0 - 1) / P.seg0;
		used *= nsub;
		size_t free_b = 0, total_b = 0;
		// (a routed call may need a second lane layout as large as the first for the pairs handed back: counted here, so that
		// a call that fits keeps fitting when that happens)
		const size_t want_b = (size_t)64 * P.max_waves * ANDI_SLOT_BYTES * (P.routed ? 2 : 1);
		const bool fits = P.max_waves < (1u << 26) && // (the device is asked only when the scratch would have to grow)
						  (want_b <= ctx->scratch_bytes || hipMemGetInfo(&free_b, &total_b) != hipSuccess || want_b < free_b / 2 + ctx->scratch_bytes);
		if (!fits || (10 * used < 7 * 64 * P.max_waves && !P.force_adaptive)) P.adaptive = false, P.max_waves = 0;
	}
	P.max_class = 0; // long segments must not leave the device short of chains
	while (P.max_class < 3 && nt / ((uint64_t)P.seg0 << (P.max_class + 1)) >= ANDI_MIN_CHAINS) P.max_class++;
	P.reduce_threads = reduce_threads(P.longest_q, P.adaptive ? P.seg0 : P.segment);
}

// The scratch of one layout, carved from base + off; returns the end offset (a null base only measures: the size of a
// scratch and its carving are one walk).  The per-slot arrays of n slots; then, where pairs != 0 (per-pair segment lengths,
// routing), the pairs' wavefront counts and offsets, with cls their classes (the call's first layout: the others share
// them); then, where nsub != 0 (the routed call's first layout), the order of the subjects and, where items != 0, the list of the
// wavefront kernel's segments, `items` of them at most, with the pairs' cost classes and the scratch of its sort (scan.h).  What is
// not carved keeps its value.
size_t carve_layout(ScanArgs &x, char *base, size_t off, size_t n, size_t pairs, bool cls, size_t nsub, size_t items = 0) {
	uintptr_t p = (uintptr_t)base + off;
	auto take = [&p](size_t bytes, size_t align = 1) {
		p = (p + align - 1) & ~(uintptr_t)(align - 1);
		const uintptr_t at = p;
		p += bytes;
		return (void *)at;
	};
	x.cold_exit = (ChainState *)take(n * sizeof(ChainState));
	x.true_exit = (ChainState *)take(n * sizeof(ChainState));
	x.used_entry = (ChainState *)take(n * sizeof(ChainState));
	x.cold_counts = (uint32_t *)take(n * 16 * sizeof(uint32_t));
	x.owned = (uint32_t *)take(n * 16 * sizeof(uint32_t));
	x.marks = (ColdMark *)take(n * ANDI_COLD_MARKS * sizeof(ColdMark));
	x.exit_p = (uint32_t *)take(n * sizeof(uint32_t));
	x.restitch_count = (uint32_t *)take(64, 16);
	x.restitch_round = 0;
	x.defer_count = x.restitch_count + 8;
	x.defer_list = (unsigned long long *)take(n * sizeof(unsigned long long));
	x.first_pub = (unsigned long long *)take(n * sizeof(unsigned long long)); // (k_lane_quad, per-pair segment lengths only)
	x.stretch_bad = (uint8_t *)x.first_pub;                                   // (pass B: a byte per slot, while first_pub is idle)
	if (pairs) {
		x.pair_waves = (uint32_t *)take(pairs * sizeof(uint32_t));
		x.pair_wave0 = (uint32_t *)take((pairs + 1) * sizeof(uint32_t));
		x.pair_bsum = (uint32_t *)take((pairs / 1024 + 2) * sizeof(uint32_t));
		if (cls) x.pair_class = (uint8_t *)take(pairs);
	}
	if (nsub) {
		x.sub_cost = (float *)take(nsub * sizeof(float), 16);
		x.sub_order = (uint32_t *)take(nsub * sizeof(uint32_t));
	}
	if (items) {
		x.pair_cost = (uint8_t *)take(pairs);
		x.item_hist = (uint32_t *)take(ANDI_COST_CLASSES * ((pairs + 1023) / 1024) * sizeof(uint32_t), 16);
		x.coop_items = (uint32_t *)take(items * sizeof(uint32_t));
	}
	return (size_t)(p - (uintptr_t)base);
}

// The call's scratch (ctx->scratch, grown on demand): lane layout a with its pairs' arrays, then -- routed -- the wavefront
// kernel's layout b at *b_off.  Carves a; b is carved from its copy of a (launch_routed).
int carve_scratch(andi_hip_ctx *ctx, const ScanPlan &P, ScanArgs &a, size_t slots, size_t slots2, size_t nsub, size_t pairs_all, size_t *b_off) {
	const size_t pairs = P.adaptive || P.routed ? pairs_all : 0, subs = P.routed ? nsub : 0;
	// The wavefront kernel's segments as a list (scan.h: coop_items) where the host is going to look at the layout anyway -- the list's length
	// comes with that look -- and the launch is at most ANDI_ITEMS_ROUNDS rounds of the device's resident wavefronts (slots2 bounds it): what
	// the order takes is the tail, and a launch of dozens of rounds -- the C4 shape's 24 680 pairs -- has little of it, while the list, sorted
	// by class, walks all its subjects' tables in every class where the grid finishes one subject after the other (C4 shape by k_pool_cold
	// 20.6-20.9 -> 21.5-21.8 ms, of 40-contig genomes by k_coop_cold 42.4-42.7 -> 42.9-43.0; profiles/r09_coop_order.md).  Such calls
	// neither build nor carve a list.
	if (!ctx->round_waves) {
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) cus = 256;
		ctx->round_waves = (uint32_t)cus * 4u * 8u; // (k_coop_cold: eight wavefronts per SIMD)
	}
	const bool listed = P.routed && !P.route_all_few && P.items_order != ANDI_ITEMS_GRID && slots2 <= (size_t)ANDI_ITEMS_ROUNDS * ctx->round_waves;
	const size_t items = listed ? slots2 : 0;
	ScanArgs m = a;
	*b_off = (carve_layout(m, nullptr, 0, slots, pairs, true, subs, items) + 15) & ~(size_t)15;
	const size_t need = (P.routed ? carve_layout(m, nullptr, *b_off, slots2, 0, false, 0) : *b_off) + 256; // (256 bytes of slack behind the last array)
	if (ctx->scratch_bytes < need) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (ctx->scratch) (void)andi_arena::dev_free(ctx->scratch);
		ctx->scratch = nullptr;
		ctx->scratch_bytes = 0;
		HIP_TRY(ctx, andi_arena::dev_malloc(&ctx->scratch, need));
		ctx->scratch_bytes = need;
	}
	carve_layout(a, (char *)ctx->scratch, 0, slots, pairs, true, subs, items);
	return 0;
}

// the subjects' descriptors, [EsaDev x nsub][int64 x nsub] (pinned host -> device, guarded by desc_done): every subject's
// walk as its index build's flags say.  Counts the pairs, their query nucleotides and the subjects on the reference's walk.
// ahead: the caller is going to look at the device before pass A anyway (launch_routed) and checks the flags then -- where every subject has its
// probe table and builds are still in flight, the descriptors are written for the probe walk WITHOUT waiting for them (*ahead stays set;
// cleared where the wait was taken after all): the host enqueued the call's first kernels only once the builders had ended, 25 us of
// idle device per call (profiles/r14_call_edges.md).
int upload_descriptors(andi_hip_ctx *ctx, andi_hip_esa *const *subjects, const int64_t *self, size_t nsub, const andi_hip_queries *q,
					   bool force_reference, int &any_reference, uint64_t &pairs, uint64_t &nt, bool *ahead) {
	const size_t desc_need = nsub * (sizeof(EsaDev) + sizeof(int64_t));
	if (ctx->desc_bytes < desc_need) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (ctx->desc_dev) (void)andi_arena::dev_free(ctx->desc_dev);
		if (ctx->desc_host) host_pool::pinned_put(ctx->desc_host, ctx->desc_bytes);
		ctx->desc_dev = ctx->desc_host = nullptr;
		ctx->desc_bytes = 0;
		const size_t desc_cap = std::max<size_t>(desc_need, 4096); // (one size for small calls: the pool of pinned buffers hands it back)
		HIP_TRY(ctx, andi_arena::dev_malloc(&ctx->desc_dev, desc_cap));
		HIP_TRY(ctx, host_pool::pinned_get(&ctx->desc_host, desc_cap));
		ctx->desc_bytes = desc_cap;
	} else {
		HIP_TRY(ctx, hipEventSynchronize(ctx->desc_done)); // previous upload consumed
	}
	auto *h_esa = (EsaDev *)ctx->desc_host;
	auto *h_self = (int64_t *)(h_esa + nsub);
	pairs = 0, nt = 0, any_reference = 0;
	// the index builds must have finished: their flags decide which walk is exact.  (Only the builds this context
	// has queued since its last scan are waited for -- not whatever else is on the stream; subjects built by another
	// context are the caller's to have synchronised, as before.)
	*ahead = *ahead && ctx->builds_pending && !force_reference;
	for (size_t s = 0; s < nsub && *ahead; ++s) *ahead = subjects[s] && subjects[s]->index_built;
	if (ctx->builds_pending && !*ahead) {
		HIP_TRY(ctx, hipEventSynchronize(ctx->built));
		ctx->builds_pending = false;
	}
	for (size_t s = 0; s < nsub; ++s) {
		andi_hip_esa *e = subjects[s];
		if (!e || (!e->index_built && !e->ref_built)) {
			ctx->err = "andi_hip_scan_rows: subject index not built";
			return 1;
		}
		if (*ahead) { // (the flags are not final yet: taken to be clear, looked at behind the first look)
			h_esa[s] = esa_view(e, ANDI_MODE_PROBE);
			h_self[s] = self ? self[s] : -1;
			const bool has_self = h_self[s] >= 0 && (size_t)h_self[s] < q->nq;
			pairs += q->nq - (has_self ? 1 : 0);
			nt += q->total_nt - (has_self ? q->len[(size_t)h_self[s]] : 0);
			continue;
		}
		int mode = ANDI_MODE_PROBE;
		if (!e->index_built || e->h_flags[0] != 0 || force_reference) {
			// a 10-mer table entry may span a separator: only the reference's
			// own walk reproduces get_match_cached there
			mode = ANDI_MODE_REFERENCE;
			if (!e->ref_built && andi_hip_esa_build(ctx, e)) return 1;
			ctx->acc.reference_subjects++;
			any_reference = 1;
		}
		if (e->index_built && e->h_flags[1]) {
			ctx->err = "andi_hip_scan_rows: a subject holds a byte outside {A,C,G,T,!,;,#}";
			return 1;
		}
		h_esa[s] = esa_view(e, mode);
		h_self[s] = self ? self[s] : -1;
		bool has_self = h_self[s] >= 0 && (size_t)h_self[s] < q->nq;
		pairs += q->nq - (has_self ? 1 : 0);
		nt += q->total_nt - (has_self ? q->len[(size_t)h_self[s]] : 0);
	}
	HIP_TRY(ctx, hipMemcpyAsync(ctx->desc_dev, ctx->desc_host, desc_need, hipMemcpyHostToDevice,
								ctx->stream));
	HIP_TRY(ctx, hipEventRecord(ctx->desc_done, ctx->stream));
	return 0;
}

// The arguments of lane layout a but its scratch (carve_scratch)
ScanArgs scan_args(andi_hip_ctx *ctx, const ScanPlan &P, size_t nsub, const andi_hip_queries *q, andi_hip_model *M_dev, int any_reference) {
	ScanArgs a;
	a.subjects = (const EsaDev *)ctx->desc_dev;
	a.self = (const int64_t *)((const EsaDev *)ctx->desc_dev + nsub);
	a.nsub = (uint32_t)nsub;
	a.qpool = q->pool, a.qnib = q->nib, a.qplanes = q->planes, a.qcodes = q->codes, a.qoff = q->d_off, a.qlen = q->d_len, a.qsep = q->d_sep, a.nq = (uint32_t)q->nq;
	a.qseg_start = q->d_qseg_start, a.seg2query = q->d_seg2query;
	a.total_segs = q->total_segs, a.seg = P.segment;
	a.adaptive = P.adaptive ? 1 : 0;
	a.seg0 = P.seg0, a.max_waves = (uint32_t)P.max_waves, a.max_class = P.max_class;
	a.pair_waves = a.pair_wave0 = a.pair_bsum = nullptr, a.pair_class = nullptr; // (carve_scratch: where the call has them)
	a.sub_cost = nullptr, a.sub_order = nullptr;
	a.pair_cost = nullptr, a.coop_items = nullptr, a.item_hist = nullptr, a.layout_count = nullptr; // (carve_scratch, launch_routed: where the call has a list)
	a.n_items = 0, a.items_order = ANDI_ITEMS_GRID;
	a.seg_factor = P.seg_factor;
	a.M = M_dev;
	a.fixups = ctx->d_fixups;
	a.any_reference = any_reference;
	a.quad_min_match = P.quad_min_match;
	a.quad_listed = 0;
	a.side_stream = ctx->side_stream, a.side_fork = ctx->side_fork, a.side_join = ctx->side_join;
	a.h_quad_waves = ctx->h_quad_waves;
	a.knock = P.knock;
	a.coop = P.coop && !a.adaptive;
	a.pool_scratch = nullptr, a.pool_ticket = nullptr, a.pool_waves = 0, a.pool_bytes = 0;
	a.pool_maxchunks = a.pool_hc = 0, a.pool_first = 0, a.pool_use = 0;
	a.pool_match = P.pool_match;
	a.route = P.routed ? ANDI_LAYOUT_LANES : 0, a.route_seg = P.coop_seg, a.route_nt = ctx->d_route;
	a.reduce_threads = P.reduce_threads;
	a.route_all_few = P.route_all_few;
	a.route_giveup = P.route_giveup;
	a.exact_equal = P.exact_equal;
	return a;
}

// Pooled walks (k_pool_cold): the scratch of the resident wavefronts -- 0.8 GB on a 256-CU part, a mapping of its own -- is
// taken only by a call that is going to run that kernel (andi_coop_wants_pool: known behind the look at the layout in a
// routed call), from the device's idle one if a destroyed context left it (host_pool), once per context; a context whose
// attempt failed does not try again (the windows then stay in LDS: k_coop_cold).
void give_pool_scratch(andi_hip_ctx *ctx, ScanArgs &x) {
	if (!andi_coop_wants_pool(x)) return;
	if (!ctx->pool_scratch && !ctx->pool_failed) {
		uint32_t waves = 0;
		const size_t bytes = andi_pool_scratch_bytes(ctx->device, &waves);
		if (bytes && (ctx->pool_scratch = host_pool::scratch_get(ctx->device, bytes)))
			ctx->pool_waves = waves, ctx->pool_bytes = bytes - 4096;
		else
			ctx->pool_failed = true;
	}
	if (!ctx->pool_scratch) return;
	x.pool_ticket = (uint32_t *)ctx->pool_scratch, x.pool_scratch = (char *)ctx->pool_scratch + 4096, x.pool_waves = ctx->pool_waves, x.pool_bytes = ctx->pool_bytes;
}

// A call that is not routed: per-pair segment lengths (the layout first) or one length for the call; pass A by lanes, or
// by wavefronts for every pair (ANDI_COOP=n, tiny calls)
hipError_t launch_direct(andi_hip_ctx *ctx, ScanArgs &a, const char *&what) {
	hipError_t e = hipSuccess;
	if (a.adaptive) {
		Timed t(ctx, 2);
		e = andi_launch_pair_layout(a, ctx->stream);
		t.stop();
		if (e != hipSuccess) return what = "scan layout", e;
	}
	give_pool_scratch(ctx, a);
	{
		Timed t(ctx, 1);
		e = andi_launch_scan_cold(a, ctx->stream);
		t.stop();
		if (e != hipSuccess) return what = "scan pass A", e;
		if (a.coop) ctx->acc.coop_calls++;
		if (a.coop && andi_coop_will_pool(a)) ctx->acc.pool_calls++;
	}
	Timed t(ctx, 2);
	e = andi_launch_scan_stitch(a, ctx->stream);
	if (e == hipSuccess) e = andi_launch_scan_reduce(a, ctx->stream);
	t.stop();
	if (e != hipSuccess) what = "scan passes B/C";
#ifdef ANDI_TEST_HOOKS
	if (e == hipSuccess && !a.adaptive) { // one segment length: the slots the suite's hook hands out (api.hip: andi_hip_test_stitch_slots)
		auto &l = ctx->last_slots;
		l.cold_exit = a.cold_exit, l.true_exit = a.true_exit, l.used_entry = a.used_entry, l.cold_counts = a.cold_counts, l.owned = a.owned;
		l.marks = a.marks, l.restitch_count = a.restitch_count, l.nsub = a.nsub, l.total_segs = a.total_segs, l.seg = a.seg;
	}
#endif
	return e;
}

// The call's pairs are routed (scan.h): the wavefront kernel's layout b (at b_off of the scratch) beside the lane scan's a.
// The pairs are sampled and routed; pass A by wavefronts (on a stream of its own) runs beside the lane scan's kernels; the
// pairs it handed back -- rare: the host looks -- get a second lane layout a2; passes B and C once per layout.
// ahead (upload_descriptors): the subjects' flags were taken to be clear; *again is set, with nothing but the layout's kernels run and the
// streams drained, where the first look finds one of them raised: the caller runs the call again, waiting for the builds first.
hipError_t launch_routed(andi_hip_ctx *ctx, const ScanPlan &P, ScanArgs &a, size_t b_off, const andi_hip_queries *q,
						 size_t slots, size_t slots2, andi_hip_esa *const *subjects, bool ahead, bool *again, const char *&what) {
	const size_t nsub = a.nsub, pairs_all = nsub * q->nq;
	ScanArgs b = a;
	b.adaptive = 0, b.coop = 1, b.route = ANDI_LAYOUT_COOP;
	b.qseg_start = q->c_qseg_start, b.seg2query = q->c_seg2query, b.total_segs = q->c_total_segs, b.seg = P.coop_seg;
	b.reduce_threads = P.coop_reduce_threads;
	carve_layout(b, (char *)ctx->scratch, b_off, slots2, 0, false, 0);
	const bool look = !a.route_all_few;
	const bool listed = b.coop_items != nullptr; // (carve_scratch: whether this call has a list)
	b.items_order = listed ? P.items_order : (uint32_t)ANDI_ITEMS_GRID;
	b.layout_count = a.restitch_count;
	hipError_t e;
	const size_t timers_before = ctx->pending.size();
	uint32_t pass_a[3] = {0, 0, 0}, rounds[3] = {0, 0, 0}; // what is launched per layout (a, b, a2), set where it is launched (the suite's hook reads them)
	{
		Timed t(ctx, 2);
		e = andi_launch_pair_layout(a, ctx->stream, b.restitch_count); // (b's counters cleared with a's: pass B's first stage counts on that, below)
		if (e == hipSuccess && listed) e = andi_launch_coop_items(b, ctx->stream);
		t.stop();
		if (e != hipSuccess) return what = "scan layout", e;
	}
	Timed t(ctx, 1);
	// Which of the two goes first: the lane scan's kernels where its pairs are few -- behind the wavefront kernel a
	// handful of lane blocks (four wavefronts and their LDS on one CU at once) found no place until that kernel's
	// tail and ended 0.2 ms after everything else --, the wavefront kernel where they are many (the tree-structured
	// set, the C4 shape: 0.4 and 1.5 ms the other way round).  The host looks at the layout (one word).
	// (Small calls do not look: the wavefront kernel first, the lane layout's passes whether it has pairs or not --
	// a look costs them 40 us of their few hundred.)
	for (int k = 0; k < 16; ++k) ctx->h_any_left[1 + k] = 0;
	ctx->h_any_left[1 + ANDI_LANE_WAVES] = 1;
	e = hipSuccess;
	if (look) e = hipMemcpyAsync(ctx->h_any_left + 1, a.restitch_count, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
	if (look && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (ahead && e == hipSuccess) { // (the look's wait implies the builds have ended: they are earlier work of the same stream)
		ctx->builds_pending = false;
		for (size_t s = 0; s < nsub; ++s)
			if (subjects[s]->h_flags[0] != 0 || subjects[s]->h_flags[1] != 0) *again = true;
		if (*again) { // (only the call's stream has work, and the look waited for it)
			// the discarded layout's timer does not count: stitch_ms and stitch_launches are the rerun's alone
			while (ctx->pending.size() > timers_before) {
				ctx->idle_events.push_back(ctx->pending.back().a), ctx->idle_events.push_back(ctx->pending.back().b);
				ctx->pending.pop_back();
			}
			return hipSuccess;
		}
	}
	const bool lanes_first = look && e == hipSuccess && (uint64_t)ctx->h_any_left[1 + ANDI_LANE_WAVES] * 20 < ctx->h_any_left[1 + ANDI_ALL_WAVES];
	// which wavefront kernel: the pooled one where the pairs that suit it hold at least half of the segments (scan.h)
	b.pool_use = look && e == hipSuccess && 2 * (uint64_t)ctx->h_any_left[1 + ANDI_POOL_SEGS] >= ctx->h_any_left[1 + ANDI_COOP_SEGS] && ctx->h_any_left[1 + ANDI_COOP_SEGS] != 0;
	give_pool_scratch(ctx, b);
	b.n_items = ctx->h_any_left[1 + ANDI_COOP_SEGS]; // (the list's length, where the call has one)
	// (k_pool_cold, whose calls are the long launches of carve_scratch's rule, keeps the grid whatever the length: its choice comes with the look)
	if (andi_coop_will_pool(b)) b.coop_items = nullptr;
	ctx->last_items.items = b.coop_items, ctx->last_items.pair_class = b.pair_class, ctx->last_items.pair_cost = b.pair_cost;
	ctx->last_items.n_items = b.n_items, ctx->last_items.pairs = (uint32_t)pairs_all, ctx->last_items.total_segs = b.total_segs;
	ctx->last_items.pair_waves = a.pair_waves, ctx->last_items.pair_wave0 = a.adaptive ? a.pair_wave0 : nullptr, ctx->last_items.sub_order = a.sub_order;
	ctx->last_items.nsub = a.nsub, ctx->last_items.looked = look ? 1u : 0u;
	for (int k = 0; k < 16; ++k) ctx->last_items.counts[k] = ctx->h_any_left[1 + k];
	// A lane layout without a pair (known from the first look; a call that does not look is taken to have some) launches nothing: its pass A
	// is a memset of 8 bytes per slot, a look of its own on the side stream and kernels whose wavefronts all return -- 0.1 ms of the bench
	// step in front of the wavefront kernel (profiles/r14_call_edges.md) --, and its passes B and C have nothing to do.  The wavefront
	// kernel and its passes then stay on the call's stream: with nothing beside them a stream of their own is two crossings for nothing.
	const bool any_lanes = ctx->h_any_left[1 + ANDI_LANE_WAVES] != 0;
	const hipStream_t bs = any_lanes ? ctx->coop_stream : ctx->stream;
	if (e == hipSuccess && any_lanes) e = hipEventRecord(ctx->coop_fork, ctx->stream);
	if (e == hipSuccess && any_lanes) e = hipStreamWaitEvent(ctx->coop_stream, ctx->coop_fork, 0);
	if (e == hipSuccess && lanes_first && any_lanes) e = andi_launch_scan_cold(a, ctx->stream), pass_a[0] = 1;
	if (e == hipSuccess) e = andi_launch_coop_cold(b, bs), pass_a[1] = 1;
	if (andi_coop_will_pool(b)) ctx->acc.pool_calls++;
	if (e == hipSuccess && any_lanes) e = hipEventRecord(ctx->coop_join, ctx->coop_stream);
	if (e == hipSuccess && !lanes_first && any_lanes) e = andi_launch_scan_cold(a, ctx->stream), pass_a[0] = 1;
	if (e == hipSuccess && any_lanes) e = hipStreamWaitEvent(ctx->stream, ctx->coop_join, 0);
	if (e != hipSuccess) return what = "scan pass A", e;
	t.stop(); // (pass A's kernels, as before; the host's wait for the look below is no longer inside)
	// Passes B and C once per layout, side by side (each is a chain of small launches).  The host must see whether a pair was handed back --
	// one word of layout b --, but nothing of b's pass B depends on that: its first stage goes right behind the wavefront kernel, and the
	// host looks behind THAT, at three words in one copy -- pairs handed back, chains of the first stage that left their segment on their
	// own, the first stage's list.  Where no chain did, the rounds that stitch again would all return at once (k_stitch_heads): they are
	// not launched.  (b's counters are clear but for the first of those words since the layout's clearing: the stage counts in them as
	// they are.)  The lane layout's passes need nothing from the look and are enqueued in front of it.
	Timed t2(ctx, 2);
	e = andi_launch_scan_stitch(b, bs, ANDI_STITCH_STAGE0);
	if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_any_left + ANDI_LOOK_B, b.restitch_count, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, bs);
	if (e == hipSuccess) e = hipEventRecord(ctx->l2_fork, ctx->stream); // (pass A of both layouts done: where the chain of the pairs handed back starts)
	if (e == hipSuccess && any_lanes) e = andi_launch_scan_stitch(a, ctx->stream, ANDI_STITCH_ALL, &rounds[0]);
	if (e == hipSuccess && any_lanes) e = andi_launch_scan_reduce(a, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(bs);
	if (e != hipSuccess) return what = "scan passes B/C", e;
	const bool any_left = (ctx->h_any_left[0] = ctx->h_any_left[ANDI_LOOK_B + ANDI_ROUTE_ANY_LEFT]) != 0;
	const bool rounds_b = ctx->h_any_left[ANDI_LOOK_B + ANDI_RESTITCH_ROUNDS] != 0;
	ScanArgs a2 = a;
	// (scratch2 may be regrown here although the lane layout's passes B and C are still in flight on the call's stream and only bs has been
	// waited for: no kernel of layouts a and b touches scratch2, and the previous call's use of it lies before this call's work on every stream, bs included)
	if (any_left) { // the pairs handed back: a lane layout of their own (as large as the first at most)
		const size_t need2 = carve_layout(a2, nullptr, 0, slots, pairs_all, false, 0) + 256;
		if (ctx->scratch2_bytes < need2) {
			if (ctx->scratch2) (void)andi_arena::dev_free(ctx->scratch2);
			ctx->scratch2 = nullptr, ctx->scratch2_bytes = 0;
			e = andi_arena::dev_malloc(&ctx->scratch2, need2);
			if (e != hipSuccess) return what = "scratch of the second lane layout", e;
			ctx->scratch2_bytes = need2;
		}
		carve_layout(a2, (char *)ctx->scratch2, 0, slots, pairs_all, false, 0);
		a2.route = ANDI_LAYOUT_LANES2;
		a2.side_stream = nullptr; // (its own kernels one after the other: it runs on the side stream itself, below)
	}
	if (rounds_b) e = andi_launch_scan_stitch(b, bs, ANDI_STITCH_ROUNDS, &rounds[1]);
	if (e == hipSuccess) e = andi_launch_scan_reduce(b, bs);
	if (e == hipSuccess && any_lanes) e = hipEventRecord(ctx->coop_join, ctx->coop_stream);
	if (e == hipSuccess && any_left) { // (they take their pass A at the head of their chain, behind both layouts' pass A)
		e = hipStreamWaitEvent(ctx->side_stream, ctx->l2_fork, 0);
		if (e == hipSuccess) e = andi_launch_pair_leftover(a2, ctx->side_stream);
		if (e == hipSuccess) e = andi_launch_scan_cold(a2, ctx->side_stream), pass_a[2] = 1;
		if (e == hipSuccess) e = andi_launch_scan_stitch(a2, ctx->side_stream, ANDI_STITCH_ALL, &rounds[2]);
		if (e == hipSuccess) e = andi_launch_scan_reduce(a2, ctx->side_stream);
		if (e == hipSuccess) e = hipEventRecord(ctx->l2_join, ctx->side_stream);
	}
	if (e == hipSuccess && any_lanes) e = hipStreamWaitEvent(ctx->stream, ctx->coop_join, 0);
	if (e == hipSuccess && any_left) e = hipStreamWaitEvent(ctx->stream, ctx->l2_join, 0);
	if (e == hipSuccess) e = andi_launch_route_count(a, ctx->stream);
	t2.stop();
#ifdef ANDI_TEST_HOOKS
	for (int k = 0; k < 3; ++k) ctx->last_edges.pass_a[k] = pass_a[k], ctx->last_edges.rounds[k] = rounds[k];
	ctx->last_edges.count_b = b.restitch_count;
#else
	(void)pass_a, (void)rounds;
#endif
	if (e != hipSuccess) return what = "scan passes B/C", e;
	ctx->acc.coop_calls++;
	ctx->acc.routed_calls++;
	return hipSuccess;
}

} // namespace

// ------------------------------------------------------------------ scan
int andi_hip_scan_rows(andi_hip_ctx *ctx, andi_hip_esa *const *subjects, const int64_t *self,
					   size_t nsub, const andi_hip_queries *q_const, int model, uint32_t segment,
					   andi_hip_model *M_dev) {
	if (!ctx || !subjects || !q_const || !M_dev || nsub == 0 || nsub > 65535) {
		if (ctx) ctx->err = "andi_hip_scan_rows: bad arguments";
		return 1;
	}
	if (model < ANDI_M_RAW || model > ANDI_M_ANI) {
		ctx->err = "andi_hip_scan_rows: unknown model";
		return 1;
	}
	auto *q = const_cast<andi_hip_queries *>(q_const);
	if (*q->h_foreign) { // the reference's reader never produces that (src/sequence.c:260-282)
		ctx->err = "andi_hip_scan_rows: a query holds a byte outside {A,C,G,T,!}";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the streams only scans use (a context that stages or uploads never asks for them: a stream costs 3 ms to create)
	if (!ctx->side_stream) HIP_TRY(ctx, host_pool::stream_get(&ctx->side_stream, ctx->device, ctx->stream_prio));
	if (!ctx->coop_stream) HIP_TRY(ctx, host_pool::stream_get(&ctx->coop_stream, ctx->device, 0));

	ctx->last_items = {}; // (what the test hook reads points into this call's scratch: nothing of an earlier call's outlives it)
#ifdef ANDI_TEST_HOOKS
	ctx->last_slots = {}; // (likewise: before the scratch may be regrown, and for a call that is routed or takes per-pair lengths)
	ctx->last_edges = {};
#endif
	for (bool may_go_ahead = true;; may_go_ahead = false) {
		ScanPlan P = plan_call(subjects, nsub, q, model, segment);
		if (ensure_segmentation(ctx, q, P.segment)) return 1;
		int any_reference = 0;
		uint64_t pairs = 0, nt = 0;
		bool ahead = may_go_ahead && P.routed && !P.route_all_few; // (the calls whose host looks at the layout: launch_routed)
		if (upload_descriptors(ctx, subjects, self, nsub, q, P.force_reference, any_reference, pairs, nt, &ahead)) return 1;
		const int64_t *h_self = (const int64_t *)((const EsaDev *)ctx->desc_host + nsub);
		plan_layout(ctx, P, h_self, nsub, q, any_reference, nt);
		if (P.routed && ensure_segmentation(ctx, q, P.coop_seg, true)) return 1;
		const size_t slots = P.adaptive ? (size_t)64 * P.max_waves : nsub * (size_t)q->total_segs;
		const size_t slots2 = P.routed ? nsub * (size_t)q->c_total_segs : 0; // (the wavefront kernel's layout, beside the lane scan's)
		ScanArgs a = scan_args(ctx, P, nsub, q, M_dev, any_reference);
		size_t b_off = 0;
		if (carve_scratch(ctx, P, a, slots, slots2, nsub, nsub * q->nq, &b_off)) return 1;

		// every error exit from here on first waits for the streams the launches fork work onto: their kernels read the scratch
		// the next call may regrow, and the context's teardown waits for ctx->stream only
		const char *what = nullptr;
		bool again = false;
		const hipError_t e = P.routed ? launch_routed(ctx, P, a, b_off, q, slots, slots2, subjects, ahead, &again, what) : launch_direct(ctx, a, what);
		if (e != hipSuccess) {
			(void)hipStreamSynchronize(ctx->coop_stream);
			(void)hipStreamSynchronize(ctx->side_stream);
			(void)hipStreamSynchronize(ctx->stream);
			return fail(ctx, what, e);
		}
#ifdef ANDI_TEST_HOOKS
		ctx->last_edges.went_ahead |= ahead ? 1u : 0u, ctx->last_edges.ran_again |= again ? 1u : 0u;
#endif
		if (again) continue; // (a flag was raised: the same call the way it runs behind finished builds -- the reference's walk, or its error)
		(P.adaptive ? ctx->acc.adaptive_calls : ctx->acc.uniform_calls)++;
		ctx->acc.scan_pairs += pairs;
		ctx->acc.scan_query_nt += nt;
		return 0;
	}
}
