// scan_coop.hip -- pass A of the anchor scan (dist_anchor, src/process.c:141-214) with ONE WAVEFRONT PER CHAIN.
//
// scan_lane.hip gives every lane a cold chain of its own: 64 chains per wavefront stand at ten different places
// of the step, a load instruction has 7 of 64 lanes active, and the wavefront executes the whole loop body once
// per trip (profiles/r03e_pmc.txt).  Here the 64 lanes work on ONE chain -- the cold chain of one segment,
// exactly the states and counts the sequential loop produces (what pass B stitches is unchanged) -- in two modes:
//
//   G  generic steps, one after the other: lucky_anchor (src/process.c:82-100) compares 2048 symbols per round
//      trip (64 lanes x 32 symbols), anchor() (113-123) probes the next 64 query positions at once (the chain
//      then hops through the answers: each step lands at most 64 positions on), the accounting of 157-190 counts
//      a gap with all lanes.  The chain is in this mode until it has found a LUCKY anchor: two anchors in a row on
//      one diagonal.
//   W  a window of W = 2048 NCH query symbols along that diagonal (NCH = 5 on segments of 32768 symbols and more), streamed
//      with fully coalesced loads -- both texts bit-sliced, 12 bytes per 32 symbols (LogDet / ANI: 4-bit symbols) -- and
//      turned into one bit per position (query symbol != subject symbol); every mismatch is counted at once as a
//      single-position gap, by kind (what the chain does not reach is taken back).  Behind a mismatch that is
//      followed by >= threshold equal symbols the next step is a lucky anchor whose outcome the bits alone decide
//      ("easy").  A mismatch followed by a shorter run but preceded by a long one is a HEAD: the chain arrives
//      there in a known (canonical) state, so the walks from ALL heads of the window -- probe, step, probe ... until
//      an anchor on the diagonal is found -- are independent and are taken by the lanes in parallel, speculatively
//      (a lane that is done takes the next head).  The chain then hops from head to head; counts follow from the
//      gap positions (all mismatches, and the stretch between a head and the anchor its walk lands on) and the
//      anchors between them.  tests/coop_model.py restates this decomposition on the CPU and checks it against the
//      plain loop; tests/test_coop_gpu.py checks this kernel against k_lane_cold slot by slot.
//
// Layout: one segment length for the call (slot = subject * total_segs + segment), wavefront w of subject
// blockIdx.y takes segment w -- or, in a routed call whose host looked at the layout, wavefront k the k-th entry of the list of the
// kernel's segments, heaviest pairs first (scan.h: coop_items).  LogDet and ANI count every anchor's nucleotides (EXACT: src/model.c:256-278).
//
// The files, each on top of the ones before it only: coop_dev.h -- what both kernels share: the wavefront's helpers, mode G's step and the
// probes, the walks' verdicts, the segment driver coop_segment with pass A's hand-off to pass B; coop_window.h -- mode W, the window in LDS;
// coop_pool.h -- mode P, the window pooled through global memory (its three sweeps are described there); this file -- the two kernels, which
// decode their item and call coop_segment, the knobs and the launch.
#include "coop_window.h"
#include "coop_pool.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int COOP_WAVES = 1; // wavefronts per block: single wavefronts find a place on a CU the moment one leaves (bench set 5.39 -> 5.24 ms against blocks of two, 5.61 with four); seven per SIMD (72 registers): 4.94

// ------------------------------------------------------------------ the kernel of mode W: a wavefront per segment, from the grid or the list
template <int NCH, bool EXACT>
#ifndef COOP_OCC
#define COOP_OCC 8
#endif
__global__ __launch_bounds__(64 * COOP_WAVES, NCH <= 5 ? COOP_OCC : 4) void k_coop_cold(ScanArgs a) {
	__shared__ CoopLds<NCH> s_lds[COOP_WAVES];
	CoopLds<NCH> &L = s_lds[threadIdx.x >> 6];
	uint32_t sub, wseg = uni(blockIdx.x * COOP_WAVES + (threadIdx.x >> 6));
	if (a.coop_items) { // (routed calls whose host looked at the layout: the wavefronts' segments as a list, scan.h)
		if (wseg >= a.n_items) return;
		const uint32_t item = uni(a.coop_items[wseg]);
		sub = item / a.total_segs, wseg = item - sub * a.total_segs;
		if (sub >= a.nsub) return;
	} else
		sub = a.sub_order ? uni(a.sub_order[blockIdx.y]) : blockIdx.y; // (routed calls on the grid: the heaviest subjects first, scan.h)
	if (wseg >= a.total_segs) return;
	WindowsLds<NCH, EXACT> win;
	coop_segment<EXACT>(a, L, sub, wseg, win);
}

// ------------------------------------------------------------------ the kernel of mode P: persistent wavefronts take the segments in order, a scratch each
__global__ __launch_bounds__(64, POOL_OCC) void k_pool_cold(ScanArgs a) {
	__shared__ PoolLds L;
	const PoolScratch Gs = pool_scratch_at(a.pool_scratch, blockIdx.x, a.pool_maxchunks, a.pool_hc);
	const uint32_t items = a.total_segs * a.nsub;
	uint32_t item = blockIdx.x; // the first one; then whatever comes next
	while (item < items) {
		const uint32_t row = item / a.total_segs;
		WindowsPool win(a, &Gs);
		coop_segment<false>(a, L, a.sub_order ? uni(a.sub_order[row]) : row, item % a.total_segs, win);
		wave_sync();
		uint32_t nx = 0;
		if (__lane_id() == 0) nx = atomicAdd(a.pool_ticket, 1u);
		item = gridDim.x + lane_read(nx, 0);
	}
}

} // namespace

// ANDI_COOP=0: never; 2, 4, 5, 8: pass A with one wavefront per chain for every pair, windows of 2048 n symbols, whatever
// the call (any other value: 4, with a warning); unset (< 0): large calls are routed per pair (scan.h)
int andi_coop_enabled(void) {
	const char *e = andi_knob(KNOB_COOP);
	if (!e) return -4;
	const int v = atoi(e);
	if (v == 0 || v == 2 || v == 4 || v == 5 || v == 8) return v;
	static bool warned = false;
	if (!warned) fprintf(stderr, "andi-hip: ANDI_COOP=%s: windows of 2, 4, 5 or 8 chunks of 2048 symbols; taking 4\n", e), warned = true;
	return 4;
}

static bool pool_enabled() { // ANDI_POOL=0: the windows stay in LDS (coop_window), as up to round 4
	const char *e = andi_knob(KNOB_POOL);
	return !e || atoi(e) != 0;
}

// The pooled kernel's scratch: a window of POOL_MW positions per resident wavefront
constexpr uint32_t POOL_FUSED_CHUNKS = POOL_MW / 2048u, POOL_FUSED_HC = POOL_MW / 64u;
size_t andi_pool_scratch_bytes(int device, uint32_t *waves) {
	*waves = 0;
	if (!pool_enabled()) return 0;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
	*waves = (uint32_t)prop.multiProcessorCount * 4u * POOL_OCC;
	return 4096 + (size_t)*waves * pool_scratch_bytes(POOL_FUSED_CHUNKS, POOL_FUSED_HC);
}

// the pooled kernel would take this launch if it had its scratch (items and ticket are 32 bits: coop_pool.h)
int andi_coop_wants_pool(const ScanArgs &a) {
	const int nch = andi_coop_enabled();
	return a.coop && !a.exact_equal && pool_enabled() && (nch < 0 || nch == 4) && a.seg >= 32768 && (!a.route || a.pool_use) &&
		   (uint64_t)a.total_segs * a.nsub < (1ull << 32);
}

int andi_coop_will_pool(const ScanArgs &a) {
	return andi_coop_wants_pool(a) && a.pool_scratch && a.pool_waves;
}

hipError_t andi_launch_coop_cold(const ScanArgs &a, hipStream_t st) { // one segment length for the call, RAW/JC/Kimura
	const bool listed = a.coop_items && !andi_coop_will_pool(a); // (k_pool_cold keeps the grid)
	if (listed && a.n_items == 0) return hipSuccess; // (the list is empty: no pair is this kernel's)
	dim3 grid((a.total_segs + COOP_WAVES - 1) / COOP_WAVES, a.nsub);
	if (listed) grid = dim3((a.n_items - 1) / COOP_WAVES + 1, 1); // (a few rounds of the device at most: scan_call.hip)
	const int nch = andi_coop_enabled();
	// The windows' walks pooled through global memory (k_pool_cold: persistent wavefronts take the segments in order): segments long enough
	// to fill its windows; in a routed call where the pairs with long sampled matches hold most of the segments (ScanArgs.pool_use)
	// (both kernels stream the texts bit-sliced -- LogDet / ANI: the 4-bit symbols --: the subjects' planes are made with their scan indexes,
	// esa_build.hip: andi_launch_index_build)
	if (andi_coop_will_pool(a)) {
		const uint64_t items = (uint64_t)a.total_segs * a.nsub;
		ScanArgs b = a;
		b.pool_first = 64;
		if (const char *pf = andi_knob(KNOB_POOL_FIRST)) // (experiments)
			if (atoi(pf) >= 1 && atoi(pf) <= (int)POOL_FUSED_CHUNKS) b.pool_first = (uint32_t)atoi(pf);
		b.pool_maxchunks = POOL_FUSED_CHUNKS, b.pool_hc = POOL_FUSED_HC;
		hipError_t e = hipMemsetAsync(a.pool_ticket, 0, sizeof(uint32_t), st);
		if (e != hipSuccess) return e;
		k_pool_cold<<<(uint32_t)(items < a.pool_waves ? items : a.pool_waves), 64, 0, st>>>(b);
	} else
	// windows of five chunks where the segments are long enough to fill them (round 6: 4.10 -> 3.87 ms on the bench set against four -- a
	// window's walks take as many trips as its longest, whatever the number of heads); short segments of small calls keep four
	switch (nch < 0 ? (a.seg >= 32768 ? 5 : 4) : nch) {
		case 5: a.exact_equal ? k_coop_cold<5, true><<<grid, 64 * COOP_WAVES, 0, st>>>(a) : k_coop_cold<5, false><<<grid, 64 * COOP_WAVES, 0, st>>>(a); break;
		case 2: a.exact_equal ? k_coop_cold<2, true><<<grid, 64 * COOP_WAVES, 0, st>>>(a) : k_coop_cold<2, false><<<grid, 64 * COOP_WAVES, 0, st>>>(a); break;
		case 8: a.exact_equal ? k_coop_cold<8, true><<<grid, 64 * COOP_WAVES, 0, st>>>(a) : k_coop_cold<8, false><<<grid, 64 * COOP_WAVES, 0, st>>>(a); break;
		default: a.exact_equal ? k_coop_cold<4, true><<<grid, 64 * COOP_WAVES, 0, st>>>(a) : k_coop_cold<4, false><<<grid, 64 * COOP_WAVES, 0, st>>>(a); break;
	}
#ifdef ANDI_COOP_STATS
	if (andi_knob(KNOB_COOP_STATS)) {
		static const char *names[28] = {"segments", "G steps", "probe blocks", "coop_lcp calls", "windows", "windows that moved", "heads", "walk trips",
										"walk lane-steps", "walk probes", "heads on the path", "hops", "gaps counted in G", "positions covered by windows",
										"heads dropped", "walks with anchors off the diagonal", "coop_lcp rounds", "nodes", "service trips (lane_probe)", "lanes served", "parked: window edge / separators / plain table", "parked: K-mer occurs several times", "parked: long match off the diagonal", "parked: other",
										"G steps that are their segment's first", "G steps settled by one lane", "... finished by coop_lcp", "... handed to the block (not unique at the cap)"};
		unsigned long long h[28];
		(void)hipStreamSynchronize(st);
		(void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_coop_stats), sizeof h);
		for (int k = 0; k < 28; ++k) fprintf(stderr, "coop_stats %-36s %llu\n", names[k], h[k]);
		memset(h, 0, sizeof h);
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_coop_stats), h, sizeof h);
		unsigned long long tl[2][8];
		(void)hipMemcpyFromSymbol(tl, HIP_SYMBOL(g_coop_trip_lanes), sizeof tl);
		for (int k = 0; k < 2; ++k)
			fprintf(stderr, "coop_stats %s trips by lanes at work (0, 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64): %llu %llu %llu %llu %llu %llu %llu %llu\n", k ? "service" : "walk", tl[k][0], tl[k][1], tl[k][2], tl[k][3], tl[k][4], tl[k][5], tl[k][6], tl[k][7]);
		memset(tl, 0, sizeof tl);
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_coop_trip_lanes), tl, sizeof tl);
		unsigned int mx[4];
		(void)hipMemcpyFromSymbol(mx, HIP_SYMBOL(g_coop_max), sizeof mx);
		fprintf(stderr, "coop_stats most G steps of a segment          %u\n", mx[0]);
		memset(mx, 0, sizeof mx);
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_coop_max), mx, sizeof mx);
		unsigned long long cy[16];
		(void)hipMemcpyFromSymbol(cy, HIP_SYMBOL(g_coop_cycles), sizeof cy);
		static const char *ph[7] = {"(mode G: the rest)", "window: bits", "window: heads", "window: walks", "window: hops", "window: stretches", "window: counting"};
		unsigned long long in_w = 0;
		for (int k = 1; k < 7; ++k) in_w += cy[k];
		for (int k = 1; k < 7; ++k) fprintf(stderr, "coop_cycles %-24s %6.2f %%\n", ph[k], 100.0 * (double)cy[k] / (double)cy[PH_LOOP]);
		fprintf(stderr, "coop_cycles %-24s %6.2f %%\n", ph[0], 100.0 * (double)(cy[PH_LOOP] - in_w) / (double)cy[PH_LOOP]);
		// mode G's parts, and what a segment costs around its loop (all as shares of the loop's cycles; what is left of "the rest": the
		// loop's own tests, the routed call's look at the pair's mark, win.begin and the test between two windows)
		static const char *gp[7] = {"G: coop_lcp (lucky)", "G: block of 64 probes", "G: one lane's probe", "G: its coop_lcp", "G: accounting, notes", "segment: prologue", "segment: epilogue"};
		for (int k = 0; k < 7; ++k) fprintf(stderr, "coop_cycles %-24s %6.2f %%\n", gp[k], 100.0 * (double)cy[PH_G_LCP + k] / (double)cy[PH_LOOP]);
		fprintf(stderr, "coop_cycles %-24s %.4f G (100 %%; shares of two builds compare through this)\n", "the segments' loops", 1e-9 * (double)cy[PH_LOOP]);
		memset(cy, 0, sizeof cy);
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_coop_cycles), cy, sizeof cy);
	}
#endif
	return hipGetLastError();
}
