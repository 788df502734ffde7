// api_internal.h — what the library's host translation units share (api.hip, scan_call.hip, seam.hip and the tree calls
// on rep_groups.h and nj_sets.h): the objects behind the C-ABI's handles, the error helpers, the scope of a call's device
// buffers (DevScope), the size of a group (nj_group_size), and the helpers the scan call and the seam take from api.hip.
// Private: no kernel code, nothing of it is exported (the functions declared here are hidden).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <string>
#include <vector>

#include "andi_dev.h"
#include "andi_hip.h"
#include "dev_arena.h"
#include "esa_build.h"
#include "knobs.h"
#include "scan.h"

// scratch per (subject, segment): three states, two count vectors, the marks, the exit position, a list slot, a published anchor
#define ANDI_SLOT_BYTES (3 * sizeof(ChainState) + 2 * 16 * sizeof(uint32_t) + ANDI_COLD_MARKS * sizeof(ColdMark) + 4 + 8 + 8)

struct EventPair {
	hipEvent_t a, b;
	int kind; // 0 build, 1 scan, 2 stitch
};

struct andi_hip_ctx {
	int device = 0;
	size_t queries_hint = 0; // andi_hip_ctx_expect_queries
	hipStream_t stream = nullptr;
	hipStream_t side_stream = nullptr; // pass A's second kernel runs beside the first
	hipEvent_t side_fork = nullptr, side_join = nullptr;
	std::string err;
	// scan scratch
	void *scratch = nullptr;
	size_t scratch_bytes = 0;
	// descriptor staging (pinned host + device), guarded by desc_done
	void *desc_host = nullptr;
	void *desc_dev = nullptr;
	size_t desc_bytes = 0;
	hipEvent_t desc_done = nullptr;
	unsigned long long *d_fixups = nullptr;
	// batched index builds: items (pinned host + device), guarded by ib_done
	void *ib_host = nullptr, *ib_dev = nullptr;
	size_t ib_cap = 0;
	hipEvent_t ib_done = nullptr;
	// index builds queued since the last scan looked at their flags (pinned host words the build kernels write)
	hipEvent_t built = nullptr;
	bool builds_pending = false;
	// device suffix sorter: workspace, two pinned ints
	void *sa_ws = nullptr;
	size_t sa_ws_bytes = 0;
	int32_t *sa_pinned = nullptr;
	int stream_prio = 0; // of stream and side_stream (host_pool: they go back there)
	uint32_t *h_quad_waves = nullptr; // pinned: the length of k_lane_quad's list of a scan call
	hipStream_t coop_stream = nullptr; // routed scan calls: pass A by wavefronts runs beside the lane scan's kernels
	hipEvent_t coop_fork = nullptr, coop_join = nullptr, l2_fork = nullptr, l2_join = nullptr;
	// pinned, 64 words: [0] the wavefront kernel handed some pair back, [1 + k] the layout's counter restitch_count[k] (ANDI_LANE_WAVES: wavefronts of
	// the lane layout, ...) at the first look, [ANDI_LOOK_B + k] restitch_count[k] of the wavefront kernel's layout at the look behind its pass A
	uint32_t *h_any_left = nullptr;
	void *pool_scratch = nullptr;      // pass A by wavefronts with pooled walks (coop_pool.h): a scratch per resident wavefront
	size_t pool_bytes = 0;
	uint32_t pool_waves = 0;
	bool pool_failed = false;          // its allocation failed once: not tried again by this context
	void *scratch2 = nullptr;          // the second lane layout (those pairs), grown on demand
	size_t scratch2_bytes = 0;
	uint32_t round_waves = 0; // resident wavefronts of k_coop_cold on this device: a round of pass A by wavefronts (scan_call.hip: carve_scratch)
	// the last routed call's list of the wavefront kernel's segments, in the call's scratch (scan.h: coop_items; null: the call had none), with
	// the pairs' classes and cost classes -- what the suite's hook andi_hip_test_coop_items reads
	struct {
		const uint32_t *items = nullptr;
		const uint8_t *pair_class = nullptr, *pair_cost = nullptr;
		uint32_t n_items = 0, pairs = 0, total_segs = 0;
		// (andi_hip_test_pair_layout) the lane layout's arrays in the call's scratch -- pair_wave0 only where the lanes' segment lengths are per
		// pair --, its subjects, and its sixteen counters as the host's first look saw them (looked: the call did look)
		const uint32_t *pair_waves = nullptr, *pair_wave0 = nullptr, *sub_order = nullptr;
		uint32_t nsub = 0, looked = 0, counts[16] = {};
	} last_items;
	unsigned long long *d_route = nullptr; // routed scan calls: query nucleotides whose pass A ran by wavefronts / by lanes, pairs handed back (read with the timings)
	std::vector<EventPair> pending;
	std::vector<hipEvent_t> idle_events; // the timers' events between uses (Timed, resolve_events): created once, destroyed with the context
	andi_hip_timings acc{};
#ifdef ANDI_TEST_HOOKS
	// (the suite's library only: every translation unit that sees this struct is compiled a second time for it, Makefile: HOOKOBJ)
	// the last scan call that used ONE segment length (not routed, no per-pair lengths): the per-slot arrays of lane layout a in the call's
	// scratch and their geometry -- what the suite's hook andi_hip_test_stitch_slots reads.  Cleared at every call's start, so by a call that
	// takes another path and before the scratch is regrown; the scratch is freed only with the context.
	struct {
		const ChainState *cold_exit = nullptr, *true_exit = nullptr, *used_entry = nullptr;
		const uint32_t *cold_counts = nullptr, *owned = nullptr, *restitch_count = nullptr;
		const ColdMark *marks = nullptr;
		uint32_t nsub = 0, total_segs = 0, seg = 0;
	} last_slots;
	// the last routed scan call, per layout (0 a: the lane scan's, 1 b: the wavefront kernel's, 2 a2: the pairs handed back): whether its pass A
	// was enqueued and how many rounds of stitching again were, and where pass B of layout b counted -- what the suite's hook andi_hip_test_call_edges reads
	struct {
		uint32_t pass_a[3] = {0, 0, 0}, rounds[3] = {0, 0, 0};
		uint32_t went_ahead = 0, ran_again = 0; // the call did not wait for the pending builds (upload_descriptors); a raised flag made it run again
		const uint32_t *count_b = nullptr; // layout b's restitch_count, in the call's scratch
	} last_edges;
#endif
};
#define ANDI_LOOK_B 32 /* andi_hip_ctx.h_any_left: where the second look's sixteen words go */

struct andi_hip_esa {
	uint8_t *S = nullptr;
	int32_t *SA = nullptr, *LCP = nullptr, *CLD = nullptr;
	uint8_t *FVC = nullptr;
	int4 *tab = nullptr;
	int32_t *min_scratch = nullptr;
	uint2 *deep = nullptr;
	uint8_t *Nraw = nullptr;              // 4-bit symbols for the lane scan: N0 and N1 with their padding
	uint8_t *N0 = nullptr, *N1 = nullptr;
	uint32_t *Praw = nullptr, *P = nullptr; // the text bit-sliced (EsaDev.P; packed from N0 when a scan call wants it), a block of padding in front
	uint32_t *rec = nullptr;    // the suffixes' records in suffix-array order, left by the device sorter (sa_device.hip) for the index build
	bool rec_valid = false;
	uint16_t *rec2 = nullptr;   // ... and the symbols behind their first deepK (same validity)
	int32_t *flags = nullptr;   // device, 4 ints
	int32_t *h_flags = nullptr; // the same 4 ints as the host sees them (flags live in pinned host memory)
	int32_t deepK = 0;
	int32_t deepK_cap = 0; // the depth the table was allocated for
	int32_t n = 0;
	int32_t thr = 0;
	size_t cap = 0;     // characters the buffers were sized for (>= n)
	size_t ref_cap = 0; // same for the reference arrays
	bool ref_built = false;   // LCP, CLD, FVC, tab valid
	bool index_built = false; // deep, flags valid
	int deep_ext = 0;         // the form of the table's entries of K-mers that occur once (andi_dev.h: 0 plain, 1 extended, 2 short extended)
	size_t bytes = 0;
};

struct andi_hip_queries {
	// a view (andi_hip_queries_view) shares its parent's pool, nib, planes, codes and h_foreign, and its d_off, d_len and d_sep point
	// into the parent's arrays; it owns only its segmentation caches
	bool owns_pool = true;
	uint8_t *pool = nullptr;
	uint8_t *nib = nullptr;       // the pool as 4-bit symbols
	uint32_t *planes = nullptr;   // ... bit-sliced (EsaDev.P)
	uint32_t *codes = nullptr;    // ... as interleaved 2-bit codes of bits 0 and 1, two words per block of 32 symbols (ScanArgs.qcodes)
	int32_t *h_foreign = nullptr; // pinned: set if the pool holds bytes outside the alphabet
	uint64_t *d_off = nullptr;
	uint32_t *d_len = nullptr;
	uint32_t *d_sep = nullptr;    // contig separators of every sequence (k_sep_counts: for the routing of the scan)
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	size_t nq = 0;
	uint64_t total_nt = 0;
	// segmentation cache
	uint32_t seg = 0;
	uint32_t *d_qseg_start = nullptr;
	uint32_t *d_seg2query = nullptr;
	uint32_t total_segs = 0;
	// a second one: the long segments of pass A by wavefronts (scan_coop.hip), kept beside the call's own so that a
	// call that falls back to the lane scan does not cut the queries anew every time
	uint32_t c_seg = 0;
	uint32_t *c_qseg_start = nullptr;
	uint32_t *c_seg2query = nullptr;
	uint32_t c_total_segs = 0;
};

namespace {

void set_err(char *buf, size_t len, const char *fmt, ...) {
	if (!buf || !len) return;
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, len, fmt, ap);
	va_end(ap);
}

int fail(andi_hip_ctx *ctx, const char *what, hipError_t e) {
	if (ctx) {
		ctx->err = std::string(what) + ": " + hipGetErrorString(e);
	}
	return 1;
}

#define HIP_TRY(ctx, call)                                                                         \
	do {                                                                                           \
		hipError_t e__ = (call);                                                                   \
		if (e__ != hipSuccess) return fail((ctx), #call, e__);                                     \
	} while (0)

template <typename T>
hipError_t dmalloc(T **p, size_t count) {
	return andi_arena::dev_malloc((void **)p, count * sizeof(T)); // (out of large chunks: dev_arena.h)
}

// The device buffers of one call.  alloc() is dmalloc() that remembers what it handed out and does nothing once an
// allocation has failed (err keeps the first failure, so a run of allocs is checked once, behind it).  release() waits
// for the stream -- nothing in flight uses the buffers then, also on an error exit --, gives them all back and leaves
// the scope as new, for a caller that tries again with less (rep_groups.h); the scope's end is a release().
struct DevScope {
	hipStream_t stream;
	hipError_t err = hipSuccess;
	std::vector<void *> held;
	explicit DevScope(hipStream_t st) : stream(st) {}
	template <typename T>
	void alloc(T **p, size_t count) {
		if (err == hipSuccess && (err = dmalloc(p, count)) == hipSuccess) held.push_back(*p);
	}
	void release() {
		(void)hipStreamSynchronize(stream);
		for (void *p : held) (void)andi_arena::dev_free(p, false);
		held.clear();
		err = hipSuccess;
	}
	~DevScope() { release(); }
	DevScope(const DevScope &) = delete;
	DevScope &operator=(const DevScope &) = delete;
};

// The members of one group, for every call that takes its items some at a time (the replicates of rep_groups.h and
// nj_sets.h, place.hip's queries): as many as `budget` bytes of device memory hold at `each` bytes per member -- at least
// one, at most `max`, what the grid dimension they go by takes.  `knob` is the call's test hook (ANDI_NJ_GROUP,
// ANDI_PLACE_GROUP): a size of the test's choosing, within the same bounds.
size_t nj_group_size(AndiKnob knob, size_t max, size_t budget, size_t each) {
	size_t G = budget / each;
	if (const char *v = andi_knob(knob))
		if (atoll(v) >= 1) G = (size_t)atoll(v);
	return G < 1 ? 1 : G > max ? max : G;
}

void resolve_events(andi_hip_ctx *ctx) {
	for (auto &ev : ctx->pending) {
		float ms = 0.f;
		if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
			if (ev.kind == 0) {
				ctx->acc.build_ms += ms;
				ctx->acc.build_launches++;
			} else if (ev.kind == 1) {
				ctx->acc.scan_ms += ms;
				ctx->acc.scan_launches++;
			} else {
				ctx->acc.stitch_ms += ms;
				ctx->acc.stitch_launches++;
			}
		}
		ctx->idle_events.push_back(ev.a); // (for the next timer: creating and destroying two events per timer, six to eight per scan call, was
		ctx->idle_events.push_back(ev.b); // time of the host thread the device waits for behind every look of a routed call)
	}
	ctx->pending.clear();
}

struct Timed {
	andi_hip_ctx *ctx;
	EventPair ev;
	bool ok;
	static bool take(andi_hip_ctx *c, hipEvent_t *e) { // an idle event of the context's, or a new one
		if (c->idle_events.empty()) return hipEventCreate(e) == hipSuccess;
		*e = c->idle_events.back();
		c->idle_events.pop_back();
		return true;
	}
	void give_back() {
		ctx->idle_events.push_back(ev.a);
		ctx->idle_events.push_back(ev.b);
	}
	Timed(andi_hip_ctx *c, int kind) : ctx(c), ok(false) {
		ev.kind = kind;
		if (!take(c, &ev.a)) return;
		if (!take(c, &ev.b)) {
			c->idle_events.push_back(ev.a);
			return;
		}
		ok = hipEventRecord(ev.a, c->stream) == hipSuccess;
		if (!ok) give_back();
	}
	void stop() {
		if (!ok) return;
		(void)hipEventRecord(ev.b, ctx->stream);
		ctx->pending.push_back(ev);
		ok = false;
		if (ctx->pending.size() > 256) resolve_events(ctx);
	}
	~Timed() { // an error exit before stop(): the events go back unused
		if (ok) give_back();
	}
	Timed(const Timed &) = delete;
	Timed &operator=(const Timed &) = delete;
};

} // namespace

// The seam's queries, packed ONCE on the host (round 4): every device uploads the 4-bit pool -- a quarter of what the
// byte pool and its packed copy were, from one host copy shared by the device threads -- and unpacks the bytes the rare
// byte-wise paths read (k_unpack_symbols).  C4's 6.5 GB of queries took 0.35 s per device as bytes from pageable memory.
struct PackedQueries {
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	uint64_t total_nt = 0;
	size_t pool_bytes = 0;
	uint8_t *nib = nullptr; // pool_bytes / 2 bytes: the pool as the device's pack kernel would leave it
	int foreign = 0;        // a byte outside the alphabet (the scan refuses the queries then)
	std::string err;
	std::atomic<int> users{0}; // devices that have not staged yet: the last one lets the host copy go (gigabytes: not at the call's end)
	void release() {
		free(nib);
		nib = nullptr;
	}
	~PackedQueries() { release(); }
};

#pragma GCC visibility push(hidden)

// api.hip
EsaDev esa_view(const andi_hip_esa *e, int mode);
int pick_deep_k(size_t n, size_t queries);
int ctx_create(andi_hip_ctx **out, int device, char *errbuf, size_t errlen, bool high_priority);
int esa_reserve(andi_hip_ctx *ctx, size_t cap, andi_hip_esa **out);
int esa_upload(andi_hip_ctx *ctx, andi_hip_esa *e, const char *RS, const int32_t *SA, size_t n,
			   size_t threshold, hipEvent_t done = nullptr); // done: do not wait -- the event says when RS (and SA) may be reused
int esa_from_query(andi_hip_ctx *ctx, andi_hip_esa *e, const andi_hip_queries *Q, size_t i, size_t threshold);
int queries_gc_counts(andi_hip_ctx *ctx, const andi_hip_queries *Q, std::vector<unsigned long long> &out);
int esa_sort_suffixes(andi_hip_ctx *ctx, andi_hip_esa *e);

int pack_queries_host(const andi_hip_seq *seqs, size_t n, int threads, PackedQueries &P);
int queries_stage_packed(andi_hip_ctx *ctx, const PackedQueries &P, andi_hip_queries **out);

// Streams, pinned buffers and the pooled kernel's scratch kept from one call to the next (api.hip: ONE pool per process)
namespace host_pool {
hipError_t stream_get(hipStream_t *out, int device, int prio);
void stream_put(hipStream_t s, int device, int prio);
hipError_t pinned_get(void **out, size_t bytes);
void pinned_put(void *p, size_t bytes);
void *word_get();
void word_put(void *p);
void *scratch_get(int device, size_t bytes);
void scratch_put(int device, void *p, size_t bytes);
} // namespace host_pool

#pragma GCC visibility pop
