// api.hip — the C-ABI of libandihip.so (include/andi_hip.h): contexts, subjects, queries and the small calls.  The scan
// call is scan_call.hip, the one-call replacement of distMatrix/distMatrixLM (src/dist_hack.h:34-96) seam.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <sys/mman.h>
#include <vector>

#include "api_internal.h"
#include "andi_dev.h"
#include "andi_hip.h"
#include "bootstrap.h"
#include "dev_arena.h"
#include "esa_build.h"
#include "knobs.h"
#include "sa_device.h"
#include "scan.h"

// ------------------------------------------------------------------ knobs (knobs.h)
namespace {
// The switches as they were when last read: an immutable snapshot behind an atomic pointer.  andi_hip_reload_knobs
// publishes a new one and never frees the old (a handful of them in a test session): a string andi_knob returned stays
// valid whatever other threads do.
struct KnobSnapshot {
	std::string value[KNOB_COUNT];
	bool set[KNOB_COUNT];
	KnobSnapshot() {
		static const char *names[KNOB_COUNT] = {
#define X(n) "ANDI_" #n,
			ANDI_KNOB_LIST(X)
#undef X
		};
		for (int k = 0; k < KNOB_COUNT; ++k) {
#ifndef ANDI_TEST_HOOKS
			if (k >= ANDI_KNOBS_SHIPPED) { // (the shipped library does not even look)
				set[k] = false;
				continue;
			}
#endif
			const char *v = getenv(names[k]);
			set[k] = v != nullptr;
			value[k] = v ? v : "";
		}
	}
};
std::atomic<const KnobSnapshot *> g_knobs{nullptr};
const KnobSnapshot &knob_store() {
	const KnobSnapshot *s = g_knobs.load(std::memory_order_acquire);
	if (!s) { // (read when the library first looks)
		const KnobSnapshot *fresh = new KnobSnapshot();
		if (g_knobs.compare_exchange_strong(s, fresh, std::memory_order_acq_rel))
			s = fresh;
		else
			delete fresh;
	}
	return *s;
}
} // namespace

const char *andi_knob_value(AndiKnob k) {
	const KnobSnapshot &s = knob_store();
	return s.set[k] ? s.value[k].c_str() : nullptr;
}


static_assert(sizeof(andi_hip_model) == 68, "struct model must be 17 x u32 (src/model.h:52-57)");
static_assert(sizeof(andi_hip_interval) == 16, "lcp_inter_t is 4 x int32 (src/esa.h:25-34)");
static_assert(sizeof(ChainState) == 32, "ChainState is padded to 32 bytes");
static_assert(sizeof(ColdMark) == 112, "ColdMark is a state, 16 counts and the first anchor");

EsaDev esa_view(const andi_hip_esa *e, int mode) {
	EsaDev v;
	v.S = e->S, v.SA = e->SA, v.LCP = e->LCP, v.CLD = e->CLD, v.FVC = e->FVC, v.tab = e->tab;
	v.deep = e->deep, v.flags = e->flags;
	v.N0 = e->N0, v.N1 = e->N1, v.P = e->P;
	v.R2 = e->rec_valid ? e->rec2 : nullptr; // (made by the device sorter for this K: api.hip esa_sort_suffixes)
	v.n = e->n, v.thr = e->thr, v.deepK = e->deepK, v.mode = mode, v.deep_ext = e->deep_ext;
	return v;
}

// probe table depth: smallest K with 4^K >= n, within [4, 13]
// (queries: how many queries a subject of this context will meet, 0 = unknown.  A table one level deeper answers more
// probes without touching the text -- pass A of a C4-shaped call 53.2 -> 50.0 ms -- and costs its build four times the
// stores -- 0.06 -> 0.19 ms per 4.2 M-character subject: it pays from about a thousand queries per subject on.)
int pick_deep_k(size_t n, size_t queries) {
	int K = 4;
	while (K < ANDI_MAX_DEEP_K && ((size_t)1 << (2 * K)) < n) ++K;
	if (queries >= 1024 && K < ANDI_MAX_DEEP_K) ++K;
	if (const char *ev = andi_knob(KNOB_DEEP_K)) {
		int v = atoi(ev);
		if (v >= 4 && v <= ANDI_MAX_DEEP_K) K = v;
	}
	return K;
}

namespace {

EsaBuildArgs build_args(const andi_hip_esa *e) {
	EsaBuildArgs a;
	a.S = e->S, a.SA = e->SA, a.LCP = e->LCP, a.CLD = e->CLD, a.FVC = e->FVC, a.tab = e->tab;
	a.deep = e->deep, a.flags = e->flags, a.deepK = e->deepK;
	a.rec = e->rec_valid ? e->rec : nullptr;
	a.rec2 = e->rec_valid ? e->rec2 : nullptr;
	a.N0 = e->N0, a.N1 = e->N1, a.P = e->P;
	a.min_scratch = e->min_scratch;
	a.n = e->n;
	return a;
}

} // namespace

// Streams and the seam's pinned upload buffer are kept from one call to the next (like the arena's chunks: andi_hip_trim
// gives them back): creating a stream takes 3 ms on this runtime -- nine per call of andi_hip_dist_matrix, 30 of a warm
// call's 105 ms -- and pinning 20 MB another 4.
namespace host_pool {
struct IdleStream {
	int device, prio;
	hipStream_t s;
};
struct IdlePinned {
	void *p;
	size_t bytes;
};
struct IdleScratch { // k_pool_cold's scratch (0.8 GB on a 256-CU part: a mapping of its own, not the arena's)
	int device;
	void *p;
	size_t bytes;
};
// The pool's state lives on the heap and is never destroyed (as dev_arena.h's arenas): a context may be released during or
// after the destruction of this library's statics, and its streams come back here.
struct State {
	std::mutex mu;
	std::vector<IdleStream> streams;
	std::vector<IdlePinned> pinned;
	std::vector<IdleScratch> scratch;
	// small pinned blocks (flags and counters the kernels write and the host reads: 16 ... 256 bytes each) out of slabs of
	// 64 KiB: a context and its subjects took two dozen hipHostMalloc / hipHostFree of a few words per call of the seam,
	// 5 of a warm call's 36 ms
	std::vector<char *> slabs;
	std::vector<void *> free_words;
	size_t words_out = 0;
};
static State &state() {
	static State *s = new State;
	return *s;
}
constexpr size_t PINNED_KEEP = (size_t)256 << 20; // bytes of pinned buffers kept at most

hipError_t stream_get(hipStream_t *out, int device, int prio) {
	{
		std::lock_guard<std::mutex> lk(state().mu);
		for (size_t i = 0; i < state().streams.size(); ++i)
			if (state().streams[i].device == device && state().streams[i].prio == prio) {
				*out = state().streams[i].s;
				state().streams.erase(state().streams.begin() + (long)i);
				return hipSuccess;
			}
	}
	return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
}
void stream_put(hipStream_t s, int device, int prio) { // (idle: the caller has synchronised it)
	if (!s) return;
	std::lock_guard<std::mutex> lk(state().mu);
	state().streams.push_back({device, prio, s});
}
hipError_t pinned_get(void **out, size_t bytes) {
	{
		std::lock_guard<std::mutex> lk(state().mu);
		size_t best = state().pinned.size();
		for (size_t i = 0; i < state().pinned.size(); ++i)
			if (state().pinned[i].bytes >= bytes && state().pinned[i].bytes <= 2 * bytes + 4096 && (best == state().pinned.size() || state().pinned[i].bytes < state().pinned[best].bytes)) best = i;
		if (best != state().pinned.size()) {
			*out = state().pinned[best].p;
			state().pinned.erase(state().pinned.begin() + (long)best);
			return hipSuccess;
		}
	}
	return hipHostMalloc(out, bytes, hipHostMallocDefault);
}
void pinned_put(void *p, size_t bytes) {
	if (!p) return;
	{
		std::lock_guard<std::mutex> lk(state().mu);
		size_t held = 0;
		for (const IdlePinned &b : state().pinned) held += b.bytes;
		if (held + bytes <= PINNED_KEEP) {
			state().pinned.push_back({p, bytes});
			return;
		}
	}
	(void)hipHostFree(p);
}
constexpr size_t WORD_BYTES = 256, SLAB_BYTES = 65536;
void *word_get() { // 256 zeroed bytes of pinned host memory (device-visible: unified addressing), 256-byte aligned
	std::lock_guard<std::mutex> lk(state().mu);
	State &S = state();
	if (S.free_words.empty()) {
		char *slab = nullptr;
		if (hipHostMalloc((void **)&slab, SLAB_BYTES, hipHostMallocDefault) != hipSuccess) {
			(void)hipGetLastError();
			return nullptr;
		}
		S.slabs.push_back(slab);
		for (size_t o = SLAB_BYTES; o >= WORD_BYTES; o -= WORD_BYTES) S.free_words.push_back(slab + o - WORD_BYTES);
	}
	void *p = S.free_words.back();
	S.free_words.pop_back();
	++S.words_out;
	memset(p, 0, WORD_BYTES);
	return p;
}
void word_put(void *p) {
	if (!p) return;
	std::lock_guard<std::mutex> lk(state().mu);
	state().free_words.push_back(p);
	--state().words_out;
}

// the pooled wavefront kernel's scratch: one per device is kept from context to context (a context of the seam lives for one
// call: 0.8 GB of hipMalloc + hipFree per call and device otherwise); andi_hip_trim returns it
void *scratch_get(int device, size_t bytes) {
	{
		std::lock_guard<std::mutex> lk(state().mu);
		auto &v = state().scratch;
		for (size_t i = 0; i < v.size(); ++i)
			if (v[i].device == device && v[i].bytes == bytes) {
				void *p = v[i].p;
				v.erase(v.begin() + (long)i);
				return p;
			}
	}
	void *p = nullptr;
	if (hipMalloc(&p, bytes) != hipSuccess) {
		(void)hipGetLastError();
		return nullptr;
	}
	return p;
}
void scratch_put(int device, void *p, size_t bytes) { // (idle: the caller has waited for the kernels that used it)
	if (!p) return;
	{
		std::lock_guard<std::mutex> lk(state().mu);
		auto &v = state().scratch;
		bool have = false;
		for (const IdleScratch &x : v) have = have || x.device == device;
		if (!have) {
			v.push_back({device, p, bytes});
			return;
		}
	}
	(void)hipFree(p);
}
static bool any() {
	std::lock_guard<std::mutex> lk(state().mu);
	return !state().streams.empty() || !state().pinned.empty() || !state().scratch.empty() || !state().slabs.empty();
}
static size_t trim() { // (the caller restores the current device); returns the device bytes given back
	std::vector<IdleStream> st;
	std::vector<IdlePinned> pb;
	std::vector<IdleScratch> sc;
	{
		std::lock_guard<std::mutex> lk(state().mu);
		st.swap(state().streams), pb.swap(state().pinned), sc.swap(state().scratch);
		if (state().words_out == 0) { // (slabs with blocks still out stay)
			for (char *slab : state().slabs) pb.push_back({slab, SLAB_BYTES});
			state().slabs.clear(), state().free_words.clear();
		}
	}
	for (const IdleStream &x : st)
		if (hipSetDevice(x.device) == hipSuccess) (void)hipStreamDestroy(x.s);
	for (const IdlePinned &b : pb) (void)hipHostFree(b.p);
	size_t freed = 0;
	for (const IdleScratch &x : sc)
		if (hipSetDevice(x.device) == hipSuccess && hipFree(x.p) == hipSuccess) freed += x.bytes;
	return freed;
}
} // namespace host_pool

int andi_hip_abi_version(void) {
	return ANDI_HIP_ABI_VERSION;
}

size_t andi_hip_trim(void) {
	if (!andi_arena::any_chunks() && !host_pool::any()) return 0; // (a process that never used the library's device memory: no HIP call at all)
	int ndev = 0, cur = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess) {
		(void)hipGetLastError();
		return 0;
	}
	(void)hipGetDevice(&cur);
	size_t freed = 0;
	for (int d = 0; d < ndev && d < 64; ++d) {
		if (!andi_arena::has_chunks(d)) continue; // (a device the library never used is not touched)
		if (hipSetDevice(d) != hipSuccess) continue;
		freed += andi_arena::trim(d);
	}
	freed += host_pool::trim(); // (idle streams, pinned upload buffers, the pooled kernel's scratch)
	(void)hipSetDevice(cur);
	return freed;
}

void andi_hip_default_opts(andi_hip_opts *o) {
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->p_value = 0.025; // ANCHOR_P_VALUE, src/andi.c:48
	o->model = ANDI_M_JC;
	o->device = 0;
	o->host_threads = 0;
	o->low_memory = 0;
	o->segment = 0;
	o->sa_on_host = 0;
	o->num_gpus = 1;
	o->devices = NULL;
}

int andi_hip_device_count(void) {
	int count = 0;
	return hipGetDeviceCount(&count) == hipSuccess && count > 0 ? count : 0;
}

// high_priority: the context's streams are served before those of other contexts on the device (the staging stage of
// andi_hip_dist_matrix: its short kernels must not queue behind the workgroups of a scan that fills the device)
int ctx_create(andi_hip_ctx **out, int device, char *errbuf, size_t errlen, bool high_priority) {
	if (!out) return 1;
	*out = nullptr;
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0) {
		set_err(errbuf, errlen, "no HIP device available (%s); the anchor-distance engine has no CPU path",
				e != hipSuccess ? hipGetErrorString(e) : "device count 0");
		return 1;
	}
	if (device < 0 || device >= count) {
		set_err(errbuf, errlen, "HIP device %d out of range (have %d)", device, count);
		return 1;
	}
	e = hipSetDevice(device);
	if (e != hipSuccess) {
		set_err(errbuf, errlen, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
		return 1;
	}
	auto *ctx = new andi_hip_ctx;
	ctx->device = device;
	andi_arena::retain(device); // (released in andi_hip_ctx_destroy)
	int prio = 0;
	if (high_priority) {
		int least = 0, greatest = 0;
		if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) prio = greatest;
	}
	ctx->stream_prio = prio;
	e = host_pool::stream_get(&ctx->stream, device, prio);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->side_join, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->desc_done, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->built, hipEventDisableTiming);
	if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_fixups, sizeof(unsigned long long));
	if (e == hipSuccess) e = hipMemset(ctx->d_fixups, 0, sizeof(unsigned long long));
	if (e == hipSuccess && !(ctx->h_quad_waves = (uint32_t *)host_pool::word_get())) e = hipErrorOutOfMemory;
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->coop_fork, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->coop_join, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->l2_fork, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->l2_join, hipEventDisableTiming);
	if (e == hipSuccess && !(ctx->h_any_left = (uint32_t *)host_pool::word_get())) e = hipErrorOutOfMemory;
	if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_route, 4 * sizeof(unsigned long long));
	if (e == hipSuccess) e = hipMemset(ctx->d_route, 0, 4 * sizeof(unsigned long long));
	if (e != hipSuccess) {
		set_err(errbuf, errlen, "context setup: %s", hipGetErrorString(e));
		andi_hip_ctx_destroy(ctx);
		return 1;
	}
	*out = ctx;
	return 0;
}

int andi_hip_ctx_create(andi_hip_ctx **out, int device, char *errbuf, size_t errlen) {
	return ctx_create(out, device, errbuf, errlen, false);
}

void andi_hip_ctx_expect_queries(andi_hip_ctx *ctx, size_t queries) {
	if (ctx) ctx->queries_hint = queries;
}

void andi_hip_ctx_destroy(andi_hip_ctx *ctx) {
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	resolve_events(ctx);
	for (hipEvent_t ev : ctx->idle_events) (void)hipEventDestroy(ev);
	ctx->idle_events.clear();
	if (ctx->scratch) (void)andi_arena::dev_free(ctx->scratch);
	if (ctx->desc_dev) (void)andi_arena::dev_free(ctx->desc_dev);
	if (ctx->desc_host) host_pool::pinned_put(ctx->desc_host, ctx->desc_bytes);
	if (ctx->d_fixups) (void)andi_arena::dev_free(ctx->d_fixups);
	if (ctx->ib_dev) (void)andi_arena::dev_free(ctx->ib_dev);
	if (ctx->ib_host) host_pool::pinned_put(ctx->ib_host, ctx->ib_cap * sizeof(AndiIndexBatchItem));
	if (ctx->ib_done) (void)hipEventDestroy(ctx->ib_done);
	if (ctx->built) (void)hipEventDestroy(ctx->built);
	if (ctx->sa_ws) (void)andi_arena::dev_free(ctx->sa_ws);
	host_pool::word_put(ctx->sa_pinned);
	host_pool::word_put(ctx->h_quad_waves);
	if (ctx->d_route) (void)andi_arena::dev_free(ctx->d_route);
	if (ctx->scratch2) (void)andi_arena::dev_free(ctx->scratch2);
	if (ctx->pool_scratch) { // (kept for the device's next context: host_pool)
		(void)hipDeviceSynchronize();
		host_pool::scratch_put(ctx->device, ctx->pool_scratch, ctx->pool_bytes + 4096);
	}
	host_pool::word_put(ctx->h_any_left);
	if (ctx->coop_stream) {
		(void)hipStreamSynchronize(ctx->coop_stream);
		host_pool::stream_put(ctx->coop_stream, ctx->device, 0);
	}
	if (ctx->coop_fork) (void)hipEventDestroy(ctx->coop_fork);
	if (ctx->coop_join) (void)hipEventDestroy(ctx->coop_join);
	if (ctx->l2_fork) (void)hipEventDestroy(ctx->l2_fork);
	if (ctx->l2_join) (void)hipEventDestroy(ctx->l2_join);
	if (ctx->desc_done) (void)hipEventDestroy(ctx->desc_done);
	if (ctx->side_stream) {
		(void)hipStreamSynchronize(ctx->side_stream);
		host_pool::stream_put(ctx->side_stream, ctx->device, ctx->stream_prio);
	}
	if (ctx->side_fork) (void)hipEventDestroy(ctx->side_fork);
	if (ctx->side_join) (void)hipEventDestroy(ctx->side_join);
	if (ctx->stream) {
		(void)hipStreamSynchronize(ctx->stream); // (events resolved above may have left work behind them)
		host_pool::stream_put(ctx->stream, ctx->device, ctx->stream_prio);
	}
	andi_arena::release(ctx->device); // (the device's last context gives its free chunks back)
	delete ctx;
}

const char *andi_hip_last_error(const andi_hip_ctx *ctx) {
	return ctx ? ctx->err.c_str() : "no context";
}

int andi_hip_sync(andi_hip_ctx *ctx) {
	if (!ctx) return 1;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return 0;
}

int andi_hip_dev_alloc(andi_hip_ctx *ctx, size_t bytes, void **dptr) {
	if (!ctx || !dptr) return 1;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : 1));
	return 0;
}

void andi_hip_dev_free(andi_hip_ctx *ctx, void *dptr) {
	if (!ctx || !dptr) return;
	(void)hipSetDevice(ctx->device);
	(void)andi_arena::dev_free(dptr);
}

int andi_hip_copy_to_host(andi_hip_ctx *ctx, void *dst, const void *src, size_t bytes) {
	if (!ctx) return 1;
	HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return 0;
}

// ------------------------------------------------------------------ subjects
// Allocate a subject slot able to hold an RS of up to `cap` characters.
int esa_reserve(andi_hip_ctx *ctx, size_t cap, andi_hip_esa **out) {
	auto *e = new andi_hip_esa;
	e->cap = cap;
	hipError_t err = hipSuccess;
	auto chk = [&](hipError_t x) {
		if (err == hipSuccess) err = x;
	};
	e->deepK_cap = pick_deep_k(cap, ctx->queries_hint);
	const size_t deep_entries = (size_t)1 << (2 * e->deepK_cap);
	chk(dmalloc(&e->S, cap + 1 + ANDI_PAD));
	chk(dmalloc(&e->SA, cap + 8)); // +8: the scan reads the occurrences of a repeated K-mer eight entries at a time
	chk(dmalloc(&e->deep, deep_entries + 2)); // +2: entries are fetched with 16-byte loads
	// symbols: [front][N0: cap/2 + 1 + back][front][N1: same]; N0 and N1 start on a 256-byte boundary, the
	// paddings (NUL symbols) let whole lines of the text be fetched around any window the scan may ask for
	const size_t nib_part = (cap / 2 + 1 + ANDI_NIB_BACK + 255) & ~(size_t)255;
	chk(dmalloc(&e->Nraw, 2 * (ANDI_NIB_FRONT + nib_part)));
	if (err == hipSuccess) {
		e->N0 = e->Nraw + ANDI_NIB_FRONT, e->N1 = e->Nraw + ANDI_NIB_FRONT + nib_part + ANDI_NIB_FRONT;
		chk(hipMemsetAsync(e->Nraw, 0x77, 2 * (ANDI_NIB_FRONT + nib_part), ctx->stream));
	}
	{ // the text bit-sliced: 12 bytes per 32 symbols, a block in front, the padding all ones (NUL symbols)
		const size_t blocks = (cap + 1 + 4096) / 32 + 4;
		chk(dmalloc(&e->Praw, 3 * blocks));
		if (err == hipSuccess) {
			e->P = e->Praw + 3;
			chk(hipMemsetAsync(e->Praw, 0xff, 3 * blocks * sizeof(uint32_t), ctx->stream));
		}
	}
	// flags: pinned host memory the kernels write directly (rare, idempotent plain stores) --
	// no per-build memset or copy; the host reads them after a stream synchronisation
	if (!(e->h_flags = (int32_t *)host_pool::word_get())) chk(hipErrorOutOfMemory);
	if (err == hipSuccess) chk(hipHostGetDevicePointer((void **)&e->flags, e->h_flags, 0));
	e->bytes = (cap + 1 + ANDI_PAD) + 4 * cap + 8 * deep_entries + 80 +
			   2 * (ANDI_NIB_FRONT + nib_part);
	if (err != hipSuccess) {
		andi_hip_esa_free(ctx, e);
		return fail(ctx, "allocating a subject", err);
	}
	*out = e;
	return 0;
}

// Put a (new) subject into a slot: uploads only.  The caller may release RS/SA
// as soon as this returns.
int esa_upload(andi_hip_ctx *ctx, andi_hip_esa *e, const char *RS, const int32_t *SA, size_t n,
					  size_t threshold, hipEvent_t done) {
	if (n > e->cap) {
		ctx->err = "subject does not fit its slot";
		return 1;
	}
	e->n = (int32_t)n;
	e->thr = (int32_t)threshold;
	e->deepK = std::min(pick_deep_k(n, ctx->queries_hint), e->deepK_cap);
	e->ref_built = e->index_built = false;
	e->rec_valid = false;
	// the flags are functions of the text and its suffix array: cleared here, only ever set by the builds
	hipError_t err = done ? hipSuccess : hipStreamSynchronize(ctx->stream); // (the slot is the caller's: nothing of it is in flight)
	memset(e->h_flags, 0, 4 * sizeof(int32_t));
	if (err == hipSuccess) err = hipMemsetAsync(e->S + n, 0, 1 + ANDI_PAD, ctx->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(e->S, RS, n, hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess && SA)
		err = hipMemcpyAsync(e->SA, SA, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = done ? hipEventRecord(done, ctx->stream) : hipStreamSynchronize(ctx->stream);
	if (err != hipSuccess) return fail(ctx, "uploading a subject", err);
	return 0;
}

// seq_subject_init (src/sequence.c:210-219) for a sequence that is already resident as a query: RS is written into the slot
// by a kernel from the query pool (esa_build.hip: k_rs_from_query) -- no host pass over the sequence, no upload.  The
// threshold is the caller's (min_anchor_length on the host, from the device's G+C count: queries_gc_counts).
int esa_from_query(andi_hip_ctx *ctx, andi_hip_esa *e, const andi_hip_queries *Q, size_t i, size_t threshold) {
	const size_t len = Q->len[i], n = 2 * len + 1;
	if (n > e->cap) {
		ctx->err = "subject does not fit its slot";
		return 1;
	}
	e->n = (int32_t)n;
	e->thr = (int32_t)threshold;
	e->deepK = std::min(pick_deep_k(n, ctx->queries_hint), e->deepK_cap);
	e->ref_built = e->index_built = false;
	e->rec_valid = false;
	memset(e->h_flags, 0, 4 * sizeof(int32_t)); // (the slot is the caller's: nothing of it is in flight)
	hipError_t err = hipMemsetAsync(e->S + (n & ~(size_t)3), 0, (n & 3) + 1 + ANDI_PAD, ctx->stream);
	if (err == hipSuccess) err = andi_launch_rs_from_query(e->S, Q->pool + Q->off[i], (uint32_t)len, ctx->stream);
	if (err != hipSuccess) return fail(ctx, "writing a subject from its resident sequence", err);
	return 0;
}

// calc_gc's numerators (src/sequence.c:197-208) of all staged sequences, counted where they lie
int queries_gc_counts(andi_hip_ctx *ctx, const andi_hip_queries *Q, std::vector<unsigned long long> &out) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	unsigned long long *d = nullptr;
	HIP_TRY(ctx, dmalloc(&d, Q->nq));
	uint32_t longest = 0;
	for (uint32_t l : Q->len) longest = std::max(longest, l);
	out.assign(Q->nq, 0);
	hipError_t err = hipMemsetAsync(d, 0, Q->nq * sizeof(unsigned long long), ctx->stream);
	if (err == hipSuccess) err = andi_launch_gc_counts(Q->pool, Q->d_off, Q->d_len, (uint32_t)Q->nq, longest, d, ctx->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(out.data(), d, Q->nq * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
	if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
	(void)andi_arena::dev_free(d);
	if (err != hipSuccess) return fail(ctx, "counting G+C of the staged sequences", err);
	return 0;
}

// esa_init_SA (src/esa.c:294-304) on the device: the text is in the slot, the suffix array is built there
int esa_sort_suffixes(andi_hip_ctx *ctx, andi_hip_esa *e) {
	const size_t need = andi_sa_device_workspace(e->n);
	if (ctx->sa_ws_bytes < need) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (ctx->sa_ws) (void)andi_arena::dev_free(ctx->sa_ws);
		ctx->sa_ws = nullptr, ctx->sa_ws_bytes = 0;
		HIP_TRY(ctx, andi_arena::dev_malloc(&ctx->sa_ws, need));
		ctx->sa_ws_bytes = need;
	}
	if (!ctx->sa_pinned && !(ctx->sa_pinned = (int32_t *)host_pool::word_get())) HIP_TRY(ctx, hipErrorOutOfMemory);
	if (!e->rec) {
		HIP_TRY(ctx, andi_arena::dev_malloc((void **)&e->rec, (e->cap + 8) * sizeof(uint32_t)));
		HIP_TRY(ctx, andi_arena::dev_malloc((void **)&e->rec2, (e->cap + 8) * sizeof(uint16_t)));
		e->bytes += (e->cap + 8) * (sizeof(uint32_t) + sizeof(uint16_t));
	}
	const auto t0 = std::chrono::steady_clock::now();
	int rounds = 0;
	hipError_t err = andi_sa_device(e->S, e->n, e->SA, ctx->sa_ws, ctx->sa_ws_bytes, ctx->sa_pinned, ctx->stream, &rounds, e->rec, e->deepK, e->rec2);
	e->rec_valid = err == hipSuccess && e->rec != nullptr;
	if (err == hipErrorInvalidSymbol) {
		ctx->err = "a subject holds a byte outside {A,C,G,T,!,;,#}";
		return 1;
	}
	if (err != hipSuccess) return fail(ctx, "building the suffix array", err);
	ctx->acc.sa_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	ctx->acc.sa_builds++;
	ctx->acc.sa_rounds += (uint64_t)rounds;
	return 0;
}

int andi_hip_esa_stage_text(andi_hip_ctx *ctx, const char *RS, size_t n, size_t threshold, andi_hip_esa **out) {
	if (!ctx || !RS || !out || n == 0 || n >= (size_t)INT32_MAX) {
		if (ctx) ctx->err = "andi_hip_esa_stage_text: bad arguments";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	andi_hip_esa *e = nullptr;
	if (esa_reserve(ctx, n, &e)) return 1;
	if (esa_upload(ctx, e, RS, nullptr, n, threshold) || esa_sort_suffixes(ctx, e)) {
		andi_hip_esa_free(ctx, e);
		return 1;
	}
	*out = e;
	return 0;
}

int andi_hip_esa_download_sa(andi_hip_ctx *ctx, const andi_hip_esa *e, int32_t *SA) {
	if (!ctx || !e || !SA) return 1;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	HIP_TRY(ctx, hipMemcpy(SA, e->SA, (size_t)e->n * sizeof(int32_t), hipMemcpyDeviceToHost));
	return 0;
}

int andi_hip_esa_stage(andi_hip_ctx *ctx, const char *RS, const int32_t *SA, size_t n,
					   size_t threshold, andi_hip_esa **out) {
	if (!ctx || !RS || !SA || !out || n == 0 || n >= (size_t)INT32_MAX) {
		if (ctx) ctx->err = "andi_hip_esa_stage: bad arguments";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	andi_hip_esa *e = nullptr;
	if (esa_reserve(ctx, n, &e)) return 1;
	if (esa_upload(ctx, e, RS, SA, n, threshold)) {
		andi_hip_esa_free(ctx, e);
		return 1;
	}
	*out = e;
	return 0;
}

static int ensure_reference_buffers(andi_hip_ctx *ctx, andi_hip_esa *e) {
	if (e->LCP && e->ref_cap >= (size_t)e->n) return 0;
	if (e->LCP) { // slot reused for a longer subject
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		(void)andi_arena::dev_free(e->LCP), (void)andi_arena::dev_free(e->CLD), (void)andi_arena::dev_free(e->FVC), (void)andi_arena::dev_free(e->tab);
		(void)andi_arena::dev_free(e->min_scratch);
		e->LCP = e->CLD = nullptr, e->FVC = nullptr, e->tab = nullptr, e->min_scratch = nullptr;
	}
	const size_t n = e->cap;
	e->ref_cap = n;
	const size_t tab_entries = (size_t)1 << (2 * ANDI_CACHE_K);
	const size_t mins = andi_min_tree_entries((int32_t)n);
	hipError_t err = hipSuccess;
	auto chk = [&](hipError_t x) {
		if (err == hipSuccess) err = x;
	};
	chk(dmalloc(&e->LCP, n + 1));
	chk(dmalloc(&e->CLD, n + 1));
	chk(dmalloc(&e->FVC, n + ANDI_PAD));
	chk(dmalloc(&e->tab, tab_entries));
	chk(dmalloc(&e->min_scratch, mins));
	if (err != hipSuccess) return fail(ctx, "allocating the reference arrays", err);
	e->bytes += 8 * (n + 1) + n + ANDI_PAD + 16 * tab_entries + 4 * mins;
	return 0;
}

int andi_hip_esa_build(andi_hip_ctx *ctx, andi_hip_esa *e) {
	if (!ctx || !e) return 1;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ensure_reference_buffers(ctx, e)) return 1;
	Timed t(ctx, 0);
	hipError_t err = andi_launch_esa_build(build_args(e), ctx->stream);
	t.stop();
	if (err == hipSuccess) err = hipEventRecord(ctx->built, ctx->stream);
	if (err != hipSuccess) return fail(ctx, "andi_hip_esa_build", err);
	e->ref_built = true, ctx->builds_pending = true;
	return 0;
}

int andi_hip_esa_build_index(andi_hip_ctx *ctx, andi_hip_esa *e) {
	if (!ctx || !e) return 1;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	Timed t(ctx, 0);
	const int ext = andi_index_single_ext(ctx->queries_hint, e->rec_valid);
	hipError_t err = andi_launch_index_build(build_args(e), ext, ctx->stream);
	t.stop();
	if (err == hipSuccess) err = hipEventRecord(ctx->built, ctx->stream);
	if (err != hipSuccess) return fail(ctx, "andi_hip_esa_build_index", err);
	e->index_built = true, e->deep_ext = (ext == 2 && !e->rec_valid) ? 0 : ext, ctx->builds_pending = true; // (the short form forced on a host-made suffix array: plain)
	return 0;
}

int andi_hip_esa_build_index_batch(andi_hip_ctx *ctx, andi_hip_esa *const *esas, size_t count) {
	if (!ctx || !esas || count == 0 || count > 65535) {
		if (ctx) ctx->err = "andi_hip_esa_build_index_batch: bad arguments";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->ib_cap < count) {
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (ctx->ib_dev) (void)andi_arena::dev_free(ctx->ib_dev);
		if (ctx->ib_host) host_pool::pinned_put(ctx->ib_host, ctx->ib_cap * sizeof(AndiIndexBatchItem));
		ctx->ib_dev = ctx->ib_host = nullptr, ctx->ib_cap = 0;
		const size_t cap = std::max<size_t>(count, 64);
		HIP_TRY(ctx, andi_arena::dev_malloc(&ctx->ib_dev, cap * sizeof(AndiIndexBatchItem)));
		HIP_TRY(ctx, host_pool::pinned_get(&ctx->ib_host, cap * sizeof(AndiIndexBatchItem)));
		if (!ctx->ib_done) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ib_done, hipEventDisableTiming));
		ctx->ib_cap = cap;
	} else {
		HIP_TRY(ctx, hipEventSynchronize(ctx->ib_done)); // the previous batch's items have been copied
	}
	auto *items = (AndiIndexBatchItem *)ctx->ib_host;
	int32_t max_n = 0, max_n_shallow = 0; // (shallow: a table of K < ANDI_CLOSED_RUN_K, andi_launch_index_build_batch)
	for (size_t k = 0; k < count; ++k) {
		andi_hip_esa *e = esas[k];
		if (!e) {
			ctx->err = "andi_hip_esa_build_index_batch: null subject";
			return 1;
		}
		items[k].S = e->S, items[k].SA = e->SA, items[k].deep = e->deep, items[k].N0 = e->N0, items[k].N1 = e->N1, items[k].P = e->P;
		items[k].flags = e->flags, items[k].n = e->n, items[k].deepK = e->deepK;
		items[k].rec = e->rec_valid ? e->rec : nullptr;
		items[k].rec2 = e->rec_valid ? e->rec2 : nullptr;
		items[k].single_ext = andi_index_single_ext(ctx->queries_hint, e->rec_valid);
		max_n = std::max(max_n, e->n);
		if (e->deepK < ANDI_CLOSED_RUN_K) max_n_shallow = std::max(max_n_shallow, e->n);
	}
	Timed t(ctx, 0);
	hipError_t err = hipMemcpyAsync(ctx->ib_dev, ctx->ib_host, count * sizeof(AndiIndexBatchItem), hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = hipEventRecord(ctx->ib_done, ctx->stream);
	if (err == hipSuccess) err = andi_launch_index_build_batch((const AndiIndexBatchItem *)ctx->ib_dev, (uint32_t)count, max_n, max_n_shallow, ctx->stream);
	t.stop();
	if (err == hipSuccess) err = hipEventRecord(ctx->built, ctx->stream);
	if (err != hipSuccess) return fail(ctx, "andi_hip_esa_build_index_batch", err);
	for (size_t k = 0; k < count; ++k) {
		const int ext = items[k].single_ext;
		esas[k]->index_built = true, esas[k]->deep_ext = (ext == 2 && !esas[k]->rec_valid) ? 0 : ext;
	}
	ctx->builds_pending = true;
	return 0;
}

int andi_hip_esa_flags(andi_hip_ctx *ctx, const andi_hip_esa *e, int32_t *out4) {
	if (!ctx || !e || !out4) return 1;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	memcpy(out4, e->h_flags, 4 * sizeof(int32_t));
	return 0;
}

int andi_hip_esa_download(andi_hip_ctx *ctx, const andi_hip_esa *e, int32_t *LCP, int32_t *CLD,
						  uint8_t *FVC, andi_hip_interval *cache) {
	if (!ctx || !e) return 1;
	if (!e->ref_built) {
		ctx->err = "andi_hip_esa_download: reference arrays not built (call andi_hip_esa_build)";
		return 1;
	}
	const size_t n = (size_t)e->n;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (LCP) HIP_TRY(ctx, hipMemcpy(LCP, e->LCP, (n + 1) * 4, hipMemcpyDeviceToHost));
	if (CLD) HIP_TRY(ctx, hipMemcpy(CLD, e->CLD, (n + 1) * 4, hipMemcpyDeviceToHost));
	if (FVC) HIP_TRY(ctx, hipMemcpy(FVC, e->FVC, n, hipMemcpyDeviceToHost));
	if (cache)
		HIP_TRY(ctx, hipMemcpy(cache, e->tab, ((size_t)16 << (2 * ANDI_CACHE_K)), hipMemcpyDeviceToHost));
	return 0;
}

int andi_hip_esa_download_index(andi_hip_ctx *ctx, const andi_hip_esa *e, uint32_t *table, int *K) {
	if (!ctx || !e) return 1;
	if (!e->index_built) {
		ctx->err = "andi_hip_esa_download_index: scan index not built (call andi_hip_esa_build_index)";
		return 1;
	}
	if (K) *K = e->deepK;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (table) HIP_TRY(ctx, hipMemcpy(table, e->deep, (size_t)8 << (2 * e->deepK), hipMemcpyDeviceToHost));
	return 0;
}

#ifdef ANDI_TEST_HOOKS
// Test hooks (the suite's library only; not part of include/andi_hip.h).
// The packed text of a subject as it lies on the device: the first nib_bytes of N0 and of N1, and p_words words of the
// bit-sliced text from the block of padding in front of P on (P itself starts at word 3).  Any pointer may be NULL.
extern "C" int andi_hip_test_download_text(andi_hip_ctx *ctx, const andi_hip_esa *e, uint8_t *N0, uint8_t *N1, size_t nib_bytes, uint32_t *P,
										   size_t p_words) {
	if (!ctx || !e) return 1;
	if (nib_bytes > e->cap / 2 + 1 + ANDI_NIB_BACK || p_words > 3 * ((e->cap + 1 + 4096) / 32 + 4)) {
		ctx->err = "andi_hip_test_download_text: more than the buffers hold";
		return 1;
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (N0) HIP_TRY(ctx, hipMemcpy(N0, e->N0, nib_bytes, hipMemcpyDeviceToHost));
	if (N1) HIP_TRY(ctx, hipMemcpy(N1, e->N1, nib_bytes, hipMemcpyDeviceToHost));
	if (P) HIP_TRY(ctx, hipMemcpy(P, e->Praw, p_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}
// The list of the wavefront kernel's segments of the context's last routed scan call (scan.h: coop_items), as it lies in the call's scratch:
// up to items_cap entries, and the class and cost-class bytes of up to pairs_cap pairs as they stand after the call.  info = { entries of the
// list, pairs of the call, segments per subject of the wavefront kernel's layout, 1 if the call had a list }.  Any pointer may be NULL.
extern "C" int andi_hip_test_coop_items(andi_hip_ctx *ctx, uint32_t *items, size_t items_cap, uint8_t *pair_class, uint8_t *pair_cost, size_t pairs_cap,
										uint32_t *info) {
	if (!ctx) return 1;
	const auto &l = ctx->last_items;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (info) info[0] = l.n_items, info[1] = l.pairs, info[2] = l.total_segs, info[3] = l.items ? 1u : 0u;
	const size_t ni = std::min<size_t>(items_cap, l.n_items), np = std::min<size_t>(pairs_cap, l.pairs);
	if (items && l.items && ni) HIP_TRY(ctx, hipMemcpy(items, l.items, ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (pair_class && l.pair_class && np) HIP_TRY(ctx, hipMemcpy(pair_class, l.pair_class, np, hipMemcpyDeviceToHost));
	if (pair_cost && l.pair_cost && np) HIP_TRY(ctx, hipMemcpy(pair_cost, l.pair_cost, np, hipMemcpyDeviceToHost));
	return 0;
}
// What the context's last routed scan call enqueued around pass A (scan_call.hip: launch_routed), per layout -- 0 the lane scan's, 1 the
// wavefront kernel's, 2 the pairs handed back: out[k] = 1 if layout k's pass A was enqueued, out[3 + k] = its rounds of stitching again (both set where the launches are made);
// out[6] = 1 if the call went ahead of the pending index builds (scan_call.hip: upload_descriptors), out[7] = 1 if a raised flag made it run again.
// count_b (may be NULL): the 16 words of the wavefront kernel's restitch_count as pass B left them (scan.h: [0 .. 2] stretches stitched again
// per round, [3] true chains that left their segment on their own, [8] the first stage's list).  All zero where the last call was not routed.
extern "C" int andi_hip_test_call_edges(andi_hip_ctx *ctx, uint32_t *out, uint32_t *count_b) {
	if (!ctx || !out) return 1;
	const auto &l = ctx->last_edges;
	for (int k = 0; k < 3; ++k) out[k] = l.pass_a[k], out[3 + k] = l.rounds[k];
	out[6] = l.went_ahead, out[7] = l.ran_again;
	if (!count_b) return 0;
	for (int k = 0; k < 16; ++k) count_b[k] = 0;
	if (!l.count_b) return 0;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	HIP_TRY(ctx, hipMemcpy(count_b, l.count_b, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}
// The lane layout of the context's last routed scan call as it lies in the call's scratch after the call (scan.h): pair_waves (pairs words),
// pair_wave0 (pairs + 1 words; only where the lanes' segment lengths are per pair), sub_order (nsub words) and the layout's sixteen counters
// as the host's first look saw them.  info = { pairs, subjects, 1 if pair_wave0 is there, 1 if the host looked }.  Any pointer may be NULL.
extern "C" int andi_hip_test_pair_layout(andi_hip_ctx *ctx, uint32_t *pair_waves, uint32_t *pair_wave0, uint32_t *sub_order, uint32_t *counts, uint32_t *info) {
	if (!ctx) return 1;
	const auto &l = ctx->last_items;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (info) info[0] = l.pairs, info[1] = l.nsub, info[2] = l.pair_wave0 ? 1u : 0u, info[3] = l.looked;
	if (pair_waves && l.pair_waves && l.pairs) HIP_TRY(ctx, hipMemcpy(pair_waves, l.pair_waves, l.pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (pair_wave0 && l.pair_wave0 && l.pairs) HIP_TRY(ctx, hipMemcpy(pair_wave0, l.pair_wave0, ((size_t)l.pairs + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (sub_order && l.sub_order && l.nsub) HIP_TRY(ctx, hipMemcpy(sub_order, l.sub_order, l.nsub * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (counts)
		for (int k = 0; k < 16; ++k) counts[k] = l.counts[k];
	return 0;
}
// The per-slot records of the context's last scan call that used ONE segment length (not routed, no per-pair lengths), as they lie in lane
// layout a of the call's scratch after the call: pass A's cold_exit, cold_counts and marks, pass B's used_entry, true_exit and owned (pass C
// only reads them: after the call they are pass B's result), `slots` slots of each at most, and the 16 words of restitch_count.
// info = { subjects, segments per subject, segment length, 1 if such a call is on record }.  The slot of segment k of query q under subject s
// is s * total_segs + qseg_start[q] + k, qseg_start the running sum of ceil(qlen / seg) over the queries; the slots of a subject's own query
// are not written.  Any pointer may be NULL; with arrays asked for and no call on record it is an error (nothing stale is handed out).
extern "C" int andi_hip_test_stitch_slots(andi_hip_ctx *ctx, ChainState *cold_exit, ChainState *true_exit, ChainState *used_entry, uint32_t *cold_counts,
										  uint32_t *owned, ColdMark *marks, size_t slots, uint32_t *restitch_count, uint32_t *info) {
	if (!ctx) return 1;
	const auto &l = ctx->last_slots;
	const bool have = l.cold_exit != nullptr;
	if (info) info[0] = l.nsub, info[1] = l.total_segs, info[2] = l.seg, info[3] = have ? 1u : 0u;
	const bool wants = cold_exit || true_exit || used_entry || cold_counts || owned || marks || restitch_count;
	if (!wants) return 0;
	if (!have || slots > (size_t)l.nsub * l.total_segs) {
		ctx->err = have ? "andi_hip_test_stitch_slots: more slots than the call had" : "andi_hip_test_stitch_slots: no scan call with one segment length on record";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (cold_exit && slots) HIP_TRY(ctx, hipMemcpy(cold_exit, l.cold_exit, slots * sizeof(ChainState), hipMemcpyDeviceToHost));
	if (true_exit && slots) HIP_TRY(ctx, hipMemcpy(true_exit, l.true_exit, slots * sizeof(ChainState), hipMemcpyDeviceToHost));
	if (used_entry && slots) HIP_TRY(ctx, hipMemcpy(used_entry, l.used_entry, slots * sizeof(ChainState), hipMemcpyDeviceToHost));
	if (cold_counts && slots) HIP_TRY(ctx, hipMemcpy(cold_counts, l.cold_counts, slots * 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (owned && slots) HIP_TRY(ctx, hipMemcpy(owned, l.owned, slots * 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (marks && slots) HIP_TRY(ctx, hipMemcpy(marks, l.marks, slots * ANDI_COLD_MARKS * sizeof(ColdMark), hipMemcpyDeviceToHost));
	if (restitch_count) HIP_TRY(ctx, hipMemcpy(restitch_count, l.restitch_count, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}
// The index build's pack kernel alone on a staged subject (no table: the text may be any bytes); forms: bit 0 with N1, bit 1 with P
extern "C" int andi_hip_test_pack_text(andi_hip_ctx *ctx, andi_hip_esa *e, int forms) {
	if (!ctx || !e) return 1;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, andi_launch_pack_text(e->S, (size_t)e->n + 1 + 64, e->N0, (forms & 1) ? e->N1 : nullptr, (forms & 2) ? e->P : nullptr, e->flags + 1,
									   ctx->stream));
	return 0;
}
// The staged 2-bit codes (andi_hip_queries.codes) of query qidx of a staged set or a view of one: `words` words from the query's first block on
extern "C" int andi_hip_test_query_codes(andi_hip_ctx *ctx, const andi_hip_queries *q, size_t qidx, uint32_t *out, size_t words) {
	if (!ctx || !q || !out || qidx >= q->nq || !q->codes || words > 2 * (((size_t)q->len[qidx] + 1 + 255) / 256 * 8)) {
		if (ctx) ctx->err = "andi_hip_test_query_codes: bad arguments, or more than the query's blocks hold";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (words) HIP_TRY(ctx, hipMemcpy(out, q->codes + 2 * (q->off[qidx] / 32), words * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}
// The layout kernels of a routed scan call (scan_lane.hip) ALONE, on arrays of the caller's: no subject, no query text, no k_pair_estimate.
// par = { nsub, nq, restitch_count[ANDI_STRUCT_WAVES], seg0, max_class, route_seg, route_all_few, adaptive, items_order, 1: with sub_order,
// 1: with a list, allow_small (andi_launch_pair_routing) }; qlen[nq], self[nsub]; pair_class, pair_waves, pair_cost (with a list) of all
// nsub * nq pairs and sub_cost[nsub] (with sub_order) as k_pair_estimate would leave them; left (may be NULL): a byte per pair, nonzero for
// the pairs that get ANDI_ROUTE_LEFT behind the routing -- as pass A by wavefronts hands pairs back.  The wavefront layout's segmentation
// (qseg_start, total_segs) is made from qlen and route_seg as the queries' cached one is (scan_call.hip: ensure_segmentation).
// Launched as launch_routed does (scan_call.hip): the routing, the list (layout_count: the lane layout's counters), a download -- stage 1:
// class1, waves1, wave01 (pairs + 1 words, adaptive only), order (with sub_order), counts1[16], quad (k_lane_quad's list, counts1[ANDI_QUAD_WAVES]
// words of it), items (counts1[ANDI_COOP_SEGS] entries) --; then, with `left`, those marks and andi_launch_pair_leftover on a second layout
// with its own pair_waves, pair_wave0, pair_bsum, counters and list; andi_launch_route_count; a download -- stage 2: class2, and with `left`
// waves2, wave02 (adaptive only) and the second layout's counts2[16]; route_nt[3].  info = { 1: the routing was k_pair_layout_small's one
// block, 2: several kernels; launches of the list's sort (0: no list, 1, 3); total_segs; words the quad list was allocated }.  Any output may
// be NULL.  Bad arguments: returns 1 with nothing launched.
extern "C" int andi_hip_test_layout_kernels(andi_hip_ctx *ctx, const uint32_t *par, const uint32_t *qlen, const int64_t *self, const uint8_t *pair_class,
											const uint32_t *pair_waves, const uint8_t *pair_cost, const float *sub_cost, const uint8_t *left,
											uint8_t *class1, uint32_t *waves1, uint32_t *wave01, uint32_t *order, uint32_t *counts1, uint32_t *quad,
											uint32_t *items, uint8_t *class2, uint32_t *waves2, uint32_t *wave02, uint32_t *counts2,
											unsigned long long *route_nt, uint32_t *info) {
	if (!ctx) return 1;
	if (!par || !qlen || !self || !pair_class || !pair_waves) {
		ctx->err = "andi_hip_test_layout_kernels: par, qlen, self, pair_class and pair_waves are required";
		return 1;
	}
	const uint32_t nsub = par[0], nq = par[1], strct = par[2], seg0 = par[3], max_class = par[4], route_seg = par[5];
	const uint32_t all_few = par[6], adaptive = par[7], items_order = par[8];
	const bool with_order = par[9] != 0, with_list = par[10] != 0, allow_small = par[11] != 0;
	const uint64_t P64 = (uint64_t)nsub * nq;
	const size_t LIMIT = (size_t)1 << 27; // (words of any one array: a hook of the suite's, not a call of gigabytes)
	if (!nsub || !nq || P64 > UINT32_MAX || P64 > LIMIT) {
		ctx->err = "andi_hip_test_layout_kernels: no pairs, or nsub * nq beyond what the kernels' 32-bit pair index (and this hook) takes";
		return 1;
	}
	if (!seg0 || seg0 > (1u << 28) || max_class > 3 || !route_seg || adaptive > 1 || all_few > 1) {
		ctx->err = "andi_hip_test_layout_kernels: seg0 in 1 .. 2^28, max_class <= 3, route_seg >= 1, adaptive and route_all_few 0 or 1";
		return 1;
	}
	if ((with_order && !sub_cost) || (with_list && !pair_cost) || (with_list && items_order != ANDI_ITEMS_HEAVY && items_order != ANDI_ITEMS_LIGHT)) {
		ctx->err = "andi_hip_test_layout_kernels: sub_order needs sub_cost, a list needs pair_cost and an order of ANDI_ITEMS_HEAVY or ANDI_ITEMS_LIGHT";
		return 1;
	}
	const size_t P = (size_t)P64;
	// the wavefront layout's segmentation, and what the lists can hold at the most: every pair's wavefronts as given, and at the
	// shortest segment length (a bumped or handed-back pair's are counted anew from its class)
	std::vector<uint32_t> start(nq + 1);
	uint64_t total = 0, waves_q = 0, waves_in = 0;
	for (size_t i = 0; i < nq; ++i) {
		start[i] = (uint32_t)total;
		total += (qlen[i] + (uint64_t)route_seg - 1) / route_seg;
		waves_q += ((qlen[i] + (uint64_t)seg0 - 1) / seg0 + 63) / 64;
		if (total >= UINT32_MAX) break;
	}
	start[nq] = (uint32_t)total;
	for (size_t i = 0; i < P; ++i) waves_in += pair_waves[i];
	const uint64_t quad_cap = waves_in + waves_q * nsub; // (a pair keeps the wavefronts it came with or gets at most those of class 0)
	if (total >= UINT32_MAX || total * nsub > UINT32_MAX || (with_list && total * nsub > LIMIT) || quad_cap > LIMIT) {
		ctx->err = "andi_hip_test_layout_kernels: more segments or wavefronts than 32 bits (and this hook) take";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const hipStream_t st = ctx->stream;
	DevScope dev(st);
	uint32_t *d_qlen = nullptr, *d_start = nullptr, *d_waves = nullptr, *d_wave0 = nullptr, *d_bsum = nullptr, *d_count = nullptr, *d_order = nullptr;
	uint32_t *d_hist = nullptr, *d_items = nullptr, *d_waves2 = nullptr, *d_wave02 = nullptr, *d_bsum2 = nullptr, *d_count2 = nullptr;
	unsigned long long *d_quad = nullptr, *d_quad2 = nullptr, *d_nt = nullptr; // (a list of words in pass B's list of 64-bit entries: scan.h)
	int64_t *d_self = nullptr;
	uint8_t *d_class = nullptr, *d_cost = nullptr;
	float *d_subcost = nullptr;
	const size_t nblocks = (P + 1023) / 1024, n_items = (size_t)(total * nsub), quad_words = (size_t)quad_cap;
	dev.alloc(&d_qlen, nq), dev.alloc(&d_start, (size_t)nq + 1), dev.alloc(&d_self, nsub), dev.alloc(&d_class, P), dev.alloc(&d_waves, P);
	dev.alloc(&d_count, 16), dev.alloc(&d_nt, 3);
	if (adaptive) dev.alloc(&d_wave0, P + 1), dev.alloc(&d_bsum, P / 1024 + 2), dev.alloc(&d_quad, quad_words / 2 + 1);
	if (with_order) dev.alloc(&d_subcost, nsub), dev.alloc(&d_order, nsub);
	if (with_list) dev.alloc(&d_cost, P), dev.alloc(&d_hist, ANDI_COST_CLASSES * nblocks), dev.alloc(&d_items, n_items + 1);
	if (left) {
		dev.alloc(&d_waves2, P), dev.alloc(&d_count2, 16);
		if (adaptive) dev.alloc(&d_wave02, P + 1), dev.alloc(&d_bsum2, P / 1024 + 2), dev.alloc(&d_quad2, quad_words / 2 + 1);
	}
	HIP_TRY(ctx, dev.err);
	uint32_t h_count[16] = {};
	h_count[ANDI_STRUCT_WAVES] = strct;
	HIP_TRY(ctx, hipMemcpyAsync(d_qlen, qlen, nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_start, start.data(), ((size_t)nq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_self, self, nsub * sizeof(int64_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_class, pair_class, P, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_waves, pair_waves, P * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(d_count, h_count, sizeof h_count, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemsetAsync(d_nt, 0, 3 * sizeof(unsigned long long), st));
	if (with_order) HIP_TRY(ctx, hipMemcpyAsync(d_subcost, sub_cost, nsub * sizeof(float), hipMemcpyHostToDevice, st));
	if (with_list) HIP_TRY(ctx, hipMemcpyAsync(d_cost, pair_cost, P, hipMemcpyHostToDevice, st));
	if (left) HIP_TRY(ctx, hipMemsetAsync(d_count2, 0, 16 * sizeof(uint32_t), st));
	HIP_TRY(ctx, hipStreamSynchronize(st)); // (h_count and start are this frame's)
	ScanArgs a{};
	a.self = d_self, a.nsub = nsub, a.qlen = d_qlen, a.nq = nq;
	a.qseg_start = d_start, a.total_segs = (uint32_t)total, a.seg = route_seg;
	a.restitch_count = d_count, a.defer_count = d_count + 8, a.defer_list = d_quad;
	a.adaptive = (int)adaptive, a.seg0 = seg0, a.max_class = max_class;
	a.pair_class = d_class, a.pair_waves = d_waves, a.pair_wave0 = d_wave0, a.pair_bsum = d_bsum;
	a.pair_cost = d_cost, a.item_hist = d_hist, a.items_order = ANDI_ITEMS_GRID;
	a.sub_cost = d_subcost, a.sub_order = d_order;
	a.route = ANDI_LAYOUT_LANES, a.route_seg = route_seg, a.route_all_few = all_few, a.route_nt = d_nt;
	ScanArgs b = a; // the wavefront kernel's layout (launch_routed)
	b.adaptive = 0, b.coop = 1, b.route = ANDI_LAYOUT_COOP;
	b.coop_items = d_items, b.items_order = with_list ? items_order : (uint32_t)ANDI_ITEMS_GRID, b.layout_count = d_count;
	const bool small = P <= 1024 && allow_small;
	if (info) info[0] = small ? 1u : 2u, info[1] = with_list ? (nblocks == 1 ? 1u : 3u) : 0u, info[2] = (uint32_t)total, info[3] = (uint32_t)quad_words;
	HIP_TRY(ctx, andi_launch_pair_routing(a, st, allow_small));
	if (with_list) HIP_TRY(ctx, andi_launch_coop_items(b, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	std::vector<uint8_t> cls(P);
	HIP_TRY(ctx, hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
	HIP_TRY(ctx, hipMemcpy(cls.data(), d_class, P, hipMemcpyDeviceToHost));
	if (h_count[ANDI_QUAD_WAVES] > quad_words || h_count[ANDI_COOP_SEGS] > n_items) {
		ctx->err = "andi_hip_test_layout_kernels: a list's counter is beyond what the list holds";
		return 1;
	}
	if (counts1) memcpy(counts1, h_count, sizeof h_count);
	if (class1) memcpy(class1, cls.data(), P);
	if (waves1) HIP_TRY(ctx, hipMemcpy(waves1, d_waves, P * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (wave01 && adaptive) HIP_TRY(ctx, hipMemcpy(wave01, d_wave0, (P + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (order && with_order) HIP_TRY(ctx, hipMemcpy(order, d_order, nsub * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (quad && adaptive && h_count[ANDI_QUAD_WAVES]) HIP_TRY(ctx, hipMemcpy(quad, d_quad, h_count[ANDI_QUAD_WAVES] * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (items && with_list && h_count[ANDI_COOP_SEGS]) HIP_TRY(ctx, hipMemcpy(items, d_items, h_count[ANDI_COOP_SEGS] * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (left) {
		for (size_t i = 0; i < P; ++i)
			if (left[i]) cls[i] |= ANDI_ROUTE_LEFT;
		HIP_TRY(ctx, hipMemcpyAsync(d_class, cls.data(), P, hipMemcpyHostToDevice, st));
		ScanArgs a2 = a; // the pairs handed back: a lane layout of their own
		a2.route = ANDI_LAYOUT_LANES2;
		a2.pair_waves = d_waves2, a2.pair_wave0 = d_wave02, a2.pair_bsum = d_bsum2;
		a2.restitch_count = d_count2, a2.defer_count = d_count2 + 8, a2.defer_list = d_quad2;
		HIP_TRY(ctx, andi_launch_pair_leftover(a2, st));
	}
	HIP_TRY(ctx, andi_launch_route_count(a, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (class2) HIP_TRY(ctx, hipMemcpy(class2, d_class, P, hipMemcpyDeviceToHost));
	if (waves2 && left) HIP_TRY(ctx, hipMemcpy(waves2, d_waves2, P * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (wave02 && left && adaptive) HIP_TRY(ctx, hipMemcpy(wave02, d_wave02, (P + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (counts2 && left) HIP_TRY(ctx, hipMemcpy(counts2, d_count2, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (route_nt) HIP_TRY(ctx, hipMemcpy(route_nt, d_nt, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return 0;
}
#endif

int andi_hip_esa_single_form(const andi_hip_esa *e) { return e && e->index_built ? e->deep_ext : 0; }

void andi_hip_esa_free(andi_hip_ctx *ctx, andi_hip_esa *e) {
	if (!e) return;
	if (ctx) (void)hipSetDevice(ctx->device);
	(void)hipDeviceSynchronize(); // once for the handle's ten buffers: nothing in flight uses them when they are handed out again
	void *bufs[] = {e->S, e->SA, e->LCP, e->CLD, e->FVC, e->tab, e->deep, e->Nraw, e->Praw, e->rec, e->rec2, e->min_scratch};
	for (void *b : bufs) (void)andi_arena::dev_free(b, false);
	host_pool::word_put(e->h_flags);
	delete e;
}

size_t andi_hip_esa_bytes(const andi_hip_esa *e) {
	return e ? e->bytes : 0;
}

// ------------------------------------------------------------------ queries
// the contig separators of every staged sequence (d_off, d_len and the byte pool are queued on the stream): one pass over the pool
static hipError_t queries_count_separators(andi_hip_ctx *ctx, andi_hip_queries *q) {
	hipError_t err = dmalloc(&q->d_sep, q->nq);
	if (err != hipSuccess) return err;
	uint32_t longest = 0;
	for (uint32_t l : q->len) longest = std::max(longest, l);
	err = hipMemsetAsync(q->d_sep, 0, q->nq * sizeof(uint32_t), ctx->stream);
	if (err == hipSuccess) err = andi_launch_sep_counts(q->pool, q->d_off, q->d_len, (uint32_t)q->nq, longest, q->d_sep, ctx->stream);
	return err;
}

int andi_hip_queries_stage(andi_hip_ctx *ctx, const andi_hip_seq *seqs, size_t n,
						   andi_hip_queries **out) {
	if (!ctx || !seqs || !out || n == 0 || n >= (size_t)UINT32_MAX) {
		if (ctx) ctx->err = "andi_hip_queries_stage: bad arguments";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	auto *q = new andi_hip_queries;
	q->nq = n;
	q->off.resize(n);
	q->len.resize(n);
	uint64_t cursor = 0;
	for (size_t i = 0; i < n; ++i) {
		if (!seqs[i].seq || seqs[i].len == 0 || seqs[i].len > (size_t)(INT32_MAX - 1) / 2) {
			ctx->err = "andi_hip_queries_stage: empty or oversized sequence";
			delete q;
			return 1;
		}
		q->off[i] = cursor;
		q->len[i] = (uint32_t)seqs[i].len;
		q->total_nt += seqs[i].len;
		cursor += (seqs[i].len + 1 + 255) & ~(uint64_t)255; // NUL; starts on 256-byte boundaries (128 of the packed pool: a cache line)
	}
	const size_t pool_bytes = cursor + ANDI_PAD;
	hipError_t err = hipSuccess;
	auto chk = [&](hipError_t x) {
		if (err == hipSuccess) err = x;
	};
	chk(dmalloc(&q->pool, pool_bytes));
	chk(dmalloc(&q->nib, pool_bytes / 2 + 64));
	chk(dmalloc(&q->planes, 3 * (pool_bytes / 32) + 16));
	chk(dmalloc(&q->codes, 2 * (pool_bytes / 32) + 16));
	if (!(q->h_foreign = (int32_t *)host_pool::word_get())) chk(hipErrorOutOfMemory);
	int32_t *d_foreign = nullptr;
	chk(dmalloc(&d_foreign, 1));
	chk(dmalloc(&q->d_off, n));
	chk(dmalloc(&q->d_len, n));
	if (err == hipSuccess) err = hipMemsetAsync(q->pool, 0, pool_bytes, ctx->stream);
	uint64_t threaded_from = (uint64_t)1 << 31;
	if (const char *um = andi_knob(KNOB_UPLOAD_MIN_MB)) // (tests: the threaded path on small sets)
		if (atoi(um) >= 0) threaded_from = (uint64_t)atoi(um) << 20;
	if (err == hipSuccess && q->total_nt >= threaded_from) {
		// Gigabytes of sequences in pageable memory (BASELINE's config 3: 6.5 GB): one hipMemcpyAsync per sequence went through the
		// runtime's staging at 10-13 GB/s (0.5-0.6 of the 10.5 s of the 3085 x 3085 matrix, before anything else can begin: now 0.35 s).  Four
		// host threads instead, each copying its share chunk by chunk into one of its two pinned buffers while the other's
		// transfer runs on a stream of its own.
		err = hipStreamSynchronize(ctx->stream); // (the pool's zeroes first: the copies run on other streams)
		constexpr size_t CHUNK = (size_t)8 << 20;
		const int nt = 4;
		std::atomic<size_t> next_seq{0};
		std::atomic<int> bad{0};
		auto work = [&]() {
			(void)hipSetDevice(ctx->device);
			hipStream_t st = nullptr;
			void *pin = nullptr;
			hipEvent_t ev[2] = {nullptr, nullptr};
			bool ok = host_pool::stream_get(&st, ctx->device, 0) == hipSuccess && host_pool::pinned_get(&pin, 2 * CHUNK) == hipSuccess &&
					  hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
			size_t k = 0; // chunks this thread has sent
			while (ok && !bad.load()) {
				const size_t i = next_seq.fetch_add(1);
				if (i >= n) break;
				for (size_t o = 0; o < seqs[i].len && ok; o += CHUNK, ++k) {
					const size_t len = std::min(CHUNK, seqs[i].len - o);
					char *buf = (char *)pin + (k & 1) * CHUNK;
					if (k >= 2) ok = hipEventSynchronize(ev[k & 1]) == hipSuccess; // (the transfer that last read this buffer)
					memcpy(buf, seqs[i].seq + o, len);
					ok = ok && hipMemcpyAsync(q->pool + q->off[i] + o, buf, len, hipMemcpyHostToDevice, st) == hipSuccess && hipEventRecord(ev[k & 1], st) == hipSuccess;
				}
			}
			if (st) ok = hipStreamSynchronize(st) == hipSuccess && ok;
			if (!ok) bad.store(1);
			for (hipEvent_t e : ev)
				if (e) (void)hipEventDestroy(e);
			if (pin) host_pool::pinned_put(pin, 2 * CHUNK);
			if (st) host_pool::stream_put(st, ctx->device, 0);
		};
		std::vector<std::thread> ts;
		for (int t = 1; t < nt; ++t) ts.emplace_back(work);
		work();
		for (auto &t : ts) t.join();
		if (bad.load() && err == hipSuccess) err = hipErrorUnknown;
	} else {
		for (size_t i = 0; i < n && err == hipSuccess; ++i)
			err = hipMemcpyAsync(q->pool + q->off[i], seqs[i].seq, seqs[i].len, hipMemcpyHostToDevice,
								 ctx->stream);
	}
	if (err == hipSuccess)
		err = hipMemcpyAsync(q->d_off, q->off.data(), n * 8, hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess)
		err = hipMemcpyAsync(q->d_len, q->len.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
	// 4-bit symbols of the whole pool (pool_bytes is a multiple of 16)
	if (err == hipSuccess) err = hipMemsetAsync(d_foreign, 0, sizeof(int32_t), ctx->stream);
	if (err == hipSuccess)
		err = andi_launch_pack_symbols(q->pool, pool_bytes, q->nib, nullptr, d_foreign, ctx->stream);
	if (err == hipSuccess) err = andi_launch_pack_planes(q->nib, pool_bytes, q->planes, q->codes, ctx->stream);
	if (err == hipSuccess) err = queries_count_separators(ctx, q);
	if (err == hipSuccess)
		err = hipMemcpyAsync(q->h_foreign, d_foreign, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
	if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
	(void)andi_arena::dev_free(d_foreign);
	if (err != hipSuccess) {
		andi_hip_queries_free(ctx, q);
		return fail(ctx, "andi_hip_queries_stage", err);
	}

	*out = q;
	return 0;
}

void andi_hip_queries_free(andi_hip_ctx *ctx, andi_hip_queries *q) {
	if (!q) return;
	if (ctx) (void)hipSetDevice(ctx->device);
	(void)hipDeviceSynchronize();
	void *own[] = {q->d_qseg_start, q->d_seg2query, q->c_qseg_start, q->c_seg2query}; // (every set's, a view's too)
	for (void *b : own) (void)andi_arena::dev_free(b, false);
	if (q->owns_pool) {
		void *bufs[] = {q->pool, q->nib, q->planes, q->codes, q->d_off, q->d_len, q->d_sep};
		for (void *b : bufs) (void)andi_arena::dev_free(b, false);
		host_pool::word_put(q->h_foreign);
	}
	delete q;
}

// Queries [first, first + count) of a staged set, on the parent's device buffers: the scan reaches a query's symbols only
// through qoff[] (scan_dev.h), so a view's offsets are the parent's own, and the pool stays where it is.  Nothing is
// copied or uploaded; the view cuts its own segments (ensure_segmentation) when a scan first asks for them.
int andi_hip_queries_view(andi_hip_ctx *ctx, const andi_hip_queries *q, size_t first, size_t count, andi_hip_queries **out) {
	if (!ctx || !q || !out || count == 0 || first > q->nq || count > q->nq - first) {
		if (ctx) ctx->err = "andi_hip_queries_view: bad arguments";
		return 1;
	}
	auto *v = new andi_hip_queries;
	v->owns_pool = false;
	v->pool = q->pool, v->nib = q->nib, v->planes = q->planes, v->codes = q->codes, v->h_foreign = q->h_foreign;
	v->d_off = q->d_off + first, v->d_len = q->d_len + first, v->d_sep = q->d_sep ? q->d_sep + first : nullptr;
	v->off.assign(q->off.begin() + first, q->off.begin() + first + count);
	v->len.assign(q->len.begin() + first, q->len.begin() + first + count);
	v->nq = count;
	for (uint32_t l : v->len) v->total_nt += l;
	*out = v;
	return 0;
}

// 4-bit symbols of a byte string, as the device's pack kernel makes them (scan_lane.hip: symbol_of, in_alphabet): byte j of
// `out` = symbol 2j | symbol 2j+1 << 4, the NUL behind an odd length included; (len + 1) / 2 bytes.  Eight bytes at a time
// where they are all nucleotides (what genomes are made of); returns 1 if a byte lies outside {A,C,G,T,!,;,#,NUL}.
extern "C" int andi_hip_pack_symbols(const unsigned char *src, size_t len, unsigned char *out) {
	static const struct Lut {
		uint8_t v[256];
		Lut() {
			for (int c = 0; c < 256; ++c) {
				const uint8_t ch = (uint8_t)c;
				const uint32_t sym = ch >= 'A' ? (uint32_t)(((ch & 6u) ^ ((ch & 6u) >> 1)) >> 1) : (ch == '!' ? 4u : ch == ';' ? 5u : ch == '#' ? 6u : 7u);
				const bool in = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == '!' || ch == ';' || ch == '#' || ch == 0;
				v[c] = (uint8_t)(sym | (in ? 0u : 0x80u));
			}
		}
	} lut;
	uint32_t bad = 0;
	size_t k = 0;
	const uint64_t ones = 0x0101010101010101ull;
	for (; k + 8 <= len; k += 8) {
		uint64_t x;
		memcpy(&x, src + k, 8);
		const uint64_t t = ((x >> 1) ^ (x >> 2)) & (3 * ones); // a nucleotide's code, per byte: ((c & 6) ^ ((c & 6) >> 1)) >> 1
		const uint64_t b0 = t & ones, b1 = (t >> 1) & ones;
		const uint64_t mc = b0 & ~b1, mg = b1 & ~b0, mt = b0 & b1;      // C, G, T (no carries: the sums stay below 0x55)
		const uint64_t expect = 0x41 * ones + 2 * mc + 6 * mg + 0x13 * mt; // the letter that code belongs to
		if (x == expect) {                                                // eight nucleotides: four bytes of symbols
			uint64_t z = (t | (t >> 4)) & 0x00ff00ff00ff00ffull;            // 16-bit lanes: symbol 2j | symbol 2j+1 << 4
			z = (z | (z >> 8)) & 0x0000ffff0000ffffull;
			const uint32_t o = (uint32_t)(z | (z >> 16));
			memcpy(out + k / 2, &o, 4);
		} else {
			for (size_t j = k; j < k + 8; j += 2) {
				const uint32_t lo = lut.v[src[j]], hi = lut.v[src[j + 1]];
				bad |= lo | hi;
				out[j / 2] = (uint8_t)((lo & 7u) | ((hi & 7u) << 4));
			}
		}
	}
	for (; k + 1 < len; k += 2) {
		const uint32_t lo = lut.v[src[k]], hi = lut.v[src[k + 1]];
		bad |= lo | hi;
		out[k / 2] = (uint8_t)((lo & 7u) | ((hi & 7u) << 4));
	}
	if (k < len) { // an odd length: the NUL behind the string is the last byte's other symbol
		const uint32_t lo = lut.v[src[k]];
		bad |= lo;
		out[k / 2] = (uint8_t)((lo & 7u) | (7u << 4));
	}
	return (bad & 0x80u) ? 1 : 0;
}


int pack_queries_host(const andi_hip_seq *seqs, size_t n, int threads, PackedQueries &P) {
	if (!seqs || n == 0 || n >= (size_t)UINT32_MAX) {
		P.err = "andi_hip_queries_stage: bad arguments";
		return 1;
	}
	P.off.resize(n), P.len.resize(n);
	uint64_t cursor = 0;
	for (size_t i = 0; i < n; ++i) { // (the layout of andi_hip_queries_stage)
		if (!seqs[i].seq || seqs[i].len == 0 || seqs[i].len > (size_t)(INT32_MAX - 1) / 2) {
			P.err = "andi_hip_queries_stage: empty or oversized sequence";
			return 1;
		}
		P.off[i] = cursor, P.len[i] = (uint32_t)seqs[i].len, P.total_nt += seqs[i].len;
		cursor += (seqs[i].len + 1 + 255) & ~(uint64_t)255;
	}
	P.pool_bytes = cursor + ANDI_PAD;
	// (2 MiB-aligned and advised as huge pages: 256 threads touching gigabytes of fresh 4 KiB pages queue up in the kernel --
	// C5's 6.4 GB took 1.3 s to pack that way)
	const size_t nib_bytes = (P.pool_bytes / 2 + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
	P.nib = (uint8_t *)aligned_alloc((size_t)2 << 20, nib_bytes);
#ifdef MADV_HUGEPAGE
	if (P.nib) (void)madvise(P.nib, nib_bytes, MADV_HUGEPAGE);
#endif
	if (!P.nib) {
		P.err = "andi_hip_dist_matrix: out of host memory for the packed queries";
		return 1;
	}
	std::atomic<size_t> next{0};
	std::atomic<int> foreign{0};
	auto work = [&]() {
		for (;;) {
			const size_t i = next.fetch_add(1);
			if (i >= n) return;
			const size_t len = seqs[i].len, end = (i + 1 < n ? (size_t)P.off[i + 1] : P.pool_bytes) / 2;
			uint8_t *dst = P.nib + P.off[i] / 2; // (offsets are multiples of 256)
			const size_t w = (len + 1) / 2;
			if (andi_hip_pack_symbols((const unsigned char *)seqs[i].seq, len, dst)) foreign.store(1);
			memset(dst + w, 0x77, end - (P.off[i] / 2 + w)); // NUL, NUL up to the next sequence (the pool's end)
		}
	};
	// (two dozen threads keep up with the host's memory; all 256 cores packing starved the devices' context creation, which
	// runs beside this: C5's contexts 1.3 -> 2.8 s)
	const int nt = std::max(1, std::min(std::min(threads, 24), (int)std::min<size_t>(n, 256)));
	std::vector<std::thread> ts;
	for (int t = 1; t < nt; ++t) ts.emplace_back(work);
	work();
	for (auto &t : ts) t.join();
	P.foreign = foreign.load();
	return 0;
}

int queries_stage_packed(andi_hip_ctx *ctx, const PackedQueries &P, andi_hip_queries **out) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	auto *q = new andi_hip_queries;
	const size_t n = P.off.size();
	q->nq = n, q->off = P.off, q->len = P.len, q->total_nt = P.total_nt;
	hipError_t err = hipSuccess;
	auto chk = [&](hipError_t x) {
		if (err == hipSuccess) err = x;
	};
	chk(dmalloc(&q->pool, P.pool_bytes));
	chk(dmalloc(&q->nib, P.pool_bytes / 2 + 64));
	chk(dmalloc(&q->planes, 3 * (P.pool_bytes / 32) + 16));
	chk(dmalloc(&q->codes, 2 * (P.pool_bytes / 32) + 16));
	if (!(q->h_foreign = (int32_t *)host_pool::word_get())) chk(hipErrorOutOfMemory);
	chk(dmalloc(&q->d_off, n));
	chk(dmalloc(&q->d_len, n));
	if (err == hipSuccess) *q->h_foreign = P.foreign;
	if (err == hipSuccess) err = hipMemcpyAsync(q->nib, P.nib, P.pool_bytes / 2, hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = andi_launch_unpack_symbols(q->nib, P.pool_bytes, q->pool, ctx->stream);
	if (err == hipSuccess) err = andi_launch_pack_planes(q->nib, P.pool_bytes, q->planes, q->codes, ctx->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(q->d_off, q->off.data(), n * 8, hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = hipMemcpyAsync(q->d_len, q->len.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = queries_count_separators(ctx, q);
	if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
	if (err != hipSuccess) {
		andi_hip_queries_free(ctx, q);
		return fail(ctx, "andi_hip_dist_matrix: staging the packed queries", err);
	}
	*out = q;
	return 0;
}

int andi_hip_match_positions(andi_hip_ctx *ctx, const andi_hip_esa *esa, const andi_hip_queries *q,
							 size_t qidx, size_t first, size_t count, int cached,
							 andi_hip_interval *out_host) {
	if (!ctx || !esa || !q || !out_host || qidx >= q->nq || !esa->ref_built) {
		if (ctx) ctx->err = "andi_hip_match_positions: bad arguments (reference arrays not built?)";
		return 1;
	}
	if (first + count > q->len[qidx]) {
		ctx->err = "andi_hip_match_positions: range beyond the query";
		return 1;
	}
	if (count == 0) return 0;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	andi_hip_interval *d_out = nullptr;
	HIP_TRY(ctx, dmalloc(&d_out, count));
	hipError_t e = andi_launch_match_positions(esa_view(esa, ANDI_MODE_REFERENCE), q->pool + q->off[qidx], q->len[qidx],
											   (uint32_t)first, (uint32_t)count, cached, d_out,
											   ctx->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(out_host, d_out, count * sizeof(andi_hip_interval), hipMemcpyDeviceToHost,
						   ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)andi_arena::dev_free(d_out);
	if (e != hipSuccess) return fail(ctx, "andi_hip_match_positions", e);
	return 0;
}

// ------------------------------------------------------------------ the measured copy ceiling (bench.py: roofline.measured_copy_GBps)
extern "C" { // (the kernel's host stub keeps the name it always had)
namespace {
__global__ __launch_bounds__(256) void k_stream_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16) {
	const size_t stride = (size_t)gridDim.x * 256;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
		uint4 v;
		v.x = __builtin_nontemporal_load(&src[i].x), v.y = __builtin_nontemporal_load(&src[i].y);
		v.z = __builtin_nontemporal_load(&src[i].z), v.w = __builtin_nontemporal_load(&src[i].w);
		__builtin_nontemporal_store(v.x, &dst[i].x), __builtin_nontemporal_store(v.y, &dst[i].y);
		__builtin_nontemporal_store(v.z, &dst[i].z), __builtin_nontemporal_store(v.w, &dst[i].w);
	}
}
} // namespace
} // extern "C"

int andi_hip_copy_ceiling(andi_hip_ctx *ctx, size_t bytes, int reps, double *gbps) {
	if (!ctx || !gbps || bytes < 4096 || reps < 1) {
		if (ctx) ctx->err = "andi_hip_copy_ceiling: bad arguments";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t n16 = bytes / 16;
	uint4 *src = nullptr, *dst = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	hipError_t err = hipMalloc((void **)&src, n16 * 16);
	if (err == hipSuccess) err = hipMalloc((void **)&dst, n16 * 16);
	if (err == hipSuccess) err = hipMemsetAsync(src, 1, n16 * 16, ctx->stream);
	if (err == hipSuccess) err = hipEventCreate(&e0);
	if (err == hipSuccess) err = hipEventCreate(&e1);
	int cus = 256;
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
	const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, (size_t)cus * 32);
	float ms = 0;
	if (err == hipSuccess) {
		k_stream_copy<<<grid, 256, 0, ctx->stream>>>(src, dst, n16); // (untimed: first touch)
		err = hipEventRecord(e0, ctx->stream);
		for (int r = 0; r < reps && err == hipSuccess; ++r) k_stream_copy<<<grid, 256, 0, ctx->stream>>>(src, dst, n16);
		if (err == hipSuccess) err = hipEventRecord(e1, ctx->stream);
		if (err == hipSuccess) err = hipEventSynchronize(e1);
		if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
	}
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	if (src) (void)hipFree(src);
	if (dst) (void)hipFree(dst);
	if (err != hipSuccess) return fail(ctx, "andi_hip_copy_ceiling", err);
	*gbps = ms > 0 ? 2.0 * (double)(n16 * 16) * reps / (ms * 1e-3) / 1e9 : 0.0;
	return 0;
}

// ------------------------------------------------------------------ bootstrap
int andi_hip_bootstrap_range(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, uint64_t seed, size_t first,
							 size_t count, andi_hip_model *B) {
	if (!ctx || !M || !B || n == 0 || n > 65535 || first > 0xffffffffull || count > 0xffffffffull ||
		first + count > 0xffffffffull) {
		if (ctx) ctx->err = "andi_hip_bootstrap_range: bad arguments (ctx, M and B must be given, 1 <= n <= 65535, first + count < 2^32)";
		return 1;
	}
	if (count == 0) return 0;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t one = n * n * sizeof(andi_hip_model);
	andi_hip_model *dM = nullptr, *dB = nullptr;
	hipError_t e = hipMalloc((void **)&dM, one);
	if (e == hipSuccess) e = hipMalloc((void **)&dB, one * count);
	if (e == hipSuccess) e = hipMemcpyAsync(dM, M, one, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess)
		e = andi_launch_bootstrap(dM, dB, (uint32_t)n, (uint32_t)first, (uint32_t)count, seed, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(B, dB, one * count, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)andi_arena::dev_free(dM);
	(void)andi_arena::dev_free(dB);
	if (e != hipSuccess) return fail(ctx, "andi_hip_bootstrap_range", e);
	return 0;
}

int andi_hip_bootstrap(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, uint64_t seed,
					   size_t replicates, andi_hip_model *B) {
	if (!ctx || !M || !B || n == 0 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_bootstrap: bad arguments";
		return 1;
	}
	return andi_hip_bootstrap_range(ctx, M, n, seed, 0, replicates, B);
}

void andi_hip_reload_knobs(void) { g_knobs.store(new KnobSnapshot(), std::memory_order_release); }

int andi_hip_timings_get(andi_hip_ctx *ctx, andi_hip_timings *t) {
	if (!ctx || !t) return 1;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	resolve_events(ctx);
	unsigned long long fx = 0, rt[4] = {0, 0, 0, 0};
	HIP_TRY(ctx, hipMemcpy(&fx, ctx->d_fixups, sizeof fx, hipMemcpyDeviceToHost));
	HIP_TRY(ctx, hipMemcpy(rt, ctx->d_route, sizeof rt, hipMemcpyDeviceToHost));
	ctx->acc.fixups = fx;
	ctx->acc.coop_query_nt = rt[0], ctx->acc.lane_query_nt = rt[1], ctx->acc.coop_fallbacks = rt[2];
	*t = ctx->acc;
	return 0;
}

void andi_hip_timings_reset(andi_hip_ctx *ctx) {
	if (!ctx) return;
	(void)hipStreamSynchronize(ctx->stream);
	resolve_events(ctx);
	(void)hipMemset(ctx->d_fixups, 0, sizeof(unsigned long long));
	(void)hipMemset(ctx->d_route, 0, 4 * sizeof(unsigned long long));
	ctx->acc = andi_hip_timings{};
}

