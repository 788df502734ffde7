// seam.hip — andi_hip_dist_matrix (include/andi_hip.h), the one-call replacement of distMatrix/distMatrixLM
// (src/dist_hack.h:34-96), with its row partition and gather; andi_hip_dist_rect, the cross blocks of that matrix for a
// set of references and a set of queries, on the same loop.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types only: librccl is loaded on demand (dlopen), see rccl() below
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_internal.h"
#include "sa_device.h"

// ------------------------------------------------------------------ the seam
// distMatrix / distMatrixLM, src/dist_hack.h:34-96: for every subject build the
// index and compare every other sequence against it.
//
// The rows of the matrix (one subject against every query) are independent given
// the subject's index.  Every device of the call owns a contiguous block of rows
// (block sizes differ by at most one) and is driven by one host thread with its own
// context: all queries staged once, a set of subject slots reused batch after batch,
// its rows kept in HBM.  A pool of host threads shared by all devices prepares RS and
// the suffix array (seq_subject_init + esa_init_SA) in the order the devices will
// ask for them.  The one exchange of the job is the gather of the row blocks on the
// first device -- RCCL send/recv over xGMI, every peer on its own link -- followed by
// one copy of the matrix to the host.  (One device, several contexts on one device,
// or no usable RCCL: every block is copied to the host matrix directly.)
//
// Both calls are one loop over ROW GROUPS: a group's subjects, staged sequences s0 ... s0 + rows - 1, are each scanned
// against one column view of the staged set (andi_hip_queries_view).  The square call has one group, every sequence
// against all of them (its own column the diagonal); andi_hip_dist_rect stages refs ++ queries and has two -- the
// references against view(nr, nq), the queries against view(0, nr) -- with no diagonal in either.
namespace {
struct Prepared {
	size_t idx = 0;
	char *RS = nullptr;
	size_t n = 0, thr = 0;
	std::vector<int32_t> SA;
	int rc = 0;
};

// librccl is loaded when a call first spans several devices: single-device users (and processes
// that carry another copy of RCCL, like PyTorch's) never touch it
struct Rccl {
	void *lib = nullptr;
	ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*GroupStart)() = nullptr;
	ncclResult_t (*GroupEnd)() = nullptr;
	ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
	bool ok = false;
};

Rccl &rccl() {
	static Rccl r;
	static std::once_flag once;
	std::call_once(once, [] {
		const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
		for (const char *nm : names)
			if ((r.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
		if (!r.lib) return;
		r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
		r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
		r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
		r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
		r.Send = (decltype(r.Send))dlsym(r.lib, "ncclSend");
		r.Recv = (decltype(r.Recv))dlsym(r.lib, "ncclRecv");
		r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
		r.ok = r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.GetErrorString;
	});
	return r;
}

thread_local char g_last_gather[200] = "none"; // how the calling thread's last andi_hip_dist_matrix call collected its rows (diagnostic)

void row_block(size_t total, size_t parts, size_t k, size_t &first, size_t &last) { // as andi_amd/shard.py: row_block
	const size_t base = total / parts, extra = total % parts;
	first = k * base + std::min(k, extra);
	last = first + base + (k < extra ? 1 : 0);
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the trace's lap timer: the time since the last lap goes to acc
struct Lap {
	double t = now_ms();
	void operator()(double &acc) {
		const double x = now_ms();
		acc += x - t, t = x;
	}
};

// ---- shared host pool: subject preparation + suffix sorting (the role of the OpenMP subject loop,
// src/dist_hack.h:46-52), in the order the devices consume, bounded look-ahead.  It also holds the call's first error:
// fail_all stops the pool and every device's driver.
struct SubjectPool {
	const andi_hip_seq *seqs;
	const andi_hip_opts &o;
	std::vector<size_t> order; // subjects in the order they are needed
	size_t window;
	std::mutex mu;
	std::condition_variable cv;
	std::deque<Prepared *> ready; // any order
	std::atomic<size_t> next{0};
	size_t consumed = 0; // subjects taken by the devices, guarded by mu
	bool abort_flag = false;
	std::string first_error;
	size_t pairs_done = 0; // guarded by mu (progress)
	std::vector<std::thread> workers;

	SubjectPool(const andi_hip_seq *s, const andi_hip_opts &opts, std::vector<size_t> ord, size_t win) : seqs(s), o(opts), order(std::move(ord)), window(win) {}
	void fail_all(const std::string &msg) {
		std::lock_guard<std::mutex> lk(mu);
		if (!abort_flag) first_error = msg;
		abort_flag = true;
		cv.notify_all();
	}
	void start(int threads) {
		for (int t = 0; t < threads; ++t) workers.emplace_back([this] { work(); });
	}
	void work() {
		const size_t n = order.size();
		for (;;) {
			const size_t pos = next.fetch_add(1);
			if (pos >= n) return;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return abort_flag || pos < consumed + window; });
				if (abort_flag) return;
			}
			const size_t i = order[pos];
			Prepared *p = nullptr;
			try {
				p = new Prepared;
				p->idx = i;
				double gc;
				p->rc = andi_hip_subject_prepare(seqs[i].seq, seqs[i].len, o.p_value, &p->RS, &p->n, &gc, &p->thr);
				if (!p->rc && o.sa_on_host) {
					p->SA.resize(p->n);
					p->rc = andi_hip_suffix_array((const unsigned char *)p->RS, p->SA.data(), (int32_t)p->n);
				}
			} catch (...) { // out of memory: report it as the reference does (src/dist_hack.h:53)
				if (p) {
					andi_hip_free(p->RS);
					delete p;
				}
				char msg[96];
				snprintf(msg, sizeof msg, "Failed to create index for sequence %zu.", i);
				fail_all(msg);
				return;
			}
			{
				std::lock_guard<std::mutex> lk(mu);
				ready.push_back(p);
			}
			cv.notify_all();
		}
	}
	Prepared *take(size_t i) { // blocks until subject i is prepared; null if the call was aborted
		std::unique_lock<std::mutex> lk(mu);
		Prepared *p = nullptr;
		cv.wait(lk, [&] {
			if (abort_flag) return true;
			for (auto *c : ready)
				if (c->idx == i) return true;
			return false;
		});
		if (abort_flag) return nullptr;
		for (auto it = ready.begin(); it != ready.end(); ++it)
			if ((*it)->idx == i) {
				p = *it;
				ready.erase(it);
				break;
			}
		return p;
	}
	void consume() { // a subject the devices took: the look-ahead moves on
		{
			std::lock_guard<std::mutex> lk(mu);
			++consumed;
		}
		cv.notify_all();
	}
	void stop() { // (the drivers are done): release any waiting worker, free what they prepared in vain
		{
			std::lock_guard<std::mutex> lk(mu);
			consumed = order.size();
			if (abort_flag) next.store(order.size());
		}
		cv.notify_all();
		for (auto &t : workers) t.join();
		for (auto *p : ready) {
			andi_hip_free(p->RS);
			delete p;
		}
	}
};

// the queries as 4-bit symbols, packed once on the host for all devices while their contexts come up (pack_queries_host)
struct QueryPacker {
	PackedQueries PQ;
	std::mutex mu;
	std::condition_variable cv;
	bool done = false;
	int rc = 0;
	std::thread th;
	void start(const andi_hip_seq *seqs, size_t n, int threads, size_t users) {
		PQ.users.store((int)users);
		th = std::thread([=] {
			const int r = pack_queries_host(seqs, n, threads, PQ);
			std::lock_guard<std::mutex> lk(mu);
			rc = r, done = true;
			cv.notify_all();
		});
	}
	int wait() {
		std::unique_lock<std::mutex> lk(mu);
		cv.wait(lk, [&] { return done; });
		return rc;
	}
	void join() {
		if (th.joinable()) th.join();
	}
	~QueryPacker() { join(); }
};

// a block of rows of one call: subjects s0 ... s0 + rows - 1 of the staged set, each against the queries v0 ... v0 + vn - 1
// of it, row s0 + r to out + r * vn.  diagonal: the view is the whole set and subject i is query i (self = i: the square
// call); otherwise no subject meets itself (self = -1).  hint: andi_hip_ctx_expect_queries for its subjects.
struct RowGroup {
	size_t s0, rows, v0, vn;
	andi_hip_model *out;
	bool diagonal;
	size_t hint;
	std::vector<size_t> first, last; // the devices' row blocks (staged-set indices)
};

// what every device's driver of one call shares
struct SeamCall {
	const char *name;         // the entry point (error messages, trace lines)
	const andi_hip_seq *seqs; // the staged set
	size_t n;
	andi_hip_opts o;
	std::vector<RowGroup> groups;
	size_t width = 0, hint_max = 0; // the widest group's vn, the largest hint
	size_t pairs_total = 0;         // (progress)
	bool allow_rccl = false;        // (the square call's gather)
	std::vector<int> devs;
	size_t rs_cap;                   // the longest subject's RS
	bool dev_prep;                   // RS and suffix arrays made on the device (not sa_on_host)
	size_t batch_max;
	bool use_rccl, pack_on_host, trace;
	double t_call;
	SubjectPool *pool;
	QueryPacker *packer;
};

// ---- one driver per device.  Two stages, two contexts (streams) and two sets of subject slots per device: while the
// scan of one batch of subjects runs, a second thread stages the next -- upload, suffix arrays, index builds -- as
// the reference's threads build one subject's index while others scan (src/dist_hack.h:46-52).
struct Driver {
	const SeamCall &C;
	const size_t d;
	const int dev;
	andi_hip_ctx *ctx = nullptr;  // scans, row copies
	andi_hip_ctx *prep = nullptr; // suffix arrays, index builds
	andi_hip_ctx *up = nullptr;   // uploads (a thread and a stream of their own: the copies of batch k + 1 run beside the sorts of batch k)
	std::vector<andi_hip_ctx *> sorters; // suffix sorts of a batch's subjects side by side (streams and workspaces of their own)
	andi_hip_queries *Q = nullptr;
	std::vector<andi_hip_queries *> views; // per group: its column view of Q (null: Q whole)
	andi_hip_model *d_rows = nullptr; // rccl: the whole row block; direct: one batch of rows
	size_t pinned_bytes = 0;
	char *pinned = nullptr;           // staging buffers for RS (two: one is filled while the other's copy runs): uploads from pinned memory go through the DMA engines, beside a scan
	hipEvent_t pinned_free[2] = {nullptr, nullptr};
	std::vector<andi_hip_esa *> slots; // sets x batch
	std::vector<unsigned long long> gcs; // G+C of every sequence (calc_gc, src/sequence.c:197-208)
	size_t rows = 0, batch = 0, nbatches = 0, sets = 0;
	struct Batch {
		size_t g, i0, nb; // its group, first subject, size
	};
	std::vector<Batch> batches; // (no batch spans two groups: one scan call has one view)
	char eb[256] = "";
	// hand-over between the stages
	std::mutex pm;
	std::condition_variable pcv;
	size_t prepared = 0, scanned = 0; // batches staged / scanned so far
	size_t uploaded = 0;              // batches whose texts are on the device
	bool prep_failed = false;
	// the trace (device 0)
	double t_ctx = 0, t_queries = 0, t_slots = 0, p_take = 0, p_upload = 0, p_sort = 0, p_build = 0, acc_wait = 0, acc_scan = 0, acc_copy = 0;

	Driver(const SeamCall &call, size_t k) : C(call), d(k), dev(call.devs[k]) {
		for (const RowGroup &G : C.groups) rows += G.last[d] - G.first[d];
	}

	void bail(const char *what, andi_hip_ctx *cx) {
		char msg[512];
		snprintf(msg, sizeof msg, "%s (device %d): %s", what, dev, cx ? andi_hip_last_error(cx) : eb);
		C.pool->fail_all(msg);
	}
	void give_up() {
		std::lock_guard<std::mutex> lk(pm);
		prep_failed = true;
		pcv.notify_all();
	}
	void set_progress(size_t &counter, size_t k) { // a stage's batch k is done
		{
			std::lock_guard<std::mutex> lk(pm);
			counter = k + 1;
		}
		pcv.notify_all();
	}
	// batch k: its first subject, its size, its set of slots, its group
	size_t batch_first(size_t k) const { return batches[k].i0; }
	size_t batch_size(size_t k) const { return batches[k].nb; }
	andi_hip_esa **batch_set(size_t k) { return slots.data() + (k % sets) * batch; }
	const RowGroup &batch_group(size_t k) const { return C.groups[batches[k].g]; }
	size_t sets_for(size_t bt) const { // (low_memory: one index resident at a time)
		const size_t nb = (rows + bt - 1) / bt;
		return C.o.low_memory ? (size_t)1 : (nb > 2 && !C.dev_prep ? (size_t)3 : (nb > 1 ? (size_t)2 : (size_t)1)); // (the third set is the uploads')
	}

	bool open();
	void upload_loop();
	void stage_loop();
	void scan_loop();
	void run();
	void close();
};

// contexts, sorters, queries, G+C counts, slot sets, pinned buffers, row buffer; false (the error reported) if one fails
bool Driver::open() {
	Lap lap;
	const size_t n = C.n;
	if (andi_hip_ctx_create(&ctx, dev, eb, sizeof eb)) return bail("creating a context", nullptr), false;
	if (ctx_create(&prep, dev, eb, sizeof eb, true)) return bail("creating a context", nullptr), false;
	if (!C.dev_prep) {
		if (ctx_create(&up, dev, eb, sizeof eb, true)) return bail("creating a context", nullptr), false;
		andi_hip_ctx_expect_queries(up, C.hint_max);
	}
	// A suffix sort is two dozen launches with two or three host round trips between them (sa_device.hip): 0.73 ms per
	// 9.8 M characters of which the device is busy half.  The subjects of a batch are sorted by up to four host threads,
	// each with a stream and a workspace of its own, so one subject's small launches and waits hide behind another's
	// radix passes.
	size_t sort_width = C.dev_prep && !C.o.low_memory ? std::min<size_t>(4, std::min(C.batch_max, rows)) : 1;
	// (a workspace of 45 bytes per character each: together at most one chunk of the arena -- eight of them for 9.8 M characters pushed a
	// 29-genome call past the 8 GiB the arena keeps from call to call, and every call paid the driver for its chunks again: 37 -> 177 ms;
	// two sorters measured like four, profiles/r07_seam/)
	while (sort_width > 1 && andi_sa_device_workspace((int32_t)C.rs_cap) * sort_width > ((size_t)2 << 30)) --sort_width;
	for (size_t w = 1; w < sort_width; ++w) {
		andi_hip_ctx *cx = nullptr;
		if (ctx_create(&cx, dev, eb, sizeof eb, true)) return bail("creating a context", nullptr), false;
		andi_hip_ctx_expect_queries(cx, C.hint_max);
		sorters.push_back(cx);
	}
	// (the slots are sized for the largest hint; every batch is staged with its group's: upload_loop, stage_loop)
	andi_hip_ctx_expect_queries(ctx, C.hint_max);
	andi_hip_ctx_expect_queries(prep, C.hint_max);
	lap(t_ctx);
	// Subject slots: device buffers sized for the longest genome, reused batch after batch (no
	// allocation inside the loop).  Several subjects per scan call keep the GPU filled; low_memory
	// keeps one index resident at a time, which is what distMatrixLM trades (src/dist_hack.h:14-16).
	batch = C.batch_max < rows ? C.batch_max : rows;
	{
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			// a slot: text + padding, suffix array, the records of the device sorter, the packed text twice, the probe table
			const size_t per_slot = 14 * C.rs_cap + ((size_t)8 << (2 * pick_deep_k(C.rs_cap, ctx->queries_hint))) + (1 << 20);
			while (batch > 1 && sets_for(batch) * batch * per_slot > free_b / (2 * C.devs.size())) batch /= 2; // (as many sets as the batches will really have)
		}
	}
	for (size_t g = 0; g < C.groups.size(); ++g)
		for (size_t i = C.groups[g].first[d]; i < C.groups[g].last[d]; i += batch) batches.push_back({g, i, std::min(batch, C.groups[g].last[d] - i)});
	nbatches = batches.size();
	// Three sets of slots: while batch k is scanned, batch k + 2 is uploaded (no compute units needed) and batch k + 1
	// is ready; the device's COMPUTE alternates strictly -- suffix sorts and index builds of batch k + 1, then the scan
	// of batch k -- because side by side the staging kernels starve behind the workgroups of a scan that fills the
	// device (sorts of 8 subjects: 6 ms alone, 38 ms beside a scan, on a high-priority stream as on a plain one).
	sets = sets_for(batch);
	slots.assign(sets * batch, nullptr);
	if (C.pack_on_host) {
		if (C.packer->wait()) {
			snprintf(eb, sizeof eb, "%s", C.packer->PQ.err.c_str());
			return bail("staging queries", nullptr), false;
		}
		const int rc = queries_stage_packed(ctx, C.packer->PQ, &Q);
		if (C.packer->PQ.users.fetch_sub(1) == 1) C.packer->PQ.release(); // (every device has its copy)
		if (rc) return bail("staging queries", ctx), false;
	} else if (andi_hip_queries_stage(ctx, C.seqs, n, &Q)) {
		return bail("staging queries", ctx), false;
	}
	for (const RowGroup &G : C.groups) {
		andi_hip_queries *v = nullptr;
		if (!(G.v0 == 0 && G.vn == n) && andi_hip_queries_view(ctx, Q, G.v0, G.vn, &v)) return bail("staging queries", ctx), false;
		views.push_back(v);
	}
	if (C.dev_prep && queries_gc_counts(ctx, Q, gcs)) return bail("staging queries", ctx), false;
	lap(t_queries);
	for (size_t b = 0; b < sets * batch; ++b)
		if (esa_reserve(prep, C.rs_cap, &slots[b])) return bail("allocating subject slots", prep), false;
	if (andi_hip_sync(prep)) return bail("allocating subject slots", prep), false;
	double t_reserve = 0, t_pinned = 0;
	lap(t_reserve);
	pinned_bytes = 2 * (C.rs_cap + 64);
	if (C.dev_prep || host_pool::pinned_get((void **)&pinned, pinned_bytes) != hipSuccess) pinned = nullptr; // (then from where RS lies)
	if (pinned && (hipEventCreateWithFlags(&pinned_free[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&pinned_free[1], hipEventDisableTiming) != hipSuccess)) {
		host_pool::pinned_put(pinned, pinned_bytes);
		pinned = nullptr;
	}
	lap(t_pinned);
	if (andi_hip_dev_alloc(ctx, (C.use_rccl ? rows : batch) * C.width * sizeof(andi_hip_model), (void **)&d_rows)) return bail("row buffer", ctx), false;
	lap(t_slots);
	t_slots += t_reserve + t_pinned;
	if (C.trace && d == 0) fprintf(stderr, "%s trace: slots = device buffers of %zu slots %.1f ms + pinned upload buffer %.1f ms + row buffer %.1f ms\n", C.name, sets * batch, t_reserve, t_pinned, t_slots - t_reserve - t_pinned);
	return true;
}

// the upload thread of this device (sa_on_host): texts from the host pool into the slot sets, a batch ahead of the sorts
void Driver::upload_loop() {
	(void)hipSetDevice(dev);
	Lap plap;
	size_t nup = 0; // texts uploaded so far
	for (size_t k = 0; k < nbatches; ++k) {
		{
			std::unique_lock<std::mutex> lk(pm);
			pcv.wait(lk, [&] { return k < scanned + sets || prep_failed; }); // its set of slots is free again
			if (prep_failed) return;
		}
		plap.t = now_ms();
		const size_t i0 = batch_first(k), nb = batch_size(k);
		andi_hip_esa **set = batch_set(k);
		andi_hip_ctx_expect_queries(up, batch_group(k).hint);
		for (size_t b = 0; b < nb; ++b) { // uploads: beside whatever the device computes
			Prepared *p = C.pool->take(i0 + b);
			if (!p) return give_up();
			plap(p_take);
			bool ok = true;
			if (p->rc) {
				char msg[96];
				snprintf(msg, sizeof msg, "Failed to create index for sequence %zu.", i0 + b); // src/dist_hack.h:53
				C.pool->fail_all(msg);
				ok = false;
			}
			// through one of two pinned buffers: the next text is copied into the other while this one's transfer runs
			const bool two = pinned && !C.o.sa_on_host; // (a suffix array from the host is pageable memory: that copy waits anyway)
			const size_t pb = nup++ & 1;
			char *pin = pinned ? pinned + pb * (C.rs_cap + 64) : nullptr;
			if (ok && two && nup > 2 && hipEventSynchronize(pinned_free[pb]) != hipSuccess) bail("staging subject", up), ok = false;
			const char *src = p->RS;
			if (ok && pin) memcpy(pin, p->RS, p->n), src = pin;
			if (ok && esa_upload(up, set[b], src, C.o.sa_on_host ? p->SA.data() : nullptr, p->n, p->thr, two ? pinned_free[pb] : nullptr)) bail("staging subject", up), ok = false;
			plap(p_upload);
			andi_hip_free(p->RS);
			delete p;
			C.pool->consume();
			if (!ok) return give_up();
		}
		if (andi_hip_sync(up)) { // (the batch's transfers)
			bail("staging subject", up);
			return give_up();
		}
		plap(p_upload);
		set_progress(uploaded, k);
	}
}

// the staging thread of this device: RS written from the resident sequences and suffix sorts (unless sa_on_host), index builds
void Driver::stage_loop() {
	(void)hipSetDevice(dev);
	Lap plap;
	for (size_t k = 0; k < nbatches; ++k) {
		{ // the batch's texts are there; with three sets the device's compute is this batch's once the scan of batch k - 2 is done
			std::unique_lock<std::mutex> lk(pm);
			pcv.wait(lk, [&] { return (uploaded > k && (C.dev_prep ? k < scanned + sets : (sets < 3 || k < scanned + 2))) || prep_failed; });
			if (prep_failed) return;
		}
		plap.t = now_ms();
		const size_t i0 = batch_first(k), nb = batch_size(k);
		andi_hip_esa **set = batch_set(k);
		andi_hip_ctx_expect_queries(prep, batch_group(k).hint);
		for (andi_hip_ctx *cx : sorters) andi_hip_ctx_expect_queries(cx, batch_group(k).hint);
		// RS from the resident sequence (the threshold on the host, same libm: src/sequence.c:210-219), then its suffix array
		auto text_and_sort = [&](andi_hip_ctx *cx, size_t b) -> const char * {
			const size_t i = i0 + b, len = C.seqs[i].len;
			const size_t thr = andi_hip_min_anchor_length(C.o.p_value, (double)gcs[i] / len, 2 * len + 1);
			if (esa_from_query(cx, set[b], Q, i, thr)) return "staging subject";
			if (esa_sort_suffixes(cx, set[b])) return "suffix array";
			return nullptr;
		};
		if (C.dev_prep) {
			const size_t width = std::min(nb, sorters.size() + 1);
			std::atomic<size_t> next_b{0};
			std::mutex em;
			const char *what = nullptr;
			andi_hip_ctx *where = nullptr;
			auto sort_some = [&](andi_hip_ctx *cx) {
				(void)hipSetDevice(dev);
				for (;;) {
					const size_t b = next_b.fetch_add(1);
					if (b >= nb) break;
					const char *w = text_and_sort(cx, b);
					if (w) {
						std::lock_guard<std::mutex> lk(em);
						if (!what) what = w, where = cx;
						next_b.store(nb);
						break;
					}
				}
				if (andi_hip_sync(cx)) {
					std::lock_guard<std::mutex> lk(em);
					if (!what) what = "suffix array", where = cx;
				}
			};
			std::vector<std::thread> helpers;
			for (size_t w = 1; w < width; ++w) helpers.emplace_back(sort_some, sorters[w - 1]);
			sort_some(prep);
			for (auto &t : helpers) t.join();
			if (what) {
				bail(what, where);
				return give_up();
			}
			plap(p_sort);
		}
		if (andi_hip_esa_build_index_batch(prep, set, nb) || andi_hip_sync(prep)) {
			bail("index build", prep);
			return give_up();
		}
		plap(p_build);
		set_progress(prepared, k);
	}
}

// the scan thread (the driver's own): every batch once it is staged, its rows to the host or into the row block
void Driver::scan_loop() {
	// the device's compute alternates between the stages where a slot set is free for it: stage k + 1, then scan k
	const bool alternate = sets >= (C.dev_prep ? (size_t)2 : (size_t)3);
	std::vector<int64_t> self(batch);
	bool failed = false;
	Lap lap;
	for (size_t k = 0; k < nbatches && !failed; ++k) {
		{
			std::unique_lock<std::mutex> lk(pm);
			pcv.wait(lk, [&] { return (prepared > k && (!alternate || prepared > k + 1 || prepared == nbatches)) || prep_failed; });
			if (prepared <= k) break; // (the staging thread has reported why)
		}
		lap(acc_wait);
		const size_t i0 = batch_first(k), nb = batch_size(k);
		andi_hip_esa **set = batch_set(k);
		const RowGroup &G = batch_group(k);
		const andi_hip_queries *view = views[batches[k].g] ? views[batches[k].g] : Q;
		for (size_t b = 0; b < nb; ++b) self[b] = G.diagonal ? (int64_t)(i0 + b) : -1;
		andi_hip_model *dst = C.use_rccl ? d_rows + (i0 - G.first[d]) * G.vn : d_rows;
		if (andi_hip_scan_rows(ctx, set, self.data(), nb, view, C.o.model, C.o.segment, dst)) bail("scan", ctx), failed = true;
		if (!failed && C.trace) (void)andi_hip_sync(ctx);
		lap(acc_scan);
		if (!failed && !C.use_rccl && andi_hip_copy_to_host(ctx, G.out + (i0 - G.s0) * G.vn, dst, nb * G.vn * sizeof(andi_hip_model))) bail("row copy", ctx), failed = true;
		if (!failed && C.use_rccl && andi_hip_sync(ctx)) bail("scan", ctx), failed = true; // the slots are reused
		lap(acc_copy);
		{
			std::lock_guard<std::mutex> lk(pm);
			scanned = k + 1;
			if (failed) prep_failed = true;
		}
		pcv.notify_all();
		if (!failed && C.o.progress) {
			std::lock_guard<std::mutex> lk(C.pool->mu);
			C.pool->pairs_done += nb * (G.diagonal ? G.vn - 1 : G.vn);
			C.o.progress(C.pool->pairs_done, C.pairs_total, C.o.ud);
		}
	}
	{
		std::lock_guard<std::mutex> lk(pm);
		if (scanned < nbatches) prep_failed = true; // (release the staging thread)
	}
	pcv.notify_all();
}

void Driver::run() {
	if (!open()) return;
	uploaded = C.dev_prep ? nbatches : 0; // (texts written on the device by the staging thread itself: all of them there)
	std::thread uploader;
	if (!C.dev_prep) uploader = std::thread([this] { upload_loop(); });
	std::thread stager([this] { stage_loop(); });
	scan_loop();
	stager.join();
	if (uploader.joinable()) uploader.join();
	if (C.trace && d == 0)
		fprintf(stderr, "%s trace (ms): contexts %.1f, queries %.1f, slots %.1f | staging thread: waiting for the host pool %.1f, subject %s %.1f, suffix arrays %.1f, index builds %.1f | scan thread: waiting for staged subjects %.1f, scans %.1f, row copies %.1f; driver total %.1f (%zu batches of %zu, %zu slot sets)\n", C.name,
				t_ctx, t_queries, t_slots, p_take, C.dev_prep ? "texts written on the device" : "uploads", p_upload, p_sort, p_build, acc_wait, acc_scan, acc_copy, now_ms() - C.t_call, nbatches, batch, sets);
}

// whatever open() got to (slots, rows and queries exist only once ctx does)
void Driver::close() {
	for (auto *cx : sorters) andi_hip_ctx_destroy(cx);
	for (auto *e : slots)
		if (e) andi_hip_esa_free(ctx, e);
	if (d_rows) andi_hip_dev_free(ctx, d_rows);
	for (auto *v : views)
		if (v) andi_hip_queries_free(ctx, v);
	if (Q) andi_hip_queries_free(ctx, Q);
	if (pinned) host_pool::pinned_put(pinned, pinned_bytes);
	for (hipEvent_t ev : pinned_free)
		if (ev) (void)hipEventDestroy(ev);
	if (prep) andi_hip_ctx_destroy(prep);
	if (up) andi_hip_ctx_destroy(up);
	if (ctx) andi_hip_ctx_destroy(ctx);
}

// ---- the gather: row blocks to the first device over RCCL, one copy to the host.  RCCL unusable on this box: the rows are
// still in HBM -- every block is copied to the host directly.  Returns nonzero (err set) if that fails too.
int gather_rccl(const SeamCall &C, const std::vector<std::unique_ptr<Driver>> &dv, std::string &first_error) {
	const size_t n = C.n, ndev = dv.size();
	const std::vector<size_t> &first = C.groups[0].first, &last = C.groups[0].last; // (the square call's one group)
	andi_hip_model *const M = C.groups[0].out;
	const std::vector<int> &devs = C.devs;
	Rccl &R = rccl();
	std::vector<ncclComm_t> comms(ndev, nullptr);
	andi_hip_model *d_full = nullptr;
	std::string err;
	auto nccl_ok = [&](ncclResult_t r, const char *what) {
		if (r == ncclSuccess) return true;
		if (err.empty()) err = std::string(what) + ": " + R.GetErrorString(r);
		return false;
	};
	// one process, one node: the communicators bootstrap over the loopback interface unless the caller chose one;
	// the caller's environment is put back as it was (a later multi-node initialisation in this process must not
	// inherit the loopback)
	// (RCCL takes the interface from the process environment and from nowhere else: two of this library's calls are
	// kept apart by a lock; a caller whose OTHER threads read or write the environment meanwhile sets
	// NCCL_SOCKET_IFNAME itself before its first call -- the library then leaves the environment alone, andi_hip.h)
	static std::mutex env_lock;
	bool ok;
	{
		std::lock_guard<std::mutex> guard(env_lock);
		const bool had_ifname = getenv("NCCL_SOCKET_IFNAME") != nullptr;
		if (!had_ifname) setenv("NCCL_SOCKET_IFNAME", "lo", 0);
		ok = nccl_ok(R.CommInitAll(comms.data(), (int)ndev, devs.data()), "ncclCommInitAll");
		if (!had_ifname) unsetenv("NCCL_SOCKET_IFNAME");
	}
	if (ok && hipSetDevice(devs[0]) != hipSuccess) ok = false, err = "hipSetDevice";
	if (ok && hipMalloc((void **)&d_full, n * n * sizeof(andi_hip_model)) != hipSuccess) ok = false, err = "allocating the gathered matrix";
	if (ok) {
		ok = nccl_ok(R.GroupStart(), "ncclGroupStart");
		for (size_t d = 1; d < ndev && ok; ++d) {
			const size_t bytes = (last[d] - first[d]) * n * sizeof(andi_hip_model);
			// (every call with the device of its communicator current)
			ok = hipSetDevice(devs[d]) == hipSuccess &&
				 nccl_ok(R.Send(dv[d]->d_rows, bytes, ncclUint8, 0, comms[d], dv[d]->ctx->stream), "ncclSend") &&
				 hipSetDevice(devs[0]) == hipSuccess &&
				 nccl_ok(R.Recv(d_full + first[d] * n, bytes, ncclUint8, (int)d, comms[0], dv[0]->ctx->stream), "ncclRecv");
		}
		if (!nccl_ok(R.GroupEnd(), "ncclGroupEnd")) ok = false;
	}
	if (ok) { // the first device's own block, then everything to the host
		hipError_t e = hipSetDevice(devs[0]);
		if (e == hipSuccess)
			e = hipMemcpyAsync(d_full + first[0] * n, dv[0]->d_rows, (last[0] - first[0]) * n * sizeof(andi_hip_model),
							   hipMemcpyDeviceToDevice, dv[0]->ctx->stream);
		for (size_t d = 1; d < ndev && e == hipSuccess; ++d) {
			e = hipSetDevice(devs[d]);
			if (e == hipSuccess) e = hipStreamSynchronize(dv[d]->ctx->stream);
		}
		if (e == hipSuccess) e = hipSetDevice(devs[0]);
		if (e == hipSuccess) e = hipStreamSynchronize(dv[0]->ctx->stream);
		if (e == hipSuccess) e = hipMemcpy(M, d_full, n * n * sizeof(andi_hip_model), hipMemcpyDeviceToHost);
		if (e != hipSuccess) ok = false, err = std::string("gathering the matrix: ") + hipGetErrorString(e);
	}
	for (auto cm : comms)
		if (cm) (void)R.CommDestroy(cm);
	if (d_full) {
		(void)hipSetDevice(devs[0]);
		(void)andi_arena::dev_free(d_full);
	}
	if (ok) return 0;
	snprintf(g_last_gather, sizeof g_last_gather, "direct (rccl: %.160s)", err.c_str());
	for (size_t d = 0; d < ndev; ++d)
		if (andi_hip_copy_to_host(dv[d]->ctx, M + first[d] * n, dv[d]->d_rows, (last[d] - first[d]) * n * sizeof(andi_hip_model))) {
			first_error = std::string("row copy: ") + andi_hip_last_error(dv[d]->ctx);
			return 1;
		}
	return 0;
}

// the devices of the call (0, error text set: none usable)
int pick_devices(const char *name, const andi_hip_opts &o, size_t n, std::vector<int> &devs, char *errbuf, size_t errlen) {
	int visible = 0;
	hipError_t e = hipGetDeviceCount(&visible);
	if (e != hipSuccess || visible <= 0) {
		set_err(errbuf, errlen, "no HIP device available (%s); the anchor-distance engine has no CPU path",
				e != hipSuccess ? hipGetErrorString(e) : "device count 0");
		return 1;
	}
	if (o.devices && o.num_gpus > 0) {
		devs.assign(o.devices, o.devices + o.num_gpus);
	} else {
		const int want = o.num_gpus < 0 ? visible - o.device : (o.num_gpus == 0 ? 1 : o.num_gpus);
		for (int k = 0; k < want; ++k) devs.push_back(o.device + k);
	}
	for (int d : devs)
		if (d < 0 || d >= visible) {
			set_err(errbuf, errlen, "HIP device %d out of range (have %d)", d, visible);
			return 1;
		}
	if (devs.empty()) {
		set_err(errbuf, errlen, "%s: no device selected", name);
		return 1;
	}
	if (devs.size() > n) devs.resize(n); // at least one row each
	return 0;
}

// RCCL gather: several distinct devices (or forced, to exercise the path on the devices there are -- with contexts that
// share a device the communicators cannot be made: the route's fallback, every block copied from HBM directly, runs),
// and the matrix fits next to the rest
bool want_rccl(const std::vector<int> &devs, size_t n) {
	const size_t ndev = devs.size();
	bool distinct = true;
	for (size_t a = 0; a < ndev; ++a)
		for (size_t b = a + 1; b < ndev; ++b) distinct = distinct && devs[a] != devs[b];
	const char *gather_env = andi_knob(KNOB_GATHER);
	bool use_rccl = (ndev > 1 && distinct && !(gather_env && !strcmp(gather_env, "direct"))) ||
					(gather_env && !strcmp(gather_env, "rccl"));
	if (use_rccl && n * n * sizeof(andi_hip_model) > ((size_t)32 << 30)) use_rccl = false;
	if (use_rccl && !rccl().ok) use_rccl = false;
	return use_rccl;
}
// sequence checks of both calls (src/andi.c:296-304), before any HIP call; `what` names the set in the message
bool check_seqs(const andi_hip_seq *seqs, size_t n, const char *what, char *errbuf, size_t errlen) {
	for (size_t i = 0; i < n; ++i) {
		if (!seqs[i].seq || seqs[i].len == 0) {
			set_err(errbuf, errlen, "%s %zu is empty", what, i); // src/andi.c:302-304
			return false;
		}
		if (seqs[i].len > (size_t)(INT32_MAX - 1) / 2) { // src/andi.c:296-300
			set_err(errbuf, errlen, "%s %zu is too long. The technical limit is %zu.", what, i, (size_t)(INT32_MAX - 1) / 2);
			return false;
		}
	}
	return true;
}

// The call once its groups are set: devices, every group's tiling, the host pool, one driver per device, the gather.
// dev_rows: the most devices the call can give a row each.
int run_seam(SeamCall &C, size_t dev_rows, char *errbuf, size_t errlen) {
	const andi_hip_opts &o = C.o;
	const andi_hip_seq *seqs = C.seqs;
	const size_t n = C.n;
	if (pick_devices(C.name, o, dev_rows, C.devs, errbuf, errlen)) return 1;
	const size_t ndev = C.devs.size();
	C.use_rccl = C.allow_rccl && want_rccl(C.devs, n);

	size_t longest = 0;
	for (size_t i = 0; i < n; ++i) longest = std::max(longest, seqs[i].len);
	C.rs_cap = 2 * longest + 1;
	std::vector<std::vector<size_t>> mine(ndev); // every device's subjects in the order it stages them
	for (RowGroup &G : C.groups) {
		G.first.resize(ndev), G.last.resize(ndev);
		for (size_t d = 0; d < ndev; ++d) {
			row_block(G.rows, ndev, d, G.first[d], G.last[d]);
			G.first[d] += G.s0, G.last[d] += G.s0;
			for (size_t i = G.first[d]; i < G.last[d]; ++i) mine[d].push_back(i);
		}
		C.width = std::max(C.width, G.vn);
		C.hint_max = std::max(C.hint_max, G.hint);
	}
	size_t max_rows = 0;
	for (auto &m : mine) max_rows = std::max(max_rows, m.size());
	std::vector<size_t> order; // subjects in the order they are needed
	order.reserve(n);
	for (size_t k = 0; k < max_rows; ++k)
		for (size_t d = 0; d < ndev; ++d)
			if (k < mine[d].size()) order.push_back(mine[d][k]);
	int threads = o.host_threads > 0 ? o.host_threads : (int)std::thread::hardware_concurrency();
	if (threads < 1) threads = 1;
	if ((size_t)threads > n) threads = (int)n;
	// Every subject is also a query, and the queries are staged in HBM before the first batch: unless the suffix arrays are
	// the host's (sa_on_host: the sorter needs RS where it runs), a device writes RS = revcomp(S) '#' S into the subject's
	// slot itself from its query pool (esa_from_query) and the host computes only min_anchor_length from the device's G+C
	// counts -- no host pass over the sequences, no second upload of what is already resident (round 5's trace of the bench
	// set's warm call: host pool 5.5 ms + subject uploads 12.9 ms of 54).
	C.dev_prep = !o.sa_on_host;
	// Calls without a diagonal (andi_hip_dist_rect) take 32 subjects per scan call: with one or a few queries per reference
	// row a batch of 8 is a scan call of a few launches' latency (3085 references x 1 query of 2.1 Mbp: scans 235 -> 90 ms,
	// the call 1.19 -> 0.96 s; the bench set's 28 + 1: 23.4 -> 21.7 ms; profiles/rect_c4.json, rect_bench_batches.json)
	C.batch_max = o.low_memory ? 1 : (C.groups[0].diagonal ? 8 : 32);
	if (const char *rb = andi_knob(KNOB_RECT_BATCH)) // (experiments: subjects per scan call of a call without a diagonal)
		if (!o.low_memory && !C.groups[0].diagonal && atoi(rb) >= 1 && atoi(rb) <= 64) C.batch_max = (size_t)atoi(rb);
	SubjectPool pool(seqs, C.o, std::move(order), (size_t)threads + ndev * C.batch_max + 1);
	C.pool = &pool;

	C.trace = andi_knob(KNOB_E2E_TRACE) != nullptr; // diagnostics: where the call's wall time goes (device 0's driver)
	C.t_call = now_ms();
	// the queries as 4-bit symbols, packed once for all devices while their contexts come up (ANDI_QUERIES_BYTES: every
	// device uploads the bytes and packs them itself, as up to round 3)
	// One device: the bytes as they lie (measured on one GPU, same box: C4's queries 0.51 s as bytes, 0.10 s packed -- but the
	// pack's pass over the host's memory and the release of its copy gave the 0.3 s back; C5 was slower packed).
	C.pack_on_host = andi_knob(KNOB_QUERIES_BYTES) == nullptr && (ndev > 1 || andi_knob(KNOB_QUERIES_PACKED) != nullptr);
	QueryPacker packer;
	C.packer = &packer;
	if (C.pack_on_host) packer.start(seqs, n, threads, ndev);

	std::vector<std::unique_ptr<Driver>> dv;
	for (size_t d = 0; d < ndev; ++d) dv.emplace_back(new Driver(C, d));
	if (!C.dev_prep) pool.start(threads);
	if (ndev == 1) {
		dv[0]->run(); // the calling thread, as before
	} else {
		std::vector<std::thread> drivers;
		for (size_t d = 0; d < ndev; ++d) drivers.emplace_back([&dv, d] { dv[d]->run(); });
		for (auto &t : drivers) t.join();
	}
	pool.stop();
	packer.join();
	int rc = pool.abort_flag ? 1 : 0;
	const double t_drivers_done = now_ms();

	snprintf(g_last_gather, sizeof g_last_gather, "%s", C.use_rccl ? "rccl" : "direct");
	if (!rc && C.use_rccl) rc = gather_rccl(C, dv, pool.first_error);
	if (rc) set_err(errbuf, errlen, "%s", pool.first_error.empty() ? (std::string(C.name) + " failed").c_str() : pool.first_error.c_str());
	const double t_gathered = now_ms();

	for (auto &D : dv) D->close();
	if (C.trace) fprintf(stderr, "%s trace: call total %.1f ms (gather %.1f, slots, queries and contexts released %.1f)\n", C.name, now_ms() - C.t_call, t_gathered - t_drivers_done, now_ms() - t_gathered);
	return rc;
}
} // namespace

extern "C" {

const char *andi_hip_last_gather(void) {
	return g_last_gather;
}

void andi_hip_row_block(size_t total, size_t parts, size_t k, size_t *first, size_t *last) {
	size_t f = 0, l = 0;
	if (parts && k < parts) row_block(total, parts, k, f, l);
	if (first) *first = f;
	if (last) *last = l;
}

int andi_hip_dist_matrix(andi_hip_model *M, const andi_hip_seq *seqs, size_t n,
						 const andi_hip_opts *opts_in, char *errbuf, size_t errlen) {
	if (!M || !seqs || n == 0) {
		set_err(errbuf, errlen, "andi_hip_dist_matrix: bad arguments");
		return 1;
	}
	SeamCall C;
	C.name = "andi_hip_dist_matrix";
	C.seqs = seqs, C.n = n;
	if (opts_in) {
		C.o = *opts_in;
	} else {
		andi_hip_default_opts(&C.o);
	}
	if (!check_seqs(seqs, n, "sequence", errbuf, errlen)) return 1;
	// one group: every sequence against all of them (distMatrix compares every sequence with every other, n - 1 queries
	// per subject: src/dist_hack.h:59-68)
	C.groups.push_back({0, n, 0, n, M, true, n - 1, {}, {}});
	C.pairs_total = n * n - n;
	C.allow_rccl = true;
	return run_seam(C, n, errbuf, errlen);
}

int andi_hip_dist_rect(andi_hip_model *MRQ, andi_hip_model *MQR, const andi_hip_seq *refs, size_t nr,
					   const andi_hip_seq *queries, size_t nq, const andi_hip_opts *opts_in, char *errbuf, size_t errlen) {
	if (!MRQ || !MQR || !refs || !queries || nr == 0 || nq == 0) {
		set_err(errbuf, errlen, "andi_hip_dist_rect: bad arguments");
		return 1;
	}
	if (!check_seqs(refs, nr, "reference", errbuf, errlen) || !check_seqs(queries, nq, "query", errbuf, errlen)) return 1;
	SeamCall C;
	C.name = "andi_hip_dist_rect";
	if (opts_in) {
		C.o = *opts_in;
	} else {
		andi_hip_default_opts(&C.o);
	}
	// the staged set is refs ++ queries (what the square call over that set would stage); its two cross blocks are two groups
	std::vector<andi_hip_seq> all(refs, refs + nr);
	all.insert(all.end(), queries, queries + nq);
	C.seqs = all.data(), C.n = nr + nq;
	C.groups.push_back({0, nr, nr, nq, MRQ, false, nq, {}, {}});  // references against the queries
	C.groups.push_back({nr, nq, 0, nr, MQR, false, nr, {}, {}});  // queries against the references
	C.pairs_total = 2 * nr * nq;
	C.allow_rccl = false; // (rows go to MRQ and MQR directly)
	return run_seam(C, std::max(nr, nq), errbuf, errlen);
}

} // extern "C"
