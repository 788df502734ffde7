// sketch.hip — k-mer sketches of sequences on the device and the shared-hash counts of every pair of two sketch sets
// (andi_hip_sketch, andi_hip_sketch_shared, andi_hip_screen; include/andi_hip.h states the contract, tests/sketch_model.py
// restates it in NumPy).  Everything is an integer: a sketch is the ascending set of the hashes fmix64(min(f, r)) of a
// sequence's windows that are <= UINT64_MAX / scale.
//
// The sequences are taken in batches of bounded packed bytes (SKETCH_BATCH_BYTES; test hook ANDI_SKETCH_BATCH): a batch
// is packed on the host to 4-bit symbols, one sequence behind the other without a gap -- so a sequence starts on an odd
// nibble where the lengths before it sum to an odd number --, through two pinned buffers (the host packs the next batch
// while the device hashes this one).  Only the sketches stay on the device.  Per batch:
//   k_hash<false>  one thread per run of P = 64 window END positions of one sequence.  It warms up on the k - 1 symbols
//                  before its run, then rolls f, r and the number of valid symbols since the last non-ACGT one; a window
//                  survives iff its hash is <= the threshold.  The thread leaves its count; a wavefront whose lanes all
//                  work on one sequence adds once to that sequence's counter, a mixed one per lane;
//   (host)         the counters give every sequence its slice, sized exactly;
//   k_hash<true>   the same walk again: a wavefront takes its room in the slice with one add (the lanes' places by a
//                  prefix sum of the counts the first pass left) and the survivors are written.  The order inside a
//                  slice depends on which wavefront came first; the sort makes the result deterministic;
//   sort           rocPRIM's segmented radix sort over the slices; a slice of more than SORT_WHOLE hashes (one block per
//                  segment would crawl there) by a device-wide radix sort of its own;
//   unique         k_flags marks the first of every run of equal hashes of a slice, an exclusive scan gives the places,
//                  k_compact writes the batch's sketches into a buffer of exactly their size, k_sizes the sizes.
// k_shared: a block stages one sketch of A in LDS (as much LDS as the longest staged sketch of the call needs, at most
// SKETCH_LDS_MAX hashes; test hook ANDI_SKETCH_LDS), each of its wavefronts takes sketches of B in turn, the lanes stride
// over that sketch's hashes and binary-search the staged one; one wave reduction, one store per pair.  A sketch of A longer
// than the limit is searched where it lies, in global memory, by the same code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include <rocprim/rocprim.hpp> // (behind <cstring>: one of its headers calls memset unqualified)

#include "api_internal.h"

namespace {

constexpr uint32_t P = 64;                               // k_hash: window end positions of a thread
constexpr uint32_t HASH_BLOCK = 256;                     //         threads of a block: a block spans 16384 positions
constexpr size_t SKETCH_BATCH_BYTES = (size_t)64 << 20;  // packed bytes of a batch (one sequence always fits)
constexpr size_t SORT_WHOLE = (size_t)1 << 16;           // a slice longer than this is sorted by a device-wide sort
constexpr uint32_t SKETCH_LDS_MAX = 20000;               // hashes of a staged sketch, at most (160 000 of a CU's 163 840 bytes)
constexpr uint32_t SHARED_BLOCK = 256;                   // k_shared: four wavefronts
constexpr uint32_t SHARED_GROUPS = 64;                   //           blocks per sketch of A, at most

__device__ inline uint64_t fmix64(uint64_t h) {
	h ^= h >> 33;
	h *= 0xff51afd7ed558ccdull;
	h ^= h >> 33;
	h *= 0xc4ceb9fe1a85ec53ull;
	h ^= h >> 33;
	return h;
}

// What a batch's kernels share.  Sequence s of the batch: nibbles off[s] ... off[s] + len[s] of text; its threads are
// first[s] ... first[s + 1) (first has nseq + 1 entries).
struct BatchDev {
	const uint64_t *text; // 16 symbols a word, the first in the lowest nibble; one word of padding behind the last symbol
	const uint64_t *off;
	const uint32_t *len;
	const uint32_t *first;
	uint32_t nseq, threads;
};

// FILL false: tcnt[t] = survivors of thread t, count[s] += them.  FILL true: the survivors go to out + start[s], places
// taken from cursor[s].
template <bool FILL>
__global__ __launch_bounds__(HASH_BLOCK) void k_hash(BatchDev B, int k, uint64_t mask, uint64_t thresh, uint32_t *__restrict__ tcnt,
													 uint32_t *__restrict__ count, const uint64_t *__restrict__ start,
													 uint32_t *__restrict__ cursor, uint64_t *__restrict__ out) {
	const uint32_t t = blockIdx.x * HASH_BLOCK + threadIdx.x;
	const bool live = t < B.threads;
	uint32_t s = 0xFFFFFFFFu;
	uint32_t lo = 0, hi = 0, from = 0;
	uint64_t g = 0;
	if (live) {
		uint32_t a = 0, b = B.nseq; // the last s with first[s] <= t (sequences without a thread share their successor's first)
		while (b - a > 1) {
			const uint32_t m = a + (b - a) / 2;
			if (B.first[m] <= t) a = m;
			else b = m;
		}
		s = a;
		const uint32_t len = B.len[s];
		lo = (t - B.first[s]) * P;
		hi = len - lo < P ? len : lo + P;
		from = lo >= (uint32_t)(k - 1) ? lo - (uint32_t)(k - 1) : 0;
		g = B.off[s] + from;
	}
	uint32_t n = 0;
	uint64_t *dst = nullptr;
	if (FILL) {
		// the lanes' places: an exclusive prefix sum of their counts over the wavefront, its total taken with one add
		const uint32_t mine = live ? tcnt[t] : 0;
		uint32_t incl = mine;
		const uint32_t lane = threadIdx.x & 63;
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t o = __shfl_up(incl, d);
			if (lane >= (uint32_t)d) incl += o;
		}
		const uint32_t s0 = __shfl(s, 0);
		const bool uniform = __all(s == s0);
		uint32_t base = 0;
		if (uniform) {
			const uint32_t total = __shfl(incl, 63);
			if (lane == 0 && total) base = atomicAdd(&cursor[s], total);
			base = __shfl(base, 0) + (incl - mine);
		} else if (mine) {
			base = atomicAdd(&cursor[s], mine);
		}
		if (live) dst = out + start[s] + base;
		if (!mine) return; // (nothing to write: no walk)
	}
	if (live) {
		uint64_t f = 0, r = 0, w = B.text[g >> 4] >> ((g & 15) * 4);
		uint32_t valid = 0;
		const int top = 2 * (k - 1);
		for (uint32_t p = from; p < hi; ++p) {
			const uint32_t sym = (uint32_t)w & 15u;
			w >>= 4;
			if ((++g & 15) == 0) w = B.text[g >> 4]; // (behind the last symbol: the padding word)
			if (sym < 4) {
				f = ((f << 2) | sym) & mask;
				r = (r >> 2) | ((uint64_t)(3u - sym) << top);
				++valid;
			} else {
				valid = 0;
			}
			if (p >= lo && valid >= (uint32_t)k) {
				const uint64_t h = fmix64(f < r ? f : r);
				if (h <= thresh) {
					if (FILL) dst[n] = h;
					++n;
				}
			}
		}
	}
	if (!FILL) {
		if (live) tcnt[t] = n;
		const uint32_t s0 = __shfl(s, 0);
		if (__all(s == s0)) {
			uint32_t total = n;
			for (int m = 32; m > 0; m >>= 1) total += __shfl_xor(total, m);
			if ((threadIdx.x & 63) == 0 && total && live) atomicAdd(&count[s], total);
		} else if (n) {
			atomicAdd(&count[s], n);
		}
	}
}

// flag[i] = hash i is the first of its value in its slice; flag[items] = 0 (the scan's last place is the total).
// head[i] is 1 where a slice starts.
__global__ __launch_bounds__(256) void k_flags(const uint64_t *__restrict__ key, const uint8_t *__restrict__ head, size_t items,
												 uint32_t *__restrict__ flag) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i > items) return;
	flag[i] = i == items ? 0u : (i == 0 || head[i] || key[i] != key[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_heads(const uint64_t *__restrict__ start, uint32_t nseq, size_t items, uint8_t *__restrict__ head) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s < nseq && start[s] < items) head[start[s]] = 1; // (an empty slice marks its successor's start: harmless)
}
__global__ __launch_bounds__(256) void k_compact(const uint64_t *__restrict__ key, const uint32_t *__restrict__ flag,
												   const uint32_t *__restrict__ pos, size_t items, uint64_t *__restrict__ out) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i < items && flag[i]) out[pos[i]] = key[i];
}
// start has nseq + 1 entries; pos items + 1.  where[s] = the place of sequence s's sketch in the batch's buffer.
__global__ __launch_bounds__(256) void k_sizes(const uint64_t *__restrict__ start, const uint32_t *__restrict__ pos, uint32_t nseq,
												 uint32_t *__restrict__ size, uint32_t *__restrict__ where) {
	const uint32_t s = blockIdx.x * 256 + threadIdx.x;
	if (s >= nseq) return;
	const uint32_t a = pos[start[s]], b = pos[start[s + 1]];
	size[s] = b - a, where[s] = a;
}

// shared[a * nb + b] for the sketches a of A from a0 on (the grid's rows) and every b of B.  Block (group, a): its
// wavefronts take the sketches b = 4 * group + wave, + 4 * groups, ...  lds_cap: the hashes the launch's LDS holds.
__global__ __launch_bounds__(SHARED_BLOCK) void k_shared(const uint64_t *const *__restrict__ Ah, const uint32_t *__restrict__ An,
														 const uint64_t *const *__restrict__ Bh, const uint32_t *__restrict__ Bn,
														 uint32_t a0, uint32_t nb, uint32_t groups, uint32_t lds_cap,
														 uint32_t *__restrict__ shared) {
	extern __shared__ uint64_t staged[];
	const uint32_t a = a0 + blockIdx.x / groups, group = blockIdx.x % groups;
	const uint32_t na = An[a];
	const uint64_t *A = Ah[a];
	if (na <= lds_cap) { // (the whole block: one sketch)
		for (uint32_t i = threadIdx.x; i < na; i += SHARED_BLOCK) staged[i] = A[i];
		__syncthreads();
		A = staged;
	}
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t b = group * 4 + wave; b < nb; b += groups * 4) {
		const uint32_t n = Bn[b];
		const uint64_t *Bk = Bh[b];
		uint32_t hits = 0;
		if (na)
			for (uint32_t j = lane; j < n; j += 64) {
				const uint64_t x = Bk[j];
				uint32_t lo = 0, hi = na; // the first place of A with a hash >= x
				while (lo < hi) {
					const uint32_t m = lo + (hi - lo) / 2;
					if (A[m] < x) lo = m + 1;
					else hi = m;
				}
				hits += lo < na && A[lo] == x;
			}
		for (int m = 32; m > 0; m >>= 1) hits += __shfl_xor(hits, m);
		if (lane == 0) shared[(size_t)a * nb + b] = hits;
	}
}

size_t knob_size(AndiKnob k, size_t dflt) {
	if (const char *v = andi_knob(k))
		if (atoll(v) >= 1) return (size_t)atoll(v);
	return dflt;
}

int fail_bytes(andi_hip_ctx *ctx, const char *what, size_t bytes, hipError_t e) {
	char msg[240];
	snprintf(msg, sizeof msg, "andi_hip_sketch: %s needs %zu bytes of device memory: %s", what, bytes, hipGetErrorString(e));
	(void)hipGetLastError();
	ctx->err = msg;
	return 1;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The 4-bit symbols of the batch's sequences [first, last) into dst, one behind the other: sequence i from nibble
// off[i - first] on.  A byte two sequences share is written by the later one (it reads its neighbour's last character),
// so the sequences are packed side by side by several threads.  Returns 1 if a byte lies outside the alphabet.
int pack_batch(const andi_hip_seq *seqs, size_t first, size_t last, const std::vector<uint64_t> &off, uint8_t *dst, size_t dst_bytes) {
	std::atomic<size_t> next{first};
	std::atomic<int> foreign{0};
	const uint64_t end_nib = off[last - first - 1] + seqs[last - 1].len;
	auto work = [&]() {
		std::vector<uint8_t> tmp;
		for (;;) {
			const size_t i = next.fetch_add(1);
			if (i >= last) return;
			const size_t len = seqs[i].len;
			if (len == 0) continue;
			const unsigned char *src = (const unsigned char *)seqs[i].seq;
			const uint64_t o = off[i - first], e = o + len;
			// the last byte is the next sequence's to write if that one starts in it
			const bool shares_end = (e & 1) && e < end_nib;
			if (!(o & 1)) {
				const size_t body = shares_end ? len - 1 : len;
				if (body && andi_hip_pack_symbols(src, body, dst + o / 2)) foreign.store(1);
				if (shares_end) { // (only the flag: the byte is the neighbour's)
					unsigned char one[1];
					if (andi_hip_pack_symbols(src + len - 1, 1, one)) foreign.store(1);
				}
			} else {
				// the byte shared with whatever lies before: that sequence's last symbol (the nearest non-empty one)
				size_t p = i;
				while (p > first && seqs[p - 1].len == 0) --p;
				unsigned char prev[1] = {0}, mine[1];
				if (p > first) (void)andi_hip_pack_symbols((const unsigned char *)seqs[p - 1].seq + seqs[p - 1].len - 1, 1, prev);
				if (andi_hip_pack_symbols(src, 1, mine)) foreign.store(1);
				dst[o / 2] = (uint8_t)((prev[0] & 15u) | ((mine[0] & 15u) << 4));
				const size_t rest = len - 1, body = shares_end ? rest - 1 : rest; // (from an even nibble on)
				if (body && andi_hip_pack_symbols(src + 1, body, dst + o / 2 + 1)) foreign.store(1);
				if (shares_end && rest) {
					unsigned char one[1];
					if (andi_hip_pack_symbols(src + len - 1, 1, one)) foreign.store(1);
				}
			}
		}
	};
	const size_t nseq = last - first;
	const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nseq, 16), std::max(1u, std::thread::hardware_concurrency())));
	std::vector<std::thread> ts;
	for (unsigned t = 1; t < nt; ++t) ts.emplace_back(work);
	work();
	for (auto &t : ts) t.join();
	// behind the last symbol: NUL symbols up to the buffer's end (the padding word the kernel may read)
	const size_t used = (size_t)((end_nib + 1) / 2);
	if (end_nib & 1) dst[used - 1] = (uint8_t)((dst[used - 1] & 15u) | 0x70u);
	memset(dst + used, 0x77, dst_bytes - used);
	return foreign.load();
}

} // namespace

struct andi_hip_sketches {
	int device = 0, k = 0;
	uint64_t scale = 0;
	size_t n = 0;
	std::vector<uint64_t *> buffers;   // one per batch that has hashes: its sketches one behind the other
	std::vector<const uint64_t *> ptr; // host copies of d_ptr, d_size
	std::vector<uint32_t> size;
	const uint64_t **d_ptr = nullptr;
	uint32_t *d_size = nullptr;
	double ms[4] = {0, 0, 0, 0}; // packing on the host, uploads, the hash kernel's two passes, sort and unique
};

extern "C" void andi_hip_sketch_free(andi_hip_ctx *ctx, andi_hip_sketches *s) {
	if (!s) return;
	if (ctx) (void)hipSetDevice(ctx->device), (void)hipStreamSynchronize(ctx->stream);
	for (uint64_t *b : s->buffers) (void)andi_arena::dev_free(b, false);
	if (s->d_ptr) (void)andi_arena::dev_free((void *)s->d_ptr, false);
	if (s->d_size) (void)andi_arena::dev_free(s->d_size, false);
	delete s;
}

extern "C" size_t andi_hip_sketch_count(const andi_hip_sketches *s) { return s ? s->n : 0; }

extern "C" int andi_hip_sketch_sizes(andi_hip_ctx *ctx, const andi_hip_sketches *s, uint32_t *sizes) {
	if (!ctx || !s || !sizes) {
		if (ctx) ctx->err = "andi_hip_sketch_sizes: bad arguments (ctx, the sketches and sizes must be given)";
		return 1;
	}
	memcpy(sizes, s->size.data(), s->n * sizeof(uint32_t));
	return 0;
}

extern "C" int andi_hip_sketch_timings(const andi_hip_sketches *s, double *ms4) {
	if (!s || !ms4) return 1;
	memcpy(ms4, s->ms, sizeof s->ms);
	return 0;
}

extern "C" int andi_hip_sketch_download(andi_hip_ctx *ctx, const andi_hip_sketches *s, size_t idx, uint64_t *hashes) {
	if (!ctx || !s || idx >= s->n || (!hashes && s->size[idx])) {
		if (ctx) ctx->err = "andi_hip_sketch_download: bad arguments (ctx, the sketches and hashes must be given, idx below the count)";
		return 1;
	}
	if (!s->size[idx]) return 0;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(hashes, s->ptr[idx], (size_t)s->size[idx] * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return 0;
}

extern "C" int andi_hip_sketch(andi_hip_ctx *ctx, const andi_hip_seq *seqs, size_t n, int k, uint64_t scale, andi_hip_sketches **out) {
	if (!ctx || !seqs || !out || n == 0 || n >= (size_t)UINT32_MAX || k < 4 || k > 32 || scale == 0) {
		if (ctx) ctx->err = "andi_hip_sketch: bad arguments (ctx, seqs and out must be given, n >= 1, 4 <= k <= 32, scale >= 1)";
		return 1;
	}
	for (size_t i = 0; i < n; ++i)
		if ((!seqs[i].seq && seqs[i].len) || seqs[i].len > (size_t)(INT32_MAX - 1) / 2) {
			ctx->err = "andi_hip_sketch: a sequence without text or an oversized one";
			return 1;
		}
	*out = nullptr;
	const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1, thresh = UINT64_MAX / scale;
	const size_t batch_bytes = knob_size(KNOB_SKETCH_BATCH, SKETCH_BATCH_BYTES);

	// the batches: consecutive sequences, as many as batch_bytes hold packed, at least one
	std::vector<size_t> cut{0};
	size_t cap_nib = 0, cap_seq = 0, cap_threads = 0;
	for (size_t i = 0; i < n;) {
		size_t nib = 0, j = i, threads = 0;
		while (j < n && (j == i || (nib + seqs[j].len + 1) / 2 <= batch_bytes)) nib += seqs[j].len, threads += (seqs[j].len + P - 1) / P, ++j;
		cap_nib = std::max(cap_nib, nib), cap_seq = std::max(cap_seq, j - i), cap_threads = std::max(cap_threads, threads);
		cut.push_back(j), i = j;
	}
	if (cap_threads >= (size_t)UINT32_MAX) { // (a batch of more than 2^38 symbols: only a hook could ask for it)
		ctx->err = "andi_hip_sketch: a batch of that many symbols is not supported";
		return 1;
	}
	const size_t text_bytes = ((cap_nib + 1) / 2 + 7) / 8 * 8 + 16;

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	auto *S = new andi_hip_sketches;
	S->device = ctx->device, S->k = k, S->scale = scale, S->n = n;
	S->ptr.assign(n, nullptr), S->size.assign(n, 0);
	struct Pinned {
		void *p[2] = {nullptr, nullptr};
		size_t bytes = 0;
		~Pinned() {
			for (void *q : p) host_pool::pinned_put(q, bytes);
		}
	} pin;
	pin.bytes = text_bytes;
	int rc = 0;
	{
		DevScope dev(st);
		uint64_t *text = nullptr, *d_off = nullptr, *d_start = nullptr;
		uint32_t *d_len = nullptr, *d_first = nullptr, *d_count = nullptr, *d_cursor = nullptr, *tcnt = nullptr, *d_size = nullptr, *d_where = nullptr;
		dev.alloc(&text, text_bytes / 8), dev.alloc(&d_off, cap_seq), dev.alloc(&d_len, cap_seq), dev.alloc(&d_first, cap_seq + 1);
		dev.alloc(&d_count, cap_seq), dev.alloc(&d_cursor, cap_seq), dev.alloc(&d_start, cap_seq + 1), dev.alloc(&tcnt, cap_threads ? cap_threads : 1);
		dev.alloc(&d_size, cap_seq), dev.alloc(&d_where, cap_seq);
		hipError_t e = dev.err;
		if (e != hipSuccess) rc = fail_bytes(ctx, "a batch's text and counters", text_bytes + cap_seq * 40 + cap_threads * 4, e);
		if (!rc && (host_pool::pinned_get(&pin.p[0], text_bytes) != hipSuccess || host_pool::pinned_get(&pin.p[1], text_bytes) != hipSuccess)) {
			(void)hipGetLastError();
			ctx->err = "andi_hip_sketch: no pinned host memory for the upload buffers";
			rc = 1;
		}
		hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
		for (auto &x : ev)
			if (!rc && hipEventCreate(&x) != hipSuccess) rc = fail(ctx, "andi_hip_sketch: hipEventCreate", hipGetLastError());

		const size_t nbatch = cut.size() - 1;
		std::vector<std::vector<uint64_t>> offs(2);
		auto pack = [&](size_t b) -> int { // batch b into pinned buffer b & 1
			const auto t0 = std::chrono::steady_clock::now();
			std::vector<uint64_t> &off = offs[b & 1];
			off.clear();
			uint64_t nib = 0;
			for (size_t i = cut[b]; i < cut[b + 1]; ++i) off.push_back(nib), nib += seqs[i].len;
			const int foreign = pack_batch(seqs, cut[b], cut[b + 1], off, (uint8_t *)pin.p[b & 1], text_bytes);
			S->ms[0] += ms_since(t0);
			return foreign;
		};
		int foreign = rc ? 0 : pack(0);
		std::vector<uint32_t> len, first, count;
		std::vector<uint64_t> start;
		for (size_t b = 0; !rc && b < nbatch; ++b) {
			if (foreign) {
				ctx->err = "andi_hip_sketch: the sequences hold a byte outside the alphabet A C G T !";
				rc = 1;
				break;
			}
			const size_t s0 = cut[b], nseq = cut[b + 1] - s0;
			const std::vector<uint64_t> &off = offs[b & 1];
			len.resize(nseq), first.resize(nseq + 1);
			uint64_t threads = 0, nib = 0;
			for (size_t i = 0; i < nseq; ++i) first[i] = (uint32_t)threads, len[i] = (uint32_t)seqs[s0 + i].len, threads += (len[i] + P - 1) / P, nib += len[i];
			first[nseq] = (uint32_t)threads;
			const size_t up = ((size_t)((nib + 1) / 2) + 7) / 8 * 8 + 16; // (with the padding word; within text_bytes)
			BatchDev B{text, d_off, d_len, d_first, (uint32_t)nseq, (uint32_t)threads};
			const unsigned blocks = (unsigned)((threads + HASH_BLOCK - 1) / HASH_BLOCK);
			// (the small copies first: they come from pageable memory, and the host waits in them for what the stream holds)
			e = hipMemcpyAsync(d_off, off.data(), nseq * sizeof(uint64_t), hipMemcpyHostToDevice, st);
			if (e == hipSuccess) e = hipMemcpyAsync(d_len, len.data(), nseq * sizeof(uint32_t), hipMemcpyHostToDevice, st);
			if (e == hipSuccess) e = hipMemcpyAsync(d_first, first.data(), (nseq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st);
			if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, nseq * sizeof(uint32_t), st);
			if (e == hipSuccess) e = hipMemsetAsync(d_cursor, 0, nseq * sizeof(uint32_t), st);
			if (e == hipSuccess) e = hipEventRecord(ev[0], st);
			if (e == hipSuccess) e = hipMemcpyAsync(text, pin.p[b & 1], up, hipMemcpyHostToDevice, st);
			if (e == hipSuccess) e = hipEventRecord(ev[1], st);
			if (e == hipSuccess && blocks) {
				k_hash<false><<<blocks, HASH_BLOCK, 0, st>>>(B, k, mask, thresh, tcnt, d_count, nullptr, nullptr, nullptr);
				e = hipGetLastError();
			}
			if (e == hipSuccess) e = hipEventRecord(ev[2], st);
			if (e != hipSuccess) break;
			if (b + 1 < nbatch) foreign = pack(b + 1); // (beside this batch's upload and first pass: nothing above waits for them)
			count.resize(nseq);
			e = hipMemcpyAsync(count.data(), d_count, nseq * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipStreamSynchronize(st);
			if (e != hipSuccess) break;
			start.resize(nseq + 1);
			size_t items = 0;
			for (size_t i = 0; i < nseq; ++i) start[i] = items, items += count[i];
			start[nseq] = items;
			float up_ms = 0, h1_ms = 0, h2_ms = 0;
			(void)hipEventElapsedTime(&up_ms, ev[0], ev[1]), (void)hipEventElapsedTime(&h1_ms, ev[1], ev[2]);
			S->ms[1] += up_ms, S->ms[2] += h1_ms;
			if (items == 0) continue; // (every sketch of the batch is empty)
			if (items >= (size_t)UINT32_MAX) {
				ctx->err = "andi_hip_sketch: a batch with 2^32 hashes or more; sketch it in smaller batches or at a larger scale";
				rc = 1;
				break;
			}
			// ---- the second pass, the sort, the unique: buffers of this batch only
			std::vector<uint32_t> hb, he; // the slices the segmented sort takes
			std::vector<size_t> whole;    // ... and those sorted one by one
			std::vector<uint32_t> where(nseq);
			uint32_t total = 0;
			DevScope bs(st); // (after what the copies in flight read and write: its end waits for the stream)
			uint64_t *keyA = nullptr, *keyB = nullptr;
			uint32_t *flag = nullptr, *pos = nullptr, *seg_b = nullptr, *seg_e = nullptr;
			uint8_t *head = nullptr;
			void *tmp = nullptr;
			for (size_t i = 0; i < nseq; ++i) {
				if (count[i] > SORT_WHOLE) whole.push_back(i);
				else if (count[i] > 1) hb.push_back((uint32_t)start[i]), he.push_back((uint32_t)start[i + 1]);
			}
			size_t max_whole = 0;
			for (size_t i : whole) max_whole = std::max<size_t>(max_whole, count[i]);
			size_t tb_seg = 0, tb_whole = 0, tb_scan = 0;
			if (!hb.empty())
				e = rocprim::segmented_radix_sort_keys(nullptr, tb_seg, keyA, keyB, (unsigned)items, (unsigned)hb.size(), seg_b, seg_e, 0, 64, st);
			if (e == hipSuccess && max_whole) e = rocprim::radix_sort_keys(nullptr, tb_whole, keyA, keyB, max_whole, 0, 64, st);
			if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb_scan, flag, pos, 0u, items + 1, rocprim::plus<uint32_t>(), st);
			if (e != hipSuccess) break;
			const size_t tmp_bytes = std::max(std::max(tb_seg, tb_whole), std::max(tb_scan, (size_t)16));
			bs.alloc(&keyA, items), bs.alloc(&keyB, items), bs.alloc(&flag, items + 1), bs.alloc(&pos, items + 1), bs.alloc(&head, items);
			bs.alloc(&seg_b, hb.size() + 1), bs.alloc(&seg_e, hb.size() + 1);
			bs.alloc((uint8_t **)&tmp, tmp_bytes);
			if (bs.err != hipSuccess) {
				rc = fail_bytes(ctx, "a batch's hashes", items * 25 + tmp_bytes, bs.err);
				break;
			}
			e = hipMemcpyAsync(d_start, start.data(), (nseq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st);
			if (e == hipSuccess) e = hipEventRecord(ev[2], st);
			if (e == hipSuccess) {
				k_hash<true><<<blocks, HASH_BLOCK, 0, st>>>(B, k, mask, thresh, tcnt, nullptr, d_start, d_cursor, keyA);
				e = hipGetLastError();
			}
			if (e == hipSuccess) e = hipEventRecord(ev[3], st);
			const auto t_sort = std::chrono::steady_clock::now();
			// slices of one hash and none stay where they are: the sorts write keyB, so start from a copy
			if (e == hipSuccess) e = hipMemcpyAsync(keyB, keyA, items * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
			if (e == hipSuccess && !hb.empty()) {
				e = hipMemcpyAsync(seg_b, hb.data(), hb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
				if (e == hipSuccess) e = hipMemcpyAsync(seg_e, he.data(), he.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
				size_t tb = tmp_bytes;
				if (e == hipSuccess)
					e = rocprim::segmented_radix_sort_keys(tmp, tb, keyA, keyB, (unsigned)items, (unsigned)hb.size(), seg_b, seg_e, 0, 64, st);
			}
			for (size_t i : whole) {
				size_t tb = tmp_bytes;
				if (e == hipSuccess) e = rocprim::radix_sort_keys(tmp, tb, keyA + start[i], keyB + start[i], (size_t)count[i], 0, 64, st);
			}
			if (e == hipSuccess) e = hipMemsetAsync(head, 0, items, st);
			if (e == hipSuccess) {
				k_heads<<<(unsigned)((nseq + 255) / 256), 256, 0, st>>>(d_start, (uint32_t)nseq, items, head);
				k_flags<<<(unsigned)((items + 1 + 255) / 256), 256, 0, st>>>(keyB, head, items, flag);
				e = hipGetLastError();
			}
			size_t tb = tmp_bytes;
			if (e == hipSuccess) e = rocprim::exclusive_scan(tmp, tb, flag, pos, 0u, items + 1, rocprim::plus<uint32_t>(), st);
			if (e == hipSuccess) e = hipMemcpyAsync(&total, pos + items, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipStreamSynchronize(st);
			if (e != hipSuccess) break;
			uint64_t *sk = nullptr;
			if ((e = dmalloc(&sk, total)) != hipSuccess) {
				rc = fail_bytes(ctx, "a batch's sketches", (size_t)total * 8, e);
				break;
			}
			S->buffers.push_back(sk);
			k_compact<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(keyB, flag, pos, items, sk);
			k_sizes<<<(unsigned)((nseq + 255) / 256), 256, 0, st>>>(d_start, pos, (uint32_t)nseq, d_size, d_where);
			e = hipGetLastError();
			if (e == hipSuccess) e = hipMemcpyAsync(&S->size[s0], d_size, nseq * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipMemcpyAsync(where.data(), d_where, nseq * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipStreamSynchronize(st);
			if (e != hipSuccess) break;
			for (size_t i = 0; i < nseq; ++i) S->ptr[s0 + i] = sk + where[i];
			(void)hipEventElapsedTime(&h2_ms, ev[2], ev[3]);
			S->ms[2] += h2_ms, S->ms[3] += ms_since(t_sort);
		}
		if (!rc && e != hipSuccess) rc = fail(ctx, "andi_hip_sketch", e);
		for (auto &x : ev)
			if (x) (void)hipEventDestroy(x);
	}
	if (!rc) {
		hipError_t e = dmalloc((uint64_t ***)&S->d_ptr, n);
		if (e == hipSuccess) e = dmalloc(&S->d_size, n);
		if (e == hipSuccess) e = hipMemcpyAsync((void *)S->d_ptr, S->ptr.data(), n * sizeof(uint64_t *), hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(S->d_size, S->size.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) rc = fail(ctx, "andi_hip_sketch: the table of the sketches", e);
	}
	if (rc) {
		andi_hip_sketch_free(ctx, S);
		return 1;
	}
	*out = S;
	return 0;
}

extern "C" int andi_hip_sketch_shared(andi_hip_ctx *ctx, const andi_hip_sketches *a, const andi_hip_sketches *b, uint32_t *shared) {
	if (!ctx || !a || !b || !shared) {
		if (ctx) ctx->err = "andi_hip_sketch_shared: bad arguments (ctx, both sketch sets and shared must be given)";
		return 1;
	}
	if (a->k != b->k || a->scale != b->scale || a->device != ctx->device || b->device != ctx->device) {
		char msg[240];
		snprintf(msg, sizeof msg, "andi_hip_sketch_shared: the sketch sets differ (k %d and %d, scale %llu and %llu) or are not this context's",
				 a->k, b->k, (unsigned long long)a->scale, (unsigned long long)b->scale);
		ctx->err = msg;
		return 1;
	}
	if (b->n >= (size_t)UINT32_MAX / 8 || a->n >= (size_t)UINT32_MAX / 8) {
		ctx->err = "andi_hip_sketch_shared: too many sketches";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const uint32_t lds_max = (uint32_t)std::min<size_t>(knob_size(KNOB_SKETCH_LDS, SKETCH_LDS_MAX), SKETCH_LDS_MAX);
	uint32_t lds_cap = 0; // the longest sketch of A that is staged
	for (uint32_t s : a->size)
		if (s <= lds_max && s > lds_cap) lds_cap = s;
	const size_t lds_bytes = (size_t)lds_cap * sizeof(uint64_t);
	if (lds_bytes > 65536)
		HIP_TRY(ctx, hipFuncSetAttribute((const void *)k_shared, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
	const uint32_t nb = (uint32_t)b->n;
	const uint32_t groups = std::min<uint32_t>(SHARED_GROUPS, (nb + 3) / 4);
	DevScope dev(st);
	uint32_t *d_shared = nullptr;
	dev.alloc(&d_shared, a->n * b->n);
	if (dev.err != hipSuccess) {
		char msg[200];
		snprintf(msg, sizeof msg, "andi_hip_sketch_shared: the counts need %zu bytes of device memory: %s", a->n * b->n * sizeof(uint32_t),
				 hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	const size_t rows_per_launch = std::max<size_t>(1, (size_t)0x7fffffff / groups);
	hipError_t e = hipSuccess;
	for (size_t a0 = 0; e == hipSuccess && a0 < a->n; a0 += rows_per_launch) {
		const size_t rows = std::min(rows_per_launch, a->n - a0);
		k_shared<<<(unsigned)(rows * groups), SHARED_BLOCK, lds_bytes, st>>>(a->d_ptr, a->d_size, b->d_ptr, b->d_size, (uint32_t)a0, nb, groups,
																			   lds_cap, d_shared);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(shared, d_shared, a->n * b->n * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_sketch_shared", e);
	return 0;
}

extern "C" int andi_hip_screen(const andi_hip_seq *refs, size_t nr, const andi_hip_seq *queries, size_t nq, int k, uint64_t scale, int device,
							   uint32_t *shared, uint32_t *ref_sizes, uint32_t *query_sizes, char *errbuf, size_t errlen) {
	if (!refs || !queries || !shared || nr == 0 || nq == 0 || k < 4 || k > 32 || scale == 0 || device < 0) {
		set_err(errbuf, errlen, "andi_hip_screen: bad arguments (refs, queries and shared must be given, nr and nq >= 1, 4 <= k <= 32, "
								"scale >= 1, device >= 0)");
		return 1;
	}
	andi_hip_ctx *ctx = nullptr;
	if (ctx_create(&ctx, device, errbuf, errlen, false)) return 1;
	andi_hip_sketches *R = nullptr, *Q = nullptr;
	int rc = andi_hip_sketch(ctx, refs, nr, k, scale, &R);
	if (!rc) rc = andi_hip_sketch(ctx, queries, nq, k, scale, &Q);
	if (!rc) rc = andi_hip_sketch_shared(ctx, Q, R, shared);
	if (!rc && ref_sizes) rc = andi_hip_sketch_sizes(ctx, R, ref_sizes);
	if (!rc && query_sizes) rc = andi_hip_sketch_sizes(ctx, Q, query_sizes);
	if (rc) set_err(errbuf, errlen, "%s", ctx->err.c_str());
	andi_hip_sketch_free(ctx, Q), andi_hip_sketch_free(ctx, R);
	andi_hip_ctx_destroy(ctx);
	return rc;
}
