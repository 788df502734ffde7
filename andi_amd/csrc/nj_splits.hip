// nj_splits.hip — every distinct bipartition among the trees of a bootstrap, with its frequency (andi_hip_nj_splits,
// include/andi_hip.h): what a majority-rule consensus tree is made of (host_model.c: andi_hip_consensus).
//
// The host's validation of the records, the replicates' groups and the kernels that build a tree's leaf sets (k_sets) and
// hash them on their canonical side (k_hash) are nj_sets.h's, shared with nj_support.hip and nj_transfer.hip.  This call's
// own: no point tree; with every replicate skipped it returns no split before any HIP call; a group is also no larger than
// hipcub counts (MAX_ITEMS sets); and a group's m = g x (n - 3) sets are hashed and then grouped EXACTLY:
//   k_keys    the sort keys: the hashes (cut to ANDI_SPLIT_HASH_BITS bits by the test hook) with the sets' indices as values;
//             a stable radix sort (hipcub) brings equal hashes together, indices ascending within a run of equal hashes;
//   k_heads   + an inclusive max scan: for every sorted position the start of its run;
//   k_class   one wavefront per position p: the earliest position of its run whose set has the same canonical words --
//             rep[p].  The run is walked from its start and all W words are compared, so sets that merely share a hash are
//             kept apart, also in the order A B A (the third finds the first past the second).  Without collisions the
//             first comparison ends the walk;
//   k_lookup  one wavefront per class (rep[p] == p): the table of the distinct splits found by the groups before this one
//             is searched -- a binary search in its sorted hashes, then the words of every entry of that hash;
//   k_append  the classes the table did not have are appended to it in the order of their earliest member's index: the
//             flags lie in (replicate, record) order and an exclusive sum over them gives the slot, so the table's order
//             is the order of first appearance and a slot IS the split's id;
//   k_count   every member: its id, and one more for its split's frequency (an integer atomic: the sum is exact);
//   k_bump    the table's length, kept on the device: no kernel waits for the host between the groups.
// The table is re-sorted by hash before each group's lookup (hipcub again; unused slots carry the largest key and are
// told apart by their slot number).  Its capacity is fixed before the first kernel: all sets of all used replicates, or as
// many as half of the free device memory holds.  Appends past it are counted but not written, and the call then fails by
// naming the bytes the table needed: it does not fault.  Two synchronisations, both at the end: one to learn the number
// of splits, one for the copies of that size.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nj_sets.h"

namespace {

constexpr size_t MAX_ITEMS = 0x7fffff00;        // hipcub counts with int
constexpr uint32_t NONE = 0xffffffffu;

__global__ __launch_bounds__(256) void k_keys(const uint64_t *__restrict__ hash, uint64_t mask, uint32_t m,
											  uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= m) return;
	keys[i] = hash[i] & mask;
	vals[i] = i;
}

__global__ __launch_bounds__(256) void k_iota(uint32_t m, uint32_t *__restrict__ vals) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < m) vals[i] = i;
}

// start[p] = p where a run of equal keys begins, else 0: the inclusive max scan turns it into the run's start
__global__ __launch_bounds__(256) void k_heads(const uint64_t *__restrict__ skeys, uint32_t m, uint32_t *__restrict__ start) {
	const uint32_t p = blockIdx.x * 256 + threadIdx.x;
	if (p >= m) return;
	start[p] = p > 0 && skeys[p] != skeys[p - 1] ? p : 0;
}

// whether two sets agree on all W canonical words; the whole wavefront calls it and gets one answer
__device__ inline bool wave_same(const uint64_t *a, bool aflip, const uint64_t *b, bool bflip, uint32_t n, uint32_t W,
								 uint32_t lane) {
	for (uint32_t base = 0; base < W; base += 64) {
		const uint32_t w = base + lane;
		const bool diff = w < W && canonical_word(a, n, W, w, aflip) != canonical_word(b, n, W, w, bflip);
		if (__any(diff)) return false;
	}
	return true;
}

// rep[p]: the earliest position q <= p of p's run of equal keys whose set equals that of p.  One wavefront per p.
__global__ __launch_bounds__(256) void k_class(const uint64_t *__restrict__ sets, const uint32_t *__restrict__ svals,
											   const uint32_t *__restrict__ start, uint32_t n, uint32_t W, uint32_t m,
											   uint32_t *__restrict__ rep) {
	const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (p >= m) return;
	const uint64_t *mine = sets + (size_t)svals[p] * W;
	const bool flip = mine[0] & 1;
	uint32_t q = start[p];
	for (; q < p; ++q) {
		const uint64_t *other = sets + (size_t)svals[q] * W;
		if (wave_same(mine, flip, other, other[0] & 1, n, W, lane)) break;
	}
	if (lane == 0) rep[p] = q;
}

// One wavefront per p.  A class (rep[p] == p) is looked up among the first min(*T, cap) slots of the table, through the
// table's hashes sorted (shash, with their slots sslot; cap entries, the unused ones with the largest key): pslot[p] = its
// slot, or NONE and isnew[its set's index] = 1.  Every other p: isnew[its set's index] = 0.
__global__ __launch_bounds__(256) void k_lookup(const uint64_t *__restrict__ sets, const uint64_t *__restrict__ skeys,
												const uint32_t *__restrict__ svals, const uint32_t *__restrict__ rep,
												uint32_t n, uint32_t W, uint32_t m, const uint64_t *__restrict__ tsets,
												const uint64_t *__restrict__ shash, const uint32_t *__restrict__ sslot,
												const unsigned long long *__restrict__ T, uint32_t cap,
												uint32_t *__restrict__ pslot, uint32_t *__restrict__ isnew) {
	const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (p >= m) return;
	const uint32_t idx = svals[p];
	if (rep[p] != p) {
		if (lane == 0) pslot[p] = NONE, isnew[idx] = 0;
		return;
	}
	const unsigned long long t = *T;
	const uint32_t have = t < cap ? (uint32_t)t : cap;
	const uint64_t key = skeys[p];
	const uint64_t *mine = sets + (size_t)idx * W;
	const bool flip = mine[0] & 1;
	uint32_t lo = 0, hi = have ? cap : 0; // the first sorted entry whose hash is not below the key
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (shash[mid] < key) lo = mid + 1;
		else hi = mid;
	}
	uint32_t found = NONE;
	for (uint32_t j = lo; have && j < cap && shash[j] == key; ++j) {
		const uint32_t slot = sslot[j];
		if (slot >= have) continue; // (an unused slot: its key is the largest there is, which a hash may be too)
		if (wave_same(mine, flip, tsets + (size_t)slot * W, false, n, W, lane)) {
			found = slot;
			break;
		}
	}
	if (lane == 0) pslot[p] = found, isnew[idx] = found == NONE;
}

// One wavefront per p.  A class the table did not have takes slot *T + newrank[its set's index] -- if the table has that
// many: its canonical words, its hash, pslot[p].  Past the capacity nothing is written (pslot[p] stays NONE).
__global__ __launch_bounds__(256) void k_append(const uint64_t *__restrict__ sets, const uint64_t *__restrict__ skeys,
												const uint32_t *__restrict__ svals, const uint32_t *__restrict__ rep,
												const uint32_t *__restrict__ isnew, const uint32_t *__restrict__ newrank,
												uint32_t n, uint32_t W, uint32_t m, uint64_t *__restrict__ tsets,
												uint64_t *__restrict__ thash, const unsigned long long *__restrict__ T,
												uint32_t cap, uint32_t *__restrict__ pslot) {
	const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (p >= m) return;
	const uint32_t idx = svals[p];
	if (rep[p] != p || !isnew[idx]) return;
	const unsigned long long slot = *T + newrank[idx];
	if (slot >= cap) return;
	const uint64_t *mine = sets + (size_t)idx * W;
	const bool flip = mine[0] & 1;
	uint64_t *to = tsets + (size_t)slot * W;
	for (uint32_t w = lane; w < W; w += 64) to[w] = canonical_word(mine, n, W, w, flip);
	if (lane == 0) thash[slot] = skeys[p], pslot[p] = (uint32_t)slot;
}

// One thread per p: the id of its set (slot[index in the group]) and one more for that split's frequency
__global__ __launch_bounds__(256) void k_count(const uint32_t *__restrict__ svals, const uint32_t *__restrict__ rep,
											   const uint32_t *__restrict__ pslot, uint32_t m, uint32_t *__restrict__ slot,
											   uint32_t *tfreq) {
	const uint32_t p = blockIdx.x * 256 + threadIdx.x;
	if (p >= m) return;
	const uint32_t id = pslot[rep[p]];
	slot[svals[p]] = id;
	if (id != NONE) atomicAdd(&tfreq[id], 1u);
}

__global__ void k_bump(const uint32_t *__restrict__ isnew, const uint32_t *__restrict__ newrank, uint32_t m,
					   unsigned long long *T) {
	*T += (unsigned long long)newrank[m - 1] + isnew[m - 1];
}

} // namespace

int andi_hip_nj_splits(andi_hip_ctx *ctx, const andi_hip_nj_join *reps, size_t n, size_t count, const uint8_t *skip,
					   uint32_t *ids, size_t *nsplits, uint32_t **freq, uint64_t **sets) {
	if (!ctx || !reps || !nsplits || !freq || !sets || count == 0 || n < 2 || n > 65535 || (n > 3 && !ids)) {
		if (ctx) ctx->err = "andi_hip_nj_splits: bad arguments (ctx, reps, ids, nsplits, freq and sets must be given, count >= 1, 2 <= n <= 65535)";
		return 1;
	}
	*nsplits = 0, *freq = nullptr, *sets = nullptr;
	if (n < 4) return 0; // (no branch that is not a leaf's)
	// a set costs, beside its words: its record's children, three 64-bit and eight 32-bit words of what sorts and classes it
	SetsPlan p;
	if (!sets_prepare(ctx, "andi_hip_nj_splits", nullptr, reps, n, count, skip,
					  sizeof(int2) + 3 * sizeof(uint64_t) + 8 * sizeof(uint32_t), p))
		return 1;
	const size_t nsets = p.nsets, W = p.W;
	const std::vector<size_t> &used = p.used;
	uint64_t mask = ~0ull;
	if (const char *v = andi_knob(KNOB_SPLIT_HASH_BITS)) { // test hook: only the low bits of the hash, so that sets collide
		const int b = atoi(v);
		if (b >= 0 && b < 64) mask = (1ull << b) - 1;
	}
	memset(ids, 0xff, count * nsets * sizeof *ids);
	if (used.empty()) return 0; // (every replicate skipped: no split)
	if (p.G * nsets > MAX_ITEMS) p.G = MAX_ITEMS / nsets;
	const size_t all = used.size() * nsets, M = p.G * nsets;

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, S = (uint32_t)nsets, Wd = (uint32_t)W;
	hipStream_t st = ctx->stream;
	// the group's buffers
	uint64_t *rsets = nullptr, *rhash = nullptr, *keys = nullptr, *skeys = nullptr;
	int2 *dkids = nullptr;
	uint32_t *vals = nullptr, *svals = nullptr, *start = nullptr, *run = nullptr, *rep = nullptr, *pslot = nullptr, *isnew = nullptr, *newrank = nullptr;
	// the table, and every set's slot
	uint64_t *tsets = nullptr, *thash = nullptr, *shash = nullptr;
	uint32_t *iota = nullptr, *sslot = nullptr, *tfreq = nullptr, *slot = nullptr;
	unsigned long long *dT = nullptr, hT = 0;
	uint8_t *tmp = nullptr;
	size_t cap = 0, tmp_bytes = 0;
	const size_t split_bytes = W * sizeof(uint64_t) + 2 * sizeof(uint64_t) + 3 * sizeof(uint32_t); // a slot of the table
	DevScope dev(st);
	dev.alloc(&dkids, M), dev.alloc(&rhash, M), dev.alloc(&keys, M), dev.alloc(&skeys, M);
	for (uint32_t **q : {&vals, &svals, &start, &run, &rep, &pslot, &isnew, &newrank}) dev.alloc(q, M);
	dev.alloc(&rsets, M * W), dev.alloc(&slot, all), dev.alloc(&dT, 1);
	hipError_t e = dev.err;
	if (e == hipSuccess) { // the table: room for every set, or for what half of the free memory holds (one tree's sets at least)
		size_t free_b = 0, total_b = 0;
		e = hipMemGetInfo(&free_b, &total_b);
		cap = free_b / 2 / split_bytes;
		cap = cap < nsets ? nsets : cap;
		cap = cap > all ? all : cap;
		cap = cap > MAX_ITEMS ? MAX_ITEMS : cap;
	}
	if (e == hipSuccess) {
		dev.alloc(&tsets, cap * W), dev.alloc(&thash, cap), dev.alloc(&shash, cap);
		dev.alloc(&iota, cap), dev.alloc(&sslot, cap), dev.alloc(&tfreq, cap);
		e = dev.err;
	}
	if (e == hipSuccess) { // hipcub's scratch, for the largest of its calls below
		size_t a = 0, b = 0, c = 0, d = 0;
		e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, keys, skeys, vals, svals, (int)M, 0, 64, st);
		if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, thash, shash, iota, sslot, (int)cap, 0, 64, st);
		if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveScan(nullptr, c, start, run, hipcub::Max(), (int)M, st);
		if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, d, isnew, newrank, (int)M, st);
		tmp_bytes = a > b ? a : b;
		tmp_bytes = tmp_bytes > c ? tmp_bytes : c;
		tmp_bytes = tmp_bytes > d ? tmp_bytes : d;
		if (e == hipSuccess) dev.alloc(&tmp, tmp_bytes ? tmp_bytes : 1), e = dev.err;
	}
	const uint32_t C = (uint32_t)cap;
	if (e == hipSuccess) e = hipMemsetAsync(dT, 0, sizeof *dT, st);
	if (e == hipSuccess) e = hipMemsetAsync(tfreq, 0, cap * sizeof *tfreq, st);
	if (e == hipSuccess) e = hipMemsetAsync(thash, 0xff, cap * sizeof *thash, st); // (unused slots sort behind every hash, or among the largest)
	if (e == hipSuccess) {
		k_iota<<<(C + 255) / 256, 256, 0, st>>>(C, iota);
		e = hipGetLastError();
	}
	if (e == hipSuccess)
		e = sets_for_groups(p, n, dkids, rsets, st, [&](size_t first, uint32_t g) {
			const uint32_t m = g * S;
			size_t tb = tmp_bytes;
			hipError_t le;
			k_hash<<<dim3((S + 3) / 4, g), 256, 0, st>>>(rsets, N, S, Wd, rhash);
			k_keys<<<(m + 255) / 256, 256, 0, st>>>(rhash, mask, m, keys, vals);
			if ((le = hipGetLastError()) != hipSuccess) return le;
			if ((le = hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, skeys, vals, svals, (int)m, 0, 64, st)) != hipSuccess) return le;
			k_heads<<<(m + 255) / 256, 256, 0, st>>>(skeys, m, start);
			tb = tmp_bytes;
			if ((le = hipcub::DeviceScan::InclusiveScan(tmp, tb, start, run, hipcub::Max(), (int)m, st)) != hipSuccess) return le;
			k_class<<<(m + 3) / 4, 256, 0, st>>>(rsets, svals, run, N, Wd, m, rep);
			tb = tmp_bytes;
			if ((le = hipcub::DeviceRadixSort::SortPairs(tmp, tb, thash, shash, iota, sslot, (int)C, 0, 64, st)) != hipSuccess) return le;
			k_lookup<<<(m + 3) / 4, 256, 0, st>>>(rsets, skeys, svals, rep, N, Wd, m, tsets, shash, sslot, dT, C, pslot, isnew);
			tb = tmp_bytes;
			if ((le = hipcub::DeviceScan::ExclusiveSum(tmp, tb, isnew, newrank, (int)m, st)) != hipSuccess) return le;
			k_append<<<(m + 3) / 4, 256, 0, st>>>(rsets, skeys, svals, rep, isnew, newrank, N, Wd, m, tsets, thash, dT, C, pslot);
			k_count<<<(m + 255) / 256, 256, 0, st>>>(svals, rep, pslot, m, slot + first * nsets, tfreq);
			k_bump<<<1, 1, 0, st>>>(isnew, newrank, m, dT);
			return hipGetLastError();
		});
	if (e == hipSuccess) e = hipMemcpyAsync(&hT, dT, sizeof hT, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	bool fits = true;
	uint32_t *hfreq = nullptr;
	uint64_t *hsets = nullptr;
	if (e == hipSuccess && hT > cap) fits = false;
	if (e == hipSuccess && fits) {
		hfreq = (uint32_t *)malloc(hT * sizeof *hfreq);
		hsets = (uint64_t *)malloc(hT * W * sizeof *hsets);
		if (!hfreq || !hsets) e = hipErrorOutOfMemory;
		if (e == hipSuccess) e = hipMemcpyAsync(hfreq, tfreq, hT * sizeof *hfreq, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(hsets, tsets, hT * W * sizeof *hsets, hipMemcpyDeviceToHost, st);
		for (size_t u = 0; e == hipSuccess && u < used.size();) { // the ids, a run of used replicates at a time
			size_t v = u + 1;
			while (v < used.size() && used[v] == used[v - 1] + 1) ++v;
			e = hipMemcpyAsync(ids + used[u] * nsets, slot + u * nsets, (v - u) * nsets * sizeof *ids, hipMemcpyDeviceToHost, st);
			u = v;
		}
		if (e == hipSuccess) e = hipStreamSynchronize(st);
	}
	if (e != hipSuccess || !fits) {
		(void)hipStreamSynchronize(st); // (an error exit: no copy in flight writes what is freed and reset here)
		free(hfreq), free(hsets);
		memset(ids, 0xff, count * nsets * sizeof *ids);
		if (e != hipSuccess) return fail(ctx, "andi_hip_nj_splits", e);
		char msg[256];
		snprintf(msg, sizeof msg,
				 "andi_hip_nj_splits: the table of distinct splits does not fit the device: up to %llu splits of %zu leaves need "
				 "%llu bytes, %zu splits (%zu bytes) had room",
				 hT, n, hT * (unsigned long long)split_bytes, cap, cap * split_bytes);
		ctx->err = msg;
		return 1;
	}
	*nsplits = (size_t)hT, *freq = hfreq, *sets = hsets;
	return 0;
}
