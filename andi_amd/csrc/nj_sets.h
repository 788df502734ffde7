// nj_sets.h — the leaf sets of neighbor-joining trees on the device, and the one driver of the three calls that work on
// the sets of a bootstrap's replicate trees: andi_hip_nj_support (nj_support.hip), andi_hip_nj_transfer (nj_transfer.hip)
// and andi_hip_nj_splits (nj_splits.hip).  Private; every translation unit that includes it gets its own copy of the
// kernels (they are small), but there is one source.
//
// A tree's leaf sets are bitsets of W = ceil(n / 64) words, set s below node n + s:
//   k_sets   one thread per (tree, word): it walks the records in order and ORs the word of the two children -- a leaf's
//            bit, or the word of an earlier record's set, which the SAME thread wrote (nothing crosses threads, so no
//            barrier and no recursion: a caterpillar 65535 deep is a loop of 65532 trips);
//   k_hash   one wavefront per set: a 64-bit hash of the set on its canonical side -- the side without leaf 0, so a set
//            that holds leaf 0 counts as its complement.  The sets in memory stay as built; the side is taken on the fly.
//
// The driver, in the order a call uses it:
//   sets_prepare     on the host, before any HIP call: the records are validated (records_ok: every child a leaf or an
//                    earlier record's node, every node a child exactly once) -- the point tree's first, if the call has
//                    one, then those of the replicates that skip leaves in, in ascending order -- and only the two
//                    children of every pair record are kept for the device; and the group's size is fixed: the used
//                    replicates are taken SETS_GROUP_BYTES of device memory at a time (nj_group_size, api_internal.h;
//                    one tree's sets are 537 MB at 65535 leaves, and one tree always fits);
//   sets_for_groups  per group: its children go up, k_sets builds its sets, and the call's own body launches what it
//                    does with them.  The groups follow one another on the context's stream; nothing waits for the host.
// What differs between the three calls stays in their files: the bytes a set costs beside its words, whether there is a
// point tree, the body, and what a call does when every replicate is skipped.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"

namespace {

// word w of the set of node v: a leaf's bit, or the word of an earlier record's set
__device__ inline uint64_t child_word(const uint64_t *sets, uint32_t n, uint32_t W, uint32_t w, int32_t v) {
	if ((uint32_t)v < n) return ((uint32_t)v >> 6) == w ? 1ull << (v & 63) : 0ull;
	return sets[(size_t)((uint32_t)v - n) * W + w];
}

// kids: per tree nsets pairs of children; sets: per tree nsets x W words.  Thread = (tree blockIdx.y, word).
__global__ __launch_bounds__(64) void k_sets(const int2 *__restrict__ kids, uint32_t n, uint32_t nsets, uint32_t W,
											 uint64_t *sets) {
	const uint32_t w = blockIdx.x * 64 + threadIdx.x;
	if (w >= W) return;
	kids += (size_t)blockIdx.y * nsets;
	sets += (size_t)blockIdx.y * nsets * W;
	for (uint32_t s = 0; s < nsets; ++s) {
		const int2 k = kids[s];
		sets[(size_t)s * W + w] = child_word(sets, n, W, w, k.x) | child_word(sets, n, W, w, k.y);
	}
}

// word w of a set on its canonical side: as it is without leaf 0, else its complement within the n leaves
__device__ inline uint64_t canonical_word(const uint64_t *set, uint32_t n, uint32_t W, uint32_t w, bool flip) {
	const uint64_t x = set[w];
	if (!flip) return x;
	const uint64_t mask = w + 1 == W && (n & 63) ? (1ull << (n & 63)) - 1 : ~0ull;
	return ~x & mask;
}

__device__ inline uint64_t mix(uint64_t x) { // (splitmix64's finaliser)
	x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27, x *= 0x94d049bb133111ebull;
	return x ^ (x >> 31);
}

// hash[tree][s]: the words of the canonical side, each mixed with its index, XORed.  One wavefront per set.
__global__ __launch_bounds__(256) void k_hash(const uint64_t *__restrict__ sets, uint32_t n, uint32_t nsets, uint32_t W,
											  uint64_t *__restrict__ hash) {
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (s >= nsets) return;
	const uint64_t *set = sets + ((size_t)blockIdx.y * nsets + s) * W;
	const bool flip = set[0] & 1;
	uint64_t h = 0;
	for (uint32_t w = lane; w < W; w += 64) h ^= mix(canonical_word(set, n, W, w, flip) + 0x9e3779b97f4a7c15ull * (w + 1));
	for (int m = 32; m > 0; m >>= 1) h ^= __shfl_xor(h, m);
	if (lane == 0) hash[(size_t)blockIdx.y * nsets + s] = h;
}

// The ids andi_hip_nj gives: a child is a leaf or the node of an earlier record (andi_hip_format_newick's rule), and every
// node but the last record's is a child exactly once.  seen: 2n bytes of scratch.  The children of the pair records go to kids.
inline bool records_ok(const andi_hip_nj_join *J, size_t n, uint8_t *seen, int2 *kids) {
	const size_t pairs = n - 3;
	memset(seen, 0, n + pairs);
	for (size_t s = 0; s <= pairs; ++s) {
		const int32_t ch[3] = {J[s].a, J[s].b, J[s].c};
		const int nk = s == pairs ? 3 : 2;
		for (int k = 0; k < nk; ++k) {
			if (ch[k] < 0 || (size_t)ch[k] >= n + s || (size_t)ch[k] >= n + pairs || seen[ch[k]]) return false;
			seen[ch[k]] = 1;
		}
		if (s < pairs) kids[s] = make_int2(ch[0], ch[1]);
	}
	return true; // (2 * pairs + 3 = n + pairs children, none twice: every node once)
}

constexpr size_t SETS_GROUP_BYTES = (size_t)2 << 30; // device memory of a group of replicates' sets, at most

// what sets_prepare leaves of a call's arguments
struct SetsPlan {
	size_t nsets, W, G;            // sets per tree, words per set, replicates per group (1 <= G <= max(used.size(), 1))
	std::vector<size_t> used;      // the replicates that count, ascending
	std::vector<int2> kids, tkids; // their pair records' children, in used's order; the point tree's, if there is one
};

// n >= 4; tree may be null (no point tree); set_bytes: the device bytes one set costs the caller beside its W words.
// false: some records are not andi_hip_nj's, and ctx->err says whose, in fn's name.
inline bool sets_prepare(andi_hip_ctx *ctx, const char *fn, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps,
						 size_t n, size_t count, const uint8_t *skip, size_t set_bytes, SetsPlan &p) {
	const size_t nsets = p.nsets = n - 3, nrec = n - 2, W = p.W = (n + 63) / 64;
	std::vector<uint8_t> seen(2 * n);
	if (tree) {
		p.tkids.resize(nsets);
		if (!records_ok(tree, n, seen.data(), p.tkids.data())) {
			ctx->err = std::string(fn) + ": the tree's records are not those of andi_hip_nj";
			return false;
		}
	}
	for (size_t k = 0; k < count; ++k)
		if (!skip || !skip[k]) p.used.push_back(k);
	p.kids.resize(p.used.size() * nsets);
	for (size_t u = 0; u < p.used.size(); ++u)
		if (!records_ok(reps + p.used[u] * nrec, n, seen.data(), p.kids.data() + u * nsets)) {
			char msg[160];
			snprintf(msg, sizeof msg, "%s: the records of replicate %zu are not those of andi_hip_nj", fn, p.used[u]);
			ctx->err = msg;
			return false;
		}
	p.G = nj_group_size(KNOB_NJ_GROUP, 65535, SETS_GROUP_BYTES, nsets * (W * sizeof(uint64_t) + set_bytes));
	if (p.G > p.used.size()) p.G = p.used.empty() ? 1 : p.used.size();
	return true;
}

// The used replicates, p.G at a time: the children of the group that starts at used[first] go to dkids (room for p.G
// trees), k_sets builds the g trees' sets in rsets (room for p.G trees' too), then body(first, g) launches the caller's
// kernels on them and returns their status.  Ends at the first HIP error and returns it.
template <typename Body>
hipError_t sets_for_groups(const SetsPlan &p, size_t n, int2 *dkids, uint64_t *rsets, hipStream_t st, Body body) {
	hipError_t e = hipSuccess;
	for (size_t first = 0; e == hipSuccess && first < p.used.size(); first += p.G) {
		const uint32_t g = (uint32_t)(p.used.size() - first < p.G ? p.used.size() - first : p.G);
		e = hipMemcpyAsync(dkids, p.kids.data() + first * p.nsets, (size_t)g * p.nsets * sizeof(int2), hipMemcpyHostToDevice, st);
		if (e != hipSuccess) break;
		k_sets<<<dim3(((uint32_t)p.W + 63) / 64, g), 64, 0, st>>>(dkids, (uint32_t)n, (uint32_t)p.nsets, (uint32_t)p.W, rsets);
		e = body(first, g);
	}
	return e;
}

} // namespace
