// nj_sets.h — the leaf sets of neighbor-joining trees on the device, shared by nj_support.hip (andi_hip_nj_support) and
// nj_splits.hip (andi_hip_nj_splits): the host's validation of the records, the kernels that build a tree's sets and hash
// them, and the canonical side of a set.  Private; every translation unit that includes it gets its own copy of the
// kernels (they are small), but there is one source.
//
// A tree's leaf sets are bitsets of W = ceil(n / 64) words, set s below node n + s:
//   k_sets   one thread per (tree, word): it walks the records in order and ORs the word of the two children -- a leaf's
//            bit, or the word of an earlier record's set, which the SAME thread wrote (nothing crosses threads, so no
//            barrier and no recursion: a caterpillar 65535 deep is a loop of 65532 trips);
//   k_hash   one wavefront per set: a 64-bit hash of the set on its canonical side -- the side without leaf 0, so a set
//            that holds leaf 0 counts as its complement.  The sets in memory stay as built; the side is taken on the fly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "andi_hip.h"

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

} // namespace
