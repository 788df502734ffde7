// nj_tile.h — the tile of the kernels that meet every leaf set of one tree with every leaf set of another: k_transfer
// (nj_transfer.hip) and its argmin sibling k_nearest (nj_taxa.hip).  Private.  Both tiles of TS sets go through LDS in
// chunks of WC words, word-major ([word][set], rows padded to LDP), and each of a block's 256 threads keeps an MS x MT
// micro-tile of 32-bit counters.  Here: the tile's constants and the three helpers the two kernels share, as
// nj_transfer.hip had them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t TS = 128, TT = 128; // sets of the point tree / of the replicate per tile
constexpr uint32_t WC = 8;             // words per chunk in LDS
constexpr uint32_t MS = 8, MT = 8;     // a thread's micro-tile: point sets col(ty, i), replicate sets col(tx, j)
constexpr uint32_t LDP = TS + 4;       // words per LDS row (the staging stores of a wavefront spread over the banks)
static_assert(TS == 16 * MS && TT == 16 * MT && TS == TT && LDP % 2 == 0, "256 threads as 16 x 16 micro-tiles; 16-byte LDS reads");

// popcount(x) + sum as the one instruction it is (the compiler's own choice is two counts from zero and a three-way add)
__device__ inline uint32_t bcnt_add(uint32_t x, uint32_t sum) {
	uint32_t r;
	asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(sum));
	return r;
}

// the tile row of micro-tile entry i of the thread with coordinate c (0 .. 15): pairs of neighbours, 32 apart
__device__ inline uint32_t col(uint32_t c, uint32_t i) { return 2 * c + (i & 1) + 16 * (i & ~1u); }

// rows first .. first + TS of sets (nsets x W), words w0 .. w0 + wc, to tile[word][row]; rows past nsets are zero
__device__ inline void stage(uint64_t (*tile)[LDP], const uint64_t *__restrict__ sets, uint32_t first, uint32_t nsets,
							 uint32_t W, uint32_t w0, uint32_t wc) {
	const uint32_t w = threadIdx.x % WC;
	if (w >= wc) return;
#pragma unroll
	for (uint32_t row = threadIdx.x / WC; row < TS; row += 256 / WC) {
		const uint32_t s = first + row;
		tile[w][row] = s < nsets ? sets[(size_t)s * W + w0 + w] : 0ull;
	}
}

} // namespace
