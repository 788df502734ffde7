// nj_support.hip — bootstrap support of a neighbor-joining tree's branches on the device (andi_hip_nj_support,
// include/andi_hip.h): for every pair record of the point-estimate tree, the number of replicate trees that have the
// same bipartition of the leaves.
//
// The host's validation of the records, the replicates' groups and the kernels that build a tree's leaf sets (k_sets)
// and hash them on their canonical side (k_hash) are nj_sets.h's, shared with nj_transfer.hip and nj_splits.hip.  This
// call's own: a set costs its hash and its record's two children beside its words, there is a point tree, and a group's
// sets are hashed and then go through
//   k_match  one block per set of the point tree: the hashes of all sets of the group's replicates are compared with its
//            own, and where a hash agrees the canonical words themselves are compared, so the count is exact.  A valid
//            tree has every bipartition once, so a replicate adds at most one; the block adds its total to support[s]
//            (the only writer of that word: no atomics; groups run one after the other on the context's stream).
// With every replicate skipped the point tree still goes through the device and the counts come back as zeros.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nj_sets.h"

namespace {

// Block s: support[s] += the number of sets among the g replicates' (g x nsets of them) that equal set s of the point tree
// on the canonical side.
__global__ __launch_bounds__(256) void k_match(const uint64_t *__restrict__ tsets, const uint64_t *__restrict__ thash,
											   const uint64_t *__restrict__ rsets, const uint64_t *__restrict__ rhash,
											   uint32_t n, uint32_t nsets, uint32_t W, uint32_t g, uint32_t *support) {
	const uint32_t s = blockIdx.x;
	const uint64_t *mine = tsets + (size_t)s * W;
	const uint64_t h = thash[s];
	const bool flip = mine[0] & 1;
	const uint64_t total = (uint64_t)g * nsets;
	uint32_t found = 0;
	for (uint64_t i = threadIdx.x; i < total; i += blockDim.x) {
		if (rhash[i] != h) continue;
		const uint64_t *other = rsets + i * W; // (the hash agrees: now the sets themselves)
		const bool oflip = other[0] & 1;
		bool same = true;
		for (uint32_t w = 0; same && w < W; ++w)
			same = canonical_word(mine, n, W, w, flip) == canonical_word(other, n, W, w, oflip);
		found += same;
	}
	__shared__ uint32_t part[4];
	for (int m = 32; m > 0; m >>= 1) found += __shfl_xor(found, m);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = found;
	__syncthreads();
	if (threadIdx.x == 0) support[s] += part[0] + part[1] + part[2] + part[3];
}

} // namespace

int andi_hip_nj_support(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
						size_t count, const uint8_t *skip, uint32_t *support) {
	if (!ctx || !tree || !reps || !support || count == 0 || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj_support: bad arguments (ctx, tree, reps and support must be given, count >= 1, 2 <= n <= 65535)";
		return 1;
	}
	if (n < 4) return 0; // (no branch that is not a leaf's)
	SetsPlan p;
	if (!sets_prepare(ctx, "andi_hip_nj_support", tree, reps, n, count, skip, sizeof(uint64_t) + sizeof(int2), p)) return 1;
	const size_t nsets = p.nsets, W = p.W, G = p.G;

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, S = (uint32_t)nsets, Wd = (uint32_t)W;
	uint64_t *tsets = nullptr, *thash = nullptr, *rsets = nullptr, *rhash = nullptr;
	int2 *dkids = nullptr;
	uint32_t *dsup = nullptr;
	hipStream_t st = ctx->stream;
	DevScope dev(st);
	dev.alloc(&tsets, nsets * W), dev.alloc(&thash, nsets), dev.alloc(&dsup, nsets);
	dev.alloc(&dkids, G * nsets), dev.alloc(&rhash, G * nsets), dev.alloc(&rsets, G * nsets * W);
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemsetAsync(dsup, 0, nsets * sizeof *dsup, st);
	// the point tree's sets and hashes (also when every replicate is skipped: the counts are zeros then)
	if (e == hipSuccess) e = hipMemcpyAsync(dkids, p.tkids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, S, Wd, tsets);
		k_hash<<<dim3((S + 3) / 4, 1), 256, 0, st>>>(tsets, N, S, Wd, thash);
		e = hipGetLastError();
	}
	if (e == hipSuccess)
		e = sets_for_groups(p, n, dkids, rsets, st, [&](size_t, uint32_t g) {
			k_hash<<<dim3((S + 3) / 4, g), 256, 0, st>>>(rsets, N, S, Wd, rhash);
			k_match<<<S, 256, 0, st>>>(tsets, thash, rsets, rhash, N, S, Wd, g, dsup);
			return hipGetLastError();
		});
	if (e == hipSuccess) e = hipMemcpyAsync(support, dsup, nsets * sizeof *dsup, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_nj_support", e);
	return 0;
}
