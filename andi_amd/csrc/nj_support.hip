// nj_support.hip — bootstrap support of a neighbor-joining tree's branches on the device (andi_hip_nj_support,
// include/andi_hip.h): for every pair record of the point-estimate tree, the number of replicate trees that have the
// same bipartition of the leaves.
//
// The host validates the records (every child a leaf or an earlier record's node, every node a child exactly once) and
// hands the device only the two children of every pair record.  On the device a tree's leaf sets are bitsets of W =
// ceil(n / 64) words, set s below node n + s, built by k_sets and hashed on their canonical side -- the side without
// leaf 0 -- by k_hash (nj_sets.h, shared with nj_splits.hip); then
//   k_match  one block per set of the point tree: the hashes of all sets of the group's replicates are compared with its
//            own, and where a hash agrees the canonical words themselves are compared, so the count is exact.  A valid
//            tree has every bipartition once, so a replicate adds at most one; the block adds its total to support[s]
//            (the only writer of that word: no atomics; groups run one after the other on the context's stream).
// Replicates are taken in groups of as many trees as GROUP_BYTES hold (one tree's sets are 537 MB at 65535 leaves).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_internal.h"
#include "nj_sets.h"

namespace {

constexpr size_t GROUP_BYTES = (size_t)2 << 30; // device memory of a group of replicates' sets, at most (one tree always fits)
constexpr size_t MAX_GROUP = 65535;             // a grid's second dimension

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
	const size_t nsets = n - 3, nrec = n - 2, W = (n + 63) / 64;
	// the group: the replicates that count, GROUP_BYTES of sets at a time
	const size_t tree_bytes = nsets * W * sizeof(uint64_t) + nsets * (sizeof(uint64_t) + sizeof(int2));
	size_t G = GROUP_BYTES / tree_bytes;
	G = G < 1 ? 1 : G > MAX_GROUP ? MAX_GROUP : G;
	if (const char *v = andi_knob(KNOB_NJ_GROUP)) { // test hook: a group size of the test's choosing (as andi_hip_nj_batch)
		const long long f = atoll(v);
		if (f >= 1) G = (size_t)f > MAX_GROUP ? MAX_GROUP : (size_t)f;
	}
	if (G > count) G = count;
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> tkids(nsets), kids;
	if (!records_ok(tree, n, seen.data(), tkids.data())) {
		ctx->err = "andi_hip_nj_support: the tree's records are not those of andi_hip_nj";
		return 1;
	}
	std::vector<size_t> used; // the replicates that count, validated all before any HIP call
	for (size_t k = 0; k < count; ++k)
		if (!skip || !skip[k]) used.push_back(k);
	kids.resize(used.size() * nsets);
	for (size_t u = 0; u < used.size(); ++u)
		if (!records_ok(reps + used[u] * nrec, n, seen.data(), kids.data() + u * nsets)) {
			char msg[128];
			snprintf(msg, sizeof msg, "andi_hip_nj_support: the records of replicate %zu are not those of andi_hip_nj", used[u]);
			ctx->err = msg;
			return 1;
		}
	if (G > used.size()) G = used.size() ? used.size() : 1;

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, S = (uint32_t)nsets, Wd = (uint32_t)W;
	uint64_t *tsets = nullptr, *thash = nullptr, *rsets = nullptr, *rhash = nullptr;
	int2 *dkids = nullptr;
	uint32_t *dsup = nullptr;
	hipStream_t st = ctx->stream;
	hipError_t e = dmalloc(&tsets, nsets * W);
	if (e == hipSuccess) e = dmalloc(&thash, nsets);
	if (e == hipSuccess) e = dmalloc(&dsup, nsets);
	if (e == hipSuccess) e = dmalloc(&dkids, (G > 1 ? G : 1) * nsets);
	if (e == hipSuccess) e = dmalloc(&rhash, G * nsets);
	if (e == hipSuccess) e = dmalloc(&rsets, G * nsets * W);
	if (e == hipSuccess) e = hipMemsetAsync(dsup, 0, nsets * sizeof *dsup, st);
	// the point tree's sets and hashes
	if (e == hipSuccess) e = hipMemcpyAsync(dkids, tkids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, S, Wd, tsets);
		k_hash<<<dim3((S + 3) / 4, 1), 256, 0, st>>>(tsets, N, S, Wd, thash);
		e = hipGetLastError();
	}
	for (size_t first = 0; e == hipSuccess && first < used.size(); first += G) {
		const uint32_t g = (uint32_t)(used.size() - first < G ? used.size() - first : G);
		e = hipMemcpyAsync(dkids, kids.data() + first * nsets, (size_t)g * nsets * sizeof(int2), hipMemcpyHostToDevice, st);
		if (e != hipSuccess) break;
		k_sets<<<dim3((Wd + 63) / 64, g), 64, 0, st>>>(dkids, N, S, Wd, rsets);
		k_hash<<<dim3((S + 3) / 4, g), 256, 0, st>>>(rsets, N, S, Wd, rhash);
		k_match<<<S, 256, 0, st>>>(tsets, thash, rsets, rhash, N, S, Wd, g, dsup);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(support, dsup, nsets * sizeof *dsup, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	(void)hipStreamSynchronize(st); // (an error exit: nothing in flight uses the buffers below)
	for (void *p : {(void *)tsets, (void *)thash, (void *)rsets, (void *)rhash, (void *)dkids, (void *)dsup})
		if (p) (void)andi_arena::dev_free(p, false);
	if (e != hipSuccess) return fail(ctx, "andi_hip_nj_support", e);
	return 0;
}
