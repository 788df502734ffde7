// bootstrap.hip — K8: pairwise bootstrap of the substitution-count matrix.
//
// calculate_bootstrap (src/process.c:289-321) resamples, for every unordered pair
// i < j, the summed counts model_average(M(i,j), M(j,i)) from a multinomial with
// N = total count and p = counts / N (model_bootstrap, src/model.c:222-232,
// gsl_ran_multinomial), mirrors the result to (j,i) and sets the diagonal to
// {counts[0] = 1, seq_len = 1}.  The reference draws from a global GSL generator
// seeded with time(NULL) and has no test for it, so there is nothing to be
// bit-identical to ("parity unpinned"); what is kept is the distribution.  Here
// every (replicate, pair) owns a counter-based Philox stream, so the result is a
// pure function of (seed, replicate, i, j) whatever the launch geometry, and all
// replicates of a matrix are one launch.
//
// andi_hip_bootstrap_nj (nj.hip) never has the replicates as models: k_pair_sums adds the two directions of every pair
// once per call, and k_bootstrap_dist draws a (replicate, pair) from those sums and stores the one double its tree needs --
// the portable estimate (andi_estimate.h) of the drawn counts doubled, which is what model_average makes of the mirrored
// replicate.  Draw and estimator are the functions k_bootstrap and the host use, so both are bit-exact to them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "andi_estimate.h"
#include "andi_hip.h"
#include "bootstrap.h"
#include "bootstrap_draw.h"

namespace {

// One thread per (replicate, unordered pair incl. diagonal); replicate rep of the launch is rep0 + rep of the stream.
__global__ __launch_bounds__(256) void k_bootstrap(const andi_hip_model *__restrict__ M,
												   andi_hip_model *__restrict__ B, uint32_t n,
												   uint32_t rep0, uint32_t replicates, uint64_t seed) {
	const uint64_t per = (uint64_t)n * (n + 1) / 2;
	uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (gid >= per * replicates) return;
	const uint32_t rep = (uint32_t)(gid / per);
	uint64_t t = gid % per;
	// unrank t -> (i, j), i <= j, row-major over the upper triangle
	uint32_t i = 0;
	{
		// rows have n, n-1, ... entries; solve by a short search from an estimate
		double est = ((2.0 * n + 1) - sqrt((2.0 * n + 1) * (2.0 * n + 1) - 8.0 * (double)t)) / 2.0;
		i = est > 0 ? (uint32_t)est : 0;
		auto start = [n](uint64_t r) { return r * n - r * (r - 1) / 2; };
		while (i > 0 && start(i) > t) --i;
		while (i + 1 < n && start(i + 1) <= t) ++i;
		t -= start(i);
	}
	const uint32_t j = i + (uint32_t)t;
	andi_hip_model *out = B + (size_t)rep * n * n;
	andi_hip_model res;
	if (i == j) { // src/process.c:303-306
		for (int c = 0; c < 16; ++c) res.counts[c] = 0;
		res.counts[0] = 1, res.seq_len = 1;
		out[(size_t)i * n + i] = res;
		return;
	}
	const andi_hip_model a = M[(size_t)i * n + j], b = M[(size_t)j * n + i];
	uint32_t sums[16];
	for (int c = 0; c < 16; ++c) sums[c] = a.counts[c] + b.counts[c]; // model_average, src/model.c:39-46
	res.seq_len = a.seq_len + b.seq_len;
	bootstrap_draw(seed, (uint64_t)rep0 + rep, (uint64_t)i * n + j, sums, res.counts);
	out[(size_t)i * n + j] = res;
	out[(size_t)j * n + i] = res; // src/process.c:314
}

// where row i of the packed strict upper triangle starts: pair (i, j), i < j, is entry tri_start(i) + j - i - 1
__device__ inline uint64_t tri_start(uint64_t i, uint64_t n) { return i * (2 * n - i - 1) / 2; }

// S[t][c] = M[i][j].counts[c] + M[j][i].counts[c] (32-bit, wrapping as model_average) for every pair t = (i, j), i < j:
// block row i, sixteen consecutive threads per pair, so the 64 bytes of a pair's counts are read and written as one piece.
__global__ __launch_bounds__(256) void k_pair_sums(const andi_hip_model *__restrict__ M, uint32_t *__restrict__ S, uint32_t n) {
	const uint32_t i = blockIdx.y;
	const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t j = (uint64_t)i + 1 + (item >> 4);
	const uint32_t c = (uint32_t)item & 15;
	if (j >= n) return;
	const uint64_t t = tri_start(i, n) + (j - i - 1);
	S[t * 16 + c] = M[(size_t)i * n + j].counts[c] + M[(size_t)j * n + i].counts[c];
}

// One thread per (replicate of the group = blockIdx.y, pair): the sums, the draw of replicate rep0 + blockIdx.y, the
// estimate, one double to D[rep][i * n + j] (the upper triangle; k_nj_init mirrors it).
template <int MODEL>
__global__ __launch_bounds__(256) void k_bootstrap_dist(const uint4 *__restrict__ S, double *__restrict__ D, uint32_t n,
														uint32_t rep0, uint64_t seed) {
	const uint64_t per = (uint64_t)n * (n - 1) / 2;
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= per) return;
	const uint32_t rep = blockIdx.y;
	uint32_t i;
	{ // unrank t -> (i, j), i < j: rows have n-1, n-2, ... entries; a short search from an estimate
		const double w = 2.0 * n - 1;
		const double est = (w - sqrt(w * w - 8.0 * (double)t)) / 2.0;
		i = est > 0 ? (uint32_t)est : 0;
		if (i > n - 2) i = n - 2;
		while (i > 0 && tri_start(i, n) > t) --i;
		while (i + 2 < n && tri_start(i + 1, n) <= t) ++i;
	}
	const uint32_t j = i + 1 + (uint32_t)(t - tri_start(i, n));
	uint32_t sums[16];
	for (int q = 0; q < 4; ++q) {
		const uint4 v = S[t * 4 + q];
		sums[4 * q] = v.x, sums[4 * q + 1] = v.y, sums[4 * q + 2] = v.z, sums[4 * q + 3] = v.w;
	}
	uint32_t draw[16];
	bootstrap_draw(seed, (uint64_t)rep0 + rep, (uint64_t)i * n + j, sums, draw);
	andi_hip_model m;
	for (int c = 0; c < 16; ++c) m.counts[c] = draw[c] + draw[c]; // model_average of the replicate's (i, j) and (j, i)
	m.seq_len = 0;                                                // (no estimator reads it)
	D[(size_t)rep * n * n + (size_t)i * n + j] = andi_estimate_portable(&m, MODEL);
}

} // namespace

hipError_t andi_launch_bootstrap(const andi_hip_model *M_dev, andi_hip_model *B_dev, uint32_t n, uint32_t first,
								 uint32_t replicates, uint64_t seed, hipStream_t st) {
	const uint64_t items = (uint64_t)n * (n + 1) / 2 * replicates;
	if (items == 0) return hipSuccess;
	k_bootstrap<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(M_dev, B_dev, n, first, replicates, seed);
	return hipGetLastError();
}

hipError_t andi_launch_pair_sums(const andi_hip_model *M_dev, uint32_t *S_dev, uint32_t n, hipStream_t st) {
	if (n < 2) return hipSuccess;
	k_pair_sums<<<dim3((unsigned)(((uint64_t)(n - 1) * 16 + 255) / 256), n - 1), 256, 0, st>>>(M_dev, S_dev, n);
	return hipGetLastError();
}

hipError_t andi_launch_bootstrap_dist(const uint32_t *S_dev, double *D_dev, uint32_t n, int model, uint32_t first,
									  uint32_t group, uint64_t seed, hipStream_t st) {
	const uint64_t per = (uint64_t)n * (n - 1) / 2;
	if (per == 0 || group == 0) return hipSuccess;
	const dim3 grid((unsigned)((per + 255) / 256), group);
	const uint4 *S = (const uint4 *)S_dev;
	switch (model) {
		case ANDI_M_RAW: k_bootstrap_dist<ANDI_M_RAW><<<grid, 256, 0, st>>>(S, D_dev, n, first, seed); break;
		case ANDI_M_JC: k_bootstrap_dist<ANDI_M_JC><<<grid, 256, 0, st>>>(S, D_dev, n, first, seed); break;
		case ANDI_M_KIMURA: k_bootstrap_dist<ANDI_M_KIMURA><<<grid, 256, 0, st>>>(S, D_dev, n, first, seed); break;
		case ANDI_M_LOGDET: k_bootstrap_dist<ANDI_M_LOGDET><<<grid, 256, 0, st>>>(S, D_dev, n, first, seed); break;
		case ANDI_M_ANI: k_bootstrap_dist<ANDI_M_ANI><<<grid, 256, 0, st>>>(S, D_dev, n, first, seed); break;
		default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
