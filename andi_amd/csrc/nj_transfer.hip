// nj_transfer.hip — transfer bootstrap support of a neighbor-joining tree's branches on the device (andi_hip_nj_transfer,
// include/andi_hip.h): for every pair record s of the point-estimate tree and every replicate k, the transfer index --
// the least number of leaves that have to move to turn a branch of the replicate's tree into branch s -- and its sum
// over the replicates (Lemoine et al. 2018: the transfer bootstrap expectation is 1 - sum / (used * (depth - 1))).
//
// The host's validation of the records, the replicates' groups and k_sets are nj_sets.h's, shared with nj_support.hip and
// nj_splits.hip; the tile's constants and stage, col and bcnt_add are nj_tile.h's, shared with nj_taxa.hip.  A tree's leaf sets are bitsets of W = ceil(n / 64) words (the padding bits of the last word are zero),
// so h(A, B) = |A xor B| is a sum of popcounts and the transfer distance is min(h, n - h).  This call's own: a set costs
// its record's two children and one index of per beside its words, there is a point tree, and a group's sets go through
// k_transfer and, if per is asked for, one copy of the group's rows to the host:
//   k_depth     one wavefront per set of the point tree: depth[s] = min(|L_s|, n - |L_s|);
//   k_transfer  a block owns a tile of TS sets of the point tree and ONE replicate (blockIdx.y) and walks that
//               replicate's sets in tiles of TT.  Both tiles go through LDS in chunks of WC words, word-major
//               ([word][set], rows padded to LDP), and every thread keeps an MS x MT micro-tile of 32-bit counters: a
//               word read from LDS meets MT (MS) partners, so a chunk word costs MS + MT LDS reads for MS * MT
//               xor/popcounts.  After a replicate tile's last chunk the counters become min(h, n - h) and fold into the
//               thread's running minimum per point set; sets past nsets (the zero rows that pad a tile: h = |L_s|, a
//               false minimum) are left out there, and words past W are neither staged nor read.  Behind the last tile
//               the 16 lanes that share a point set reduce their minima, the first of them applies the cap depth - 1
//               (what the replicate's leaf branches contribute), writes per[k][s] -- its only writer -- and adds it to
//               transfer[s] with a 64-bit integer atomic (exact in any order).
// With every replicate skipped the point tree still goes through the device: depth, zero sums, and per all 0xFFFFFFFF.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "nj_sets.h"
#include "nj_tile.h"

namespace {

// depth[s] = min(|L_s|, n - |L_s|).  One wavefront per set.
__global__ __launch_bounds__(256) void k_depth(const uint64_t *__restrict__ sets, uint32_t n, uint32_t nsets, uint32_t W,
											   uint32_t *__restrict__ depth) {
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (s >= nsets) return;
	const uint64_t *set = sets + (size_t)s * W;
	uint32_t c = 0;
	for (uint32_t w = lane; w < W; w += 64) c += (uint32_t)__builtin_popcountll(set[w]);
	for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
	if (lane == 0) depth[s] = c < n - c ? c : n - c;
}

// Block (x, y): point sets x * TS ..., replicate y of the group.  per (may be null) and transfer as in the header;
// per points at the group's first row.
__global__ __launch_bounds__(256) void k_transfer(const uint64_t *__restrict__ tsets, const uint64_t *__restrict__ rsets,
												  const uint32_t *__restrict__ depth, uint32_t n, uint32_t nsets, uint32_t W,
												  uint32_t *__restrict__ per, unsigned long long *transfer) {
	__shared__ alignas(16) uint64_t A[WC][LDP], B[WC][LDP];
	const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	const uint32_t s0 = blockIdx.x * TS;
	rsets += (size_t)blockIdx.y * nsets * W;
	uint32_t best[MS];
#pragma unroll
	for (uint32_t i = 0; i < MS; ++i) best[i] = 0xFFFFFFFFu;
	for (uint32_t t0 = 0; t0 < nsets; t0 += TT) {
		uint32_t acc[MS][MT];
#pragma unroll
		for (uint32_t i = 0; i < MS; ++i)
#pragma unroll
			for (uint32_t j = 0; j < MT; ++j) acc[i][j] = 0;
		for (uint32_t w0 = 0; w0 < W; w0 += WC) {
			const uint32_t wc = W - w0 < WC ? W - w0 : WC;
			__syncthreads(); // (the chunk before this one has been read)
			stage(A, tsets, s0, nsets, W, w0, wc);
			stage(B, rsets, t0, nsets, W, w0, wc);
			__syncthreads();
			for (uint32_t w = 0; w < wc; ++w) {
				uint64_t a[MS], b[MT];
#pragma unroll
				for (uint32_t i = 0; i < MS; i += 2) { // (two neighbouring sets: one 16-byte LDS read)
					const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(&A[w][2 * ty + 16 * i]);
					a[i] = v.x, a[i + 1] = v.y;
				}
#pragma unroll
				for (uint32_t j = 0; j < MT; j += 2) {
					const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(&B[w][2 * tx + 16 * j]);
					b[j] = v.x, b[j + 1] = v.y;
				}
#pragma unroll
				for (uint32_t i = 0; i < MS; ++i)
#pragma unroll
					for (uint32_t j = 0; j < MT; ++j) {
						const uint64_t x = a[i] ^ b[j];
						acc[i][j] = bcnt_add((uint32_t)(x >> 32), bcnt_add((uint32_t)x, acc[i][j]));
					}
			}
		}
#pragma unroll
		for (uint32_t j = 0; j < MT; ++j) {
			if (t0 + col(tx, j) >= nsets) continue; // (a padding row of the replicate's tile is no branch)
#pragma unroll
			for (uint32_t i = 0; i < MS; ++i) {
				const uint32_t h = acc[i][j], d = h < n - h ? h : n - h;
				best[i] = d < best[i] ? d : best[i];
			}
		}
	}
#pragma unroll
	for (uint32_t i = 0; i < MS; ++i) {
		uint32_t m = best[i];
		for (int x = 8; x > 0; x >>= 1) { // the 16 lanes tx = 0 .. 15 of this ty: neighbours in one wavefront
			const uint32_t o = __shfl_xor(m, x);
			m = o < m ? o : m;
		}
		const uint32_t s = s0 + col(ty, i);
		if (tx == 0 && s < nsets) {
			const uint32_t cap = depth[s] - 1;
			m = m < cap ? m : cap;
			if (per) per[(size_t)blockIdx.y * nsets + s] = m;
			atomicAdd(&transfer[s], (unsigned long long)m);
		}
	}
}

} // namespace

int andi_hip_nj_transfer(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
						 size_t count, const uint8_t *skip, uint32_t *depth, uint64_t *transfer, uint32_t *per) {
	if (!ctx || !tree || !reps || !depth || !transfer || count == 0 || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj_transfer: bad arguments (ctx, tree, reps, depth and transfer must be given, count >= 1, 2 <= n <= 65535)";
		return 1;
	}
	if (n < 4) return 0; // (no branch that is not a leaf's)
	SetsPlan p;
	if (!sets_prepare(ctx, "andi_hip_nj_transfer", tree, reps, n, count, skip, sizeof(int2) + sizeof(uint32_t), p)) return 1;
	const size_t nsets = p.nsets, W = p.W, G = p.G;
	const std::vector<size_t> &used = p.used;
	std::vector<uint32_t> hper(per ? used.size() * nsets : 0); // the used replicates' rows, as the groups deliver them

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, S = (uint32_t)nsets, Wd = (uint32_t)W;
	uint64_t *tsets = nullptr, *rsets = nullptr;
	unsigned long long *dsum = nullptr;
	int2 *dkids = nullptr;
	uint32_t *ddepth = nullptr, *dper = nullptr;
	hipStream_t st = ctx->stream;
	{
		DevScope dev(st);
		dev.alloc(&tsets, nsets * W), dev.alloc(&ddepth, nsets), dev.alloc(&dsum, nsets), dev.alloc(&dkids, G * nsets);
		if (per) dev.alloc(&dper, G * nsets);
		dev.alloc(&rsets, G * nsets * W);
		hipError_t e = dev.err;
		if (e == hipSuccess) e = hipMemsetAsync(dsum, 0, nsets * sizeof *dsum, st);
		// the point tree's sets and depths (also when every replicate is skipped: depth, and zero sums)
		if (e == hipSuccess) e = hipMemcpyAsync(dkids, p.tkids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
		if (e == hipSuccess) {
			k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, S, Wd, tsets);
			k_depth<<<(S + 3) / 4, 256, 0, st>>>(tsets, N, S, Wd, ddepth);
			e = hipGetLastError();
		}
		if (e == hipSuccess)
			e = sets_for_groups(p, n, dkids, rsets, st, [&](size_t first, uint32_t g) {
				k_transfer<<<dim3((S + TS - 1) / TS, g), 256, 0, st>>>(tsets, rsets, ddepth, N, S, Wd, dper, dsum);
				const hipError_t le = hipGetLastError();
				if (le != hipSuccess || !per) return le;
				return hipMemcpyAsync(hper.data() + first * nsets, dper, (size_t)g * nsets * sizeof *dper, hipMemcpyDeviceToHost, st);
			});
		static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the sums are copied as they are");
		if (e == hipSuccess) e = hipMemcpyAsync(depth, ddepth, nsets * sizeof *ddepth, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(transfer, dsum, nsets * sizeof *dsum, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) return fail(ctx, "andi_hip_nj_transfer", e);
	}
	if (per) {
		memset(per, 0xFF, count * nsets * sizeof *per); // (a skipped replicate's row)
		for (size_t u = 0; u < used.size(); ++u) memcpy(per + used[u] * nsets, hper.data() + u * nsets, nsets * sizeof *per);
	}
	return 0;
}
