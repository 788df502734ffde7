// nj_taxa.hip — the rogue genomes of a bootstrap on the device (andi_hip_nj_transfer_taxa, include/andi_hip.h): for every
// pair record s of the point-estimate tree and every replicate k, WHICH branch t of the replicate is nearest to branch s
// in the transfer distance, and, per leaf, in how many of the pairs (k, s) that are near enough to count that leaf is one
// of those that have to move (Lemoine et al. 2018 and their booster: the per-taxon transfer score).
//
// The host's validation of the records, the replicates' groups and k_sets are nj_sets.h's, the tile is nj_tile.h's, shared
// with nj_transfer.hip.  This call's own: a set costs its record's two children and one key beside its words, and a
// group's sets go through k_nearest and k_moved and, if match or dist is asked for, one copy of the group's keys to the host:
//   k_limit    one wavefront per set of the point tree: limit[s] = floor(cutoff * (depth[s] - 1)) with depth[s] =
//              min(|L_s|, n - |L_s|), one rounded multiplication in doubles;
//   k_nearest  k_transfer's tiling and inner loop (nj_transfer.hip).  After a replicate tile's last chunk the counters h
//              become the key d << 17 | t << 1 | flip, with d = min(h, n - h) < 2^15, t < 2^16 the replicate's pair
//              record and flip = h > n - h, and fold into the thread's running unsigned minimum per point set: the
//              least d, the least t among those, through the micro-tile, the 16 lanes that share a point set and the
//              replicate's tiles alike.  Sets past nsets (the zero rows that pad a tile) are left out; the first of the
//              16 lanes writes key[k][s], its only writer.  No cap: the replicate's leaf branches are no candidates;
//   k_moved    one wavefront per set word w (8 neighbouring words per block, so their 64-byte lines are shared) and
//              replicate: its lane l is leaf 64 w + l.  It takes the replicate's pairs 64 at a time, lane l that of pair
//              record s0 + l: the key, whether d <= limit[s], and x = word w of L_s xor L_{k,t}, complemented within the n
//              leaves on flip (0 where the pair does not count).  Bit b of the 64 lanes' x is one ballot, and its
//              popcount is what lane b adds to its 32-bit counter (a replicate has fewer than 65536 pairs).  At the
//              end one 64-bit atomicAdd per lane with a leaf into moved, and one per replicate -- by the wavefront of
//              word 0 -- into pairs: integers, exact in any order.
// With every replicate skipped the point tree still goes through the device and the sums stay zero.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "nj_sets.h"
#include "nj_tile.h"

namespace {

constexpr uint32_t MW = 8; // k_moved: words (wavefronts) per block

// limit[s] = floor(cutoff * (depth[s] - 1)), depth[s] = min(|L_s|, n - |L_s|) >= 1.  One wavefront per set.
__global__ __launch_bounds__(256) void k_limit(const uint64_t *__restrict__ sets, uint32_t n, uint32_t nsets, uint32_t W,
											   double cutoff, uint32_t *__restrict__ limit) {
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (s >= nsets) return;
	const uint64_t *set = sets + (size_t)s * W;
	uint32_t c = 0;
	for (uint32_t w = lane; w < W; w += 64) c += (uint32_t)__builtin_popcountll(set[w]);
	for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
	const uint32_t depth = c < n - c ? c : n - c;
	if (lane == 0) limit[s] = (uint32_t)floor(cutoff * (double)(depth - 1));
}

// Block (x, y): point sets x * TS ..., replicate y of the group.  key points at the group's first row.
__global__ __launch_bounds__(256) void k_nearest(const uint64_t *__restrict__ tsets, const uint64_t *__restrict__ rsets,
												 uint32_t n, uint32_t nsets, uint32_t W, uint32_t *__restrict__ key) {
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
			const uint32_t t = t0 + col(tx, j);
			if (t >= nsets) continue; // (a padding row of the replicate's tile is no branch)
#pragma unroll
			for (uint32_t i = 0; i < MS; ++i) {
				const uint32_t h = acc[i][j], flip = h > n - h, d = flip ? n - h : h;
				const uint32_t k = d << 17 | t << 1 | flip;
				best[i] = k < best[i] ? k : best[i];
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
		if (tx == 0 && s < nsets) key[(size_t)blockIdx.y * nsets + s] = m;
	}
}

// Block (x, y): words x * MW ... of replicate y of the group, one per wavefront.  key: the group's rows.
__global__ __launch_bounds__(64 * MW) void k_moved(const uint64_t *__restrict__ tsets, const uint64_t *__restrict__ rsets,
												   const uint32_t *__restrict__ key, const uint32_t *__restrict__ limit,
												   uint32_t n, uint32_t nsets, uint32_t W, unsigned long long *moved,
												   unsigned long long *pairs) {
	const uint32_t w = blockIdx.x * MW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (w >= W) return; // (the whole wavefront)
	rsets += (size_t)blockIdx.y * nsets * W;
	key += (size_t)blockIdx.y * nsets;
	const uint64_t mask = w + 1 == W && (n & 63) ? (1ull << (n & 63)) - 1 : ~0ull;
	uint32_t mine = 0, counted = 0;
	for (uint32_t s0 = 0; s0 < nsets; s0 += 64) {
		const uint32_t s = s0 + lane;
		uint64_t x = 0;
		bool on = false;
		if (s < nsets) {
			const uint32_t k = key[s];
			on = (k >> 17) <= limit[s];
			if (on) {
				const uint32_t t = (k >> 1) & 0xFFFFu;
				x = tsets[(size_t)s * W + w] ^ rsets[(size_t)t * W + w];
				if (k & 1) x = ~x & mask;
			}
		}
		const uint64_t any = __ballot(on);
		if (!any) continue; // (wavefront-uniform)
		counted += (uint32_t)__builtin_popcountll(any);
#pragma unroll
		for (uint32_t b = 0; b < 64; ++b) {
			const uint64_t has = __ballot((x >> b) & 1);
			if (lane == b) mine += (uint32_t)__builtin_popcountll(has);
		}
	}
	const uint32_t leaf = 64 * w + lane;
	if (leaf < n && mine) atomicAdd(&moved[leaf], (unsigned long long)mine);
	if (w == 0 && lane == 0 && counted) atomicAdd(pairs, (unsigned long long)counted);
}

} // namespace

int andi_hip_nj_transfer_taxa(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
							  size_t count, const uint8_t *skip, double cutoff, uint64_t *moved, uint64_t *pairs,
							  uint32_t *match, uint32_t *dist) {
	if (!ctx || !tree || !reps || !moved || !pairs || count == 0 || n < 2 || n > 65535 || !(cutoff >= 0.0 && cutoff <= 1.0)) {
		if (ctx) ctx->err = "andi_hip_nj_transfer_taxa: bad arguments (ctx, tree, reps, moved and pairs must be given, count >= 1, 2 <= n <= 65535, 0 <= cutoff <= 1)";
		return 1;
	}
	memset(moved, 0, n * sizeof *moved);
	*pairs = 0;
	if (n < 4) return 0; // (no branch that is not a leaf's)
	SetsPlan p;
	if (!sets_prepare(ctx, "andi_hip_nj_transfer_taxa", tree, reps, n, count, skip, sizeof(int2) + sizeof(uint32_t), p)) return 1;
	const size_t nsets = p.nsets, W = p.W, G = p.G;
	const std::vector<size_t> &used = p.used;
	const bool detail = match || dist;
	std::vector<uint32_t> hkey(detail ? used.size() * nsets : 0); // the used replicates' keys, as the groups deliver them
	std::vector<uint64_t> hsum(n + 1);                            // moved, then pairs

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, S = (uint32_t)nsets, Wd = (uint32_t)W;
	uint64_t *tsets = nullptr, *rsets = nullptr;
	unsigned long long *dsum = nullptr;
	int2 *dkids = nullptr;
	uint32_t *dlimit = nullptr, *dkey = nullptr;
	hipStream_t st = ctx->stream;
	{
		DevScope dev(st);
		dev.alloc(&tsets, nsets * W), dev.alloc(&dlimit, nsets), dev.alloc(&dsum, n + 1), dev.alloc(&dkids, G * nsets);
		dev.alloc(&dkey, G * nsets), dev.alloc(&rsets, G * nsets * W);
		hipError_t e = dev.err;
		if (e == hipSuccess) e = hipMemsetAsync(dsum, 0, (n + 1) * sizeof *dsum, st);
		if (e == hipSuccess) e = hipMemcpyAsync(dkids, p.tkids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
		if (e == hipSuccess) {
			k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, S, Wd, tsets);
			k_limit<<<(S + 3) / 4, 256, 0, st>>>(tsets, N, S, Wd, cutoff, dlimit);
			e = hipGetLastError();
		}
		if (e == hipSuccess)
			e = sets_for_groups(p, n, dkids, rsets, st, [&](size_t first, uint32_t g) {
				k_nearest<<<dim3((S + TS - 1) / TS, g), 256, 0, st>>>(tsets, rsets, N, S, Wd, dkey);
				k_moved<<<dim3((Wd + MW - 1) / MW, g), 64 * MW, 0, st>>>(tsets, rsets, dkey, dlimit, N, S, Wd, dsum, dsum + n);
				const hipError_t le = hipGetLastError();
				if (le != hipSuccess || !detail) return le;
				return hipMemcpyAsync(hkey.data() + first * nsets, dkey, (size_t)g * nsets * sizeof *dkey, hipMemcpyDeviceToHost, st);
			});
		static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the sums are copied as they are");
		if (e == hipSuccess) e = hipMemcpyAsync(hsum.data(), dsum, (n + 1) * sizeof *dsum, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) return fail(ctx, "andi_hip_nj_transfer_taxa", e);
	}
	memcpy(moved, hsum.data(), n * sizeof *moved);
	*pairs = hsum[n];
	if (match) memset(match, 0xFF, count * nsets * sizeof *match); // (a skipped replicate's row)
	if (dist) memset(dist, 0xFF, count * nsets * sizeof *dist);
	for (size_t u = 0; detail && u < used.size(); ++u)
		for (size_t s = 0; s < nsets; ++s) {
			const uint32_t k = hkey[u * nsets + s];
			if (match) match[used[u] * nsets + s] = (k >> 1) & 0xFFFFu;
			if (dist) dist[used[u] * nsets + s] = k >> 17;
		}
	return 0;
}
