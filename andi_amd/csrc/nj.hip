// nj.hip — neighbor-joining of a distance matrix on the device (andi_hip_nj, include/andi_hip.h).
//
// The reference stops at the matrix; its users run PHYLIP's neighbor on it (docs/manual/andi-manual.tex:301-341).  This
// is that step on the MI355X, bit for bit the arithmetic contract in andi_hip.h (tests/nj_model.py restates it in NumPy).
// D stays resident as doubles, indexed by SLOT: leaf i starts in slot i, a join's node takes the lower slot of its two
// children and the other slot retires.  The active slots are kept as an ascending compacted list (act), ping-ponged
// between two buffers, so every step reads only the r x r active block.  A step with r >= 4 active nodes is three
// launches on the context's stream, with no host synchronisation between steps:
//   k_nj_rowsum  R[x] for every active slot x: one wavefront per row, its active entries loaded by all lanes at once
//                (1024 in flight), then added one after the other in slot order from +0.0 (sequential, as the contract
//                asks) by a chain that reads them lane by lane;
//   k_nj_argmin  the least (Q, id_x, id_y) of every 64 x 64 tile of the active upper triangle, one result per block;
//   k_nj_join    one block: the least of those results, the record, the new node's row and column, the list compacted.
// One D2H copy of the records at the end.  No graph capture, no grid-wide barrier, no atomics on the step path.
//
// Every kernel takes the REPLICATE as its grid's second dimension (andi_hip_nj_batch): matrices of one n are all at the
// same r at step s, so a step of a whole group of them is still these three launches.  The buffers hold one replicate
// after the other -- D (n x n), R (n), the lists (two act lists and the ids: 3n), the tile results, the records -- and a
// block offsets its pointers by blockIdx.y.  andi_hip_nj is the group of one.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_internal.h"
#include "bootstrap.h"
#include "nj_cand.h" // Cand, better, none, wave_min, block_min

static_assert(sizeof(andi_hip_nj_join) == 40, "andi_hip_nj_join: 3 ids, pad, 3 lengths");

namespace {

constexpr int RS_CHUNKS = 16;                // k_nj_rowsum: 16 x 64 entries of a row in flight per wavefront
constexpr int TILE = 64;                     // k_nj_argmin: 64 x 64 pairs per block, 16 rows per wavefront
constexpr int JOIN_THREADS = 1024;

// Mirror the upper triangle (row i = block i), diagonal +0.0; the first non-finite D[i][j], i < j, in row-major order
// goes to the replicate's bad word as i * n + j.  act = id = identity.
__global__ __launch_bounds__(256) void k_nj_init(double *__restrict__ D, uint32_t n, int32_t *__restrict__ lists,
												 unsigned long long *bad) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, bad += rep;
	int32_t *act = lists + rep * 3 * n, *id = act + 2 * (size_t)n;
	const uint32_t i = blockIdx.x;
	double *row = D + (size_t)i * n;
	unsigned long long first = ~0ull;
	for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
		if (j > i) {
			if (!__builtin_isfinite(row[j]) && first == ~0ull) first = (unsigned long long)i * n + j;
		} else {
			row[j] = j < i ? D[(size_t)j * n + i] : 0.0;
		}
	}
	if (first != ~0ull) atomicMin(bad, first);
	if (threadIdx.x == 0) act[i] = (int32_t)i, id[i] = (int32_t)i;
}

// R[x] = sum over k = 0 .. r-1 of D[x][act[k]], in that order, from +0.0, for x = act[row]: one wavefront per row.  The
// lanes load RS_CHUNKS x 64 entries of the row at once (all in flight together); the chain of adds then takes them lane by
// lane (v_readlane into scalar registers), so the sum stays sequential while the loads are spread over every CU.
__device__ inline double lane_value(double v, int l) {
	const long long b = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
	return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__global__ __launch_bounds__(256) void k_nj_rowsum(const double *__restrict__ D, uint32_t n, const int32_t *__restrict__ lists,
												   uint32_t cur, uint32_t r, double *__restrict__ R) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, R += rep * n;
	const int32_t *act = lists + rep * 3 * n + cur;
	const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (x >= r) return;
	const size_t sx = (size_t)act[x];
	const double *row = D + sx * n;
	double acc = 0.0;
	for (uint32_t base = 0; base < r; base += 64 * RS_CHUNKS) {
		double v[RS_CHUNKS];
#pragma unroll
		for (int c = 0; c < RS_CHUNKS; ++c) {
			const uint32_t k = base + 64 * c + lane;
			v[c] = k < r ? row[act[k]] : 0.0;
		}
#pragma unroll
		for (int c = 0; c < RS_CHUNKS; ++c) {
			const uint32_t k0 = base + 64 * c;
			if (k0 + 64 <= r) {
#pragma unroll
				for (int l = 0; l < 64; ++l) acc += lane_value(v[c], l);
			} else if (k0 < r) {
				for (int l = 0; l < (int)(r - k0); ++l) acc += lane_value(v[c], l);
			}
		}
	}
	if (lane == 0) R[sx] = acc;
}

// Block b = tile (tp, tq), tp <= tq, of the active pairs in list positions: wave w takes rows tp*64 + 16w .. +15, lane l
// column tq*64 + l.  Q = ((r-2) * D[x][y] - R_x) - R_y with x the member of smaller id.
__global__ __launch_bounds__(256) void k_nj_argmin(const double *__restrict__ D, uint32_t n,
												   const int32_t *__restrict__ lists, uint32_t cur, uint32_t r,
												   const double *__restrict__ R, Cand *__restrict__ part, uint32_t part_stride) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, R += rep * n, part += rep * part_stride;
	const int32_t *act = lists + rep * 3 * n + cur, *id = lists + rep * 3 * n + 2 * (size_t)n;
	const uint64_t b = blockIdx.x;
	uint32_t tq = (uint32_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
	while ((uint64_t)tq * (tq + 1) / 2 > b) --tq;
	while ((uint64_t)(tq + 1) * (tq + 2) / 2 <= b) ++tq;
	const uint32_t tp = (uint32_t)(b - (uint64_t)tq * (tq + 1) / 2);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t q = tq * TILE + lane;
	Cand best = none();
	if (q < r) {
		const int32_t sq = act[q], iq = id[sq];
		const double Rq = R[sq], c = (double)(r - 2);
		const uint32_t p0 = tp * TILE + wave * 16;
		double d[16];
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const uint32_t p = p0 + k;
			d[k] = p < q ? D[(size_t)act[p] * n + sq] : 0.0;
		}
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const uint32_t p = p0 + k;
			if (p >= q) continue;
			const int32_t sp = act[p], ip = id[sp];
			const double Rp = R[sp];
			Cand cand;
			if (ip < iq) cand = Cand{(c * d[k] - Rp) - Rq, ip, iq, sp, sq};
			else cand = Cand{(c * d[k] - Rq) - Rp, iq, ip, sq, sp};
			if (better(cand, best)) best = cand;
		}
	}
	best = block_min(best);
	if (threadIdx.x == 0) part[b] = best;
}

// One block: the least of nparts tile results, its record, node u = n + step in the lower slot, the other slot retired
// (the list at cur -> the other list, order kept).
__global__ __launch_bounds__(JOIN_THREADS) void k_nj_join(double *__restrict__ D, uint32_t n, int32_t *__restrict__ lists,
														  uint32_t cur, uint32_t r, const double *__restrict__ R,
														  const Cand *__restrict__ part, uint32_t part_stride, uint32_t nparts,
														  andi_hip_nj_join *__restrict__ rec, uint32_t nrec, uint32_t step) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, R += rep * n, part += rep * part_stride, rec += rep * nrec;
	const int32_t *act_in = lists + rep * 3 * n + cur;
	int32_t *act_out = lists + rep * 3 * n + (n - cur), *id = lists + rep * 3 * n + 2 * (size_t)n;
	Cand best = none();
	for (uint32_t k = threadIdx.x; k < nparts; k += blockDim.x)
		if (better(part[k], best)) best = part[k];
	best = block_min(best);
	const size_t sa = (size_t)best.sa, sb = (size_t)best.sb;
	const size_t su = sa < sb ? sa : sb, so = sa < sb ? sb : sa;
	const double d = D[sa * n + sb];
	if (threadIdx.x == 0) {
		const double la = d * 0.5 + (R[sa] - R[sb]) / (double)(2 * (r - 2));
		andi_hip_nj_join j;
		j.a = best.ia, j.b = best.ib, j.c = -1, j.pad = 0;
		j.la = la, j.lb = d - la, j.lc = 0.0;
		rec[step] = j;
	}
	for (uint32_t i = threadIdx.x; i < r; i += blockDim.x) {
		const size_t k = (size_t)act_in[i];
		if (k == so) continue;
		act_out[i - (k > so)] = (int32_t)k;
		if (k == su) continue;
		const double v = ((D[sa * n + k] + D[sb * n + k]) - d) * 0.5;
		D[su * n + k] = v;
		D[k * n + su] = v;
	}
	if (threadIdx.x == 0) {
		D[su * n + su] = 0.0;
		id[su] = (int32_t)(n + step);
	}
}

// The last record: the three remaining nodes x < y < z by id (r = 3), or the two leaves of n = 2.
__global__ void k_nj_final(const double *__restrict__ D, uint32_t n, const int32_t *__restrict__ lists, uint32_t cur,
						   uint32_t r, andi_hip_nj_join *__restrict__ rec, uint32_t nrec) {
	if (threadIdx.x != 0) return;
	const size_t rep = blockIdx.y;
	D += rep * n * n, rec += rep * nrec + (nrec - 1);
	const int32_t *act = lists + rep * 3 * n + cur, *id = lists + rep * 3 * n + 2 * (size_t)n;
	andi_hip_nj_join j;
	j.pad = 0;
	if (r == 2) {
		const double h = D[(size_t)act[0] * n + act[1]] * 0.5;
		j.a = id[act[0]], j.b = id[act[1]], j.c = -1;
		j.la = h, j.lb = h, j.lc = 0.0;
	} else {
		int32_t s[3] = {act[0], act[1], act[2]};
		for (int a = 0; a < 2; ++a) // (by id)
			for (int b = 0; b < 2 - a; ++b)
				if (id[s[b]] > id[s[b + 1]]) {
					const int32_t t = s[b];
					s[b] = s[b + 1], s[b + 1] = t;
				}
		const double xy = D[(size_t)s[0] * n + s[1]], xz = D[(size_t)s[0] * n + s[2]], yz = D[(size_t)s[1] * n + s[2]];
		j.a = id[s[0]], j.b = id[s[1]], j.c = id[s[2]];
		j.la = ((xy + xz) - yz) * 0.5;
		j.lb = ((xy + yz) - xz) * 0.5;
		j.lc = ((xz + yz) - xy) * 0.5;
	}
	*rec = j;
}

uint64_t tiles_of(uint32_t r) {
	const uint64_t t = (r + TILE - 1) / TILE;
	return t * (t + 1) / 2;
}

constexpr unsigned long long NOT_BAD = ~0ull;
constexpr size_t GROUP_BYTES = (size_t)4 << 30; // andi_hip_nj_batch: device memory of a group of replicates, at most (one always fits)

// device bytes of one replicate: D, R, the lists, the tile results, the records, the bad word
size_t replicate_bytes(size_t n) {
	const size_t nrec = n == 2 ? 1 : n - 2;
	return n * n * sizeof(double) + n * sizeof(double) + 3 * n * sizeof(int32_t) + tiles_of((uint32_t)n) * sizeof(Cand) +
		   nrec * sizeof(andi_hip_nj_join) + sizeof(unsigned long long);
}

// the buffers of a group of g replicates of n x n, one replicate after the other in each
struct NjBuffers {
	double *D = nullptr, *R = nullptr;
	int32_t *lists = nullptr; // per replicate: two act lists, the ids
	Cand *part = nullptr;
	andi_hip_nj_join *rec = nullptr;
	unsigned long long *bad = nullptr;
};

// (the caller has waited for the stream)
void nj_free(NjBuffers &b) {
	for (void *p : {(void *)b.D, (void *)b.R, (void *)b.lists, (void *)b.part, (void *)b.rec, (void *)b.bad})
		if (p) (void)andi_arena::dev_free(p, false);
	b = NjBuffers{};
}

hipError_t nj_alloc(NjBuffers &b, size_t n, size_t g) {
	const size_t nrec = n == 2 ? 1 : n - 2;
	hipError_t e = dmalloc(&b.D, g * n * n);
	if (e == hipSuccess) e = dmalloc(&b.R, g * n);
	if (e == hipSuccess) e = dmalloc(&b.lists, g * 3 * n);
	if (e == hipSuccess) e = dmalloc(&b.part, g * tiles_of((uint32_t)n));
	if (e == hipSuccess) e = dmalloc(&b.rec, g * nrec);
	if (e == hipSuccess) e = dmalloc(&b.bad, g);
	return e;
}

// Neighbor-joining of g matrices (host, one after the other; D == nullptr: their upper triangles are in b.D already, left
// there by kernels on the context's stream) in buffers for at least g; D_out, if given, receives the g matrices as
// k_nj_init leaves them (mirrored, diagonal +0.0), copied before the first join step: bad[k] receives replicate k's
// first non-finite entry (i * n + j) or NOT_BAD, joins the records of all g when at least one matrix is usable -- and
// nothing when none is.  A bad replicate among good ones is NOT kept out of the step kernels: better() and none() make
// every pick a real pair of active slots whatever the values in D are (every index comes from the lists and the ids,
// never from a distance), so its steps run like any other's on NaN and inf, fault nothing, and leave records the caller
// throws away (andi_hip_nj_batch zeroes them).  Synchronous; the one host synchronisation before the steps is the read of
// the bad words, none between steps.
hipError_t nj_group(andi_hip_ctx *ctx, const NjBuffers &b, const double *D, uint32_t N, uint32_t g, andi_hip_nj_join *joins,
					unsigned long long *bad, double *D_out = nullptr) {
	const size_t n = N, nrec = n == 2 ? 1 : n - 2;
	const uint32_t parts = (uint32_t)tiles_of(N);
	hipStream_t st = ctx->stream;
	hipError_t e = D ? hipMemcpyAsync(b.D, D, g * n * n * sizeof(double), hipMemcpyHostToDevice, st) : hipSuccess;
	if (e == hipSuccess) e = hipMemsetAsync(b.bad, 0xff, g * sizeof *bad, st);
	if (e == hipSuccess) {
		k_nj_init<<<dim3(N, g), 256, 0, st>>>(b.D, N, b.lists, b.bad);
		e = hipGetLastError();
	}
	if (e == hipSuccess && D_out) e = hipMemcpyAsync(D_out, b.D, g * n * n * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(bad, b.bad, g * sizeof *bad, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return e;
	bool any_good = false;
	for (uint32_t k = 0; k < g; ++k) any_good |= bad[k] == NOT_BAD;
	if (!any_good) return hipSuccess;
	uint32_t cur = 0; // where in a replicate's lists the current act list starts: 0 or n
	for (uint32_t s = 0; e == hipSuccess && n >= 4 && s < N - 3; ++s) {
		const uint32_t r = N - s;
		const uint64_t nb = tiles_of(r);
		k_nj_rowsum<<<dim3((r + 3) / 4, g), 256, 0, st>>>(b.D, N, b.lists, cur, r, b.R);
		k_nj_argmin<<<dim3((unsigned)nb, g), 256, 0, st>>>(b.D, N, b.lists, cur, r, b.R, b.part, parts);
		k_nj_join<<<dim3(1, g), JOIN_THREADS, 0, st>>>(b.D, N, b.lists, cur, r, b.R, b.part, parts, (uint32_t)nb, b.rec,
														(uint32_t)nrec, s);
		e = hipGetLastError();
		cur = N - cur;
	}
	if (e == hipSuccess) {
		k_nj_final<<<dim3(1, g), 64, 0, st>>>(b.D, N, b.lists, cur, n == 2 ? 2 : 3, b.rec, (uint32_t)nrec);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(joins, b.rec, g * nrec * sizeof *joins, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	return e;
}

// The buffers of andi_hip_nj_batch's group: as many replicates as GROUP_BYTES hold (nj_group_size, api_internal.h), as
// there are; G receives the group's size.
hipError_t nj_alloc_group(NjBuffers &b, size_t n, size_t count, size_t &G) {
	G = nj_group_size(GROUP_BYTES, replicate_bytes(n));
	if (G > count) G = count;
	hipError_t e = nj_alloc(b, n, G);
	while (e != hipSuccess && G > 1) { // the memory is not there: smaller groups, down to the one matrix andi_hip_nj needs too
		nj_free(b);
		(void)hipGetLastError();
		G = (G + 1) / 2;
		e = nj_alloc(b, n, G);
	}
	return e;
}

} // namespace

int andi_hip_nj(andi_hip_ctx *ctx, const double *D, size_t n, andi_hip_nj_join *joins) {
	if (!ctx || !D || !joins || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj: bad arguments (ctx, D and joins must be given, 2 <= n <= 65535)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	NjBuffers b;
	unsigned long long bad = NOT_BAD;
	hipError_t e = nj_alloc(b, n, 1);
	if (e == hipSuccess) e = nj_group(ctx, b, D, (uint32_t)n, 1, joins, &bad);
	(void)hipStreamSynchronize(ctx->stream); // (an error exit: nothing in flight uses the buffers below)
	nj_free(b);
	if (e != hipSuccess) return fail(ctx, "andi_hip_nj", e);
	if (bad != NOT_BAD) {
		const size_t i = (size_t)(bad / n), j = (size_t)(bad % n);
		char msg[160];
		snprintf(msg, sizeof msg, "andi_hip_nj: D[%zu][%zu] is not finite (%g)", i, j, D[i * n + j]);
		ctx->err = msg;
		return 1;
	}
	return 0;
}

int andi_hip_nj_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, andi_hip_nj_join *joins, int64_t *bad) {
	if (!ctx || !D || !joins || !bad || count == 0 || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj_batch: bad arguments (ctx, D, joins and bad must be given, count >= 1, 2 <= n <= 65535)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t nrec = n == 2 ? 1 : n - 2;
	NjBuffers b;
	size_t G = 0;
	hipError_t e = nj_alloc_group(b, n, count, G);
	std::vector<unsigned long long> hb(G);
	for (size_t first = 0; e == hipSuccess && first < count; first += G) {
		const size_t g = count - first < G ? count - first : G;
		andi_hip_nj_join *J = joins + first * nrec;
		e = nj_group(ctx, b, D + first * n * n, (uint32_t)n, (uint32_t)g, J, hb.data());
		for (size_t k = 0; e == hipSuccess && k < g; ++k) {
			bad[first + k] = hb[k] == NOT_BAD ? -1 : (int64_t)hb[k];
			if (hb[k] != NOT_BAD) memset(J + k * nrec, 0, nrec * sizeof *J);
		}
	}
	(void)hipStreamSynchronize(ctx->stream); // (an error exit: nothing in flight uses the buffers below)
	nj_free(b);
	if (e != hipSuccess) return fail(ctx, "andi_hip_nj_batch", e);
	return 0;
}

// Draw, estimate and join on the device (include/andi_hip.h): the summed counts of every pair once (k_pair_sums; M's
// device copy goes before the groups' buffers come), then per group of replicates k_bootstrap_dist into the group's D
// and andi_hip_nj_batch's steps on it.  No replicate exists as models, and none as doubles on the host unless D asks.
int andi_hip_bootstrap_nj(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, uint64_t seed, size_t first,
						  size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D) {
	if (!ctx || !M || !joins || !bad || count == 0 || n < 2 || n > 65535 || model < 0 || model > 4 || first > 0xffffffffull ||
		count > 0xffffffffull || first + count > 0xffffffffull) {
		if (ctx)
			ctx->err = "andi_hip_bootstrap_nj: bad arguments (ctx, M, joins and bad must be given, count >= 1, 2 <= n <= 65535, "
					   "0 <= model <= 4, first + count < 2^32)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t nrec = n == 2 ? 1 : n - 2, pairs = n * (n - 1) / 2;
	hipStream_t st = ctx->stream;
	andi_hip_model *dM = nullptr;
	uint32_t *S = nullptr;
	hipError_t e = dmalloc(&S, pairs * 16);
	if (e == hipSuccess) e = dmalloc(&dM, n * n);
	if (e == hipSuccess) e = hipMemcpyAsync(dM, M, n * n * sizeof *M, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = andi_launch_pair_sums(dM, S, (uint32_t)n, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	else (void)hipStreamSynchronize(st);
	(void)andi_arena::dev_free(dM, false);
	NjBuffers b;
	size_t G = 0;
	if (e == hipSuccess) e = nj_alloc_group(b, n, count, G);
	std::vector<unsigned long long> hb(G);
	for (size_t done = 0; e == hipSuccess && done < count; done += G) {
		const size_t g = count - done < G ? count - done : G;
		andi_hip_nj_join *J = joins + done * nrec;
		e = andi_launch_bootstrap_dist(S, b.D, (uint32_t)n, model, (uint32_t)(first + done), (uint32_t)g, seed, st);
		if (e == hipSuccess) e = nj_group(ctx, b, nullptr, (uint32_t)n, (uint32_t)g, J, hb.data(), D ? D + done * n * n : nullptr);
		for (size_t k = 0; e == hipSuccess && k < g; ++k) {
			bad[done + k] = hb[k] == NOT_BAD ? -1 : (int64_t)hb[k];
			if (hb[k] != NOT_BAD) memset(J + k * nrec, 0, nrec * sizeof *J);
		}
	}
	(void)hipStreamSynchronize(st); // (an error exit: nothing in flight uses the buffers below)
	nj_free(b);
	(void)andi_arena::dev_free(S, false);
	if (e != hipSuccess) return fail(ctx, "andi_hip_bootstrap_nj", e);
	return 0;
}
