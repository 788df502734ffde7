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
// block offsets its pointers by blockIdx.y.  andi_hip_nj is the group of one.  The host code around a group's steps --
// its size and buffers, the loop over the groups, what happens to an unusable matrix, the buffers' lifetime -- is
// rep_groups.h's, shared with linkage.hip; here are the kernels, a replicate's buffers and the step loop.
//
// BIONJ (andi_hip_tree with ANDI_TREE_BIONJ) is the same step with another join kernel: a second matrix V beside D, by the
// same slots, that k_nj_init leaves equal to D; row sums and the pick are k_nj_rowsum's and k_nj_argmin's on D alone;
// k_bionj_join sums rows a and b of V by k_nj_rowsum's chain (row_chain, two wavefronts, one row each), takes lambda from
// the two sums and writes the new node's row and column of D and of V in one pass.  V exists only for BIONJ.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "api_internal.h"
#include "bootstrap.h"
#include "nj_cand.h" // Cand, better, none, wave_min, block_min
#include "rep_groups.h"

static_assert(sizeof(andi_hip_nj_join) == 40, "andi_hip_nj_join: 3 ids, pad, 3 lengths");

namespace {

constexpr int RS_CHUNKS = 16;                // k_nj_rowsum: 16 x 64 entries of a row in flight per wavefront
constexpr int TILE = 64;                     // k_nj_argmin: 64 x 64 pairs per block, 16 rows per wavefront
constexpr int JOIN_THREADS = 1024;

// Mirror the upper triangle (row i = block i), diagonal +0.0; the first non-finite D[i][j], i < j, in row-major order
// goes to the replicate's bad word as i * n + j.  act = id = identity.  BIONJ: row i of V receives what row i of D holds
// then (only D's upper triangle is read, and no block writes it).
template <bool BIONJ>
__global__ __launch_bounds__(256) void k_nj_init(double *__restrict__ D, double *__restrict__ V, uint32_t n,
												 int32_t *__restrict__ lists, unsigned long long *bad) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, bad += rep;
	int32_t *act = lists + rep * 3 * n, *id = act + 2 * (size_t)n;
	const uint32_t i = blockIdx.x;
	double *row = D + (size_t)i * n;
	double *vrow = BIONJ ? V + rep * n * n + (size_t)i * n : nullptr;
	unsigned long long first = ~0ull;
	for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
		if (j > i) {
			const double v = row[j];
			if (!__builtin_isfinite(v) && first == ~0ull) first = (unsigned long long)i * n + j;
			if (BIONJ) vrow[j] = v;
		} else {
			const double v = j < i ? D[(size_t)j * n + i] : 0.0;
			row[j] = v;
			if (BIONJ) vrow[j] = v;
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

// the sum of row[act[k]], k = 0 .. r-1, in that order from +0.0, by one wavefront (every lane returns it).  Always inline:
// with two callers the compiler otherwise makes it a function, and k_nj_rowsum pays a call and twice the registers
__device__ __forceinline__ double row_chain(const double *__restrict__ row, const int32_t *__restrict__ act, uint32_t r, int lane) {
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
	return acc;
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
	const double acc = row_chain(D + sx * n, act, r, lane);
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

// k_nj_join for BIONJ (andi_hip_tree's contract): the same pick, record, list and ids; the new node's distances are
// weighted by lambda, which comes from the sums of rows a and b of V -- wavefront 0 chains row a, wavefront 1 row b, while
// the others wait at the barrier; the two sums go through LDS and every thread takes lambda from them by the same
// operations.  lambda is a weight only: no index and no loop bound comes from it, so a bad replicate's NaN stays harmless.
__global__ __launch_bounds__(JOIN_THREADS) void k_bionj_join(double *__restrict__ D, double *__restrict__ V, uint32_t n,
															 int32_t *__restrict__ lists, uint32_t cur, uint32_t r,
															 const double *__restrict__ R, const Cand *__restrict__ part,
															 uint32_t part_stride, uint32_t nparts, andi_hip_nj_join *__restrict__ rec,
															 uint32_t nrec, uint32_t step) {
	__shared__ double rv[2];
	const size_t rep = blockIdx.y;
	D += rep * n * n, V += rep * n * n, R += rep * n, part += rep * part_stride, rec += rep * nrec;
	const int32_t *act_in = lists + rep * 3 * n + cur;
	int32_t *act_out = lists + rep * 3 * n + (n - cur), *id = lists + rep * 3 * n + 2 * (size_t)n;
	Cand best = none();
	for (uint32_t k = threadIdx.x; k < nparts; k += blockDim.x)
		if (better(part[k], best)) best = part[k];
	best = block_min(best);
	const size_t sa = (size_t)best.sa, sb = (size_t)best.sb;
	const size_t su = sa < sb ? sa : sb, so = sa < sb ? sb : sa;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	if (wave < 2) {
		const double sum = row_chain(V + (wave ? sb : sa) * n, act_in, r, lane);
		if (lane == 0) rv[wave] = sum;
	}
	const double d = D[sa * n + sb], vab = V[sa * n + sb];
	const double la = d * 0.5 + (R[sa] - R[sb]) / (double)(2 * (r - 2)), lb = d - la;
	__syncthreads(); // the sums are there, and rows a and b of V have been read before one of them is written
	double lam = 0.5 + (rv[1] - rv[0]) / ((double)(2 * (r - 2)) * vab);
	if (vab == 0.0 || __builtin_isnan(lam)) lam = 0.5;
	if (lam < 0.0) lam = 0.0;
	if (lam > 1.0) lam = 1.0;
	const double mu = 1.0 - lam, lm = lam * mu;
	if (threadIdx.x == 0) {
		andi_hip_nj_join j;
		j.a = best.ia, j.b = best.ib, j.c = -1, j.pad = 0;
		j.la = la, j.lb = lb, j.lc = 0.0;
		rec[step] = j;
	}
	for (uint32_t i = threadIdx.x; i < r; i += blockDim.x) {
		const size_t k = (size_t)act_in[i];
		if (k == so) continue;
		act_out[i - (k > so)] = (int32_t)k;
		if (k == su) continue;
		const double dv = lam * (D[sa * n + k] - la) + mu * (D[sb * n + k] - lb);
		const double vv = (lam * V[sa * n + k] + mu * V[sb * n + k]) - lm * vab;
		D[su * n + k] = dv;
		D[k * n + su] = dv;
		V[su * n + k] = vv;
		V[k * n + su] = vv;
	}
	if (threadIdx.x == 0) {
		D[su * n + su] = 0.0;
		V[su * n + su] = 0.0;
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

size_t records_of(size_t n) { return n == 2 ? 1 : n - 2; }


// the buffers of a group of g replicates of n x n, one replicate after the other in each (rep_groups.h: alloc_group);
// V is BIONJ's second matrix and exists for that method only
struct NjBuffers {
	int method = ANDI_TREE_NJ;
	double *D = nullptr, *V = nullptr, *R = nullptr;
	int32_t *lists = nullptr; // per replicate: two act lists, the ids
	Cand *part = nullptr;
	andi_hip_nj_join *rec = nullptr;
	unsigned long long *bad = nullptr;

	explicit NjBuffers(int method_) : method(method_) {}
	bool bionj() const { return method == ANDI_TREE_BIONJ; }
	// device bytes of one replicate: D (and V), R, the lists, the tile results, the records, the bad word
	size_t replicate_bytes(size_t n) const {
		return (bionj() ? 2 : 1) * n * n * sizeof(double) + n * sizeof(double) + 3 * n * sizeof(int32_t) +
			   tiles_of((uint32_t)n) * sizeof(Cand) + records_of(n) * sizeof(andi_hip_nj_join) + sizeof(unsigned long long);
	}
	hipError_t alloc(DevScope &dev, size_t n, size_t g) {
		dev.alloc(&D, g * n * n), dev.alloc(&R, g * n), dev.alloc(&lists, g * 3 * n);
		dev.alloc(&part, g * tiles_of((uint32_t)n)), dev.alloc(&rec, g * records_of(n)), dev.alloc(&bad, g);
		if (bionj()) dev.alloc(&V, g * n * n);
		return dev.err;
	}
};

// The tree (b.method) of g matrices in buffers for at least g, between group_begin and group_end (rep_groups.h: what D,
// D_out and bad are; the init kernel is k_nj_init, an unusable entry a non-finite one): joins receives the records of all
// g when at least one matrix is usable -- and nothing when none is.  Synchronous; no host synchronisation between steps.
hipError_t nj_group(andi_hip_ctx *ctx, const NjBuffers &b, const double *D, uint32_t N, uint32_t g, andi_hip_nj_join *joins,
					unsigned long long *bad, double *D_out = nullptr) {
	const size_t n = N, nrec = records_of(n);
	const uint32_t parts = (uint32_t)tiles_of(N);
	const bool bionj = b.bionj();
	hipStream_t st = ctx->stream;
	bool any_good;
	hipError_t e = group_begin(
		st, b.D, D, n, g, b.bad, bad, D_out,
		[&] {
			if (bionj) k_nj_init<true><<<dim3(N, g), 256, 0, st>>>(b.D, b.V, N, b.lists, b.bad);
			else k_nj_init<false><<<dim3(N, g), 256, 0, st>>>(b.D, nullptr, N, b.lists, b.bad);
		},
		any_good);
	if (e != hipSuccess || !any_good) return e;
	uint32_t cur = 0; // where in a replicate's lists the current act list starts: 0 or n
	for (uint32_t s = 0; e == hipSuccess && n >= 4 && s < N - 3; ++s) {
		const uint32_t r = N - s;
		const uint64_t nb = tiles_of(r);
		k_nj_rowsum<<<dim3((r + 3) / 4, g), 256, 0, st>>>(b.D, N, b.lists, cur, r, b.R);
		k_nj_argmin<<<dim3((unsigned)nb, g), 256, 0, st>>>(b.D, N, b.lists, cur, r, b.R, b.part, parts);
		if (bionj)
			k_bionj_join<<<dim3(1, g), JOIN_THREADS, 0, st>>>(b.D, b.V, N, b.lists, cur, r, b.R, b.part, parts, (uint32_t)nb, b.rec,
																(uint32_t)nrec, s);
		else
			k_nj_join<<<dim3(1, g), JOIN_THREADS, 0, st>>>(b.D, N, b.lists, cur, r, b.R, b.part, parts, (uint32_t)nb, b.rec,
															(uint32_t)nrec, s);
		e = hipGetLastError();
		cur = N - cur;
	}
	if (e == hipSuccess) {
		k_nj_final<<<dim3(1, g), 64, 0, st>>>(b.D, N, b.lists, cur, n == 2 ? 2 : 3, b.rec, (uint32_t)nrec);
		e = hipGetLastError();
	}
	return e == hipSuccess ? group_end(st, joins, b.rec, g * nrec) : e;
}

bool method_ok(int method) { return method == ANDI_TREE_NJ || method == ANDI_TREE_BIONJ; }

// The three calls behind their argument checks; `who` is the public function the context's error names.
int tree_one(andi_hip_ctx *ctx, const char *who, const double *D, size_t n, int method, andi_hip_nj_join *joins) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	NjBuffers b(method);
	unsigned long long bad = NOT_BAD;
	hipError_t e = b.alloc(dev, n, 1);
	if (e == hipSuccess) e = nj_group(ctx, b, D, (uint32_t)n, 1, joins, &bad);
	if (e != hipSuccess) return fail(ctx, who, e);
	if (bad != NOT_BAD) {
		const Entry at = bad_entry(bad, n);
		char msg[160];
		snprintf(msg, sizeof msg, "%s: D[%zu][%zu] is not finite (%g)", who, at.i, at.j, D[at.i * n + at.j]);
		ctx->err = msg;
		return 1;
	}
	return 0;
}

int tree_many(andi_hip_ctx *ctx, const char *who, const double *D, size_t n, size_t count, int method, andi_hip_nj_join *joins,
			  int64_t *bad) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	NjBuffers b(method);
	size_t G = 0;
	hipError_t e = alloc_group(dev, b, n, count, G);
	if (e == hipSuccess)
		e = for_groups(count, G, records_of(n), joins, bad, [&](size_t first, size_t g, andi_hip_nj_join *J, unsigned long long *hb) {
			return nj_group(ctx, b, D + first * n * n, (uint32_t)n, (uint32_t)g, J, hb);
		});
	if (e != hipSuccess) return fail(ctx, who, e);
	return 0;
}

// Draw, estimate and join on the device (include/andi_hip.h): the summed counts of every pair once (k_pair_sums; M's
// device copy goes before the groups' buffers come), then per group of replicates k_bootstrap_dist into the group's D
// and tree_many's steps on it.  No replicate exists as models, and none as doubles on the host unless D asks.
int tree_bootstrap(andi_hip_ctx *ctx, const char *who, const andi_hip_model *M, size_t n, int model, int method, uint64_t seed,
				   size_t first, size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D) {
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t pairs = n * (n - 1) / 2;
	hipStream_t st = ctx->stream;
	DevScope sums(st), dev(st); // S for the whole call; M's copy, then the groups' buffers (alloc_group gives back all of its scope)
	andi_hip_model *dM = nullptr;
	uint32_t *S = nullptr;
	sums.alloc(&S, pairs * 16);
	if (sums.err == hipSuccess) dev.alloc(&dM, n * n);
	hipError_t e = sums.err != hipSuccess ? sums.err : dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dM, M, n * n * sizeof *M, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = andi_launch_pair_sums(dM, S, (uint32_t)n, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	dev.release(); // (M's copy is 650 MB at n = 3085)
	NjBuffers b(method);
	size_t G = 0;
	if (e == hipSuccess) e = alloc_group(dev, b, n, count, G);
	if (e == hipSuccess)
		e = for_groups(count, G, records_of(n), joins, bad, [&](size_t done, size_t g, andi_hip_nj_join *J, unsigned long long *hb) {
			hipError_t eg = andi_launch_bootstrap_dist(S, b.D, (uint32_t)n, model, (uint32_t)(first + done), (uint32_t)g, seed, st);
			if (eg == hipSuccess) eg = nj_group(ctx, b, nullptr, (uint32_t)n, (uint32_t)g, J, hb, D ? D + done * n * n : nullptr);
			return eg;
		});
	if (e != hipSuccess) return fail(ctx, who, e);
	return 0;
}

bool bootstrap_args_ok(const andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, size_t first, size_t count,
					   const andi_hip_nj_join *joins, const int64_t *bad) {
	return ctx && M && joins && bad && count != 0 && n >= 2 && n <= 65535 && model >= 0 && model <= 4 && first <= 0xffffffffull &&
		   count <= 0xffffffffull && first + count <= 0xffffffffull;
}

} // namespace

int andi_hip_nj(andi_hip_ctx *ctx, const double *D, size_t n, andi_hip_nj_join *joins) {
	if (!ctx || !D || !joins || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj: bad arguments (ctx, D and joins must be given, 2 <= n <= 65535)";
		return 1;
	}
	return tree_one(ctx, "andi_hip_nj", D, n, ANDI_TREE_NJ, joins);
}

int andi_hip_nj_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, andi_hip_nj_join *joins, int64_t *bad) {
	if (!ctx || !D || !joins || !bad || count == 0 || n < 2 || n > 65535) {
		if (ctx) ctx->err = "andi_hip_nj_batch: bad arguments (ctx, D, joins and bad must be given, count >= 1, 2 <= n <= 65535)";
		return 1;
	}
	return tree_many(ctx, "andi_hip_nj_batch", D, n, count, ANDI_TREE_NJ, joins, bad);
}

int andi_hip_bootstrap_nj(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, uint64_t seed, size_t first,
						  size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D) {
	if (!bootstrap_args_ok(ctx, M, n, model, first, count, joins, bad)) {
		if (ctx)
			ctx->err = "andi_hip_bootstrap_nj: bad arguments (ctx, M, joins and bad must be given, count >= 1, 2 <= n <= 65535, "
					   "0 <= model <= 4, first + count < 2^32)";
		return 1;
	}
	return tree_bootstrap(ctx, "andi_hip_bootstrap_nj", M, n, model, ANDI_TREE_NJ, seed, first, count, joins, bad, D);
}

int andi_hip_tree(andi_hip_ctx *ctx, const double *D, size_t n, int method, andi_hip_nj_join *joins) {
	if (!ctx || !D || !joins || n < 2 || n > 65535 || !method_ok(method)) {
		if (ctx) ctx->err = "andi_hip_tree: bad arguments (ctx, D and joins must be given, 2 <= n <= 65535, 0 <= method <= 1)";
		return 1;
	}
	return tree_one(ctx, "andi_hip_tree", D, n, method, joins);
}

int andi_hip_tree_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, int method, andi_hip_nj_join *joins,
						int64_t *bad) {
	if (!ctx || !D || !joins || !bad || count == 0 || n < 2 || n > 65535 || !method_ok(method)) {
		if (ctx)
			ctx->err = "andi_hip_tree_batch: bad arguments (ctx, D, joins and bad must be given, count >= 1, 2 <= n <= 65535, "
					   "0 <= method <= 1)";
		return 1;
	}
	return tree_many(ctx, "andi_hip_tree_batch", D, n, count, method, joins, bad);
}

int andi_hip_bootstrap_tree(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, int method, uint64_t seed,
							size_t first, size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D) {
	if (!bootstrap_args_ok(ctx, M, n, model, first, count, joins, bad) || !method_ok(method)) {
		if (ctx)
			ctx->err = "andi_hip_bootstrap_tree: bad arguments (ctx, M, joins and bad must be given, count >= 1, 2 <= n <= 65535, "
					   "0 <= model <= 4, 0 <= method <= 1, first + count < 2^32)";
		return 1;
	}
	return tree_bootstrap(ctx, "andi_hip_bootstrap_tree", M, n, model, method, seed, first, count, joins, bad, D);
}
