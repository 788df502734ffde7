// place.hip — distance-based placement of queries on a neighbor-joining tree on the device (andi_hip_place,
// include/andi_hip.h): for every (query, edge) the least-squares point on the edge and its error, bit for bit the contract
// in andi_hip.h (tests/place_model.py restates it in NumPy), and per query the edge with the least error.
//
// The form is the O(n) one per (query, edge) -- n^2 per query -- not the O(n) tree recurrences per query: those offer one
// thread per query and subtract sums of nearly equal size; this one has a thread per (query, edge), every sum in one
// fixed order, and a table that is built once per call:
//   k_sets     (nj_sets.h) the leaf set below every pair node: below(v, i) is bit i of the set of v; a leaf's own edge
//              holds its leaf alone;
//   k_paths    (tree_paths.h) T[v][i] = below(v, i) ? h(v, i) : h(parent(v), i), the length from the endpoint of edge v
//              the contract measures leaf i from, one thread per leaf;
//   k_weights  one block per query: w once per (query, leaf) -- the division stays out of the hot loop --, the number of
//              usable leaves and the first usable leaf at distance 0.0 (FM);
//   k_place    the hot path.  A block is ET = 64 edges (the lanes) x QT = 4 queries (the wavefronts).  The leaves pass
//              through LDS in ascending tiles of LT = 64: the tile of T (64 x 64 doubles, rows padded to 65 so that the
//              lanes reading one column hit distinct banks) serves the four queries, the tile of distances and weights
//              (a wavefront reads one address: a broadcast) serves the 64 edges.  Both passes in one launch; the thread
//              adds in ascending i.  An unusable leaf is skipped by a branch the whole wavefront takes: no 0 * inf
//              reaches a sum;
//   k_choose   one wavefront per query: the least (err, edge) over the edges, a NaN last.
// The queries are taken in groups, sized by the rule of the replicates' groups (nj_group_size, api_internal.h) with this
// call's budget, PLACE_GROUP_BYTES of device memory, and its own test hook, ANDI_PLACE_GROUP; a group's launches follow
// the one before on the context's stream, and one synchronisation ends the call.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nj_sets.h"
#include "tree_paths.h"

static_assert(sizeof(andi_hip_placement) == 32, "andi_hip_placement: edge, used, three doubles");

namespace {

constexpr int ET = 64;      // k_place: edges of a block (the lanes of a wavefront)
constexpr int QT = 4;       //          queries of a block (its wavefronts)
constexpr int LT = 64;      //          leaves of a tile: one word of a leaf set
constexpr int PAD = LT + 1; //          a row of the tile of T in LDS, in doubles: lane l reads bank (2 * 65 * l + 2 * i) % 64

// what k_weights leaves of a query: the usable leaves, the first usable leaf at distance 0.0 under FM or -1
struct QueryInfo {
	uint32_t used;
	int32_t zero;
};

// Block q: w[q][i], +0.0 for a leaf that is not usable (k_place skips it by its distance, not by this value).
__global__ __launch_bounds__(256) void k_weights(const double *__restrict__ D, uint32_t n, int method, double *__restrict__ w,
												 QueryInfo *__restrict__ info) {
	const size_t q = blockIdx.x;
	const double *row = D + q * n;
	uint32_t used = 0, zero = ~0u;
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		const double d = row[i];
		double wi = 0.0;
		if (__builtin_fabs(d) < __builtin_inf()) {
			++used;
			wi = method == ANDI_PLACE_FM ? 1.0 / (d * d) : 1.0;
			if (method == ANDI_PLACE_FM && d == 0.0 && i < zero) zero = i;
		}
		w[q * n + i] = wi;
	}
	__shared__ uint32_t su[4], sz[4];
	for (int m = 32; m > 0; m >>= 1) {
		used += __shfl_xor(used, m);
		const uint32_t o = __shfl_xor(zero, m);
		zero = o < zero ? o : zero;
	}
	if ((threadIdx.x & 63) == 0) su[threadIdx.x >> 6] = used, sz[threadIdx.x >> 6] = zero;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t z = sz[0];
		for (int k = 1; k < 4; ++k) z = sz[k] < z ? sz[k] : z;
		info[q] = QueryInfo{su[0] + su[1] + su[2] + su[3], z == ~0u ? -1 : (int32_t)z};
	}
}

__device__ inline double pos(double a) { return a > 0 ? a : 0.0; }
// a orders before b: by value, a NaN after every number
__device__ inline bool less_nan_last(double a, double b) { return a < b || (!__builtin_isnan(a) && __builtin_isnan(b)); }

__device__ inline double objective(double WA, double WB, double s, double t, double p, double x) {
	const double e = (p + x) - s, f = (p - x) - t;
	return WA * (e * e) + WB * (f * f);
}

// the contract's solve: (p, x) of an edge whose two sums of weights are not 0.0
__device__ inline void solve(double WA, double UA, double WB, double UB, double Lc, double &p, double &x) {
	const double s = UA / WA, t = UB / WB, W = WA + WB;
	const double p0 = (s + t) * 0.5, x0 = (s - t) * 0.5;
	if (p0 >= 0 && x0 >= 0 && x0 <= Lc) {
		p = p0, x = x0;
		return;
	}
	const double c = ((WA * s) - (WB * t)) / W;
	const double cp[3] = {pos(((WA * s) + (WB * t)) / W), pos(((WA * (s - Lc)) + (WB * (t + Lc))) / W), 0.0};
	const double cx[3] = {0.0, Lc, c > 0 ? (c < Lc ? c : Lc) : 0.0};
	p = cp[0], x = cx[0];
	double best = objective(WA, WB, s, t, p, x);
	for (int k = 1; k < 3; ++k) {
		const double q = objective(WA, WB, s, t, cp[k], cx[k]);
		if (less_nan_last(q, best)) best = q, p = cp[k], x = cx[k];
	}
}

// The tile of leaves from i0 on into LDS: T's rows v0 ... v0 + 63 (0.0 beyond the edges and the leaves), the distances and
// weights of queries q0 ... q0 + 3 (a NaN, not usable, beyond the queries and the leaves).  All 256 threads.
__device__ inline void stage(const double *__restrict__ T, const double *__restrict__ D, const double *__restrict__ Wt,
							 uint32_t n, uint32_t E, uint32_t g, uint32_t v0, uint32_t q0, uint32_t i0, double *sT, double *sd,
							 double *sw) {
	const uint32_t col = threadIdx.x & 63, i = i0 + col;
	for (uint32_t row = threadIdx.x >> 6; row < ET; row += 4) {
		const uint32_t v = v0 + row;
		sT[row * PAD + col] = v < E && i < n ? T[(size_t)v * n + i] : 0.0;
	}
	const uint32_t q = q0 + (threadIdx.x >> 6);
	const bool in = q < g && i < n;
	sd[threadIdx.x] = in ? D[(size_t)q * n + i] : __builtin_nan("");
	sw[threadIdx.x] = in ? Wt[(size_t)q * n + i] : 0.0;
}

// Thread = (edge v0 + lane, query q0 + wavefront): err, x, p of the edge for the query, into [q][v] of the three outputs.
__global__ __launch_bounds__(ET *QT) void k_place(const double *__restrict__ T, const uint64_t *__restrict__ sets,
												  const double *__restrict__ len, const double *__restrict__ D,
												  const double *__restrict__ Wt, const QueryInfo *__restrict__ info, uint32_t n,
												  uint32_t W, uint32_t E, uint32_t g, double *__restrict__ err_out,
												  double *__restrict__ x_out, double *__restrict__ p_out) {
	__shared__ double sT[ET * PAD];
	__shared__ double sd[QT * LT], sw[QT * LT];
	const uint32_t lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
	const uint32_t v0 = blockIdx.x * ET, q0 = blockIdx.y * QT;
	const uint32_t v = v0 + lane, q = q0 + wq;
	const bool live = v < E && q < g;
	const double L = v < E ? len[v] : 0.0, Lc = L > 0 ? L : 0.0;
	const double *myT = sT + lane * PAD, *myd = sd + wq * LT, *myw = sw + wq * LT;
	const double inf = __builtin_inf();

	double WA = 0.0, UA = 0.0, WB = 0.0, UB = 0.0;
	for (uint32_t i0 = 0, tile = 0; i0 < n; i0 += LT, ++tile) {
		stage(T, D, Wt, n, E, g, v0, q0, i0, sT, sd, sw);
		__syncthreads();
		if (live) {
			const uint64_t below = child_word(sets, n, W, tile, (int32_t)v);
			const uint32_t cnt = n - i0 < LT ? n - i0 : LT;
			for (uint32_t i = 0; i < cnt; ++i) {
				const double d = myd[i];
				if (!(__builtin_fabs(d) < inf)) continue; // (the whole wavefront: one query)
				const double w = myw[i], u = d - myT[i];
				if ((below >> i) & 1) {
					WA += w;
					UA += w * u;
				} else {
					WB += w;
					UB += w * (u - L);
				}
			}
		}
		__syncthreads();
	}
	const bool cand = !(WA == 0.0 || WB == 0.0);
	double p = 0.0, x = 0.0;
	if (live && cand) solve(WA, UA, WB, UB, Lc, p, x);
	const double px = p + x, pl = p + (L - x);
	double err = 0.0;
	for (uint32_t i0 = 0, tile = 0; i0 < n; i0 += LT, ++tile) {
		stage(T, D, Wt, n, E, g, v0, q0, i0, sT, sd, sw);
		__syncthreads();
		if (live && cand) {
			const uint64_t below = child_word(sets, n, W, tile, (int32_t)v);
			const uint32_t cnt = n - i0 < LT ? n - i0 : LT;
			for (uint32_t i = 0; i < cnt; ++i) {
				const double d = myd[i];
				if (!(__builtin_fabs(d) < inf)) continue;
				const double m = ((below >> i) & 1 ? px : pl) + myT[i];
				const double r = d - m;
				err += myw[i] * (r * r);
			}
		}
		__syncthreads();
	}
	if (!live) return;
	if (!cand) err = inf;
	const int32_t zero = info[q].zero;
	if (zero >= 0) err = v == (uint32_t)zero ? 0.0 : inf, x = 0.0, p = 0.0; // the query is that leaf
	const size_t at = (size_t)q * E + v;
	err_out[at] = err, x_out[at] = x, p_out[at] = p;
}

// One wavefront per query: the edge of the least err, ties to the smaller edge, a NaN after every number.
__global__ __launch_bounds__(256) void k_choose(const double *__restrict__ err, const double *__restrict__ xs,
												const double *__restrict__ ps, const QueryInfo *__restrict__ info, uint32_t E,
												uint32_t g, andi_hip_placement *__restrict__ out) {
	const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (q >= g) return;
	const double *row = err + (size_t)q * E;
	double best = __builtin_nan("");
	uint32_t bv = ~0u; // (no edge yet: any edge orders before it)
	for (uint32_t v = lane; v < E; v += 64) {
		const double e = row[v];
		if (bv == ~0u || less_nan_last(e, best)) best = e, bv = v; // (ascending v: on a tie the earlier one stays)
	}
	for (int m = 32; m > 0; m >>= 1) {
		const double oe = __shfl_xor(best, m);
		const uint32_t ov = __shfl_xor(bv, m);
		const bool same = oe == best || (__builtin_isnan(oe) && __builtin_isnan(best));
		if (ov != ~0u && (bv == ~0u || less_nan_last(oe, best) || (same && ov < bv))) best = oe, bv = ov;
	}
	if (lane != 0) return;
	andi_hip_placement r;
	r.used = info[q].used;
	if (bv == ~0u || !(best < __builtin_inf())) {
		r.edge = -1, r.distal = 0.0, r.pendant = 0.0, r.err = __builtin_inf();
	} else {
		r.edge = (int32_t)bv, r.distal = xs[(size_t)q * E + bv], r.pendant = ps[(size_t)q * E + bv], r.err = best;
	}
	out[q] = r;
}

constexpr size_t PLACE_GROUP_BYTES = (size_t)1 << 30; // device memory of a group of queries, at most (one always fits)

// device bytes of one query: its distances and weights, err, x and p of every edge, its info and its record
size_t query_bytes(size_t n) {
	return 2 * n * sizeof(double) + 3 * (2 * n - 3) * sizeof(double) + sizeof(QueryInfo) + sizeof(andi_hip_placement);
}

} // namespace

int andi_hip_place(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, size_t nq, int method,
				   andi_hip_placement *out, double *per_err, double *per_x, double *per_p) {
	if (!ctx || !tree || !D || !out || nq == 0 || n < 3 || n > 65535 || (method != ANDI_PLACE_OLS && method != ANDI_PLACE_FM)) {
		if (ctx)
			ctx->err = "andi_hip_place: bad arguments (ctx, tree, D and out must be given, nq >= 1, 3 <= n <= 65535, method OLS "
					   "or FM)";
		return 1;
	}
	const size_t E = 2 * n - 3, C = E, nsets = n - 3, W = (n + 63) / 64;
	for (size_t s = 0; s + 2 < n; ++s) {
		const double l[3] = {tree[s].la, tree[s].lb, s + 3 == n ? tree[s].lc : 0.0};
		for (int k = 0; k < 3; ++k)
			if (!std::isfinite(l[k])) {
				char msg[160];
				snprintf(msg, sizeof msg, "andi_hip_place: a branch length of the tree's record %zu is not finite", s);
				ctx->err = msg;
				return 1;
			}
	}
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> kids(nsets ? nsets : 1);
	if (!records_ok(tree, n, seen.data(), kids.data())) {
		ctx->err = "andi_hip_place: the tree's records are not those of andi_hip_nj";
		return 1;
	}
	std::vector<int32_t> par(E);
	std::vector<double> len(E);
	for (size_t s = 0; s + 2 < n; ++s) {
		const bool last = s + 3 == n;
		const int32_t ch[3] = {tree[s].a, tree[s].b, tree[s].c};
		const double l[3] = {tree[s].la, tree[s].lb, tree[s].lc};
		for (int k = 0; k < (last ? 3 : 2); ++k) par[ch[k]] = (int32_t)(last ? C : n + s), len[ch[k]] = l[k];
	}

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the queries of a group: at most what k_place's grid takes as its second dimension, QT queries a block
	size_t G = nj_group_size(KNOB_PLACE_GROUP, (size_t)65535 * QT, PLACE_GROUP_BYTES, query_bytes(n));
	if (G > nq) G = nq;
	const uint32_t N = (uint32_t)n, Ed = (uint32_t)E, Wd = (uint32_t)W;
	hipStream_t st = ctx->stream;
	DevScope dev(st);
	double *T = nullptr, *dlen = nullptr, *dD = nullptr, *dw = nullptr, *derr = nullptr, *dx = nullptr, *dp = nullptr;
	int32_t *dpar = nullptr;
	int2 *dkids = nullptr;
	uint64_t *sets = nullptr;
	QueryInfo *info = nullptr;
	andi_hip_placement *dout = nullptr;
	dev.alloc(&T, E * n);
	if (dev.err != hipSuccess) {
		char msg[200];
		snprintf(msg, sizeof msg, "andi_hip_place: the table of path lengths needs %zu bytes of device memory: %s",
				 E * n * sizeof(double), hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	dev.alloc(&dpar, E), dev.alloc(&dlen, E), dev.alloc(&dkids, nsets ? nsets : 1), dev.alloc(&sets, nsets ? nsets * W : 1);
	dev.alloc(&dD, G * n), dev.alloc(&dw, G * n), dev.alloc(&derr, G * E), dev.alloc(&dx, G * E), dev.alloc(&dp, G * E);
	dev.alloc(&info, G), dev.alloc(&dout, G);
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dpar, par.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dlen, len.data(), E * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess && nsets) e = hipMemcpyAsync(dkids, kids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		if (nsets) k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, (uint32_t)nsets, Wd, sets);
		k_paths<<<(N + 63) / 64, 64, 0, st>>>(dpar, dlen, sets, N, Wd, T);
		e = hipGetLastError();
	}
	for (size_t first = 0; e == hipSuccess && first < nq; first += G) {
		const size_t g = nq - first < G ? nq - first : G;
		const uint32_t gd = (uint32_t)g;
		e = hipMemcpyAsync(dD, D + first * n, g * n * sizeof(double), hipMemcpyHostToDevice, st);
		if (e != hipSuccess) break;
		k_weights<<<gd, 256, 0, st>>>(dD, N, method, dw, info);
		k_place<<<dim3((Ed + ET - 1) / ET, (gd + QT - 1) / QT), ET * QT, 0, st>>>(T, sets, dlen, dD, dw, info, N, Wd, Ed, gd, derr,
																					  dx, dp);
		k_choose<<<(gd + 3) / 4, 256, 0, st>>>(derr, dx, dp, info, Ed, gd, dout);
		e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(out + first, dout, g * sizeof *out, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess && per_err) e = hipMemcpyAsync(per_err + first * E, derr, g * E * sizeof(double), hipMemcpyDeviceToHost, st);
		if (e == hipSuccess && per_x) e = hipMemcpyAsync(per_x + first * E, dx, g * E * sizeof(double), hipMemcpyDeviceToHost, st);
		if (e == hipSuccess && per_p) e = hipMemcpyAsync(per_p + first * E, dp, g * E * sizeof(double), hipMemcpyDeviceToHost, st);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_place", e);
	return 0;
}
