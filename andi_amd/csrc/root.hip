// root.hip — the root of a neighbor-joining tree on the device (andi_hip_root, include/andi_hip.h): minimal ancestor
// deviation (MAD: Tria, Landan and Dagan 2017) and the midpoint of the longest path, bit for bit the contract in andi_hip.h
// (tests/root_model.py restates it in NumPy).
//
// MAD asks of every edge v the point x on it that balances the leaf pairs straddling it best, and then the sum SS of the
// squared deviations of ALL pairs b < c under a root at that point: (2n - 3) * n(n - 1)/2 pair visits, each with a division,
// twice.  The table is andi_hip_place's: the leaf sets (k_sets, nj_sets.h) and T[v][i] (k_paths, tree_paths.h).  Row b of T,
// b a leaf, is leaf b's own edge: T[b][c] + len(b) is the path length p(b, c), so a leaf's distances to all others are one
// contiguous row, and no n x n matrix is kept beside the table.
//   k_rows     one block per leaf b: the used pairs (b, c), c > b, and the first of the greatest p among them;
//   k_far      one wavefront: the number of used pairs of the tree and the first pair of the greatest p (the midpoint's);
//   k_root<1>  the hot path, k_place's tiling.  A block is ET = 64 edges (the lanes) x BT = 4 leaves b (the wavefronts).
//              The leaves c > b pass through LDS in ascending tiles of LT = 64: the tile of T (64 x 64 doubles, rows padded
//              to 65) serves the four b, the tile of p(b, .) and 1 / (p * p) (a wavefront reads one address: a broadcast)
//              serves the 64 edges.  A pair that is not used -- c <= b, past the leaves, p not finite or p <= 0 -- is a
//              NaN in the tile and skipped by a branch the whole wavefront takes; which side of the edge b and c are on
//              comes from the sets, and a pair on one side adds +0.0 by a select (the sums start at +0.0 and never turn
//              -0.0, so that is no operation).  The thread leaves the sums N and W of (v, b) over c ascending;
//   k_fold     one thread per edge: the sums of the group's leaves b are added, b ascending, to the edge's running sums;
//   k_solve    one thread per edge: x from N and W;
//   k_root<2>  the same tiling, SS of (v, b) over c ascending; k_fold again;
//   k_choose   one wavefront: the edge of the least SS, and the least SS among the others.
// The leaves b are taken in groups, sized by the rule of the replicates' groups (nj_group_size, api_internal.h) with this
// call's budget, ROOT_GROUP_BYTES of device memory, and its own test hook, ANDI_ROOT_GROUP.  A sum of (v, b) does not
// know its group, and k_fold adds the groups' sums in the order of b: the results do not depend on the grouping.  Every
// launch follows the one before on the context's stream, and one synchronisation ends the call.  The midpoint's walk along
// the path is host code.
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

static_assert(sizeof(andi_hip_root_result) == 48, "andi_hip_root_result: edge, pad, two doubles, pairs, a double, two leaves");

namespace {

constexpr int ET = 64;      // k_root: edges of a block (the lanes of a wavefront)
constexpr int BT = 4;       //         leaves b of a block (its wavefronts)
constexpr int LT = 64;      //         leaves c of a tile: one word of a leaf set
constexpr int PAD = LT + 1; //         a row of the tile of T in LDS, in doubles: lane l reads bank (2 * 65 * l + 2 * i) % 64

// what k_far and k_choose leave of a tree
struct RootDev {
	unsigned long long pairs; // used pairs
	double p;                 // the greatest p of a used pair, of the pair (b, c); NaN, ~0u, ~0u without a used pair
	uint32_t b, c;
	int32_t edge; // MAD's
	uint32_t pad;
	double x, ss, ss_second;
};

// a orders before b: by value, a NaN after every number
__device__ inline bool less_nan_last(double a, double b) { return a < b || (!__builtin_isnan(a) && __builtin_isnan(b)); }

// p(b, c) of the leaves b != c, or a NaN if the pair is not used
__device__ inline double pair_p(const double *__restrict__ T, const double *__restrict__ len, uint32_t n, uint32_t b, uint32_t c) {
	const double p = T[(size_t)b * n + c] + len[b];
	return p > 0.0 && p < __builtin_inf() ? p : __builtin_nan("");
}

// Block b: the number of used pairs (b, c), c > b, and the first c of the greatest p among them (~0u: none).
__global__ __launch_bounds__(256) void k_rows(const double *__restrict__ T, const double *__restrict__ len, uint32_t n,
											   uint32_t *__restrict__ cnt, double *__restrict__ far_p, uint32_t *__restrict__ far_c) {
	const uint32_t b = blockIdx.x;
	uint32_t used = 0, bc = ~0u;
	double best = 0.0;
	for (uint32_t c = b + 1 + threadIdx.x; c < n; c += blockDim.x) {
		const double p = pair_p(T, len, n, b, c);
		if (!(p > 0.0)) continue;
		++used;
		if (bc == ~0u || p > best) best = p, bc = c; // (ascending c: on a tie the earlier one stays)
	}
	__shared__ uint32_t su[4], sc[4];
	__shared__ double sp[4];
	for (int m = 32; m > 0; m >>= 1) {
		used += __shfl_xor(used, m);
		const double op = __shfl_xor(best, m);
		const uint32_t oc = __shfl_xor(bc, m);
		if (oc != ~0u && (bc == ~0u || op > best || (op == best && oc < bc))) best = op, bc = oc;
	}
	if ((threadIdx.x & 63) == 0) su[threadIdx.x >> 6] = used, sc[threadIdx.x >> 6] = bc, sp[threadIdx.x >> 6] = best;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int k = 1; k < 4; ++k) {
			used += su[k];
			if (sc[k] != ~0u && (bc == ~0u || sp[k] > best || (sp[k] == best && sc[k] < bc))) best = sp[k], bc = sc[k];
		}
		cnt[b] = used, far_p[b] = best, far_c[b] = bc;
	}
}

// One wavefront: the tree's used pairs, and the first pair in (b, c) order of the greatest p.
__global__ __launch_bounds__(64) void k_far(const uint32_t *__restrict__ cnt, const double *__restrict__ far_p,
											 const uint32_t *__restrict__ far_c, uint32_t n, RootDev *__restrict__ out) {
	const uint32_t lane = threadIdx.x;
	unsigned long long pairs = 0;
	uint32_t bb = ~0u, bc = ~0u;
	double best = 0.0;
	for (uint32_t b = lane; b < n; b += 64) {
		pairs += cnt[b];
		const uint32_t c = far_c[b];
		if (c != ~0u && (bb == ~0u || far_p[b] > best)) best = far_p[b], bb = b, bc = c; // (ascending b)
	}
	for (int m = 32; m > 0; m >>= 1) {
		pairs += __shfl_xor(pairs, m);
		const double op = __shfl_xor(best, m);
		const uint32_t ob = __shfl_xor(bb, m), oc = __shfl_xor(bc, m);
		if (ob != ~0u && (bb == ~0u || op > best || (op == best && ob < bb))) best = op, bb = ob, bc = oc;
	}
	if (lane != 0) return;
	out->pairs = pairs;
	out->p = bb == ~0u ? __builtin_nan("") : best;
	out->b = bb, out->c = bc;
	out->edge = 0, out->pad = 0, out->x = 0.0, out->ss = 0.0, out->ss_second = 0.0;
}

// The tile of leaves from i0 on into LDS: T's rows v0 ... v0 + 63 (0.0 beyond the edges and the leaves), and of the leaves
// b0 ... b0 + 3 the p of the pairs (b, c), c in the tile, and 1 / (p * p): a NaN for a pair that is not used -- c <= b, b or
// c past the leaves [b past bend], p not finite or p <= 0.  All 256 threads.
__device__ inline void stage(const double *__restrict__ T, const double *__restrict__ len, uint32_t n, uint32_t E, uint32_t bend,
							 uint32_t v0, uint32_t b0, uint32_t i0, double *sT, double *sp, double *sw) {
	const uint32_t col = threadIdx.x & 63, c = i0 + col;
	for (uint32_t row = threadIdx.x >> 6; row < ET; row += 4) {
		const uint32_t v = v0 + row;
		sT[row * PAD + col] = v < E && c < n ? T[(size_t)v * n + c] : 0.0;
	}
	const uint32_t b = b0 + (threadIdx.x >> 6);
	const double p = b < bend && c < n && c > b ? pair_p(T, len, n, b, c) : __builtin_nan("");
	sp[threadIdx.x] = p;
	sw[threadIdx.x] = 1.0 / (p * p);
}

// Thread = (edge v0 + lane, leaf b0 + wavefront), b0 = first + 4 * blockIdx.y, over the leaves c > b in ascending order.
// PASS 1: the sums N and W of the pairs (b, c) that straddle the edge, into [b - first][v] of out0 and out1.
// PASS 2: the sum SS of all pairs (b, c) under the root at xs[v], into [b - first][v] of out0.
template <int PASS>
__global__ __launch_bounds__(ET *BT) void k_root(const double *__restrict__ T, const uint64_t *__restrict__ sets,
												 const double *__restrict__ len, const double *__restrict__ xs, uint32_t n,
												 uint32_t W, uint32_t E, uint32_t first, uint32_t g, double *__restrict__ out0,
												 double *__restrict__ out1) {
	__shared__ double sT[ET * PAD];
	__shared__ double sp[BT * LT], sw[BT * LT];
	const uint32_t lane = threadIdx.x & 63, wb = threadIdx.x >> 6;
	const uint32_t v0 = blockIdx.x * ET, b0 = first + blockIdx.y * BT, bend = first + g;
	const uint32_t v = v0 + lane, b = b0 + wb;
	const bool live = v < E && b < bend;
	const double L = v < E ? len[v] : 0.0;
	const double tb = live ? T[(size_t)v * n + b] : 0.0;
	const bool sideb = live && ((child_word(sets, n, W, b >> 6, (int32_t)v) >> (b & 63)) & 1);
	const double *myT = sT + lane * PAD, *myp = sp + wb * LT, *myw = sw + wb * LT;

	double two_d = 0.0; // PASS 2: twice the distance from b to the root, for a pair that straddles the edge
	if (PASS == 2 && live) {
		const double x = xs[v];
		two_d = 2.0 * (sideb ? tb + x : tb + (L - x));
	}
	double s0 = 0.0, s1 = 0.0;
	for (uint32_t i0 = ((b0 + 1) / LT) * LT, tile = i0 / LT; i0 < n; i0 += LT, ++tile) { // (c > b0)
		stage(T, len, n, E, bend, v0, b0, i0, sT, sp, sw);
		__syncthreads();
		if (live) {
			const uint64_t below = child_word(sets, n, W, tile, (int32_t)v);
			const uint32_t cnt = n - i0 < LT ? n - i0 : LT;
			for (uint32_t i = 0; i < cnt; ++i) {
				const double p = myp[i];
				if (!(p > 0.0)) continue; // (the whole wavefront: one pair)
				const double tc = myT[i];
				const bool straddle = (bool)((below >> i) & 1) != sideb;
				if (PASS == 1) {
					const double val = (p - 2.0 * (sideb ? tb : tc)) / (p * p);
					s0 += straddle ? val : 0.0;
					s1 += straddle ? myw[i] : 0.0;
				} else {
					const double q = (straddle ? two_d : tb - tc) / p;
					const double r = straddle ? q - 1.0 : q;
					s0 += r * r;
				}
			}
		}
		__syncthreads();
	}
	if (!live) return;
	const size_t at = (size_t)(b - first) * E + v;
	out0[at] = s0;
	if (PASS == 1) out1[at] = s1;
}

// acc[v] += part[k][v] for the g leaves k of a group, in ascending order
__global__ __launch_bounds__(64) void k_fold(const double *__restrict__ part, uint32_t E, uint32_t g, double *__restrict__ acc) {
	const uint32_t v = blockIdx.x * 64 + threadIdx.x;
	if (v >= E) return;
	double a = acc[v];
	uint32_t k = 0;
	for (; k + 8 <= g; k += 8) { // (eight loads in flight; the additions stay one after the other, in the order of k)
		double p[8];
#pragma unroll
		for (int j = 0; j < 8; ++j) p[j] = part[(size_t)(k + j) * E + v];
#pragma unroll
		for (int j = 0; j < 8; ++j) a = a + p[j];
	}
	for (; k < g; ++k) a = a + part[(size_t)k * E + v];
	acc[v] = a;
}

__global__ __launch_bounds__(64) void k_solve(const double *__restrict__ N, const double *__restrict__ Wt,
											   const double *__restrict__ len, uint32_t E, double *__restrict__ xs) {
	const uint32_t v = blockIdx.x * 64 + threadIdx.x;
	if (v >= E) return;
	const double L = len[v], Lc = L > 0 ? L : 0.0, w = Wt[v];
	const double a = N[v] / (2.0 * w);
	xs[v] = w == 0.0 ? 0.0 : a > 0 ? (a < Lc ? a : Lc) : 0.0;
}

// the least (ss, edge) over the lanes' candidates: ties to the smaller edge, a NaN after every number, ~0u is no edge
__device__ inline void wave_least(double &best, uint32_t &bv) {
	for (int m = 32; m > 0; m >>= 1) {
		const double oe = __shfl_xor(best, m);
		const uint32_t ov = __shfl_xor(bv, m);
		const bool same = oe == best || (__builtin_isnan(oe) && __builtin_isnan(best));
		if (ov != ~0u && (bv == ~0u || less_nan_last(oe, best) || (same && ov < bv))) best = oe, bv = ov;
	}
}

// One wavefront: the edge of the least SS, and the least SS among the other edges.
__global__ __launch_bounds__(64) void k_choose(const double *__restrict__ ss, const double *__restrict__ xs, uint32_t E,
												RootDev *__restrict__ out) {
	const uint32_t lane = threadIdx.x;
	double best = __builtin_nan("");
	uint32_t bv = ~0u;
	for (uint32_t v = lane; v < E; v += 64) {
		const double e = ss[v];
		if (bv == ~0u || less_nan_last(e, best)) best = e, bv = v; // (ascending v: on a tie the earlier one stays)
	}
	wave_least(best, bv);
	const uint32_t chosen = bv;
	double second = __builtin_nan("");
	uint32_t sv = ~0u;
	for (uint32_t v = lane; v < E; v += 64) {
		if (v == chosen) continue;
		const double e = ss[v];
		if (sv == ~0u || less_nan_last(e, second)) second = e, sv = v;
	}
	wave_least(second, sv);
	if (lane != 0) return;
	out->edge = (int32_t)chosen, out->x = xs[chosen], out->ss = best, out->ss_second = second;
}

constexpr size_t ROOT_GROUP_BYTES = (size_t)1 << 30; // device memory of a group of leaves' sums, at most (one always fits)

// The midpoint of the path from leaf b to leaf c, p * 0.5 from b (the contract's walk): the edge that holds it and the
// distance from the edge's child end.
void midpoint_walk(const std::vector<int32_t> &par, const std::vector<double> &len, uint32_t b, uint32_t c, double p,
				   int32_t &edge, double &distal) {
	const int32_t C = (int32_t)par.size();
	std::vector<uint8_t> mark(par.size() + 1);
	for (int32_t v = (int32_t)b; v != C; v = par[v]) mark[v] = 1;
	mark[C] = 1;
	std::vector<int32_t> down; // the edges from c up to the node where the two paths meet
	int32_t top = (int32_t)c;
	for (; !mark[top]; top = par[top]) down.push_back(top);
	double rem = p * 0.5;
	for (int32_t v = (int32_t)b; v != top; v = par[v]) {
		if (rem < len[v]) {
			edge = v, distal = rem;
			return;
		}
		rem = rem - len[v];
	}
	for (size_t k = down.size(); k-- > 0;) {
		const int32_t u = down[k];
		if (rem < len[u]) {
			edge = u, distal = len[u] - rem;
			return;
		}
		rem = rem - len[u];
	}
	edge = (int32_t)c, distal = 0.0; // (rounding or negative lengths took it past c)
}

} // namespace

int andi_hip_root(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, int method, andi_hip_root_result *out, double *per_x,
				  double *per_ss) {
	if (!ctx || !tree || !out || n < 3 || n > 65535 || (method != ANDI_ROOT_MAD && method != ANDI_ROOT_MIDPOINT)) {
		if (ctx)
			ctx->err = "andi_hip_root: bad arguments (ctx, tree and out must be given, 3 <= n <= 65535, method MAD or MIDPOINT)";
		return 1;
	}
	const size_t E = 2 * n - 3, C = E, nsets = n - 3, W = (n + 63) / 64;
	for (size_t s = 0; s + 2 < n; ++s) {
		const double l[3] = {tree[s].la, tree[s].lb, s + 3 == n ? tree[s].lc : 0.0};
		for (int k = 0; k < 3; ++k)
			if (!std::isfinite(l[k])) {
				char msg[160];
				snprintf(msg, sizeof msg, "andi_hip_root: a branch length of the tree's record %zu is not finite", s);
				ctx->err = msg;
				return 1;
			}
	}
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> kids(nsets ? nsets : 1);
	if (!records_ok(tree, n, seen.data(), kids.data())) {
		ctx->err = "andi_hip_root: the tree's records are not those of andi_hip_nj";
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
	const bool mad = method == ANDI_ROOT_MAD;
	// the leaves of a group: at most what k_root's grid takes as its second dimension, BT leaves a block
	size_t G = nj_group_size(KNOB_ROOT_GROUP, (size_t)65535 * BT, ROOT_GROUP_BYTES, 2 * E * sizeof(double));
	if (G > n) G = n;
	const uint32_t N = (uint32_t)n, Ed = (uint32_t)E, Wd = (uint32_t)W;
	hipStream_t st = ctx->stream;
	DevScope dev(st);
	double *T = nullptr, *dlen = nullptr, *part0 = nullptr, *part1 = nullptr, *acc = nullptr, *dx = nullptr, *farp = nullptr;
	int32_t *dpar = nullptr;
	int2 *dkids = nullptr;
	uint64_t *sets = nullptr;
	uint32_t *cnt = nullptr, *farc = nullptr;
	RootDev *dres = nullptr;
	dev.alloc(&T, E * n);
	if (dev.err != hipSuccess) {
		char msg[200];
		snprintf(msg, sizeof msg, "andi_hip_root: the table of path lengths needs %zu bytes of device memory: %s",
				 E * n * sizeof(double), hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	dev.alloc(&dpar, E), dev.alloc(&dlen, E), dev.alloc(&dkids, nsets ? nsets : 1), dev.alloc(&sets, nsets ? nsets * W : 1);
	dev.alloc(&cnt, n), dev.alloc(&farc, n), dev.alloc(&farp, n), dev.alloc(&dres, 1);
	if (mad) dev.alloc(&part0, G * E), dev.alloc(&part1, G * E), dev.alloc(&acc, 3 * E), dev.alloc(&dx, E);
	double *accN = acc, *accW = acc + E, *accS = acc + 2 * E;
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dpar, par.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dlen, len.data(), E * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess && nsets) e = hipMemcpyAsync(dkids, kids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
	if (e == hipSuccess && mad) e = hipMemsetAsync(acc, 0, 3 * E * sizeof(double), st); // (+0.0)
	if (e == hipSuccess) {
		if (nsets) k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, (uint32_t)nsets, Wd, sets);
		k_paths<<<(N + 63) / 64, 64, 0, st>>>(dpar, dlen, sets, N, Wd, T);
		k_rows<<<N, 256, 0, st>>>(T, dlen, N, cnt, farp, farc);
		k_far<<<1, 64, 0, st>>>(cnt, farp, farc, N, dres);
		e = hipGetLastError();
	}
	for (int pass = 1; mad && pass <= 2; ++pass) {
		for (size_t first = 0; e == hipSuccess && first < n; first += G) {
			const uint32_t g = (uint32_t)(n - first < G ? n - first : G);
			const dim3 grid((Ed + ET - 1) / ET, (g + BT - 1) / BT);
			if (pass == 1) {
				k_root<1><<<grid, ET * BT, 0, st>>>(T, sets, dlen, nullptr, N, Wd, Ed, (uint32_t)first, g, part0, part1);
				k_fold<<<(Ed + 63) / 64, 64, 0, st>>>(part0, Ed, g, accN);
				k_fold<<<(Ed + 63) / 64, 64, 0, st>>>(part1, Ed, g, accW);
			} else {
				k_root<2><<<grid, ET * BT, 0, st>>>(T, sets, dlen, dx, N, Wd, Ed, (uint32_t)first, g, part0, nullptr);
				k_fold<<<(Ed + 63) / 64, 64, 0, st>>>(part0, Ed, g, accS);
			}
			e = hipGetLastError();
		}
		if (e == hipSuccess) {
			if (pass == 1) k_solve<<<(Ed + 63) / 64, 64, 0, st>>>(accN, accW, dlen, Ed, dx);
			else k_choose<<<1, 64, 0, st>>>(accS, dx, Ed, dres);
			e = hipGetLastError();
		}
	}
	RootDev res;
	std::vector<double> hx(mad && per_x ? E : 0), hss(mad && per_ss ? E : 0); // (the caller's arrays are written on success only)
	if (e == hipSuccess) e = hipMemcpyAsync(&res, dres, sizeof res, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && mad && per_x) e = hipMemcpyAsync(hx.data(), dx, E * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess && mad && per_ss) e = hipMemcpyAsync(hss.data(), accS, E * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_root", e);

	andi_hip_root_result r;
	memset(&r, 0, sizeof r);
	r.pairs = res.pairs;
	r.far_b = res.b == ~0u ? -1 : (int32_t)res.b, r.far_c = res.c == ~0u ? -1 : (int32_t)res.c;
	if (mad) {
		r.edge = res.edge, r.distal = res.x, r.ss = res.ss, r.ss_second = res.ss_second;
		if (per_x) memcpy(per_x, hx.data(), E * sizeof(double));
		if (per_ss) memcpy(per_ss, hss.data(), E * sizeof(double));
	} else if (res.b != ~0u) {
		midpoint_walk(par, len, res.b, res.c, res.p, r.edge, r.distal);
	}
	*out = r;
	return 0;
}
