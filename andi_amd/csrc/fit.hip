// fit.hip — the branch lengths of a fixed tree refit to a distance matrix by ordinary least squares on the device
// (andi_hip_fit, include/andi_hip.h), and how well the tree explains the matrix under the refit lengths and under its own:
// bit for bit the contract in andi_hip.h (tests/fit_model.py restates it in NumPy).
//
// The least-squares length of an edge has a closed form (Rzhetsky and Nei 1993; Desper and Gascuel 2002, eq. 3) in the
// mean distances between the four subtrees around it -- two below the edge (classes 0 and 1), two above (2 and 3) --, so
// every edge asks for the sums of D over the pairs of its four classes: (2n - 3) * n(n - 1)/2 pair visits, k_root's shape
// (root.hip) without its divisions and without the table of path lengths.
//   k_mirror   one block per row: the lower triangle of D from the upper, the diagonal +0.0;
//   k_fit      the hot path, k_root's tiling.  A block is ET = 64 edges (the lanes) x BT = 4 leaves b (the wavefronts).
//              The leaves c > b pass through LDS in ascending tiles of LT = 64: the tile of D[b][.] (a wavefront reads
//              one address: a broadcast) serves the 64 edges, +0.0 where c <= b or past the leaves.  An edge's classes
//              of a tile are 64-bit words made from three words of the leaf sets -- of v's first child, of v and of the
//              node of class 2 --, and a thread keeps four sums, one a class; a pair adds D to the sum of c's class and
//              +0.0 to the others by a select (the sums start at +0.0 and never turn -0.0, so that is no operation).
//              No division, no test of the value: D was checked finite on the host.  The thread leaves the four sums
//              of (v, b) over c ascending;
//   k_fold6    one thread per edge: over the group's leaves b ascending, the four sums go to the six S_xy by b's class;
//   k_lengths  one thread per edge: the means and the closed form;
//   k_paths    (tree_paths.h) the table of path lengths under a length vector; then, n^2 work and kept simple,
//   k_resid    the residual r of every pair into a symmetric n x n matrix,
//   k_leaf     one thread per leaf i: the sum of r*r over j != i ascending, the part of it with j > i (row i of rss), and
//              the first j > i of the greatest |r|; down a column of the symmetric matrix, so a wavefront reads one run;
//   k_rows_d, k_mean, k_rows_t   the same for tss: the rows' sums of D, their mean, the rows' sums of (D - mean)^2;
//   k_record   one wavefront: the rows' sums added over b ascending, and the first pair of the greatest |r|.
// k_paths ... k_leaf run twice: under the refit lengths, which never leave the device in between, and under the records'.
// The leaves b of k_fit are taken in groups, sized by the rule of the replicates' groups (nj_group_size, api_internal.h)
// with this call's budget, FIT_GROUP_BYTES of device memory, and its own test hook, ANDI_FIT_GROUP.  A sum of (v, b) does
// not know its group, and k_fold6 adds the groups' sums in the order of b: the results do not depend on the grouping.
// Every launch follows the one before on the context's stream, and one synchronisation ends the call.
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

static_assert(sizeof(andi_hip_fit_result) == 72, "andi_hip_fit_result: six doubles, pairs, two counts, two leaves");

namespace {

constexpr int ET = 64; // k_fit: edges of a block (the lanes of a wavefront)
constexpr int BT = 4;  //        leaves b of a block (its wavefronts)
constexpr int LT = 64; //        leaves c of a tile: one word of a leaf set

// what an edge's classes are made from: the first child of v's pair record (v itself for a leaf), the node of class 2,
// and the sizes of the four classes
struct FitEdge {
	int32_t k0, k2;
	uint32_t n0, n1, n2, n3;
};

// what k_mean and k_record leave
struct FitDev {
	double rss, rss_joined, tss, worst, mean;
	uint32_t b, c; // ~0u, ~0u: every residual is a NaN
};

// Block i: row i of D below the diagonal from column i above it, the diagonal +0.0.
__global__ __launch_bounds__(256) void k_mirror(double *__restrict__ D, uint32_t n) {
	const uint32_t i = blockIdx.x;
	for (uint32_t j = threadIdx.x; j <= i; j += blockDim.x) D[(size_t)i * n + j] = j < i ? D[(size_t)j * n + i] : 0.0;
}

// Thread = (edge v0 + lane, leaf b0 + wavefront), b0 = first + 4 * blockIdx.y, over the leaves c > b in ascending order:
// the sum of D[b][c] over the c of class k into [k][b - first][v] of part, a plane of `plane` doubles a class.
__global__ __launch_bounds__(ET *BT) void k_fit(const double *__restrict__ D, const uint64_t *__restrict__ sets,
												const FitEdge *__restrict__ edges, uint32_t n, uint32_t W, uint32_t E,
												uint32_t first, uint32_t g, double *__restrict__ part, size_t plane) {
	__shared__ double sD[BT * LT];
	const uint32_t lane = threadIdx.x & 63, wb = threadIdx.x >> 6;
	const uint32_t v0 = blockIdx.x * ET, b0 = first + blockIdx.y * BT, bend = first + g;
	const uint32_t v = v0 + lane, b = b0 + wb;
	const bool live = v < E && b < bend;
	int32_t k0 = 0, k2 = 0;
	if (v < E) k0 = edges[v].k0, k2 = edges[v].k2;
	const double *myD = sD + wb * LT;

	double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
	for (uint32_t i0 = ((b0 + 1) / LT) * LT, tile = i0 / LT; i0 < n; i0 += LT, ++tile) { // (c > b0)
		const uint32_t c = i0 + lane;
		sD[threadIdx.x] = b < bend && c < n && c > b ? D[(size_t)b * n + c] : 0.0;
		__syncthreads();
		if (live) {
			const uint64_t w0 = child_word(sets, n, W, tile, k0), wv = child_word(sets, n, W, tile, (int32_t)v);
			const uint64_t w2 = child_word(sets, n, W, tile, k2);
			const uint64_t m0 = w0, m1 = wv & ~w0, m2 = w2, m3 = ~(wv | w2); // (a leaf past n is in class 3 and adds +0.0)
#pragma unroll
			for (uint32_t i = 0; i < LT; ++i) {
				const double d = myD[i];
				s0 += (m0 >> i) & 1 ? d : 0.0;
				s1 += (m1 >> i) & 1 ? d : 0.0;
				s2 += (m2 >> i) & 1 ? d : 0.0;
				s3 += (m3 >> i) & 1 ? d : 0.0;
			}
		}
		__syncthreads();
	}
	if (!live) return;
	const size_t at = (size_t)(b - first) * E + v;
	part[at] = s0, part[plane + at] = s1, part[2 * plane + at] = s2, part[3 * plane + at] = s3;
}

// the class of leaf b around edge v
__device__ inline int class_of(const uint64_t *sets, uint32_t n, uint32_t W, const FitEdge &e, uint32_t v, uint32_t b) {
	const uint32_t w = b >> 6, i = b & 63;
	if ((child_word(sets, n, W, w, e.k0) >> i) & 1) return 0;
	if ((child_word(sets, n, W, w, (int32_t)v) >> i) & 1) return 1;
	return (child_word(sets, n, W, w, e.k2) >> i) & 1 ? 2 : 3;
}

// acc[xy][v], xy = 01 02 03 12 13 23: over the g leaves b = first + k of a group in ascending order, s_y(v, b) where b is
// of class x and s_x(v, b) where it is of class y (+0.0 otherwise)
__global__ __launch_bounds__(64) void k_fold6(const double *__restrict__ part, size_t plane, const uint64_t *__restrict__ sets,
											   const FitEdge *__restrict__ edges, uint32_t n, uint32_t W, uint32_t E, uint32_t first,
											   uint32_t g, double *__restrict__ acc) {
	const uint32_t v = blockIdx.x * 64 + threadIdx.x;
	if (v >= E) return;
	const FitEdge e = edges[v];
	double a01 = acc[v], a02 = acc[(size_t)E + v], a03 = acc[2 * (size_t)E + v], a12 = acc[3 * (size_t)E + v],
		   a13 = acc[4 * (size_t)E + v], a23 = acc[5 * (size_t)E + v];
	for (uint32_t k0 = 0; k0 < g; k0 += 4) { // (the loads of four leaves in flight; the additions stay in the order of k)
		double p[4][4];
		int cl[4];
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const uint32_t k = k0 + j < g ? k0 + j : g - 1;
			const size_t at = (size_t)k * E + v;
			p[j][0] = part[at], p[j][1] = part[plane + at], p[j][2] = part[2 * plane + at], p[j][3] = part[3 * plane + at];
			cl[j] = k0 + j < g ? class_of(sets, n, W, e, v, first + k) : -1; // (-1: past the group, nothing is added)
		}
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const double p0 = p[j][0], p1 = p[j][1], p2 = p[j][2], p3 = p[j][3];
			const int c = cl[j];
			a01 += c == 0 ? p1 : c == 1 ? p0 : 0.0;
			a02 += c == 0 ? p2 : c == 2 ? p0 : 0.0;
			a03 += c == 0 ? p3 : c == 3 ? p0 : 0.0;
			a12 += c == 1 ? p2 : c == 2 ? p1 : 0.0;
			a13 += c == 1 ? p3 : c == 3 ? p1 : 0.0;
			a23 += c == 2 ? p3 : c == 3 ? p2 : 0.0;
		}
	}
	acc[v] = a01, acc[(size_t)E + v] = a02, acc[2 * (size_t)E + v] = a03, acc[3 * (size_t)E + v] = a12;
	acc[4 * (size_t)E + v] = a13, acc[5 * (size_t)E + v] = a23;
}

__device__ inline double mean_of(double S, uint32_t nx, uint32_t ny) { return S / (double)((uint64_t)nx * ny); }

__global__ __launch_bounds__(64) void k_lengths(const double *__restrict__ acc, const FitEdge *__restrict__ edges, uint32_t n,
												 uint32_t E, double *__restrict__ len) {
	const uint32_t v = blockIdx.x * 64 + threadIdx.x;
	if (v >= E) return;
	const FitEdge e = edges[v];
	const double m02 = mean_of(acc[(size_t)E + v], e.n0, e.n2), m03 = mean_of(acc[2 * (size_t)E + v], e.n0, e.n3);
	const double m23 = mean_of(acc[5 * (size_t)E + v], e.n2, e.n3);
	if (v < n) {
		len[v] = ((m02 + m03) - m23) * 0.5;
		return;
	}
	const double m01 = mean_of(acc[v], e.n0, e.n1), m12 = mean_of(acc[3 * (size_t)E + v], e.n1, e.n2);
	const double m13 = mean_of(acc[4 * (size_t)E + v], e.n1, e.n3);
	const double gm = (double)((uint64_t)e.n1 * e.n2 + (uint64_t)e.n0 * e.n3) /
					  (double)((uint64_t)(e.n0 + e.n1) * (uint64_t)(e.n2 + e.n3));
	len[v] = ((gm * (m02 + m13) + (1.0 - gm) * (m12 + m03)) - (m01 + m23)) * 0.5;
}

// R[b][c] = D[lo][hi] - p(lo, hi) for the leaves b != c, lo < hi the two; the diagonal +0.0.  Block = (256 c, b).
__global__ __launch_bounds__(256) void k_resid(const double *__restrict__ D, const double *__restrict__ T,
												const double *__restrict__ len, uint32_t n, double *__restrict__ R) {
	const uint32_t b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
	if (c >= n) return;
	const uint32_t lo = b < c ? b : c, hi = b < c ? c : b;
	const size_t at = (size_t)lo * n + hi;
	const double p = T[at] + len[lo];
	R[(size_t)b * n + c] = b == c ? 0.0 : D[at] - p;
}

// Thread i: ss[i], the sum of r*r over the leaves j != i ascending; row[i], over j > i only; and, if wr is given, of the
// pairs (i, j), j > i, the first of the greatest |r| (a NaN counts for nothing): wc[i] = j (~0u: none), wr[i] = its r.
__global__ __launch_bounds__(64) void k_leaf(const double *__restrict__ R, uint32_t n, double *__restrict__ ss,
											  double *__restrict__ row, double *__restrict__ wr, uint32_t *__restrict__ wc) {
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) return;
	double all = 0.0, up = 0.0, best = 0.0, br = __builtin_nan("");
	uint32_t bc = ~0u;
	for (uint32_t j0 = 0; j0 < n; j0 += 8) { // (eight loads in flight; the additions stay one after the other, in the order of j)
		double r[8];
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) r[k] = j0 + k < n ? R[(size_t)(j0 + k) * n + i] : 0.0;
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t j = j0 + k;
			if (j >= n || j == i) continue;
			const double q = r[k] * r[k];
			all = all + q;
			if (j < i) continue;
			up = up + q;
			const double a = __builtin_fabs(r[k]);
			if (!__builtin_isnan(a) && (bc == ~0u || a > best)) best = a, br = r[k], bc = j; // (ascending j: on a tie the earlier one stays)
		}
	}
	ss[i] = all, row[i] = up;
	if (wr) wr[i] = br, wc[i] = bc;
}

// Thread b: the sum over c > b ascending of D[b][c] (mean == nullptr) or of (D[b][c] - mean)^2, down column b of the
// mirrored matrix.
__global__ __launch_bounds__(64) void k_rows_d(const double *__restrict__ D, uint32_t n, const FitDev *__restrict__ mean,
												double *__restrict__ row) {
	const uint32_t b = blockIdx.x * 64 + threadIdx.x;
	if (b >= n) return;
	double s = 0.0;
	const double m = mean ? mean->mean : 0.0;
	for (uint32_t c0 = b + 1; c0 < n; c0 += 8) { // (eight loads in flight; the additions stay in the order of c)
		double d[8];
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) d[k] = c0 + k < n ? D[(size_t)(c0 + k) * n + b] : 0.0;
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			if (c0 + k >= n) continue;
			if (mean) {
				const double x = d[k] - m;
				s = s + x * x;
			} else {
				s = s + d[k];
			}
		}
	}
	row[b] = s;
}

// The sum of row[0 ... n) in ascending order, by one wavefront: 64 entries are loaded at a time, one a lane, and every
// lane adds them in the order of the lanes (all lanes hold the same sum).
__device__ inline double sum_rows(const double *row, uint32_t n) {
	double s = 0.0;
	for (uint32_t base = 0; base < n; base += 64) {
		const double x = base + threadIdx.x < n ? row[base + threadIdx.x] : 0.0;
		const uint32_t cnt = n - base < 64 ? n - base : 64;
		for (uint32_t j = 0; j < cnt; ++j) s = s + __shfl(x, (int)j);
	}
	return s;
}

// One wavefront: the mean of the n(n - 1)/2 distances from the rows' sums.
__global__ __launch_bounds__(64) void k_mean(const double *__restrict__ row, uint32_t n, FitDev *__restrict__ out) {
	const double s = sum_rows(row, n);
	if (threadIdx.x == 0) out->mean = s / (double)((unsigned long long)n * (n - 1) / 2);
}

// One wavefront: rss under both length vectors and tss from the rows' sums, b ascending, and the first pair in (b, c)
// order of the greatest |r| under the refit lengths.
__global__ __launch_bounds__(64) void k_record(const double *__restrict__ row_fit, const double *__restrict__ row_joined,
						 const double *__restrict__ row_t, const double *__restrict__ wr, const uint32_t *__restrict__ wc, uint32_t n,
						 FitDev *__restrict__ out) {
	const double rss = sum_rows(row_fit, n), rss_joined = sum_rows(row_joined, n), tss = sum_rows(row_t, n);
	double best = 0.0, br = __builtin_nan("");
	uint32_t bb = ~0u, bc = ~0u;
	for (uint32_t b = threadIdx.x; b < n; b += 64) {
		if (wc[b] == ~0u) continue;
		const double a = __builtin_fabs(wr[b]);
		if (bb == ~0u || a > best) best = a, br = wr[b], bb = b, bc = wc[b]; // (ascending b: on a tie the earlier one stays)
	}
	for (int m = 32; m > 0; m >>= 1) {
		const double oa = __shfl_xor(best, m), orr = __shfl_xor(br, m);
		const uint32_t ob = __shfl_xor(bb, m), oc = __shfl_xor(bc, m);
		if (ob != ~0u && (bb == ~0u || oa > best || (oa == best && ob < bb))) best = oa, br = orr, bb = ob, bc = oc;
	}
	if (threadIdx.x != 0) return;
	out->rss = rss, out->rss_joined = rss_joined, out->tss = tss;
	out->worst = br, out->b = bb, out->c = bc;
}

constexpr size_t FIT_GROUP_BYTES = (size_t)1 << 30; // device memory of a group of leaves' sums, at most (one always fits)

// the sum of the lengths over v ascending, and how many are negative
void length_sum(const double *len, size_t E, double &sum, uint32_t &negative) {
	sum = 0.0, negative = 0;
	for (size_t v = 0; v < E; ++v) sum = sum + len[v], negative += len[v] < 0;
}

} // namespace

int andi_hip_fit(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, int method, double *len_out,
				 andi_hip_fit_result *out, double *leaf_ss, double *leaf_ss_joined) {
	if (!ctx || !tree || !D || !len_out || !out || n < 3 || n > 65535 || method != ANDI_FIT_OLS) {
		if (ctx)
			ctx->err = "andi_hip_fit: bad arguments (ctx, tree, D, len and out must be given, 3 <= n <= 65535, method OLS)";
		return 1;
	}
	const size_t E = 2 * n - 3, C = E, nsets = n - 3, W = (n + 63) / 64;
	for (size_t s = 0; s + 2 < n; ++s) {
		const double l[3] = {tree[s].la, tree[s].lb, s + 3 == n ? tree[s].lc : 0.0};
		for (int k = 0; k < 3; ++k)
			if (!std::isfinite(l[k])) {
				char msg[160];
				snprintf(msg, sizeof msg, "andi_hip_fit: a branch length of the tree's record %zu is not finite", s);
				ctx->err = msg;
				return 1;
			}
	}
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> kids(nsets ? nsets : 1);
	if (!records_ok(tree, n, seen.data(), kids.data())) {
		ctx->err = "andi_hip_fit: the tree's records are not those of andi_hip_nj";
		return 1;
	}
	for (size_t i = 0; i < n; ++i)
		for (size_t j = i + 1; j < n; ++j)
			if (!std::isfinite(D[i * n + j])) {
				char msg[160];
				snprintf(msg, sizeof msg, "andi_hip_fit: D[%zu][%zu] is not finite (%g)", i, j, D[i * n + j]);
				ctx->err = msg;
				return 1;
			}
	std::vector<int32_t> par(E);
	std::vector<double> len(E);
	std::vector<uint32_t> size(E + 1);
	std::vector<FitEdge> edges(E);
	for (size_t i = 0; i < n; ++i) size[i] = 1;
	for (size_t s = 0; s + 2 < n; ++s) {
		const bool last = s + 3 == n;
		const int32_t ch[3] = {tree[s].a, tree[s].b, tree[s].c};
		const double l[3] = {tree[s].la, tree[s].lb, tree[s].lc};
		const int nk = last ? 3 : 2;
		for (int k = 0; k < nk; ++k) {
			par[ch[k]] = (int32_t)(last ? C : n + s), len[ch[k]] = l[k];
			edges[ch[k]].k2 = ch[(k == 0) ? 1 : 0]; // (the other child, or the first of the other two in record order)
		}
		if (!last) size[n + s] = size[ch[0]] + size[ch[1]];
	}
	for (size_t v = 0; v < E; ++v) {
		FitEdge &e = edges[v];
		e.k0 = v < n ? (int32_t)v : tree[v - n].a;
		e.n0 = size[e.k0], e.n1 = size[v] - e.n0, e.n2 = size[e.k2], e.n3 = (uint32_t)n - size[v] - e.n2;
	}

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// the leaves of a group: at most what k_fit's grid takes as its second dimension, BT leaves a block
	size_t G = nj_group_size(KNOB_FIT_GROUP, (size_t)65535 * BT, FIT_GROUP_BYTES, 4 * E * sizeof(double));
	if (G > n) G = n;
	const uint32_t N = (uint32_t)n, Ed = (uint32_t)E, Wd = (uint32_t)W;
	const size_t plane = G * E;
	hipStream_t st = ctx->stream;
	DevScope dev(st);
	double *T = nullptr, *dD = nullptr, *R = nullptr, *dlen = nullptr, *dfit = nullptr, *part = nullptr, *acc = nullptr;
	double *ss = nullptr, *rows = nullptr, *wr = nullptr;
	int32_t *dpar = nullptr;
	int2 *dkids = nullptr;
	uint64_t *sets = nullptr;
	uint32_t *wc = nullptr;
	FitEdge *dedges = nullptr;
	FitDev *dres = nullptr;
	dev.alloc(&T, E * n);
	if (dev.err != hipSuccess) {
		char msg[200];
		snprintf(msg, sizeof msg, "andi_hip_fit: the table of path lengths needs %zu bytes of device memory: %s",
				 E * n * sizeof(double), hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	dev.alloc(&dD, n * n), dev.alloc(&R, n * n), dev.alloc(&part, 4 * plane), dev.alloc(&acc, 6 * E);
	dev.alloc(&dpar, E), dev.alloc(&dlen, E), dev.alloc(&dfit, E), dev.alloc(&dedges, E);
	dev.alloc(&dkids, nsets ? nsets : 1), dev.alloc(&sets, nsets ? nsets * W : 1);
	dev.alloc(&ss, 2 * n), dev.alloc(&rows, 4 * n), dev.alloc(&wr, n), dev.alloc(&wc, n), dev.alloc(&dres, 1);
	double *row_fit = rows, *row_joined = rows + n, *row_d = rows + 2 * n, *row_t = rows + 3 * n;
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, n * n * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dpar, par.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dlen, len.data(), E * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dedges, edges.data(), E * sizeof(FitEdge), hipMemcpyHostToDevice, st);
	if (e == hipSuccess && nsets) e = hipMemcpyAsync(dkids, kids.data(), nsets * sizeof(int2), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(acc, 0, 6 * E * sizeof(double), st); // (+0.0)
	if (e == hipSuccess) {
		if (nsets) k_sets<<<dim3((Wd + 63) / 64, 1), 64, 0, st>>>(dkids, N, (uint32_t)nsets, Wd, sets);
		k_mirror<<<N, 256, 0, st>>>(dD, N);
		e = hipGetLastError();
	}
	for (size_t first = 0; e == hipSuccess && first < n; first += G) {
		const uint32_t g = (uint32_t)(n - first < G ? n - first : G);
		k_fit<<<dim3((Ed + ET - 1) / ET, (g + BT - 1) / BT), ET * BT, 0, st>>>(dD, sets, dedges, N, Wd, Ed, (uint32_t)first, g, part,
																				plane);
		k_fold6<<<(Ed + 63) / 64, 64, 0, st>>>(part, plane, sets, dedges, N, Wd, Ed, (uint32_t)first, g, acc);
		e = hipGetLastError();
	}
	if (e == hipSuccess) {
		const uint32_t nb = (N + 63) / 64;
		k_lengths<<<(Ed + 63) / 64, 64, 0, st>>>(acc, dedges, N, Ed, dfit);
		k_paths<<<nb, 64, 0, st>>>(dpar, dfit, sets, N, Wd, T);
		k_resid<<<dim3((N + 255) / 256, N), 256, 0, st>>>(dD, T, dfit, N, R);
		k_leaf<<<nb, 64, 0, st>>>(R, N, ss, row_fit, wr, wc);
		k_paths<<<nb, 64, 0, st>>>(dpar, dlen, sets, N, Wd, T);
		k_resid<<<dim3((N + 255) / 256, N), 256, 0, st>>>(dD, T, dlen, N, R);
		k_leaf<<<nb, 64, 0, st>>>(R, N, ss + n, row_joined, nullptr, nullptr);
		k_rows_d<<<nb, 64, 0, st>>>(dD, N, nullptr, row_d);
		k_mean<<<1, 64, 0, st>>>(row_d, N, dres);
		k_rows_d<<<nb, 64, 0, st>>>(dD, N, dres, row_t);
		k_record<<<1, 64, 0, st>>>(row_fit, row_joined, row_t, wr, wc, N, dres);
		e = hipGetLastError();
	}
	FitDev res;
	std::vector<double> hfit(E), hss(2 * n); // (the caller's arrays are written on success only)
	if (e == hipSuccess) e = hipMemcpyAsync(&res, dres, sizeof res, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(hfit.data(), dfit, E * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(hss.data(), ss, 2 * n * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_fit", e);

	andi_hip_fit_result r;
	memset(&r, 0, sizeof r);
	r.rss = res.rss, r.rss_joined = res.rss_joined, r.tss = res.tss, r.worst = res.worst;
	r.pairs = (uint64_t)n * (n - 1) / 2;
	length_sum(hfit.data(), E, r.length, r.negative);
	length_sum(len.data(), E, r.length_joined, r.negative_joined);
	r.worst_b = res.b == ~0u ? -1 : (int32_t)res.b, r.worst_c = res.c == ~0u ? -1 : (int32_t)res.c;
	memcpy(len_out, hfit.data(), E * sizeof(double));
	if (leaf_ss) memcpy(leaf_ss, hss.data(), n * sizeof(double));
	if (leaf_ss_joined) memcpy(leaf_ss_joined, hss.data() + n, n * sizeof(double));
	*out = r;
	return 0;
}
