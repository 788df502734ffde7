// refine.hip — a joined tree refined by balanced nearest-neighbor interchanges on the device (andi_hip_refine,
// include/andi_hip.h), and its balanced (BME) branch lengths: bit for bit the contract in andi_hip.h (tests/bme_model.py
// restates it in NumPy).
//
// The tree is rooted at the centre C and keeps its node ids; a move re-hangs two subtrees in the parent and child arrays on
// the device.  Every round evaluates the tree as it stands from nothing (no incremental update: DESIGN.md 10.17):
//   k_order    one wavefront: the non-centre nodes breadth-first from C (64 queue entries a trip, the children appended in
//              lane order by a ballot, so the order is the sequential one), lev[], the edges from C, and where every level
//              begins in the order.  The nodes of a level do not depend on one another, and a level's children are all in
//              the next; after a move the ids no longer say who comes before whom;
//   k_rsets    one block, the deepest level first, a barrier a level: thread = (node of the level, word of its leaf set,
//              nj_sets.h's layout), the OR of the children's words;
//   k_table    the hot path: a block is 64 leaves c (the lanes) x 16 wavefronts, column c of the table A only.  First
//              the far-side values of all nodes, the deepest level first, the wavefronts sharing a level's nodes and a
//              barrier ending it (a leaf's row is D's); then one wavefront takes the near-side values down the path from C
//              to c, the child that holds c found in the leaf sets.  The leaf is the fastest index: a wavefront's
//              accesses are runs of 512 bytes, and the set words, the order and the children are wavefront-uniform.
//              k_paths' form (tree_paths.h), one thread per leaf walking all nodes, gives the same bits at the latency of
//              2n - 3 dependent loads: 3.0 ms a round at 3085 leaves;
//   k_sums     one wavefront per (node x, one of its four rows): the lanes load 64 words of x's leaf set at a time, and the
//              wavefront visits the words that are not empty; lane l adds w * A[row][c] of the leaves c = 64 word + l below
//              x to its partial sum, and the 64 partial sums are added in lane order;
//   k_blen     one thread per edge: the balanced lengths from the sums (before the first round, after the last);
//   k_choose   one block: the two gains of every inner edge, and the greatest by the contract's order;
//   k_apply    one wavefront: the least leaves of the two subtrees of the chosen move (for the log), and the move itself.
// The host reads one record of 32 bytes a round: the gain, the move and whether the search goes on.
// D is mirrored once, by k_mirror's rule (fit.hip).  The output numbering is the host's, O(n).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nj_sets.h"

static_assert(sizeof(andi_hip_refine_result) == 32, "andi_hip_refine_result: two doubles, the moves, converged, pad");
static_assert(sizeof(andi_hip_refine_move) == 16, "andi_hip_refine_move: the gain and two leaves");

namespace {

// what a round leaves for the host: the greatest gain, its edge and alternative (v = -1: the tree has no inner edge), the
// least leaves of the outgoing and the incoming subtree, and stop = 0 (the move was made), 1 (converged), 2 (max_moves)
struct RefRec {
	double gain;
	int32_t v, alt, first, second, stop, pad;
};

// Block i: row i of D below the diagonal from column i above it, the diagonal +0.0.
__global__ __launch_bounds__(256) void k_mirror(double *__restrict__ D, uint32_t n) {
	const uint32_t i = blockIdx.x;
	for (uint32_t j = threadIdx.x; j <= i; j += blockDim.x) D[(size_t)i * n + j] = j < i ? D[(size_t)j * n + i] : 0.0;
}

// The children of inner node q are kid[2 (q - n)], kid[2 (q - n) + 1]; the centre C = 2n - 3 has a third.
// o0, o1: the children of q but x, in slot order (o1 = -1 unless q is the centre).
__device__ inline void others_of(const int32_t *kid, uint32_t n, uint32_t q, int32_t x, int32_t &o0, int32_t &o1) {
	const int32_t *k = kid + 2 * (size_t)(q - n);
	o0 = k[0] == x ? k[1] : k[0];
	o1 = q == 2 * n - 3 ? (k[2] == x ? k[1] : k[2]) : -1;
}

// the row of A that sum k of node x is taken against: the sibling, the parent's row, the uncle, the grandparent's row;
// where the parent (the grandparent) is the centre, its other two children in slot order instead.  -1: none.
__device__ inline int32_t row_of(const int32_t *par, const int32_t *kid, uint32_t n, uint32_t x, uint32_t k) {
	const uint32_t C = 2 * n - 3, p = (uint32_t)par[x];
	int32_t o0, o1;
	if (p == C) {
		others_of(kid, n, C, (int32_t)x, o0, o1);
		return k == 0 ? o0 : k == 1 ? o1 : -1;
	}
	if (k == 1) return (int32_t)p;
	if (k == 0) {
		others_of(kid, n, p, (int32_t)x, o0, o1);
		return o0;
	}
	const uint32_t g = (uint32_t)par[p];
	others_of(kid, n, g, (int32_t)p, o0, o1);
	if (g == C) return k == 2 ? o0 : o1;
	return k == 2 ? o0 : (int32_t)g;
}

// One wavefront.  order: the E = 2n - 3 non-centre nodes breadth-first; lev: E + 1 entries; lstart: E + 2 entries --
// lstart[0] the deepest level, lstart[l] where level l >= 1 begins in order (a level is one run of it), E behind the last.
// SLOTS = false: the children are kid's.  SLOTS = true (the SPR search): src holds three neighbour slots per inner node,
// src[3 (q - n) + s]; the children of a node are its neighbours but its parent, in slot order, and par and kid are written.
// Returns the deepest level.
template <bool SLOTS>
__device__ inline int32_t order_from_centre(const int32_t *__restrict__ src, uint32_t n, int32_t *par, int32_t *kid, int32_t *order,
											 int32_t *lev, int32_t *lstart) {
	const uint32_t E = 2 * n - 3, C = E, lane = threadIdx.x;
	if (lane < 3) {
		const int32_t x = src[(SLOTS ? 3 : 2) * (size_t)(C - n) + lane];
		order[lane] = x, lev[x] = 1;
		if (SLOTS) par[x] = (int32_t)C, kid[2 * (size_t)(C - n) + lane] = x;
	}
	if (lane == 0) lev[C] = 0;
	__syncthreads();
	uint32_t head = 0, tail = 3;
	while (head < tail) {
		const uint32_t i = head + lane;
		const int32_t x = i < tail ? order[i] : -1;
		const bool inner = x >= (int32_t)n;
		const unsigned long long m = __ballot(inner);
		if (i < tail) {
			const int32_t l = lev[x];
			if (i == 0 || lev[order[i - 1]] != l) lstart[l] = (int32_t)i;
		}
		if (inner) {
			const uint32_t at = tail + 2 * (uint32_t)__popcll(m & ((1ull << lane) - 1));
			int32_t a, b;
			if (SLOTS) {
				const int32_t *s = src + 3 * (size_t)(x - (int32_t)n);
				const int32_t p = par[x];
				a = s[0] == p ? s[1] : s[0], b = s[2] == p ? s[1] : s[2];
			} else a = src[2 * (size_t)(x - (int32_t)n)], b = src[2 * (size_t)(x - (int32_t)n) + 1];
			const int32_t l = lev[x] + 1;
			if (at + 1 < E) { // (a tree's nodes are queued once each: it fits)
				order[at] = a, order[at + 1] = b, lev[a] = l, lev[b] = l;
				if (SLOTS) par[a] = x, par[b] = x, kid[2 * (size_t)(x - (int32_t)n)] = a, kid[2 * (size_t)(x - (int32_t)n) + 1] = b;
			}
		}
		head += tail - head < 64 ? tail - head : 64;
		tail += 2 * (uint32_t)__popcll(m);
		if (tail > E) tail = E;
		__syncthreads();
	}
	const int32_t deepest = lev[order[E - 1]];
	if (lane == 0) lstart[0] = deepest, lstart[deepest + 1] = (int32_t)E;
	return deepest;
}

__global__ __launch_bounds__(64) void k_order(const int32_t *__restrict__ kid, uint32_t n, int32_t *order, int32_t *lev,
											  int32_t *lstart) {
	order_from_centre<false>(kid, n, nullptr, nullptr, order, lev, lstart);
}

constexpr int LT = 1024; // k_rsets, k_table: the threads of a block that works level by level

// One block: the n - 3 pair nodes' leaf sets, the deepest level first.  The nodes of a level do not depend on one another:
// thread = (node of the level, word), and a barrier ends the level.
__global__ __launch_bounds__(LT) void k_rsets(const int32_t *__restrict__ order, const int32_t *__restrict__ lstart,
											  const int32_t *__restrict__ kid, uint32_t n, uint32_t W, uint64_t *sets) {
	for (int32_t l = lstart[0]; l >= 1; --l) {
		const uint32_t first = (uint32_t)lstart[l], cells = ((uint32_t)lstart[l + 1] - first) * W;
		for (uint32_t t = threadIdx.x; t < cells; t += LT) {
			const int32_t x = order[first + t / W];
			if (x < (int32_t)n) continue;
			const uint32_t w = t % W;
			const int32_t a = kid[2 * (size_t)(x - (int32_t)n)], b = kid[2 * (size_t)(x - (int32_t)n) + 1];
			sets[(size_t)(x - (int32_t)n) * W + w] = child_word(sets, n, W, w, a) | child_word(sets, n, W, w, b);
		}
		__syncthreads();
	}
}

// Block = 64 leaves c (the lanes) x 16 wavefronts: A[v * n + c] for the E non-centre nodes v.  A thread per leaf walking
// all nodes runs at the latency of 2n - 3 dependent loads (k_paths' form: 3.0 ms a round at 3085 leaves); the nodes of a
// level do not depend on one another, so the wavefronts share them and a barrier ends the level.
__global__ __launch_bounds__(LT) void k_table(const double *__restrict__ D, const int32_t *__restrict__ kid,
											  const int32_t *__restrict__ order, const int32_t *__restrict__ lstart,
											  const uint64_t *__restrict__ sets, uint32_t n, uint32_t W, double *A) {
	const uint32_t c = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6, NW = LT / 64;
	const bool live = c < n;
	const uint32_t E = 2 * n - 3, C = E, w = c >> 6;
	const uint64_t bit = 1ull << (c & 63);
	for (uint32_t v = wave; v < n; v += NW)
		if (live && v != c) A[(size_t)v * n + c] = D[(size_t)v * n + c];
	__syncthreads();
	for (int32_t l = lstart[0]; l >= 1; --l) { // the far side below x: the deepest level first
		const uint32_t end = (uint32_t)lstart[l + 1];
		for (uint32_t i = (uint32_t)lstart[l] + wave; i < end; i += NW) {
			const int32_t x = order[i];
			if (!live || x < (int32_t)n || (child_word(sets, n, W, w, x) & bit)) continue;
			const int32_t a = kid[2 * (size_t)(x - (int32_t)n)], b = kid[2 * (size_t)(x - (int32_t)n) + 1];
			A[(size_t)x * n + c] = (A[(size_t)a * n + c] + A[(size_t)b * n + c]) * 0.5;
		}
		__syncthreads();
	}
	if (wave != 0 || !live) return;
	// the far side above v, down the path from the centre to c, by one wavefront
	const int32_t *kc = kid + 2 * (size_t)(C - n);
	int32_t v = kc[0];
	if (!(child_word(sets, n, W, w, v) & bit)) v = (child_word(sets, n, W, w, kc[1]) & bit) ? kc[1] : kc[2];
	int32_t o0, o1;
	others_of(kid, n, C, v, o0, o1);
	double up = (A[(size_t)o0 * n + c] + A[(size_t)o1 * n + c]) * 0.5;
	A[(size_t)v * n + c] = up;
	for (uint32_t step = 0; v >= (int32_t)n && step < E; ++step) { // (a path has fewer than E nodes)
		const int32_t a = kid[2 * (size_t)(v - (int32_t)n)], b = kid[2 * (size_t)(v - (int32_t)n) + 1];
		const bool in_a = child_word(sets, n, W, w, a) & bit;
		const int32_t x = in_a ? a : b, s = in_a ? b : a;
		up = (A[(size_t)s * n + c] + up) * 0.5;
		A[(size_t)x * n + c] = up;
		v = x;
	}
}

// Wavefront (x, k): T[4 x + k] = S(x, row k of x), +0.0 where x has no such row.
__global__ __launch_bounds__(256) void k_sums(const double *__restrict__ A, const int32_t *__restrict__ par,
											  const int32_t *__restrict__ kid, const uint64_t *__restrict__ sets,
											  const int32_t *__restrict__ lev, uint32_t n, uint32_t W, double *__restrict__ T) {
	const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, E = 2 * n - 3;
	const uint32_t x = g >> 2, k = g & 3;
	if (x >= E) return;
	const int32_t r = row_of(par, kid, n, x, k);
	if (r < 0) {
		if (lane == 0) T[g] = 0.0;
		return;
	}
	const double *row = A + (size_t)r * n;
	const int32_t lx = lev[x];
	double p = 0.0;
	if (x < n) {
		if (lane == (x & 63)) p = p + 1.0 * row[x];
	} else {
		const uint64_t *set = sets + (size_t)(x - n) * W;
		for (uint32_t w0 = 0; w0 < W; w0 += 64) {
			const uint64_t mine = w0 + lane < W ? set[w0 + lane] : 0ull;
			unsigned long long m = __ballot(mine != 0);
			while (m) {
				const int j = __builtin_ctzll(m);
				m &= m - 1;
				const uint64_t word = __shfl((unsigned long long)mine, j);
				if ((word >> lane) & 1) {
					const uint32_t c = (w0 + (uint32_t)j) * 64 + lane; // (a set holds leaves only: c < n)
					const int32_t e = lev[c] - lx;
					const double wgt = e > 1022 ? 0.0 : __longlong_as_double((long long)(1023 - e) << 52);
					p = p + wgt * row[c];
				}
			}
		}
	}
	double s = 0.0;
	for (int j = 0; j < 64; ++j) s = s + __shfl(p, j);
	if (lane == 0) T[g] = s;
}

// S(o0, o1) of two children of the centre
__device__ inline double between_top(const double *T, const int32_t *kid, uint32_t n, int32_t o0, int32_t o1) {
	int32_t a0, a1;
	others_of(kid, n, 2 * n - 3, o0, a0, a1);
	return T[4 * (size_t)o0 + (a0 == o1 ? 0 : 1)];
}

struct Six {
	double ab, as, bs, au, bu, su;
};

// the six averages around the inner edge v
__device__ inline Six six_of(const double *T, const int32_t *par, const int32_t *kid, uint32_t n, uint32_t v) {
	const int32_t a = kid[2 * (size_t)(v - n)], b = kid[2 * (size_t)(v - n) + 1];
	const uint32_t q = (uint32_t)par[v];
	int32_t o0, o1;
	others_of(kid, n, q, (int32_t)v, o0, o1);
	Six d;
	d.su = q == 2 * n - 3 ? between_top(T, kid, n, o0, o1) : T[4 * (size_t)o0 + 1];
	d.ab = T[4 * (size_t)a], d.as = T[4 * (size_t)a + 2], d.bs = T[4 * (size_t)b + 2];
	d.au = T[4 * (size_t)a + 3], d.bu = T[4 * (size_t)b + 3];
	return d;
}

// Thread v: the balanced length of edge v.
__global__ __launch_bounds__(64) void k_blen(const double *__restrict__ T, const int32_t *__restrict__ par,
											 const int32_t *__restrict__ kid, uint32_t n, double *__restrict__ len) {
	const uint32_t v = blockIdx.x * 64 + threadIdx.x, E = 2 * n - 3;
	if (v >= E) return;
	if (v >= n) {
		const Six d = six_of(T, par, kid, n, v);
		len[v] = ((d.as + d.au) + (d.bs + d.bu)) * 0.25 - (d.ab + d.su) * 0.5;
		return;
	}
	const uint32_t q = (uint32_t)par[v];
	int32_t o0, o1;
	others_of(kid, n, q, (int32_t)v, o0, o1);
	const double su = q == E ? between_top(T, kid, n, o0, o1) : T[4 * (size_t)o0 + 1];
	len[v] = ((T[4 * (size_t)v] + T[4 * (size_t)v + 1]) - su) * 0.5;
}

// candidate (g, i) comes before (G, I): the greater gain, a NaN below every number, ties to the smaller index; I < 0: none yet
__device__ inline bool before(double g, int32_t i, double G, int32_t I) {
	if (I < 0) return true;
	if (i < 0) return false;
	const bool gn = __builtin_isnan(g), Gn = __builtin_isnan(G);
	if (gn || Gn) return gn == Gn ? i < I : Gn;
	return g > G || (g == G && i < I);
}

constexpr int CT = 1024; // k_choose: the threads of its one block

// One block: the greatest of the 2 (n - 3) gains, index 2 (v - n) + alternative, and whether the search goes on.
__global__ __launch_bounds__(CT) void k_choose(const double *__restrict__ T, const int32_t *__restrict__ par,
											   const int32_t *__restrict__ kid, uint32_t n, double tol, int can_move,
											   RefRec *__restrict__ rec) {
	__shared__ double sg[CT];
	__shared__ int32_t si[CT];
	const uint32_t E = 2 * n - 3;
	double G = 0.0;
	int32_t I = -1;
	for (uint32_t v = n + threadIdx.x; v < E; v += CT) { // (v ascending: on a tie the earlier one stays)
		const Six d = six_of(T, par, kid, n, v);
		const double g0 = ((d.ab + d.su) - (d.as + d.bu)) * 0.25, g1 = ((d.ab + d.su) - (d.bs + d.au)) * 0.25;
		const int32_t i = 2 * (int32_t)(v - n);
		if (before(g0, i, G, I)) G = g0, I = i;
		if (before(g1, i + 1, G, I)) G = g1, I = i + 1;
	}
	sg[threadIdx.x] = G, si[threadIdx.x] = I;
	__syncthreads();
	for (uint32_t h = CT / 2; h > 0; h >>= 1) {
		if (threadIdx.x < h && before(sg[threadIdx.x + h], si[threadIdx.x + h], sg[threadIdx.x], si[threadIdx.x]))
			sg[threadIdx.x] = sg[threadIdx.x + h], si[threadIdx.x] = si[threadIdx.x + h];
		__syncthreads();
	}
	if (threadIdx.x != 0) return;
	G = sg[0], I = si[0];
	rec->gain = I < 0 ? 0.0 : G;
	rec->v = I < 0 ? -1 : (int32_t)n + (I >> 1), rec->alt = I < 0 ? 0 : I & 1;
	rec->first = rec->second = -1, rec->pad = 0;
	rec->stop = (I < 0 || !(G > tol)) ? 1 : can_move ? 0 : 2;
}

// the least leaf below x, by one wavefront
__device__ inline int32_t least_leaf(const uint64_t *sets, uint32_t n, uint32_t W, int32_t x, uint32_t lane) {
	if (x < (int32_t)n) return x;
	uint32_t m = ~0u;
	const uint64_t *set = sets + (size_t)(x - (int32_t)n) * W;
	for (uint32_t w = lane; w < W; w += 64) {
		const uint64_t word = set[w];
		if (word && m == ~0u) m = w * 64 + (uint32_t)__builtin_ctzll(word); // (w ascending: the first is the least of the lane)
	}
	for (int s = 32; s > 0; s >>= 1) {
		const uint32_t o = __shfl_xor(m, s);
		m = o < m ? o : m;
	}
	return (int32_t)m;
}

// One wavefront: the chosen move's least leaves into the record; if the search goes on, the incoming subtree s takes the
// outgoing one's slot in v and the outgoing one takes s's slot in q = parent(v).
__global__ __launch_bounds__(64) void k_apply(RefRec *rec, int32_t *par, int32_t *kid, const uint64_t *__restrict__ sets, uint32_t n,
											  uint32_t W) {
	const int32_t v = rec->v, alt = rec->alt, stop = rec->stop;
	if (v < 0) return;
	const uint32_t C = 2 * n - 3, q = (uint32_t)par[v];
	int32_t *kv = kid + 2 * (size_t)(v - (int32_t)n), *kq = kid + 2 * (size_t)(q - n);
	int32_t s, o1;
	others_of(kid, n, q, v, s, o1);
	const int32_t o = kv[alt == 0 ? 1 : 0];
	const int32_t first = least_leaf(sets, n, W, o, threadIdx.x), second = least_leaf(sets, n, W, s, threadIdx.x);
	if (threadIdx.x != 0) return;
	rec->first = first, rec->second = second;
	if (stop) return;
	kv[alt == 0 ? 1 : 0] = s;
	const int nk = q == C ? 3 : 2;
	for (int j = 0; j < nk; ++j)
		if (kq[j] == s) {
			kq[j] = o;
			break;
		}
	par[s] = v, par[o] = (int32_t)q;
}

// The records of the final tree in the output numbering: the centre the final record, children visited in order of their
// least leaf, inner nodes n, n + 1, ... in post-order, a pair record's smaller id first, the final record's ascending.
void number_records(const int32_t *kid, const double *len, size_t n, andi_hip_nj_join *out) {
	const size_t E = 2 * n - 3, C = E;
	std::vector<int32_t> order, least(C + 1), id(C + 1);
	order.reserve(E);
	for (int k = 0; k < 3; ++k) order.push_back(kid[2 * (C - n) + k]);
	for (size_t h = 0; h < order.size(); ++h)
		if ((size_t)order[h] >= n) order.push_back(kid[2 * (order[h] - n)]), order.push_back(kid[2 * (order[h] - n) + 1]);
	for (size_t v = 0; v <= C; ++v) least[v] = id[v] = (int32_t)v;
	for (size_t h = order.size(); h-- > 0;) {
		const size_t x = (size_t)order[h];
		if (x >= n) least[x] = std::min(least[kid[2 * (x - n)]], least[kid[2 * (x - n) + 1]]);
	}
	struct Visit {
		int32_t x, k;
	};
	std::vector<Visit> stack{{(int32_t)C, 0}};
	size_t next = 0;
	while (!stack.empty()) {
		const Visit t = stack.back();
		stack.pop_back();
		const size_t x = (size_t)t.x;
		const int nk = x == C ? 3 : 2;
		int32_t ch[3] = {kid[2 * (x - n)], kid[2 * (x - n) + 1], nk == 3 ? kid[2 * (x - n) + 2] : -1};
		for (int i = 1; i < nk; ++i) // by the least leaf
			for (int j = i; j > 0 && least[ch[j]] < least[ch[j - 1]]; --j) std::swap(ch[j], ch[j - 1]);
		int k = t.k;
		while (k < nk && (size_t)ch[k] < n) ++k;
		if (k < nk) {
			stack.push_back({t.x, k + 1}), stack.push_back({ch[k], 0});
			continue;
		}
		for (int i = 1; i < nk; ++i) // by the new id
			for (int j = i; j > 0 && id[ch[j]] < id[ch[j - 1]]; --j) std::swap(ch[j], ch[j - 1]);
		andi_hip_nj_join r;
		memset(&r, 0, sizeof r);
		r.a = id[ch[0]], r.b = id[ch[1]], r.c = nk == 3 ? id[ch[2]] : -1;
		r.la = len[ch[0]], r.lb = len[ch[1]], r.lc = nk == 3 ? len[ch[2]] : 0.0;
		if (x == C) out[n - 3] = r;
		else id[x] = (int32_t)(n + next), out[next++] = r;
	}
}

double length_sum(const double *len, size_t E) {
	double s = 0.0;
	for (size_t v = 0; v < E; ++v) s = s + len[v];
	return s;
}

// What both searches check on the host before any HIP call: the records are andi_hip_nj's and D is finite above the
// diagonal (the message names the first in row-major order).  par: 2n - 3, kid: 2 (n - 3) + 3 -- the tree rooted at C.
bool tree_input_ok(andi_hip_ctx *ctx, const char *who, const andi_hip_nj_join *tree, size_t n, const double *D, int32_t *par,
				   int32_t *kid) {
	const size_t C = 2 * n - 3, nsets = n - 3;
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> pairs(nsets ? nsets : 1);
	if (!records_ok(tree, n, seen.data(), pairs.data())) {
		ctx->err = std::string(who) + ": the tree's records are not those of andi_hip_nj";
		return false;
	}
	for (size_t i = 0; i < n; ++i)
		for (size_t j = i + 1; j < n; ++j)
			if (!std::isfinite(D[i * n + j])) {
				char msg[160];
				snprintf(msg, sizeof msg, "%s: D[%zu][%zu] is not finite (%g)", who, i, j, D[i * n + j]);
				ctx->err = msg;
				return false;
			}
	for (size_t s = 0; s + 2 < n; ++s) {
		const bool last = s + 3 == n;
		const int32_t ch[3] = {tree[s].a, tree[s].b, tree[s].c};
		for (int k = 0; k < (last ? 3 : 2); ++k) par[ch[k]] = (int32_t)(last ? C : n + s), kid[2 * s + k] = ch[k];
	}
	return true;
}

} // namespace

int andi_hip_refine(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, int method, double tol,
					size_t max_moves, andi_hip_nj_join *out, andi_hip_refine_result *res, andi_hip_refine_move *log) {
	if (!ctx || !tree || !D || !out || !res || n < 3 || n > 65535 || method != ANDI_REFINE_BNNI || !(tol >= 0)) {
		if (ctx)
			ctx->err = "andi_hip_refine: bad arguments (ctx, tree, D, out and res must be given, 3 <= n <= 65535, method BNNI, "
					   "tol >= 0)";
		return 1;
	}
	const size_t E = 2 * n - 3, nsets = n - 3, W = (n + 63) / 64, nkid = 2 * nsets + 3;
	std::vector<int32_t> par(E), kid(nkid);
	if (!tree_input_ok(ctx, "andi_hip_refine", tree, n, D, par.data(), kid.data())) return 1;

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, Ed = (uint32_t)E, Wd = (uint32_t)W, nb = (N + 63) / 64;
	hipStream_t st = ctx->stream;
	DevScope dev(st);
	double *A = nullptr, *dD = nullptr, *T = nullptr, *dlen = nullptr;
	int32_t *dpar = nullptr, *dkid = nullptr, *order = nullptr, *lev = nullptr, *lstart = nullptr;
	uint64_t *sets = nullptr;
	RefRec *drec = nullptr;
	dev.alloc(&A, E * n);
	if (dev.err != hipSuccess) {
		char msg[200];
		snprintf(msg, sizeof msg, "andi_hip_refine: the table of averages needs %zu bytes of device memory: %s",
				 E * n * sizeof(double), hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	dev.alloc(&dD, n * n), dev.alloc(&T, 4 * E), dev.alloc(&dlen, 2 * E), dev.alloc(&dpar, E), dev.alloc(&dkid, nkid);
	dev.alloc(&order, E), dev.alloc(&lev, E + 1), dev.alloc(&lstart, E + 2), dev.alloc(&sets, nsets ? nsets * W : 1), dev.alloc(&drec, 1);
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, n * n * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dpar, par.data(), E * sizeof(int32_t), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dkid, kid.data(), nkid * sizeof(int32_t), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		k_mirror<<<N, 256, 0, st>>>(dD, N);
		e = hipGetLastError();
	}
	std::vector<andi_hip_refine_move> moves; // (the caller's arrays are written on success only)
	RefRec rec;
	int converged = 0;
	while (e == hipSuccess) {
		k_order<<<1, 64, 0, st>>>(dkid, N, order, lev, lstart);
		if (nsets) k_rsets<<<1, LT, 0, st>>>(order, lstart, dkid, N, Wd, sets);
		k_table<<<nb, LT, 0, st>>>(dD, dkid, order, lstart, sets, N, Wd, A);
		k_sums<<<Ed, 256, 0, st>>>(A, dpar, dkid, sets, lev, N, Wd, T); // (4 Ed wavefronts, four a block)
		if (moves.empty()) k_blen<<<(Ed + 63) / 64, 64, 0, st>>>(T, dpar, dkid, N, dlen);
		k_choose<<<1, CT, 0, st>>>(T, dpar, dkid, N, tol, moves.size() < max_moves ? 1 : 0, drec);
		k_apply<<<1, 64, 0, st>>>(drec, dpar, dkid, sets, N, Wd);
		e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) break;
		if (rec.stop) {
			converged = rec.stop == 1;
			break;
		}
		andi_hip_refine_move m;
		m.gain = rec.gain, m.first = rec.first, m.second = rec.second;
		moves.push_back(m);
	}
	std::vector<double> len(2 * E);
	if (e == hipSuccess) {
		k_blen<<<(Ed + 63) / 64, 64, 0, st>>>(T, dpar, dkid, N, dlen + E);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(len.data(), dlen, 2 * E * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(kid.data(), dkid, nkid * sizeof(int32_t), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_refine", e);

	number_records(kid.data(), len.data() + E, n, out);
	andi_hip_refine_result r;
	memset(&r, 0, sizeof r);
	r.length_before = length_sum(len.data(), E), r.length_after = length_sum(len.data() + E, E);
	r.moves = moves.size(), r.converged = converged;
	*res = r;
	if (log && !moves.empty()) memcpy(log, moves.data(), moves.size() * sizeof(andi_hip_refine_move));
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Balanced subtree pruning and regrafting (andi_hip_refine_spr): the same rounds with a wider set of moves.  The tree is
// kept as three neighbour slots per inner node (nb), which a move rewires; every round orients it from C again:
//   k_orient   k_order on the slots: it also writes par and kid (the children of a node are its non-parent neighbours in
//              slot order), so k_rsets, k_table, k_sums and k_blen above run on the tree unchanged;
//   k_pre      one block, level by level: the nodes below every node and its preorder number, so that "y lies below x"
//              is two comparisons of wavefront-uniform against per-lane values;
//   k_leafrows B[x][.] of the leaves x: A transposed through LDS tiles, both sides in runs of 512 bytes;
//   k_pairs    k_table with an edge y where the leaf c was: block = 64 columns y x 16 wavefronts, the far sides below x the
//              deepest level first, then one wavefront down the path from C to y;
//   k_walk     thread = (pruned edge u, which side is pruned, which of v0's other two neighbours the path leaves by): the
//              other side depth-first, pending nodes with their R on a stack in global memory (entry d of thread t at
//              d * threads + t), the best candidate kept;
//   k_pick     one block: the greatest of the threads' bests by the contract's order (k_choose's pattern);
//   k_rehang   one wavefront: the least leaves of X and Z for the log, and the move in the slots.
// The host reads one record of 56 bytes a round; it carries the next tree's depth, which sizes the stacks.
static_assert(sizeof(andi_hip_spr_move) == 24, "andi_hip_spr_move: the gain, two leaves, the hops, pad");

namespace {

struct SprRec {
	double gain;
	int32_t x, v0, q, vk, w, hops, first, second, stop, depth;
	int32_t over, pad; // over: a walk's stack was too short (never, while the host sizes it from depth); the call fails
};

struct SprBest { // a thread's best candidate: the target edge f (-1: none), its ends and its hops
	int32_t f, vk, w, k;
};

// One wavefront: k_order on the neighbour slots; the tree's depth goes into the round's record.
__global__ __launch_bounds__(64) void k_orient(const int32_t *__restrict__ nb, uint32_t n, int32_t *par, int32_t *kid,
											   int32_t *order, int32_t *lev, int32_t *lstart, SprRec *rec) {
	const int32_t deepest = order_from_centre<true>(nb, n, par, kid, order, lev, lstart);
	if (threadIdx.x == 0) rec->depth = deepest;
}

// One block: sz[x], the nodes of the subtree of x, the deepest level first; then tin[x], x's preorder number among the
// non-centre nodes, the first level first.  y lies below x, or is x: tin[y] - tin[x] < sz[x], unsigned.
__global__ __launch_bounds__(LT) void k_pre(const int32_t *__restrict__ order, const int32_t *__restrict__ lstart,
											const int32_t *__restrict__ kid, uint32_t n, int32_t *sz, int32_t *tin) {
	const int32_t deepest = lstart[0];
	for (int32_t l = deepest; l >= 1; --l) {
		const uint32_t end = (uint32_t)lstart[l + 1];
		for (uint32_t i = (uint32_t)lstart[l] + threadIdx.x; i < end; i += LT) {
			const int32_t x = order[i];
			sz[x] = x < (int32_t)n ? 1 : 1 + sz[kid[2 * (size_t)(x - (int32_t)n)]] + sz[kid[2 * (size_t)(x - (int32_t)n) + 1]];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const int32_t *kc = kid + 2 * (size_t)(n - 3);
		tin[kc[0]] = 0, tin[kc[1]] = sz[kc[0]], tin[kc[2]] = sz[kc[0]] + sz[kc[1]];
	}
	__syncthreads();
	for (int32_t l = 1; l <= deepest; ++l) {
		const uint32_t end = (uint32_t)lstart[l + 1];
		for (uint32_t i = (uint32_t)lstart[l] + threadIdx.x; i < end; i += LT) {
			const int32_t x = order[i];
			if (x < (int32_t)n) continue;
			const int32_t a = kid[2 * (size_t)(x - (int32_t)n)], b = kid[2 * (size_t)(x - (int32_t)n) + 1];
			tin[a] = tin[x] + 1, tin[b] = tin[x] + 1 + sz[a];
		}
		__syncthreads();
	}
}

// Block = a tile of 64 leaves x by 64 edges y, four wavefronts: B[x][y] = A[y][x].
__global__ __launch_bounds__(256) void k_leafrows(const double *__restrict__ A, uint32_t n, double *__restrict__ B) {
	__shared__ double tile[64][65];
	const uint32_t E = 2 * n - 3, y0 = blockIdx.x * 64, x0 = blockIdx.y * 64, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t r = wave; r < 64; r += 4)
		if (y0 + r < E && x0 + lane < n) tile[r][lane] = A[(size_t)(y0 + r) * n + x0 + lane];
	__syncthreads();
	for (uint32_t r = wave; r < 64; r += 4)
		if (x0 + r < n && y0 + lane < E) B[(size_t)(x0 + r) * E + y0 + lane] = tile[lane][r];
}

// Block = 64 edges y (the lanes) x 16 wavefronts: B[x * E + y] for the inner nodes x; the leaves' rows are k_leafrows'.
__global__ __launch_bounds__(LT) void k_pairs(const int32_t *__restrict__ kid, const int32_t *__restrict__ order,
											  const int32_t *__restrict__ lstart, const int32_t *__restrict__ sz,
											  const int32_t *__restrict__ tin, uint32_t n, double *B) {
	const uint32_t E = 2 * n - 3, C = E, y = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6, NW = LT / 64;
	const bool live = y < E;
	const uint32_t ty = live ? (uint32_t)tin[y] : 0;
	for (int32_t l = lstart[0]; l >= 1; --l) { // the far side below x: the deepest level first
		const uint32_t end = (uint32_t)lstart[l + 1];
		for (uint32_t i = (uint32_t)lstart[l] + wave; i < end; i += NW) {
			const int32_t x = order[i];
			if (!live || x < (int32_t)n || ty - (uint32_t)tin[x] < (uint32_t)sz[x]) continue;
			const int32_t a = kid[2 * (size_t)(x - (int32_t)n)], b = kid[2 * (size_t)(x - (int32_t)n) + 1];
			B[(size_t)x * E + y] = (B[(size_t)a * E + y] + B[(size_t)b * E + y]) * 0.5;
		}
		__syncthreads();
	}
	if (wave != 0 || !live) return;
	// the far side above v, down the path from the centre to y, by one wavefront
	const int32_t *kc = kid + 2 * (size_t)(C - n);
	int32_t v = kc[0];
	if (!(ty - (uint32_t)tin[v] < (uint32_t)sz[v])) v = ty - (uint32_t)tin[kc[1]] < (uint32_t)sz[kc[1]] ? kc[1] : kc[2];
	int32_t o0, o1;
	others_of(kid, n, C, v, o0, o1);
	double up = (B[(size_t)o0 * E + y] + B[(size_t)o1 * E + y]) * 0.5;
	B[(size_t)v * E + y] = up;
	for (uint32_t step = 0; v != (int32_t)y && v >= (int32_t)n && step < E; ++step) { // (a path has fewer than E nodes)
		const int32_t a = kid[2 * (size_t)(v - (int32_t)n)], b = kid[2 * (size_t)(v - (int32_t)n) + 1];
		const bool in_a = ty - (uint32_t)tin[a] < (uint32_t)sz[a];
		const int32_t x = in_a ? a : b, s = in_a ? b : a;
		up = (B[(size_t)s * E + y] + up) * 0.5;
		B[(size_t)x * E + y] = up;
		v = x;
	}
}

// the two neighbours of inner node v but `from`, kids before the parent, in slot order
__device__ inline void beyond(const int32_t *par, const int32_t *kid, uint32_t n, int32_t v, int32_t from, int32_t &o0, int32_t &o1) {
	const int32_t *k = kid + 2 * (size_t)(v - (int32_t)n);
	if ((uint32_t)v == 2 * n - 3) {
		o0 = k[0] == from ? k[1] : k[0], o1 = k[2] == from ? k[1] : k[2];
		return;
	}
	const int32_t p = par[v];
	o0 = k[0] == from ? k[1] : k[0], o1 = p == from ? k[1] : p;
}

// the edge between the adjacent nodes a and b: its lower node
__device__ inline int32_t edge_of(const int32_t *par, uint32_t n, int32_t a, int32_t b) {
	return (uint32_t)b != 2 * n - 3 && par[b] == a ? b : a;
}

// candidate t = 4 u + 2 side + way: the pruned node x, its neighbour v0, and v0's other two: q where the path leaves, p.
// false: no such candidate (the upper side of a leaf edge).
__device__ inline bool pruned_of(const int32_t *par, const int32_t *kid, uint32_t n, uint32_t t, int32_t &x, int32_t &v0, int32_t &p,
								 int32_t &q) {
	const int32_t u = (int32_t)(t >> 2);
	const bool up = t & 2, second = t & 1;
	if (up && u < (int32_t)n) return false;
	x = up ? par[u] : u, v0 = up ? u : par[u];
	int32_t o0, o1;
	beyond(par, kid, n, v0, x, o0, o1);
	q = second ? o1 : o0, p = second ? o0 : o1;
	return true;
}

// candidate (g, i) comes before (G, I), as before() above, on the wider index of the SPR candidates
__device__ inline bool before64(double g, int64_t i, double G, int64_t I) {
	if (I < 0) return true;
	if (i < 0) return false;
	const bool gn = __builtin_isnan(g), Gn = __builtin_isnan(G);
	if (gn || Gn) return gn == Gn ? i < I : Gn;
	return g > G || (g == G && i < I);
}

// Thread t: the best target edge of candidate t.  SR, SN: the stacks, cap entries a thread.
__global__ __launch_bounds__(64) void k_walk(const double *__restrict__ B, const int32_t *__restrict__ par,
											 const int32_t *__restrict__ kid, uint32_t n, uint32_t cap, double *SR, int4 *SN,
											 double *__restrict__ bg, SprBest *__restrict__ bb, SprRec *rec) {
	const uint32_t E = 2 * n - 3, NT = 4 * E, t = blockIdx.x * 64 + threadIdx.x;
	if (t >= NT) return;
	double G = 0.0;
	SprBest best = {-1, -1, -1, 0};
	int32_t x, v0, p, q;
	if (pruned_of(par, kid, n, t, x, v0, p, q) && q >= (int32_t)n && cap > 0) {
		const int32_t ep = edge_of(par, n, v0, p), e1 = edge_of(par, n, v0, q);
		const double *Bx = B + (size_t)(t >> 2) * E, *By = B + (size_t)ep * E;
		const double dXY0 = Bx[ep], dXW = Bx[e1], dYW = By[e1];
		uint32_t sp = 1;
		SR[t] = 0.0, SN[t] = make_int4(q, v0, 0, 0);
		while (sp > 0) {
			--sp;
			const int4 fr = SN[(size_t)sp * NT + t];
			const double Rp = SR[(size_t)sp * NT + t];
			const int32_t v = fr.x, k = fr.z + 1;
			int32_t o[2];
			beyond(par, kid, n, v, fr.y, o[0], o[1]);
			const double h = k > 1022 ? 0.0 : __longlong_as_double((long long)(1023 - k) << 52);
			for (int j = 0; j < 2; ++j) {
				const int32_t w = o[j], f = edge_of(par, n, v, w);
				const double R = 0.5 * Rp + Bx[edge_of(par, n, v, o[1 - j])];
				const double dXZ = Bx[f], dYZ = By[f], Bff = B[(size_t)f * E + f];
				const double t1 = (0.5 * (1.0 - h)) * (dXY0 - dXZ), t2 = 0.5 * dXW - (0.5 * h) * dXZ;
				const double t3 = 0.5 * dYW - (0.5 * h) * dYZ, t4 = 0.5 * Bff - (0.25 * h) * (dYZ + dXZ);
				const double g = (((t1 + t2) - t3) + t4) - 0.25 * R;
				if (before64(g, f, G, best.f)) G = g, best = {f, v, w, k};
				if (w < (int32_t)n) continue;
				if (sp < cap) { // (pending entries: one per node of the path and one more; cap holds them)
					SR[(size_t)sp * NT + t] = R, SN[(size_t)sp * NT + t] = make_int4(w, v, k, 0);
					++sp;
				} else rec->over = 1;
			}
		}
	}
	bg[t] = G, bb[t] = best;
}

// One block: the greatest of the 4 E bests, index (2 u + side) E + f, and whether the search goes on.
__global__ __launch_bounds__(CT) void k_pick(const double *__restrict__ bg, const SprBest *__restrict__ bb,
											 const int32_t *__restrict__ par, const int32_t *__restrict__ kid, uint32_t n, double tol,
											 int can_move, SprRec *__restrict__ rec) {
	__shared__ double sg[CT];
	__shared__ int64_t si[CT];
	__shared__ uint32_t st[CT];
	const uint32_t E = 2 * n - 3;
	double G = 0.0;
	int64_t I = -1;
	uint32_t Tb = 0;
	for (uint32_t t = threadIdx.x; t < 4 * E; t += CT) {
		const int32_t f = bb[t].f;
		const int64_t i = f < 0 ? -1 : (int64_t)(t >> 1) * E + f;
		if (before64(bg[t], i, G, I)) G = bg[t], I = i, Tb = t;
	}
	sg[threadIdx.x] = G, si[threadIdx.x] = I, st[threadIdx.x] = Tb;
	__syncthreads();
	for (uint32_t h = CT / 2; h > 0; h >>= 1) {
		if (threadIdx.x < h && before64(sg[threadIdx.x + h], si[threadIdx.x + h], sg[threadIdx.x], si[threadIdx.x]))
			sg[threadIdx.x] = sg[threadIdx.x + h], si[threadIdx.x] = si[threadIdx.x + h], st[threadIdx.x] = st[threadIdx.x + h];
		__syncthreads();
	}
	if (threadIdx.x != 0) return;
	G = sg[0], I = si[0], Tb = st[0];
	rec->gain = I < 0 ? 0.0 : G;
	rec->x = -1, rec->v0 = rec->q = rec->vk = rec->w = -1, rec->hops = 0, rec->first = rec->second = -1;
	if (I >= 0) {
		int32_t x, v0, p, q;
		pruned_of(par, kid, n, Tb, x, v0, p, q);
		rec->x = x, rec->v0 = v0, rec->q = q, rec->vk = bb[Tb].vk, rec->w = bb[Tb].w, rec->hops = bb[Tb].k;
	}
	rec->stop = (I < 0 || !(G > tol)) ? 1 : can_move ? 0 : 2;
}

// the least leaf that is not below x, by one wavefront
__device__ inline int32_t least_outside(const uint64_t *sets, uint32_t n, uint32_t W, int32_t x, uint32_t lane) {
	if (x < (int32_t)n) return x == 0 ? 1 : 0;
	uint32_t m = ~0u;
	const uint64_t *set = sets + (size_t)(x - (int32_t)n) * W;
	for (uint32_t w = lane; w < W; w += 64) {
		const uint64_t word = ~set[w] & (w + 1 == W && (n & 63) ? (1ull << (n & 63)) - 1 : ~0ull);
		if (word && m == ~0u) m = w * 64 + (uint32_t)__builtin_ctzll(word);
	}
	for (int s = 32; s > 0; s >>= 1) {
		const uint32_t o = __shfl_xor(m, s);
		m = o < m ? o : m;
	}
	return (int32_t)m;
}

// the slot of inner node i that holds t
__device__ inline int32_t *slot_of(int32_t *nb, uint32_t n, int32_t i, int32_t t) {
	int32_t *s = nb + 3 * (size_t)(i - (int32_t)n);
	return s[0] == t ? s : s[1] == t ? s + 1 : s + 2;
}

// One wavefront: the least leaves of X and Z into the record; if the search goes on, the move in the slots.
__global__ __launch_bounds__(64) void k_rehang(SprRec *rec, int32_t *nb, const int32_t *__restrict__ par,
											   const uint64_t *__restrict__ sets, uint32_t n, uint32_t W) {
	const int32_t x = rec->x, v0 = rec->v0, q = rec->q, vk = rec->vk, w = rec->w, stop = rec->stop;
	if (x < 0) return;
	const uint32_t C = 2 * n - 3, lane = threadIdx.x;
	const bool x_below = (uint32_t)x != C && par[x] == v0, w_below = (uint32_t)w != C && par[w] == vk;
	const int32_t first = x_below ? least_leaf(sets, n, W, x, lane) : least_outside(sets, n, W, v0, lane);
	const int32_t second = w_below ? least_leaf(sets, n, W, w, lane) : least_outside(sets, n, W, vk, lane);
	if (lane != 0) return;
	rec->first = first, rec->second = second;
	if (stop) return;
	int32_t *s0 = nb + 3 * (size_t)(v0 - (int32_t)n);
	const int32_t p = s0[0] != x && s0[0] != q ? s0[0] : s0[1] != x && s0[1] != q ? s0[1] : s0[2];
	int32_t *in_p = p >= (int32_t)n ? slot_of(nb, n, p, v0) : nullptr, *in_q = q >= (int32_t)n ? slot_of(nb, n, q, v0) : nullptr;
	int32_t *of_p = slot_of(nb, n, v0, p), *of_q = slot_of(nb, n, v0, q), *in_k = slot_of(nb, n, vk, w);
	int32_t *in_w = w >= (int32_t)n ? slot_of(nb, n, w, vk) : nullptr;
	if (in_p) *in_p = q;
	if (in_q) *in_q = p;
	*of_p = vk, *of_q = w, *in_k = v0;
	if (in_w) *in_w = v0;
}

} // namespace

int andi_hip_refine_spr(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, double tol, size_t max_moves,
						andi_hip_nj_join *out, andi_hip_refine_result *res, andi_hip_spr_move *log) {
	if (!ctx || !tree || !D || !out || !res || n < 3 || n > 65535 || !(tol >= 0)) {
		if (ctx) ctx->err = "andi_hip_refine_spr: bad arguments (ctx, tree, D, out and res must be given, 3 <= n <= 65535, tol >= 0)";
		return 1;
	}
	const size_t E = 2 * n - 3, C = E, nsets = n - 3, W = (n + 63) / 64, nkid = 2 * nsets + 3, NT = 4 * E;
	std::vector<int32_t> par(E), kid(nkid), slots(3 * (n - 2));
	if (!tree_input_ok(ctx, "andi_hip_refine_spr", tree, n, D, par.data(), kid.data())) return 1;
	for (size_t i = n; i <= C; ++i) {
		int32_t *s = slots.data() + 3 * (i - n);
		s[0] = kid[2 * (i - n)], s[1] = kid[2 * (i - n) + 1], s[2] = i == C ? kid[2 * (i - n) + 2] : par[i];
	}

	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t N = (uint32_t)n, Ed = (uint32_t)E, Wd = (uint32_t)W, nb = (N + 63) / 64, eb = (Ed + 63) / 64;
	hipStream_t st = ctx->stream;
	DevScope dev(st), stacks(st);
	double *A = nullptr, *B = nullptr, *dD = nullptr, *T = nullptr, *dlen = nullptr, *bg = nullptr, *SR = nullptr;
	int32_t *dnb = nullptr, *dpar = nullptr, *dkid = nullptr, *order = nullptr, *lev = nullptr, *lstart = nullptr, *sz = nullptr, *tin = nullptr;
	uint64_t *sets = nullptr;
	SprBest *bb = nullptr;
	int4 *SN = nullptr;
	SprRec *drec = nullptr;
	dev.alloc(&B, E * E), dev.alloc(&A, E * n);
	if (dev.err != hipSuccess) {
		char msg[240];
		snprintf(msg, sizeof msg, "andi_hip_refine_spr: the tables of averages need %zu + %zu bytes of device memory: %s",
				 E * E * sizeof(double), E * n * sizeof(double), hipGetErrorString(dev.err));
		(void)hipGetLastError();
		ctx->err = msg;
		return 1;
	}
	dev.alloc(&dD, n * n), dev.alloc(&T, 4 * E), dev.alloc(&dlen, 2 * E), dev.alloc(&dpar, E + 1), dev.alloc(&dkid, nkid);
	dev.alloc(&dnb, slots.size()), dev.alloc(&order, E), dev.alloc(&lev, E + 1), dev.alloc(&lstart, E + 2), dev.alloc(&sz, E);
	dev.alloc(&tin, E), dev.alloc(&sets, nsets ? nsets * W : 1), dev.alloc(&bg, NT), dev.alloc(&bb, NT), dev.alloc(&drec, 1);
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, n * n * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dnb, slots.data(), slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
	SprRec rec;
	if (e == hipSuccess) e = hipMemsetAsync(drec, 0, sizeof rec, st);
	if (e == hipSuccess) {
		k_mirror<<<N, 256, 0, st>>>(dD, N);
		k_orient<<<1, 64, 0, st>>>(dnb, N, dpar, dkid, order, lev, lstart, drec);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	std::vector<andi_hip_spr_move> moves; // (the caller's arrays are written on success only)
	int converged = 0;
	size_t cap = 0;
	while (e == hipSuccess) {
		const size_t need = 2 * (size_t)rec.depth + 2; // a path has at most 2 depth edges
		if (need > cap) {
			stacks.release();
			cap = need;
			stacks.alloc(&SR, cap * NT), stacks.alloc(&SN, cap * NT);
			if (stacks.err != hipSuccess) {
				char msg[240];
				snprintf(msg, sizeof msg, "andi_hip_refine_spr: the walk's stacks need %zu bytes of device memory (depth %d): %s",
						 cap * NT * (sizeof(double) + sizeof(int4)), rec.depth, hipGetErrorString(stacks.err));
				(void)hipGetLastError();
				ctx->err = msg;
				return 1;
			}
		}
		if (nsets) k_rsets<<<1, LT, 0, st>>>(order, lstart, dkid, N, Wd, sets);
		k_pre<<<1, LT, 0, st>>>(order, lstart, dkid, N, sz, tin);
		k_table<<<nb, LT, 0, st>>>(dD, dkid, order, lstart, sets, N, Wd, A);
		k_sums<<<Ed, 256, 0, st>>>(A, dpar, dkid, sets, lev, N, Wd, T);
		if (moves.empty()) k_blen<<<eb, 64, 0, st>>>(T, dpar, dkid, N, dlen);
		k_leafrows<<<dim3(eb, nb), 256, 0, st>>>(A, N, B);
		k_pairs<<<eb, LT, 0, st>>>(dkid, order, lstart, sz, tin, N, B);
		k_walk<<<(uint32_t)(NT + 63) / 64, 64, 0, st>>>(B, dpar, dkid, N, (uint32_t)cap, SR, SN, bg, bb, drec);
		k_pick<<<1, CT, 0, st>>>(bg, bb, dpar, dkid, N, tol, moves.size() < max_moves ? 1 : 0, drec);
		k_rehang<<<1, 64, 0, st>>>(drec, dnb, dpar, sets, N, Wd);
		k_orient<<<1, 64, 0, st>>>(dnb, N, dpar, dkid, order, lev, lstart, drec); // (a stop leaves the slots: the same tree again)
		e = hipGetLastError();
		if (e == hipSuccess) e = hipMemcpyAsync(&rec, drec, sizeof rec, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess) break;
		if (rec.over) {
			ctx->err = "andi_hip_refine_spr: a walk's stack was too short for the tree's depth (a bug: the result is not used)";
			return 1;
		}
		if (rec.stop) {
			converged = rec.stop == 1;
			break;
		}
		andi_hip_spr_move m;
		m.gain = rec.gain, m.first = rec.first, m.second = rec.second, m.hops = rec.hops, m.pad = 0;
		moves.push_back(m);
	}
	std::vector<double> len(2 * E);
	if (e == hipSuccess) {
		k_blen<<<eb, 64, 0, st>>>(T, dpar, dkid, N, dlen + E);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(len.data(), dlen, 2 * E * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(kid.data(), dkid, nkid * sizeof(int32_t), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(ctx, "andi_hip_refine_spr", e);

	number_records(kid.data(), len.data() + E, n, out);
	andi_hip_refine_result r;
	memset(&r, 0, sizeof r);
	r.length_before = length_sum(len.data(), E), r.length_after = length_sum(len.data() + E, E);
	r.moves = moves.size(), r.converged = converged;
	*res = r;
	if (log && !moves.empty()) memcpy(log, moves.data(), moves.size() * sizeof(andi_hip_spr_move));
	return 0;
}
