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
__global__ __launch_bounds__(64) void k_order(const int32_t *__restrict__ kid, uint32_t n, int32_t *order, int32_t *lev,
											  int32_t *lstart) {
	const uint32_t E = 2 * n - 3, C = E, lane = threadIdx.x;
	if (lane < 3) {
		const int32_t x = kid[2 * (size_t)(C - n) + lane];
		order[lane] = x, lev[x] = 1;
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
			const int32_t a = kid[2 * (size_t)(x - (int32_t)n)], b = kid[2 * (size_t)(x - (int32_t)n) + 1], l = lev[x] + 1;
			if (at + 1 < E) order[at] = a, order[at + 1] = b, lev[a] = l, lev[b] = l; // (a tree's nodes are queued once each: it fits)
		}
		head += tail - head < 64 ? tail - head : 64;
		tail += 2 * (uint32_t)__popcll(m);
		if (tail > E) tail = E;
		__syncthreads();
	}
	if (lane == 0) {
		const int32_t deepest = lev[order[E - 1]];
		lstart[0] = deepest, lstart[deepest + 1] = (int32_t)E;
	}
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

} // namespace

int andi_hip_refine(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, int method, double tol,
					size_t max_moves, andi_hip_nj_join *out, andi_hip_refine_result *res, andi_hip_refine_move *log) {
	if (!ctx || !tree || !D || !out || !res || n < 3 || n > 65535 || method != ANDI_REFINE_BNNI || !(tol >= 0)) {
		if (ctx)
			ctx->err = "andi_hip_refine: bad arguments (ctx, tree, D, out and res must be given, 3 <= n <= 65535, method BNNI, "
					   "tol >= 0)";
		return 1;
	}
	const size_t E = 2 * n - 3, C = E, nsets = n - 3, W = (n + 63) / 64, nkid = 2 * nsets + 3;
	std::vector<uint8_t> seen(2 * n);
	std::vector<int2> pairs(nsets ? nsets : 1);
	if (!records_ok(tree, n, seen.data(), pairs.data())) {
		ctx->err = "andi_hip_refine: the tree's records are not those of andi_hip_nj";
		return 1;
	}
	for (size_t i = 0; i < n; ++i)
		for (size_t j = i + 1; j < n; ++j)
			if (!std::isfinite(D[i * n + j])) {
				char msg[160];
				snprintf(msg, sizeof msg, "andi_hip_refine: D[%zu][%zu] is not finite (%g)", i, j, D[i * n + j]);
				ctx->err = msg;
				return 1;
			}
	std::vector<int32_t> par(E), kid(nkid);
	for (size_t s = 0; s + 2 < n; ++s) {
		const bool last = s + 3 == n;
		const int32_t ch[3] = {tree[s].a, tree[s].b, tree[s].c};
		for (int k = 0; k < (last ? 3 : 2); ++k) par[ch[k]] = (int32_t)(last ? C : n + s), kid[2 * s + k] = ch[k];
	}

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
