// linkage.hip — agglomerative (linkage) clustering of a distance matrix on the device (andi_hip_linkage, include/andi_hip.h):
// single, complete and average (UPGMA) linkage, bit for bit the contract in andi_hip.h (tests/linkage_model.py restates it
// in NumPy).  PHYLIP's neighbor, which --tree replaces, has a UPGMA mode; this is its counterpart, and unlike
// neighbor-joining it takes a pair without a distance (+inf: farther than anything measurable).
//
// The layout is nj.hip's: D resident as doubles indexed by SLOT (leaf i starts in slot i, a join's node takes the lower
// slot of its two children, the other slot retires), the active slots an ascending compacted list ping-ponged between two
// buffers, the REPLICATE as every grid's second dimension (andi_hip_linkage_batch; the single call is the group of one),
// no host synchronisation between steps, no grid-wide barrier, no in-launch hand-off between blocks, one D2H copy of the
// records at the end.  The host code around a group's steps is not a copy of nj.hip's but the same code (rep_groups.h:
// the group's size and buffers, the loop over the groups, what happens to an unusable matrix, the buffers' lifetime).
//
// Unlike nj.hip no step searches the active triangle.  Every active row keeps its NEAREST NEIGHBOUR: nn[x], the least
// (d, id_lo, id_hi) over the pairs of x with every other active slot, in the contract's order (better(), nj_cand.h).  The
// least pair of the whole triangle is the least of the r cached entries, because it is the least entry of both of its
// rows.  A step with r active nodes is two launches:
//   k_link_join  one block per replicate: the least of the r cached entries, the record, the new node's row and column by
//                the method's rule, its size and id, the list compacted, and {slot a, slot b, slot u} left for
//   k_link_nn    one wavefront per row of the r - 1 that remain: the new node's own row, and every row whose cached pair
//                held a or b (that pair no longer exists), scan their r - 1 entries again, all loads of a wavefront in
//                flight at once; every other row only compares its cached entry with its one new entry D[k][u].
// The rescan is the same for all three methods.  Single linkage looks as if it needed none but the new row's -- the new
// D[k][u] has the cached value when k's neighbour was a or b -- but the new pair carries the id n + s, the largest there
// is, so on a TIE every other entry of the row now orders before it; a cache that kept (d, k, u) there would hand
// k_link_join a pair that is not the least one.  Work per matrix: n^2 for the first caches, then r per step plus
// r per rescanned row -- ~n^2 in all on distinct distances, ~n^3 / 3 when every distance ties (every row rescans).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "api_internal.h"
#include "nj_cand.h"
#include "rep_groups.h"

static_assert(sizeof(andi_hip_link) == 24, "andi_hip_link: 2 ids, size, pad, height");

namespace {

constexpr int NN_CHUNKS = 8; // k_link_nn: 8 x 64 entries of a row in flight per wavefront
constexpr int JOIN_THREADS = 1024;

// the slots of a replicate's last join, from k_link_join to k_link_nn
struct Joined {
	int32_t sa, sb, su, pad;
};

// Mirror the upper triangle (row i = block i), a NaN taken as +inf, diagonal +0.0; the first -inf D[i][j], i < j, in
// row-major order goes to the replicate's bad word as i * n + j.  act = id = identity, every size 1.  (Block j reads
// D[i][j], i < j, while block i may be replacing a NaN there: both make +inf of it, whichever the read sees.)
__global__ __launch_bounds__(256) void k_link_init(double *__restrict__ D, uint32_t n, int32_t *__restrict__ lists,
												   uint32_t *__restrict__ size, unsigned long long *bad) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, bad += rep, size += rep * n;
	int32_t *act = lists + rep * 3 * n, *id = act + 2 * (size_t)n;
	const uint32_t i = blockIdx.x;
	double *row = D + (size_t)i * n;
	const double inf = __builtin_inf();
	unsigned long long first = ~0ull;
	for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
		if (j > i) {
			const double v = row[j];
			if (__builtin_isnan(v)) row[j] = inf;
			else if (v == -inf && first == ~0ull) first = (unsigned long long)i * n + j;
		} else if (j < i) {
			const double v = D[(size_t)j * n + i];
			row[j] = __builtin_isnan(v) ? inf : v;
		} else {
			row[j] = 0.0;
		}
	}
	if (first != ~0ull) atomicMin(bad, first);
	if (threadIdx.x == 0) act[i] = (int32_t)i, id[i] = (int32_t)i, size[i] = 1;
}

// nn[k] for the r active rows k = act[x], one wavefront per row.  all != 0 (before the first step): every row scans its r
// entries.  Otherwise (behind step `step`, whose k_link_join left its slots in `joined`): the new node's row and the rows
// whose cached pair held slot a or b scan; the others compare their cached pair with (D[k][u], id k, id u).
__global__ __launch_bounds__(256) void k_link_nn(const double *__restrict__ D, uint32_t n, const int32_t *__restrict__ lists,
												 uint32_t cur, uint32_t r, Cand *__restrict__ nn,
												 const Joined *__restrict__ joined, int all) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, nn += rep * n, joined += rep;
	const int32_t *act = lists + rep * 3 * n + cur, *id = lists + rep * 3 * n + 2 * (size_t)n;
	const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (x >= r) return;
	const int32_t k = act[x], ik = id[k];
	const double *row = D + (size_t)k * n;
	if (!all) {
		const Joined j = *joined;
		Cand c = nn[k];
		if (k != j.su && c.sa != j.sa && c.sa != j.sb && c.sb != j.sa && c.sb != j.sb) {
			if (lane == 0) {
				const int32_t iu = id[j.su];
				const double v = row[j.su];
				const Cand cand = ik < iu ? Cand{v, ik, iu, k, j.su} : Cand{v, iu, ik, j.su, k};
				if (better(cand, c)) nn[k] = cand;
			}
			return;
		}
	}
	Cand best = none();
	for (uint32_t base = 0; base < r; base += 64 * NN_CHUNKS) {
		double v[NN_CHUNKS];
		int32_t y[NN_CHUNKS];
#pragma unroll
		for (int c = 0; c < NN_CHUNKS; ++c) {
			const uint32_t p = base + 64 * c + lane;
			y[c] = p < r ? act[p] : -1;
			v[c] = p < r ? row[y[c]] : 0.0;
		}
#pragma unroll
		for (int c = 0; c < NN_CHUNKS; ++c) {
			if (y[c] < 0 || y[c] == k) continue;
			const int32_t iy = id[y[c]];
			const Cand cand = ik < iy ? Cand{v[c], ik, iy, k, y[c]} : Cand{v[c], iy, ik, y[c], k};
			if (better(cand, best)) best = cand;
		}
	}
	best = wave_min(best);
	if (lane == 0) nn[k] = best;
}

// One block per replicate: the least of the r cached pairs, its record, node u = n + step in the lower slot with its row
// and column by the method's rule, the other slot retired (the list at cur -> the other list, order kept).
__global__ __launch_bounds__(JOIN_THREADS) void k_link_join(double *__restrict__ D, uint32_t n, int32_t *__restrict__ lists,
															uint32_t cur, uint32_t r, const Cand *__restrict__ nn,
															uint32_t *__restrict__ size, Joined *__restrict__ joined,
															andi_hip_link *__restrict__ rec, uint32_t step, int method) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, nn += rep * n, size += rep * n, joined += rep, rec += rep * (n - 1);
	const int32_t *act_in = lists + rep * 3 * n + cur;
	int32_t *act_out = lists + rep * 3 * n + (n - cur), *id = lists + rep * 3 * n + 2 * (size_t)n;
	Cand best = none();
	for (uint32_t i = threadIdx.x; i < r; i += blockDim.x) {
		const Cand c = nn[act_in[i]];
		if (better(c, best)) best = c;
	}
	best = block_min(best);
	const size_t sa = (size_t)best.sa, sb = (size_t)best.sb; // a: the member of smaller id
	const size_t su = sa < sb ? sa : sb, so = sa < sb ? sb : sa;
	const double d = D[sa * n + sb];
	const uint32_t na = size[sa], nb = size[sb];
	const double fa = (double)na, fb = (double)nb, fs = (double)(na + nb);
	if (threadIdx.x == 0) {
		andi_hip_link l;
		l.a = best.ia, l.b = best.ib, l.size = na + nb, l.pad = 0, l.height = d;
		rec[step] = l;
		*joined = Joined{(int32_t)sa, (int32_t)sb, (int32_t)su, 0};
	}
	for (uint32_t i = threadIdx.x; i < r; i += blockDim.x) {
		const size_t k = (size_t)act_in[i];
		if (k == so) continue;
		act_out[i - (k > so)] = (int32_t)k;
		if (k == su) continue;
		const double da = D[sa * n + k], db = D[sb * n + k];
		double v;
		if (method == ANDI_LINK_SINGLE) v = db < da ? db : da;
		else if (method == ANDI_LINK_COMPLETE) v = db > da ? db : da;
		else v = (fa * da + fb * db) / fs;
		D[su * n + k] = v;
		D[k * n + su] = v;
	}
	__syncthreads(); // (every thread has read the sizes of a and b)
	if (threadIdx.x == 0) {
		size[su] = na + nb;
		id[su] = (int32_t)(n + step);
	}
}

// the buffers of a group of g replicates of n x n, one replicate after the other in each (rep_groups.h: alloc_group)
struct LinkBuffers {
	double *D = nullptr;
	Cand *nn = nullptr;
	int32_t *lists = nullptr; // per replicate: two act lists, the ids
	uint32_t *size = nullptr;
	Joined *joined = nullptr;
	andi_hip_link *rec = nullptr;
	unsigned long long *bad = nullptr;

	// device bytes of one replicate: D, the caches, the lists, the sizes, the last join's slots, the records, the bad word
	static size_t replicate_bytes(size_t n) {
		return n * n * sizeof(double) + n * sizeof(Cand) + 3 * n * sizeof(int32_t) + n * sizeof(uint32_t) + sizeof(Joined) +
			   (n - 1) * sizeof(andi_hip_link) + sizeof(unsigned long long);
	}
	hipError_t alloc(DevScope &dev, size_t n, size_t g) {
		dev.alloc(&D, g * n * n), dev.alloc(&nn, g * n), dev.alloc(&lists, g * 3 * n), dev.alloc(&size, g * n);
		dev.alloc(&joined, g), dev.alloc(&rec, g * (n - 1)), dev.alloc(&bad, g);
		return dev.err;
	}
};

// The clustering of g host matrices (one after the other) in buffers for at least g, between group_begin and group_end
// (rep_groups.h: what bad is; the init kernel is k_link_init, an unusable entry a -inf): links receives the records of all
// g when at least one matrix is usable -- and nothing when none is.  Synchronous; no host synchronisation between steps.
hipError_t link_group(andi_hip_ctx *ctx, const LinkBuffers &b, const double *D, uint32_t N, uint32_t g, int method,
					  andi_hip_link *links, unsigned long long *bad) {
	const size_t n = N;
	hipStream_t st = ctx->stream;
	bool any_good;
	hipError_t e = group_begin(
		st, b.D, D, n, g, b.bad, bad, nullptr, [&] { k_link_init<<<dim3(N, g), 256, 0, st>>>(b.D, N, b.lists, b.size, b.bad); },
		any_good);
	if (e != hipSuccess || !any_good) return e;
	uint32_t cur = 0; // where in a replicate's lists the current act list starts: 0 or n
	k_link_nn<<<dim3((N + 3) / 4, g), 256, 0, st>>>(b.D, N, b.lists, cur, N, b.nn, b.joined, 1);
	e = hipGetLastError();
	for (uint32_t s = 0; e == hipSuccess && s + 1 < N; ++s) {
		const uint32_t r = N - s;
		k_link_join<<<dim3(1, g), JOIN_THREADS, 0, st>>>(b.D, N, b.lists, cur, r, b.nn, b.size, b.joined, b.rec, s, method);
		cur = N - cur;
		if (r - 1 >= 2) k_link_nn<<<dim3((r - 1 + 3) / 4, g), 256, 0, st>>>(b.D, N, b.lists, cur, r - 1, b.nn, b.joined, 0);
		e = hipGetLastError();
	}
	return e == hipSuccess ? group_end(st, links, b.rec, g * (n - 1)) : e;
}

bool bad_method(int method) { return method != ANDI_LINK_SINGLE && method != ANDI_LINK_COMPLETE && method != ANDI_LINK_AVERAGE; }

} // namespace

int andi_hip_linkage(andi_hip_ctx *ctx, const double *D, size_t n, int method, andi_hip_link *links) {
	if (!ctx || !D || !links || n < 2 || n > 65535 || bad_method(method)) {
		if (ctx)
			ctx->err = "andi_hip_linkage: bad arguments (ctx, D and links must be given, 2 <= n <= 65535, method single, "
					   "complete or average)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	LinkBuffers b;
	unsigned long long bad = NOT_BAD;
	hipError_t e = b.alloc(dev, n, 1);
	if (e == hipSuccess) e = link_group(ctx, b, D, (uint32_t)n, 1, method, links, &bad); // (an unusable matrix: nothing reaches links)
	if (e != hipSuccess) return fail(ctx, "andi_hip_linkage", e);
	if (bad != NOT_BAD) {
		const Entry at = bad_entry(bad, n);
		char msg[160];
		snprintf(msg, sizeof msg, "andi_hip_linkage: D[%zu][%zu] is -inf", at.i, at.j);
		ctx->err = msg;
		return 1;
	}
	return 0;
}

int andi_hip_linkage_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, int method, andi_hip_link *links,
						   int64_t *bad) {
	if (!ctx || !D || !links || !bad || count == 0 || n < 2 || n > 65535 || bad_method(method)) {
		if (ctx)
			ctx->err = "andi_hip_linkage_batch: bad arguments (ctx, D, links and bad must be given, count >= 1, 2 <= n <= 65535, "
					   "method single, complete or average)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	LinkBuffers b;
	size_t G = 0;
	hipError_t e = alloc_group(dev, b, n, count, G);
	if (e == hipSuccess)
		e = for_groups(count, G, n - 1, links, bad, [&](size_t first, size_t g, andi_hip_link *L, unsigned long long *hb) {
			return link_group(ctx, b, D + first * n * n, (uint32_t)n, (uint32_t)g, method, L, hb);
		});
	if (e != hipSuccess) return fail(ctx, "andi_hip_linkage_batch", e);
	return 0;
}
