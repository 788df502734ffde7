// complete.hip — missing distances estimated from quartets on the device (andi_hip_complete, andi_hip_complete_batch,
// include/andi_hip.h), bit for bit the contract there (tests/complete_model.py restates it in NumPy): a pair without a
// distance gets the least of max(D[i][k] + D[j][l], D[i][l] + D[j][k]) - D[k][l] over the pairs {k, l} whose five distances
// are known (the four-point condition), round after round, every round reading the matrix as it stood at the round's start.
//
// The layout is linkage.hip's: the matrices resident as doubles, the REPLICATE as every grid's second dimension (the single
// call is the group of one), the groups taken through rep_groups.h.  A group is
//   k_complete_init      one wavefront per row: mirrors the upper triangle (a missing entry becomes the quiet NaN, the
//                        diagonal +0.0) and counts the row's missing pairs;
//   k_complete_scan      one block per replicate: the rows' offsets into the replicate's list and into its items;
//   (the host reads every replicate's counts, sizes the list and the items by them -- sketch.hip's count-then-fill)
//   k_complete_list      one wavefront per row: the row's missing pairs in ascending j, and its ITEMS: up to P consecutive
//                        missing partners of one row, the work of one block;
// and per round
//   k_complete_quartets  one block per item, the hot path: writes the round's fills into the list, not into D;
//   k_complete_apply     commits them to D (both triangles) -- this is what makes the round Jacobi;
//   (the host reads the replicates' counters of fills and goes on while one of them is not zero).
//
// k_complete_quartets.  A block owns row i and up to P of its missing partners j_q.  Columns go by chunks of CH: the block
// stages a[l] = D[i][l] and b_q[l] = D[j_q][l] of a chunk in LDS, an unusable one as +inf, with the mask of the q for which
// column l is usable at all (both known, and l not i).  Then every wavefront takes one k < the chunk's end at a time -- its
// a[k] and b_q[k] are wave-uniform -- and its 64 lanes run over the chunk's l > k, reading row k of D from global memory in
// aligned 512-byte loads: one load of D[k][l] serves P candidates.  A lane keeps a minimum and a count per q; a candidate
// counts iff the masks of k and l and the finiteness of D[k][l] say so, and only then does its value meet the minimum, so
// no NaN is ever compared.  Reduction: across the wavefront by shuffles, across the block through a few LDS words.
// LDS: CH * (8 * (1 + P) + 4) = 28 KiB a block of 4 wavefronts, so 5 blocks (20 wavefronts) a CU of 160 KiB.
// Traffic: a block reads the upper triangle of D once (38 MB at 3085 leaves: from the Infinity Cache, not from L2), P
// partners share it.  Work: (n - 2)(n - 3) / 2 candidates per missing pair and round at most.
// P: measured at 3085 leaves with 1 % and 10 % of the pairs missing, the whole call took 0.270 / 2.09 s with P = 1,
// 0.231 / 1.78 s with 2, 0.246 / 1.78 s with 4 and 0.279 / 1.92 s with 8: sharing the load is worth 15 %, not more -- the
// kernel is bound by its vector instructions, not by the cache -- and a block whose row has fewer
// partners left than P computes the empty places too (a row has 15 missing partners on average at 1 %), which is what a
// larger P loses again.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "api_internal.h"
#include "rep_groups.h"

static_assert(sizeof(andi_hip_fill) == 32, "andi_hip_fill: i, j, round, pad, quartets, value");

namespace {

constexpr int CH = 1024;              // columns of a row staged in LDS at a time (tests/test_complete_gpu.py reads this line)
constexpr int P = 2;                  // missing partners of one row that a block serves per load of D[k][l] (and this one)
constexpr int QT = 256, QW = QT / 64; // k_complete_quartets: threads, wavefronts

__device__ inline double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline bool known(double v) { return __builtin_isfinite(v); }

// an item: `count` (1 ... P) consecutive entries of a replicate's list from `start` on, all of one row
struct Item {
	uint32_t start, count;
};

// what the host reads of a replicate after the first two kernels
struct Counts {
	uint32_t missing, items;
};

// Row i = blockIdx.x * 4 + wavefront.  Only D[i][j], i < j, is read as input: a missing one becomes the quiet NaN, the
// others are copied below the diagonal, the diagonal becomes +0.0; rowcnt[i] = the row's missing pairs.  (The wavefront of
// row j reads D[i][j], i < j, while that of row i may be replacing it by the quiet NaN: missing either way.)
__global__ __launch_bounds__(256) void k_complete_init(double *__restrict__ D, uint32_t n, uint32_t *__restrict__ rowcnt) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, rowcnt += rep * n;
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= n) return;
	double *row = D + (size_t)i * n;
	uint32_t count = 0;
	for (uint32_t base = 0; base < n; base += 64) {
		const uint32_t j = base + lane;
		bool miss = false;
		if (j < n) {
			if (j > i) {
				miss = !known(row[j]);
				if (miss) row[j] = qnan();
			} else if (j < i) {
				const double v = D[(size_t)j * n + i];
				row[j] = known(v) ? v : qnan();
			} else {
				row[j] = 0.0;
			}
		}
		count += (uint32_t)__popcll(__ballot(miss));
	}
	if (lane == 0) rowcnt[i] = count;
}

// One block per replicate: rowoff[i] = the missing pairs of the rows before i (rowoff[n]: all), itemoff[i] likewise of
// their items, ceil(rowcnt / P) a row; counts = {rowoff[n], itemoff[n]}.  Both fit 32 bits: n <= 65535.
__global__ __launch_bounds__(1024) void k_complete_scan(uint32_t n, const uint32_t *__restrict__ rowcnt,
														 uint32_t *__restrict__ rowoff, uint32_t *__restrict__ itemoff,
														 Counts *__restrict__ counts) {
	const size_t rep = blockIdx.y;
	rowcnt += rep * n, rowoff += rep * (n + 1), itemoff += rep * (n + 1), counts += rep;
	__shared__ uint32_t pr[1024], pi[1024];
	const uint32_t per = (n + 1023) / 1024, t = threadIdx.x;
	const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
	uint32_t sr = 0, si = 0;
	for (uint32_t i = lo; i < hi; ++i) sr += rowcnt[i], si += (rowcnt[i] + P - 1) / P;
	pr[t] = sr, pi[t] = si;
	__syncthreads();
	if (t == 0) {
		uint32_t ar = 0, ai = 0;
		for (int x = 0; x < 1024; ++x) {
			const uint32_t r = pr[x], it = pi[x];
			pr[x] = ar, pi[x] = ai;
			ar += r, ai += it;
		}
		rowoff[n] = ar, itemoff[n] = ai;
		*counts = Counts{ar, ai};
	}
	__syncthreads();
	sr = pr[t], si = pi[t];
	for (uint32_t i = lo; i < hi; ++i) {
		rowoff[i] = sr, itemoff[i] = si;
		sr += rowcnt[i], si += (rowcnt[i] + P - 1) / P;
	}
}

// Row i = blockIdx.x * 4 + wavefront: its missing pairs (the quiet NaNs k_complete_init left above the diagonal) in
// ascending j into the replicate's list from rowoff[i] on, each {i, j, round 0, 0, quartets 0, NaN}, and its items.
// The list holds exactly rowoff[n] entries and the items itemoff[n]: nothing is written past what was counted.
__global__ __launch_bounds__(256) void k_complete_list(const double *__restrict__ D, uint32_t n, const uint32_t *__restrict__ rowoff,
														 const uint32_t *__restrict__ itemoff, const uint64_t *__restrict__ bases,
														 andi_hip_fill *__restrict__ list, Item *__restrict__ items) {
	const size_t rep = blockIdx.y;
	D += rep * n * n, rowoff += rep * (n + 1), itemoff += rep * (n + 1);
	list += bases[2 * rep], items += bases[2 * rep + 1];
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= n) return;
	const double *row = D + (size_t)i * n;
	const uint32_t first = rowoff[i], cnt = rowoff[i + 1] - first;
	if (cnt == 0) return;
	uint32_t at = first;
	for (uint32_t base = (i + 1) & ~63u; base < n; base += 64) {
		const uint32_t j = base + lane;
		const bool miss = j < n && j > i && !known(row[j]);
		const unsigned long long b = __ballot(miss);
		if (miss) {
			andi_hip_fill f;
			f.i = i, f.j = j, f.round = 0, f.pad = 0, f.quartets = 0, f.value = qnan();
			list[at + (uint32_t)__popcll(b & ((1ull << lane) - 1))] = f;
		}
		at += (uint32_t)__popcll(b);
	}
	const uint32_t nit = (cnt + P - 1) / P;
	for (uint32_t t = lane; t < nit; t += 64)
		items[itemoff[i] + t] = Item{first + t * P, cnt - t * P < (uint32_t)P ? cnt - t * P : (uint32_t)P};
}

__device__ inline double wave_min_d(double v) {
	for (int m = 32; m > 0; m >>= 1) {
		const double o = __shfl_xor(v, m);
		if (o < v) v = o;
	}
	return v;
}

__device__ inline unsigned long long wave_sum_u(unsigned long long v) {
	for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
	return v;
}

// Round `round` of one item (blockIdx.x) of replicate blockIdx.y: see the head of the file.  D is only read.  A pair of
// the item that an earlier round filled is left alone; a filled pair gets its value, round and quartets in the list and
// counts in fills[(round & 1) * g + rep].  A replicate whose last round filled nothing has nothing left to fill: its
// blocks leave at once.
__global__ __launch_bounds__(QT) void k_complete_quartets(const double *__restrict__ D, uint32_t n, andi_hip_fill *__restrict__ list,
														   const Item *__restrict__ items, const uint64_t *__restrict__ bases,
														   const Counts *__restrict__ counts, uint32_t *__restrict__ fills, uint32_t g,
														   uint32_t round) {
	const size_t rep = blockIdx.y;
	if (blockIdx.x >= counts[rep].items) return;
	if (round > 1 && fills[((round - 1) & 1) * g + rep] == 0) return;
	D += rep * n * n;
	const Item it = items[bases[2 * rep + 1] + blockIdx.x];
	andi_hip_fill *L = list + bases[2 * rep] + it.start;

	__shared__ double sa[CH], sb[P][CH];
	__shared__ uint32_t sm[CH];
	__shared__ double wmin[QW][P];
	__shared__ unsigned long long wcnt[QW][P];

	const uint32_t i = L[0].i;
	const double *Di = D + (size_t)i * n, *Dj[P];
	bool act[P], any = false;
#pragma unroll
	for (int q = 0; q < P; ++q) {
		act[q] = (uint32_t)q < it.count && L[q].round == 0;
		Dj[q] = D + (size_t)(act[q] ? L[q].j : i) * n;
		any |= act[q];
	}
	if (!any) return;

	const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const double inf = __builtin_inf();
	double mn[P];
	uint32_t cnt[P];
#pragma unroll
	for (int q = 0; q < P; ++q) mn[q] = inf, cnt[q] = 0;

	for (uint32_t L0 = 0; L0 < n; L0 += CH) {
		const uint32_t len = n - L0 < (uint32_t)CH ? n - L0 : (uint32_t)CH;
		__syncthreads(); // (the chunk before this one has been used)
		for (uint32_t x = threadIdx.x; x < len; x += QT) {
			const uint32_t l = L0 + x;
			const double a = Di[l];
			const bool fa = known(a) && l != i; // (l == j_q: D[i][j_q] is missing)
			uint32_t m = 0;
#pragma unroll
			for (int q = 0; q < P; ++q) {
				const double b = act[q] ? Dj[q][l] : inf;
				const bool f = fa && known(b);
				sb[q][x] = f ? b : inf;
				m |= (uint32_t)f << q;
			}
			sa[x] = fa ? a : inf;
			sm[x] = m;
		}
		__syncthreads();
		const uint32_t kend = L0 + len; // k < l < kend
		for (uint32_t k = wave; k + 1 < kend; k += QW) {
			const double ak = Di[k];
			if (!known(ak) || k == i) continue;
			double bk[P];
			uint32_t mk = 0;
#pragma unroll
			for (int q = 0; q < P; ++q) {
				const double b = act[q] ? Dj[q][k] : inf;
				const bool f = known(b);
				bk[q] = f ? b : inf;
				mk |= (uint32_t)f << q;
			}
			if (mk == 0) continue;
			const double *Dk = D + (size_t)k * n;
			const uint32_t lo = k + 1 > L0 ? k + 1 : L0;
#pragma unroll 4
			for (uint32_t x = ((lo - L0) & ~63u) + lane; x < len; x += 64) {
				const uint32_t l = L0 + x;
				const double d = Dk[l];
				const uint32_t v = l > k && known(d) ? sm[x] & mk : 0u;
				const double al = sa[x];
#pragma unroll
				for (int q = 0; q < P; ++q) {
					const double s1 = ak + sb[q][x], s2 = al + bk[q];
					const double c = (s1 > s2 ? s1 : s2) - d;
					const bool ok = (v >> q) & 1u; // all five known: every operand above is finite, c is no NaN
					cnt[q] += ok;
					if (ok && c < mn[q]) mn[q] = c;
				}
			}
		}
	}

#pragma unroll
	for (int q = 0; q < P; ++q) {
		const double m = wave_min_d(mn[q]);
		const unsigned long long c = wave_sum_u(cnt[q]);
		if (lane == 0) wmin[wave][q] = m, wcnt[wave][q] = c;
	}
	__syncthreads();
	if (threadIdx.x < (uint32_t)P) {
		const int q = (int)threadIdx.x;
		double m = wmin[0][q];
		unsigned long long c = wcnt[0][q];
		for (int w = 1; w < QW; ++w) {
			if (wmin[w][q] < m) m = wmin[w][q];
			c += wcnt[w][q];
		}
		if ((uint32_t)q < it.count && L[q].round == 0 && c > 0 && m < inf) {
			L[q].value = m <= 0.0 ? 0.0 : m;
			L[q].quartets = c;
			L[q].round = round;
			atomicAdd(&fills[(round & 1) * g + rep], 1u);
		}
	}
}

// the fills of round `round` into D, both triangles
__global__ __launch_bounds__(256) void k_complete_apply(double *__restrict__ D, uint32_t n, const andi_hip_fill *__restrict__ list,
														  const uint64_t *__restrict__ bases, const Counts *__restrict__ counts,
														  uint32_t round) {
	const size_t rep = blockIdx.y;
	const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (x >= counts[rep].missing) return;
	const andi_hip_fill f = list[bases[2 * rep] + x];
	if (f.round != round) return;
	D += rep * n * n;
	D[(size_t)f.i * n + f.j] = f.value;
	D[(size_t)f.j * n + f.i] = f.value;
}

// the buffers of a group of g replicates of n x n whose size the host knows before it has seen a matrix (rep_groups.h:
// alloc_group); the list and the items are sized by the counts, per group (complete_group)
struct CompleteBuffers {
	double *D = nullptr;
	uint32_t *rowcnt = nullptr, *rowoff = nullptr, *itemoff = nullptr, *fills = nullptr;
	Counts *counts = nullptr;
	uint64_t *bases = nullptr; // per replicate: where its list starts, where its items start

	static size_t replicate_bytes(size_t n) {
		return n * n * sizeof(double) + (3 * n + 2) * sizeof(uint32_t) + 2 * sizeof(uint32_t) + sizeof(Counts) + 2 * sizeof(uint64_t);
	}
	hipError_t alloc(DevScope &dev, size_t n, size_t g) {
		dev.alloc(&D, g * n * n), dev.alloc(&rowcnt, g * n), dev.alloc(&rowoff, g * (n + 1)), dev.alloc(&itemoff, g * (n + 1));
		dev.alloc(&fills, 2 * g), dev.alloc(&counts, g), dev.alloc(&bases, 2 * g);
		return dev.err;
	}
};

// The completion of g host matrices (one after the other in D) in buffers for at least g: C receives the g completed
// matrices, missing[k] and left[k] replicate k's counts.  fills (the single call's; else nullptr): the first
// min(cap, missing[0]) entries of replicate 0's list.  Synchronous: one host synchronisation for the counts, one per round.
hipError_t complete_group(andi_hip_ctx *ctx, const CompleteBuffers &b, const double *D, uint32_t N, uint32_t g, unsigned max_rounds,
						  double *C, uint64_t *missing, uint64_t *left, andi_hip_fill *fills, size_t cap) {
	const size_t n = N;
	hipStream_t st = ctx->stream;
	std::vector<Counts> hc(g);
	hipError_t e = hipMemcpyAsync(b.D, D, g * n * n * sizeof(double), hipMemcpyHostToDevice, st);
	if (e != hipSuccess) return e;
	k_complete_init<<<dim3((N + 3) / 4, g), 256, 0, st>>>(b.D, N, b.rowcnt);
	k_complete_scan<<<dim3(1, g), 1024, 0, st>>>(N, b.rowcnt, b.rowoff, b.itemoff, b.counts);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if ((e = hipMemcpyAsync(hc.data(), b.counts, g * sizeof(Counts), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
	if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;

	std::vector<uint64_t> hb(2 * (size_t)g);
	uint64_t total = 0, total_items = 0;
	uint32_t most = 0, most_items = 0;
	for (uint32_t k = 0; k < g; ++k) {
		hb[2 * k] = total, hb[2 * k + 1] = total_items;
		total += hc[k].missing, total_items += hc[k].items;
		most = hc[k].missing > most ? hc[k].missing : most;
		most_items = hc[k].items > most_items ? hc[k].items : most_items;
		missing[k] = left[k] = hc[k].missing;
	}
	DevScope dev(st); // the list and the items go back when the group is done, behind the stream
	andi_hip_fill *list = nullptr;
	Item *items = nullptr;
	if (total > 0) {
		dev.alloc(&list, total), dev.alloc(&items, total_items);
		if (dev.err != hipSuccess) return dev.err;
		if ((e = hipMemcpyAsync(b.bases, hb.data(), hb.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
		k_complete_list<<<dim3((N + 3) / 4, g), 256, 0, st>>>(b.D, N, b.rowoff, b.itemoff, b.bases, list, items);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		std::vector<uint32_t> hf(g);
		for (uint32_t round = 1; n >= 4 && (max_rounds == 0 || round <= max_rounds); ++round) {
			uint32_t *f = b.fills + (round & 1) * (size_t)g;
			if ((e = hipMemsetAsync(f, 0, g * sizeof(uint32_t), st)) != hipSuccess) return e;
			k_complete_quartets<<<dim3(most_items, g), QT, 0, st>>>(b.D, N, list, items, b.bases, b.counts, b.fills, g, round);
			k_complete_apply<<<dim3((most + 255) / 256, g), 256, 0, st>>>(b.D, N, list, b.bases, b.counts, round);
			if ((e = hipGetLastError()) != hipSuccess) return e;
			if ((e = hipMemcpyAsync(hf.data(), f, g * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
			if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
			bool any = false;
			for (uint32_t k = 0; k < g; ++k) left[k] -= hf[k], any |= hf[k] != 0;
			if (!any) break;
		}
		const size_t take = cap < hc[0].missing ? cap : hc[0].missing;
		if (fills && take > 0 &&
			(e = hipMemcpyAsync(fills, list, take * sizeof(andi_hip_fill), hipMemcpyDeviceToHost, st)) != hipSuccess)
			return e;
	}
	return group_end(st, C, b.D, g * n * n);
}

} // namespace

int andi_hip_complete(andi_hip_ctx *ctx, const double *D, size_t n, unsigned max_rounds, double *C, andi_hip_fill *fills, size_t cap,
					  size_t *missing, size_t *left) {
	if (!ctx || !D || !C || !missing || !left || (!fills && cap > 0) || n < 2 || n > 65535) {
		if (ctx)
			ctx->err = "andi_hip_complete: bad arguments (ctx, D, C, missing and left must be given, fills unless cap is 0, "
					   "2 <= n <= 65535)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	CompleteBuffers b;
	uint64_t m = 0, l = 0;
	hipError_t e = b.alloc(dev, n, 1);
	if (e == hipSuccess) e = complete_group(ctx, b, D, (uint32_t)n, 1, max_rounds, C, &m, &l, fills, cap);
	if (e != hipSuccess) return fail(ctx, "andi_hip_complete", e);
	*missing = (size_t)m, *left = (size_t)l;
	return 0;
}

int andi_hip_complete_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, unsigned max_rounds, double *C,
							uint64_t *missing, uint64_t *left) {
	if (!ctx || !D || !C || !missing || !left || count == 0 || n < 2 || n > 65535) {
		if (ctx)
			ctx->err = "andi_hip_complete_batch: bad arguments (ctx, D, C, missing and left must be given, count >= 1, "
					   "2 <= n <= 65535)";
		return 1;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevScope dev(ctx->stream);
	CompleteBuffers b;
	size_t G = 0;
	std::vector<int64_t> bad(count); // (no matrix is unusable to this call: for_groups' bad words stay NOT_BAD)
	hipError_t e = alloc_group(dev, b, n, count, G);
	if (e == hipSuccess)
		e = for_groups(count, G, n * n, C, bad.data(), [&](size_t first, size_t g, double *Cg, unsigned long long *hb) {
			for (size_t k = 0; k < g; ++k) hb[k] = NOT_BAD;
			return complete_group(ctx, b, D + first * n * n, (uint32_t)n, (uint32_t)g, max_rounds, Cg, missing + first, left + first,
								  nullptr, 0);
		});
	if (e != hipSuccess) return fail(ctx, "andi_hip_complete_batch", e);
	return 0;
}
