// delta.hip — the tree-likeness score of every genome from all quartets on the device (andi_hip_delta_scores,
// include/andi_hip.h), bit for bit the contract there (tests/delta_model.py restates it in NumPy): for every quartet
// i < j < k < l whose six distances are known the three sums s1 = D[i][j] + D[k][l], s2 = D[i][k] + D[j][l],
// s3 = D[i][l] + D[j][k], sorted a >= b >= c, give delta = (a - b) / (a - c) (Holland, Huber, Dress and Moulton 2002) and the
// integer t = floor(delta * 2^24); each of the four genomes is credited t and one quartet.  Integers only are summed, by
// integer atomics, so the records do not depend on the schedule.
//
// The access pattern is k_complete_quartets' (complete.hip), every quartet visited once.  The host cuts the work into ITEMS:
// a row i and a range [j0, j1) of its partners, about `target` quartets each -- the pair (i, j) has C(n - 1 - j, 2) of them,
// whatever i is, so a row's C(n - 1 - i, 3) are badly uneven across rows -- and launches them heaviest first, one block each.
//
// k_delta_quartets.  The block goes over the tiles (K0, L0), L0 >= K0, of chunks of CH columns: k in the one, l in the other.
// Per tile it stages a[l] = D[i][l] of the l chunk in LDS, and per j of its range b[l] = D[j][l]; an unusable value (not
// finite, or past the matrix) is +inf there.  Every wavefront takes one k > j of the k chunk at a time -- D[i][k], D[j][k]
// are wave-uniform -- and its 64 lanes run over the chunk's l > k, reading row k of D in aligned 512-byte loads.  Only
// the upper triangle is ever used (an aligned load also fetches columns at or below k, which l > k masks), so the matrix
// goes to the device as it is.  No NaN is ever an operand of a comparison:
// every operand of a sum is finite or +inf, so a sum is finite, +inf or (overflowed) -inf; a quartet with a missing
// distance has a sum of +inf, hence a = +inf and w = a - c either +inf or NaN: not finite, not used -- the contract's own
// test does the masking.
// The credits of a used quartet, t and 1, travel as ONE 64-bit word, the count above a sum field of SB = 44 bits:
//   l   one ds_add_u64 per candidate into accL[l - L0]; the lanes of a wavefront hit distinct columns.  Between two flushes
//       (one tile) a column receives at most JMAX * CH < 2^20 adds of at most 2^24: the sum stays below 2^44, the count
//       below 2^20.  Flushed per tile, unpacked, as contiguous rows of 64-bit integer atomics, zeros left out;
//   k   a lane's register over the l loop (at most CH / 64 adds), one wave reduction per (j, k, tile), unpacked, then one
//       lane's two LDS adds into accKs / accKc[k - K0], flushed per k chunk like accL;
//   j   the sum of its k's credits, wave-uniform registers; one LDS add per wavefront, j and tile, one global pair per j, tile;
//   i   the sum of its j's credits; one global pair per wavefront and item.
// LDS: 4 arrays of CH 64-bit words and one of 32-bit words = 36 KiB a block of 4 wavefronts: 4 blocks (16 wavefronts) a CU
// of 160 KiB.
// Global atomics at 3085 leaves, about 14 000 items of at most 10 tiles: 3 * 10^8 lanes of row-shaped adds for l and k,
// 10^8 lone ones for j -- beside 3.8 * 10^12 candidates, each some 50 vector instructions.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "api_internal.h"

static_assert(sizeof(andi_hip_delta) == 16, "andi_hip_delta: sum, quartets");

namespace {

constexpr int CH = 1024;               // columns of a row staged in LDS at a time (tests/test_delta_gpu.py reads this line)
constexpr int JMAX = 1023;             // the most partners j of one item (and this one)
constexpr uint64_t MINW = 65536;       // an item's least target of quartets (and this one)
constexpr uint64_t NITEMS = 8192;      // target = max(MINW, quartets / NITEMS) (and this one)
constexpr int DT = 256, DW = DT / 64;  // k_delta_quartets: threads, wavefronts
constexpr int SB = 44;                 // the packed word: sum in bits 0 ... SB - 1, count above
constexpr unsigned long long SM = (1ull << SB) - 1;
static_assert((uint64_t)JMAX * CH < (1ull << (64 - SB)) && SB - 24 == 64 - SB, "a column's adds between two flushes fit both fields");
constexpr size_t NMAX = 16384;

// the work of one block: row i and its partners j0 <= j < j1 (j1 - j0 <= JMAX)
struct Item {
	uint32_t i, j0, j1, pad;
};

__device__ inline unsigned long long wave_sum_u(unsigned long long v) {
	for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
	return v;
}

__device__ inline double usable(double v) { return __builtin_isfinite(v) ? v : __builtin_inf(); }

__device__ inline void credit(andi_hip_delta *rec, unsigned long long sum, unsigned long long count) {
	atomicAdd((unsigned long long *)&rec->sum, sum);
	atomicAdd((unsigned long long *)&rec->quartets, count);
}

__global__ __launch_bounds__(DT) void k_delta_quartets(const double *__restrict__ D, uint32_t n, const Item *__restrict__ items,
													   andi_hip_delta *__restrict__ out) {
	__shared__ double sa[CH], sb[CH];
	__shared__ unsigned long long accL[CH], accKs[CH];
	__shared__ uint32_t accKc[CH]; // (an item's quartets with one k: at most JMAX * n < 2^24)
	__shared__ unsigned long long sj[2];

	const Item it = items[blockIdx.x];
	const uint32_t i = it.i, tid = threadIdx.x;
	const uint32_t lane = tid & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const double *Di = D + (size_t)i * n;
	const double inf = __builtin_inf();
	unsigned long long isum = 0, icnt = 0; // this wavefront's share of i's credit

	for (uint32_t x = tid; x < (uint32_t)CH; x += DT) accL[x] = 0, accKs[x] = 0, accKc[x] = 0, sa[x] = inf, sb[x] = inf;
	if (tid < 2) sj[tid] = 0;

	for (uint32_t K0 = ((it.j0 + 1) / CH) * CH; K0 + 1 < n; K0 += CH) { // k > j0, k < n - 1
		const uint32_t kend = n - 1 - K0 < (uint32_t)CH ? n - 1 : K0 + CH; // k < kend
		const uint32_t jend = it.j1 < kend - 1 ? it.j1 : kend - 1;          // j < jend: j < k
		for (uint32_t L0 = K0; L0 < n; L0 += CH) {
			const uint32_t len = n - L0 < (uint32_t)CH ? n - L0 : (uint32_t)CH;
			__syncthreads(); // (the tile before this one has been flushed)
			for (uint32_t x = tid; x < len; x += DT) sa[x] = usable(Di[L0 + x]);
			uint32_t jprev = ~0u;
			for (uint32_t j = it.j0; j < jend; ++j) {
				const double dij = Di[j];
				if (!__builtin_isfinite(dij)) continue; // (wave- and block-uniform: no quartet of this pair is used)
				const double *Dj = D + (size_t)j * n;
				__syncthreads(); // (the j before this one has been used: sb is free, sj is complete)
				if (tid == 0 && jprev != ~0u) {
					const unsigned long long s = sj[0], c = sj[1];
					sj[0] = 0, sj[1] = 0;
					if (c) credit(&out[jprev], s, c);
				}
				jprev = j;
				for (uint32_t x = tid; x < len; x += DT) sb[x] = usable(Dj[L0 + x]);
				__syncthreads();
				unsigned long long jsum = 0, jcnt = 0;
				for (uint32_t k = (j + 1 > K0 ? j + 1 : K0) + wave; k < kend && k + 1 < L0 + len; k += DW) {
					const double aik = Di[k], bjk = Dj[k];
					if (!__builtin_isfinite(aik) || !__builtin_isfinite(bjk)) continue;
					const double *Dk = D + (size_t)k * n;
					const uint32_t lo = k + 1 > L0 ? k + 1 : L0;
					unsigned long long ck = 0;
					// (the trip count is wave-uniform and the body straight-line; the load of the next trip goes out before this
					// trip's arithmetic -- the compiler moves no load across the LDS atomic; a lane past the chunk's end, or
					// at an l <= k, reads an address inside the row and takes +inf for it)
					const uint32_t last = len - 1, first = (lo - L0) & ~63u;
					double dnext = Dk[L0 + (first + lane < last ? first + lane : last)];
#pragma unroll 2
					for (uint32_t x0 = first; x0 < len; x0 += 64) {
						const uint32_t x = x0 + lane, l = L0 + x; // x < CH: x0 is a multiple of 64 below len <= CH
						const double dv = dnext;
						dnext = Dk[L0 + (x + 64 < last ? x + 64 : last)];
						const double d = l > k && x < len && __builtin_isfinite(dv) ? dv : inf;
						const double s1 = dij + d, s2 = aik + sb[x], s3 = sa[x] + bjk;
						const double hi = __builtin_fmax(s1, s2), lw = __builtin_fmin(s1, s2);
						const double a = __builtin_fmax(hi, s3), c = __builtin_fmin(lw, s3);
						const double b = __builtin_fmax(lw, __builtin_fmin(hi, s3));
						const double w = a - c, u = a - b;
						// 0 <= u <= w.  A quartet that is not used (w not finite) takes 0 / 1 and adds the word 0; w == 0 has
						// u == 0, and 0 / 1 is the contract's 0
						const bool used = __builtin_isfinite(w);
						const double delta = (used ? u : 0.0) / (used && w > 0.0 ? w : 1.0);
						const unsigned long long v = ((unsigned long long)used << SB) | (unsigned long long)(uint32_t)(delta * 16777216.0);
						ck += v;
						atomicAdd(&accL[x], v);
					}
					ck = wave_sum_u(ck);
					if (ck) {
						const unsigned long long s = ck & SM, c = ck >> SB;
						if (lane == 0) atomicAdd(&accKs[k - K0], s), atomicAdd(&accKc[k - K0], (uint32_t)c);
						jsum += s, jcnt += c;
					}
				}
				if (lane == 0 && jcnt) atomicAdd(&sj[0], jsum), atomicAdd(&sj[1], jcnt);
				isum += jsum, icnt += jcnt;
			}
			__syncthreads();
			if (tid == 0 && jprev != ~0u) {
				const unsigned long long s = sj[0], c = sj[1];
				sj[0] = 0, sj[1] = 0;
				if (c) credit(&out[jprev], s, c);
			}
			for (uint32_t x = tid; x < len; x += DT) {
				const unsigned long long v = accL[x];
				if (v) {
					accL[x] = 0;
					credit(&out[L0 + x], v & SM, v >> SB);
				}
			}
		}
		__syncthreads();
		for (uint32_t x = tid; x < kend - K0; x += DT) {
			const uint32_t c = accKc[x];
			if (c) {
				credit(&out[K0 + x], accKs[x], c);
				accKs[x] = 0, accKc[x] = 0;
			}
		}
	}
	if (lane == 0 && icnt) credit(&out[i], isum, icnt);
}

// The items of an n x n matrix, heaviest first.  The pair (i, j) has C(n - 1 - j, 2) quartets above it; a row's partners are
// taken in order until they hold `target` quartets or JMAX partners.
std::vector<Item> cut_items(uint32_t n) {
	const uint64_t m = n;
	const uint64_t total = m * (m - 1) / 2 * (m - 2) / 3 * (m - 3) / 4; // C(n, 4): every prefix product is a binomial
	const uint64_t target = total / NITEMS > MINW ? total / NITEMS : MINW;
	std::vector<Item> items;
	std::vector<uint64_t> work;
	for (uint32_t i = 0; i + 3 < n; ++i) {
		uint32_t j0 = i + 1;
		uint64_t acc = 0;
		for (uint32_t j = i + 1; j + 2 < n; ++j) {
			const uint64_t r = n - 1 - j;
			acc += r * (r - 1) / 2;
			if (acc >= target || j + 1 - j0 == (uint32_t)JMAX || j + 3 == n) {
				items.push_back(Item{i, j0, j + 1, 0});
				work.push_back(acc);
				j0 = j + 1, acc = 0;
			}
		}
	}
	std::vector<uint32_t> order(items.size());
	for (uint32_t x = 0; x < order.size(); ++x) order[x] = x;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return work[a] > work[b]; });
	std::vector<Item> sorted(items.size());
	for (size_t x = 0; x < order.size(); ++x) sorted[x] = items[order[x]];
	return sorted;
}

} // namespace

int andi_hip_delta_scores(andi_hip_ctx *ctx, const double *D, size_t n, andi_hip_delta *out) {
	if (!ctx || !D || !out || n < 2 || n > NMAX) {
		if (ctx) ctx->err = "andi_hip_delta_scores: bad arguments (ctx, D and out must be given, 2 <= n <= 16384)";
		return 1;
	}
	if (n < 4) { // no quartet
		memset(out, 0, n * sizeof *out);
		return 0;
	}
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const std::vector<Item> items = cut_items((uint32_t)n);
	DevScope dev(st);
	double *dD = nullptr;
	Item *dI = nullptr;
	andi_hip_delta *dO = nullptr;
	dev.alloc(&dD, n * n), dev.alloc(&dI, items.size()), dev.alloc(&dO, n);
	hipError_t e = dev.err;
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, n * n * sizeof(double), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(dI, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(dO, 0, n * sizeof(andi_hip_delta), st);
	if (e == hipSuccess) {
		k_delta_quartets<<<dim3((uint32_t)items.size()), DT, 0, st>>>(dD, (uint32_t)n, dI, dO);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out, dO, n * sizeof(andi_hip_delta), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st); // (items lives until here)
	if (e != hipSuccess) return fail(ctx, "andi_hip_delta_scores", e);
	return 0;
}
