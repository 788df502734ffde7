// nj_cand.h — a candidate pair and its order, shared by the kernels that pick the least pair of a step (nj.hip: the least
// Q of neighbor-joining; linkage.hip: the least distance of agglomerative clustering).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// a candidate pair: its value (Q, or a distance), the two node ids (ia < ib) and their slots
struct Cand {
	double q;
	int32_t ia, ib, sa, sb;
};

// the contracts' order: the least value (-0.0 == +0.0), then the smaller id_x, then the smaller id_y.  A NaN (only from
// overflow) orders after every number, so the pick is always a real pair.
__device__ inline bool better(const Cand &a, const Cand &b) {
	const bool na = __builtin_isnan(a.q), nb = __builtin_isnan(b.q);
	if (na != nb) return nb;
	if (!na && a.q != b.q) return a.q < b.q;
	return a.ia < b.ia || (a.ia == b.ia && a.ib < b.ib);
}

__device__ inline Cand none() { return Cand{__builtin_nan(""), INT32_MAX, INT32_MAX, 0, 0}; }

__device__ inline Cand shfl_xor(const Cand &c, int m) {
	return Cand{__shfl_xor(c.q, m), __shfl_xor(c.ia, m), __shfl_xor(c.ib, m), __shfl_xor(c.sa, m), __shfl_xor(c.sb, m)};
}

__device__ inline Cand wave_min(Cand c) {
	for (int m = 32; m > 0; m >>= 1) {
		const Cand o = shfl_xor(c, m);
		if (better(o, c)) c = o;
	}
	return c;
}

// the block's least candidate, returned to every thread (blockDim.x / 64 waves, at most 16)
__device__ Cand block_min(Cand c) {
	__shared__ Cand w[16];
	c = wave_min(c);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
	if (lane == 0) w[wave] = c;
	__syncthreads();
	c = w[0];
	for (int k = 1; k < waves; ++k)
		if (better(w[k], c)) c = w[k];
	__syncthreads();
	return c;
}

} // namespace
