// tree_paths.h — the table of path lengths of a neighbor-joining tree on the device, T[v][i] for the 2n - 3 edges v and
// the n leaves i: what andi_hip_place (place.hip) and andi_hip_root (root.hip) both work from.  Private; both translation
// units get their own copy of the kernel (it is small), but there is one source.  The leaf sets it reads are nj_sets.h's.
//   k_paths    one thread per leaf i walks up to the centre (h(v, i) for the nodes on its path), then down over all nodes
//              in descending id order, and leaves T[v][i] = below(v, i) ? h(v, i) : h(parent(v), i), the length from the
//              endpoint of edge v the contract measures leaf i from.  The thread touches column i only, so nothing crosses
//              threads; the leaf is the fastest index, so a wavefront's accesses are one run of 512 bytes.  h of a node
//              off the path is not kept: where a child needs it, it is T[v][i] + len(v) again, the same rounded sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nj_sets.h"

namespace {

// T[v * n + i] for the E = 2n - 3 edges v.  par, len: E entries; sets: the pair nodes' leaf sets (k_sets), W words each.
__global__ __launch_bounds__(64) void k_paths(const int32_t *__restrict__ par, const double *__restrict__ len,
											  const uint64_t *__restrict__ sets, uint32_t n, uint32_t W, double *T) {
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) return;
	const uint32_t E = 2 * n - 3, C = E;
	double h = 0.0;
	for (uint32_t v = i; v != C; v = (uint32_t)par[v]) { // (parents have greater ids: the walk ends at C)
		T[(size_t)v * n + i] = h;
		h = h + len[v];
	}
	const double hC = h;
	const uint32_t w = i >> 6;
	const uint64_t bit = 1ull << (i & 63);
	for (uint32_t c = E; c-- > 0;) {
		if (child_word(sets, n, W, w, (int32_t)c) & bit) continue; // on the path: written above
		const uint32_t pc = (uint32_t)par[c];                      // (an inner node, or C)
		double hp;
		if (pc == C) hp = hC;
		else {
			hp = T[(size_t)pc * n + i];
			if (!(child_word(sets, n, W, w, (int32_t)pc) & bit)) hp = hp + len[pc];
		}
		T[(size_t)c * n + i] = hp;
	}
}

} // namespace
