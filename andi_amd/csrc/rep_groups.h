// rep_groups.h — the one host driver of the calls that build a tree per distance matrix, REPLICATES of one n taken a
// group at a time as their grids' second dimension: andi_hip_nj, andi_hip_nj_batch and andi_hip_bootstrap_nj and their
// method-taking forms andi_hip_tree, andi_hip_tree_batch and andi_hip_bootstrap_tree (nj.hip),
// andi_hip_linkage and andi_hip_linkage_batch (linkage.hip) -- and andi_hip_complete_batch (complete.hip), which fills
// missing distances in front of them and takes alloc_group and for_groups alone.  Private, host code only.  In the order a call uses it:
//   alloc_group  the group's size (nj_group_size, api_internal.h: GROUP_BYTES of device memory) and its buffers, in the
//                call's DevScope -- so every exit of a call, an error exit too, waits for the stream before a buffer goes
//                back; a group that does not fit is halved, down to the one matrix a single call needs too;
//   for_groups   the replicates a group at a time: the caller's body does one group, the loop offsets the records,
//                translates the device's bad words and zeroes the records of a bad replicate;
//   group_begin  a group's first launches, to the point where the host knows which of its matrices are usable;
//   group_end    its records back.
// What differs stays in the callers' files: the kernels, the step loop between group_begin and group_end, a replicate's
// buffers and their bytes, and what a single call says of an unusable matrix.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "api_internal.h"

namespace {

constexpr unsigned long long NOT_BAD = ~0ull;   // a replicate's bad word: no entry of its matrix is unusable
constexpr size_t GROUP_BYTES = (size_t)4 << 30; // device memory of a group of replicates, at most (one always fits)

// the entry a bad word names: the init kernels leave i * n + j, i < j
struct Entry {
	size_t i, j;
};
inline Entry bad_entry(unsigned long long bad, size_t n) { return Entry{(size_t)(bad / n), (size_t)(bad % n)}; }

// The buffers of a call's group in dev: as many replicates as GROUP_BYTES hold, as there are; G receives the group's
// size.  b says what a replicate costs (replicate_bytes(n): nj.hip's depends on the tree method) and how g of them are
// allocated (alloc(dev, n, g)).
template <typename Buffers>
hipError_t alloc_group(DevScope &dev, Buffers &b, size_t n, size_t count, size_t &G) {
	G = nj_group_size(KNOB_NJ_GROUP, 65535, GROUP_BYTES, b.replicate_bytes(n));
	if (G > count) G = count;
	hipError_t e = b.alloc(dev, n, G);
	while (e != hipSuccess && G > 1) { // the memory is not there: smaller groups, down to the one matrix a single call needs too
		dev.release();
		(void)hipGetLastError();
		G = (G + 1) / 2;
		e = b.alloc(dev, n, G);
	}
	return e;
}

// count replicates, G at a time (the last group may be shorter): body(first, g, records, bad_words) does the g replicates
// from `first` on -- their nrec records each go to `records`, their bad words to `bad_words` (group_begin) -- and returns
// its status.  bad[k] receives replicate k's bad word, -1 for NOT_BAD; the records of a bad replicate are zeroed, also
// where its whole group was bad and nothing was written.  Ends at the first HIP error and returns it.
template <typename Rec, typename Body>
hipError_t for_groups(size_t count, size_t G, size_t nrec, Rec *records, int64_t *bad, Body body) {
	std::vector<unsigned long long> hb(G);
	hipError_t e = hipSuccess;
	for (size_t first = 0; e == hipSuccess && first < count; first += G) {
		const size_t g = count - first < G ? count - first : G;
		Rec *R = records + first * nrec;
		e = body(first, g, R, hb.data());
		for (size_t k = 0; e == hipSuccess && k < g; ++k) {
			bad[first + k] = hb[k] == NOT_BAD ? -1 : (int64_t)hb[k];
			if (hb[k] != NOT_BAD) memset(R + k * nrec, 0, nrec * sizeof(Rec));
		}
	}
	return e;
}

// The start of a group of g matrices of n x n in dD: D (host, one matrix after the other) goes up -- D == nullptr: their
// upper triangles are in dD already, left there by kernels on the stream --, init() launches the caller's init kernel,
// which completes the matrices and leaves in dbad[k] replicate k's first unusable entry (i * n + j) or NOT_BAD; D_out, if
// given, receives the g matrices as that kernel leaves them; bad receives the g bad words.  This is the one host
// synchronisation of a group before its records; any_good says whether a matrix is usable.  When none is the caller
// returns: no step runs and nothing is written to its records.
//
// A bad replicate among good ones is NOT kept out of the step kernels: every index they use comes from the lists, the ids
// and the cached slots, never from a distance, and better() and none() (nj_cand.h) make every pick a real pair of active
// slots whatever D holds, so its steps run like any other's on NaN and inf, fault nothing, and leave records that
// for_groups zeroes.  That costs the good replicates nothing: no flag to load per block.
template <typename Init>
hipError_t group_begin(hipStream_t st, double *dD, const double *D, size_t n, size_t g, unsigned long long *dbad,
					   unsigned long long *bad, double *D_out, Init init, bool &any_good) {
	any_good = false;
	hipError_t e = D ? hipMemcpyAsync(dD, D, g * n * n * sizeof(double), hipMemcpyHostToDevice, st) : hipSuccess;
	if (e == hipSuccess) e = hipMemsetAsync(dbad, 0xff, g * sizeof *bad, st);
	if (e == hipSuccess) {
		init();
		e = hipGetLastError();
	}
	if (e == hipSuccess && D_out) e = hipMemcpyAsync(D_out, dD, g * n * n * sizeof(double), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipMemcpyAsync(bad, dbad, g * sizeof *bad, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	for (size_t k = 0; e == hipSuccess && k < g; ++k) any_good |= bad[k] == NOT_BAD;
	return e;
}

// The end of a group: its `count` records back, once the steps before them on the stream are done.  Synchronous.
template <typename Rec>
hipError_t group_end(hipStream_t st, Rec *records, const Rec *drec, size_t count) {
	const hipError_t e = hipMemcpyAsync(records, drec, count * sizeof(Rec), hipMemcpyDeviceToHost, st);
	return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

} // namespace
