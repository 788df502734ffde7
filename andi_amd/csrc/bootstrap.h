// bootstrap.h — launch interface of the pairwise bootstrap kernels (bootstrap.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "andi_hip.h"

// replicates first ... first + replicates - 1 of the stream, as models: B_dev holds `replicates` matrices
hipError_t andi_launch_bootstrap(const andi_hip_model *M_dev, andi_hip_model *B_dev, uint32_t n, uint32_t first,
								 uint32_t replicates, uint64_t seed, hipStream_t st);
// S_dev[t * 16 + c]: the summed counts of pair t of the packed strict upper triangle, n (n - 1) / 2 x 64 bytes
hipError_t andi_launch_pair_sums(const andi_hip_model *M_dev, uint32_t *S_dev, uint32_t n, hipStream_t st);
// D_dev[k][i * n + j], i < j, k < group: the portable estimate of replicate first + k's draw for that pair
hipError_t andi_launch_bootstrap_dist(const uint32_t *S_dev, double *D_dev, uint32_t n, int model, uint32_t first,
									  uint32_t group, uint64_t seed, hipStream_t st);
