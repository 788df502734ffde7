/*
 * host_estimate.c — the host entry point of the portable estimator (andi_estimate.h): the function the device computes
 * in andi_hip_bootstrap_nj, for the host to compare against.  Compiled with -ffp-contract=off (Makefile): every
 * operation of the header is rounded on its own, here as on the device.
 */
#include "andi_estimate.h"

int andi_hip_estimate_portable(const andi_hip_model *m, size_t count, int model, double *out) {
	if (model < ANDI_M_RAW || model > ANDI_M_ANI || (count && (!m || !out))) return 1;
	for (size_t k = 0; k < count; k++) out[k] = andi_estimate_portable(&m[k], model);
	return 0;
}
