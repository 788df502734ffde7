/*
 * andi_estimate.h — the portable estimator: andi_log and the five distance estimators of host_model.c over one
 * andi_hip_model, from ONE text for the host (C99, gcc) and the device (hipcc).  Every operation is an IEEE double
 * + - * /, a comparison, an integer operation or a move of bits, each rounded on its own: no libm, no ocml, no FMA.  So
 * a distance computed on the device equals the one andi_hip_estimate_portable computes on the host, bit for bit.
 * include/andi_hip.h states andi_log completely; tests/estimate_model.py restates all of this in NumPy.
 *
 * No contraction: on the device every function carries `#pragma clang fp contract(off)`; the host object that includes
 * this header is compiled with -ffp-contract=off (andi_amd/csrc/Makefile).
 */
#ifndef ANDI_ESTIMATE_H
#define ANDI_ESTIMATE_H
#include <stdint.h>

#include "andi_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ANDI_HD __host__ __device__
#else
#define ANDI_HD
#endif
#ifdef __clang__
#define ANDI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ANDI_NO_CONTRACT
#endif

ANDI_HD static inline uint64_t andi_bits_of(double x) {
	uint64_t b;
	__builtin_memcpy(&b, &x, 8);
	return b;
}

ANDI_HD static inline double andi_from_bits(uint64_t b) {
	double x;
	__builtin_memcpy(&x, &b, 8);
	return x;
}

#define ANDI_BITS_NAN 0x7ff8000000000000ull
#define ANDI_BITS_INF 0x7ff0000000000000ull

/* The natural logarithm (the contract: include/andi_hip.h).  x = 2^k * m with m in (sqrt(2)/2, sqrt(2)], f = m - 1,
 * s = f / (2 + f), log(m) = 2 atanh(s) = 2s + 2s z (1/3 + z/5 + ... + z^12/27), z = s^2, put together in fdlibm's
 * arrangement around hfsq = f^2/2 and a two-part ln 2. */
ANDI_HD static inline double andi_log(double x) {
	ANDI_NO_CONTRACT
	if (!(x > 0.0)) return andi_from_bits(x == 0.0 ? ANDI_BITS_INF | 0x8000000000000000ull : ANDI_BITS_NAN);
	uint64_t b = andi_bits_of(x);
	if (b == ANDI_BITS_INF) return x;
	int k = 0;
	if ((b >> 52) == 0) { /* subnormal: times 2^54 (exact) */
		x = x * 18014398509481984.0;
		k = -54;
		b = andi_bits_of(x);
	}
	k += (int)(b >> 52) - 1023;
	double m = andi_from_bits((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull); /* [1, 2) */
	if (m > 1.4142135623730951) {
		m = m * 0.5;
		k = k + 1;
	}
	const double f = m - 1.0; /* exact */
	const double s = f / (2.0 + f);
	const double z = s * s;
	double p = 0.0;
	for (int i = 27; i >= 3; i -= 2) p = p * z + 1.0 / (double)i;
	const double hfsq = (0.5 * f) * f;
	const double R = (2.0 * z) * p;
	const double t = s * (hfsq + R);
	if (k == 0) return f - (hfsq - t);
	const double dk = (double)k;
	return dk * 6.93147180369123816490e-01 - ((hfsq - (t + dk * 1.90821492927058770002e-10)) - f);
}

/* cell index = 4*from + to, A C G T = 0 1 2 3 (host_model.c) */
ANDI_HD static inline uint64_t andi_est_total(const andi_hip_model *m) {
	uint64_t t = 0;
	for (int k = 0; k < 16; k++) t += m->counts[k];
	return t;
}

ANDI_HD static inline uint64_t andi_est_off_diagonal(const andi_hip_model *m) {
	uint64_t t = 0;
	for (int f = 0; f < 4; f++)
		for (int g = 0; g < 4; g++)
			if (f != g) t += m->counts[4 * f + g];
	return t;
}

ANDI_HD static inline double andi_est_raw(const andi_hip_model *m) {
	ANDI_NO_CONTRACT
	const uint64_t nucl = andi_est_total(m), snps = andi_est_off_diagonal(m);
	if (nucl <= 3) return andi_from_bits(ANDI_BITS_NAN);
	return (double)snps / (double)nucl;
}

ANDI_HD static inline double andi_est_jc(const andi_hip_model *m) {
	ANDI_NO_CONTRACT
	double d = andi_est_raw(m);
	d = -0.75 * andi_log(1.0 - (4.0 / 3.0) * d);
	return d <= 0.0 ? 0.0 : d;
}

ANDI_HD static inline double andi_est_kimura(const andi_hip_model *m) {
	ANDI_NO_CONTRACT
	const uint64_t nucl = andi_est_total(m);
	const uint64_t ts = (uint64_t)m->counts[4 * 0 + 2] + m->counts[4 * 2 + 0] + m->counts[4 * 1 + 3] + m->counts[4 * 3 + 1];
	const uint64_t tv = andi_est_off_diagonal(m) - ts;
	const double P = (double)ts / (double)nucl;
	const double Q = (double)tv / (double)nucl;
	const double w = 1.0 - 2.0 * P - Q;
	const double d = -0.25 * andi_log((1.0 - 2.0 * Q) * w * w);
	return d <= 0.0 ? 0.0 : d;
}

/* (the 4x4 determinant in host_model.c's term order) */
ANDI_HD static inline double andi_est_logdet(const andi_hip_model *m) {
	ANDI_NO_CONTRACT
	const double nucl = (double)andi_est_total(m);
	double P[16];
	for (int k = 0; k < 16; k++) P[k] = (double)m->counts[k] / nucl;

	double lg = 0.0;
	for (int f = 0; f < 4; f++) {
		uint64_t s = 0;
		for (int g = 0; g < 4; g++) s += m->counts[4 * f + g];
		const double term = andi_log((double)s / nucl);
		lg = f ? lg + term : term;
	}
	for (int g = 0; g < 4; g++) {
		uint64_t s = 0;
		for (int f = 0; f < 4; f++) s += m->counts[4 * f + g];
		lg = lg + andi_log((double)s / nucl);
	}

#define ANDI_P(f, g) P[4 * (f) + (g)]
	const double det = ANDI_P(0, 0) * ANDI_P(1, 1) * (ANDI_P(2, 2) * ANDI_P(3, 3) - ANDI_P(3, 2) * ANDI_P(2, 3)) -
					   ANDI_P(0, 0) * ANDI_P(1, 2) * (ANDI_P(2, 1) * ANDI_P(3, 3) - ANDI_P(3, 1) * ANDI_P(2, 3)) +
					   ANDI_P(0, 0) * ANDI_P(1, 3) * (ANDI_P(2, 1) * ANDI_P(3, 2) - ANDI_P(3, 1) * ANDI_P(2, 2)) -

					   ANDI_P(0, 1) * ANDI_P(1, 0) * (ANDI_P(2, 2) * ANDI_P(3, 3) - ANDI_P(3, 2) * ANDI_P(2, 3)) +
					   ANDI_P(0, 1) * ANDI_P(1, 2) * (ANDI_P(2, 0) * ANDI_P(3, 3) - ANDI_P(3, 0) * ANDI_P(2, 3)) -
					   ANDI_P(0, 1) * ANDI_P(1, 3) * (ANDI_P(2, 0) * ANDI_P(3, 2) - ANDI_P(3, 0) * ANDI_P(2, 2)) +

					   ANDI_P(0, 2) * ANDI_P(1, 0) * (ANDI_P(2, 1) * ANDI_P(3, 3) - ANDI_P(3, 1) * ANDI_P(2, 3)) -
					   ANDI_P(0, 2) * ANDI_P(1, 1) * (ANDI_P(2, 0) * ANDI_P(3, 3) - ANDI_P(3, 0) * ANDI_P(2, 3)) +
					   ANDI_P(0, 2) * ANDI_P(1, 3) * (ANDI_P(2, 0) * ANDI_P(3, 1) - ANDI_P(3, 0) * ANDI_P(2, 1)) -

					   ANDI_P(0, 3) * ANDI_P(1, 0) * (ANDI_P(2, 1) * ANDI_P(3, 2) - ANDI_P(3, 1) * ANDI_P(2, 2)) +
					   ANDI_P(0, 3) * ANDI_P(1, 1) * (ANDI_P(2, 0) * ANDI_P(3, 2) - ANDI_P(3, 0) * ANDI_P(2, 2)) -
					   ANDI_P(0, 3) * ANDI_P(1, 2) * (ANDI_P(2, 0) * ANDI_P(3, 1) - ANDI_P(3, 0) * ANDI_P(2, 1));
#undef ANDI_P
	const double d = -0.25 * (andi_log(det) - 0.5 * lg);
	return d <= 0.0 ? 0.0 : d;
}

ANDI_HD static inline double andi_est_ani(const andi_hip_model *m) {
	ANDI_NO_CONTRACT
	return (1.0 - andi_est_raw(m)) * 100;
}

/* andi_hip_estimate's dispatch (JC for anything else) */
ANDI_HD static inline double andi_estimate_portable(const andi_hip_model *m, int model) {
	switch (model) {
		case ANDI_M_RAW: return andi_est_raw(m);
		case ANDI_M_KIMURA: return andi_est_kimura(m);
		case ANDI_M_LOGDET: return andi_est_logdet(m);
		case ANDI_M_ANI: return andi_est_ani(m);
		default: return andi_est_jc(m);
	}
}

#endif
