/* A stand-alone run of andi_hip_relength (andi_amd/csrc/host_model.c) under the host sanitizers: no GPU, no Python.  From
 * the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_fit_host.c andi_amd/csrc/host_model.c -lm -lpthread -o asan_fit_host && ./asan_fit_host
 * For every n = 3 ... 400 it takes a caterpillar (the deepest tree) and a balanced tree and 2n - 3 lengths in a buffer of
 * exactly that size, relengths into records of exactly n - 2 and in place, and checks that every child carries
 * len[child] and that nothing else changed.  NULL pointers, n < 3 and malformed records must give 1 and write nothing.
 * Prints one line and returns 0 when everything held. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "andi_hip.h"

#define CHECK(c)                                                                                   \
	do {                                                                                           \
		if (!(c)) {                                                                                \
			fprintf(stderr, "%s:%d: n = %zu: %s\n", __FILE__, __LINE__, n, #c);                      \
			exit(1);                                                                               \
		}                                                                                          \
	} while (0)

static void caterpillar(andi_hip_nj_join *J, size_t n) {
	int32_t top = 0;
	for (size_t s = 0; s + 3 < n; s++) {
		J[s] = (andi_hip_nj_join){s ? (int32_t)(s + 1) : 0, s ? top : 1, -1, 0, 0.125 * (double)(s + 1), -0.5, 0.0};
		top = (int32_t)(n + s);
	}
	if (n == 3) J[0] = (andi_hip_nj_join){0, 1, 2, 0, 1.0, 2.0, 3.0};
	else J[n - 3] = (andi_hip_nj_join){(int32_t)(n - 2), (int32_t)(n - 1), top, 0, 1.0, 0.0, 3e-9};
}

static void balanced(andi_hip_nj_join *J, size_t n) {
	int32_t *active = malloc(2 * n * sizeof *active);
	size_t lo = 0, hi = n, s = 0;
	for (size_t i = 0; i < n; i++) active[i] = (int32_t)i;
	while (hi - lo > 3) {
		J[s] = (andi_hip_nj_join){active[lo], active[lo + 1], -1, 0, 0.25, 1e-7 * (double)s, 0.0};
		lo += 2, active[hi++] = (int32_t)(n + s++);
	}
	J[n - 3] = (andi_hip_nj_join){active[lo], active[lo + 1], active[lo + 2], 0, 0.5, 0.25, 0.125};
	free(active);
}

int main(void) {
	size_t trees = 0;
	for (size_t n = 3; n <= 400; n += n < 40 ? 1 : 37) {
		const size_t nrec = n - 2, E = 2 * n - 3;
		for (int shape = 0; shape < 2; shape++) {
			andi_hip_nj_join *J = malloc(nrec * sizeof *J), *out = malloc(nrec * sizeof *out), *same = malloc(nrec * sizeof *same);
			double *len = malloc(E * sizeof *len);
			if (shape) balanced(J, n);
			else caterpillar(J, n);
			for (size_t v = 0; v < E; v++) len[v] = v % 7 == 3 ? -0.001 * (double)v : 1.0 + (double)v;
			memset(out, 0xab, nrec * sizeof *out);
			CHECK(andi_hip_relength(J, n, len, out) == 0);
			for (size_t s = 0; s < nrec; s++) {
				CHECK(out[s].a == J[s].a && out[s].b == J[s].b && out[s].c == J[s].c && out[s].pad == J[s].pad);
				CHECK(out[s].la == len[J[s].a] && out[s].lb == len[J[s].b]);
				if (s + 1 == nrec) CHECK(out[s].lc == len[J[s].c]);
				else CHECK(memcmp(&out[s].lc, &J[s].lc, sizeof(double)) == 0);
			}
			memcpy(same, J, nrec * sizeof *J);
			CHECK(andi_hip_relength(same, n, len, same) == 0 && memcmp(same, out, nrec * sizeof *out) == 0);
			/* the refusals: nothing is written */
			memset(out, 0xab, nrec * sizeof *out);
			memcpy(same, out, nrec * sizeof *out);
			CHECK(andi_hip_relength(NULL, n, len, out) == 1 && andi_hip_relength(J, n, NULL, out) == 1);
			CHECK(andi_hip_relength(J, n, len, NULL) == 1 && andi_hip_relength(J, 2, len, out) == 1);
			andi_hip_nj_join keep = J[nrec - 1];
			J[nrec - 1].a = J[nrec - 1].b; /* a node that is a child twice */
			CHECK(andi_hip_relength(J, n, len, out) == 1);
			J[nrec - 1] = keep, J[nrec - 1].c = (int32_t)(n + nrec); /* a child that no record made */
			CHECK(andi_hip_relength(J, n, len, out) == 1);
			J[nrec - 1] = keep, J[0].a = -1;
			CHECK(andi_hip_relength(J, n, len, out) == 1);
			CHECK(memcmp(same, out, nrec * sizeof *out) == 0);
			free(J), free(out), free(same), free(len);
			trees++;
		}
	}
	printf("asan_fit_host: %zu trees relengthed, every refusal held\n", trees);
	return 0;
}
