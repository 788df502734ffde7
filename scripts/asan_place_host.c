/* A stand-alone run of the placement host functions (andi_amd/csrc/host_model.c: andi_hip_parse_newick,
 * andi_hip_format_jplace, andi_hip_distances_rect) under the host sanitizers: no GPU, no Python.  From the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_place_host.c andi_amd/csrc/host_model.c -lm -lpthread -o asan_place_host && ./asan_place_host
 * For every n = 3 ... 400 it takes a caterpillar (the deepest tree) and a balanced tree with names that need quotes, every
 * buffer exactly as large as the call may use: formats the tree, parses it back into exactly n - 2 records, formats those
 * and parses again (a fixed point), parses every prefix of the text and the text with every single byte replaced by each
 * of ( ) , : ; ' -- all must be refused or accepted without a stray access --, formats the jplace text into a buffer of
 * exactly the size the call asked for and again with short caps, and fills a table of distances.  Prints one line and
 * returns 0 when everything held. */
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

static char *exact_newick(const andi_hip_nj_join *J, size_t n, const char *const *names, size_t *len) {
	const size_t need = andi_hip_format_newick(J, n, names, 0, NULL, 0);
	char *t = malloc(need + 1);
	if (andi_hip_format_newick(J, n, names, 0, t, need + 1) != need || strlen(t) != need) exit(2);
	*len = need;
	return t;
}

int main(void) {
	size_t trees = 0, mutants = 0;
	for (size_t n = 3; n <= 400; n += n < 40 ? 1 : 37) {
		char **names = malloc(n * sizeof *names);
		for (size_t i = 0; i < n; i++) {
			names[i] = malloc(24);
			snprintf(names[i], 24, i % 5 == 0 ? "it's %zu" : i % 7 == 0 ? "(b,%zu);" : "leaf_%zu", i);
		}
		const char *const *cn = (const char *const *)names;
		for (int shape = 0; shape < 2; shape++) {
			andi_hip_nj_join *J = malloc((n - 2) * sizeof *J), *J1 = malloc((n - 2) * sizeof *J1), *J2 = malloc((n - 2) * sizeof *J2);
			(shape ? balanced : caterpillar)(J, n);
			size_t len, len1, len2;
			char *t = exact_newick(J, n, cn, &len), err[8];
			CHECK(andi_hip_parse_newick(t, cn, n, 0, J1, err, sizeof err) == 0);
			char *t1 = exact_newick(J1, n, cn, &len1);
			CHECK(andi_hip_parse_newick(t1, cn, n, 0, J2, NULL, 0) == 0);
			char *t2 = exact_newick(J2, n, cn, &len2);
			CHECK(len1 == len2 && !strcmp(t1, t2));
			if (n <= 40) {
				/* every prefix, in a buffer that ends with it */
				for (size_t k = 0; k < len; k++) {
					char *p = malloc(k + 1);
					memcpy(p, t, k), p[k] = '\0';
					CHECK(andi_hip_parse_newick(p, cn, n, 0, J2, err, sizeof err) == 1 || k + 1 >= len);
					free(p);
				}
				/* every byte replaced by a character the grammar gives a meaning to */
				for (size_t k = 0; k < len; k++)
					for (const char *c = "(),:;' x"; *c; c++) {
						char *p = malloc(len + 1);
						memcpy(p, t, len + 1), p[k] = *c;
						(void)andi_hip_parse_newick(p, cn, n, 0, J2, err, sizeof err);
						(void)andi_hip_parse_newick(p, cn, n, 1, J2, NULL, 0);
						free(p), mutants++;
					}
			}
			/* the jplace text: exact room, then short caps */
			const size_t nq = 3;
			const andi_hip_placement P[3] = {{0, (uint32_t)n, 0.0, 0.25, 1e-9}, {-1, 1, 0.0, 0.0, INFINITY}, {(int32_t)(2 * n - 4), 2, 0.5, 0.0, 3.0}};
			const char *const qn[3] = {"q \"one\" \\", "none", "tab\there and a long name"};
			for (int trunc = 0; trunc < 2; trunc++) {
				const size_t need = andi_hip_format_jplace(J, n, cn, trunc, P, nq, qn, ANDI_PLACE_FM, NULL, 0);
				CHECK(need > 0);
				char *out = malloc(need + 1);
				CHECK(andi_hip_format_jplace(J, n, cn, trunc, P, nq, qn, ANDI_PLACE_FM, out, need + 1) == need && strlen(out) == need);
				CHECK(!strstr(out, "none") && strstr(out, "q \\\"one\\\""));
				for (size_t cap = 1; cap < need; cap += need / 13 + 1) {
					char *cut = malloc(cap);
					CHECK(andi_hip_format_jplace(J, n, cn, trunc, P, nq, qn, ANDI_PLACE_OLS, cut, cap) > 0 && strlen(cut) == cap - 1);
					free(cut);
				}
				free(out);
			}
			J[0].a = (int32_t)(2 * n);
			CHECK(andi_hip_format_jplace(J, n, cn, 0, P, nq, qn, ANDI_PLACE_FM, NULL, 0) == 0);
			free(t), free(t1), free(t2), free(J), free(J1), free(J2), trees++;
		}
		/* a table of distances, exactly nq x nr doubles */
		const size_t nq = 7;
		andi_hip_model *MRQ = calloc(n * nq, sizeof *MRQ), *MQR = calloc(n * nq, sizeof *MQR);
		for (size_t k = 0; k < n * nq; k++) {
			for (int c = 0; c < 16; c++) MRQ[k].counts[c] = MQR[k].counts[c] = (uint32_t)(c % 5 == 0 ? 1000 + k % 17 : k % 3);
			MRQ[k].seq_len = MQR[k].seq_len = 5000;
		}
		double *D = malloc(n * nq * sizeof *D);
		CHECK(andi_hip_distances_rect(MRQ, MQR, n, nq, ANDI_M_JC, D) == 0);
		for (size_t k = 0; k < n * nq; k++) CHECK(D[k] >= 0.0);
		free(MRQ), free(MQR), free(D);
		for (size_t i = 0; i < n; i++) free(names[i]);
		free(names);
	}
	printf("placement host functions: %zu trees, %zu mutated texts, clean\n", trees, mutants);
	return 0;
}
