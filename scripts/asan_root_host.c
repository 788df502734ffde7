/* A stand-alone run of the rooted Newick formatter (andi_amd/csrc/host_model.c: andi_hip_format_newick_rooted) under the
 * host sanitizers: no GPU, no Python.  From the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_root_host.c andi_amd/csrc/host_model.c -lm -lpthread -o asan_root_host && ./asan_root_host
 * For every n = 3 ... 400 it takes a caterpillar (the deepest tree) and a balanced tree with names that need quotes and
 * roots it on EVERY edge, with labels (some missing) and without, into a buffer of exactly the size the call asked for,
 * and on some edges again with every short cap up to 40 bytes: the text must end in ";\n" and hold every label behind
 * exactly one ")" -- the root edge's behind two, one per half.  Edges out of range, a distal that is not finite and
 * malformed records must give 0 and an empty string.  Prints one line and returns 0 when
 * everything held. */
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

static size_t count(const char *t, const char *what) {
	size_t k = 0;
	for (const char *p = strstr(t, what); p; p = strstr(p + 1, what)) k++;
	return k;
}

int main(void) {
	size_t texts = 0;
	for (size_t n = 3; n <= 400; n += n < 40 ? 1 : 37) {
		char **names = malloc(n * sizeof *names), **labels = malloc((n - 3 ? n - 3 : 1) * sizeof *labels);
		for (size_t i = 0; i < n; i++) {
			names[i] = malloc(24);
			snprintf(names[i], 24, i % 5 == 0 ? "it's %zu" : i % 7 == 0 ? "(b,%zu);" : "leaf_%zu", i);
		}
		for (size_t s = 0; s + 3 < n; s++) {
			labels[s] = s % 4 == 3 ? NULL : malloc(24);
			if (labels[s]) snprintf(labels[s], 24, "<%zu>", s);
		}
		const char *const *cn = (const char *const *)names, *const *cl = (const char *const *)labels;
		for (int shape = 0; shape < 2; shape++) {
			andi_hip_nj_join *J = malloc((n - 2) * sizeof *J);
			(shape ? balanced : caterpillar)(J, n);
			for (size_t e = 0; e < 2 * n - 3; e++)
				for (int with = 0; with < 2; with++) {
					const double distal = e % 3 == 0 ? 0.0 : 0.0625;
					const size_t need = andi_hip_format_newick_rooted(J, n, cn, (int)(e & 1), (int32_t)e, distal, with ? cl : NULL, NULL, 0);
					CHECK(need > 0);
					char *t = malloc(need + 1);
					CHECK(andi_hip_format_newick_rooted(J, n, cn, (int)(e & 1), (int32_t)e, distal, with ? cl : NULL, t, need + 1) == need);
					CHECK(strlen(t) == need && need > 2 && !strcmp(t + need - 2, ";\n"));
					texts++;
					if (with)
						for (size_t s = 0; s + 3 < n; s++) {
							if (!labels[s]) continue;
							char key[32];
							snprintf(key, sizeof key, ")%s:", labels[s]);
							/* (the root edge's label stands on both halves: its child end is node n + s, the other half a group) */
							CHECK(count(t, key) == (e == n + s ? 2u : 1u));
						}
					else CHECK(!strchr(t, '<'));
					if (e % 17 == 0)
						for (size_t cap = 1; cap <= 40 && cap <= need; cap++) {
							char *small = malloc(cap);
							CHECK(andi_hip_format_newick_rooted(J, n, cn, (int)(e & 1), (int32_t)e, distal, with ? cl : NULL, small, cap) == need);
							CHECK(strlen(small) == cap - 1 && !strncmp(small, t, cap - 1));
							free(small);
						}
					free(t);
				}
			/* refusals */
			char buf[64];
			const int32_t E = (int32_t)(2 * n - 3);
			strcpy(buf, "x");
			CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, -1, 0.0, NULL, buf, sizeof buf) == 0 && !buf[0]);
			strcpy(buf, "x");
			CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, E, 0.0, NULL, buf, sizeof buf) == 0 && !buf[0]);
			CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, 0, NAN, NULL, buf, sizeof buf) == 0);
			CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, 0, INFINITY, NULL, buf, sizeof buf) == 0);
			CHECK(andi_hip_format_newick_rooted(NULL, n, cn, 0, 0, 0.0, NULL, buf, sizeof buf) == 0);
			CHECK(andi_hip_format_newick_rooted(J, 2, cn, 0, 0, 0.0, NULL, buf, sizeof buf) == 0);
			if (n > 4) {
				andi_hip_nj_join keep = J[1];
				J[1].a = J[0].a; /* a node that is a child twice */
				CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, 0, 0.0, NULL, buf, sizeof buf) == 0 && !buf[0]);
				J[1] = keep, J[1].b = (int32_t)(n + 1); /* its own node */
				CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, 0, 0.0, NULL, buf, sizeof buf) == 0);
				J[1] = keep, J[1].a = -1;
				CHECK(andi_hip_format_newick_rooted(J, n, cn, 0, 0, 0.0, NULL, buf, sizeof buf) == 0);
				J[1] = keep;
			}
			free(J);
		}
		for (size_t i = 0; i < n; i++) free(names[i]);
		for (size_t s = 0; s + 3 < n; s++) free(labels[s]);
		free(names), free(labels);
	}
	printf("asan_root_host: %zu rooted texts, all as expected\n", texts);
	return 0;
}
