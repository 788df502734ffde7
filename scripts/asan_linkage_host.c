/* A stand-alone run of the linkage host functions (andi_amd/csrc/host_model.c: andi_hip_linkage_cut,
 * andi_hip_cluster_medoids, andi_hip_cluster_stability, andi_hip_format_newick_linkage) under the host sanitizers: no GPU,
 * no Python.  From the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_linkage_host.c andi_amd/csrc/host_model.c -lm -lpthread -o asan_linkage_host && ./asan_linkage_host
 * For every n = 2 ... 1200 it takes a caterpillar (the deepest tree) and a balanced tree, every buffer exactly as large as
 * the call may use: cuts them below, inside and above their heights and checks the labels against the records' sizes,
 * takes the medoids of those clusters in a matrix with NaN entries, counts the stability of the clustering against
 * itself, a shifted numbering and the singletons, formats the tree into a buffer of exactly the size the call asked for
 * and again with short caps, and tries the refusals.  Prints one line and returns 0 when everything held. */
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

/* leaf 0 and 1 at height 1, that node and leaf 2 at height 2, ... */
static void caterpillar(andi_hip_link *Z, size_t n) {
	for (size_t s = 0; s + 1 < n; s++)
		Z[s] = (andi_hip_link){s ? (int32_t)(s + 1) : 0, s ? (int32_t)(n + s - 1) : 1, (uint32_t)(s + 2), 0, (double)(s + 1)};
}

/* join the two oldest nodes of a queue until one is left; heights ascend */
static void balanced(andi_hip_link *Z, size_t n) {
	int32_t *queue = malloc(2 * n * sizeof *queue);
	uint32_t *size = malloc(2 * n * sizeof *size);
	size_t head = 0, tail = 0, s = 0;
	for (size_t i = 0; i < n; i++) size[i] = 1, queue[tail++] = (int32_t)i;
	while (tail - head > 1) {
		const int32_t a = queue[head], b = queue[head + 1];
		size[n + s] = size[a] + size[b];
		Z[s] = (andi_hip_link){a, b, size[n + s], 0, 0.25 * (double)(s + 1)};
		head += 2;
		queue[tail++] = (int32_t)(n + s++);
	}
	free(queue), free(size);
}

int main(void) {
	size_t trees = 0, bytes = 0;
	for (size_t n = 2; n <= 1200; n++) {
		andi_hip_link *Z = malloc((n - 1) * sizeof *Z);
		uint32_t *labels = malloc(n * sizeof *labels), *medoid = malloc(n * sizeof *medoid), *stab = malloc(n * sizeof *stab);
		uint32_t *reps = malloc(3 * n * sizeof *reps), *members = malloc(n * sizeof *members);
		double *D = malloc(n * n * sizeof *D);
		char **names = malloc(n * sizeof *names);
		for (size_t i = 0; i < n; i++) {
			names[i] = malloc(24);
			snprintf(names[i], 24, i % 7 == 3 ? "it's %zu" : "taxon_number_%zu", i);
			for (size_t j = 0; j < n; j++) D[i * n + j] = (i * 31 + j * 17) % 11 == 0 ? NAN : (double)((i * 7 + j * 13) % 23);
		}
		for (int shape = 0; shape < 2; shape++) {
			(shape ? balanced : caterpillar)(Z, n);
			const double top = Z[n - 2].height, ts[5] = {Z[0].height * 0.5, Z[(n - 2) / 2].height, top, INFINITY, NAN};
			for (int k = 0; k < 5; k++) {
				size_t nc = 0;
				CHECK(andi_hip_linkage_cut(Z, n, ts[k], labels, &nc) == 0);
				CHECK(nc >= 1 && nc <= n && labels[0] == 0);
				if (k == 0 || k == 4) CHECK(nc == n);
				if (k == 2 || k == 3) CHECK(nc == 1);
				memset(members, 0, n * sizeof *members);
				for (size_t i = 0; i < n; i++) {
					CHECK(labels[i] < nc);
					members[labels[i]]++;
				}
				CHECK(andi_hip_cluster_medoids(D, n, labels, nc, medoid) == 0);
				for (size_t c = 0; c < nc; c++) CHECK(medoid[c] < n && labels[medoid[c]] == c);
				/* three replicates: the clustering itself, the same with another numbering, the singletons */
				for (size_t i = 0; i < n; i++) reps[i] = labels[i], reps[n + i] = (uint32_t)((labels[i] + 1) % nc), reps[2 * n + i] = (uint32_t)i;
				CHECK(andi_hip_cluster_stability(labels, nc, reps, n, 3, stab) == 0);
				for (size_t c = 0; c < nc; c++) CHECK(stab[c] == (members[c] == 1 ? 3u : 2u));
			}
			for (int truncate = 0; truncate < 2; truncate++) {
				const size_t need = andi_hip_format_newick_linkage(Z, n, (const char *const *)names, truncate, NULL, 0);
				CHECK(need > 0);
				char *text = malloc(need + 1);
				CHECK(andi_hip_format_newick_linkage(Z, n, (const char *const *)names, truncate, text, need + 1) == need);
				CHECK(strlen(text) == need && text[need - 1] == '\n' && text[need - 2] == ';');
				const size_t caps[3] = {1, need / 2, need};
				for (int c = 0; c < 3; c++) {
					if (!caps[c]) continue;
					char *part = malloc(caps[c]);
					CHECK(andi_hip_format_newick_linkage(Z, n, (const char *const *)names, truncate, part, caps[c]) == need);
					CHECK(strlen(part) == caps[c] - 1 && !memcmp(part, text, caps[c] - 1));
					free(part);
				}
				trees++, bytes += need;
				free(text);
			}
		}
		/* the refusals */
		char small[8] = "xxxxxxx";
		size_t nc = 0;
		const double h = Z[n - 2].height;
		Z[n - 2].height = INFINITY;
		CHECK(andi_hip_format_newick_linkage(Z, n, (const char *const *)names, 0, small, sizeof small) == 0 && !small[0]);
		Z[n - 2].height = h;
		Z[n - 2].a = (int32_t)(2 * n - 2); /* no node of an earlier record */
		CHECK(andi_hip_format_newick_linkage(Z, n, (const char *const *)names, 0, small, sizeof small) == 0);
		CHECK(andi_hip_linkage_cut(Z, n, 1.0, labels, &nc) == 1);
		Z[n - 2].a = Z[n - 2].b; /* a child twice */
		CHECK(andi_hip_linkage_cut(Z, n, 1.0, labels, &nc) == 1);
		for (size_t i = 0; i < n; i++) labels[i] = 0;
		labels[n - 1] = 2; /* cluster 1 has no member */
		CHECK(andi_hip_cluster_medoids(D, n, labels, 3, medoid) == 1);
		CHECK(andi_hip_cluster_stability(labels, 3, reps, n, 3, stab) == 1);
		CHECK(andi_hip_cluster_medoids(D, n, labels, 2, medoid) == 1); /* a label beyond the clusters */
		for (size_t i = 0; i < n; i++) free(names[i]);
		free(names), free(Z), free(labels), free(medoid), free(stab), free(reps), free(members), free(D);
	}
	printf("linkage host functions: %zu trees (n = 2 ... 1200, caterpillar and balanced), %zu bytes of Newick, clean\n", trees, bytes);
	return 0;
}
