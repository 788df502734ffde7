/* A stand-alone run of andi_hip_format_newick_transfer (andi_amd/csrc/host_model.c) under the host sanitizers: no GPU, no
 * Python.  From the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_newick_transfer.c andi_amd/csrc/host_model.c -lm -lpthread -o asan_newick_transfer && ./asan_newick_transfer
 * For every n = 2 ... 3000 it formats a caterpillar (the deepest tree) and a balanced tree with the labels 1, 0 and values
 * in between into a buffer of exactly the size the call asked for, checks the return value, the NUL, the number of labels
 * and that the two other formatters agree on the unlabelled text's length, asks again with every short cap class (0, 1,
 * half), and tries the refusals.  Prints one line and returns 0 when everything held. */
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

/* join leaf 0 and 1, then that node with leaf 2, ... */
static void caterpillar(andi_hip_nj_join *J, size_t n) {
	if (n == 2) {
		J[0] = (andi_hip_nj_join){0, 1, -1, 0, 0.5, 0.5, 0.0};
		return;
	}
	for (size_t s = 0; s + 3 < n; s++)
		J[s] = (andi_hip_nj_join){s ? (int32_t)(n + s - 1) : 0, (int32_t)(s + 1), -1, 0, 0.5, 0.25, 0.0};
	J[n - 3] = (andi_hip_nj_join){(int32_t)(n - 2), (int32_t)(n - 1), n > 3 ? (int32_t)(n + n - 4) : 0, 0, 0.125, 0.125, 0.125};
	if (n == 3) J[0].a = 0, J[0].b = 1, J[0].c = 2;
}

/* join the two oldest nodes of a queue until three are left */
static void balanced(andi_hip_nj_join *J, size_t n) {
	if (n < 4) {
		caterpillar(J, n);
		return;
	}
	int32_t *queue = malloc((2 * n) * sizeof *queue);
	size_t head = 0, tail = 0, s = 0;
	for (size_t i = 0; i < n; i++) queue[tail++] = (int32_t)i;
	while (tail - head > 3) {
		J[s] = (andi_hip_nj_join){queue[head], queue[head + 1], -1, 0, 0.01, 0.02, 0.0};
		head += 2;
		queue[tail++] = (int32_t)(n + s++);
	}
	J[s] = (andi_hip_nj_join){queue[head], queue[head + 1], queue[head + 2], 0, 0.1, 0.2, 0.3};
	free(queue);
}

/* the sizes of the leaf sets below the pair records' nodes, as depth = min(size, n - size) */
static void depths(const andi_hip_nj_join *J, size_t n, uint32_t *depth) {
	size_t *size = calloc(2 * n, sizeof *size);
	for (size_t i = 0; i < n; i++) size[i] = 1;
	for (size_t s = 0; s + 3 < n; s++) {
		size[n + s] = size[J[s].a] + size[J[s].b];
		depth[s] = (uint32_t)(size[n + s] < n - size[n + s] ? size[n + s] : n - size[n + s]);
	}
	free(size);
}

static size_t count_labels(const char *text) {
	size_t labels = 0;
	for (const char *p = text; *p; p++) labels += p[0] == ')' && p[1] != ':' && p[1] != ';';
	return labels;
}

int main(void) {
	size_t trees = 0, bytes = 0;
	for (size_t n = 2; n <= 3000; n++) {
		const size_t nrec = n == 2 ? 1 : n - 2, nsup = n > 3 ? n - 3 : 0, used = 100;
		/* exactly as many elements as the call may read: the sanitizer sees any step past them */
		andi_hip_nj_join *J = malloc(nrec * sizeof *J);
		uint32_t *depth = malloc(nsup ? nsup * sizeof *depth : 1);
		uint64_t *transfer = malloc(nsup ? nsup * sizeof *transfer : 1);
		char **names = malloc(n * sizeof *names);
		for (size_t i = 0; i < n; i++) {
			names[i] = malloc(24);
			snprintf(names[i], 24, i % 7 == 3 ? "it's %zu" : "taxon_number_%zu", i);
		}
		for (int shape = 0; shape < 2; shape++) {
			(shape ? balanced : caterpillar)(J, n);
			depths(J, n, depth);
			for (size_t s = 0; s < nsup; s++) {
				const uint64_t most = (uint64_t)used * (depth[s] - 1);
				transfer[s] = s % 3 == 0 ? 0 : s % 3 == 1 ? most : (uint64_t)(s * 2654435761u) % (most + 1);
			}
			for (int truncate = 0; truncate < 2; truncate++) {
				const size_t need = andi_hip_format_newick_transfer(J, depth, transfer, used, n, (const char *const *)names, truncate, NULL, 0);
				CHECK(need > 0);
				char *text = malloc(need + 1);
				CHECK(andi_hip_format_newick_transfer(J, depth, transfer, used, n, (const char *const *)names, truncate, text, need + 1) == need);
				CHECK(strlen(text) == need && text[need - 1] == '\n' && text[need - 2] == ';');
				CHECK(count_labels(text) == nsup);
				const size_t caps[3] = {1, need / 2, need};
				for (int c = 0; c < 3; c++) {
					if (!caps[c]) continue;
					char *part = malloc(caps[c]);
					CHECK(andi_hip_format_newick_transfer(J, depth, transfer, used, n, (const char *const *)names, truncate, part, caps[c]) == need);
					CHECK(strlen(part) == caps[c] - 1 && !memcmp(part, text, caps[c] - 1));
					free(part);
				}
				/* the two older formatters walk the same way: support == NULL is the plain text */
				const size_t plain = andi_hip_format_newick(J, n, (const char *const *)names, truncate, NULL, 0);
				CHECK(plain == andi_hip_format_newick_support(J, NULL, n, (const char *const *)names, truncate, NULL, 0));
				CHECK(plain + nsup <= need);
				trees++, bytes += need;
				free(text);
			}
		}
		/* the refusals */
		char small[8] = "xxxxxxx";
		CHECK(andi_hip_format_newick_transfer(J, depth, transfer, 0, n, (const char *const *)names, 0, small, sizeof small) == 0 && !small[0]);
		CHECK(andi_hip_format_newick_transfer(J, NULL, transfer, used, n, (const char *const *)names, 0, small, sizeof small) == 0);
		CHECK(andi_hip_format_newick_transfer(J, depth, NULL, used, n, (const char *const *)names, 0, small, sizeof small) == 0);
		if (nsup) {
			depth[nsup - 1] = 1;
			CHECK(andi_hip_format_newick_transfer(J, depth, transfer, used, n, (const char *const *)names, 0, small, sizeof small) == 0);
			depth[nsup - 1] = 2;
			J[0].a = (int32_t)(n + nsup); /* no node of an earlier record */
			CHECK(andi_hip_format_newick_transfer(J, depth, transfer, used, n, (const char *const *)names, 0, small, sizeof small) == 0);
		}
		for (size_t i = 0; i < n; i++) free(names[i]);
		free(names), free(J), free(depth), free(transfer);
	}
	printf("andi_hip_format_newick_transfer: %zu trees (n = 2 ... 3000, caterpillar and balanced), %zu bytes, clean\n", trees, bytes);
	return 0;
}
