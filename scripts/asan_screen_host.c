/* A stand-alone run of the screen's host function (andi_amd/csrc/host_screen.c: andi_hip_screen_select) under the host
 * sanitizers: no GPU, no Python.  From the repository root:
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       scripts/asan_screen_host.c andi_amd/csrc/host_screen.c -o asan_screen_host && ./asan_screen_host
 * Count matrices of every shape from 1 x 1 to 9 x 41 -- random counts, rows of ties, all-zero rows, counts at the top of
 * uint32 -- in buffers of exactly nq * nr, nr and nq elements (so that a stray access is the sanitizer's), with every keep
 * from 1 to nr + 2 and SIZE_MAX and several floors, each result held against a selection by sorting; taken == NULL; the
 * refusals.  Prints one line and returns 0 when everything held. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "andi_hip.h"

#define CHECK(c)                                                                                   \
	do {                                                                                           \
		if (!(c)) {                                                                                \
			fprintf(stderr, "%s:%d: %zu x %zu, keep %zu, floor %u: %s\n", __FILE__, __LINE__, nq, nr, keep, (unsigned)min_shared, #c); \
			exit(1);                                                                               \
		}                                                                                          \
	} while (0)

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t draw(void) { /* xorshift64* */
	state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
	return (uint32_t)((state * 0x2545f4914f6cdd1dull) >> 32);
}

static const uint32_t *row_for_sort;
static int by_count_then_index(const void *a, const void *b) {
	const size_t x = *(const size_t *)a, y = *(const size_t *)b;
	if (row_for_sort[x] != row_for_sort[y]) return row_for_sort[x] > row_for_sort[y] ? -1 : 1;
	return x < y ? -1 : x > y;
}

int main(void) {
	size_t calls = 0;
	for (size_t nq = 1; nq <= 9; nq += 2)
		for (size_t nr = 1; nr <= 41; nr += nr < 6 ? 1 : 7) {
			for (int kind = 0; kind < 4; kind++) {
				uint32_t *shared = malloc(nq * nr * sizeof *shared), *taken = malloc(nq * sizeof *taken), *want_taken = malloc(nq * sizeof *taken);
				uint8_t *kept = malloc(nr), *want = malloc(nr);
				size_t *order = malloc(nr * sizeof *order);
				for (size_t i = 0; i < nq * nr; i++)
					shared[i] = kind == 0 ? draw() % 50 : kind == 1 ? 3 + draw() % 2 : kind == 2 ? (i / nr % 2 ? 0 : draw() % 4) : 0xFFFFFFFFu - draw() % 3;
				const size_t keeps[] = {1, 2, nr > 1 ? nr - 1 : 1, nr, nr + 1, nr + 2, (size_t)-1};
				const uint32_t floors[] = {0, 1, 2, 4, 49, 0xFFFFFFFEu, 0xFFFFFFFFu};
				for (size_t a = 0; a < sizeof keeps / sizeof *keeps; a++)
					for (size_t b = 0; b < sizeof floors / sizeof *floors; b++) {
						const size_t keep = keeps[a];
						const uint32_t min_shared = floors[b], floor_ = min_shared > 1 ? min_shared : 1;
						memset(want, 0, nr);
						for (size_t q = 0; q < nq; q++) {
							for (size_t r = 0; r < nr; r++) order[r] = r;
							row_for_sort = shared + q * nr;
							qsort(order, nr, sizeof *order, by_count_then_index);
							uint32_t n = 0;
							for (size_t j = 0; j < nr && n < keep; j++)
								if (row_for_sort[order[j]] >= floor_) want[order[j]] = 1, n++;
							want_taken[q] = n;
						}
						memset(kept, 0xAA, nr), memset(taken, 0xAA, nq * sizeof *taken);
						CHECK(andi_hip_screen_select(shared, nq, nr, keep, min_shared, kept, taken) == 0);
						CHECK(!memcmp(kept, want, nr) && !memcmp(taken, want_taken, nq * sizeof *taken));
						memset(kept, 0xAA, nr);
						CHECK(andi_hip_screen_select(shared, nq, nr, keep, min_shared, kept, NULL) == 0 && !memcmp(kept, want, nr));
						calls += 2;
					}
				const size_t keep = 1;
				const uint32_t min_shared = 1;
				CHECK(andi_hip_screen_select(NULL, nq, nr, keep, min_shared, kept, taken) == 1);
				CHECK(andi_hip_screen_select(shared, nq, nr, keep, min_shared, NULL, taken) == 1);
				CHECK(andi_hip_screen_select(shared, 0, nr, keep, min_shared, kept, taken) == 1);
				CHECK(andi_hip_screen_select(shared, nq, 0, keep, min_shared, kept, taken) == 1);
				free(shared), free(taken), free(want_taken), free(kept), free(want), free(order);
			}
		}
	printf("screen host function: %zu selections, clean\n", calls);
	return 0;
}
