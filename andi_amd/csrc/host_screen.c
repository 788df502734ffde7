/* host_screen.c — the selection rule of the k-mer sketch screen (andi_hip_screen_select, include/andi_hip.h): which
 * references the queries keep, from the shared-hash counts of every (query, reference) pair.  Plain C, no GPU. */
#include <stdlib.h>
#include <string.h>

#include "andi_hip.h"

/* Query q takes references in the order (shared descending, reference index ascending), the first `keep` of them whose
 * count is at least max(1, min_shared).  The best remaining one is picked by a pass over the row, `keep` times at most:
 * O(keep * nr) per query, no allocation. */
int andi_hip_screen_select(const uint32_t *shared, size_t nq, size_t nr, size_t keep, uint32_t min_shared, uint8_t *kept,
						   uint32_t *taken) {
	if (!shared || !kept || nq == 0 || nr == 0) return 1;
	const uint32_t floor_ = min_shared > 1 ? min_shared : 1;
	memset(kept, 0, nr);
	for (size_t q = 0; q < nq; q++) {
		const uint32_t *row = shared + q * nr;
		/* the last reference taken: count `lc` at index `li`; the next one is the best (count, index) that orders behind it */
		uint32_t lc = 0, n = 0;
		size_t li = 0;
		int first = 1;
		if (keep >= nr) { /* every reference that passes the floor */
			for (size_t r = 0; r < nr; r++)
				if (row[r] >= floor_) kept[r] = 1, n++;
			if (taken) taken[q] = n;
			continue;
		}
		while (n < keep) {
			uint32_t bc = 0;
			size_t bi = nr;
			for (size_t r = 0; r < nr; r++) {
				const uint32_t c = row[r];
				if (c < floor_) continue;
				if (!first && (c > lc || (c == lc && r <= li))) continue; /* taken already */
				if (bi == nr || c > bc) bc = c, bi = r;                    /* (ascending r: on a tie the earlier one stays) */
			}
			if (bi == nr) break;
			kept[bi] = 1, lc = bc, li = bi, first = 0;
			if (++n == UINT32_MAX) break;
		}
		if (taken) taken[q] = n;
	}
	return 0;
}
