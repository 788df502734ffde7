/*
 * andi_hip.h — C-ABI of libandihip.so, the MI355X (gfx950) engine behind
 * andi's anchor-distance hot path.
 *
 * The reference has no FFI for this path; its seam is internal:
 * calculate_distances() (src/process.c:230) allocates the n*n `struct model`
 * matrix and calls distMatrix()/distMatrixLM() (src/dist_hack.h:34), which per
 * subject run seq_subject_init (src/sequence.c:210), esa_init
 * (src/esa.c:254) and, per query, dist_anchor (src/process.c:141).  Every
 * entry point below names the reference function it replaces.  All
 * signatures are plain C: pointers, sizes, PODs.  Functions return 0 on
 * success; on failure they return non-zero and write a message to
 * errbuf (when given).  Nothing here falls back to a CPU implementation of a
 * device step: without a usable HIP device the device entry points fail.
 *
 * ABI 5 also gained, without changing anything that was there, the query-versus-
 * reference mode: andi_hip_dist_rect, andi_hip_queries_view and
 * andi_hip_format_distances_rect (additions only; the version stays 5); and the tree the matrix feeds:
 * andi_hip_distances, andi_hip_nj and andi_hip_format_newick (additions only as well); and bootstrap support on that
 * tree: andi_hip_nj_batch, andi_hip_nj_support and andi_hip_format_newick_support (additions only); and the majority-rule
 * consensus tree of the bootstrap: andi_hip_nj_splits, andi_hip_consensus and andi_hip_format_newick_consensus (additions only);
 * and transfer bootstrap support: andi_hip_nj_transfer and andi_hip_format_newick_transfer (additions only), and the genomes
 * behind it: andi_hip_nj_transfer_taxa (an addition only); and bootstrap
 * trees without matrices: andi_hip_estimate_portable, andi_hip_bootstrap_range and andi_hip_bootstrap_nj (additions only); and linkage
 * clustering: andi_hip_linkage, andi_hip_linkage_batch, andi_hip_linkage_cut, andi_hip_cluster_medoids,
 * andi_hip_cluster_stability and andi_hip_format_newick_linkage (additions only); and placement of queries on a tree:
 * andi_hip_place, andi_hip_distances_rect, andi_hip_parse_newick and andi_hip_format_jplace (additions only); and the k-mer
 * sketch screen in front of the query-versus-reference mode: andi_hip_sketch and the calls around it,
 * andi_hip_sketch_shared, andi_hip_screen_select and andi_hip_screen (additions only); and the tree builder by method
 * (neighbor-joining or BIONJ): andi_hip_tree, andi_hip_tree_batch and andi_hip_bootstrap_tree (additions only); and missing
 * distances estimated from quartets, in front of those trees: andi_hip_complete and andi_hip_complete_batch (additions only);
 * and the tree-likeness score of every genome from all quartets: andi_hip_delta_scores (an addition only); and the root of
 * a tree without an outgroup: andi_hip_root and andi_hip_format_newick_rooted (additions only); and a tree's branch
 * lengths refit to its matrix by least squares: andi_hip_fit and andi_hip_relength (additions only); and a tree refined
 * by balanced nearest-neighbor interchanges, with its balanced lengths: andi_hip_refine, and by balanced subtree pruning
 * and regrafting: andi_hip_refine_spr (additions only).
 */
#ifndef ANDI_HIP_H
#define ANDI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANDI_HIP_ABI_VERSION 5

/* enum in src/global.h:50 */
enum { ANDI_M_RAW = 0, ANDI_M_JC = 1, ANDI_M_KIMURA = 2, ANDI_M_LOGDET = 3, ANDI_M_ANI = 4 };

/* seq_t (src/sequence.h:18-25) without the name: NUL-terminated, over
 * {A,C,G,T,!} as produced by normalize() (src/sequence.c:260-282).  Any other
 * byte is refused by the scan (andi_hip_scan_rows / andi_hip_dist_matrix return an
 * error): the device index codes a symbol in 2 or 4 bits. */
typedef struct {
	const char *seq;
	size_t len;
} andi_hip_seq;

/* struct model (src/model.h:52-57): counts[4*from+to], then the query length.
 * 68 bytes, no padding. */
typedef struct {
	uint32_t counts[16];
	uint32_t seq_len;
} andi_hip_model;

/* lcp_inter_t (src/esa.h:25-34) */
typedef struct {
	int32_t l, i, j, m;
} andi_hip_interval;

/* The globals the reference reads deep inside the path, made explicit:
 * ANCHOR_P_VALUE (src/andi.c:48), MODEL (src/andi.c:50; selects the equal-run
 * attribution of src/model.c:247), THREADS (src/andi.c:46), F_LOW_MEMORY
 * (src/global.h:63), the progress line of src/dist_hack.h:40-43,74-87. */
typedef struct {
	double p_value;
	int model;
	int device;        /* first HIP device ordinal */
	int host_threads;  /* <=0: all cores (suffix sorting pool, shared by the devices) */
	int low_memory;    /* bound the number of resident subject indexes */
	uint32_t segment;  /* query nucleotides per scan work item; 0 = default */
	void (*progress)(size_t done, size_t total, void *ud); /* serialised; called from the devices' driver threads */
	void *ud;
	int sa_on_host;    /* 0: suffix arrays are built on the device (sa_device.hip); 1: by the host pool
	                    * (andi_hip_suffix_array), as the reference does with libdivsufsort (src/esa.c:303) */
	/* The N x N loop is tiled over the GPUs of the node by rows (the parallel loop of
	 * src/dist_hack.h:46-47): num_gpus devices device, device + 1, ...; 0 or 1 = one device; < 0 = all
	 * visible devices from `device` on.  Every device owns a contiguous block of subject rows; the row
	 * blocks are gathered on the first device with RCCL (send/recv over xGMI) and copied to M once. */
	int num_gpus;
	const int *devices; /* optional: exactly these num_gpus ordinals (an ordinal may repeat: several contexts
	                     * on one device, rows then go to M directly) */
} andi_hip_opts;

void andi_hip_default_opts(andi_hip_opts *o);
int andi_hip_abi_version(void);

/* Device memory: the library carves its buffers out of large chunks (2 GiB, ANDI_ARENA_MB).  Up to ANDI_ARENA_KEEP MiB of
 * them (default 8192; 0: none, as up to ABI 3) stay with the process when the last context on a device is destroyed, so
 * that the next call of the seam does not pay the driver for them again (on some hosts 0.3 s per call for a 29-genome
 * job); what a larger job took beyond that goes back with its last context.  This gives every chunk nobody holds a block of
 * back to the driver -- all devices the library has used; waits for each --, and returns the bytes released; the idle streams
 * and pinned upload buffers destroyed contexts left behind (kept for the next call as well: a stream costs this runtime 3 ms to
 * create, nine per call of the seam) go with them.  A process that never used the library makes no HIP call here. */
size_t andi_hip_trim(void);

/* Host helper: the 4-bit symbols of a byte string as the engine keeps its texts (A C G T ! ; # NUL = 0 ... 7; byte j of out
 * = symbol 2j | symbol 2j+1 << 4, the NUL behind an odd length included): (len + 1) / 2 bytes.  Returns 1 if a byte lies
 * outside that alphabet (src/sequence.c:260-282 never produces one).  The seam packs its queries with it, once for all
 * devices; no GPU is touched. */
int andi_hip_pack_symbols(const unsigned char *src, size_t len, unsigned char *out);

/* ------------------------------------------------------------------ */
/* The seam: replaces distMatrix / distMatrixLM (src/dist_hack.h:34-96) */
/* as called from calculate_distances (src/process.c:247-251).         */
/* M is caller-owned, n*n row-major, M[i*n+j] = subject i vs query j,  */
/* diagonal = {counts[0]=9, seq_len=9} (src/dist_hack.h:61-64).        */
/* ------------------------------------------------------------------ */
int andi_hip_dist_matrix(andi_hip_model *M, const andi_hip_seq *seqs, size_t n,
						 const andi_hip_opts *opts, char *errbuf, size_t errlen);
/* The query-versus-reference mode: the two cross blocks of andi_hip_dist_matrix over refs ++ queries, bit for bit, and
 * nothing else -- MRQ (nr*nq, row r = reference r as subject: MRQ[r*nq+q] = M[r][nr+q]) and MQR (nq*nr, row q = query q
 * as subject: MQR[q*nr+r] = M[nr+q][r]).  andi's distance of a pair needs both directions (model_average of the two,
 * src/io.c:246-322).  The union is staged once as the query pool; reference rows scan a view of its last nq sequences,
 * query rows a view of its first nr; no entry is a diagonal placeholder (a sequence in both sets is scanned against
 * itself).  Same opts as the square call: model, p_value, low_memory, sa_on_host, num_gpus/devices (the reference rows
 * and the query rows each tiled over the devices with andi_hip_row_block; rows are copied to MRQ/MQR directly, so
 * andi_hip_last_gather reports "direct"), progress with total = 2*nr*nq.  Bad arguments (NULL pointers, nr or nq 0,
 * an empty or oversized sequence) fail through errbuf before any HIP call.  Growing a matrix: old x old is kept, the new
 * cross blocks come from this call with refs = old, queries = new, and new x new from andi_hip_dist_matrix. */
int andi_hip_dist_rect(andi_hip_model *MRQ, andi_hip_model *MQR,
					   const andi_hip_seq *refs, size_t nr, const andi_hip_seq *queries, size_t nq,
					   const andi_hip_opts *opts, char *errbuf, size_t errlen);
/* how the calling thread's last call collected its rows: "rccl", "direct (...)" (diagnostic; per thread).
 * A call that spans several devices initialises RCCL communicators, and RCCL reads the bootstrap interface from the
 * process environment only: unless NCCL_SOCKET_IFNAME is set, the library sets it to "lo" around ncclCommInitAll and
 * takes it back (its own calls serialised by a lock).  A caller with other threads that touch the environment sets
 * NCCL_SOCKET_IFNAME itself beforehand: the library then never writes the environment. */
const char *andi_hip_last_gather(void);
/* The seam's tiling of the parallel subject loop (src/dist_hack.h:46-47) over `parts` devices: part k owns the
 * contiguous rows [*first, *last) of `total`; sizes differ by at most one, the longer blocks come first.  A caller that
 * runs one process per GPU instead (bench.py --gpus N, andi_amd/shard.py) partitions with the same rule.  No GPU is touched. */
void andi_hip_row_block(size_t total, size_t parts, size_t k, size_t *first, size_t *last);

/* ------------------------------------------------------------------ */
/* Host pieces of the path (stay on the host, same libm)               */
/* ------------------------------------------------------------------ */
/* seq_subject_init (src/sequence.c:210-219): RS = revcomp(S) '#' S '\0'
 * (malloc'ed, free with andi_hip_free), RSlen = 2*len+1, gc, threshold. */
int andi_hip_subject_prepare(const char *seq, size_t len, double p_value,
							 char **RS, size_t *RSlen, double *gc, size_t *threshold);
void andi_hip_free(void *p);
/* min_anchor_length / shustring_cum_prob (src/sequence.c:296-304,353-373) */
size_t andi_hip_min_anchor_length(double p, double g, size_t l);
double andi_hip_shustring_cum_prob(size_t x, double p, size_t l);
/* divsufsort() as called at src/esa.c:303: T[0..n) unsigned bytes, T[n]
 * must be readable; SA[0..n).  Re-entrant. */
int andi_hip_suffix_array(const unsigned char *T, int32_t *SA, int32_t n);
/* which sorter that is: libdivsufsort where the host has it (loaded at first use with dlopen -- the reference's own,
 * configure.ac:33-38; ANDI_HIP_NO_DIVSUFSORT in the environment keeps it away), else the built-in linear-time SA-IS */
const char *andi_hip_suffix_sorter(void);
/* model_average / model_coverage / estimate_* (src/model.c:39-210) */
andi_hip_model andi_hip_model_average(const andi_hip_model *a, const andi_hip_model *b);
double andi_hip_model_coverage(const andi_hip_model *m);
double andi_hip_estimate(const andi_hip_model *m, int model);
/* print_distances (src/io.c:246-322) into a caller buffer: PHYLIP text of the
 * n*n matrix.  names[i] as seq_t.name.  Returns the number of bytes needed
 * (excluding NUL); writes at most cap.  *warn_flags gets bit0 = a NaN was
 * reported, bit1 = coverage < 0.2 reported; warning lines go to warnbuf. */
size_t andi_hip_format_distances(const andi_hip_model *M, const char *const *names, size_t n,
								 int model, int extra_verbose, int truncate_names, int warnings,
								 char *out, size_t cap, char *warnbuf, size_t warncap,
								 int *warn_flags);
/* The table of the query-versus-reference mode (andi_hip_dist_rect's MRQ, MQR) into a caller buffer: "nq nr\n"; ten
 * spaces and " %s" per reference name (truncated to ten characters under truncate_names); then per query its name as
 * print_distances prints it and nr distances, estimate(model_average(MRQ[r][q], MQR[q][r])) -- MQR[q][r] alone under
 * extra_verbose.  Every cell is the string print_distances prints for that pair of refs ++ queries; the %1.4f / %1.4e
 * switch is decided over this whole table.  NaN and low-coverage warnings as print_distances words them, once per
 * (query, reference) pair, into warnbuf; return value and *warn_flags as andi_hip_format_distances. */
size_t andi_hip_format_distances_rect(const andi_hip_model *MRQ, const andi_hip_model *MQR,
									  const char *const *ref_names, size_t nr, const char *const *query_names, size_t nq,
									  int model, int extra_verbose, int truncate_names, int warnings,
									  char *out, size_t cap, char *warnbuf, size_t warncap, int *warn_flags);

/* The distance matrix as doubles: D[i*n+j] = D[j*n+i] = andi_hip_estimate(model_average(M[i][j], M[j][i]), model) for
 * i != j -- the unrounded value andi_hip_format_distances prints for that cell (without extra_verbose; it is the same
 * computation) -- and D[i*n+i] = +0.0.  Row-parallel like the formatter.  Returns 1 on NULL pointers or when memory runs
 * out.  No GPU is touched. */
int andi_hip_distances(const andi_hip_model *M, size_t n, int model, double *D);

/* One record of a neighbor-joining tree (andi_hip_nj): node ids a, b (and c for the final record, else -1) with the
 * lengths of their branches.  40 bytes. */
typedef struct {
	int32_t a, b, c, pad;
	double la, lb, lc;
} andi_hip_nj_join;
/* The Newick text of andi_hip_nj's records J (n leaves: n - 2 records, one for n = 2), one line ending in ";\n".  A leaf is
 * names[i] (cut to ten characters under truncate_names, as the matrix prints it), in single quotes with every ' doubled
 * if it holds a blank, a tab or one of ( ) [ ] ' : ; ,; a pair record is "(" T(a) ":" L(la) "," T(b) ":" L(lb) ")"; the
 * final record "(" T(x):L(lx) "," T(y):L(ly) "," T(z):L(lz) ");" (two children for n = 2); L is %.8g.  Not recursive:
 * any depth works.  Returns the bytes needed without the NUL, writes at most cap and NUL-terminates (as
 * andi_hip_format_distances); records whose ids are not those andi_hip_nj gives (a child that is no leaf and no earlier
 * record's node) give 0 and an empty string. */
size_t andi_hip_format_newick(const andi_hip_nj_join *J, size_t n, const char *const *names, int truncate_names,
							  char *out, size_t cap);
/* The same text with support values as internal node labels: the decimal support[s] directly behind the ")" that closes
 * pair record s, 0 <= s < n - 3 -- "(A:0.1,B:0.2)87:0.05".  The number is the COUNT andi_hip_nj_support gives, not a
 * percentage; the final record gets no label.  support == NULL gives exactly the bytes of the function above (both are
 * one walk).  Return value, cap and the rule for malformed records as above. */
size_t andi_hip_format_newick_support(const andi_hip_nj_join *J, const uint32_t *support, size_t n,
									  const char *const *names, int truncate_names, char *out, size_t cap);
/* The same walk with the transfer bootstrap expectation (TBE) as internal node labels, from andi_hip_nj_transfer's depth
 * and transfer and the number `used` of replicates that were summed: behind the ")" of pair record s, %.6g of
 * 1.0 - (double)transfer[s] / ((double)used * (double)(depth[s] - 1)), each operation rounded; the final record gets no
 * label.  Return value, cap and malformed records as andi_hip_format_newick.  used == 0, a depth[s] < 2 (s < n - 3) and a
 * NULL depth or transfer give 0 and an empty string, whatever n. */
size_t andi_hip_format_newick_transfer(const andi_hip_nj_join *J, const uint32_t *depth, const uint64_t *transfer,
									   size_t used, size_t n, const char *const *names, int truncate_names,
									   char *out, size_t cap);

/* One node of a consensus tree (andi_hip_consensus): the index of its parent in the same array (-1 for the root), the
 * number of replicates that have the branch above it, and that branch's length.  16 bytes. */
typedef struct {
	int32_t parent;
	uint32_t support;
	double length;
} andi_hip_cons_node;
/* The majority-rule consensus tree (PHYLIP consense's "MR") of the replicate trees reps (count * (n - 2) records; one
 * record per replicate for n = 2), from what andi_hip_nj_splits said about them: ids (count * (n - 3)), nsplits, freq,
 * sets; skip as there.  No GPU is touched.  With used = the number of replicates with !skip || !skip[k]:
 *  - split id enters iff 2 * freq[id] > used (a strict majority; a split in exactly half of the replicates stays out).
 *    Such splits are pairwise compatible, and as every canonical side lacks leaf 0 they are a laminar family: any two
 *    are nested or disjoint;
 *  - nodes (room for 2n - 2 entries; 3 for n = 2): nodes[0 .. n) the leaves, nodes[n .. n + m) the majority splits in
 *    ascending id order, m returned in *ninner, nodes[n + m] the root {-1, used, +0.0};
 *  - an inner node's parent is the smallest majority split that properly contains its set, else the root; a leaf's
 *    parent is the smallest majority split that contains the leaf, else the root; leaf 0's parent is the root;
 *  - an inner node's support is freq[id], a leaf's is used;
 *  - an inner node's length: the sequential sum, from +0.0, in ascending k (and ascending s within k), of the length of
 *    the branch above node n + s -- the la, lb or lc of the record that has n + s as a child -- over every used replicate
 *    k and pair record s with ids[k*(n-3) + s] == id, divided by (double)freq[id]; a leaf's length: the same sum of its
 *    own branch over all used replicates, divided by (double)used;
 *  - n = 2 and n = 3: the leaves under the root, m = 0 (ids, freq and sets are not read).
 * Returns 1, with nodes and *ninner unspecified, on a NULL reps, nodes or ninner (ids, freq, sets for n >= 4 and nsplits
 * > 0), n outside 2 ... 65535, count == 0, used == 0, and on inconsistent arguments: a child id of a used replicate that
 * is out of range or a child twice, an id >= nsplits that is not 0xFFFFFFFF, a used replicate with an id 0xFFFFFFFF, a
 * majority split that does not occur freq[id] times among the ids, whose set is empty or holds leaf 0 or a leaf >= n, or
 * majority sets that are not laminar.  Work: O(count * n) plus the number of leaves of every majority split (at most
 * n^2 / 2, a caterpillar).  Not recursive. */
int andi_hip_consensus(const andi_hip_nj_join *reps, size_t n, size_t count, const uint8_t *skip, const uint32_t *ids,
					   size_t nsplits, const uint32_t *freq, const uint64_t *sets, andi_hip_cons_node *nodes, size_t *ninner);
/* The Newick text of andi_hip_consensus's nodes (n leaves, ninner inner nodes, the root at n + ninner), one line ending
 * in ";\n".  The children of a node are listed in ascending order of the least leaf id below them (so leaf 0 comes first
 * at the root).  A leaf is name ":" L, the name quoted and truncated exactly as andi_hip_format_newick does; an inner
 * node is "(" children ")" support ":" L, the support in decimal; the root is "(" children ");"; L is %.8g.  Not
 * recursive: a 65535-leaf caterpillar works.  Return value and cap as andi_hip_format_newick.  Malformed nodes give 0 and
 * an empty string: n < 2, a parent that is no inner node and not the root (or a root whose parent is not -1), a cycle,
 * an inner node with fewer than two children. */
size_t andi_hip_format_newick_consensus(const andi_hip_cons_node *nodes, size_t n, size_t ninner,
										const char *const *names, int truncate_names, char *out, size_t cap);

/* ------------------------------------------------------------------ */
/* Device-resident objects                                             */
/* ------------------------------------------------------------------ */
typedef struct andi_hip_ctx andi_hip_ctx;         /* device + streams + scratch */
typedef struct andi_hip_esa andi_hip_esa;         /* one subject's esa_s (src/esa.h:42-59) in HBM */
typedef struct andi_hip_queries andi_hip_queries; /* all query sequences in HBM */

int andi_hip_device_count(void); /* visible HIP devices; 0 if none (or no usable runtime) */
int andi_hip_ctx_create(andi_hip_ctx **ctx, int device, char *errbuf, size_t errlen);
void andi_hip_ctx_destroy(andi_hip_ctx *ctx);
/* How many queries the subjects staged in this context from now on will be scanned against (0 = unknown, the
 * default).  Decides the depth of their probe tables: from 1024 queries on, one level deeper than the text's length
 * asks for (4x the table, built once per subject; fewer text accesses per probe, paid back over the queries).
 * andi_hip_dist_matrix sets it itself (n - 1: distMatrix compares every sequence with every other,
 * src/dist_hack.h:59-68).  Results do not depend on it. */
void andi_hip_ctx_expect_queries(andi_hip_ctx *ctx, size_t queries);
const char *andi_hip_last_error(const andi_hip_ctx *ctx);
int andi_hip_sync(andi_hip_ctx *ctx);

/* Upload RS (n bytes + NUL) and its suffix array (esa_init_SA's output,
 * src/esa.c:294-304).  Host→device copies only. */
int andi_hip_esa_stage(andi_hip_ctx *ctx, const char *RS, const int32_t *SA, size_t n,
					   size_t threshold, andi_hip_esa **out);
/* The same with the suffix array built on the device (esa_init_SA, src/esa.c:294-304, without the host:
 * prefix doubling on radix sorts): only RS is uploaded.  Synchronous. */
int andi_hip_esa_stage_text(andi_hip_ctx *ctx, const char *RS, size_t n, size_t threshold, andi_hip_esa **out);
/* Test hook: the suffix array as the device holds it, n entries. */
int andi_hip_esa_download_sa(andi_hip_ctx *ctx, const andi_hip_esa *esa, int32_t *SA);
/* esa_init_LCP, _CLD, _FVC, _cache (src/esa.c:373-426, 312-363, 229-245,
 * 73-215) as HIP kernels on the context's stream (asynchronous): the
 * reference's own arrays, bit for bit. */
int andi_hip_esa_build(andi_hip_ctx *ctx, andi_hip_esa *esa);
/* The index the anchor scan uses in place of those arrays: a 4^K table holding,
 * per K-mer, the outcome of get_match_cached (src/esa.c:636-656) as far as
 * the K-mer decides it, built from RS and SA alone (asynchronous).  When the
 * build finds that the reference's 10-mer table may contain an entry spanning
 * a separator (flags[0], see andi_hip_esa_flags), andi_hip_scan_rows builds
 * the reference arrays for that subject and follows the reference's walk. */
int andi_hip_esa_build_index(andi_hip_ctx *ctx, andi_hip_esa *esa);
/* The same for several staged subjects in two launches (no launch gaps, one tail). */
int andi_hip_esa_build_index_batch(andi_hip_ctx *ctx, andi_hip_esa *const *esas, size_t count);
/* flags[0]: see above; flags[2]: the 10-mer table kernel really produced such an
 * entry (only after andi_hip_esa_build). */
int andi_hip_esa_flags(andi_hip_ctx *ctx, const andi_hip_esa *esa, int32_t *flags4);
/* Test hook: copy the built arrays back.  Any pointer may be NULL.
 * LCP/CLD have n+1 entries, FVC n, cache 4^10. */
int andi_hip_esa_download(andi_hip_ctx *ctx, const andi_hip_esa *esa, int32_t *LCP,
						  int32_t *CLD, uint8_t *FVC, andi_hip_interval *cache);
/* Test hook: the scan index's probe table (what the scan consults in place of get_match_cached,
 * src/esa.c:636-656), 4^K entries of two 32-bit words {x, y}; *K receives the depth.  y & 3 is the kind:
 * 0 FINAL -- the K-mer is absent from RS, its longest match is y >> 8 (< K) characters, unique iff y & 4,
 * and then x is the suffix-array index of the one suffix; 1 SINGLE -- it occurs once, at RS offset x;
 * 2 MULTI -- it occurs (y >> 8) + 1 times, at the suffix-array indices x, x + 1, ...; 3 -- search the
 * whole suffix array.  `table` may be NULL (only K is wanted); it needs 8 << 2K bytes. */
int andi_hip_esa_download_index(andi_hip_ctx *ctx, const andi_hip_esa *esa, uint32_t *table, int *K);
/* the form of the table's entries of K-mers that occur once (test hook): 0 plain, 1 the up to 13 nucleotides behind the
 * occurrence in the entry, 2 the up to min(4, 16 - K) the device sorter's keys held (the default for subjects sorted on the device) */
int andi_hip_esa_single_form(const andi_hip_esa *esa);
void andi_hip_esa_free(andi_hip_ctx *ctx, andi_hip_esa *esa);
size_t andi_hip_esa_bytes(const andi_hip_esa *esa);

int andi_hip_queries_stage(andi_hip_ctx *ctx, const andi_hip_seq *seqs, size_t n,
						   andi_hip_queries **out);
void andi_hip_queries_free(andi_hip_ctx *ctx, andi_hip_queries *q);
/* Queries [first, first + count) of q, sharing q's device buffers (no copy, no upload): scan with it like any staged set
 * (query k of the view is query first + k of q).  Free it with andi_hip_queries_free before q; that frees only what the
 * view owns (its segmentation). */
int andi_hip_queries_view(andi_hip_ctx *ctx, const andi_hip_queries *q, size_t first, size_t count,
						  andi_hip_queries **out);

/* get_match_cached / get_match (src/esa.c:615-656) for `count` consecutive
 * suffixes of query `qidx`: out[k] = match of Q[first+k ..] (fields l,i,j;
 * m = SA[i], the pos_S dist_anchor would use, src/process.c:120). */
int andi_hip_match_positions(andi_hip_ctx *ctx, const andi_hip_esa *esa,
							 const andi_hip_queries *q, size_t qidx, size_t first, size_t count,
							 int cached, andi_hip_interval *out_host);

/* dist_anchor (src/process.c:141-214) for every (subject, query) pair of
 * `nsub` staged subjects whose index is built (andi_hip_esa_build_index, or
 * andi_hip_esa_build for the reference walk) against all queries.  self[s] = index of the
 * query that is subject s itself (gets the diagonal placeholder) or -1.
 * M_dev: device pointer, nsub * nq models, row s = subject s.  Asynchronous
 * on the context's stream. */
int andi_hip_scan_rows(andi_hip_ctx *ctx, andi_hip_esa *const *subjects,
					   const int64_t *self, size_t nsub, const andi_hip_queries *q, int model,
					   uint32_t segment, andi_hip_model *M_dev);

/* calculate_bootstrap (src/process.c:289-321): `replicates` resampled matrices
 * from M (host, n*n) into B (host, replicates*n*n).  For every pair i < j the
 * summed counts model_average(M(i,j), M(j,i)) are redrawn from a multinomial
 * (model_bootstrap, src/model.c:222-232), mirrored, diagonal {counts[0]=1,
 * seq_len=1}.  Deterministic in (seed, replicate, i, j).  The reference seeds
 * GSL from the clock, so only the distribution can be compared, not the draws. */
int andi_hip_bootstrap(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, uint64_t seed,
					   size_t replicates, andi_hip_model *B);

/* Replicates first ... first + count - 1 of the stream andi_hip_bootstrap draws, into B (host, count*n*n): bit for bit
 * B[first : first + count] of a call of andi_hip_bootstrap for first + count replicates, so a caller can work in pieces
 * that fit.  andi_hip_bootstrap is the range from 0.  first + count must be below 2^32; that, a NULL pointer or n outside
 * 1 ... 65535 fail with 1 before any HIP call; count == 0 does nothing. */
int andi_hip_bootstrap_range(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, uint64_t seed, size_t first,
							 size_t count, andi_hip_model *B);

/* The PORTABLE estimator: out[k] = the portable estimate of m[k], k < count.  No GPU is touched; returns 1 on a NULL
 * pointer (with count > 0) or a model outside 0 ... 4.  It is, operation for operation, andi_hip_estimate -- the same
 * sums, divisions, term order of LogDet's determinant, nucl <= 3 -> NaN, d <= 0.0 ? 0.0 : d -- with every operation an
 * IEEE double operation rounded on its own (no a*b+c contracted into an FMA) and libm's log replaced by andi_log, which
 * is made of + - * /, comparisons and moves of bits only.  The device computes the same function from the same text
 * (andi_amd/csrc/andi_estimate.h), so andi_hip_bootstrap_nj's distances equal this function's bit for bit; RAW and ANI
 * take no logarithm and equal andi_hip_estimate bit for bit; the others differ from it by what andi_log differs from the
 * host's log (at most 1 ulp of the logarithm measured against glibc; DESIGN.md 10.6 has the distances' figures).
 *
 * andi_log(x), the contract (tests/estimate_model.py restates it in NumPy):
 *  - x is NaN or x < 0: the quiet NaN 0x7ff8000000000000; x == 0.0 (either sign): -inf; x == +inf: +inf;
 *  - k = 0; a subnormal x (exponent field 0) is first multiplied by 2^54 (exact) and k = -54;
 *  - k += (exponent field of x) - 1023; m = x with its exponent field set to 1023, in [1, 2);
 *    if m > 1.4142135623730951 (0x3ff6a09e667f3bcd): m = m * 0.5, k += 1;
 *  - f = m - 1.0 (exact); s = f / (2.0 + f); z = s * s;
 *  - p = 0.0; for i = 27, 25, ..., 3: p = p * z + 1.0 / i   (thirteen steps; 1.0 / i is the rounded quotient);
 *  - hfsq = (0.5 * f) * f; R = (2.0 * z) * p; t = s * (hfsq + R);
 *  - k == 0: the result is f - (hfsq - t);
 *  - otherwise, dk = (double)k, ln2_hi = 6.93147180369123816490e-01 (0x3fe62e42fee00000), ln2_lo =
 *    1.90821492927058770002e-10 (0x3dea39ef35793c76): the result is dk * ln2_hi - ((hfsq - (t + dk * ln2_lo)) - f);
 *  every operation rounded to double, in the order the parentheses give.  (x = 2^k m, log m = 2 atanh(s) = 2s + 2s z
 *  (1/3 + z/5 + ... + z^12/27), in fdlibm's arrangement.) */
int andi_hip_estimate_portable(const andi_hip_model *m, size_t count, int model, double *out);

/* Neighbor-joining (Saitou & Nei 1987, as PHYLIP's neighbor) of the n x n distance matrix D (host memory, row-major) on
 * the context's device.  Only D[i][j] with i < j is read; those entries are mirrored, the diagonal and the lower
 * triangle are ignored.  Writes n - 2 records for n >= 3 -- n - 3 pair joins, then the final three -- and one for n = 2.
 * A non-finite entry fails through the context's error, which names the first such D[i][j] in row-major order; nothing
 * is written then.  2 <= n <= 65535; bad arguments fail with 1 before any HIP call.  Synchronous.
 *
 * The result is bit-exact to this contract (tests/nj_model.py restates it):
 *  - leaf i has id i and starts in slot i; the node join step s creates (from 0) has id n + s and takes the lower slot of
 *    its two children; the other slot leaves the active set;
 *  - a step with r >= 4 active nodes: R_x is the sequential sum, from +0.0, of D[x][k] over the active slots k in
 *    ascending order (x included, D[x][x] = +0.0); for each active pair, with x the member of smaller id,
 *    Q = ((double)(r-2) * D[x][y] - R_x) - R_y, each operation rounded; the least Q by value (-0.0 == +0.0) is joined,
 *    ties to the smaller id(x), then the smaller id(y); a NaN Q (finite input can overflow: inf - inf) orders after
 *    every number, and among NaN Q values the same id order decides; with a the smaller id, b the other and d = D[a][b]:
 *    la = d*0.5 + (R_a - R_b) / (double)(2*(r-2)), lb = d - la, record {a, b, -1, 0, la, lb, 0.0}; for every other
 *    active k, D[u][k] = D[k][u] = ((D[a][k] + D[b][k]) - d) * 0.5, D[u][u] = +0.0;
 *  - r = 3: the nodes x < y < z by id, lx = ((D[x][y] + D[x][z]) - D[y][z]) * 0.5, ly = ((D[x][y] + D[y][z]) - D[x][z]) * 0.5,
 *    lz = ((D[x][z] + D[y][z]) - D[x][y]) * 0.5, record {x, y, z, 0, lx, ly, lz};
 *  - n = 2: {0, 1, -1, 0, D[0][1]*0.5, D[0][1]*0.5, 0.0};
 *  - negative branch lengths are kept as computed. */
int andi_hip_nj(andi_hip_ctx *ctx, const double *D, size_t n, andi_hip_nj_join *joins);
/* Neighbor-joining of `count` matrices of one n in shared launches: D is count row-major n x n matrices one after the
 * other (host memory, upper triangles read), joins receives count * nrec records, nrec = n - 2 (1 for n = 2), matrix k's
 * from joins + k * nrec on -- bit for bit what the call above writes for D + k*n*n (the same kernels, the replicate as
 * the grid's second dimension; a step of all matrices is the three launches a step of one is).  bad[k] = -1 for a usable
 * matrix; else i*n + j of its first non-finite D[i][j] (i < j, row-major order), its nrec records are all-zero bytes, and
 * the other matrices are not affected.  Returns 0 when it ran, bad matrices or not; 1 through the context's error on a
 * HIP error; 1 before any HIP call on bad arguments (a NULL pointer, count == 0, n outside 2 ... 65535).  When
 * count * n * n * 8 bytes do not fit the device (or count > 65535) the matrices are taken in groups; the results do not
 * depend on the grouping, and the call does not fail on size while one matrix fits.  Synchronous. */
int andi_hip_nj_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, andi_hip_nj_join *joins, int64_t *bad);
/* Bootstrap trees without matrices: draw, estimate and join on the device.  For k < count, replicate first + k of the
 * stream andi_hip_bootstrap draws from M (host, n*n) is turned into distances and joined; joins (count * nrec records)
 * and bad (count) are those of andi_hip_nj_batch.  No replicate exists as models anywhere, nor as doubles on the host
 * unless D is given.  The contract, for replicate first + k and every pair i < j:
 *  - the sixteen counts are those andi_hip_bootstrap_range draws for that replicate and pair;
 *  - the distance is the portable estimate (andi_hip_estimate_portable) of the model whose counts[c] is
 *    (uint32_t)(draw[c] + draw[c]) -- what andi_hip_model_average makes of the mirrored replicate, which is what
 *    andi_hip_distances sees; seq_len enters no estimator;
 *  - the records are what andi_hip_nj_batch writes for those matrices, bit for bit; a replicate with a non-finite distance
 *    gets bad[k] = i*n + j of the first one and all-zero records, and the others are not affected;
 *  - D, if not NULL, receives the count matrices (n x n, mirrored, diagonal +0.0) as the joins start from them, copied
 *    out before the first join step; it costs a copy only when asked for.
 * model is 0 ... 4 (ANDI_M_*).  A NULL ctx, M, joins or bad, count == 0, n outside 2 ... 65535, a model outside 0 ... 4 or
 * first + count of 2^32 or more fail with 1 before any HIP call.  On the device: the summed counts of every pair, 64
 * bytes each (n(n-1)/2 of them), and a group of replicates sized as andi_hip_nj_batch's; the results depend neither on the
 * grouping nor on how a range is split over calls, and the call does not fail on size while one replicate fits.
 * Synchronous. */
int andi_hip_bootstrap_nj(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, uint64_t seed, size_t first,
						  size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D);
/* The tree builder by method: neighbor-joining as above, or BIONJ (Gascuel, Mol. Biol. Evol. 14:685, 1997), which is
 * neighbor-joining but for the weight lambda with which a join averages its two nodes' distances to the rest: chosen per
 * join to minimise the variance of the new distances, not fixed at 1/2. */
#define ANDI_TREE_NJ 0
#define ANDI_TREE_BIONJ 1
/* The tree of the n x n matrix D by `method` (ANDI_TREE_*): arguments, records, errors and limits as andi_hip_nj; a method
 * outside 0 ... 1 fails with 1 before any HIP call, like the other bad arguments.  With ANDI_TREE_NJ the records are
 * andi_hip_nj's, bit for bit.  Synchronous.
 *
 * BIONJ is bit-exact to this contract (tests/bionj_model.py restates it):
 *  - andi_hip_nj's, word for word: the input (upper triangle read and mirrored, diagonal +0.0, a non-finite entry fails
 *    and names the first one); slots, ids and the ascending active list; R_x and Q; the choice of the pair, its tie rule
 *    and its NaN rule; la, lb and the record; the r = 3 record; n = 2; negative lengths kept; 2 <= n <= 65535;
 *  - a second matrix V, by the same slots: before the first step V = D, mirrored, diagonal +0.0;
 *  - a step with r >= 4: the pair (a, b), a the smaller id, and d, la, lb as in andi_hip_nj; then, every operation rounded
 *    and none fused:
 *      RV_x = the sequential sum, from +0.0, of V[x][k] over the active slots k in ascending order (x included): R_x's rule;
 *      vab = V[a][b];
 *      lambda = 0.5 + (RV_b - RV_a) / ((double)(2*(r-2)) * vab);
 *      if vab == 0.0 (either sign) or lambda is NaN: lambda = 0.5;  then lambda < 0 -> 0.0 and lambda > 1 -> 1.0;
 *      mu = 1.0 - lambda;
 *      for every other active k: D[u][k] = D[k][u] = lambda*(D[a][k] - la) + mu*(D[b][k] - lb),
 *                                V[u][k] = V[k][u] = (lambda*V[a][k] + mu*V[b][k]) - (lambda*mu)*vab;
 *      D[u][u] = V[u][u] = +0.0.
 *    (V[a][a] and V[b][b] are +0.0 and V[a][b] = V[b][a], so RV_b - RV_a is Gascuel's sum over k != a, b of V[b][k] - V[a][k]
 *    in exact arithmetic; it is stated through row sums because the device sums a row of V by the chain that sums a row of D.)
 *  Overflow of finite input can make lengths inf or NaN, as in andi_hip_nj; a NaN lambda is 1/2. */
int andi_hip_tree(andi_hip_ctx *ctx, const double *D, size_t n, int method, andi_hip_nj_join *joins);
/* andi_hip_nj_batch by method: matrix k's records are bit for bit what andi_hip_tree writes for D + k*n*n with that method;
 * bad, the grouping ("the results do not depend on the grouping") and the return values are andi_hip_nj_batch's, a method
 * outside 0 ... 1 one more bad argument.  A BIONJ matrix costs two n x n matrices of doubles on the device, so its groups
 * are half as large. */
int andi_hip_tree_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, int method, andi_hip_nj_join *joins,
						int64_t *bad);
/* andi_hip_bootstrap_nj by method: the same replicates and distances, joined by `method`; the records are what
 * andi_hip_tree_batch writes for those matrices with that method, bit for bit.  D, if given, receives the distance
 * matrices only (never V).  A method outside 0 ... 1 is one more bad argument. */
int andi_hip_bootstrap_tree(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, int method, uint64_t seed,
							size_t first, size_t count, andi_hip_nj_join *joins, int64_t *bad, double *D);
/* Bootstrap support of the branches of `tree` (n - 2 records) among the `count` replicate trees `reps` (count * (n - 2)
 * records, replicate k's from reps + k*(n - 2) on).  Pair record s of a tree, 0 <= s < n - 3, defines the bipartition
 * {L, leaves \ L} with L the leaves below node n + s; an unrooted binary tree has exactly these n - 3 non-trivial
 * bipartitions.  support[s] = the number of replicates k with !skip || !skip[k] whose tree has the same bipartition as an
 * UNORDERED pair of sets: trees of one unrooted topology joined in another order, or with another final three, agree on
 * every branch.  The count is exact (a hash of the leaf set only pre-filters; a match is confirmed on the sets).  n < 4:
 * nothing is written, returns 0.  The records are validated on the host before any HIP call, in O(n * count): the ids
 * must be those andi_hip_nj gives -- every child a leaf or an earlier record's node (andi_hip_format_newick's rule) and
 * every node a child exactly once; a skipped replicate's records are not looked at (skip may be NULL).  Bad arguments (a
 * NULL ctx, tree, reps or support, count == 0, n outside 2 ... 65535) and bad records return 1 through the context's
 * error.  Not recursive: any depth works; the replicates' leaf sets are built in groups that fit the device.  Synchronous. */
int andi_hip_nj_support(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
						size_t count, const uint8_t *skip, uint32_t *support);
/* Every distinct non-trivial bipartition ("split") among the `count` replicate trees `reps` (as above: count * (n - 2)
 * records, what andi_hip_nj_batch writes), with its frequency: what a consensus tree is made of (andi_hip_consensus).
 * A split is kept as its canonical side, the leaf set WITHOUT leaf 0 (a set that holds leaf 0 counts as its complement),
 * in W = ceil(n / 64) words, bit i & 63 of word i >> 6 = leaf i.  Distinct splits are numbered by first appearance:
 * replicates in ascending k (those with skip && skip[k] left out and not looked at), within a replicate the pair records
 * in ascending s; the first split seen is id 0.
 *  - ids[k*(n-3) + s] = the id of the bipartition of pair record s of replicate k; 0xFFFFFFFF for a skipped replicate;
 *  - *nsplits = the number of distinct splits;
 *  - (*freq)[id] = the number of used replicates whose tree has split id (a valid tree has each of its splits once);
 *  - (*sets)[id*W + w] = word w of the canonical side of split id.
 * *freq and *sets are malloc'ed by the library: free each with andi_hip_free.  The result is exact: a hash of the set only
 * pre-filters, two sets are one split iff all W canonical words agree, whatever else shares their hash.  n < 4: *nsplits
 * = 0, *freq = *sets = NULL, ids is not written (it may be NULL), returns 0.  Every replicate skipped: *nsplits = 0, the
 * pointers NULL, ids all 0xFFFFFFFF, returns 0.  Argument checks (a NULL ctx, reps, ids, nsplits, freq or sets, count ==
 * 0, n outside 2 ... 65535) and the validation of the used replicates' records are those of andi_hip_nj_support, on the
 * host before any HIP call; they return 1 through the context's error.  Not recursive; the replicates' leaf sets are
 * built in groups that fit the device and are never resident all at once.
 * Unlike andi_hip_nj_support this call CAN FAIL ON SIZE: the table of the distinct splits -- W * 8 + 28 bytes each -- is
 * resident on the device.  It gets room for every set of every used replicate or, if that is more, for as many splits as
 * half of the device memory that is free at the call holds; when the trees have more distinct splits than that, the call
 * returns 1 and the context's error names the bytes the table needed (at 65535 leaves a split is 8 KiB and a tree has
 * 65532 of them: 537 MB per replicate that shares no branch with the others).  On any failure *nsplits = 0 and the
 * pointers are NULL.  Synchronous. */
int andi_hip_nj_splits(andi_hip_ctx *ctx, const andi_hip_nj_join *reps, size_t n, size_t count, const uint8_t *skip,
					   uint32_t *ids, size_t *nsplits, uint32_t **freq, uint64_t **sets);
/* Transfer bootstrap support (Lemoine et al., Nature 2018) of the branches of `tree` among the replicate trees `reps`;
 * tree, reps, n, count and skip as andi_hip_nj_support.  Pair record s (0 <= s < n - 3) of a tree defines the leaf set
 * L_s below node n + s; for two leaf sets h(A, B) = |A xor B| over the n leaves, and the transfer distance is
 * d(A, B) = min(h, n - h), which does not depend on the side either bipartition is kept on.
 *  - depth[s] = min(|L_s|, n - |L_s|) of the tree's pair record s (n - 3 values; >= 2 for andi_hip_nj's records);
 *  - per[k*(n-3) + s], the transfer index of branch s in replicate k, = min(depth[s] - 1, min over the pair records t of
 *    replicate k of d(L_s, L_{k,t})): the cap depth[s] - 1 is what the replicate's leaf branches contribute (a leaf of
 *    the smaller side is that far away).  0xFFFFFFFF for a skipped replicate.  per may be NULL;
 *  - transfer[s] = the sum of per[k][s] over the used replicates, 64 bits (n - 3 values).  The sums of calls over
 *    disjoint chunks of replicates add up to the sum of one call.
 * The transfer bootstrap expectation of branch s is 1 - transfer[s] / (used * (depth[s] - 1)), which
 * andi_hip_format_newick_transfer prints.  The number of used replicates with per[k][s] == 0 is andi_hip_nj_support's
 * support[s].  Everything is an integer and exact.  n < 4: nothing is written, returns 0.  Every replicate skipped:
 * transfer all 0, depth written, per all 0xFFFFFFFF, returns 0.  Bad arguments (a NULL ctx, tree, reps, depth or
 * transfer, count == 0, n outside 2 ... 65535) and the validation of the tree's and the used replicates' records are
 * those of andi_hip_nj_support, on the host before any HIP call; they return 1 through the context's error.  The
 * replicates' leaf sets are built in groups that fit the device; the results do not depend on the grouping, and the call
 * does not fail on size while one tree's sets fit.  Work: (n - 3)^2 * used * ceil(n / 64) word pairs.  Synchronous. */
int andi_hip_nj_transfer(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
						 size_t count, const uint8_t *skip, uint32_t *depth, uint64_t *transfer, uint32_t *per);
/* The rogue genomes of the bootstrap: per leaf, how often it is one of the leaves that have to move (the per-taxon
 * transfer score of Lemoine et al. 2018 and their booster).  tree, reps, n, count, skip, L_s, the validation of the records
 * and the grouping of the replicates are those of andi_hip_nj_transfer.  For a used replicate k and a pair record s of the
 * tree (0 <= s < n - 3):
 *  - for every pair record t of replicate k, h = |L_s xor L_{k,t}| over the n leaves and d = min(h, n - h);
 *  - dist[k*(n-3) + s] = the least d over t.  It is NOT capped: the replicate's leaf branches are no candidates;
 *  - match[k*(n-3) + s] = the LEAST t that attains it.  In a tie the result therefore depends on the order of the
 *    replicate's records (as booster's depends on its traversal): another writing of the same replicate tree can name
 *    another branch and so other leaves;
 *  - flip = h > n - h at that t (none at h == n - h); M(k, s) = L_s xor L_{k,match}, with flip its complement within the
 *    n leaves (the padding bits of the last word stay zero): |M(k, s)| = dist[k][s], the leaves that have to move;
 *  - limit[s] = (uint32_t)floor(cutoff * (double)(depth[s] - 1)), one rounded multiplication, depth as in
 *    andi_hip_nj_transfer; the pair (k, s) is COUNTED iff dist[k][s] <= limit[s].  A counted pair has dist <= depth - 1,
 *    so its dist is andi_hip_nj_transfer's per;
 *  - moved[i] (n values) = the number of counted pairs with leaf i in M(k, s); *pairs = the number of counted pairs.
 * match and dist are count * (n - 3) values each; either may be NULL; a skipped replicate's row is 0xFFFFFFFF in both.
 * What follows: min(dist, depth - 1) is andi_hip_nj_transfer's per; the sum of moved is the sum of dist over the counted
 * pairs; cutoff = 0 gives moved all 0 and *pairs = the sum of andi_hip_nj_support's support; the moved and pairs of calls
 * over disjoint chunks of replicates add up to those of one call; nothing depends on the grouping.  Everything is an
 * integer and exact.  n < 4: moved[0 .. n) and *pairs are set to 0, match and dist are not written, returns 0.  Every
 * replicate skipped: zeros, the rows 0xFFFFFFFF, returns 0.  Bad arguments (a NULL ctx, tree, reps, moved or pairs, count
 * == 0, n outside 2 ... 65535, a cutoff that is NaN or outside [0, 1]) and records that are not andi_hip_nj's return 1
 * through the context's error, on the host before any HIP call.  Synchronous, on the context's stream. */
int andi_hip_nj_transfer_taxa(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, const andi_hip_nj_join *reps, size_t n,
							  size_t count, const uint8_t *skip, double cutoff, uint64_t *moved, uint64_t *pairs,
							  uint32_t *match, uint32_t *dist);

/* Agglomerative (linkage) clustering of the n x n distance matrix D (host memory, row-major) on the context's device:
 * single, complete or average linkage (UPGMA, the other mode of PHYLIP's neighbor).  Unlike neighbor-joining it takes a
 * pair without a distance.  Writes n - 1 records.  2 <= n <= 65535; bad arguments (a NULL pointer, a method outside
 * 0 ... 2, n out of range) fail with 1 before any HIP call.  Synchronous, on the context's stream.
 *
 * The result is bit-exact to this contract (tests/linkage_model.py restates it):
 *  - input: only D[i][j] with i < j is read; those entries are mirrored, the diagonal is +0.0.  A NaN is taken as +inf
 *    (the pair without a distance: farther than anything measurable); +inf, negative values and +-0.0 are used as they
 *    are.  A -inf fails through the context's error, which names the first such D[i][j] in row-major order; nothing is
 *    written then;
 *  - leaf i has id i, size 1 and starts in slot i; step s (from 0) creates node n + s, which takes the lower slot of its
 *    two children; the other slot leaves the active set.  These are the ids of SciPy's Z;
 *  - a step: among the active pairs, with x the member of smaller id, the least D[x][y] by value (-0.0 == +0.0) is
 *    joined, ties to the smaller id(x), then the smaller id(y).  A NaN (only from overflow in the average rule: inf - inf)
 *    orders after every number, +inf included, and among NaNs the same id order decides.  With a = id(x), b = id(y):
 *    record {a, b, n_a + n_b, 0, D[a][b]}, the height's bits those of that entry;
 *  - the update, for every other active k, D[u][k] = D[k][u] =
 *      single:   D[b][k] < D[a][k] ? D[b][k] : D[a][k]
 *      complete: D[b][k] > D[a][k] ? D[b][k] : D[a][k]
 *        (a's value on equality, which fixes the bits where +0.0 meets -0.0),
 *      average:  ((double)n_a * D[a][k] + (double)n_b * D[b][k]) / (double)(n_a + n_b), each operation rounded, no FMA;
 *    n_u = n_a + n_b.
 * With ties the heights of the average rule need not ascend (nor do they under rounding): see andi_hip_linkage_cut. */
enum { ANDI_LINK_SINGLE = 0, ANDI_LINK_COMPLETE = 1, ANDI_LINK_AVERAGE = 2 };
/* One record of a linkage tree (andi_hip_linkage): node ids a, b (a the smaller), the leaves below the new node, the
 * height at which it was made.  24 bytes. */
typedef struct {
	int32_t a, b;
	uint32_t size, pad;
	double height;
} andi_hip_link;
int andi_hip_linkage(andi_hip_ctx *ctx, const double *D, size_t n, int method, andi_hip_link *links);
/* The clustering of `count` matrices of one n in shared launches: D is count row-major n x n matrices one after the other,
 * links receives count * (n - 1) records, matrix k's from links + k * (n - 1) on -- bit for bit what the call above writes
 * for D + k*n*n (the same kernels, the replicate as the grid's second dimension).  bad[k] = -1 for a usable matrix; else
 * i*n + j of its first -inf D[i][j] (i < j, row-major order), its records are all-zero bytes, and the other matrices are
 * not affected (andi_hip_nj_batch's rule).  Returns 0 when it ran, bad matrices or not; 1 through the context's error on
 * a HIP error; 1 before any HIP call on bad arguments (a NULL pointer, count == 0, a method outside 0 ... 2, n outside
 * 2 ... 65535).  The matrices are taken in groups that fit the device; the results do not depend on the grouping, and the
 * call does not fail on size while one matrix fits.  Synchronous. */
int andi_hip_linkage_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, int method, andi_hip_link *links,
						   int64_t *bad);
/* Flat clusters of a linkage tree at threshold t.  Node n + s is CLOSED iff height[s] <= t and each of its children is a
 * leaf or closed -- so an inversion of the heights cannot split a subtree.  The clusters are the maximal closed nodes and
 * the leaves below none; labels[i] (n values) is leaf i's cluster, 0-based, numbered by first appearance in ascending
 * leaf id; *nclusters their number.  A NaN height or threshold closes nothing.  Returns 1 on a NULL pointer, n outside
 * 2 ... 65535 and malformed records: a child must be a leaf or an earlier record's node, the two children differ, and no
 * node is a child twice.  Not recursive.  No GPU is touched. */
int andi_hip_linkage_cut(const andi_hip_link *links, size_t n, double t, uint32_t *labels, size_t *nclusters);
/* One representative per cluster: medoid[c] = the member i of cluster c with the least sum of D'[i][j] over the cluster's
 * members j, taken in ascending leaf id, sequentially from +0.0 (j = i included: +0.0); D' is D as andi_hip_linkage reads
 * it (upper triangle, mirrored, a NaN as +inf).  Ties go to the smaller id; a NaN sum (inf - inf) orders last.  Returns 1
 * on a NULL pointer, n outside 2 ... 65535, a label >= nclusters, a cluster without a member, or a -inf in the upper
 * triangle.  No GPU is touched. */
int andi_hip_cluster_medoids(const double *D, size_t n, const uint32_t *labels, size_t nclusters, uint32_t *medoid);
/* How often a clustering's clusters recur: stability[c] = the number of replicates k < count in which the leaf set of
 * cluster c of `labels` is exactly one cluster of rep_labels + k*n (labels of any numbering, each < n).  The counts of
 * calls over disjoint chunks of replicates add up.  Returns 1 on a NULL pointer, n outside 2 ... 65535, a label >=
 * nclusters, a replicate's label >= n, or a cluster without a member.  No GPU is touched. */
int andi_hip_cluster_stability(const uint32_t *labels, size_t nclusters, const uint32_t *rep_labels, size_t n, size_t count,
							   uint32_t *stability);
/* The Newick text of andi_hip_linkage's records, a rooted tree (dendrogram) on one line ending in ";\n".  Leaves are
 * quoted and truncated exactly as andi_hip_format_newick does; node n + s is "(" T(a) ":" L "," T(b) ":" L ")", children
 * in record order; the branch above a child is height(parent) - height(child), a leaf's height +0.0, printed %.8g;
 * negative lengths are kept; the root has no length.  Not recursive: a 65535-leaf caterpillar works.  Return value and
 * cap as andi_hip_format_newick.  Malformed records (andi_hip_linkage_cut's rule) and a branch length that is not finite
 * (a height of +inf: a pair without a distance) give 0 and an empty string. */
size_t andi_hip_format_newick_linkage(const andi_hip_link *links, size_t n, const char *const *names, int truncate_names,
									  char *out, size_t cap);

/* Missing distances estimated from quartets on the context's device, in front of the tree calls, which refuse a matrix with
 * a pair that has no distance.  D: an n x n matrix in host memory, row-major.  The estimate of a missing d(i, j) is the
 * four-point condition's bound d(i,j) <= max(d(i,k) + d(j,l), d(i,l) + d(j,k)) - d(k,l), least over the pairs {k, l}
 * whose five distances are known: equality holds in every quartet whose topology does not put i and j together.
 *
 * The result is bit-exact to this contract (tests/complete_model.py restates it in NumPy):
 *  - input: only D[i][j] with i < j is read; it is mirrored, the diagonal is +0.0.  A pair is KNOWN iff its entry is
 *    finite; NaN, +inf and -inf are MISSING.  Negative finite entries are known and kept;
 *  - rounds t = 1, 2, ... run Jacobi-style: every read of round t sees the matrix as it stood when the round began;
 *  - for every missing pair i < j the CANDIDATES of the round are the unordered pairs {k, l}, k != l, both outside {i, j},
 *    with all five of (i,k), (i,l), (j,k), (j,l), (k,l) known at the round's start; each is
 *    c = max(D[i][k] + D[j][l], D[i][l] + D[j][k]) - D[k][l], every operation rounded to double.  c is symmetric in k and
 *    l and never a NaN (the operands are finite); it may overflow to +-inf;
 *  - m = the least candidate.  With at least one candidate and m < +inf the pair is FILLED in round t with
 *    m <= 0.0 ? +0.0 : m (the estimator's own clamp; it also removes -0.0, so the signs of zero and the order of the
 *    minimum do not matter).  It is known from round t + 1 on, on equal footing with a measured entry, and never revised;
 *  - a filled pair records its round and its quartets: the number of candidates in that round;
 *  - the rounds end after one that fills nothing, or after max_rounds of them (0: no limit; every round but the last
 *    fills a pair, so there is at most one round per missing pair, and one more);
 *  - a pair still missing is the quiet NaN 0x7ff8000000000000 (andi_log's) in the output;
 *  - n < 4: there is never a candidate.
 * What the estimate is worth, on distances that a tree with branch lengths generates exactly (checked on random trees with
 * dyadic branch lengths, where every sum is exact: tests/test_complete_host.py): a value of round 1 is never below the true
 * distance, and it IS the true distance whenever some known quartet separates i from j; with 20-50 % of the pairs of 8-24
 * leaves missing at random nearly every pair was filled, within three rounds, and about four fills in five were exact.  From round 2
 * on a value can also be too small: a filled over-estimate may be the d(k,l) that is subtracted.  On noisy data the
 * minimum is biased low; round and quartets are what lets a user judge a fill.
 *
 * C receives the completed n x n matrix (it may be D); *missing the number of missing pairs of the input, *left the
 * number still missing at the end; fills the first min(cap, *missing) missing pairs in row-major (i < j) order: a filled one
 * with its value, round and quartets, an unfilled one with round 0, quartets 0 and the quiet NaN.  fills may be NULL when
 * cap is 0.  A matrix with nothing missing comes back mirrored with *missing == 0, and no quartet kernel is launched.
 * Pairs left over are no error of this call: the caller decides.  2 <= n <= 65535; bad arguments (a NULL ctx, D, C, missing
 * or left, a NULL fills with cap > 0, n out of range) fail with 1 before any HIP call and set the context's error; a HIP
 * error fails with 1 through the context's error.  Synchronous, on the context's stream.  On the device: the matrix (8 n^2
 * bytes) and 32 bytes per missing pair.  Work per round: (n - 2)(n - 3) / 2 candidates per pair still missing, at most. */
typedef struct {
	uint32_t i, j, round, pad;
	uint64_t quartets;
	double value;
} andi_hip_fill; /* 32 bytes; pad is 0 */
int andi_hip_complete(andi_hip_ctx *ctx, const double *D, size_t n, unsigned max_rounds, double *C, andi_hip_fill *fills,
					  size_t cap, size_t *missing, size_t *left);
/* The completion of `count` matrices of one n in shared launches: D is count row-major n x n matrices one after the other,
 * C receives them completed (it may be D), missing[k] and left[k] matrix k's counts -- bit for bit what the call above
 * writes for D + k*n*n (the same kernels, the replicate as the grid's second dimension; a matrix of which a round fills
 * nothing is done, whatever the others still do).  The matrices are taken in groups that fit the device; the results do
 * not depend on the grouping.  Bad arguments (a NULL pointer, count == 0, n outside 2 ... 65535) fail with 1 before any
 * HIP call.  Synchronous. */
int andi_hip_complete_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, unsigned max_rounds, double *C,
							uint64_t *missing, uint64_t *left);

/* Tree-likeness scores from all quartets on the context's device: how far the distances around every genome are from
 * fitting any tree at all, which everything above (the joined trees, their support, the completion of missing pairs)
 * takes for granted.  The score is the delta of Holland, Huber, Dress and Moulton (2002; `delta.plot` in ape): 0 for a
 * quartet that satisfies the four-point condition, towards 1 for one that is a box.  A genome's mean over the quartets it
 * is in singles out recombinants, chimeric or contaminated assemblies and mislabelled drafts before a tree is built.
 * D: an n x n matrix in host memory, row-major.
 *
 * The result is bit-exact to this contract (tests/delta_model.py restates it in NumPy):
 *  - input, as andi_hip_complete takes it: only D[i][j] with i < j is read; it is mirrored.  A pair is KNOWN iff its entry
 *    is finite; NaN, +inf and -inf are MISSING.  Negative finite entries are known;
 *  - the three sums: for every unordered quartet {x, y, u, v} of distinct genomes whose six distances are known,
 *    s1 = d(x,y) + d(u,v), s2 = d(x,u) + d(y,v), s3 = d(x,v) + d(y,u), each one rounded double addition.  Each is symmetric
 *    in its operands and the three are a set, so the quartet's value does not depend on how it is visited;
 *  - the quartet's delta: a, b, c the largest, the middle and the smallest of the three by value; w = a - c, u = a - b.
 *    The quartet is USED iff w is finite (which also drops a quartet one of whose sums overflowed).
 *    delta = w > 0 ? u / w : 0, an IEEE division, no operation contracted into an FMA.  Rounding is monotone, so
 *    0 <= u <= w and delta lies in [0, 1];
 *  - the integer: t = (uint64) floor(delta * 2^24); the multiplication is exact, t is 0 ... 2^24;
 *  - the records: out[x].quartets is the number of used quartets that contain x, out[x].sum the sum of their t.  Both are
 *    sums of integers, so the result does not depend on any order of summation (the device sums with integer atomics);
 *  - the mean: a genome's mean delta is sum / (quartets * 2^24); it resolves 6e-8;
 *  - 2 <= n <= 16384.  At n < 4 every record is {0, 0}.  The upper bound is what keeps sum below 2^64: a genome is in
 *    C(16383, 3) = 7.33e11 < 2^40 quartets.  The work is C(n, 4), about n^4 / 24, quartets: 3.8e12 at 3085 genomes, and
 *    the time follows it -- measured on one MI355X, about 5.6e11 quartets a second: 7 s at 3085 genomes, and by that rate
 *    45 s at 5000, 12 minutes at 10000, an hour and a half at 16384, in one kernel launch.
 * Bad arguments (a NULL ctx, D or out, n out of range) fail with 1 before any HIP call and set the context's error; a HIP
 * error fails with 1 through the context's error.  Synchronous, on the context's stream.  On the device: the matrix
 * (8 n^2 bytes).  There is no batch form: the scores are asked of the point estimate only. */
typedef struct {
	uint64_t sum, quartets;
} andi_hip_delta; /* 16 bytes */
int andi_hip_delta_scores(andi_hip_ctx *ctx, const double *D, size_t n, andi_hip_delta *out /* n records */);

/* Distance-based placement of queries on a neighbor-joining tree (least-squares placement, as APPLES does it): for every
 * query, the edge of the tree, the point on it and the length of the branch hanging there that fit the query's distances
 * to the leaves best.  tree: the n - 2 records of andi_hip_nj for n leaves (validated on the host by andi_hip_nj_support's
 * rule); D: nq rows of n distances, D[q*n + i] from query q to leaf i (host memory; andi_hip_distances_rect gives them);
 * method: ANDI_PLACE_OLS or ANDI_PLACE_FM; out: nq records; per_err, per_x, per_p: NULL, or nq * (2n - 3) doubles each, the
 * values of every edge.  3 <= n <= 65535.  Bad arguments (a NULL ctx, tree, D or out, nq == 0, n out of range, a method
 * outside 0 ... 1) fail with 1 before any HIP call; a branch length that is not finite and records that are not
 * andi_hip_nj's fail with 1 through the context's error, also before any HIP call.  Synchronous, on the context's stream.
 *
 * The result is bit-exact to this contract (tests/place_model.py restates it); every operation is an IEEE double operation
 * rounded on its own (no a*b+c contracted into an FMA), every sum sequential in the order given:
 *  - the tree: leaf i has id i, pair record s < n - 3 makes node n + s, the final record the centre C = 2n - 3.  parent(v)
 *    and len(v) come from the record that has v as a child (la, lb or lc).  There are 2n - 3 edges; edge v, 0 <= v < 2n - 3,
 *    joins v to parent(v) (its jplace edge number as well).  Negative lengths are kept as they are;
 *  - path lengths h(v, i) from node v to leaf i: h(i, i) = +0.0; upwards from i to C, h(parent(v), i) = h(v, i) + len(v);
 *    for every other node c, in descending id order, h(c, i) = h(parent(c), i) + len(c).  below(v, i) iff v lies on the
 *    path from i to C;
 *  - a query's row d = D[q*n .. q*n + n); leaf i is USABLE iff d_i is finite (a NaN is a pair without a distance and counts
 *    for nothing, as in andi_hip_linkage); its weight w_i is 1.0 under OLS and 1.0 / (d_i * d_i) under FM (Fitch and
 *    Margoliash's weights; the default of the command line);
 *  - per edge v, with L = len(v) and Lc = L > 0 ? L : +0.0, pass 1 over the usable i in ascending order, four sums from
 *    +0.0: if below(v, i): u = d_i - h(v, i), WA += w, UA += w*u; otherwise u = (d_i - h(parent(v), i)) - L, WB += w,
 *    UB += w*u.  If WA == 0.0 or WB == 0.0 the edge is no candidate: err = +inf, x = p = +0.0;
 *  - the solve: s = UA/WA, t = UB/WB, W = WA + WB, p0 = (s + t)*0.5, x0 = (s - t)*0.5.  If p0 >= 0 && x0 >= 0 && x0 <= Lc,
 *    (p, x) = (p0, x0).  Otherwise three candidates, in this order: (pos(((WA*s) + (WB*t))/W), +0.0);
 *    (pos(((WA*(s - Lc)) + (WB*(t + Lc)))/W), Lc); (+0.0, clamp(((WA*s) - (WB*t))/W)), with pos(a) = a > 0 ? a : +0.0 and
 *    clamp(a) = a > 0 ? (a < Lc ? a : Lc) : +0.0; the one with the least Q = WA*(e*e) + WB*(f*f), e = (p + x) - s,
 *    f = (p - x) - t, ties to the earlier one, a NaN after every number.  (In (p + x, p - x) the objective decouples, so
 *    the optimum over x in [0, Lc], p >= 0 is the free one or lies on one of the three boundary lines.)
 *  - pass 2, err from +0.0 over the usable i in ascending order: m = below(v, i) ? ((p + x) + h(v, i)) :
 *    ((p + (L - x)) + h(parent(v), i)); r = d_i - m; err += w*(r*r);
 *  - under FM, if some usable d_i == 0.0 the query IS the first such leaf i: every edge gets err = +inf, x = p = +0.0, but
 *    edge i err = +0.0 (this rule comes before the one below);
 *  - the choice: the edge with the least err by value, ties to the smaller v, a NaN after every number; the record is
 *    {v, used, x, p, err}, used the number of usable leaves.  If the least err is +inf or NaN the query is unplaced:
 *    {-1, used, +0.0, +0.0, +inf} -- always so with fewer than two usable leaves.
 * distal is x, measured from the child end of the edge (the end away from the centre: jplace's distal end).
 * On the device: the table of the (2n - 3) x n path lengths, 8 bytes each (152 MB at 3085 leaves, 68.7 GB at 65535); when
 * it does not fit the call fails through the context's error, which names the bytes.  The queries are taken in groups
 * that fit; the results do not depend on the grouping.  Work: nq * (2n - 3) * n leaf visits, twice. */
enum { ANDI_PLACE_OLS = 0, ANDI_PLACE_FM = 1 };
/* One placement (andi_hip_place): the edge (-1: unplaced), the usable leaves, the point on the edge, the length of the
 * hanging branch, the weighted squared error.  32 bytes. */
typedef struct {
	int32_t edge;
	uint32_t used;
	double distal, pendant, err;
} andi_hip_placement;
int andi_hip_place(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, size_t nq, int method,
				   andi_hip_placement *out, double *per_err, double *per_x, double *per_p);
/* The distances of the query-versus-reference mode as doubles: D[q*nr + r] = the unrounded value
 * andi_hip_format_distances_rect prints for that cell (without extra_verbose; it is the same computation).  Row-parallel
 * like andi_hip_distances.  Returns 1 on NULL pointers.  No GPU is touched. */
int andi_hip_distances_rect(const andi_hip_model *MRQ, const andi_hip_model *MQR, size_t nr, size_t nq, int model, double *D);
/* The inverse of andi_hip_format_newick: the n - 2 records (joins) of the unrooted binary tree in `text`, whose leaves are
 * the n names (3 <= n <= 65535).  The leaf whose text -- unquoted, '' undoubled, cut to ten characters under
 * truncate_names -- equals names[i] (cut likewise) gets id i.  Pair nodes are numbered n + s in the order their ")"
 * closes; a pair record has a < b, the final record x < y < z.  Labels behind a ")" (support, TBE and consensus numbers)
 * are ignored, blanks, tabs and line ends between tokens too; lengths are parsed by strtod.  Not recursive.  Refused, with
 * a message in errbuf that names the byte offset: a root without exactly three subtrees, an inner node without exactly two
 * children, a missing or non-finite length, an unknown name, a duplicate name, a missing name, and trailing text other
 * than whitespace.  Returns 0, or 1 (also on a NULL text, names or joins and n out of range).  No GPU is touched. */
int andi_hip_parse_newick(const char *text, const char *const *names, size_t n, int truncate_names, andi_hip_nj_join *joins,
						  char *errbuf, size_t errlen);
/* Placements as jplace text (version 3) for the usual readers.  "tree" is the text of andi_hip_format_newick's walk over
 * `tree` with "{v}" behind every length, v the edge number; "fields" are edge_num, likelihood, like_weight_ratio,
 * distal_length, pendant_length -- likelihood carries err and the ratio is 1, as distance-based placers fill them; one
 * {"p":[[...]],"n":["name"]} per placed query in input order, numbers %.17g, names JSON-escaped (and cut to ten characters
 * under truncate_names, as the table prints them); unplaced queries (edge -1) are left out; "metadata" names the method.
 * Return value and cap as andi_hip_format_newick; malformed records, a NULL pointer and a method outside 0 ... 1 give 0
 * and an empty string. */
size_t andi_hip_format_jplace(const andi_hip_nj_join *tree, size_t n, const char *const *ref_names, int truncate_names,
							  const andi_hip_placement *placements, size_t nq, const char *const *query_names, int method,
							  char *out, size_t cap);

/* The root of a neighbor-joining tree without an outgroup: minimal ancestor deviation (MAD; Tria, Landan and Dagan,
 * Nat. Ecol. Evol. 2017) or the midpoint of the longest path.  tree: the n - 2 records of andi_hip_nj / andi_hip_tree /
 * andi_hip_parse_newick for n leaves (validated on the host by andi_hip_place's rule); method: ANDI_ROOT_MAD or
 * ANDI_ROOT_MIDPOINT; out: one record; per_x, per_ss: NULL, or 2n - 3 doubles each, x and SS of every edge (MAD only).
 * 3 <= n <= 65535.  Bad arguments (a NULL ctx, tree or out, n out of range, a method outside 0 ... 1), a branch length that
 * is not finite and records that are not andi_hip_nj's fail with 1 before any HIP call, through the context's error, and
 * write nothing.  Synchronous, on the context's stream.
 *
 * The result is bit-exact to this contract (tests/root_model.py restates it); every operation is an IEEE double operation
 * rounded on its own (no a*b+c contracted into an FMA), every sum sequential in the order given:
 *  - the tree: leaf i has id i, pair record s < n - 3 makes node n + s, the final record the centre C = 2n - 3.  parent(v)
 *    and len(v) come from the record that has v as a child (la, lb or lc).  There are 2n - 3 edges; edge v, 0 <= v < 2n - 3,
 *    joins v to parent(v) (its jplace edge number as well).  Negative lengths are kept as they are;
 *  - path lengths h(v, i) from node v to leaf i: h(i, i) = +0.0; upwards from i to C, h(parent(v), i) = h(v, i) + len(v);
 *    for every other node c, in descending id order, h(c, i) = h(parent(c), i) + len(c).  below(v, i) iff v lies on the
 *    path from i to C;
 *  - the near-end distance t_v(i) = below(v, i) ? h(v, i) : h(parent(v), i), from the end of edge v on leaf i's side;
 *  - the patristic distance of the leaves b < c: p(b, c) = t_b(c) + len(b) = h(parent(b), c) + len(b), edge b being leaf b's
 *    own (the chain that ends at the LOWER leaf's branch; it is h(b, c)).  The pair is USED iff p is finite and p > 0:
 *    identical genomes and negative branches can give p <= 0, and such a pair counts for nothing, on every edge alike.
 *    pairs is the number of used pairs;
 *  - per edge v, with L = len(v) and Lc = L > 0 ? L : +0.0, pass 1 over the used pairs that STRADDLE the edge, those with
 *    below(v, b) != below(v, c): a is the one of b, c below v; N += (p - 2*t_v(a)) / (p*p), W += 1.0 / (p*p).  Then
 *    x = W == 0.0 ? +0.0 : clamp(N / (2*W)), clamp(a) = a > 0 ? (a < Lc ? a : Lc) : +0.0 (a NaN gives +0.0).  x is the
 *    distance of the root from the child end v of the edge (jplace's distal end, as in andi_hip_placement);
 *  - pass 2 over all used pairs, SS += r*r: for a straddling pair r = (2*d) / p - 1.0 with d the distance from b, the
 *    lower-numbered leaf, to the root: d = below(v, b) ? t_v(b) + x : t_v(b) + (L - x); for a pair on one side
 *    r = (t_v(b) - t_v(c)) / p (their deepest common ancestor under a root on edge v is the point of their path nearest
 *    to the edge, and 2*d(b, anc)/p - 1 reduces to this);
 *  - the order of the sums, in both passes: for a fixed (v, b) the inner sum over c > b ascending, from +0.0 (in pass 1 a
 *    pair that does not straddle adds nothing); then the inner sums are added over b ascending, from +0.0;
 *  - the choice: the edge with the least SS by value, ties to the smaller v, a NaN after every number.  The record is
 *    {v, 0, x, SS, pairs, ss_second, far_b, far_c}, ss_second the least SS among the other edges by the same order.  With
 *    no used pair every SS and x is +0.0 and edge 0 is chosen.  The score sqrt(ss / pairs) and the root ambiguity index
 *    sqrt(ss / ss_second) are left to the caller;
 *  - far_b < far_c is the used pair of the greatest p, ties to the first in (b, c) order; -1, -1 without a used pair.  Both
 *    methods fill it;
 *  - ANDI_ROOT_MIDPOINT: the root is the point at p*0.5 from far_b on the path to far_c.  The walk: rem = p*0.5; over the
 *    edges v of the path in order from far_b -- first upwards (towards C) to the node where the paths of far_b and far_c to
 *    C meet, then downwards to far_c --: if rem < len(v) the edge holds the root, at distal = rem on the way up and
 *    distal = len(v) - rem on the way down; otherwise rem = rem - len(v).  So a point that falls on a node belongs to the
 *    NEXT edge of the path, at that node's end of it, and an edge of length <= 0 never holds the root; if no edge takes it
 *    (rounding, negative lengths) it is far_c's edge at distal +0.0.  ss and ss_second are +0.0, per_x and per_ss are
 *    untouched; without a used pair the record is {0, 0, +0.0, +0.0, 0, +0.0, -1, -1}.
 * On the device: andi_hip_place's table of the (2n - 3) x n path lengths, 8 bytes each; when it does not fit the call fails
 * through the context's error, which names the bytes.  Under MAD the leaves b are taken in groups that fit (16 (2n - 3)
 * bytes a leaf); the results do not depend on the grouping.  Work: (2n - 3) * n(n - 1)/2 pair visits, twice -- measured on
 * one MI355X, 66 ms at 3085 leaves with the copies, 4.5 ms for the midpoint. */
enum { ANDI_ROOT_MAD = 0, ANDI_ROOT_MIDPOINT = 1 };
typedef struct {
	int32_t edge;
	uint32_t pad;
	double distal, ss;
	uint64_t pairs;
	double ss_second;
	int32_t far_b, far_c;
} andi_hip_root_result; /* 48 bytes */
int andi_hip_root(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, int method, andi_hip_root_result *out,
				  double *per_x, double *per_ss);
/* andi_hip_format_newick's text of the records J rooted on `edge` (0 <= edge < 2n - 3, n >= 3), `distal` from the edge's
 * child end: "(" T(child) ":" L(distal) "," U ":" L(len(edge) - distal) ");\n", L is %.8g, len(edge) - distal one rounded
 * subtraction.  T(v) is the subtree below v as andi_hip_format_newick prints it.  U is the rest of the tree seen from
 * parent(edge) = q: "(" then the other children of q in record order, as T(.) with their lengths, then, unless q is the
 * centre, "," U(q) ":" L(len(q)), the same construction one level up, then ")".  The old centre becomes an ordinary inner
 * node with two children (its three without the one the path to the root passes through).
 * labels: NULL, or n - 3 strings (an entry may be NULL: no label), one per pair record s; a label belongs to the EDGE
 * n + s and stands behind the ")" of whichever end of that edge is the lower one in the rooted tree: node n + s itself, or,
 * on the path from the centre to the root, its former parent (the group U(n + s)); if the root edge is an inner edge both
 * root children that are inner nodes carry its label.  The strings are printed as they are.
 * Not recursive.  Return value, cap and malformed records as andi_hip_format_newick; an edge out of range, n < 3 and a
 * distal that is not finite give 0 and an empty string too.  No GPU is touched. */
size_t andi_hip_format_newick_rooted(const andi_hip_nj_join *J, size_t n, const char *const *names, int truncate_names,
									 int32_t edge, double distal, const char *const *labels, char *out, size_t cap);

/* The branch lengths of a fixed tree refit to a distance matrix by ordinary least squares (as FastME's OLS lengths and the
 * unconstrained form of phangorn's nnls.tree; the closed form per edge of Rzhetsky and Nei 1993 and of Desper and Gascuel
 * 2002, eq. 3), and how well the tree explains the matrix under the refit lengths and under the records' own.  The
 * lengths the joining gives come from reduced matrices; these are the best fit to the distances themselves, what
 * least-squares placement (andi_hip_place) and MAD (andi_hip_root) read path lengths as.
 * tree: the n - 2 records of andi_hip_nj / andi_hip_tree / andi_hip_parse_newick for n leaves (validated on the host by
 * andi_hip_place's rule); D: the n x n host matrix -- as in andi_hip_nj only the upper triangle is read, the lower is
 * mirrored and the diagonal ignored; method: ANDI_FIT_OLS; len: 2n - 3 doubles, the refit length of every edge; out: one
 * record; leaf_ss, leaf_ss_joined: NULL, or n doubles each.  3 <= n <= 65535.  Bad arguments (a NULL ctx, tree, D, len or
 * out, n out of range, a method other than 0), a branch length of the records that is not finite, records that are not
 * andi_hip_nj's and a D[i][j], i < j, that is not finite (the message names the first in row-major order, as
 * andi_hip_nj's does) fail with 1 before any HIP call, through the context's error, and write nothing.  Synchronous, on
 * the context's stream.  andi_hip_relength puts the lengths into the records.
 *
 * The result is bit-exact to this contract (tests/fit_model.py restates it); every operation is an IEEE double operation
 * rounded on its own (no a*b+c contracted into an FMA), every sum sequential from +0.0 in the order given:
 *  - the tree, the edges, parent(v), len(v), below(v, i) and the path lengths h(v, i): andi_hip_place's.  Edge v,
 *    0 <= v < 2n - 3, joins v to parent(v); C = 2n - 3 is the centre;
 *  - the classes of the leaves around edge v, with q = parent(v): class 0 is the leaves below the first child of v's pair
 *    record, class 1 those below its second child; for a leaf edge (v < n) class 0 is {v} and class 1 is empty.  If
 *    q != C, class 2 is the leaves below the other child of q (v's sibling) and class 3 every leaf not below q; if q == C,
 *    classes 2 and 3 are the leaves below the other two children of the final record, in record order;
 *  - the sums: for fixed (v, b) and each class k != class(v, b), s_k(v, b) is the sum of D[b][c] over c > b ascending with
 *    class(v, c) == k.  For x < y, S_xy(v) is the sum over b ascending of s_y(v, b) where class(v, b) == x and of
 *    s_x(v, b) where class(v, b) == y; any other b adds nothing;
 *  - the means: n_k the sizes of the classes, m_xy = S_xy / (double)(n_x * n_y), the product in 64-bit integers;
 *  - the lengths: of a leaf edge len = ((m_02 + m_03) - m_23) * 0.5; of an inner edge, with
 *    g = (double)(n_1*n_2 + n_0*n_3) / (double)((n_0 + n_1)*(n_2 + n_3)),
 *    len = ((g*(m_02 + m_13) + (1.0 - g)*(m_12 + m_03)) - (m_01 + m_23)) * 0.5.  Negative results are kept; sums of finite
 *    input that overflow may give +-inf or NaN, which are returned as they are;
 *  - the fit, once under the refit lengths (rss, leaf_ss, length, negative, worst) and once under the records' own
 *    (rss_joined, leaf_ss_joined, length_joined, negative_joined): the path lengths h by andi_hip_place's rule under that
 *    length vector; for b < c, p(b, c) = h(parent(b), c) + len(b) (andi_hip_root's chain; every pair counts) and
 *    r = D[b][c] - p.  rss is the sum over b ascending of the sum over c > b ascending of r*r; leaf_ss[i] the sum over
 *    j != i ascending of r*r of the pair {i, j}; length the sum of len(v) over v ascending; negative the number of v with
 *    len(v) < 0;
 *  - tss: mean = (the sum over b ascending of the sum over c > b ascending of D[b][c]) / (double)pairs, pairs =
 *    n(n - 1)/2; tss is the sum of (D[b][c] - mean)^2 in the same nested order.  R^2 = 1 - rss / tss is left to the caller;
 *  - worst_b < worst_c: the pair of the greatest |r| under the refit lengths, ties to the first in (b, c) order, a NaN
 *    below every number; worst is its r.  If every residual is a NaN: -1, -1 and worst a NaN.
 * On the device: the matrix and the residuals (8 n^2 bytes each), andi_hip_place's table of the (2n - 3) x n path lengths
 * (when it does not fit the call fails through the context's error, which names the bytes), and the leaves b in groups
 * that fit 1 GiB (32 (2n - 3) bytes a leaf); the results do not depend on the grouping.  Work: (2n - 3) * n(n - 1)/2 pair
 * visits, once, without a division. */
enum { ANDI_FIT_OLS = 0 };
typedef struct {
	double rss, rss_joined;       /* residual sums of squares: refit lengths, the records' own lengths */
	double tss;                   /* sum of (D - mean)^2 */
	double length, length_joined; /* sum of all branch lengths */
	double worst;                 /* the residual D - p of the pair below */
	uint64_t pairs;               /* n(n-1)/2 */
	uint32_t negative, negative_joined; /* edges with len < 0 */
	int32_t worst_b, worst_c;     /* pair of the greatest |residual| under the refit lengths */
} andi_hip_fit_result; /* 72 bytes */
int andi_hip_fit(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, int method, double *len /* 2n-3 */,
				 andi_hip_fit_result *out, double *leaf_ss /* NULL or n */, double *leaf_ss_joined /* NULL or n */);
/* The records J with their lengths replaced: la, lb (and lc of the final record) of every record become len[child], len
 * the 2n - 3 lengths by edge (andi_hip_fit's); everything else is copied, and out may be J itself.  Returns 1, and writes
 * nothing, on a NULL pointer, n < 3 or records that are not andi_hip_nj's (andi_hip_place's rule).  No GPU is touched. */
int andi_hip_relength(const andi_hip_nj_join *J, size_t n, const double *len, andi_hip_nj_join *out);

/* A tree refined by balanced nearest-neighbor interchanges (BNNI: FastME's topology search, Desper and Gascuel 2002), and
 * its balanced (BME) branch lengths.  Neighbor-joining is one greedy pass over the balanced minimum evolution criterion and
 * never revisits a join; BNNI swaps subtrees across inner branches until no swap shortens the tree under Pauplin's length,
 * the sum over i < j of 2^(1 - hops(i, j)) D[i][j], and is consistent from any start tree (Bordewich et al. 2009).
 * tree: the n - 2 records of andi_hip_nj / andi_hip_tree / andi_hip_parse_newick for n leaves (validated on the host by
 * andi_hip_place's rule; their lengths are not read); D: as in andi_hip_fit -- the upper triangle is read and mirrored, the
 * diagonal ignored; method: ANDI_REFINE_BNNI; tol >= 0: a move is made only if it shortens the tree by more than tol;
 * max_moves: the moves made at most; out: n - 2 records, the refined tree with its balanced lengths (out may be tree
 * itself); res: one record; log: NULL, or max_moves entries, of which the first res->moves are written.  3 <= n <= 65535.
 * Bad arguments (a NULL ctx, tree, D, out or res, n out of range, a method other than 0, a tol that is negative or a NaN),
 * records that are not andi_hip_nj's and a D[i][j], i < j, that is not finite (the message names the first in row-major
 * order) fail with 1 before any HIP call, through the context's error, and write nothing.  Synchronous, on the context's
 * stream; the host looks at one record of 32 bytes a round.  The records pass andi_hip_place's validation: the formatters,
 * andi_hip_root, andi_hip_fit, andi_hip_nj_support, _transfer, _splits and andi_hip_place take them unchanged.
 *
 * The result is bit-exact to this contract (tests/bme_model.py restates it); every operation is an IEEE double operation
 * rounded on its own (no a*b+c contracted into an FMA):
 *  - the tree is rooted at the centre C = 2n - 3, the final record's node; node n + s is pair record s's; the children of
 *    a node keep slots, at first the record's order (a, b, and c for C).  Node ids stay fixed during the search: a move
 *    only re-hangs subtrees.  lev(x) is the number of edges from C to x;
 *  - A(v, c), the balanced average distance between leaf c and the subtree on the far side of edge v (v to parent(v)) from
 *    c, for every non-centre node v and every leaf c -- andi_hip_place's table shape, (2n - 3) x n.  c not below v: for a
 *    leaf v, A(v, c) = D[v][c]; for an inner v with children a and b, A(v, c) = (A(a, c) + A(b, c)) * 0.5.  c below v (a
 *    leaf is below itself): with q = parent(v) != C and s the sibling of v, A(v, c) = (A(s, c) + A(q, c)) * 0.5; with
 *    parent(v) = C, A(v, c) = (A(s1, c) + A(s2, c)) * 0.5 over the other two children of C;
 *  - S(x, r) = the sum of w(x, c) * A(r, c) over the leaves c below x, w(x, c) = 2^-(lev(c) - lev(x)), exact, and 0 once
 *    the exponent passes 1022 (w is never subnormal).  The sum is taken as 64 partial sums: p_l takes the c with
 *    c mod 64 = l in ascending order, p_l = p_l + w * A starting from +0.0; the total is the sequential sum of p_0 ... p_63
 *    in ascending l, from +0.0 (what a wavefront that reads runs of 512 bytes of a table row produces);
 *  - around an inner non-centre edge v with children a and b in slot order and q = parent(v): if q != C, s is v's sibling
 *    and sums "against u" read row q; if q = C, s and u are C's other two children in slot order and sums against u read
 *    row u.  The six averages: d_ab = S(a, b), d_as = S(a, s), d_bs = S(b, s), d_au = S(a, row of u), d_bu = S(b, row of u),
 *    d_su = S(s, row of u);
 *  - the gains: alternative 0 swaps b with s, g0 = ((d_ab + d_su) - (d_as + d_bu)) * 0.25; alternative 1 swaps a with s,
 *    g1 = ((d_ab + d_su) - (d_bs + d_au)) * 0.25;
 *  - a round takes the greatest gain over all (v, alternative), ties to the smaller v, then to alternative 0, a NaN below
 *    every number.  If it is > tol and fewer than max_moves moves were made, the move is made -- the incoming subtree s
 *    takes the outgoing one's slot in v, the outgoing one takes s's slot in q -- and the next round evaluates the new tree
 *    from nothing.  If it is not > tol the search stops with converged = 1; if it is, but max_moves moves were made, with
 *    converged = 0.  A log entry is the move's gain and the least leaves of the outgoing (first) and the incoming (second)
 *    subtree, which name them whatever the numbering;
 *  - the balanced lengths, from the same sums, on the first round's tree (length_before) and on the final tree (the
 *    output, length_after): of a leaf edge v, ((S(v, s) + S(v, row of u)) - d_su) * 0.5 with s and u as for an inner edge;
 *    of an inner edge, ((d_as + d_au) + (d_bs + d_bu)) * 0.25 - (d_ab + d_su) * 0.5.  Negative lengths are kept.  length_*
 *    is the sequential sum of the lengths over v ascending, from +0.0; it is Pauplin's length of the tree up to rounding.
 *    n = 3 has no inner edge: 0 moves, and the three balanced lengths;
 *  - the output numbering (on the host, O(n)): the centre stays the final record; children are visited in order of their
 *    least leaf; inner nodes get ids n, n + 1, ... in post-order; a pair record has the smaller id as a, the final record
 *    x < y < z; the lengths are the balanced ones of the final tree.
 * tol should lie above the gains' rounding noise, about n * 2^-53 times the largest distance: with a smaller one a search
 * may go on making moves that mean nothing until max_moves ends it.
 * On the device: the table (8 (2n - 3) n bytes; when it does not fit the call fails through the context's error, which
 * names the bytes), the matrix (8 n^2), the leaf sets.  Work a round: the table once, read about twice. */
enum { ANDI_REFINE_BNNI = 0 };
typedef struct {
	double length_before, length_after; /* the sum of the balanced lengths: of the tree given, of the refined one */
	uint64_t moves;                     /* interchanges made */
	int32_t converged;                  /* 1: no interchange gains more than tol; 0: max_moves ended the search */
	int32_t pad;
} andi_hip_refine_result; /* 32 bytes */
typedef struct {
	double gain;           /* what the move shortened the tree by */
	int32_t first, second; /* the least leaf of the subtree that left the edge's lower node, of the one that took its place */
} andi_hip_refine_move; /* 16 bytes */
int andi_hip_refine(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, int method, double tol,
					size_t max_moves, andi_hip_nj_join *out, andi_hip_refine_result *res,
					andi_hip_refine_move *log /* NULL or max_moves */);

/* The same search with FastME's wider move, balanced subtree pruning and regrafting (SPR): a round prunes one subtree and
 * re-hangs it on any other branch, so it leaves the local optima of interchanges and comes back from a far start in few
 * rounds.  Arguments, validation (messages begin "andi_hip_refine_spr:"), error path, result record, output numbering and
 * the balanced lengths are andi_hip_refine's; there is no method argument.  log: NULL, or max_moves entries of 24 bytes.
 *
 * The move.  The tree is unrooted.  Prune the side X of an edge (x, v0), x the node on X's side; the inner node v0 has two
 * other neighbours p and q.  Y0 is the side of (p, v0) away from v0.  A path v0, v1 = q, ..., vk (k >= 1) of inner nodes
 * ends in a target edge f = (vk, w); Z is the side of f beyond w, Y_i the side of v_i's third edge, W1 the side of (v0, v1)
 * beyond v1.  After the move p and q are adjacent and v0 sits on f with the neighbours x, vk and w.  k = 1 is an
 * interchange.  The candidates of a round: every side of every edge as X (the upper side only of an inner edge), with
 * every edge on the other side that is not adjacent to v0 as f.
 *
 * Bit-exact to this contract (tests/spr_model.py restates it), every operation rounded on its own:
 *  - the tree, A, S and the lengths are andi_hip_refine's, on the tree rooted at C.  An edge goes by its lower node;
 *  - B(e, f) for all edges e, f, a (2n - 3)^2 table: the balanced average between the side of e away from f and the side
 *    of f away from e; B(e, e) between the two sides of e.  It is A's recursion with the edge f where the leaf c was, "f
 *    lies below e or is e" where "c lies below v" was: f not below e: for a leaf e, B(e, f) = A(f, e); for an inner e with
 *    children a and b, B(e, f) = (B(a, f) + B(b, f)) * 0.5.  f below e or e: with q = parent(e) != C and s the sibling,
 *    B(e, f) = (B(s, f) + B(q, f)) * 0.5; with parent(e) = C, (B(s1, f) + B(s2, f)) * 0.5 over C's other two children in
 *    slot order.  B is symmetric only up to rounding; the terms below name the entry they read;
 *  - with ex, ep, e1, ey_i the edges of X, Y0, W1 and Y_i (ex = (x, v0), ep = (p, v0), e1 = (v0, v1)):
 *    R_0 = +0.0, R_i = 0.5 * R_(i-1) + B(ex, ey_i); h = 2^-k, exact, and +0.0 once k > 1022;
 *      t1 = (0.5 * (1.0 - h)) * (B(ex, ep) - B(ex, f))      t2 = 0.5 * B(ex, e1) - (0.5 * h) * B(ex, f)
 *      t3 = 0.5 * B(ep, e1) - (0.5 * h) * B(ep, f)          t4 = 0.5 * B(f, f) - (0.25 * h) * (B(ep, f) + B(ex, f))
 *      gain = (((t1 + t2) - t3) + t4) - 0.25 * R_k
 *    which is Pauplin's length of the tree minus that of the tree after the move, up to rounding;
 *  - a round takes the greatest gain, a NaN below every number; ties go to the smaller edge ex, then to its lower side as
 *    X before its upper side, then to the smaller edge f;
 *  - the tree after a move.  Every inner node keeps three neighbour slots: at first a, b and the parent for a pair
 *    record's node, a, b, c for C.  In p the slot that held v0 takes q, in q it takes p; in v0 the slot of p takes vk and
 *    the slot of q takes w; in vk the slot of w takes v0, in w the slot of vk takes v0 (a leaf has no slots).  The next
 *    round roots the tree at C again: the children of a node are its neighbours but its parent, in slot order, and
 *    everything above is evaluated on that tree from nothing.  Node ids stay fixed;
 *  - the stop rule is andi_hip_refine's: a gain that is not > tol ends the search with converged = 1, max_moves with
 *    converged = 0.  A log entry: the gain, the least leaf of X (first), the least leaf of Z (second), and k (hops).
 * On the device: B (8 (2n - 3)^2 bytes: 304 MB at 3085 leaves) beside andi_hip_refine's buffers, and the walk's stacks,
 * 96 (2n - 3) (2 depth + 2) bytes for a tree `depth` edges deep from C; when either does not fit, the call fails through
 * the context's error, which names the bytes.  The host looks at one record of 56 bytes a round. */
typedef struct {
	double gain;           /* what the move shortened the tree by */
	int32_t first, second; /* the least leaf of the pruned side X, of the side Z beyond the target edge */
	int32_t hops;          /* k: the inner nodes from v0 to the target edge, 1 for an interchange */
	int32_t pad;
} andi_hip_spr_move; /* 24 bytes */
int andi_hip_refine_spr(andi_hip_ctx *ctx, const andi_hip_nj_join *tree, size_t n, const double *D, double tol,
						size_t max_moves, andi_hip_nj_join *out, andi_hip_refine_result *res,
						andi_hip_spr_move *log /* NULL or max_moves */);

/* ------------------------------------------------------------------ */
/* The k-mer sketch screen: which references are worth an exact run    */
/* ------------------------------------------------------------------ */
/* A screen in front of the query-versus-reference mode, as Mash and sourmash are put in front of exact methods: a sketch of
 * every sequence, the number of hashes every (query, reference) pair shares, and a rule that keeps each query's best
 * references.  Everything is an integer and exact (tests/sketch_model.py restates the contract in NumPy).
 *
 * Sketch(seq, k, scale), 4 <= k <= 32, scale >= 1; seq is an andi_hip_seq, bytes over A C G T !:
 *  - a window is k consecutive bytes that are all in ACGT; a window that holds a '!' yields nothing, a sequence shorter
 *    than k has no window;
 *  - its forward code f: A = 0, C = 1, G = 2, T = 3, two bits a symbol, the first symbol most significant, a uint64; its
 *    reverse-complement code r: the same coding of the reverse complement; its canonical code c = min(f, r);
 *  - its hash h = fmix64(c), MurmurHash3's 64-bit finaliser: h ^= h >> 33; h *= 0xff51afd7ed558ccd; h ^= h >> 33;
 *    h *= 0xc4ceb9fe1a85ec53; h ^= h >> 33; all arithmetic mod 2^64;
 *  - the window is kept iff h <= UINT64_MAX / scale (integer division; scale = 1 keeps every window);
 *  - the sketch is the set of the kept hashes, ascending, each once.  Its size fits a uint32.
 * A sequence and its reverse complement have the same sketch.  shared(A, B) is the number of hashes in both sketches.
 *
 * andi_hip_sketch: the sketches of n sequences, device-resident.  The sequences are packed to 4-bit symbols
 * (andi_hip_pack_symbols), uploaded and sketched in batches of bounded size through pinned buffers; only the sketches stay
 * on the device, and the results do not depend on the batching.  A byte outside the alphabet of andi_hip_pack_symbols is
 * refused through the context's error, as the scan refuses it (';', '#' and NUL end a window as '!' does).  Bad arguments (a
 * NULL pointer, n == 0, k outside 4 ... 32, scale == 0, a sequence of more than (INT32_MAX - 1) / 2 bytes) fail with 1 before any
 * HIP call; an empty sequence is allowed and has an empty sketch.  Scratch that does not fit the device fails through the
 * context's error, which names the bytes; a batch may not yield 2^32 hashes or more.  Synchronous, on the context's stream.
 * Free the result with andi_hip_sketch_free before the context is destroyed. */
typedef struct andi_hip_sketches andi_hip_sketches; /* the sketches of a set of sequences in HBM */
int andi_hip_sketch(andi_hip_ctx *ctx, const andi_hip_seq *seqs, size_t n, int k, uint64_t scale, andi_hip_sketches **out);
size_t andi_hip_sketch_count(const andi_hip_sketches *s); /* n; 0 for NULL */
/* the sizes of the n sketches (no HIP call: the host knows them) */
int andi_hip_sketch_sizes(andi_hip_ctx *ctx, const andi_hip_sketches *s, uint32_t *sizes);
/* the hashes of sketch idx, ascending: as many as its size says */
int andi_hip_sketch_download(andi_hip_ctx *ctx, const andi_hip_sketches *s, size_t idx, uint64_t *hashes);
void andi_hip_sketch_free(andi_hip_ctx *ctx, andi_hip_sketches *s);
/* where the time of the call that made s went, in milliseconds: ms4[0] packing on the host, [1] the uploads and [2] the hash
 * kernel's two passes (HIP events), [3] sort, unique and compaction (wall time with their synchronisations).  For
 * scripts/screen_bench.py; returns 1 on a NULL pointer. */
int andi_hip_sketch_timings(const andi_hip_sketches *s, double *ms4);
/* shared[i * count(b) + j] = shared(sketch i of a, sketch j of b): host memory, count(a) x count(b), row-major.  Both sets
 * must come from this context's device and have the same k and scale; otherwise the call fails through the context's
 * error.  a == b is allowed.  A sketch of a is staged in LDS where it fits (20000 hashes) and searched in global memory
 * where it does not; the numbers are the same.  Synchronous. */
int andi_hip_sketch_shared(andi_hip_ctx *ctx, const andi_hip_sketches *a, const andi_hip_sketches *b, uint32_t *shared);
/* Selection, on the host, no GPU: from shared (nq x nr, row-major) every query takes references in the order (shared
 * descending, reference index ascending), the first `keep` of them whose count is >= max(1, min_shared).  kept[r] (nr
 * bytes) = 1 iff any query took reference r, else 0; taken[q] (nq values; may be NULL) = the number of references query q
 * took.  Returns 1 on a NULL shared or kept, nq == 0 or nr == 0. */
int andi_hip_screen_select(const uint32_t *shared, size_t nq, size_t nr, size_t keep, uint32_t min_shared, uint8_t *kept,
						   uint32_t *taken);
/* The one call: a context on `device`, the sketches of both sets, shared[q * nr + r] (nq x nr), the sketch sizes
 * (ref_sizes: nr values, query_sizes: nq; either may be NULL), everything freed.  Bad arguments (a NULL refs, queries or
 * shared, nr or nq 0, k outside 4 ... 32, scale 0, a negative device) fail through errbuf before any HIP call. */
int andi_hip_screen(const andi_hip_seq *refs, size_t nr, const andi_hip_seq *queries, size_t nq, int k, uint64_t scale,
					int device, uint32_t *shared, uint32_t *ref_sizes, uint32_t *query_sizes, char *errbuf, size_t errlen);

/* plain device memory helpers so callers need no HIP headers */
int andi_hip_dev_alloc(andi_hip_ctx *ctx, size_t bytes, void **dptr);
void andi_hip_dev_free(andi_hip_ctx *ctx, void *dptr);
int andi_hip_copy_to_host(andi_hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* The measured device-copy ceiling the roofline is reported beside: `reps` passes of a 16-bytes-per-lane
 * streaming copy kernel of the engine's own over `bytes` (source and destination allocated here, non-temporal loads and
 * stores, grid-stride), timed with HIP events on the context's stream; *gbps = read + written bytes per second / 1e9. */
int andi_hip_copy_ceiling(andi_hip_ctx *ctx, size_t bytes, int reps, double *gbps);

/* Kernel timing, measured with HIP events on the stream the kernels run on.
 * Accumulates since the last reset; read after andi_hip_sync(). */
typedef struct {
	double build_ms;      /* index builds: the scan index (andi_hip_esa_build_index), the reference arrays K1-K4 (andi_hip_esa_build) */
	uint64_t build_launches;
	double scan_ms;       /* anchor scan pass A (the dominant kernel) */
	uint64_t scan_launches;
	double stitch_ms;     /* passes B + C */
	uint64_t stitch_launches;
	uint64_t scan_query_nt; /* sum of query lengths over scanned pairs */
	uint64_t scan_pairs;
	uint64_t fixups;      /* segments whose speculative entry state was wrong */
	uint64_t reference_subjects; /* subjects scanned with the reference walk */
	double sa_ms;            /* suffix arrays built on the device (wall time of the calls: they synchronise per round) */
	uint64_t sa_builds;
	uint64_t sa_rounds;      /* sorting rounds of those builds */
	uint64_t adaptive_calls; /* scan calls that chose the segment length per pair */
	uint64_t uniform_calls;  /* ... one segment length for the call */
	uint64_t coop_calls;     /* scan calls in which pass A by wavefronts (scan_coop.hip) ran: for every pair (ANDI_COOP=n; by default calls of 2^18 ... 2^25 query symbols x subjects) or for the pairs routed to it */
	uint64_t coop_fallbacks; /* routed calls: PAIRS that kernel handed back to the lane scan (a stretch without homology, a match longer than a segment) */
	uint64_t routed_calls;   /* scan calls whose pass A was routed per pair (by default calls of 2^25 query symbols x subjects and more) */
	uint64_t coop_query_nt;  /* routed calls: query nucleotides of the pairs whose pass A ran by wavefronts ... */
	uint64_t lane_query_nt;  /* ... and by lanes */
	uint64_t pool_calls;     /* scan calls whose pass A by wavefronts was k_pool_cold's (the windows' walks pooled through global memory), not k_coop_cold's (ABI 5) */
} andi_hip_timings;

/* The library's ANDI_* environment switches (experiments, diagnostics: INTEGRATION.md lists them) are read once, when
 * the library first looks at one; this reads them again (the tests change them under a live context).  Not to be
 * called while another thread is inside the library. */
void andi_hip_reload_knobs(void);
int andi_hip_timings_get(andi_hip_ctx *ctx, andi_hip_timings *t);
void andi_hip_timings_reset(andi_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
