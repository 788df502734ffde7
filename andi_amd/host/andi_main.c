/*
 * andi_main.c — command-line front end with andi's interface (multi-FASTA in,
 * PHYLIP matrix out; same options, warnings and exit codes as src/andi.c:63-394,
 * input handling of src/io.c:103-233 and src/sequence.c:78-125,234-282), driving
 * the MI355X engine through the C-ABI in include/andi_hip.h.  Written for this
 * project; only the observable behaviour follows the reference.
 */
#define _GNU_SOURCE
#include <err.h>
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>

#include "andi_hip.h"

#define PROGRAM_VERSION "0.1"

typedef struct {
	char *name;
	char *seq;
	size_t len;
} genome;

typedef struct {
	genome *v;
	size_t n, cap;
} genome_list;

static int soft_error = 0; /* F_SOFT_ERROR, src/global.h:85-99 */
static int saw_non_acgt = 0;

#define soft_warnx(...)                                                                            \
	do {                                                                                           \
		soft_error = 1;                                                                            \
		warnx(__VA_ARGS__);                                                                        \
	} while (0)

static void *xmalloc(size_t n) {
	void *p = malloc(n ? n : 1);
	if (!p) err(errno, "Out of memory");
	return p;
}

static void push_genome(genome_list *l, genome g) {
	if (l->n == l->cap) {
		l->cap = l->cap ? l->cap * 3 / 2 + 1 : 4;
		l->v = realloc(l->v, l->cap * sizeof *l->v);
		if (!l->v) err(errno, "Out of memory");
	}
	l->v[l->n++] = g;
}

/* What reading ONE input file produced.  The files are read by a pool of threads (3085 assemblies, 6.5 GB: BASELINE's
 * config 3 -- SURVEY.md 8 f2 names ingest as the next wall-clock term); the main thread takes the results in the order of
 * the command line, so sequences, messages and flags come out as if the files had been read one after the other. */
typedef struct {
	genome_list seqs;
	char *msgs; /* the lines warnx()/warn() would have printed, in order */
	size_t mlen, mcap;
	int soft, non_acgt;
} file_result;

static void fmsg(file_result *r, int with_errno, const char *fmt, ...) {
	char line[4096];
	const int saved = errno;
	int k = snprintf(line, sizeof line, "%s: ", program_invocation_short_name);
	va_list ap;
	va_start(ap, fmt);
	k += vsnprintf(line + k, sizeof line - (size_t)k - 2, fmt, ap);
	va_end(ap);
	if (k > (int)sizeof line - 2) k = (int)sizeof line - 2;
	if (with_errno) k += snprintf(line + k, sizeof line - (size_t)k - 1, ": %s", strerror(saved));
	if (k > (int)sizeof line - 2) k = (int)sizeof line - 2;
	line[k++] = '\n';
	if (r->mlen + (size_t)k + 1 > r->mcap) {
		r->mcap = 2 * r->mcap + (size_t)k + 256;
		r->msgs = realloc(r->msgs, r->mcap);
		if (!r->msgs) err(errno, "Out of memory");
	}
	memcpy(r->msgs + r->mlen, line, (size_t)k);
	r->mlen += (size_t)k;
	r->msgs[r->mlen] = '\0';
}
#define file_soft_warnx(r, ...)                                                                    \
	do {                                                                                           \
		(r)->soft = 1;                                                                             \
		fmsg((r), 0, __VA_ARGS__);                                                                 \
	} while (0)

/* normalize, src/sequence.c:260-282: keep ACGT and '!', upper-case acgt, drop the rest (by table: a byte maps to itself,
 * to its upper case, or to 0 = dropped) */
static unsigned char norm_table[256];
static void norm_table_init(void) {
	const char *keep = "ACGT!";
	for (const char *k = keep; *k; k++) norm_table[(unsigned char)*k] = (unsigned char)*k;
	norm_table['a'] = 'A', norm_table['c'] = 'C', norm_table['g'] = 'G', norm_table['t'] = 'T';
}
static size_t normalize(char *s, size_t len, int *dropped) {
	char *w = s;
	int lost = 0;
	for (size_t i = 0; i < len; i++) {
		const unsigned char c = norm_table[(unsigned char)s[i]];
		*w = (char)c;
		w += c != 0;
		lost |= c == 0;
	}
	*w = '\0';
	if (lost) *dropped = 1;
	return (size_t)(w - s);
}

/* a reader thread's buffer, reused from file to file (read(), not a fresh allocation per file) */
typedef struct {
	char *buf;
	size_t cap;
} read_buffer;

static char *slurp(const char *file_name, size_t *len_out, read_buffer *rb) {
	const int fd = strcmp(file_name, "-") ? open(file_name, O_RDONLY) : STDIN_FILENO;
	if (fd < 0) return NULL;
	if (!rb->buf) rb->cap = (size_t)4 << 20, rb->buf = xmalloc(rb->cap + 1);
	size_t len = 0;
	int bad = 0;
	for (;;) {
		if (len == rb->cap) {
			rb->cap *= 2;
			rb->buf = realloc(rb->buf, rb->cap + 1);
			if (!rb->buf) err(errno, "Out of memory");
		}
		const ssize_t got = read(fd, rb->buf + len, rb->cap - len);
		if (got < 0) {
			if (errno == EINTR) continue;
			bad = 1;
			break;
		}
		if (got == 0) break;
		len += (size_t)got;
	}
	const int saved = errno;
	if (fd != STDIN_FILENO) close(fd);
	if (bad) {
		errno = saved;
		return NULL;
	}
	rb->buf[len] = '\0';
	*len_out = len;
	return rb->buf;
}

/* read_fasta, src/io.c:196-233: every record of the file becomes one sequence.  The record grammar and the
 * messages are those of the reference's parser (libs/pfasta.c:304-480): the file must start with '>'; the name is
 * the word behind it, the rest of the line a comment; the sequence is every following word of a line that starts
 * with a letter, '-' or '*', across blank lines and blanks inside lines, CR LF or LF; anything else must be the
 * next record's '>'.  A malformed record ends the file with a message (records read before it are kept). */
#define IS_SPACE(c) (((c) >= '\t' && (c) <= '\r') || (c) == ' ')
static void read_fasta(const char *file_name, file_result *res, read_buffer *rb) {
	genome_list *out = &res->seqs;
	size_t len = 0;
	char *text = slurp(file_name, &len, rb);
	if (!text) {
		res->soft = 1;
		fmsg(res, 1, "%s", file_name);
		return;
	}
	if (len == 0) {
		file_soft_warnx(res, "%s: File is empty.", file_name);
		return;
	}
	if (text[0] != '>') {
		file_soft_warnx(res, "%s: File must start with '>'.", file_name);
		return;
	}
	char *p = text, *end = text + len;
	size_t line = 1;
	while (p < end) {
		if (*p != '>') {
			file_soft_warnx(res, "%s: Expected '>' but found '%c' on line %zu.", file_name, *p, line);
			break;
		}
		/* name */
		char *h = ++p;
		while (p < end && !IS_SPACE(*p)) p++;
		if (p == end) {
			file_soft_warnx(res, "%s: Unexpected EOF in name on line %zu.", file_name, line);
			break;
		}
		if (p == h) {
			file_soft_warnx(res, "%s: Empty name on line %zu.", file_name, line);
			break;
		}
		char *name_end = p;
		/* comment: the rest of the line */
		p = memchr(p, '\n', (size_t)(end - p));
		if (!p) {
			file_soft_warnx(res, "%s: Unexpected EOF in comment on line %zu.", file_name, line);
			break;
		}
		/* sequence: first where it ends (the next line that starts with something else), then one copy of its words */
		while (p < end && IS_SPACE(*p)) line += *p++ == '\n';
		char *s0 = p;
		size_t n = 0;
		while (p < end && (isalpha((unsigned char)*p) || *p == '-' || *p == '*')) {
			char *w = p;
			while (p < end && !IS_SPACE(*p)) p++;
			n += (size_t)(p - w);
			while (p < end && IS_SPACE(*p)) line += *p++ == '\n';
		}
		if (n == 0) {
			file_soft_warnx(res, "%s: Empty sequence on line %zu.", file_name, line);
			break;
		}
		genome g;
		g.seq = xmalloc(n + 1);
		size_t k = 0;
		for (char *q = s0; q < p;) { /* the words again: copied, then normalised in place */
			char *w = q;
			while (q < p && !IS_SPACE(*q)) q++;
			memcpy(g.seq + k, w, (size_t)(q - w));
			k += (size_t)(q - w);
			while (q < p && IS_SPACE(*q)) q++;
		}
		g.name = strndup(h, (size_t)(name_end - h));
		if (!g.name) err(errno, "Out of memory");
		g.len = normalize(g.seq, n, &res->non_acgt);
		if (g.len + 4096 < n) { /* (much was dropped: give the memory back) */
			char *fit = realloc(g.seq, g.len + 1);
			if (fit) g.seq = fit;
		}
		push_genome(out, g);
	}
}

/* read_fasta_join + dsa_join, src/io.c:159-194, src/sequence.c:78-125: all records of
 * a file joined by '!', named after the file without directory and extension */
static void read_fasta_join(const char *file_name, file_result *res, read_buffer *rb) {
	file_result one = {0};
	read_fasta(file_name, &one, rb);
	res->msgs = one.msgs, res->mlen = one.mlen, res->mcap = one.mcap, res->soft = one.soft, res->non_acgt = one.non_acgt;
	genome_list single = one.seqs;
	if (single.n == 0) return;
	size_t total = 0;
	for (size_t i = 0; i < single.n; i++) total += single.v[i].len + 1;
	genome g;
	g.seq = xmalloc(total);
	char *w = g.seq;
	for (size_t i = 0; i < single.n; i++) {
		if (i) *w++ = '!';
		memcpy(w, single.v[i].seq, single.v[i].len);
		w += single.v[i].len;
	}
	*w = '\0';
	g.len = total - 1;
	const char *left = strrchr(file_name, '/');
	left = left ? left + 1 : file_name;
	const char *dot = strchrnul(left, '.');
	g.name = strndup(left, (size_t)(dot - left));
	if (!g.name) err(errno, "Out of memory");
	push_genome(&res->seqs, g);
	for (size_t i = 0; i < single.n; i++) {
		free(single.v[i].name);
		free(single.v[i].seq);
	}
	free(single.v);
}

/* the input files, read by up to `threads` threads (each takes the next unread file); results in command-line order */
typedef struct {
	char **files;
	size_t nfiles;
	int join;
	file_result *results;
	size_t next; /* atomic */
} read_job;

static void *read_worker(void *arg) {
	read_job *job = arg;
	read_buffer rb = {0};
	for (;;) {
		const size_t i = __atomic_fetch_add(&job->next, 1, __ATOMIC_RELAXED);
		if (i >= job->nfiles) break;
		if (job->join) read_fasta_join(job->files[i], &job->results[i], &rb);
		else read_fasta(job->files[i], &job->results[i], &rb);
	}
	free(rb.buf);
	return NULL;
}

static void read_all_files(char **files, size_t nfiles, int join, int threads, genome_list *all) {
	norm_table_init();
	read_job job = {files, nfiles, join, calloc(nfiles ? nfiles : 1, sizeof(file_result)), 0};
	if (!job.results) err(errno, "Out of memory");
	size_t nt = threads > 0 ? (size_t)threads : 1;
	if (nt > nfiles) nt = nfiles;
	if (nt > 64) nt = 64; /* (the files come from one file system: more readers do not make it faster) */
	pthread_t *tid = xmalloc(nt * sizeof *tid);
	size_t started = 0;
	for (size_t t = 1; t < nt; t++)
		if (pthread_create(&tid[started], NULL, read_worker, &job) == 0) started++;
	read_worker(&job);
	for (size_t t = 0; t < started; t++) pthread_join(tid[t], NULL);
	free(tid);
	for (size_t i = 0; i < nfiles; i++) {
		file_result *r = &job.results[i];
		if (r->msgs) fputs(r->msgs, stderr);
		free(r->msgs);
		soft_error |= r->soft;
		saw_non_acgt |= r->non_acgt;
		for (size_t k = 0; k < r->seqs.n; k++) push_genome(all, r->seqs.v[k]);
		free(r->seqs.v);
	}
	free(job.results);
}

/* file names, as the command line and the files of file names give them */
typedef struct {
	char **v;
	size_t n, cap;
} name_list;

static void push_name(name_list *l, const char *name) {
	if (l->n == l->cap) {
		l->cap = l->cap ? l->cap * 2 : 16;
		l->v = realloc(l->v, l->cap * sizeof *l->v);
		if (!l->v) err(errno, "Out of memory");
	}
	l->v[l->n++] = strdup(name);
}

/* read_into_string_vector, src/io.c:103-144 */
static void read_file_of_filenames(const char *file_name, name_list *names) {
	FILE *f = strcmp(file_name, "-") ? fopen(file_name, "r") : stdin;
	if (!f) {
		soft_error = 1;
		warn("%s", file_name);
		return;
	}
	char *line = NULL;
	size_t bufsz = 0;
	while (getline(&line, &bufsz, f) != -1) {
		char *nl = strchr(line, '\n');
		if (nl) *nl = '\0';
		if (*line) push_name(names, line);
	}
	free(line);
	if (f != stdin) fclose(f);
}

static void usage(int status) {
	static const char str[] =
		"Usage: andi-hip [OPTIONS...] FILES...\n"
		"\tFILES... can be any sequence of FASTA files.\n"
		"\tUse '-' as file name to read from stdin.\n"
		"Options:\n"
		"  -b, --bootstrap=INT  Print additional bootstrap matrices\n"
		"      --file-of-filenames=FILE  Read additional filenames from FILE; one per line\n"
		"  -j, --join           Treat all sequences from one file as a single genome\n"
		"  -l, --low-memory     Use less memory at the cost of speed\n"
		"  -m, --model=MODEL    Pick an evolutionary model of 'Raw', 'JC', 'Kimura', 'LogDet', 'ANI'; "
		"default: JC\n"
		"  -p FLOAT             Significance of an anchor; default: 0.025\n"
		"      --progress=WHEN  Print a progress bar 'always', 'never', or 'auto'; default: auto\n"
		"      --reference=FILE  Compare FILES... against the sequences of FILE only (repeatable); prints one row\n"
		"                       per query, one column per reference\n"
		"      --reference-list=FILE  Read reference filenames from FILE; one per line\n"
		"      --backbone=FILE  With --reference and --place: the tree of the references, as --tree wrote it for exactly\n"
		"                       these references (Newick, unrooted, binary; support labels are ignored)\n"
		"      --place=FILE     With --reference and --backbone: write to FILE (jplace) where on the backbone tree each\n"
		"                       query sits -- the branch, the point on it and the length of the query's own branch that\n"
		"                       fit its distances to the references best (least squares)\n"
		"      --place-method=METHOD  Weigh the squared errors with 'fm' (1/d^2, Fitch-Margoliash) or 'ols' (all alike);\n"
		"                       default: fm\n"
		"      --screen=K       With --reference or --reference-list: sketch every sequence first (k-mer hashes, on the GPU)\n"
		"                       and compare each query only with its K references that share the most hashes with it\n"
		"      --screen-kmer=INT  The k-mer length of the sketches, 4 to 32; default: 21 (sourmash's default)\n"
		"      --screen-scale=INT  Keep one hash in INT (a hash h is kept iff h <= (2^64 - 1) / INT); default: 1000\n"
		"                       (sourmash's default)\n"
		"      --screen-min=INT  A reference must share at least INT hashes with a query to be taken; default: 1\n"
		"      --screen-report=FILE  Write every (query, reference) pair that shares a hash to FILE, tab-separated: the\n"
		"                       counts, the sketch sizes, the containment of the query and whether the reference was kept\n"
		"  -t, --threads=INT    Set the number of host threads; by default, all processors are used\n"
		"      --tree=FILE      Write a neighbor-joining tree of each printed matrix to FILE (Newick, one line per\n"
		"                       matrix)\n"
		"      --support=FILE   With -b: write the tree of the first matrix to FILE, each inner branch labelled with the\n"
		"                       number of bootstrap matrices whose tree has that branch\n"
		"      --consensus=FILE With -b: write the majority-rule consensus tree of the bootstrap matrices' trees to FILE,\n"
		"                       each inner branch labelled with the number of those trees that have it\n"
		"      --transfer=FILE  With -b: write the tree of the first matrix to FILE, each inner branch labelled with its\n"
		"                       transfer bootstrap expectation (TBE, between 0 and 1) over the bootstrap matrices' trees\n"
		"      --rogues=FILE    With -b: write one line per sequence to FILE: in how many pairs of a branch of the first\n"
		"                       matrix's tree and the nearest branch of a bootstrap matrix's tree the sequence is one of\n"
		"                       those that have to move (its transfer score), and that number per counted pair\n"
		"      --rogue-cutoff=X With --rogues: count a pair of branches up to the transfer distance X * (depth - 1), with\n"
		"                       X from 0 to 1; default: 0.3\n"
		"      --trees-only     With -b and at least one of --tree, --support, --consensus, --transfer: do not print the\n"
		"                       bootstrap matrices; their trees are drawn, estimated and joined on the GPU, for any number\n"
		"                       of replicates.  These trees come from the portable estimator (its own logarithm, within\n"
		"                       an ulp of the C library's); in a rare tie they can differ from those of a run that\n"
		"                       prints the matrices\n"
		"      --tree-method=M  Build the trees of --tree, --support, --consensus, --transfer and --rogues by 'nj'\n"
		"                       (neighbor-joining) or 'bionj' (BIONJ, Gascuel 1997); default: nj\n"
		"      --complete       Before a tree is joined (--tree, --support, --consensus, --transfer, --rogues): estimate every\n"
		"                       distance that is missing ('nan') from the known distances around it -- the least of\n"
		"                       max(d(i,k) + d(j,l), d(i,l) + d(j,k)) - d(k,l) over the pairs k, l whose five distances are\n"
		"                       known (the four-point condition), on the GPU.  The printed matrices are not changed\n"
		"      --complete-report=FILE  Implies --complete: write one line per missing distance of the first matrix to\n"
		"                       FILE, tab-separated: the two names, the estimate, the round that found it and the number\n"
		"                       of quartets it is the least of ('nan', 0, 0: it could not be derived)\n"
		"      --delta=FILE     Write the tree-likeness score of every genome to FILE, tab-separated: its name, its mean delta\n"
		"                       over all quartets of genomes that contain it (Holland et al. 2002: 0 where the distances fit\n"
		"                       a tree, towards 1 where they do not) and the number of those quartets; on the GPU, from the\n"
		"                       first matrix as it is printed (--complete does not change it)\n"
		"      --root=METHOD    Write every tree of --tree, --support and --transfer rooted: by 'mad' (minimal ancestor deviation,\n"
		"                       Tria et al. 2017: the point whose distances to the leaves disagree least with a clock, over all\n"
		"                       leaf pairs) or at the 'midpoint' of the longest path; on the GPU, each tree with its own root.\n"
		"                       Support and TBE labels stay with their branches.  The consensus tree is not rooted, and a\n"
		"                       rooted file is no --backbone: that goes on requiring an unrooted tree\n"
		"      --root-report=FILE  With --root: write the root of the first matrix's tree to FILE, tab-separated: the method,\n"
		"                       the branch (its jplace edge number), the distance from the branch's lower end, the branch's\n"
		"                       length, the score sqrt(SS / pairs), the root ambiguity index and the number of leaf pairs used\n"
		"                       ('nan' for score and ambiguity under midpoint)\n"
		"      --lengths=KIND   The branch lengths of every tree of --tree, --support and --transfer: 'joined' (as the joining\n"
		"                       gives them; the default) or 'ols': refit to the tree's own matrix by ordinary least squares on\n"
		"                       the GPU (as FastME's OLS lengths; negative lengths are kept), before --root roots the tree.\n"
		"                       The consensus tree, placements and clusters are not touched; not together with --trees-only\n"
		"      --fit=FILE       Write how well the first matrix's tree explains its distances to FILE, tab-separated: the\n"
		"                       residual sum of squares and R^2 under least-squares and under the joined lengths, the trees'\n"
		"                       lengths and negative branches, the worst-fitted pair; then every genome's share of the two\n"
		"                       sums of squares.  Works without --tree; after --complete, if given\n"
		"      --refine=METHOD  Refine every joined tree of --tree, --support, --consensus, --transfer and --rogues against its own\n"
		"                       matrix right after the join: 'none' (the default) or 'bnni', balanced nearest-neighbor\n"
		"                       interchanges on the GPU until none shortens the tree (as FastME's BNNI); the tree then carries\n"
		"                       its balanced (BME) lengths, which --lengths, --root and --fit start from; not together with\n"
		"                       --trees-only\n"
		"      --refine-moves=MOVES  With --refine=bnni: the moves of the search, 'nni' (the default), interchanges across one\n"
		"                       branch, or 'spr', balanced subtree pruning and regrafting: a round re-hangs one subtree on any\n"
		"                       other branch (as FastME's SPR), which leaves the local optima of interchanges\n"
		"      --refine-tol=X   With --refine: an interchange is made only if it shortens the tree by more than X, in the units\n"
		"                       of the printed matrix; default: 1e-9\n"
		"      --refine-report=FILE  With --refine: write the refinement of the first matrix's tree to FILE, tab-separated: the\n"
		"                       method, the interchanges made, whether the search converged, the tree's length before and\n"
		"                       after, the joined tree's inner branches that the refined tree lacks; then every interchange:\n"
		"                       its gain and the first genome of each of the two subtrees it swapped\n"
		"      --linkage=METHOD Cluster with 'single', 'complete' or 'average' linkage; default: average (UPGMA)\n"
		"      --dendrogram=FILE  Write the linkage tree of each printed matrix to FILE (Newick, rooted, one line per\n"
		"                       matrix); a pair without a distance counts as farther apart than any other\n"
		"      --clusters=FILE  With --threshold: write the clusters of the first matrix to FILE, one line per sequence:\n"
		"                       name, cluster, the cluster's representative (its medoid) and, with -b, the number of\n"
		"                       bootstrap matrices whose clustering has exactly this cluster\n"
		"      --threshold=T    The distance up to which --clusters joins, in the units of the printed matrix\n"
		"      --truncate-names Truncate names to ten characters\n"
		"  -v, --verbose        Prints additional information\n"
		"  -h, --help           Display this help and exit\n"
		"      --version        Output version information and acknowledgments\n";
	fputs(str, status == EXIT_SUCCESS ? stdout : stderr);
	exit(status);
}

static void version(void) {
	printf("andi-hip " PROGRAM_VERSION " (command-line interface of andi 1.15)\n"
		   "Anchor distances on AMD MI355X through libandihip (ABI %d).\n\n"
		   "Acknowledgments:\n"
		   "1) Method: Haubold, B. Kl\xc3\xb6tzl, F. and Pfaffelhuber, P. (2015). Fast and accurate estimation of "
		   "evolutionary distances between closely related genomes, Bioinformatics.\n"
		   "2) Bootstrapping: Kl\xc3\xb6tzl, F. and Haubold, B. (2016). Support Values for Genome Phylogenies, "
		   "Life 6.1.\n",
		   andi_hip_abi_version());
	exit(EXIT_SUCCESS);
}

static size_t progress_n = 0;
static void progress_cb(size_t done, size_t total, void *ud) {
	(void)ud; /* src/dist_hack.h:74-87 */
	fprintf(stderr, "\rComparing %zu sequences: %5.1f%% (%zu/%zu)", progress_n,
			total ? 100.0 * (double)done / (double)total : 100.0, done, total);
}

static const char **name_array(const genome *g, size_t n) {
	const char **names = xmalloc(n * sizeof *names);
	for (size_t i = 0; i < n; i++) names[i] = g[i].name;
	return names;
}

/* The square matrix M of the nr sequences rn (qn == NULL), or the query-versus-reference table (--reference) of the two
 * cross blocks M and MQR: one row per query qn, one column per reference rn.  To stdout, the warnings as soft warnings. */
static void print_distances(const andi_hip_model *M, const andi_hip_model *MQR, const char **rn, size_t nr, const char **qn, size_t nq,
							int model, int vv, int truncate, int warnings) {
	/* the warnings' buffer grows on demand (a line per pair at worst -- n^2 x 512 bytes up front would be 4.9 GB for
	 * BASELINE's 3085 genomes): a buffer that came back full is doubled and the call repeated */
	size_t cap = 64 + (qn ? nq : nr) * (300 + 16 * nr), wcap = (size_t)1 << 16;
	for (size_t i = 0; qn && i < nr; i++) cap += strlen(rn[i]) + 1;
	char *out = xmalloc(cap), *wbuf = xmalloc(wcap);
	int flags = 0;
	for (;;) {
		const size_t need = qn ? andi_hip_format_distances_rect(M, MQR, rn, nr, qn, nq, model, vv, truncate, warnings, out, cap, wbuf, wcap, &flags)
							   : andi_hip_format_distances(M, rn, nr, model, vv, truncate, warnings, out, cap, wbuf, wcap, &flags);
		const int out_short = need >= cap, warn_short = strlen(wbuf) + 1 >= wcap; /* (long names: the call says how much it needs) */
		if (!out_short && !warn_short) break;
		if (out_short) free(out), cap = need + 1, out = xmalloc(cap);
		if (warn_short) free(wbuf), wcap *= 4, wbuf = xmalloc(wcap);
	}
	for (char *line = strtok(wbuf, "\n"); line; line = strtok(NULL, "\n")) soft_warnx("%s", line);
	fputs(out, stdout);
	free(out);
	free(wbuf);
}

/* The four files of trees.  Each is refused under --reference / --reference-list, and all but --tree without bootstrap
 * matrices; main parses, refuses, opens and closes them in this order. */
enum { OUT_TREE, OUT_SUPPORT, OUT_CONSENSUS, OUT_TRANSFER, OUT_COUNT };
typedef struct {
	const char *option, *with_reference, *without_bootstrap; /* the long option and its two refusals (NULL: none) */
	const char *path;
	FILE *f;
} tree_file;
#define WITH_REFERENCE " not available together with --reference or --reference-list."
#define NEEDS_B " bootstrap matrices: give -b N with N of at least 2."
static tree_file outs[OUT_COUNT] = {
	{"tree", "A tree (--tree) is" WITH_REFERENCE, NULL, NULL, NULL},
	{"support", "Support values (--support) are" WITH_REFERENCE, "Support values (--support) need" NEEDS_B, NULL, NULL},
	{"consensus", "A consensus tree (--consensus) is" WITH_REFERENCE, "A consensus tree (--consensus) needs" NEEDS_B, NULL, NULL},
	{"transfer", "Transfer support (--transfer) is" WITH_REFERENCE, "Transfer support (--transfer) needs" NEEDS_B, NULL, NULL},
};

/* --rogues: the table of the genomes' transfer scores; not one of the four files of trees, but written from the same state */
typedef struct {
	const char *path, *cutoff_arg;
	FILE *f;
	double cutoff;
} rogue_out;

/* what one Newick line is made of: the consensus tree's nodes; or the records J with the transfer bootstrap expectation
 * (depth, transfer, used) or the support values (NULL: none) as inner labels */
typedef struct {
	const andi_hip_nj_join *J;
	const uint32_t *support;
	const uint32_t *depth;
	const uint64_t *transfer;
	size_t used;
	const andi_hip_cons_node *nodes;
	size_t ninner;
	andi_hip_ctx *ctx; /* --root, --lengths: the context the tree is rooted and refit on */
	int point;         /* --root-report: this is the point estimate's tree */
	const double *D;   /* --lengths=ols: the n x n matrix J was joined from (NULL: the lengths stay) */
} newick_src;

/* --lengths=ols: every line of records J that comes with its matrix is written with the least-squares lengths of that
 * matrix (andi_hip_fit, andi_hip_relength), before it is rooted; the consensus tree has no records and is not. */
static int lengths_ols;

/* The records of w with the refit lengths, or NULL (and a soft warning) if the fit failed. */
static andi_hip_nj_join *refit_records(const newick_src *w, size_t n) {
	double *len = xmalloc((2 * n - 3) * sizeof *len);
	andi_hip_nj_join *out = xmalloc((n - 2) * sizeof *out);
	andi_hip_fit_result r;
	if (andi_hip_fit(w->ctx, w->J, n, w->D, ANDI_FIT_OLS, len, &r, NULL, NULL)) {
		soft_warnx("A tree is written with its joined lengths: %s", andi_hip_last_error(w->ctx));
		free(out), out = NULL;
	} else if (andi_hip_relength(w->J, n, len, out)) {
		soft_warnx("A tree is written with its joined lengths: its records are malformed.");
		free(out), out = NULL;
	}
	free(len);
	return out;
}

/* --root: every line of records J is written rooted (andi_hip_root, andi_hip_format_newick_rooted), with the labels that
 * belong to its branches moved with them; the consensus tree is not.  --root-report: the point estimate's root. */
typedef struct {
	int on, method, reported;
	const char *report_path;
	FILE *rf;
} root_opts;
static root_opts rootopt;

static size_t format_newick(const newick_src *w, const char **names, size_t n, int truncate, char *text, size_t cap) {
	if (w->nodes) return andi_hip_format_newick_consensus(w->nodes, n, w->ninner, names, truncate, text, cap);
	if (w->depth) return andi_hip_format_newick_transfer(w->J, w->depth, w->transfer, w->used, n, names, truncate, text, cap);
	return andi_hip_format_newick_support(w->J, w->support, n, names, truncate, text, cap);
}

/* The line of format_newick rooted, or NULL (and a soft warning) if the tree could not be rooted: the labels are the
 * strings format_newick prints behind the pair records' nodes.  The point estimate's root goes to --root-report, once. */
static char *rooted_newick(const newick_src *w, const char **names, size_t n, int truncate) {
	andi_hip_root_result r;
	if (andi_hip_root(w->ctx, w->J, n, rootopt.method, &r, NULL, NULL)) {
		soft_warnx("A tree is written without a root: %s", andi_hip_last_error(w->ctx));
		return NULL;
	}
	if (w->point && rootopt.rf && !rootopt.reported++) {
		double len = 0.0;
		for (size_t s = 0; s + 2 < n; s++) {
			if (w->J[s].a == r.edge) len = w->J[s].la;
			if (w->J[s].b == r.edge) len = w->J[s].lb;
			if (s + 3 == n && w->J[s].c == r.edge) len = w->J[s].lc;
		}
		const int mad = rootopt.method == ANDI_ROOT_MAD;
		double score = mad ? sqrt(r.ss / (double)r.pairs) : NAN, ambiguity = mad ? sqrt(r.ss / r.ss_second) : NAN;
		if (isnan(score)) score = NAN; /* (0 / 0 carries a sign that would be printed) */
		if (isnan(ambiguity)) ambiguity = NAN;
		fprintf(rootopt.rf, "%s\t%d\t%.8g\t%.8g\t%.8g\t%.8g\t%llu\n", mad ? "mad" : "midpoint", (int)r.edge, r.distal, len, score,
				ambiguity, (unsigned long long)r.pairs);
		if (ferror(rootopt.rf)) err(1, "%s", rootopt.report_path);
	}
	const size_t nlab = n - 3;
	char (*buf)[32] = NULL;
	const char **labels = NULL;
	if (nlab && (w->support || w->depth)) {
		buf = xmalloc(nlab * sizeof *buf), labels = xmalloc(nlab * sizeof *labels);
		for (size_t s = 0; s < nlab; s++) {
			if (w->support) snprintf(buf[s], sizeof buf[s], "%u", (unsigned)w->support[s]);
			else snprintf(buf[s], sizeof buf[s], "%.6g", 1.0 - (double)w->transfer[s] / ((double)w->used * (double)(w->depth[s] - 1)));
			labels[s] = buf[s];
		}
	}
	size_t cap = 96 + n * (labels ? 92 : 44);
	for (size_t i = 0; i < n; i++) cap += strlen(names[i]) * 2 + 2;
	char *text = xmalloc(cap);
	const size_t need = andi_hip_format_newick_rooted(w->J, n, names, truncate, r.edge, r.distal, labels, text, cap);
	if (need >= cap)
		free(text), cap = need + 1, text = xmalloc(cap), andi_hip_format_newick_rooted(w->J, n, names, truncate, r.edge, r.distal, labels, text, cap);
	free(buf), free(labels);
	return text;
}

/* one Newick line to the file o */
static void put_newick(const tree_file *o, const newick_src *given, const char **names, size_t n, int truncate) {
	newick_src src = *given;
	const newick_src *w = &src;
	andi_hip_nj_join *refit = NULL;
	if (lengths_ols && src.J && src.D && src.ctx && n >= 3 && (refit = refit_records(given, n))) src.J = refit;
	size_t cap = 64 + n * (w->nodes ? 80 : w->depth ? 60 : 52);
	for (size_t i = 0; i < n; i++) cap += strlen(names[i]);
	char *text = xmalloc(cap);
	const size_t need = format_newick(w, names, n, truncate, text, cap);
	if (need >= cap) free(text), cap = need + 1, text = xmalloc(cap), format_newick(w, names, n, truncate, text, cap);
	if (rootopt.on && need && w->J && w->ctx && n >= 3) { /* (a text that is refused stays refused; two leaves have no root to find) */
		char *rooted = rooted_newick(w, names, n, truncate);
		if (rooted) free(text), text = rooted;
	}
	if (fputs(text, o->f) == EOF) err(1, "%s", o->path);
	free(text), free(refit);
}

/* --complete: every matrix that goes into a joined tree has its missing distances estimated from quartets first
 * (andi_hip_complete), in place; what the run prints is not touched.  --complete-report: the point estimate's missing pairs. */
typedef struct {
	int on;
	const char *report_path;
	FILE *rf;
} complete_opts;
static complete_opts cmpl;
#define NOT_FINITE (cmpl.on ? " is not finite and could not be derived." : " is not finite.")

/* the one warning of a matrix that received fills; k: the matrix as the run counts them (1 = the point estimate) */
static void complete_warn(unsigned long k, size_t missing, size_t left) {
	static int said_1; /* (--tree and --support both complete the point estimate) */
	if (k == 1 && said_1++) return;
	if (missing > left)
		soft_warnx("Matrix %lu: %zu of %zu missing distances were derived from quartets (--complete).", k, missing - left, missing);
}

/* the K-th matrix D completed in place; 0, or 1 with the context's error set */
static int complete_one(andi_hip_ctx *ctx, double *D, size_t n, unsigned long k) {
	size_t missing = 0, left = 0;
	if (andi_hip_complete(ctx, D, n, 0, D, NULL, 0, &missing, &left)) return 1;
	complete_warn(k, missing, left);
	return 0;
}

/* --tree-method: the builder of every joined tree.  Neighbor-joining goes through the calls it always went through, so a
 * run without the option says of a failure what it always said (the context's error names the function called). */
static int join_one(andi_hip_ctx *ctx, const double *D, size_t n, int method, andi_hip_nj_join *J) {
	return method == ANDI_TREE_NJ ? andi_hip_nj(ctx, D, n, J) : andi_hip_tree(ctx, D, n, method, J);
}

static int join_batch(andi_hip_ctx *ctx, const double *D, size_t n, size_t count, int method, andi_hip_nj_join *J, int64_t *bad) {
	return method == ANDI_TREE_NJ ? andi_hip_nj_batch(ctx, D, n, count, J, bad) : andi_hip_tree_batch(ctx, D, n, count, method, J, bad);
}

static int join_bootstrap(andi_hip_ctx *ctx, const andi_hip_model *M, size_t n, int model, int method, uint64_t seed, size_t first,
						  size_t count, andi_hip_nj_join *J, int64_t *bad) {
	return method == ANDI_TREE_NJ ? andi_hip_bootstrap_nj(ctx, M, n, model, seed, first, count, J, bad, NULL)
								  : andi_hip_bootstrap_tree(ctx, M, n, model, method, seed, first, count, J, bad, NULL);
}

/* --refine=bnni: every joined tree is refined against the matrix it was joined from (andi_hip_refine) right after the join,
 * so every file of trees sees the refined records, with their balanced lengths.  --refine-report: the point estimate's. */
typedef struct {
	int on, reported, spr;
	double tol;
	const char *tol_arg, *report_path, *moves_arg;
	FILE *rf;
} refine_opts;
static refine_opts refopt = {.tol = 1e-9};

static size_t set_words; /* (for cmp_sets) */
static int cmp_sets(const void *a, const void *b) {
	const uint64_t *x = a, *y = b;
	for (size_t w = 0; w < set_words; w++)
		if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
	return 0;
}

/* the leaf sets of the n - 3 pair records, each on its side without leaf 0, sorted */
static uint64_t *sorted_sets(const andi_hip_nj_join *J, size_t n) {
	const size_t W = (n + 63) / 64, nsets = n - 3;
	uint64_t *sets = xmalloc((nsets ? nsets : 1) * W * sizeof *sets);
	memset(sets, 0, (nsets ? nsets : 1) * W * sizeof *sets);
	for (size_t s = 0; s < nsets; s++) {
		const int32_t ch[2] = {J[s].a, J[s].b};
		for (int k = 0; k < 2; k++) {
			if ((size_t)ch[k] < n) sets[s * W + (size_t)ch[k] / 64] |= (uint64_t)1 << (ch[k] % 64);
			else
				for (size_t w = 0; w < W; w++) sets[s * W + w] |= sets[((size_t)ch[k] - n) * W + w];
		}
	}
	for (size_t s = 0; s < nsets; s++) {
		if (!(sets[s * W] & 1)) continue;
		for (size_t w = 0; w < W; w++) sets[s * W + w] = ~sets[s * W + w];
		if (n % 64) sets[s * W + W - 1] &= ((uint64_t)1 << (n % 64)) - 1;
	}
	set_words = W;
	qsort(sets, nsets, W * sizeof *sets, cmp_sets);
	return sets;
}

/* the inner branches of the tree `before` that the tree `after` lacks */
static size_t changed_branches(const andi_hip_nj_join *before, const andi_hip_nj_join *after, size_t n) {
	const size_t W = (n + 63) / 64, nsets = n - 3;
	uint64_t *x = sorted_sets(before, n), *y = sorted_sets(after, n);
	size_t changed = 0;
	for (size_t s = 0; s < nsets; s++) changed += !bsearch(x + s * W, y, nsets, W * sizeof *y, cmp_sets);
	free(x), free(y);
	return changed;
}

/* The records J of the K-th matrix D (1 = the point estimate) refined in place.  A tree that cannot be refined stays as it
 * was joined, with a soft warning; one whose search ends at the cap of 10 n interchanges is kept as it stands, with one.
 * --refine-moves=spr: the same through andi_hip_refine_spr, whose log has the hops of every move beside. */
static void refine_joined(andi_hip_ctx *ctx, andi_hip_nj_join *J, size_t n, const double *D, unsigned long k, const char **names,
						  int truncate) {
	if (!refopt.on || n < 3) return;
	const int report = k == 1 && refopt.rf && !refopt.reported;
	const size_t cap = 10 * n;
	andi_hip_nj_join *out = xmalloc((n - 2) * sizeof *out);
	andi_hip_refine_move *log = report && !refopt.spr ? xmalloc(cap * sizeof *log) : NULL;
	andi_hip_spr_move *slog = report && refopt.spr ? xmalloc(cap * sizeof *slog) : NULL;
	andi_hip_refine_result r;
	if (refopt.spr ? andi_hip_refine_spr(ctx, J, n, D, refopt.tol, cap, out, &r, slog)
				   : andi_hip_refine(ctx, J, n, D, ANDI_REFINE_BNNI, refopt.tol, cap, out, &r, log)) {
		soft_warnx("The tree of matrix %lu is written unrefined: %s", k, andi_hip_last_error(ctx));
	} else {
		if (!r.converged)
			soft_warnx("The tree of matrix %lu is written as it stood after %zu interchanges: the refinement (--refine) did not converge.", k, cap);
		if (report) {
			FILE *f = refopt.rf;
			const int w = truncate ? 10 : -1; /* (as the matrix prints a name) */
			refopt.reported = 1;
			fputs("#method\tmoves\tconverged\tlength_before\tlength_after\tchanged\n", f);
			fprintf(f, "%s\t%llu\t%d\t%.8g\t%.8g\t%zu\n", refopt.spr ? "bspr" : "bnni", (unsigned long long)r.moves, (int)r.converged,
					r.length_before, r.length_after, changed_branches(J, out, n));
			fputs(refopt.spr ? "#move\tgain\tfirst\tsecond\thops\n" : "#move\tgain\tfirst\tsecond\n", f);
			for (size_t m = 0; m < r.moves; m++)
				if (refopt.spr)
					fprintf(f, "%zu\t%.8g\t%.*s\t%.*s\t%d\n", m + 1, slog[m].gain, w, names[slog[m].first], w, names[slog[m].second],
							(int)slog[m].hops);
				else fprintf(f, "%zu\t%.8g\t%.*s\t%.*s\n", m + 1, log[m].gain, w, names[log[m].first], w, names[log[m].second]);
			if (ferror(f)) err(1, "%s", refopt.report_path);
		}
		memcpy(J, out, (n - 2) * sizeof *out);
	}
	free(out), free(log), free(slog);
}

/* --tree: the tree (neighbor-joining, or --tree-method's) of the K-th printed matrix (1 = the point estimate) as one Newick
 * line, from the averaged distances whatever -vv asks the matrix to print */
typedef struct {
	const tree_file *o;
	int method;        /* ANDI_TREE_* */
	andi_hip_ctx *ctx; /* one for all trees, on opts.device */
	int device_for_ctx;
	int failed;        /* it could not be created: said once */
} tree_out;

/* --complete-report: the missing pairs of the point estimate, one line each in row-major order, from a completion of its
 * own (on the context of --tree, made here if this comes first) */
static void complete_report(tree_out *t, const andi_hip_model *M, const char **names, size_t n, int model, int truncate) {
	char msg[512];
	if (!t->failed && !t->ctx && andi_hip_ctx_create(&t->ctx, t->device_for_ctx, msg, sizeof msg)) {
		t->failed = 1, t->ctx = NULL;
		soft_warnx("No trees: %s", msg);
	}
	if (t->failed) return;
	double *D = malloc(n * n * sizeof *D);
	if (!D || andi_hip_distances(M, n, model, D)) err(errno, "Could not allocate enough memory for the report of derived distances.");
	size_t cap = 0, missing = 0, left = 0;
	for (size_t i = 0; i < n; i++)
		for (size_t j = i + 1; j < n; j++) cap += !isfinite(D[i * n + j]);
	andi_hip_fill *fills = malloc((cap ? cap : 1) * sizeof *fills);
	if (!fills) err(errno, "Could not allocate enough memory for the report of derived distances.");
	if (andi_hip_complete(t->ctx, D, n, 0, D, fills, cap, &missing, &left)) {
		soft_warnx("No report of derived distances: %s", andi_hip_last_error(t->ctx));
	} else {
		fprintf(cmpl.rf, "#first\tsecond\tdistance\tround\tquartets\n");
		for (size_t x = 0; x < missing && x < cap; x++) {
			const andi_hip_fill *f = &fills[x];
			const int w = truncate ? 10 : -1; /* (as the matrix prints a name) */
			fprintf(cmpl.rf, "%.*s\t%.*s\t", w, names[f->i], w, names[f->j]);
			if (f->round) fprintf(cmpl.rf, "%.8g\t%u\t%llu\n", f->value, f->round, (unsigned long long)f->quartets);
			else fprintf(cmpl.rf, "nan\t0\t0\n");
		}
		if (ferror(cmpl.rf)) err(1, "%s", cmpl.report_path);
	}
	free(D), free(fills);
}

/* --delta: the tree-likeness score of every genome of the point estimate (andi_hip_delta_scores), from the distances as
 * they are printed -- a pair without a distance takes its quartets out, whatever --complete derives for it (a derived
 * distance satisfies the four-point condition by construction).  On the context of --tree, made here if this comes first. */
typedef struct {
	const char *path;
	FILE *f;
} delta_opts;
static delta_opts dlt;

static void delta_report(tree_out *t, const andi_hip_model *M, const char **names, size_t n, int model, int truncate) {
	char msg[512];
	if (n <= 16384 && !t->failed && !t->ctx && andi_hip_ctx_create(&t->ctx, t->device_for_ctx, msg, sizeof msg)) {
		t->failed = 1, t->ctx = NULL;
		if (t->o->f) soft_warnx("No trees: %s", msg); /* (write_tree says nothing more) */
	}
	const int was = soft_error; /* the scores are an extra: without them the run ends as it would have */
	if (n > 16384) {
		soft_warnx("No tree-likeness scores (--delta): they are limited to 16384 sequences (%zu given).", n);
		soft_error = was;
		return;
	}
	if (t->failed) {
		soft_warnx("No tree-likeness scores (--delta): there is no GPU context.");
		soft_error = was;
		return;
	}
	double *D = malloc(n * n * sizeof *D);
	andi_hip_delta *rec = malloc(n * sizeof *rec);
	if (!D || !rec || andi_hip_distances(M, n, model, D)) err(errno, "Could not allocate enough memory for the tree-likeness scores.");
	if (andi_hip_delta_scores(t->ctx, D, n, rec)) {
		soft_warnx("No tree-likeness scores (--delta): %s", andi_hip_last_error(t->ctx));
		soft_error = was;
	} else {
		unsigned __int128 sum = 0, quartets = 0;
		const double one = 16777216.0; /* 2^24: a quartet's delta is kept as floor(delta * 2^24) */
		fprintf(dlt.f, "#name\tdelta\tquartets\n");
		for (size_t i = 0; i < n; i++) {
			sum += rec[i].sum, quartets += rec[i].quartets;
			fprintf(dlt.f, "%.*s\t", truncate ? 10 : -1, names[i]); /* (as the matrix prints a name) */
			if (rec[i].quartets) fprintf(dlt.f, "%.6f", (double)((long double)rec[i].sum / ((long double)rec[i].quartets * one)));
			else fprintf(dlt.f, "nan");
			fprintf(dlt.f, "\t%llu\n", (unsigned long long)rec[i].quartets);
		}
		if (quartets) fprintf(dlt.f, "#mean\t%.6f", (double)((long double)sum / ((long double)quartets * one)));
		else fprintf(dlt.f, "#mean\tnan");
		fprintf(dlt.f, "\t%llu\n", (unsigned long long)(quartets / 4));
		if (ferror(dlt.f)) err(1, "%s", dlt.path);
	}
	free(D), free(rec);
}

/* --fit: how well the point estimate's tree explains its matrix (andi_hip_fit), from a tree of its own (--tree-method's),
 * joined from the matrix as --complete leaves it.  On the context of --tree, made here if this comes first. */
typedef struct {
	const char *path;
	FILE *f;
} fit_opts;
static fit_opts fitopt;

static void put_g(FILE *f, double x, char end) {
	if (isnan(x)) fprintf(f, "nan%c", end); /* (a NaN carries a sign that would be printed) */
	else fprintf(f, "%.8g%c", x, end);
}

static void fit_report(tree_out *t, const andi_hip_model *M, const genome *g, const char **names, size_t n, int model, int truncate) {
	char msg[512];
	if (!t->failed && !t->ctx && andi_hip_ctx_create(&t->ctx, t->device_for_ctx, msg, sizeof msg)) {
		t->failed = 1, t->ctx = NULL;
		soft_warnx("No trees: %s", msg);
	}
	if (t->failed) return;
	double *D = malloc(n * n * sizeof *D), *len = malloc((2 * n) * sizeof *len), *ss = malloc(2 * n * sizeof *ss);
	andi_hip_nj_join *J = malloc(n * sizeof *J);
	if (!D || !len || !ss || !J || andi_hip_distances(M, n, model, D)) err(errno, "Could not allocate enough memory for the fit report.");
	andi_hip_fit_result r;
	int ok = 1;
	if (cmpl.on && complete_one(t->ctx, D, n, 1)) {
		soft_warnx("No fit report: %s", andi_hip_last_error(t->ctx));
		ok = 0;
	}
	for (size_t i = 0; i < n && ok; i++)
		for (size_t j = i + 1; j < n; j++)
			if (!isfinite(D[i * n + j])) {
				soft_warnx("No fit report: the distance of '%s' and '%s'%s", g[i].name, g[j].name, NOT_FINITE);
				ok = 0;
				break;
			}
	if (ok && n < 3) {
		soft_warnx("No fit report: a tree of two sequences has one branch and nothing to fit.");
		ok = 0;
	}
	if (ok && join_one(t->ctx, D, n, t->method, J)) {
		soft_warnx("No fit report: %s", andi_hip_last_error(t->ctx));
		ok = 0;
	}
	if (ok) refine_joined(t->ctx, J, n, D, 1, names, truncate);
	if (ok && andi_hip_fit(t->ctx, J, n, D, ANDI_FIT_OLS, len, &r, ss, ss + n)) {
		soft_warnx("No fit report: %s", andi_hip_last_error(t->ctx));
		ok = 0;
	}
	if (ok) {
		const int w = truncate ? 10 : -1; /* (as the matrix prints a name) */
		FILE *f = fitopt.f;
		fputs("#method\tpairs\trss\trss_joined\ttss\tr2\tr2_joined\tlength\tlength_joined\tnegative\tnegative_joined\tworst_first\t"
			  "worst_second\tworst_residual\n", f);
		fprintf(f, "ols\t%llu\t", (unsigned long long)r.pairs);
		put_g(f, r.rss, '\t'), put_g(f, r.rss_joined, '\t'), put_g(f, r.tss, '\t');
		put_g(f, r.tss == 0 ? NAN : 1.0 - r.rss / r.tss, '\t'), put_g(f, r.tss == 0 ? NAN : 1.0 - r.rss_joined / r.tss, '\t');
		put_g(f, r.length, '\t'), put_g(f, r.length_joined, '\t');
		fprintf(f, "%u\t%u\t", (unsigned)r.negative, (unsigned)r.negative_joined);
		if (r.worst_b >= 0) fprintf(f, "%.*s\t%.*s\t", w, names[r.worst_b], w, names[r.worst_c]);
		else fputs("-\t-\t", f);
		put_g(f, r.worst, '\n');
		fputs("#name\tss\tss_joined\n", f);
		for (size_t i = 0; i < n; i++) {
			fprintf(f, "%.*s\t", w, names[i]);
			put_g(f, ss[i], '\t'), put_g(f, ss[n + i], '\n');
		}
		if (ferror(f)) err(1, "%s", fitopt.path);
	}
	free(D), free(len), free(ss), free(J);
}

static void write_tree(tree_out *t, const andi_hip_model *M, const genome *g, const char **names, size_t n, int model, int truncate,
					   int k) {
	if (t->failed) return;
	char msg[512];
	if (!t->ctx && andi_hip_ctx_create(&t->ctx, t->device_for_ctx, msg, sizeof msg)) {
		t->failed = 1, t->ctx = NULL;
		soft_warnx("No trees: %s", msg);
		return;
	}
	double *D = malloc(n * n * sizeof *D);
	andi_hip_nj_join *J = malloc(n * sizeof *J);
	if (!D || !J || andi_hip_distances(M, n, model, D)) err(errno, "Could not allocate enough memory for the tree.");
	if (cmpl.on && complete_one(t->ctx, D, n, (unsigned long)k)) {
		soft_warnx("No tree for matrix %d: %s", k, andi_hip_last_error(t->ctx));
		free(D), free(J);
		return;
	}
	for (size_t i = 0; i < n; i++)
		for (size_t j = i + 1; j < n; j++)
			if (!isfinite(D[i * n + j])) {
				soft_warnx("No tree for matrix %d: the distance of '%s' and '%s'%s", k, g[i].name, g[j].name, NOT_FINITE);
				free(D), free(J);
				return;
			}
	if (join_one(t->ctx, D, n, t->method, J)) {
		soft_warnx("No tree for matrix %d: %s", k, andi_hip_last_error(t->ctx));
		free(D), free(J);
		return;
	}
	refine_joined(t->ctx, J, n, D, (unsigned long)k, names, truncate);
	put_newick(t->o, &(newick_src){.J = J, .ctx = t->ctx, .point = k == 1, .D = D}, names, n, truncate);
	free(D), free(J);
}

/* --support (f): the tree of the point estimate with, on every inner branch, the number of bootstrap matrices whose tree has
 * that branch.  The replicates' trees come from andi_hip_nj_batch, in chunks that bound the host's doubles; the counts
 * of the chunks add up.  With --tree, the replicates' lines of that file are written from the same records (bit for bit
 * those of andi_hip_nj, so the same text), in the same order.
 * --consensus (cf): the majority-rule consensus of the replicates' trees, from the same records -- the replicates are
 * joined once whichever of the four files are asked for; all chunks' records are kept (40 bytes each) and go through one
 * andi_hip_nj_splits call behind the loop.
 * --transfer (tf): the point estimate's tree again, labelled with the transfer bootstrap expectation: per chunk one
 * andi_hip_nj_transfer call next to the support count's, on the same records; the chunks' sums add up.
 * --rogues (rf): per chunk one andi_hip_nj_transfer_taxa call on the same records again; the chunks' counts add up.
 *
 * One state over the run: support_begin (the point estimate's tree), support_chunk for every chunk of replicates main
 * draws -- as matrices B, or, under --trees-only, as nothing: andi_hip_bootstrap_nj draws, estimates and joins them on the
 * device and the records are all that comes back -- and support_end (the files). */
typedef struct { /* what a run gives them */
	andi_hip_ctx *ctx;
	const genome *g;
	const char **names;
	size_t n;
	unsigned long replicates;
	int model, truncate, trees_only;
	uint64_t seed;
	const rogue_out *rogues;
	int method; /* ANDI_TREE_*: the builder of the point estimate's tree and of the replicates' */
} boot_run;

typedef struct {
	boot_run r;
	const tree_file *o; /* outs */
	size_t nrec, nsup, cap; /* cap: the replicates of one andi_hip_nj_batch / andi_hip_bootstrap_nj call, at most */
	unsigned long counted;
	double *D, *Dpoint; /* Dpoint: --lengths=ols: the point estimate's matrix, kept beside its tree */
	andi_hip_nj_join *J, *Rall;
	int64_t *bad;
	uint64_t *cmissing, *cleft; /* --complete: a chunk's counts of andi_hip_complete_batch */
	uint8_t *skipall;
	uint32_t *total, *part, *depth;
	uint64_t *ttotal, *tpart, *moved, *mpart, pairs;
	int point_ok, trans_ok, cons_ok, rogue_ok, stopped;
} support_state;

static void support_begin(support_state *s, const tree_file *o, const boot_run *r, const andi_hip_model *M) {
	memset(s, 0, sizeof *s);
	s->r = *r, s->o = o;
	FILE *f = o[OUT_SUPPORT].f, *cf = o[OUT_CONSENSUS].f, *tf = o[OUT_TRANSFER].f, *rf = r->rogues->f;
	const genome *g = r->g;
	const size_t n = r->n, replicates = r->replicates;
	const int trees_only = r->trees_only;
	const size_t nrec = s->nrec = n == 2 ? 1 : n - 2, nsup = s->nsup = n > 3 ? n - 3 : 1;
	/* at most 1 GiB at a time: of doubles, or -- the replicates never being matrices -- of the records kept on the host */
	size_t chunk = ((size_t)1 << 30) / (trees_only ? nrec * sizeof(andi_hip_nj_join) : n * n * sizeof(double));
	chunk = chunk < 1 ? 1 : chunk > replicates ? replicates : chunk;
	s->cap = chunk;
	const size_t kept = cf ? replicates : chunk; /* the replicates whose records and skip flags stay */
	double *D = s->D = malloc((trees_only ? 1 : chunk) * n * n * sizeof *D);
	s->J = malloc(nrec * sizeof *s->J), s->Rall = malloc(kept * nrec * sizeof *s->Rall);
	s->bad = malloc(chunk * sizeof *s->bad);
	s->cmissing = calloc(chunk, sizeof *s->cmissing), s->cleft = calloc(chunk, sizeof *s->cleft);
	s->skipall = malloc(kept);
	s->total = calloc(nsup, sizeof *s->total), s->part = calloc(nsup, sizeof *s->part), s->depth = calloc(nsup, sizeof *s->depth);
	s->ttotal = calloc(nsup, sizeof *s->ttotal), s->tpart = calloc(nsup, sizeof *s->tpart);
	s->moved = calloc(n, sizeof *s->moved), s->mpart = calloc(n, sizeof *s->mpart);
	if (!D || !s->J || !s->Rall || !s->bad || !s->cmissing || !s->cleft || !s->skipall || !s->total || !s->part || !s->depth || !s->ttotal || !s->tpart ||
		!s->moved || !s->mpart || ((f || tf || rf) && andi_hip_distances(M, n, r->model, D)))
		err(errno, "Could not allocate enough memory for the support values.");
	s->point_ok = f != NULL, s->trans_ok = tf != NULL, s->cons_ok = cf != NULL, s->rogue_ok = rf != NULL;
	if (cmpl.on && (f || tf || rf) && complete_one(r->ctx, D, n, 1)) {
		if (f) soft_warnx("No support values: %s", andi_hip_last_error(r->ctx));
		if (tf) soft_warnx("No transfer support: %s", andi_hip_last_error(r->ctx));
		if (rf) soft_warnx("No rogue table: %s", andi_hip_last_error(r->ctx));
		s->point_ok = s->trans_ok = s->rogue_ok = 0;
	}
	for (size_t i = 0; i < n && (s->point_ok || s->trans_ok || s->rogue_ok); i++)
		for (size_t j = i + 1; j < n; j++)
			if (!isfinite(D[i * n + j])) {
				if (f) soft_warnx("No support values: the distance of '%s' and '%s'%s", g[i].name, g[j].name, NOT_FINITE);
				if (tf) soft_warnx("No transfer support: the distance of '%s' and '%s'%s", g[i].name, g[j].name, NOT_FINITE);
				if (rf) soft_warnx("No rogue table: the distance of '%s' and '%s'%s", g[i].name, g[j].name, NOT_FINITE);
				s->point_ok = s->trans_ok = s->rogue_ok = 0;
				break;
			}
	if ((s->point_ok || s->trans_ok || s->rogue_ok) && join_one(r->ctx, D, n, r->method, s->J)) {
		if (f) soft_warnx("No support values: %s", andi_hip_last_error(r->ctx));
		if (tf) soft_warnx("No transfer support: %s", andi_hip_last_error(r->ctx));
		if (rf) soft_warnx("No rogue table: %s", andi_hip_last_error(r->ctx));
		s->point_ok = s->trans_ok = s->rogue_ok = 0;
	}
	if (s->point_ok || s->trans_ok || s->rogue_ok) refine_joined(r->ctx, s->J, n, D, 1, r->names, r->truncate);
	if (lengths_ols && !trees_only && (s->point_ok || s->trans_ok)) { /* (the chunks' matrices take D's place) */
		if (!(s->Dpoint = malloc(n * n * sizeof *D))) err(errno, "Could not allocate enough memory for the support values.");
		memcpy(s->Dpoint, D, n * n * sizeof *D);
	}
}

/* replicates start ... start + count - 1: their matrices B (count * n * n models), or NULL under --trees-only */
static void support_chunk(support_state *s, unsigned long start, size_t count, const andi_hip_model *B, const andi_hip_model *M) {
	const size_t n = s->r.n, nrec = s->nrec;
	const genome *g = s->r.g;
	andi_hip_ctx *ctx = s->r.ctx;
	FILE *f = s->o[OUT_SUPPORT].f, *cf = s->o[OUT_CONSENSUS].f, *tf = s->o[OUT_TRANSFER].f, *rf = s->r.rogues->f;
	for (unsigned long first = start; first < start + count && !s->stopped; first += s->cap) {
		const size_t c = start + count - first < s->cap ? start + count - first : s->cap;
		andi_hip_nj_join *R = cf ? s->Rall + first * nrec : s->Rall;
		uint8_t *skip = cf ? s->skipall + first : s->skipall;
		int failed;
		if (s->r.trees_only) {
			failed = join_bootstrap(ctx, M, n, s->r.model, s->r.method, s->r.seed, first, c, R, s->bad);
		} else {
			for (size_t k = 0; k < c; k++)
				if (andi_hip_distances(B + (first - start + k) * n * n, n, s->r.model, s->D + k * n * n))
					err(errno, "Could not allocate enough memory for the support values.");
			failed = cmpl.on && andi_hip_complete_batch(ctx, s->D, n, c, 0, s->D, s->cmissing, s->cleft);
			for (size_t k = 0; cmpl.on && !failed && k < c; k++)
				complete_warn(first + (unsigned long)k + 2, (size_t)s->cmissing[k], (size_t)s->cleft[k]);
			if (!failed) failed = join_batch(ctx, s->D, n, c, s->r.method, R, s->bad);
		}
		if (failed) {
			if (f) soft_warnx("No support values: %s", andi_hip_last_error(ctx));
			if (cf) soft_warnx("No consensus tree: %s", andi_hip_last_error(ctx));
			if (tf) soft_warnx("No transfer support: %s", andi_hip_last_error(ctx));
			if (rf) soft_warnx("No rogue table: %s", andi_hip_last_error(ctx));
			if (!f && !cf && !tf && !rf) soft_warnx("No trees: %s", andi_hip_last_error(ctx));
			s->point_ok = s->cons_ok = s->trans_ok = s->rogue_ok = 0;
			s->stopped = 1;
			break;
		}
		for (size_t k = 0; k < c; k++) {
			skip[k] = s->bad[k] >= 0;
			if (skip[k])
				soft_warnx("No tree for matrix %lu: the distance of '%s' and '%s'%s", first + (unsigned long)k + 2,
						   g[s->bad[k] / (int64_t)n].name, g[s->bad[k] % (int64_t)n].name, NOT_FINITE);
			else if (!s->r.trees_only) refine_joined(ctx, R + k * nrec, n, s->D + k * n * n, first + (unsigned long)k + 2, s->r.names, s->r.truncate);
			if (!skip[k] && s->o[OUT_TREE].f) put_newick(&s->o[OUT_TREE], &(newick_src){.J = R + k * nrec, .ctx = ctx, .D = s->r.trees_only ? NULL : s->D + k * n * n}, s->r.names, n, s->r.truncate);
			s->counted += !skip[k];
		}
		/* (whatever fails below, the replicates' lines of --tree are still written) */
		if (s->point_ok) {
			if (andi_hip_nj_support(ctx, s->J, R, n, c, skip, s->part)) {
				soft_warnx("No support values: %s", andi_hip_last_error(ctx));
				s->point_ok = 0;
			} else
				for (size_t k = 0; k + 3 < n; k++) s->total[k] += s->part[k];
		}
		if (s->trans_ok) {
			if (andi_hip_nj_transfer(ctx, s->J, R, n, c, skip, s->depth, s->tpart, NULL)) {
				soft_warnx("No transfer support: %s", andi_hip_last_error(ctx));
				s->trans_ok = 0;
			} else
				for (size_t k = 0; k + 3 < n; k++) s->ttotal[k] += s->tpart[k];
		}
		if (s->rogue_ok) {
			uint64_t pairs = 0;
			if (andi_hip_nj_transfer_taxa(ctx, s->J, R, n, c, skip, s->r.rogues->cutoff, s->mpart, &pairs, NULL, NULL)) {
				soft_warnx("No rogue table: %s", andi_hip_last_error(ctx));
				s->rogue_ok = 0;
			} else {
				for (size_t i = 0; i < n; i++) s->moved[i] += s->mpart[i];
				s->pairs += pairs;
			}
		}
	}
}

/* the files; complete = 0: the replicates were not all drawn, nothing is written */
static void support_end(support_state *s, int complete) {
	const size_t n = s->r.n;
	const char **names = s->r.names;
	andi_hip_ctx *ctx = s->r.ctx;
	const unsigned long counted = s->counted, replicates = s->r.replicates;
	if (!complete) s->point_ok = s->trans_ok = s->cons_ok = s->rogue_ok = 0;
	if (s->point_ok) {
		if (counted < replicates) soft_warnx("Support values from %lu of %lu bootstrap matrices.", counted, replicates);
		put_newick(&s->o[OUT_SUPPORT], &(newick_src){.J = s->J, .support = s->total, .ctx = ctx, .point = 1, .D = s->Dpoint}, names, n, s->r.truncate);
	}
	if (s->trans_ok && counted == 0) {
		soft_warnx("No transfer support: no bootstrap matrix has a tree.");
		s->trans_ok = 0;
	}
	if (s->trans_ok) {
		if (counted < replicates) soft_warnx("Transfer support from %lu of %lu bootstrap matrices.", counted, replicates);
		put_newick(&s->o[OUT_TRANSFER], &(newick_src){.J = s->J, .depth = s->depth, .transfer = s->ttotal, .used = counted, .ctx = ctx, .point = 1, .D = s->Dpoint}, names, n,
				   s->r.truncate);
	}
	if (s->rogue_ok && counted == 0) {
		soft_warnx("No rogue table: no bootstrap matrix has a tree.");
		s->rogue_ok = 0;
	}
	if (s->rogue_ok) {
		const rogue_out *ro = s->r.rogues;
		if (counted < replicates) soft_warnx("Rogue table from %lu of %lu bootstrap matrices.", counted, replicates);
		if (s->pairs == 0) warnx("Rogue table: no branch of a bootstrap matrix's tree is within the cutoff; every index is 0.");
		const int w = s->r.truncate ? 10 : INT_MAX;
		int bad = fputs("#name\tmoved\tindex\n", ro->f) == EOF;
		for (size_t i = 0; i < n && !bad; i++)
			bad = fprintf(ro->f, "%.*s\t%llu\t%.6g\n", w, names[i], (unsigned long long)s->moved[i],
						  s->pairs ? (double)s->moved[i] / (double)s->pairs : 0.0) < 0;
		if (bad) err(1, "%s", ro->path);
	}
	if (s->cons_ok && counted == 0) {
		soft_warnx("No consensus tree: no bootstrap matrix has a tree.");
		s->cons_ok = 0;
	}
	if (s->cons_ok) {
		uint32_t *ids = malloc(replicates * s->nsup * sizeof *ids), *freq = NULL;
		uint64_t *sets = NULL;
		size_t nsplits = 0, ninner = 0;
		andi_hip_cons_node *nodes = malloc((2 * n - 1) * sizeof *nodes);
		if (!ids || !nodes) err(errno, "Could not allocate enough memory for the consensus tree.");
		if (andi_hip_nj_splits(ctx, s->Rall, n, replicates, s->skipall, ids, &nsplits, &freq, &sets)) {
			soft_warnx("No consensus tree: %s", andi_hip_last_error(ctx));
		} else if (andi_hip_consensus(s->Rall, n, replicates, s->skipall, ids, nsplits, freq, sets, nodes, &ninner)) {
			soft_warnx("No consensus tree: the bootstrap matrices' trees are inconsistent.");
		} else {
			if (counted < replicates) soft_warnx("Consensus tree from %lu of %lu bootstrap matrices.", counted, replicates);
			put_newick(&s->o[OUT_CONSENSUS], &(newick_src){.nodes = nodes, .ninner = ninner}, names, n, s->r.truncate);
		}
		andi_hip_free(freq), andi_hip_free(sets);
		free(ids), free(nodes);
	}
	free(s->D), free(s->Dpoint), free(s->J), free(s->Rall), free(s->bad), free(s->cmissing), free(s->cleft), free(s->skipall), free(s->total), free(s->part), free(s->depth), free(s->ttotal),
		free(s->tpart), free(s->moved), free(s->mpart);
}

/* --dendrogram, --clusters: agglomerative clustering (andi_hip_linkage) of every printed matrix, from the averaged distances
 * whatever -vv asks the matrix to print.  A pair without a distance does not stop it: it is the pair farthest apart.
 * cluster_point takes the point estimate (its dendrogram line, its clusters at the threshold and their medoids),
 * cluster_chunk every chunk of bootstrap matrices main draws (one andi_hip_linkage_batch call: their dendrogram lines, and
 * how many of their clusterings hold each cluster of the point estimate; the chunks' counts add up), cluster_end writes
 * the clusters. */
typedef struct {
	const char *dendro_path, *clusters_path;
	FILE *df, *cf;
	int method, have_threshold;
	double threshold;
	andi_hip_ctx *ctx; /* one for all matrices, on opts.device */
	int device_for_ctx;
	int failed; /* it could not be created: said once */
	uint32_t *labels, *medoid, *stability;
	size_t nclusters;
	int clusters_ok; /* the point estimate has clusters */
	unsigned long counted; /* the bootstrap matrices behind the stability */
} cluster_out;

static int cluster_ctx(cluster_out *c) {
	char msg[512];
	if (c->failed) return 0;
	if (!c->ctx && andi_hip_ctx_create(&c->ctx, c->device_for_ctx, msg, sizeof msg)) {
		c->failed = 1, c->ctx = NULL;
		soft_warnx("No clustering: %s", msg);
		return 0;
	}
	return 1;
}

/* the dendrogram of the K-th printed matrix, one Newick line */
static void put_dendrogram(const cluster_out *c, const andi_hip_link *Z, const char **names, size_t n, int truncate, unsigned long k) {
	size_t cap = 64 + n * 40;
	for (size_t i = 0; i < n; i++) cap += strlen(names[i]);
	char *text = xmalloc(cap);
	size_t need = andi_hip_format_newick_linkage(Z, n, names, truncate, text, cap);
	if (need >= cap) free(text), cap = need + 1, text = xmalloc(cap), need = andi_hip_format_newick_linkage(Z, n, names, truncate, text, cap);
	if (need == 0) soft_warnx("No dendrogram for matrix %lu: a branch is not finite (a pair of sequences has no distance).", k);
	else if (fputs(text, c->df) == EOF) err(1, "%s", c->dendro_path);
	free(text);
}

static void cluster_point(cluster_out *c, const andi_hip_model *M, const char **names, size_t n, int model, int truncate) {
	if (!cluster_ctx(c)) return;
	double *D = malloc(n * n * sizeof *D);
	andi_hip_link *Z = malloc(n * sizeof *Z);
	c->labels = malloc(n * sizeof *c->labels), c->medoid = malloc(n * sizeof *c->medoid), c->stability = calloc(n, sizeof *c->stability);
	if (!D || !Z || !c->labels || !c->medoid || !c->stability || andi_hip_distances(M, n, model, D))
		err(errno, "Could not allocate enough memory for the clustering.");
	if (andi_hip_linkage(c->ctx, D, n, c->method, Z)) {
		if (c->df) soft_warnx("No dendrogram for matrix 1: %s", andi_hip_last_error(c->ctx));
		if (c->cf) soft_warnx("No clusters: %s", andi_hip_last_error(c->ctx));
	} else {
		if (c->df) put_dendrogram(c, Z, names, n, truncate, 1);
		if (c->cf) {
			if (andi_hip_linkage_cut(Z, n, c->threshold, c->labels, &c->nclusters) ||
				andi_hip_cluster_medoids(D, n, c->labels, c->nclusters, c->medoid))
				soft_warnx("No clusters: the linkage tree is inconsistent.");
			else c->clusters_ok = 1;
		}
	}
	free(D), free(Z);
}

/* bootstrap matrices first ... first + count - 1 (the printed matrices first + 2 ...) */
static void cluster_chunk(cluster_out *c, const andi_hip_model *B, unsigned long first, size_t count, const genome *g, const char **names,
						  size_t n, int model, int truncate) {
	if (!cluster_ctx(c) || (!c->df && !c->clusters_ok)) return;
	double *D = malloc(count * n * n * sizeof *D);
	andi_hip_link *Z = malloc(count * n * sizeof *Z);
	int64_t *bad = malloc(count * sizeof *bad);
	uint32_t *rep = malloc(count * n * sizeof *rep), *part = malloc(n * sizeof *part);
	if (!D || !Z || !bad || !rep || !part) err(errno, "Could not allocate enough memory for the clustering.");
	for (size_t k = 0; k < count; k++)
		if (andi_hip_distances(B + k * n * n, n, model, D + k * n * n)) err(errno, "Could not allocate enough memory for the clustering.");
	if (andi_hip_linkage_batch(c->ctx, D, n, count, c->method, Z, bad)) {
		soft_warnx("No clustering of the bootstrap matrices: %s", andi_hip_last_error(c->ctx));
		c->failed = 1;
	} else {
		size_t used = 0;
		for (size_t k = 0; k < count; k++) {
			const andi_hip_link *Zk = Z + k * (n - 1);
			size_t theirs = 0;
			if (bad[k] >= 0) {
				soft_warnx("No clustering of matrix %lu: the distance of '%s' and '%s' is -inf.", first + (unsigned long)k + 2,
						   g[bad[k] / (int64_t)n].name, g[bad[k] % (int64_t)n].name);
				continue;
			}
			if (c->df) put_dendrogram(c, Zk, names, n, truncate, first + (unsigned long)k + 2);
			if (c->clusters_ok && !andi_hip_linkage_cut(Zk, n, c->threshold, rep + used * n, &theirs)) used++;
		}
		if (c->clusters_ok && used) {
			if (andi_hip_cluster_stability(c->labels, c->nclusters, rep, n, used, part)) {
				soft_warnx("No stability: the clusterings are inconsistent.");
				c->failed = 1;
			} else {
				for (size_t k = 0; k < c->nclusters; k++) c->stability[k] += part[k];
				c->counted += used;
			}
		}
	}
	free(D), free(Z), free(bad), free(rep), free(part);
}

/* the clusters file; replicates: the bootstrap matrices of the run (0: no stability column), complete: all were drawn */
static void cluster_end(cluster_out *c, const char **names, size_t n, int truncate, unsigned long replicates, int complete) {
	if (c->cf && c->clusters_ok) {
		const int stab = replicates > 0 && complete && !c->failed;
		if (replicates > 0 && !stab) soft_warnx("No stability: the bootstrap matrices were not all clustered.");
		else if (stab && c->counted < replicates) soft_warnx("Stability from %lu of %lu bootstrap matrices.", c->counted, replicates);
		const int w = truncate ? 10 : INT_MAX;
		int bad = fprintf(c->cf, "#name\tcluster\trepresentative%s\n", stab ? "\tstability" : "") < 0;
		for (size_t i = 0; i < n && !bad; i++) {
			const uint32_t l = c->labels[i];
			bad |= fprintf(c->cf, "%.*s\t%u\t%.*s", w, names[i], (unsigned)l + 1, w, names[c->medoid[l]]) < 0;
			if (stab) bad |= fprintf(c->cf, "\t%u", (unsigned)c->stability[l]) < 0;
			bad |= fputc('\n', c->cf) == EOF;
		}
		if (bad) err(1, "%s", c->clusters_path);
	}
	free(c->labels), free(c->medoid), free(c->stability);
	if (c->ctx) andi_hip_ctx_destroy(c->ctx);
	if (c->df && fclose(c->df)) err(1, "%s", c->dendro_path);
	if (c->cf && fclose(c->cf)) err(1, "%s", c->clusters_path);
}

/* the checks and warnings the input gets (src/andi.c:282-310): the sequences of a, then those of b (may be NULL) */
static void check_genomes(const genome_list *a, const genome_list *b, int truncate) {
	if (saw_non_acgt)
		warnx("The input sequences contained characters other than acgtACGT. These were automatically "
			  "stripped to ensure correct results.");
	int any_short = 0;
	const size_t limit = (INT_MAX - 1) / 2;
	for (const genome_list *l = a; l; l = l == a ? b : NULL)
		for (size_t i = 0; i < l->n; i++) {
			const genome *g = &l->v[i];
			if (truncate && strlen(g->name) > 10)
				warnx("The sequence name '%s' is longer than ten characters. It will be truncated in the output "
					  "to '%.10s'.", g->name, g->name);
			if (g->len > limit) errx(1, "The sequence %s is too long. The technical limit is %zu.", g->name, limit);
			if (g->len == 0) errx(1, "The sequence %s is empty.", g->name);
			if (g->len < 1000) any_short = 1;
		}
	if (any_short)
		soft_warnx("One of the given input sequences is shorter than a thousand nucleotides. This may result "
				   "in inaccurate distances. Try an alignment instead.");
}

static andi_hip_seq *seq_array(const genome_list *l) {
	andi_hip_seq *in = xmalloc(l->n * sizeof *in);
	for (size_t i = 0; i < l->n; i++) in[i].seq = l->v[i].seq, in[i].len = l->v[i].len;
	return in;
}

/* --place: where on the backbone tree (--backbone, a tree of the references) every query sits, as jplace text */
typedef struct {
	const char *path, *backbone_path;
	FILE *f;
	int method;
	andi_hip_nj_join *J; /* the backbone's records, the references its leaves */
} place_out;

/* the backbone is read before anything is computed: a tree of other sequences ends the run with the parser's message */
static void place_read_backbone(place_out *pl, const genome *refs, size_t nr, int truncate) {
	if (nr < 3) errx(1, "Placement (--place) needs a tree: give at least three references.");
	if (nr > 65535) errx(1, "Placement (--place) is limited to 65535 references (%zu given).", nr);
	size_t len = 0;
	read_buffer rb = {0};
	char *text = slurp(pl->backbone_path, &len, &rb);
	if (!text) err(1, "%s", pl->backbone_path);
	const char **rn = name_array(refs, nr);
	pl->J = xmalloc((nr - 2) * sizeof *pl->J);
	char msg[512];
	if (andi_hip_parse_newick(text, rn, nr, truncate, pl->J, msg, sizeof msg)) errx(1, "%s: %s", pl->backbone_path, msg);
	free(rn), free(text);
}

/* rn, nr: the backbone's leaves.  col == NULL: MRQ and MQR hold all of them; else (--screen) they hold the nk references
 * col[0] < col[1] < ... only, and the others count as references without a distance (NaN) */
static void place_queries(const place_out *pl, const andi_hip_model *MRQ, const andi_hip_model *MQR, const char **rn, size_t nr,
						  const size_t *col, size_t nk, const char **qn, size_t nq, int model, int truncate, int device) {
	andi_hip_ctx *ctx = NULL;
	char msg[512];
	if (andi_hip_ctx_create(&ctx, device, msg, sizeof msg)) {
		soft_warnx("No placements: %s", msg);
		return;
	}
	double *D = malloc(nq * nr * sizeof *D);
	andi_hip_placement *P = malloc(nq * sizeof *P);
	if (!D || !P || andi_hip_distances_rect(MRQ, MQR, col ? nk : nr, nq, model, D)) err(errno, "Could not allocate enough memory for the placements.");
	if (col) /* the nq x nk distances lie at the front of D: spread every row over its nr columns, from the back */
		for (size_t q = nq; q-- > 0;) {
			size_t j = nk;
			for (size_t r = nr; r-- > 0;) {
				if (j > 0 && col[j - 1] == r) D[q * nr + r] = D[q * nk + --j];
				else D[q * nr + r] = NAN;
			}
		}
	if (andi_hip_place(ctx, pl->J, nr, D, nq, pl->method, P, NULL, NULL, NULL)) {
		soft_warnx("No placements: %s", andi_hip_last_error(ctx));
	} else {
		for (size_t q = 0; q < nq; q++)
			if (P[q].edge < 0) soft_warnx("No placement for '%s': only %u of its distances to the references can be used.", qn[q], P[q].used);
		size_t cap = 512 + nr * 64 + nq * 128;
		for (size_t i = 0; i < nr; i++) cap += 2 * strlen(rn[i]);
		for (size_t q = 0; q < nq; q++) cap += 6 * strlen(qn[q]);
		char *text = xmalloc(cap);
		const size_t need = andi_hip_format_jplace(pl->J, nr, rn, truncate, P, nq, qn, pl->method, text, cap);
		if (need >= cap) free(text), cap = need + 1, text = xmalloc(cap), andi_hip_format_jplace(pl->J, nr, rn, truncate, P, nq, qn, pl->method, text, cap);
		if (fputs(text, pl->f) == EOF) err(1, "%s", pl->path);
		free(text);
	}
	free(D), free(P);
	andi_hip_ctx_destroy(ctx);
}

/* --screen=K: a k-mer sketch screen in front of the query-versus-reference mode */
typedef struct {
	size_t keep; /* 0: no screen */
	int k, k_given, scale_given, min_given;
	uint64_t scale;
	uint32_t min;
	const char *report_path;
	FILE *rf;
} screen_opts;

/* Sketches both sets, selects, writes the report; returns the indices of the kept references, ascending, *nk of them.
 * A run that keeps nothing ends here. */
static size_t *screen_references(const screen_opts *sc, const genome_list *refs, const genome_list *qs, int truncate, int verbose,
								 int device, size_t *nk) {
	const size_t nr = refs->n, nq = qs->n;
	if (SIZE_MAX / sizeof(uint32_t) / nr < nq) errx(1, "The screen is limited to fewer sequences (%zu given).", nr + nq);
	uint32_t *shared = malloc(nr * nq * sizeof *shared), *rs = malloc(nr * sizeof *rs), *qsz = malloc(nq * sizeof *qsz);
	uint32_t *taken = malloc(nq * sizeof *taken);
	uint8_t *kept = malloc(nr);
	if (!shared || !rs || !qsz || !taken || !kept) err(errno, "Could not allocate enough memory for the screen.");
	andi_hip_seq *rin = seq_array(refs), *qin = seq_array(qs);
	char msg[512];
	if (andi_hip_screen(rin, nr, qin, nq, sc->k, sc->scale, device, shared, rs, qsz, msg, sizeof msg)) errx(1, "%s", msg);
	if (andi_hip_screen_select(shared, nq, nr, sc->keep, sc->min, kept, taken)) errx(1, "The screen could not select references.");
	if (sc->rf) {
		const int w = truncate ? 10 : INT_MAX;
		int bad = fprintf(sc->rf, "#query\treference\tshared\tquery_hashes\treference_hashes\tcontainment\tkept\n") < 0;
		for (size_t q = 0; q < nq && !bad; q++)
			for (size_t r = 0; r < nr && !bad; r++) {
				const uint32_t c = shared[q * nr + r];
				if (c)
					bad |= fprintf(sc->rf, "%.*s\t%.*s\t%u\t%u\t%u\t%.6f\t%d\n", w, qs->v[q].name, w, refs->v[r].name, (unsigned)c,
								   (unsigned)qsz[q], (unsigned)rs[r], (double)c / (double)qsz[q], (int)kept[r]) < 0;
			}
		if (bad || fclose(sc->rf)) err(1, "%s", sc->report_path);
	}
	size_t *col = xmalloc(nr * sizeof *col), n = 0;
	for (size_t r = 0; r < nr; r++)
		if (kept[r]) col[n++] = r;
	if (verbose) fprintf(stderr, "%s: The screen kept %zu of %zu references.\n", program_invocation_short_name, n, nr);
	if (n == 0)
		errx(1, "The screen kept no reference: no query shares %u or more hashes with any of them (--screen-kmer=%d, --screen-scale=%llu).",
			 (unsigned)(sc->min > 1 ? sc->min : 1), sc->k, (unsigned long long)sc->scale);
	for (size_t q = 0; q < nq; q++)
		if (!taken[q]) soft_warnx("The screen kept no reference for '%s': it shares too few hashes with every one of them.", qs->v[q].name);
	free(shared), free(rs), free(qsz), free(taken), free(kept), free(rin), free(qin);
	*nk = n;
	return col;
}

/* --reference: the queries (the FILES) against the references, the two cross blocks of the square run over both sets */
static int run_rect(const name_list *ref_files, const name_list *files, int join, int verbose, int truncate, int show_progress,
					andi_hip_opts *opts, place_out *pl, const screen_opts *sc) {
	genome_list refs = {0}, qs = {0}, all_refs = {0};
	read_all_files(ref_files->v, ref_files->n, join, opts->host_threads, &refs);
	read_all_files(files->v, files->n, join, opts->host_threads, &qs);
	if (refs.n == 0) errx(1, "No reference sequences given: --reference and --reference-list name no readable sequence.");
	if (qs.n == 0) errx(1, "No query sequences given: name at least one FASTA file besides the references.");
	size_t *col = NULL; /* --screen: the kept references' places among all of them; from here on refs holds the kept ones only */
	if (sc->keep) {
		size_t nk = 0;
		col = screen_references(sc, &refs, &qs, truncate, verbose, opts->device, &nk);
		all_refs = refs;
		refs.v = xmalloc(nk * sizeof *refs.v), refs.n = refs.cap = nk;
		for (size_t j = 0; j < nk; j++) refs.v[j] = all_refs.v[col[j]];
	}
	check_genomes(&refs, &qs, truncate);
	const size_t nr = refs.n, nq = qs.n;
	if (pl->path) place_read_backbone(pl, col ? all_refs.v : refs.v, col ? all_refs.n : nr, truncate);
	if (show_progress) {
		progress_n = nr + nq;
		opts->progress = progress_cb;
		progress_cb(0, 2 * nr * nq, NULL);
	}
	if (SIZE_MAX / sizeof(andi_hip_model) / nr < nq) errx(1, "Comparison is limited to fewer sequences (%zu given).", nr + nq);
	andi_hip_model *MRQ = malloc(nr * nq * sizeof *MRQ), *MQR = malloc(nr * nq * sizeof *MQR);
	if (!MRQ || !MQR) err(errno, "Could not allocate enough memory for the comparison matrix. Try using --join or --low-memory.");
	andi_hip_seq *rin = seq_array(&refs), *qin = seq_array(&qs);
	char msg[512];
	if (andi_hip_dist_rect(MRQ, MQR, rin, nr, qin, nq, opts, msg, sizeof msg)) errx(1, "%s", msg);
	if (show_progress) fprintf(stderr, ", done.\n");
	const char **rn = name_array(refs.v, nr), **qn = name_array(qs.v, nq);
	print_distances(MRQ, MQR, rn, nr, qn, nq, opts->model, verbose >= 2, truncate, 1);
	if (verbose) { /* print_coverages, src/io.c:329-338, of the query rows */
		printf("\nCoverage:\n");
		for (size_t q = 0; q < nq; q++) {
			for (size_t r = 0; r < nr; r++) printf("%1.4e ", andi_hip_model_coverage(&MQR[q * nr + r]));
			printf("\n");
		}
	}
	if (pl->path) {
		const char **an = col ? name_array(all_refs.v, all_refs.n) : rn;
		place_queries(pl, MRQ, MQR, an, col ? all_refs.n : nr, col, nr, qn, nq, opts->model, truncate, opts->device);
		if (col) free(an);
		if (fclose(pl->f)) err(1, "%s", pl->path);
		free(pl->J);
	}
	free(rn), free(qn);
	free(MRQ);
	free(MQR);
	free(rin);
	free(qin);
	free(col);
	return soft_error ? EXIT_FAILURE : EXIT_SUCCESS;
}

/* a positive integer of at most `max`, or 0 */
static unsigned long long positive_arg(const char *text, unsigned long long max) {
	errno = 0;
	char *end;
	if (!isdigit((unsigned char)*text)) return 0;
	const unsigned long long v = strtoull(text, &end, 10);
	return errno || end == text || *end || v > max ? 0 : v;
}

int main(int argc, char *argv[]) {
	static const struct option long_options[] = {{"version", no_argument, NULL, 0},
												 {"truncate-names", no_argument, NULL, 0},
												 {"file-of-filenames", required_argument, NULL, 0},
												 {"progress", optional_argument, NULL, 0},
												 {"reference", required_argument, NULL, 0},
												 {"reference-list", required_argument, NULL, 0},
												 {"backbone", required_argument, NULL, 0},
												 {"place", required_argument, NULL, 0},
												 {"place-method", required_argument, NULL, 0},
												 {"screen", required_argument, NULL, 0},
												 {"screen-kmer", required_argument, NULL, 0},
												 {"screen-scale", required_argument, NULL, 0},
												 {"screen-min", required_argument, NULL, 0},
												 {"screen-report", required_argument, NULL, 0},
												 {"tree", required_argument, NULL, 0},
												 {"support", required_argument, NULL, 0},
												 {"consensus", required_argument, NULL, 0},
												 {"transfer", required_argument, NULL, 0},
												 {"rogues", required_argument, NULL, 0},
												 {"rogue-cutoff", required_argument, NULL, 0},
												 {"trees-only", no_argument, NULL, 0},
												 {"tree-method", required_argument, NULL, 0},
												 {"complete", no_argument, NULL, 0},
												 {"complete-report", required_argument, NULL, 0},
												 {"delta", required_argument, NULL, 0},
												 {"root", required_argument, NULL, 0},
												 {"root-report", required_argument, NULL, 0},
												 {"lengths", required_argument, NULL, 0},
												 {"fit", required_argument, NULL, 0},
												 {"refine", required_argument, NULL, 0},
												 {"refine-moves", required_argument, NULL, 0},
												 {"refine-tol", required_argument, NULL, 0},
												 {"refine-report", required_argument, NULL, 0},
												 {"linkage", required_argument, NULL, 0},
												 {"dendrogram", required_argument, NULL, 0},
												 {"clusters", required_argument, NULL, 0},
												 {"threshold", required_argument, NULL, 0},
												 {"help", no_argument, NULL, 'h'},
												 {"verbose", no_argument, NULL, 'v'},
												 {"join", no_argument, NULL, 'j'},
												 {"low-memory", no_argument, NULL, 'l'},
												 {"threads", required_argument, NULL, 't'},
												 {"bootstrap", required_argument, NULL, 'b'},
												 {"model", required_argument, NULL, 'm'},
												 {0, 0, 0, 0}};
	andi_hip_opts opts;
	andi_hip_default_opts(&opts);
	long procs = sysconf(_SC_NPROCESSORS_ONLN);
	opts.host_threads = procs > 0 ? (int)procs : 1;
	/* one GPU unless asked: ANDI_HIP_GPUS=k tiles the rows of the matrix over the first k visible GPUs, ANDI_HIP_GPUS=all over
	 * all of them (the gather between distinct devices has not run on hardware yet: opt-in until it has) */
	opts.num_gpus = 1;
	if (getenv("ANDI_HIP_GPUS")) {
		if (!strcmp(getenv("ANDI_HIP_GPUS"), "all")) opts.num_gpus = -1;
		else if (atoi(getenv("ANDI_HIP_GPUS")) > 0) opts.num_gpus = atoi(getenv("ANDI_HIP_GPUS"));
	}
	int verbose = 0, join = 0, truncate = 0;
	unsigned long bootstrap = 0;
	enum { P_AUTO, P_NEVER, P_ALWAYS } progress = P_AUTO;
	name_list files = {0}, ref_files = {0}; /* ref_files: --reference, --reference-list, the query-versus-reference mode */
	int rect = 0, bootstrap_given = 0, trees_only = 0;
	tree_out tree = {.o = &outs[OUT_TREE], .method = ANDI_TREE_NJ};
	rogue_out rogues = {.cutoff = 0.3}; /* (booster's default for the same cutoff) */
	cluster_out clus = {.method = ANDI_LINK_AVERAGE};
	place_out place = {.method = ANDI_PLACE_FM};
	screen_opts screen = {.k = 21, .scale = 1000, .min = 1};
	int screen_given = 0;

	for (;;) {
		int idx = 0;
		int c = getopt_long(argc, argv, "jvht:p:m:b:l", long_options, &idx);
		if (c == -1) break;
		switch (c) {
			case 0: {
				const char *o = long_options[idx].name;
				if (!strcmp(o, "version")) version();
				if (!strcmp(o, "truncate-names")) truncate = 1;
				if (!strcmp(o, "file-of-filenames")) read_file_of_filenames(optarg, &files);
				for (int k = 0; k < OUT_COUNT; k++)
					if (!strcmp(o, outs[k].option)) outs[k].path = optarg;
				if (!strcmp(o, "trees-only")) trees_only = 1;
				if (!strcmp(o, "complete")) cmpl.on = 1;
				if (!strcmp(o, "complete-report")) cmpl.on = 1, cmpl.report_path = optarg;
				if (!strcmp(o, "delta")) dlt.path = optarg;
				if (!strcmp(o, "root")) {
					if (!strcasecmp(optarg, "mad")) rootopt.method = ANDI_ROOT_MAD;
					else if (!strcasecmp(optarg, "midpoint")) rootopt.method = ANDI_ROOT_MIDPOINT;
					else errx(1, "Expected one of 'mad' or 'midpoint' for --root, but '%s' was given.", optarg);
					rootopt.on = 1;
				}
				if (!strcmp(o, "root-report")) rootopt.report_path = optarg;
				if (!strcmp(o, "lengths")) {
					if (!strcasecmp(optarg, "joined")) lengths_ols = 0;
					else if (!strcasecmp(optarg, "ols")) lengths_ols = 1;
					else errx(1, "Expected one of 'joined' or 'ols' for --lengths, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "fit")) fitopt.path = optarg;
				if (!strcmp(o, "refine")) {
					if (!strcasecmp(optarg, "none")) refopt.on = 0;
					else if (!strcasecmp(optarg, "bnni")) refopt.on = 1;
					else errx(1, "Expected one of 'none' or 'bnni' for --refine, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "refine-moves")) {
					refopt.moves_arg = optarg;
					if (!strcasecmp(optarg, "nni")) refopt.spr = 0;
					else if (!strcasecmp(optarg, "spr")) refopt.spr = 1;
					else errx(1, "Expected one of 'nni' or 'spr' for --refine-moves, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "refine-tol")) refopt.tol_arg = optarg;
				if (!strcmp(o, "refine-report")) refopt.report_path = optarg;
				if (!strcmp(o, "rogues")) rogues.path = optarg;
				if (!strcmp(o, "rogue-cutoff")) rogues.cutoff_arg = optarg;
				if (!strcmp(o, "dendrogram")) clus.dendro_path = optarg;
				if (!strcmp(o, "clusters")) clus.clusters_path = optarg;
				if (!strcmp(o, "tree-method")) {
					if (!strcasecmp(optarg, "nj")) tree.method = ANDI_TREE_NJ;
					else if (!strcasecmp(optarg, "bionj")) tree.method = ANDI_TREE_BIONJ;
					else errx(1, "Expected one of 'nj' or 'bionj' for --tree-method, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "linkage")) {
					if (!strcasecmp(optarg, "single")) clus.method = ANDI_LINK_SINGLE;
					else if (!strcasecmp(optarg, "complete")) clus.method = ANDI_LINK_COMPLETE;
					else if (!strcasecmp(optarg, "average")) clus.method = ANDI_LINK_AVERAGE;
					else errx(1, "Expected one of 'single', 'complete' or 'average' for --linkage, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "threshold")) {
					errno = 0;
					char *end;
					clus.threshold = strtod(optarg, &end);
					if (errno || end == optarg || *end || !isfinite(clus.threshold) || clus.threshold < 0.0)
						errx(1, "Expected a finite number of at least 0 for --threshold, but '%s' was given.", optarg);
					clus.have_threshold = 1;
				}
				if (!strcmp(o, "backbone")) place.backbone_path = optarg;
				if (!strcmp(o, "place")) place.path = optarg;
				if (!strcmp(o, "place-method")) {
					if (!strcasecmp(optarg, "fm")) place.method = ANDI_PLACE_FM;
					else if (!strcasecmp(optarg, "ols")) place.method = ANDI_PLACE_OLS;
					else errx(1, "Expected one of 'fm' or 'ols' for --place-method, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "screen")) {
					screen_given = 1;
					if (!(screen.keep = (size_t)positive_arg(optarg, SIZE_MAX)))
						errx(1, "Expected a positive number of references to keep for --screen, but '%s' was given.", optarg);
				}
				if (!strcmp(o, "screen-kmer")) {
					const unsigned long long v = positive_arg(optarg, 32);
					if (v < 4) errx(1, "Expected a k-mer length of 4 to 32 for --screen-kmer, but '%s' was given.", optarg);
					screen.k = (int)v, screen.k_given = 1;
				}
				if (!strcmp(o, "screen-scale")) {
					if (!(screen.scale = positive_arg(optarg, UINT64_MAX)))
						errx(1, "Expected a positive integer for --screen-scale, but '%s' was given.", optarg);
					screen.scale_given = 1;
				}
				if (!strcmp(o, "screen-min")) {
					if (!(screen.min = (uint32_t)positive_arg(optarg, UINT32_MAX)))
						errx(1, "Expected a positive integer for --screen-min, but '%s' was given.", optarg);
					screen.min_given = 1;
				}
				if (!strcmp(o, "screen-report")) screen.report_path = optarg;
				if (!strcmp(o, "reference-list")) rect = 1, read_file_of_filenames(optarg, &ref_files);
				if (!strcmp(o, "reference")) rect = 1, push_name(&ref_files, optarg);
				if (!strcmp(o, "progress")) {
					if (!optarg || !strcasecmp(optarg, "always")) progress = P_ALWAYS;
					else if (!strcasecmp(optarg, "auto")) progress = P_AUTO;
					else if (!strcasecmp(optarg, "never")) progress = P_NEVER;
					else
						warnx("invalid argument to --progress '%s'. Expected one of 'auto', 'always', or "
							  "'never'.", optarg);
				}
				break;
			}
			case 'h': usage(EXIT_SUCCESS); break;
			case 'v': verbose++; break;
			case 'l': opts.low_memory = 1; break;
			case 'j': join = 1; break;
			case 'p': {
				errno = 0;
				char *end;
				double v = strtod(optarg, &end);
				if (errno || end == optarg || *end) {
					soft_warnx("Expected a floating point number for -p argument, but '%s' was given. "
							   "Skipping argument.", optarg);
				} else if (v <= 0.0 || v >= 1.0) {
					soft_warnx("A probability should be a value between 0 and 1, exclusive; Ignoring -p %f "
							   "argument.", v);
				} else {
					opts.p_value = v;
				}
				break;
			}
			case 't': {
				errno = 0;
				char *end;
				unsigned long t = strtoul(optarg, &end, 10);
				if (errno || end == optarg || *end) {
					warnx("Expected a number for -t argument, but '%s' was given. Ignoring -t argument.", optarg);
				} else if (procs > 0 && t > (unsigned long)procs) {
					warnx("The number of threads to be used, is greater than the number of available "
						  "processors; Ignoring -t %lu argument.", t);
				} else if (t > 0) {
					opts.host_threads = (int)t;
				}
				break;
			}
			case 'b': {
				errno = 0;
				char *end;
				unsigned long b = strtoul(optarg, &end, 10);
				if (errno || end == optarg || *end || b == 0) {
					soft_warnx("Expected a positive number for -b argument, but '%s' was given. Ignoring -b "
							   "argument.", optarg);
				} else {
					bootstrap = b - 1; /* -b N prints N matrices in total, src/andi.c:198 */
					bootstrap_given = 1;
				}
				break;
			}
			case 'm':
				if (!strcasecmp(optarg, "RAW")) opts.model = ANDI_M_RAW;
				else if (!strcasecmp(optarg, "JC")) opts.model = ANDI_M_JC;
				else if (!strcasecmp(optarg, "KIMURA")) opts.model = ANDI_M_KIMURA;
				else if (!strcasecmp(optarg, "LOGDET")) opts.model = ANDI_M_LOGDET;
				else if (!strcasecmp(optarg, "ANI")) opts.model = ANDI_M_ANI;
				else soft_warnx("Ignoring argument for --model. Expected Raw, JC, Kimura, LogDet or ANI");
				break;
			default: usage(EXIT_FAILURE);
		}
	}
	for (int i = optind; i < argc; i++) push_name(&files, argv[i]);
	if (rect && bootstrap_given) errx(1, "Bootstrapping (-b) is not available together with --reference or --reference-list.");
	int any_out = 0;
	for (int k = 0; k < OUT_COUNT; k++) {
		if (!outs[k].path) continue;
		any_out = 1;
		if (rect) errx(1, "%s", outs[k].with_reference);
		if (!bootstrap && outs[k].without_bootstrap) errx(1, "%s", outs[k].without_bootstrap);
	}
	if (clus.dendro_path && rect) errx(1, "A dendrogram (--dendrogram) is" WITH_REFERENCE);
	if (clus.clusters_path && rect) errx(1, "Clusters (--clusters) are" WITH_REFERENCE);
	if (clus.dendro_path && trees_only) errx(1, "A dendrogram (--dendrogram) is not available together with --trees-only: there are no matrices to cluster.");
	if (clus.clusters_path && trees_only) errx(1, "Clusters (--clusters) are not available together with --trees-only: there are no matrices to cluster.");
	if (dlt.path && rect) errx(1, "Tree-likeness scores (--delta) are" WITH_REFERENCE);
	if (rootopt.report_path && !rootopt.on) errx(1, "A root report (--root-report) needs a rooting method: give --root=mad or --root=midpoint.");
	if (cmpl.on && trees_only)
		errx(1, "Missing distances (--complete) are not derived together with --trees-only: the bootstrap matrices stay on the GPU.");
	if (lengths_ols && trees_only)
		errx(1, "Branch lengths (--lengths=ols) are not refit together with --trees-only: the bootstrap matrices stay on the GPU.");
	if (fitopt.path && rect) errx(1, "A fit report (--fit) is" WITH_REFERENCE);
	if (refopt.on && trees_only)
		errx(1, "Trees (--refine=bnni) are not refined together with --trees-only: the bootstrap matrices stay on the GPU.");
	if (refopt.report_path && !refopt.on) errx(1, "A refinement report (--refine-report) needs --refine=bnni.");
	if (refopt.moves_arg && !refopt.on) errx(1, "The moves of the refinement (--refine-moves) need --refine=bnni.");
	if (refopt.tol_arg) {
		errno = 0;
		char *end;
		refopt.tol = strtod(refopt.tol_arg, &end);
		if (errno || end == refopt.tol_arg || *end || !(refopt.tol >= 0.0))
			errx(1, "Expected a number that is not negative for --refine-tol, but '%s' was given.", refopt.tol_arg);
	}
	if (clus.clusters_path && !clus.have_threshold) errx(1, "Clusters (--clusters) need a threshold: give --threshold=T.");
	if (clus.have_threshold && !clus.clusters_path) errx(1, "A threshold (--threshold) needs somewhere to go: give --clusters=FILE.");
	if (place.path && !rect) errx(1, "Placement (--place) needs references to place on: give --reference=FILE or --reference-list=FILE.");
	if (place.path && !place.backbone_path) errx(1, "Placement (--place) needs the tree of the references: give --backbone=FILE.");
	if (place.backbone_path && !place.path) errx(1, "A backbone tree (--backbone) needs somewhere to go: give --place=FILE.");
	if (screen_given && !rect) errx(1, "A screen (--screen) needs references to choose from: give --reference=FILE or --reference-list=FILE.");
	if (!screen_given && (screen.k_given || screen.scale_given || screen.min_given || screen.report_path))
		errx(1, "The options --screen-kmer, --screen-scale, --screen-min and --screen-report need a screen: give --screen=K.");
	if (trees_only && !bootstrap) errx(1, "Trees without matrices (--trees-only) need bootstrap replicates: give -b N with N of at least 2.");
	if (trees_only && !any_out)
		errx(1, "Trees without matrices (--trees-only) need somewhere to go: give at least one of --tree, --support, --consensus, --transfer.");
	if (rogues.path && rect) errx(1, "Rogue genomes (--rogues) are" WITH_REFERENCE);
	if (rogues.path && !bootstrap) errx(1, "Rogue genomes (--rogues) need" NEEDS_B);
	if (rogues.cutoff_arg && !rogues.path) errx(1, "A cutoff (--rogue-cutoff) needs somewhere to go: give --rogues=FILE.");
	if (rogues.cutoff_arg) {
		errno = 0;
		char *end;
		rogues.cutoff = strtod(rogues.cutoff_arg, &end);
		if (errno || end == rogues.cutoff_arg || *end || !(rogues.cutoff >= 0.0 && rogues.cutoff <= 1.0))
			errx(1, "Expected a number from 0 to 1 for --rogue-cutoff, but '%s' was given.", rogues.cutoff_arg);
	}
	for (int k = 0; k < OUT_COUNT; k++)
		if (outs[k].path && !(outs[k].f = fopen(outs[k].path, "w"))) err(1, "%s", outs[k].path);
	if (rogues.path && !(rogues.f = fopen(rogues.path, "w"))) err(1, "%s", rogues.path);
	if (cmpl.report_path && !(cmpl.rf = fopen(cmpl.report_path, "w"))) err(1, "%s", cmpl.report_path);
	if (dlt.path && !(dlt.f = fopen(dlt.path, "w"))) err(1, "%s", dlt.path);
	if (fitopt.path && !(fitopt.f = fopen(fitopt.path, "w"))) err(1, "%s", fitopt.path);
	if (refopt.report_path && !(refopt.rf = fopen(refopt.report_path, "w"))) err(1, "%s", refopt.report_path);
	if (rootopt.report_path) {
		if (!(rootopt.rf = fopen(rootopt.report_path, "w"))) err(1, "%s", rootopt.report_path);
		fputs("#method\tedge\tdistal\tlength\tscore\tambiguity\tpairs\n", rootopt.rf);
	}
	if (clus.dendro_path && !(clus.df = fopen(clus.dendro_path, "w"))) err(1, "%s", clus.dendro_path);
	if (clus.clusters_path && !(clus.cf = fopen(clus.clusters_path, "w"))) err(1, "%s", clus.clusters_path);
	if (place.path && !(place.f = fopen(place.path, "w"))) err(1, "%s", place.path);
	if (screen.report_path && !(screen.rf = fopen(screen.report_path, "w"))) err(1, "%s", screen.report_path);
	tree.device_for_ctx = clus.device_for_ctx = opts.device;
	if (join && files.n == 0) errx(1, "In join mode at least one filename needs to be supplied.");
	if (files.n < (size_t)(join && !rect ? 2 : 1)) {
		if (isatty(STDIN_FILENO)) usage(EXIT_FAILURE);
		push_name(&files, "-");
	}

	/* ANDI_HIP_CLI_TRACE=1: where the wall time goes -- reading the input, the matrix, printing it (stderr; scripts/full_size.py --cli) */
	if (progress == P_AUTO && rect) progress = isatty(STDERR_FILENO) ? P_ALWAYS : P_NEVER;
	if (rect) return run_rect(&ref_files, &files, join, verbose, truncate, progress == P_ALWAYS, &opts, &place, &screen);
	const int cli_trace = getenv("ANDI_HIP_CLI_TRACE") != NULL;
	struct timespec ts0, ts1, ts2, ts3;
	clock_gettime(CLOCK_MONOTONIC, &ts0);
	genome_list all = {0};
	read_all_files(files.v, files.n, join, opts.host_threads, &all);
	clock_gettime(CLOCK_MONOTONIC, &ts1);
	const size_t n = all.n;
	if (n < 2)
		errx(1, "I am truly sorry, but with less than two sequences (%zu given) there is nothing to compare.", n);
	check_genomes(&all, NULL, truncate);

	if (progress == P_AUTO) progress = isatty(STDERR_FILENO) ? P_ALWAYS : P_NEVER;
	if (progress == P_ALWAYS) {
		progress_n = n;
		opts.progress = progress_cb;
		progress_cb(0, n * n - n, NULL);
	}

	/* calculate_distances, src/process.c:230-270 */
	if (SIZE_MAX / sizeof(andi_hip_model) / n < n) errx(1, "Comparison is limited to fewer sequences (%zu given).", n);
	andi_hip_model *M = malloc(n * n * sizeof *M);
	if (!M) err(errno, "Could not allocate enough memory for the comparison matrix. Try using --join or --low-memory.");
	andi_hip_seq *in = seq_array(&all);
	char msg[512];
	if (andi_hip_dist_matrix(M, in, n, &opts, msg, sizeof msg)) errx(1, "%s", msg);
	if (progress == P_ALWAYS) fprintf(stderr, ", done.\n");
	clock_gettime(CLOCK_MONOTONIC, &ts2);

	const char **names = name_array(all.v, n);
	print_distances(M, NULL, names, n, NULL, 0, opts.model, verbose >= 2, truncate, 1);
	if (cmpl.rf) complete_report(&tree, M, names, n, opts.model, truncate);
	if (dlt.f) delta_report(&tree, M, names, n, opts.model, truncate);
	if (fitopt.f) fit_report(&tree, M, all.v, names, n, opts.model, truncate);
	if (tree.o->f) write_tree(&tree, M, all.v, names, n, opts.model, truncate, 1);
	if (clus.df || clus.cf) cluster_point(&clus, M, names, n, opts.model, truncate);
	if (cli_trace) {
		fflush(stdout);
		clock_gettime(CLOCK_MONOTONIC, &ts3);
#define SECS(a, b) ((double)((b).tv_sec - (a).tv_sec) + 1e-9 * (double)((b).tv_nsec - (a).tv_nsec))
		size_t nt_total = 0;
		for (size_t i = 0; i < n; i++) nt_total += all.v[i].len;
		fprintf(stderr, "andi-hip trace: %zu sequences, %zu nucleotides from %zu files: ingest %.3f s, matrix %.3f s, print %.3f s\n", n, nt_total,
				files.n, SECS(ts0, ts1), SECS(ts1, ts2), SECS(ts2, ts3));
	}
	if (verbose) { /* print_coverages, src/io.c:329-338 */
		printf("\nCoverage:\n");
		for (size_t i = 0; i < n; i++) {
			for (size_t j = 0; j < n; j++) printf("%1.4e ", andi_hip_model_coverage(&M[i * n + j]));
			printf("\n");
		}
	}
	if (bootstrap) { /* calculate_bootstrap, src/process.c:289-321 */
		andi_hip_ctx *ctx = NULL;
		/* the replicates are drawn, printed and handed to the trees in chunks of at most 1 GiB of models (at least one
		 * replicate): a draw depends on (seed, replicate, i, j) alone, so the output does not depend on the chunks.
		 * ANDI_HIP_BOOT_CHUNK=k: chunks of k replicates (the tests').  Under --trees-only nothing is drawn here at all. */
		size_t chunk = ((size_t)1 << 30) / (n * n * sizeof(andi_hip_model));
		if (trees_only) chunk = bootstrap;
		if (getenv("ANDI_HIP_BOOT_CHUNK") && strtoull(getenv("ANDI_HIP_BOOT_CHUNK"), NULL, 10) > 0)
			chunk = strtoull(getenv("ANDI_HIP_BOOT_CHUNK"), NULL, 10);
		chunk = chunk < 1 ? 1 : chunk > bootstrap ? bootstrap : chunk;
		andi_hip_model *B = trees_only ? NULL : malloc(chunk * n * n * sizeof *B);
		/* the reference seeds its generator from the clock; ANDI_HIP_SEED=k draws the same matrices on every run */
		const uint64_t seed = getenv("ANDI_HIP_SEED") ? strtoull(getenv("ANDI_HIP_SEED"), NULL, 10) : (uint64_t)time(NULL);
		const int trees = outs[OUT_SUPPORT].f || outs[OUT_CONSENSUS].f || outs[OUT_TRANSFER].f || rogues.f || trees_only;
		support_state st;
		int begun = 0, ok = 1;
		if ((!trees_only && !B) || andi_hip_ctx_create(&ctx, opts.device, msg, sizeof msg)) ok = 0;
		for (unsigned long first = 0; ok && first < bootstrap; first += chunk) {
			const size_t c = bootstrap - first < chunk ? bootstrap - first : chunk;
			if (!trees_only) {
				if (andi_hip_bootstrap_range(ctx, M, n, seed, first, c, B)) {
					ok = 0;
					break;
				}
				for (size_t b = 0; b < c; b++) {
					print_distances(B + b * n * n, NULL, names, n, NULL, 0, opts.model, verbose >= 2, truncate, 0);
					if (tree.o->f && !trees) write_tree(&tree, B + b * n * n, all.v, names, n, opts.model, truncate, (int)(first + b) + 2);
				}
			}
			if (clus.df || clus.cf) cluster_chunk(&clus, B, first, c, all.v, names, n, opts.model, truncate);
			if (!trees) continue;
			if (!begun) {
				const boot_run run = {ctx, all.v, names, n, bootstrap, opts.model, truncate, trees_only, seed, &rogues, tree.method};
				support_begin(&st, outs, &run, M);
			}
			begun = 1;
			support_chunk(&st, first, c, B, M);
		}
		if (!ok) soft_warnx("Bootstrapping failed.");
		if (begun) support_end(&st, ok);
		if (clus.df || clus.cf) cluster_end(&clus, names, n, truncate, bootstrap, ok);
		if (ctx) andi_hip_ctx_destroy(ctx);
		free(B);
	}
	if (!bootstrap && (clus.df || clus.cf)) cluster_end(&clus, names, n, truncate, 0, 1);
	if (tree.ctx) andi_hip_ctx_destroy(tree.ctx);
	for (int k = 0; k < OUT_COUNT; k++)
		if (outs[k].f && fclose(outs[k].f)) err(1, "%s", outs[k].path);
	if (rogues.f && fclose(rogues.f)) err(1, "%s", rogues.path);
	if (cmpl.rf && fclose(cmpl.rf)) err(1, "%s", cmpl.report_path);
	if (dlt.f && fclose(dlt.f)) err(1, "%s", dlt.path);
	if (fitopt.f && fclose(fitopt.f)) err(1, "%s", fitopt.path);
	if (refopt.rf && fclose(refopt.rf)) err(1, "%s", refopt.report_path);
	if (rootopt.rf && fclose(rootopt.rf)) err(1, "%s", rootopt.report_path);
	free(M);
	free(in);
	free(names);
	return soft_error ? EXIT_FAILURE : EXIT_SUCCESS;
}
