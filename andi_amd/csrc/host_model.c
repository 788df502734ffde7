/*
 * host_model.c — what happens to the integer counts after the device scan:
 * symmetrisation, distance estimators and the PHYLIP printer.  Kept on the
 * host so RAW/JC/Kimura distances are bit-identical to the reference given
 * identical counts.  Follows src/model.c:39-210 and
 * src/io.c:246-338.
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "andi_hip.h"

/* cell index = 4*from + to, A C G T = 0 1 2 3 (src/model.h:14-32) */
#define CELL(f, t) (4 * (f) + (t))
enum { nA, nC, nG, nT };

/* model_average, src/model.c:39-46 — element-wise sum, seq_len included */
andi_hip_model andi_hip_model_average(const andi_hip_model *a, const andi_hip_model *b) {
	andi_hip_model r = *a;
	for (int k = 0; k < 16; k++) r.counts[k] += b->counts[k];
	r.seq_len += b->seq_len;
	return r;
}

/* model_total, src/model.c:54-60 */
static size_t total(const andi_hip_model *m) {
	size_t t = 0;
	for (int k = 0; k < 16; k++) t += m->counts[k];
	return t;
}

/* model_coverage, src/model.c:68-73 */
double andi_hip_model_coverage(const andi_hip_model *m) {
	return (double)total(m) / (double)m->seq_len;
}

static size_t off_diagonal(const andi_hip_model *m) {
	size_t t = 0;
	for (int f = 0; f < 4; f++)
		for (int g = 0; g < 4; g++)
			if (f != g) t += m->counts[CELL(f, g)];
	return t;
}

/* estimate_RAW, src/model.c:81-92 */
static double raw(const andi_hip_model *m) {
	size_t nucl = total(m);
	size_t snps = off_diagonal(m);
	if (nucl <= 3) return NAN;
	return (double)snps / (double)nucl;
}

/* estimate_JC, src/model.c:100-106 */
static double jc(const andi_hip_model *m) {
	double d = raw(m);
	d = -0.75 * log(1.0 - (4.0 / 3.0) * d);
	return d <= 0.0 ? 0.0 : d;
}

/* estimate_KIMURA, src/model.c:113-127 */
static double kimura(const andi_hip_model *m) {
	size_t nucl = total(m);
	size_t ts = (size_t)m->counts[CELL(nA, nG)] + m->counts[CELL(nG, nA)] +
				m->counts[CELL(nC, nT)] + m->counts[CELL(nT, nC)];
	size_t tv = off_diagonal(m) - ts;
	double P = (double)ts / (double)nucl;
	double Q = (double)tv / (double)nucl;
	double w = 1.0 - 2.0 * P - Q;
	double d = -0.25 * log((1.0 - 2.0 * Q) * w * w);
	return d <= 0.0 ? 0.0 : d;
}

/* estimate_LOGDET, src/model.c:155-199.  The 4x4 determinant is expanded in
 * the same term order as the reference so the double matches. */
static double logdet(const andi_hip_model *m) {
	double nucl = (double)total(m);
	double P[16];
	for (int k = 0; k < 16; k++) P[k] = m->counts[k] / nucl;

	double lg = 0.0;
	for (int f = 0; f < 4; f++) {
		size_t s = 0;
		for (int g = 0; g < 4; g++) s += m->counts[CELL(f, g)];
		double term = log(s / nucl);
		lg = f ? lg + term : term;
	}
	for (int g = 0; g < 4; g++) {
		size_t s = 0;
		for (int f = 0; f < 4; f++) s += m->counts[CELL(f, g)];
		lg = lg + log(s / nucl);
	}

#define p(f, g) P[CELL(n##f, n##g)]
	double det = p(A, A) * p(C, C) * (p(G, G) * p(T, T) - p(T, G) * p(G, T)) -
				 p(A, A) * p(C, G) * (p(G, C) * p(T, T) - p(T, C) * p(G, T)) +
				 p(A, A) * p(C, T) * (p(G, C) * p(T, G) - p(T, C) * p(G, G)) -

				 p(A, C) * p(C, A) * (p(G, G) * p(T, T) - p(T, G) * p(G, T)) +
				 p(A, C) * p(C, G) * (p(G, A) * p(T, T) - p(T, A) * p(G, T)) -
				 p(A, C) * p(C, T) * (p(G, A) * p(T, G) - p(T, A) * p(G, G)) +

				 p(A, G) * p(C, A) * (p(G, C) * p(T, T) - p(T, C) * p(G, T)) -
				 p(A, G) * p(C, C) * (p(G, A) * p(T, T) - p(T, A) * p(G, T)) +
				 p(A, G) * p(C, T) * (p(G, A) * p(T, C) - p(T, A) * p(G, C)) -

				 p(A, T) * p(C, A) * (p(G, C) * p(T, G) - p(T, C) * p(G, G)) +
				 p(A, T) * p(C, C) * (p(G, A) * p(T, G) - p(T, A) * p(G, G)) -
				 p(A, T) * p(C, G) * (p(G, A) * p(T, C) - p(T, A) * p(G, C));
#undef p
	double d = -0.25 * (log(det) - 0.5 * lg);
	return d <= 0.0 ? 0.0 : d;
}

/* estimate_ANI, src/model.c:207-210 */
static double ani(const andi_hip_model *m) {
	return (1.0 - raw(m)) * 100;
}

/* dispatch as in print_distances, src/io.c:259-268 (JC is the default) */
double andi_hip_estimate(const andi_hip_model *m, int model) {
	switch (model) {
		case ANDI_M_RAW: return raw(m);
		case ANDI_M_KIMURA: return kimura(m);
		case ANDI_M_LOGDET: return logdet(m);
		case ANDI_M_ANI: return ani(m);
		default: return jc(m);
	}
}

typedef struct {
	char *buf;
	size_t cap, len;
} sink;

static void put(sink *s, const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	size_t room = s->len < s->cap ? s->cap - s->len : 0;
	int w = vsnprintf(room ? s->buf + s->len : NULL, room, fmt, ap);
	va_end(ap);
	if (w > 0) s->len += (size_t)w;
}

/* print_distances, src/io.c:246-322 — same averaging rule, scientific-notation
 * switch, warnings and row format, written into buffers instead of stdout /
 * stderr so the caller decides where they go.
 *
 * Row-parallel (BASELINE's config 3 is a 3085 x 3085 matrix: 9.5 M estimates and as many printf conversions, seconds on one
 * thread beside a 13 s matrix): the rows are dealt to a pool of threads twice -- first the distances, the warnings of
 * each row and whether any distance calls for the scientific format (a property of the WHOLE matrix, src/io.c:283), then
 * the rows' text -- and put together in row order, so the bytes are those of the sequential loop. */
typedef struct {
	const andi_hip_model *M;
	const char *const *names;
	size_t n;
	int model, extra_verbose, truncate_names, warnings;
	double *D;
	sink *row_warn, *row_text; /* one growing buffer per row */
	int *row_flags, *row_sci;
	int scientific;
	int phase;
	size_t next; /* atomic: the next block of rows */
} fmt_job;

static void put_grow(sink *s, const char *fmt, ...) { /* a sink that owns its buffer */
	for (;;) {
		va_list ap;
		va_start(ap, fmt);
		const size_t room = s->cap - s->len;
		const int w = vsnprintf(room ? s->buf + s->len : NULL, room, fmt, ap);
		va_end(ap);
		if (w < 0) return;
		if ((size_t)w < room) {
			s->len += (size_t)w;
			return;
		}
		s->cap = 2 * s->cap + (size_t)w + 64;
		s->buf = realloc(s->buf, s->cap);
		if (!s->buf) abort();
	}
}

/* the distance print_distances prints for cell (i, j): model_average of both directions (M[i][j] alone under extra_verbose),
 * +0.0 on the diagonal -- what the formatter prints and andi_hip_distances returns */
static double cell_distance(const andi_hip_model *M, size_t n, size_t i, size_t j, int model, int extra_verbose) {
	if (i == j) return 0.0;
	andi_hip_model datum = M[i * n + j];
	if (!extra_verbose) datum = andi_hip_model_average(&M[i * n + j], &M[j * n + i]);
	return andi_hip_estimate(&datum, model);
}

static void fmt_rows(fmt_job *job, size_t i0, size_t i1) {
	const andi_hip_model *M = job->M;
	const size_t n = job->n;
	for (size_t i = i0; i < i1; i++) {
		if (job->phase == 2) { /* andi_hip_distances: the distances alone */
			for (size_t j = 0; j < n; j++) job->D[i * n + j] = cell_distance(M, n, i, j, job->model, 0);
		} else if (job->phase == 0) {
			int flags = 0, sci = 0;
			sink *w = &job->row_warn[i];
			for (size_t j = 0; j < n; j++) {
				double d = job->D[i * n + j] = cell_distance(M, n, i, j, job->model, job->extra_verbose);
				if (d > 0 && d < 0.001) sci = 1;
				if (isnan(d) && job->warnings) {
					flags |= 1;
					put_grow(w,
							 "For the two sequences '%s' and '%s' the distance computation failed and "
							 "is reported as nan. Please refer to the documentation for further "
							 "details.\n",
							 job->names[i], job->names[j]);
				}
				if (!isnan(d) && i < j && job->warnings) {
					double c1 = andi_hip_model_coverage(&M[i * n + j]);
					double c2 = andi_hip_model_coverage(&M[j * n + i]);
					if (c1 < 0.2 || c2 < 0.2) {
						flags |= 2;
						put_grow(w,
								 "For the two sequences '%s' and '%s' very little homology was found "
								 "(%f and %f, respectively).\n",
								 job->names[i], job->names[j], c1, c2);
					}
				}
			}
			job->row_flags[i] = flags, job->row_sci[i] = sci;
		} else {
			sink *o = &job->row_text[i];
			put_grow(o, job->truncate_names ? "%-10.10s" : "%-10s", job->names[i]);
			const char *f = job->scientific ? " %1.4e" : " %1.4f";
			for (size_t j = 0; j < n; j++) put_grow(o, f, job->D[i * n + j]);
			put_grow(o, "\n");
		}
	}
}

#include <pthread.h>
#include <unistd.h>
static void *fmt_worker(void *arg) {
	fmt_job *job = arg;
	for (;;) {
		const size_t i0 = __atomic_fetch_add(&job->next, 16, __ATOMIC_RELAXED);
		if (i0 >= job->n) break;
		fmt_rows(job, i0, i0 + 16 < job->n ? i0 + 16 : job->n);
	}
	return NULL;
}

static void fmt_run(fmt_job *job, int phase) {
	job->phase = phase, job->next = 0;
	long procs = sysconf(_SC_NPROCESSORS_ONLN);
	size_t nt = procs > 0 ? (size_t)procs : 1;
	if (nt > 32) nt = 32;
	if (nt > job->n / 64 + 1) nt = job->n / 64 + 1; /* (small matrices: the calling thread alone) */
	pthread_t tid[32];
	size_t started = 0;
	for (size_t t = 1; t < nt; t++)
		if (pthread_create(&tid[started], NULL, fmt_worker, job) == 0) started++;
	fmt_worker(job);
	for (size_t t = 0; t < started; t++) pthread_join(tid[t], NULL);
}

size_t andi_hip_format_distances(const andi_hip_model *M, const char *const *names, size_t n,
								 int model, int extra_verbose, int truncate_names, int warnings,
								 char *out, size_t cap, char *warnbuf, size_t warncap,
								 int *warn_flags) {
	fmt_job job = {M, names, n, model, extra_verbose, truncate_names, warnings, NULL, NULL, NULL, NULL, NULL, 0, 0, 0};
	job.D = malloc((n ? n * n : 1) * sizeof *job.D);
	job.row_warn = calloc(n ? n : 1, sizeof *job.row_warn);
	job.row_text = calloc(n ? n : 1, sizeof *job.row_text);
	job.row_flags = calloc(n ? n : 1, sizeof *job.row_flags);
	job.row_sci = calloc(n ? n : 1, sizeof *job.row_sci);
	if (!job.D || !job.row_warn || !job.row_text || !job.row_flags || !job.row_sci) {
		free(job.D), free(job.row_warn), free(job.row_text), free(job.row_flags), free(job.row_sci);
		return 0;
	}
	sink o = {out, cap, 0}, w = {warnbuf, warncap, 0};
	int flags = 0;

	fmt_run(&job, 0);
	for (size_t i = 0; i < n; i++) job.scientific |= job.row_sci[i], flags |= job.row_flags[i];
	fmt_run(&job, 1);

	put(&o, "%zu\n", n);
	for (size_t i = 0; i < n; i++) {
		const sink *r = &job.row_text[i], *rw = &job.row_warn[i];
		if (o.len < o.cap && r->len) memcpy(o.buf + o.len, r->buf, r->len < o.cap - o.len ? r->len : o.cap - o.len);
		o.len += r->len;
		if (w.len < w.cap && rw->len) memcpy(w.buf + w.len, rw->buf, rw->len < w.cap - w.len ? rw->len : w.cap - w.len);
		w.len += rw->len;
		free(r->buf), free(rw->buf);
	}
	free(job.D), free(job.row_warn), free(job.row_text), free(job.row_flags), free(job.row_sci);
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	if (warnbuf && warncap) warnbuf[w.len < warncap ? w.len : warncap - 1] = '\0';
	if (warn_flags) *warn_flags = flags;
	return o.len;
}

int andi_hip_distances(const andi_hip_model *M, size_t n, int model, double *D) {
	if (!M || !D) return 1;
	fmt_job job = {M, NULL, n, model, 0, 0, 0, D, NULL, NULL, NULL, NULL, 0, 0, 0};
	fmt_run(&job, 2);
	return 0;
}

/* The query-versus-reference table (andi_hip_dist_rect's two cross blocks, include/andi_hip.h): query q is row nr + q of
 * refs ++ queries, reference r is column r, so a cell is what fmt_rows computes for that pair of the union --
 * model_average(M[i][j], M[j][i]) with M[i][j] = MQR[q][r], M[j][i] = MRQ[r][q] (extra_verbose: MQR[q][r] alone) -- and the
 * low-coverage check is the union's for i = r < j = nr + q.  One thread: the table is nq x nr, not n x n. */
size_t andi_hip_format_distances_rect(const andi_hip_model *MRQ, const andi_hip_model *MQR,
									  const char *const *ref_names, size_t nr, const char *const *query_names, size_t nq,
									  int model, int extra_verbose, int truncate_names, int warnings,
									  char *out, size_t cap, char *warnbuf, size_t warncap, int *warn_flags) {
	double *D = malloc((nq && nr ? nq * nr : 1) * sizeof *D);
	if (!D) return 0;
	sink o = {out, cap, 0}, w = {warnbuf, warncap, 0};
	int flags = 0, scientific = 0;
	for (size_t q = 0; q < nq; q++)
		for (size_t r = 0; r < nr; r++) {
			const andi_hip_model *qr = &MQR[q * nr + r], *rq = &MRQ[r * nq + q];
			andi_hip_model datum = extra_verbose ? *qr : andi_hip_model_average(qr, rq);
			const double d = D[q * nr + r] = andi_hip_estimate(&datum, model);
			if (d > 0 && d < 0.001) scientific = 1;
			if (!warnings) continue;
			if (isnan(d)) {
				flags |= 1;
				put(&w,
					"For the two sequences '%s' and '%s' the distance computation failed and "
					"is reported as nan. Please refer to the documentation for further "
					"details.\n",
					query_names[q], ref_names[r]);
			}
			andi_hip_model upper = extra_verbose ? *rq : datum; /* (the union's row r, column nr + q) */
			if (!isnan(andi_hip_estimate(&upper, model))) {
				const double c1 = andi_hip_model_coverage(rq), c2 = andi_hip_model_coverage(qr);
				if (c1 < 0.2 || c2 < 0.2) {
					flags |= 2;
					put(&w,
						"For the two sequences '%s' and '%s' very little homology was found "
						"(%f and %f, respectively).\n",
						ref_names[r], query_names[q], c1, c2);
				}
			}
		}
	put(&o, "%zu %zu\n", nq, nr);
	put(&o, "%10s", "");
	for (size_t r = 0; r < nr; r++) put(&o, truncate_names ? " %.10s" : " %s", ref_names[r]);
	put(&o, "\n");
	const char *f = scientific ? " %1.4e" : " %1.4f";
	for (size_t q = 0; q < nq; q++) {
		put(&o, truncate_names ? "%-10.10s" : "%-10s", query_names[q]);
		for (size_t r = 0; r < nr; r++) put(&o, f, D[q * nr + r]);
		put(&o, "\n");
	}
	free(D);
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	if (warnbuf && warncap) warnbuf[w.len < warncap ? w.len : warncap - 1] = '\0';
	if (warn_flags) *warn_flags = flags;
	return o.len;
}

/* a leaf of the Newick text: the name (cut to ten characters under truncate), quoted if it holds a character Newick
 * gives a meaning to */
static void put_leaf(sink *o, const char *name, int truncate) {
	const size_t len = truncate ? strnlen(name, 10) : strlen(name);
	int quote = 0;
	for (size_t k = 0; k < len; k++) quote |= strchr(" \t()[]':;,", name[k]) != NULL && name[k] != '\0';
	if (!quote) {
		put(o, "%.*s", (int)len, name);
		return;
	}
	put(o, "'");
	for (size_t k = 0; k < len; k++) put(o, name[k] == '\'' ? "''" : "%c", name[k]);
	put(o, "'");
}

/* andi_hip_nj's records as Newick text (include/andi_hip.h), depth first with a stack of its own instead of recursion;
 * the label behind the ")" of pair record s is support[s] if support is given, else the transfer bootstrap expectation
 * from depth, transfer and used if depth is given, else none; edge_nums: "{v}" behind the length of the branch above node
 * v (jplace's edge numbers, andi_hip_format_jplace) */
static size_t format_newick(const andi_hip_nj_join *J, const uint32_t *support, const uint32_t *depth,
							const uint64_t *transfer, size_t used, size_t n, const char *const *names, int truncate_names,
							int edge_nums, char *out, size_t cap) {
	sink o = {out, cap, 0};
	if (out && cap) out[0] = '\0';
	if (!J || !names || n < 2) return 0;
	const size_t pairs = n == 2 ? 0 : n - 3, root = n == 2 ? 0 : n - 3; /* records 0 .. pairs-1 are the pair joins */
	for (size_t s = 0; s <= root; s++) { /* every child a leaf or an earlier record's node: the walk below ends */
		const int32_t ch[3] = {J[s].a, J[s].b, J[s].c};
		const int kids = s == root && n > 2 ? 3 : 2;
		for (int k = 0; k < kids; k++)
			if (ch[k] < 0 || (size_t)ch[k] >= n + s || (s == root && (size_t)ch[k] >= n + pairs)) return 0;
	}
	typedef struct {
		size_t rec; /* record of this node */
		int next;   /* its next child */
		double len; /* its own branch length */
	} frame;
	frame *stack = malloc((pairs + 1) * sizeof *stack);
	if (!stack) return 0;
	size_t top = 0;
	stack[top++] = (frame){root, 0, 0.0};
	put(&o, "(");
	while (top) {
		frame *f = &stack[top - 1];
		const andi_hip_nj_join *r = &J[f->rec];
		const int kids = f->rec == root && n > 2 ? 3 : 2;
		if (f->next == kids) {
			const double len = f->len;
			const size_t rec = f->rec;
			top--;
			put(&o, ")");
			if (top && support) put(&o, "%u", (unsigned)support[rec]);
			else if (top && depth) put(&o, "%.6g", 1.0 - (double)transfer[rec] / ((double)used * (double)(depth[rec] - 1)));
			if (top) put(&o, ":%.8g", len);
			else put(&o, ";\n");
			if (top && edge_nums) put(&o, "{%zu}", n + rec);
			continue;
		}
		const int k = f->next++;
		if (k) put(&o, ",");
		const size_t child = (size_t)(k == 0 ? r->a : k == 1 ? r->b : r->c);
		const double len = k == 0 ? r->la : k == 1 ? r->lb : r->lc;
		if (child < n) {
			put_leaf(&o, names[child], truncate_names);
			put(&o, ":%.8g", len);
			if (edge_nums) put(&o, "{%zu}", child);
		} else {
			stack[top++] = (frame){child - n, 0, len};
			put(&o, "(");
		}
	}
	free(stack);
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	return o.len;
}

size_t andi_hip_format_newick_support(const andi_hip_nj_join *J, const uint32_t *support, size_t n,
									  const char *const *names, int truncate_names, char *out, size_t cap) {
	return format_newick(J, support, NULL, NULL, 0, n, names, truncate_names, 0, out, cap);
}

size_t andi_hip_format_newick(const andi_hip_nj_join *J, size_t n, const char *const *names, int truncate_names,
							  char *out, size_t cap) {
	return format_newick(J, NULL, NULL, NULL, 0, n, names, truncate_names, 0, out, cap);
}

size_t andi_hip_format_newick_transfer(const andi_hip_nj_join *J, const uint32_t *depth, const uint64_t *transfer,
									   size_t used, size_t n, const char *const *names, int truncate_names,
									   char *out, size_t cap) {
	if (out && cap) out[0] = '\0';
	if (!depth || !transfer || used == 0) return 0;
	for (size_t s = 0; s + 3 < n; s++)
		if (depth[s] < 2) return 0;
	return format_newick(J, NULL, depth, transfer, used, n, names, truncate_names, 0, out, cap);
}

/* the label of the edge above node v in a rooted text: that of pair record v - n, if there is one */
static void put_edge_label(sink *o, const char *const *labels, size_t n, size_t v) {
	if (labels && v >= n && v < 2 * n - 3 && labels[v - n]) put(o, "%s", labels[v - n]);
}

/* T(v) of andi_hip_format_newick_rooted: the subtree below node v with its label, without its length; the walk of
 * format_newick.  stack: room for n - 2 frames */
typedef struct {
	size_t rec;
	int next;
	double len;
} rooted_frame;
static void put_subtree(sink *o, const andi_hip_nj_join *J, size_t n, const char *const *names, int truncate_names,
						const char *const *labels, size_t v, rooted_frame *stack) {
	if (v < n) {
		put_leaf(o, names[v], truncate_names);
		return;
	}
	size_t top = 0;
	stack[top++] = (rooted_frame){v - n, 0, 0.0};
	put(o, "(");
	while (top) {
		rooted_frame *f = &stack[top - 1];
		const andi_hip_nj_join *r = &J[f->rec];
		if (f->next == 2) {
			const double len = f->len;
			const size_t rec = f->rec;
			top--;
			put(o, ")");
			put_edge_label(o, labels, n, n + rec);
			if (top) put(o, ":%.8g", len);
			continue;
		}
		const int k = f->next++;
		if (k) put(o, ",");
		const size_t child = (size_t)(k == 0 ? r->a : r->b);
		const double len = k == 0 ? r->la : r->lb;
		if (child < n) {
			put_leaf(o, names[child], truncate_names);
			put(o, ":%.8g", len);
		} else {
			stack[top++] = (rooted_frame){child - n, 0, len};
			put(o, "(");
		}
	}
}

size_t andi_hip_format_newick_rooted(const andi_hip_nj_join *J, size_t n, const char *const *names, int truncate_names,
									 int32_t edge, double distal, const char *const *labels, char *out, size_t cap) {
	sink o = {out, cap, 0};
	if (out && cap) out[0] = '\0';
	if (!J || !names || n < 3 || edge < 0 || (size_t)edge >= 2 * n - 3 || !isfinite(distal)) return 0;
	const size_t pairs = n - 3, E = 2 * n - 3, C = E;
	size_t *par = malloc(E * sizeof *par);
	double *len = malloc(E * sizeof *len);
	rooted_frame *stack = malloc((pairs + 1) * sizeof *stack);
	size_t *path = malloc((pairs + 2) * sizeof *path);
	size_t ret = 0;
	if (!par || !len || !stack || !path) goto done;
	for (size_t v = 0; v < E; v++) par[v] = (size_t)-1;
	for (size_t s = 0; s <= pairs; s++) { /* every child a leaf or an earlier record's node, and a child once */
		const int32_t ch[3] = {J[s].a, J[s].b, J[s].c};
		const double l[3] = {J[s].la, J[s].lb, J[s].lc};
		const int kids = s == pairs ? 3 : 2;
		for (int k = 0; k < kids; k++) {
			if (ch[k] < 0 || (size_t)ch[k] >= n + s || (size_t)ch[k] >= n + pairs || par[ch[k]] != (size_t)-1) goto done;
			par[ch[k]] = s == pairs ? C : n + s, len[ch[k]] = l[k];
		}
	}
	/* (2 * pairs + 3 = E children, none twice: every node has its parent) */
	const size_t v = (size_t)edge;
	size_t m = 0; /* the nodes from parent(edge) up to the centre */
	for (size_t q = par[v]; ; q = par[q]) {
		path[m++] = q;
		if (q == C) break;
	}
	put(&o, "(");
	put_subtree(&o, J, n, names, truncate_names, labels, v, stack);
	put(&o, ":%.8g,", distal);
	for (size_t j = 0; j < m; j++) { /* U(path[j]): its children but the one the path came through, then the level above */
		const size_t q = path[j], from = j ? path[j - 1] : v;
		const andi_hip_nj_join *r = &J[q == C ? pairs : q - n];
		const int kids = q == C ? 3 : 2;
		put(&o, "(");
		int first = 1;
		for (int k = 0; k < kids; k++) {
			const size_t child = (size_t)(k == 0 ? r->a : k == 1 ? r->b : r->c);
			if (child == from) continue;
			if (!first) put(&o, ",");
			first = 0;
			put_subtree(&o, J, n, names, truncate_names, labels, child, stack);
			put(&o, ":%.8g", len[child]);
		}
		if (j + 1 < m) put(&o, ",");
	}
	for (size_t j = m; j-- > 0;) {
		const size_t from = j ? path[j - 1] : v;
		put(&o, ")");
		put_edge_label(&o, labels, n, from);
		put(&o, ":%.8g", j ? len[from] : len[v] - distal);
	}
	put(&o, ");\n");
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	ret = o.len;
done:
	free(par), free(len), free(stack), free(path);
	if (!ret && out && cap) out[0] = '\0';
	return ret;
}

/* andi_hip_fit's lengths put into the records (include/andi_hip.h) */
int andi_hip_relength(const andi_hip_nj_join *J, size_t n, const double *len, andi_hip_nj_join *out) {
	if (!J || !len || !out || n < 3) return 1;
	const size_t pairs = n - 3;
	uint8_t *seen = calloc(n + pairs, 1);
	if (!seen) return 1;
	for (size_t s = 0; s <= pairs; s++) { /* every child a leaf or an earlier record's node, and a child once */
		const int32_t ch[3] = {J[s].a, J[s].b, J[s].c};
		const int kids = s == pairs ? 3 : 2;
		for (int k = 0; k < kids; k++) {
			if (ch[k] < 0 || (size_t)ch[k] >= n + s || (size_t)ch[k] >= n + pairs || seen[ch[k]]) {
				free(seen);
				return 1;
			}
			seen[ch[k]] = 1;
		}
	}
	free(seen);
	for (size_t s = 0; s <= pairs; s++) {
		andi_hip_nj_join r = J[s];
		r.la = len[r.a], r.lb = len[r.b];
		if (s == pairs) r.lc = len[r.c];
		out[s] = r;
	}
	return 0;
}

/* ------------------------------------------------------------------ */
/* The majority-rule consensus tree of a bootstrap (include/andi_hip.h) */
/* ------------------------------------------------------------------ */
#define NO_SPLIT 0xffffffffu

static uint32_t uf_find(uint32_t *uf, uint32_t x) { /* (path halving) */
	while (uf[x] != x) x = uf[x] = uf[uf[x]];
	return x;
}

static int cmp_u64(const void *a, const void *b) {
	const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
	return x < y ? -1 : x > y;
}

int andi_hip_consensus(const andi_hip_nj_join *reps, size_t n, size_t count, const uint8_t *skip, const uint32_t *ids,
					   size_t nsplits, const uint32_t *freq, const uint64_t *sets, andi_hip_cons_node *nodes, size_t *ninner) {
	if (!reps || !nodes || !ninner || count == 0 || n < 2 || n > 65535) return 1;
	const size_t S = n > 3 ? n - 3 : 0, nrec = n == 2 ? 1 : n - 2, W = (n + 63) / 64;
	if (S && (!ids || !freq || !sets || nsplits == 0)) return 1;
	size_t used = 0, m = 0;
	for (size_t k = 0; k < count; k++) used += !skip || !skip[k];
	if (used == 0) return 1;
	if (!S) nsplits = 0;

	/* the splits that enter: node_of[id] = the inner node of split id (0 ... m-1), or NO_SPLIT */
	int rc = 1;
	uint32_t *node_of = malloc((nsplits ? nsplits : 1) * sizeof *node_of);
	uint32_t *split_of = malloc((S ? S : 1) * sizeof *split_of), *occ = calloc(S ? S : 1, sizeof *occ);
	double *isum = calloc(S ? S : 1, sizeof *isum), *lsum = calloc(n, sizeof *lsum), *above = malloc((n + S) * sizeof *above);
	uint8_t *seen = malloc(n + S);
	uint64_t *order = malloc((S ? S : 1) * sizeof *order);
	uint32_t *uf = malloc(4 * n * sizeof *uf); /* the leaves' components: union-find, sizes, marks, the node on top */
	uint32_t *roots = malloc(n * sizeof *roots); /* the components of one set */
	if (!node_of || !split_of || !occ || !isum || !lsum || !above || !seen || !order || !uf || !roots) goto done;
	for (size_t id = 0; id < nsplits; id++) {
		node_of[id] = NO_SPLIT;
		if (2 * (uint64_t)freq[id] <= used) continue;
		if (m == S) goto done; /* (more than n - 3 majority splits: they cannot all be compatible) */
		split_of[m] = (uint32_t)id, node_of[id] = (uint32_t)m++;
	}

	/* the sums of the branch lengths, replicates in ascending order */
	for (size_t k = 0; k < count; k++) {
		if (skip && skip[k]) continue;
		const andi_hip_nj_join *R = reps + k * nrec;
		memset(seen, 0, n + S);
		for (size_t t = 0; t < nrec; t++) {
			const int32_t ch[3] = {R[t].a, R[t].b, R[t].c};
			const double len[3] = {R[t].la, R[t].lb, R[t].lc};
			const int nk = t + 1 == nrec && n > 2 ? 3 : 2;
			for (int c = 0; c < nk; c++) {
				if (ch[c] < 0 || (size_t)ch[c] >= n + S || seen[ch[c]]) goto done;
				seen[ch[c]] = 1, above[ch[c]] = len[c];
			}
		} /* (n + S children, none twice: every node but the last record's has its branch) */
		for (size_t i = 0; i < n; i++) lsum[i] += above[i];
		for (size_t s = 0; s < S; s++) {
			const uint32_t id = ids[k * S + s];
			if (id >= nsplits) goto done; /* (NO_SPLIT in a used replicate included) */
			const uint32_t j = node_of[id];
			if (j != NO_SPLIT) isum[j] += above[n + s], occ[j]++;
		}
	}

	/* parents: the majority sets in ascending size; each must be a union of whole components of the leaves so far (a
	 * laminar family), whose top nodes become its children and which it then merges */
	uint32_t *csize = uf + n, *mark = uf + 2 * n, *top = uf + 3 * n;
	for (size_t i = 0; i < n; i++) uf[i] = top[i] = (uint32_t)i, csize[i] = 1, mark[i] = 0;
	for (size_t j = 0; j < m; j++) {
		const uint64_t *X = sets + (size_t)split_of[j] * W;
		size_t size = 0;
		for (size_t w = 0; w < W; w++) size += (size_t)__builtin_popcountll(X[w]);
		const uint64_t valid = n & 63 ? (1ull << (n & 63)) - 1 : ~0ull;
		if (occ[j] != freq[split_of[j]] || (X[0] & 1) || (X[W - 1] & ~valid) || size < 2 || size > n - 2) goto done;
		order[j] = (uint64_t)size << 32 | j;
	}
	qsort(order, m, sizeof *order, cmp_u64);
	for (size_t o = 0; o < m; o++) {
		const uint32_t j = (uint32_t)order[o];
		const size_t size = (size_t)(order[o] >> 32);
		const uint64_t *X = sets + (size_t)split_of[j] * W;
		size_t nroots = 0, total = 0;
		for (size_t w = 0; w < W; w++)
			for (uint64_t bits = X[w]; bits; bits &= bits - 1) {
				const uint32_t r = uf_find(uf, (uint32_t)(w * 64 + (size_t)__builtin_ctzll(bits)));
				if (mark[r] == o + 1) continue;
				mark[r] = (uint32_t)o + 1, roots[nroots++] = r, total += csize[r];
			}
		if (total != size) goto done; /* a component reaches out of the set: not laminar */
		uint32_t big = roots[0];
		for (size_t q = 1; q < nroots; q++)
			if (csize[roots[q]] > csize[big]) big = roots[q];
		for (size_t q = 0; q < nroots; q++) {
			nodes[top[roots[q]]].parent = (int32_t)(n + j);
			if (roots[q] != big) uf[roots[q]] = big;
		}
		csize[big] = (uint32_t)size, top[big] = (uint32_t)(n + j), mark[big] = (uint32_t)o + 1;
	}
	for (size_t i = 0; i < n; i++) nodes[top[uf_find(uf, (uint32_t)i)]].parent = (int32_t)(n + m);
	for (size_t i = 0; i < n; i++) nodes[i].support = (uint32_t)used, nodes[i].length = lsum[i] / (double)used;
	for (size_t j = 0; j < m; j++)
		nodes[n + j].support = freq[split_of[j]], nodes[n + j].length = isum[j] / (double)freq[split_of[j]];
	nodes[n + m] = (andi_hip_cons_node){-1, (uint32_t)used, 0.0};
	*ninner = m;
	rc = 0;
done:
	free(node_of), free(split_of), free(occ), free(isum), free(lsum), free(above), free(seen), free(order), free(uf), free(roots);
	return rc;
}

/* one walk over the consensus nodes from the root, depth first with a stack of its own; kids[first[v] .. first[v+1]) are
 * v's children in the order of the text.  Returns the nodes it met; writes the text only with o. */
static size_t cons_walk(const andi_hip_cons_node *nodes, size_t n, size_t root, const uint32_t *first, const uint32_t *kids,
						uint32_t *stack, uint32_t *next, const char *const *names, int truncate, sink *o) {
	size_t depth = 0, met = 1;
	stack[depth++] = (uint32_t)root, next[root] = first[root];
	if (o) put(o, "(");
	while (depth) {
		const uint32_t v = stack[depth - 1];
		if (next[v] == first[v + 1]) {
			depth--;
			if (!o) continue;
			if (depth) put(o, ")%u:%.8g", (unsigned)nodes[v].support, nodes[v].length);
			else put(o, ");\n");
			continue;
		}
		if (o && next[v] != first[v]) put(o, ",");
		const uint32_t c = kids[next[v]++];
		met++;
		if (c < n) {
			if (o) put_leaf(o, names[c], truncate), put(o, ":%.8g", nodes[c].length);
		} else {
			stack[depth++] = c, next[c] = first[c];
			if (o) put(o, "(");
		}
	}
	return met;
}

size_t andi_hip_format_newick_consensus(const andi_hip_cons_node *nodes, size_t n, size_t ninner,
										const char *const *names, int truncate_names, char *out, size_t cap) {
	sink o = {out, cap, 0};
	if (out && cap) out[0] = '\0';
	if (!nodes || !names || n < 2 || n > 65535 || ninner > n) return 0;
	const size_t root = n + ninner, total = root + 1;
	if (nodes[root].parent != -1) return 0;
	uint32_t *first = calloc(total + 1, sizeof *first), *kids = malloc(total * sizeof *kids);
	uint32_t *fill = malloc(total * sizeof *fill), *stack = malloc(total * sizeof *stack), *next = malloc(total * sizeof *next);
	uint8_t *seen = calloc(total, 1);
	size_t need = 0;
	if (!first || !kids || !fill || !stack || !next || !seen) goto done;
	for (size_t v = 0; v < root; v++) {
		const int32_t p = nodes[v].parent;
		if (p < (int32_t)n || (size_t)p > root) goto done; /* a parent is an inner node or the root */
		first[p + 1]++;
	}
	for (size_t v = n; v < total; v++)
		if (first[v + 1] < 2) goto done; /* an inner node (and the root) has two children at least */
	for (size_t v = 0; v < total; v++) first[v + 1] += first[v], fill[v] = first[v];
	/* the children of every node in ascending order of their least leaf: from leaf 0, 1, ... upwards, each node is entered
	 * at its parent when the first leaf -- its least -- reaches it */
	size_t entered = 0;
	for (size_t l = 0; l < n; l++)
		for (uint32_t v = (uint32_t)l; v != root && !seen[v]; v = (uint32_t)nodes[v].parent)
			seen[v] = 1, kids[fill[nodes[v].parent]++] = v, entered++;
	if (entered != root) goto done; /* an inner node without a leaf below it */
	if (cons_walk(nodes, n, root, first, kids, stack, next, names, truncate_names, NULL) != total) goto done; /* a cycle */
	cons_walk(nodes, n, root, first, kids, stack, next, names, truncate_names, &o);
	need = o.len;
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
done:
	free(first), free(kids), free(fill), free(stack), free(next), free(seen);
	return need;
}

/* ------------------------------------------------------------------ */
/* Linkage clustering: what the host makes of andi_hip_linkage's records (include/andi_hip.h) */
/* ------------------------------------------------------------------ */

/* the records are a tree over the leaves 0 .. n-1: every child a leaf or an earlier record's node, the two children
 * differ, no node a child twice -- so node 2n - 2 is the one root and every walk from it ends */
static int links_are_a_tree(const andi_hip_link *L, size_t n) {
	uint8_t *child = calloc(2 * n, 1);
	if (!child) return 0;
	int ok = 1;
	for (size_t s = 0; ok && s + 1 < n; s++) {
		const int32_t ch[2] = {L[s].a, L[s].b};
		for (int k = 0; k < 2; k++)
			if (ch[k] < 0 || (size_t)ch[k] >= n + s || child[ch[k]]++) ok = 0;
	}
	free(child);
	return ok;
}

int andi_hip_linkage_cut(const andi_hip_link *links, size_t n, double t, uint32_t *labels, size_t *nclusters) {
	if (!links || !labels || !nclusters || n < 2 || n > 65535 || !links_are_a_tree(links, n)) return 1;
	const size_t nodes = 2 * n - 1;
	uint8_t *closed = calloc(nodes, 1);
	uint32_t *top = malloc(nodes * sizeof *top), *label = malloc(nodes * sizeof *label);
	if (!closed || !top || !label) {
		free(closed), free(top), free(label);
		return 1;
	}
	for (size_t s = 0; s + 1 < n; s++) { /* children come before their parents */
		const size_t a = (size_t)links[s].a, b = (size_t)links[s].b;
		closed[n + s] = links[s].height <= t && (a < n || closed[a]) && (b < n || closed[b]);
	}
	top[nodes - 1] = (uint32_t)(nodes - 1);
	for (size_t s = n - 1; s-- > 0;) { /* parents before their children: top[v] is the maximal closed node above v, or v */
		const size_t v = n + s, a = (size_t)links[s].a, b = (size_t)links[s].b;
		top[a] = closed[v] ? top[v] : (uint32_t)a;
		top[b] = closed[v] ? top[v] : (uint32_t)b;
	}
	memset(label, 0xff, nodes * sizeof *label);
	uint32_t next = 0;
	for (size_t i = 0; i < n; i++) {
		if (label[top[i]] == 0xffffffffu) label[top[i]] = next++;
		labels[i] = label[top[i]];
	}
	*nclusters = next;
	free(closed), free(top), free(label);
	return 0;
}

/* the members of every cluster in ascending leaf id: first[c] .. first[c + 1] of order (a counting sort); NULL on bad
 * labels or an empty cluster */
static uint32_t *cluster_members(const uint32_t *labels, size_t n, size_t nclusters, uint32_t **first_out) {
	if (nclusters == 0 || nclusters > n) return NULL;
	uint32_t *first = calloc(nclusters + 1, sizeof *first), *order = malloc(n * sizeof *order), *fill = malloc(nclusters * sizeof *fill);
	int ok = first && order && fill;
	for (size_t i = 0; ok && i < n; i++) {
		if (labels[i] >= nclusters) ok = 0;
		else first[labels[i] + 1]++;
	}
	for (size_t c = 0; ok && c < nclusters; c++) {
		if (first[c + 1] == 0) ok = 0;
		first[c + 1] += first[c], fill[c] = first[c];
	}
	for (size_t i = 0; ok && i < n; i++) order[fill[labels[i]]++] = (uint32_t)i;
	free(fill);
	if (!ok) {
		free(first), free(order);
		return NULL;
	}
	*first_out = first;
	return order;
}

int andi_hip_cluster_medoids(const double *D, size_t n, const uint32_t *labels, size_t nclusters, uint32_t *medoid) {
	if (!D || !labels || !medoid || n < 2 || n > 65535) return 1;
	for (size_t i = 0; i < n; i++)
		for (size_t j = i + 1; j < n; j++)
			if (D[i * n + j] == -INFINITY) return 1;
	uint32_t *first = NULL, *order = cluster_members(labels, n, nclusters, &first);
	if (!order) return 1;
	for (size_t c = 0; c < nclusters; c++) {
		double best = NAN;
		for (uint32_t p = first[c]; p < first[c + 1]; p++) {
			const size_t i = order[p];
			double sum = 0.0;
			for (uint32_t q = first[c]; q < first[c + 1]; q++) {
				const size_t j = order[q];
				const double d = i == j ? 0.0 : i < j ? D[i * n + j] : D[j * n + i];
				sum += isnan(d) ? INFINITY : d;
			}
			if (p == first[c] || (isnan(best) && !isnan(sum)) || sum < best) best = sum, medoid[c] = (uint32_t)i;
		}
	}
	free(first), free(order);
	return 0;
}

int andi_hip_cluster_stability(const uint32_t *labels, size_t nclusters, const uint32_t *rep_labels, size_t n, size_t count,
							   uint32_t *stability) {
	if (!labels || !rep_labels || !stability || n < 2 || n > 65535) return 1;
	uint32_t *first = NULL, *order = cluster_members(labels, n, nclusters, &first);
	uint32_t *members = malloc(n * sizeof *members); /* of every cluster of one replicate */
	int bad = !order || !members;
	for (size_t c = 0; !bad && c < nclusters; c++) stability[c] = 0;
	for (size_t k = 0; !bad && k < count; k++) {
		const uint32_t *R = rep_labels + k * n;
		memset(members, 0, n * sizeof *members);
		for (size_t i = 0; i < n; i++) {
			if (R[i] >= n) {
				bad = 1;
				break;
			}
			members[R[i]]++;
		}
		for (size_t c = 0; !bad && c < nclusters; c++) {
			const uint32_t l = R[order[first[c]]];
			int same = members[l] == first[c + 1] - first[c];
			for (uint32_t p = first[c] + 1; same && p < first[c + 1]; p++) same = R[order[p]] == l;
			stability[c] += (uint32_t)same;
		}
	}
	free(first), free(order), free(members);
	return bad;
}

size_t andi_hip_format_newick_linkage(const andi_hip_link *links, size_t n, const char *const *names, int truncate_names,
									  char *out, size_t cap) {
	sink o = {out, cap, 0};
	if (out && cap) out[0] = '\0';
	if (!links || !names || n < 2 || n > 65535 || !links_are_a_tree(links, n)) return 0;
#define LINK_HEIGHT(v) ((size_t)(v) < n ? 0.0 : links[(size_t)(v) - n].height)
	for (size_t s = 0; s + 1 < n; s++) /* every branch: the parent's height less the child's */
		if (!isfinite(links[s].height - LINK_HEIGHT(links[s].a)) || !isfinite(links[s].height - LINK_HEIGHT(links[s].b))) return 0;
	typedef struct {
		uint32_t rec; /* record of this node */
		int next;     /* its next child */
		double len;   /* its own branch length */
	} frame;
	frame *stack = malloc(n * sizeof *stack);
	if (!stack) return 0;
	size_t top = 0;
	stack[top++] = (frame){(uint32_t)(n - 2), 0, 0.0};
	put(&o, "(");
	while (top) {
		frame *f = &stack[top - 1];
		const andi_hip_link *r = &links[f->rec];
		if (f->next == 2) {
			const double len = f->len;
			top--;
			if (top) put(&o, "):%.8g", len);
			else put(&o, ");\n");
			continue;
		}
		const int k = f->next++;
		if (k) put(&o, ",");
		const size_t child = (size_t)(k == 0 ? r->a : r->b);
		const double len = r->height - LINK_HEIGHT(child);
		if (child < n) {
			put_leaf(&o, names[child], truncate_names);
			put(&o, ":%.8g", len);
		} else {
			stack[top++] = (frame){(uint32_t)(child - n), 0, len};
			put(&o, "(");
		}
	}
#undef LINK_HEIGHT
	free(stack);
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	return o.len;
}

/* ------------------------------------------------------------------ */
/* Placement on a tree (include/andi_hip.h): the host's pieces          */
/* ------------------------------------------------------------------ */

/* andi_hip_distances_rect: the cells of andi_hip_format_distances_rect, blocks of query rows dealt to a pool of threads */
typedef struct {
	const andi_hip_model *MRQ, *MQR;
	size_t nr, nq;
	int model;
	double *D;
	size_t next; /* atomic: the next block of query rows */
} rect_job;

static void *rect_worker(void *arg) {
	rect_job *job = arg;
	for (;;) {
		const size_t q0 = __atomic_fetch_add(&job->next, 4, __ATOMIC_RELAXED);
		if (q0 >= job->nq) break;
		for (size_t q = q0; q < q0 + 4 && q < job->nq; q++)
			for (size_t r = 0; r < job->nr; r++) {
				const andi_hip_model datum = andi_hip_model_average(&job->MQR[q * job->nr + r], &job->MRQ[r * job->nq + q]);
				job->D[q * job->nr + r] = andi_hip_estimate(&datum, job->model);
			}
	}
	return NULL;
}

int andi_hip_distances_rect(const andi_hip_model *MRQ, const andi_hip_model *MQR, size_t nr, size_t nq, int model, double *D) {
	if (!MRQ || !MQR || !D) return 1;
	rect_job job = {MRQ, MQR, nr, nq, model, D, 0};
	long procs = sysconf(_SC_NPROCESSORS_ONLN);
	size_t nt = procs > 0 ? (size_t)procs : 1;
	if (nt > 32) nt = 32;
	if (nt > nq * nr / 4096 + 1) nt = nq * nr / 4096 + 1; /* (small tables: the calling thread alone) */
	pthread_t tid[32];
	size_t started = 0;
	for (size_t t = 1; t < nt; t++)
		if (pthread_create(&tid[started], NULL, rect_worker, &job) == 0) started++;
	rect_worker(&job);
	for (size_t t = 0; t < started; t++) pthread_join(tid[t], NULL);
	return 0;
}

/* a name as the tree's text holds it (cut to ten characters under truncate_names), with its leaf */
typedef struct {
	const char *s;
	size_t len;
	uint32_t id;
} nwk_name;

static int nwk_cmp(const char *a, size_t la, const char *b, size_t lb) {
	const int c = memcmp(a, b, la < lb ? la : lb);
	return c ? c : la < lb ? -1 : la > lb;
}

static int nwk_cmp_names(const void *a, const void *b) {
	const nwk_name *x = a, *y = b;
	const int c = nwk_cmp(x->s, x->len, y->s, y->len);
	return c ? c : x->id < y->id ? -1 : x->id > y->id; /* (names that agree: the first is the one found) */
}

/* an inner node of the text while it is open: its children so far, where its "(" is */
typedef struct {
	int32_t id[3];
	double len[3];
	int kids;
} nwk_frame;

static size_t nwk_blanks(const char *t, size_t pos) {
	while (t[pos] == ' ' || t[pos] == '\t' || t[pos] == '\n' || t[pos] == '\r') pos++;
	return pos;
}

/* a quoted string from its opening quote on: its text ('' undoubled) into buf; the position behind its closing quote, or
 * 0 when the text ends first */
static size_t nwk_quoted(const char *t, size_t pos, char *buf, size_t *len) {
	size_t k = 0;
	for (pos++;; pos++) {
		if (!t[pos]) return 0;
		if (t[pos] == '\'') {
			if (t[pos + 1] != '\'') break;
			pos++;
		}
		buf[k++] = t[pos];
	}
	*len = k;
	return pos + 1;
}

int andi_hip_parse_newick(const char *text, const char *const *names, size_t n, int truncate_names, andi_hip_nj_join *joins,
						  char *errbuf, size_t errlen) {
#define NWK_FAIL(...)                                                                              \
	do {                                                                                           \
		if (errbuf && errlen) snprintf(errbuf, errlen, "andi_hip_parse_newick: " __VA_ARGS__);      \
		goto fail;                                                                                 \
	} while (0)
	if (errbuf && errlen) errbuf[0] = '\0';
	nwk_name *index = NULL;
	nwk_frame *stack = NULL;
	uint8_t *seen = NULL;
	char *buf = NULL;
	if (!text || !names || !joins || n < 3 || n > 65535) NWK_FAIL("bad arguments (text, names and joins must be given, 3 <= n <= 65535)");
	index = malloc(n * sizeof *index), stack = malloc(n * sizeof *stack), seen = calloc(n, 1), buf = malloc(strlen(text) + 1);
	if (!index || !stack || !seen || !buf) NWK_FAIL("out of memory");
	for (size_t i = 0; i < n; i++) index[i] = (nwk_name){names[i], truncate_names ? strnlen(names[i], 10) : strlen(names[i]), (uint32_t)i};
	qsort(index, n, sizeof *index, nwk_cmp_names);

	size_t pos = nwk_blanks(text, 0), top = 0, pairs = 0, leaves = 0;
	if (text[pos] != '(') NWK_FAIL("byte %zu: expected '(' at the start of the tree", pos);
	for (;;) {
		/* a subtree starts here */
		pos = nwk_blanks(text, pos);
		if (text[pos] == '(') {
			if (top == n - 1) NWK_FAIL("byte %zu: nested deeper than a tree of %zu leaves can be", pos, n);
			stack[top++].kids = 0;
			pos++;
			continue;
		}
		const size_t at = pos;
		size_t len = 0;
		if (text[pos] == '\'') {
			pos = nwk_quoted(text, pos, buf, &len);
			if (!pos) NWK_FAIL("byte %zu: a quoted name does not end", at);
		} else {
			while (text[pos] && !strchr(":,(); \t\n\r", text[pos])) buf[len++] = text[pos++];
		}
		if (truncate_names && len > 10) len = 10;
		size_t lo = 0, hi = n; /* the first name not before the text */
		while (lo < hi) {
			const size_t mid = (lo + hi) / 2;
			if (nwk_cmp(index[mid].s, index[mid].len, buf, len) < 0) lo = mid + 1;
			else hi = mid;
		}
		if (lo == n || nwk_cmp(index[lo].s, index[lo].len, buf, len)) NWK_FAIL("byte %zu: unknown name '%.*s'", at, (int)len, buf);
		int32_t child = (int32_t)index[lo].id;
		if (seen[child]) NWK_FAIL("byte %zu: duplicate name '%.*s'", at, (int)len, buf);
		seen[child] = 1, leaves++;
		for (;;) { /* a child of the open node is complete but for its length */
			pos = nwk_blanks(text, pos);
			if (text[pos] != ':') NWK_FAIL("byte %zu: missing branch length", pos);
			const size_t lat = pos + 1;
			char *end;
			const double l = strtod(text + lat, &end);
			if (end == text + lat) NWK_FAIL("byte %zu: missing branch length", lat);
			if (!isfinite(l)) NWK_FAIL("byte %zu: the branch length is not finite", lat);
			pos = (size_t)(end - text);
			nwk_frame *f = &stack[top - 1];
			if (top == 1 && f->kids == 3) NWK_FAIL("byte %zu: the root has more than three subtrees", lat);
			if (top > 1 && f->kids == 2) NWK_FAIL("byte %zu: an inner node has more than two children", lat);
			f->id[f->kids] = child, f->len[f->kids] = l, f->kids++;
			pos = nwk_blanks(text, pos);
			if (text[pos] == ',') {
				pos++;
				break; /* the next subtree */
			}
			if (text[pos] != ')') NWK_FAIL("byte %zu: expected ',' or ')'", pos);
			if (top == 1) goto root_closes;
			if (f->kids != 2) NWK_FAIL("byte %zu: an inner node has %d child, not two", pos, f->kids);
			if (pairs + 2 >= n) /* (one more than an unrooted tree has: a rooted text gets as far as its root, and fails there) */
				NWK_FAIL("byte %zu: more inner nodes than a binary tree of %zu leaves has", pos, n);
			const int lower = f->id[0] < f->id[1] ? 0 : 1;
			joins[pairs] = (andi_hip_nj_join){f->id[lower], f->id[1 - lower], -1, 0, f->len[lower], f->len[1 - lower], 0.0};
			child = (int32_t)(n + pairs++);
			top--;
			pos++; /* behind the ")": a label (support, TBE, consensus numbers) is not looked at */
			if (text[pos] == '\'') {
				const size_t q = nwk_quoted(text, pos, buf, &len);
				if (!q) NWK_FAIL("byte %zu: a quoted label does not end", pos);
				pos = q;
			} else {
				while (text[pos] && !strchr(":,(); \t\n\r", text[pos])) pos++;
			}
		}
	}
root_closes:;
	const nwk_frame *f = &stack[0];
	if (f->kids != 3) NWK_FAIL("byte %zu: the root has %d subtrees, not three", pos, f->kids);
	pos++;
	while (text[pos] && !strchr(":,(); \t\n\r", text[pos])) pos++; /* (a label) */
	pos = nwk_blanks(text, pos);
	if (text[pos] != ';') NWK_FAIL("byte %zu: expected ';' at the end of the tree", pos);
	pos = nwk_blanks(text, pos + 1);
	if (text[pos]) NWK_FAIL("byte %zu: trailing text behind the tree", pos);
	if (leaves < n) {
		size_t i = 0;
		while (seen[i]) i++;
		NWK_FAIL("byte %zu: the tree has %zu of the %zu names; missing name '%s'", pos, leaves, n, names[i]);
	}
	{ /* (all n names once, every inner node binary, the root ternary: n - 3 pair records) */
		int o[3] = {0, 1, 2};
		for (int a = 0; a < 3; a++)
			for (int b = a + 1; b < 3; b++)
				if (f->id[o[b]] < f->id[o[a]]) {
					const int t = o[a];
					o[a] = o[b], o[b] = t;
				}
		joins[n - 3] = (andi_hip_nj_join){f->id[o[0]], f->id[o[1]], f->id[o[2]], 0, f->len[o[0]], f->len[o[1]], f->len[o[2]]};
	}
	free(index), free(stack), free(seen), free(buf);
	return 0;
fail:
	free(index), free(stack), free(seen), free(buf);
	return 1;
#undef NWK_FAIL
}

/* s as the inside of a JSON string */
static void put_json(sink *o, const char *s, size_t len) {
	for (size_t k = 0; k < len; k++) {
		const unsigned char c = (unsigned char)s[k];
		if (c == '"' || c == '\\') put(o, "\\%c", c);
		else if (c < 0x20) put(o, "\\u%04x", c);
		else put(o, "%c", c);
	}
}

size_t andi_hip_format_jplace(const andi_hip_nj_join *tree, size_t n, const char *const *ref_names, int truncate_names,
							  const andi_hip_placement *placements, size_t nq, const char *const *query_names, int method,
							  char *out, size_t cap) {
	sink o = {out, cap, 0};
	if (out && cap) out[0] = '\0';
	if (!tree || !ref_names || (nq && (!placements || !query_names)) || n < 3 || (method != ANDI_PLACE_OLS && method != ANDI_PLACE_FM))
		return 0;
	const size_t need = format_newick(tree, NULL, NULL, NULL, 0, n, ref_names, truncate_names, 1, NULL, 0);
	if (!need) return 0;
	char *text = malloc(need + 1);
	if (!text) return 0;
	format_newick(tree, NULL, NULL, NULL, 0, n, ref_names, truncate_names, 1, text, need + 1);
	put(&o, "{\n\"tree\":\"");
	put_json(&o, text, need - 1); /* (without the line's end) */
	free(text);
	put(&o, "\",\n\"placements\":[");
	int first = 1;
	for (size_t q = 0; q < nq; q++) {
		const andi_hip_placement *p = &placements[q];
		if (p->edge < 0) continue;
		put(&o, first ? "\n" : ",\n");
		first = 0;
		put(&o, "{\"p\":[[%d,%.17g,1,%.17g,%.17g]],\"n\":[\"", (int)p->edge, p->err, p->distal, p->pendant);
		put_json(&o, query_names[q], truncate_names ? strnlen(query_names[q], 10) : strlen(query_names[q]));
		put(&o, "\"]}");
	}
	put(&o, "\n],\n\"metadata\":{\"program\":\"andi-hip\",\"placement\":\"least squares on anchor distances\",\"method\":\"%s\"},\n",
		method == ANDI_PLACE_FM ? "fm" : "ols");
	put(&o, "\"version\":3,\n\"fields\":[\"edge_num\",\"likelihood\",\"like_weight_ratio\",\"distal_length\",\"pendant_length\"]\n}\n");
	if (out && cap) out[o.len < cap ? o.len : cap - 1] = '\0';
	return o.len;
}
