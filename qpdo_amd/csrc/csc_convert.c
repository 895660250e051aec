/*
 * csc_convert.c -- CSC -> int32 CSR images of A, A' and the full symmetric Q on the host: the only implementation, shared by
 * qpdo_setup (row-partitioned workspaces, QPDO_SETUP_HOST=1), the fused batches, the batch streams and the resident fleets.
 * The contract is in csc_convert.h.
 */
#include <stdlib.h>
#include <string.h>
#include <omp.h>

#include "csc_convert.h"

#define PAR_MIN_NNZ 200000      /* below this many entries a conversion stays serial unless threads were asked for */

void conv_scratch_init(ConvScratch *W) { memset(W, 0, sizeof(*W)); }
void conv_scratch_free(ConvScratch *W) {
    free(W->cnt.p); free(W->cut.p); free(W->rrp.p); free(W->rci.p); free(W->rval.p); free(W->rmap.p);
    memset(W, 0, sizeof(*W));
}
/* at least `bytes` bytes (contents undefined), or NULL */
static void *conv_buf(ConvBuf *b, size_t bytes) {
    if (b->cap < bytes || !b->p) {
        free(b->p);
        b->cap = bytes ? bytes : 1;
        b->p = malloc(b->cap);
        if (!b->p) b->cap = 0;
    }
    return b->p;
}
static int team_size(int threads) {
    if (threads > 0) return threads;
    const int t = omp_get_max_threads();
    return t > 16 ? 16 : t < 1 ? 1 : t;
}

/* ---- CSR(A') ------------------------------------------------------------------------------------------------------------ */
/* (index arrays and itype go through locals everywhere below: a store into the caller's int arrays may alias the fields of M) */
static void narrow(const cholmod_sparse *M, int32_t *rp, int32_t *ci, double *val, int64_t j0, int64_t j1, int64_t k0, int64_t k1) {
    const void *Mp = M->p, *Mi = M->i; const int it = M->itype;
    for (int64_t j = j0; j < j1; j++) rp[j] = (int32_t)idx_at(Mp, it, j);
    for (int64_t k = k0; k < k1; k++) ci[k] = (int32_t)idx_at(Mi, it, k);
    if (k1 > k0) memcpy(val + k0, (const double *)M->x + k0, (size_t)(k1 - k0) * sizeof(double));
}
void csc_as_csr_of_transpose(const cholmod_sparse *M, int32_t *rp, int32_t *ci, double *val, int threads) {
    const int64_t nc = (int64_t)M->ncol, nnz = idx_at(M->p, M->itype, nc);
    const int T = nnz > PAR_MIN_NNZ ? team_size(threads) : 1;
    if (T == 1) { narrow(M, rp, ci, val, 0, nc + 1, 0, nnz); return; }
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) narrow(M, rp, ci, val, (nc + 1) * t / T, (nc + 1) * (t + 1) / T, nnz * t / T, nnz * (t + 1) / T);
}

/* ---- CSR(A) ---------------------------------------------------------------------------------------------------------------
 * The columns are cut into T contiguous ranges of equal nnz; thread t counts its range per row, a prefix over (row, t) gives
 * every thread its first slot in each row, and the threads scatter their ranges in column order -- the result is the one a
 * serial counting pass gives.  c is range t's slice of cnt[t * nr + i]. */
static void count_range(const cholmod_sparse *M, const int64_t *cut, int t, int32_t *c, int64_t nr) {
    const void *Mi = M->i; const int it = M->itype;
    const int64_t kb = idx_at(M->p, it, cut[t]), ke = idx_at(M->p, it, cut[t + 1]);
    if (nr) memset(c, 0, (size_t)nr * sizeof(int32_t));
    for (int64_t k = kb; k < ke; k++) c[idx_at(Mi, it, k)]++;
}
/* the total of row i into rp[i + 1]; cnt becomes the offset of thread t inside row i (scatter_range adds the row's start) */
static inline void row_offsets(int32_t *cnt, int T, int64_t nr, int64_t i, int32_t *rp) {
    int32_t run = 0;
    for (int t = 0; t < T; t++) { const int32_t v = cnt[(size_t)t * (size_t)nr + i]; cnt[(size_t)t * (size_t)nr + i] = run; run += v; }
    rp[i + 1] = run;
}
static void scatter_range(const cholmod_sparse *M, const int64_t *cut, int t, int32_t *c, int64_t nr, const int32_t *rp, int32_t *ci, double *val, int32_t *map) {
    const double *x = M->x;
    const void *Mp = M->p, *Mi = M->i; const int it = M->itype;
    const int64_t j0 = cut[t], j1 = cut[t + 1];
    for (int64_t i = 0; i < nr; i++) c[i] += rp[i];      /* the next free slot of range t in row i */
    for (int64_t j = j0; j < j1; j++) {
        const int64_t b = idx_at(Mp, it, j), e = idx_at(Mp, it, j + 1);
        for (int64_t k = b; k < e; k++) {
            const int32_t s = c[idx_at(Mi, it, k)]++;
            ci[s] = (int32_t)j; val[s] = x[k];
            if (map) map[s] = (int32_t)k;
        }
    }
}
int csc_to_csr(const cholmod_sparse *M, int32_t *rp, int32_t *ci, double *val, int32_t *map, int threads, ConvScratch *W) {
    const int64_t nr = (int64_t)M->nrow, nc = (int64_t)M->ncol, nnz = idx_at(M->p, M->itype, nc);
    int T = team_size(threads);
    if ((nnz < PAR_MIN_NNZ && threads <= 0) || (int64_t)T * nr > 400000000LL) T = 1;
    int32_t *cnt = conv_buf(&W->cnt, (size_t)T * (size_t)nr * sizeof(int32_t));
    int64_t *cut = conv_buf(&W->cut, ((size_t)T + 1) * sizeof(int64_t));
    if (!cnt || !cut) return -1;
    cut[0] = 0; cut[T] = nc;
    for (int t = 1; t < T; t++) {            /* first column whose start offset reaches t/T of the entries */
        const int64_t target = nnz / T * t;
        int64_t lo = cut[t - 1], hi = nc;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (idx_at(M->p, M->itype, mid) < target) lo = mid + 1; else hi = mid; }
        cut[t] = lo;
    }
    rp[0] = 0;
    if (T == 1) {
        count_range(M, cut, 0, cnt, nr);
        for (int64_t i = 0; i < nr; i++) { row_offsets(cnt, 1, nr, i, rp); rp[i + 1] += rp[i]; }
        scatter_range(M, cut, 0, cnt, nr, rp, ci, val, map);
        return 0;
    }
#pragma omp parallel num_threads(T)
    {      /* every loop is over ranges or rows, not over thread numbers: right also when the runtime grants fewer than T threads */
#pragma omp for schedule(static)
        for (int t = 0; t < T; t++) count_range(M, cut, t, cnt + (size_t)t * (size_t)nr, nr);
#pragma omp for schedule(static)
        for (int64_t i = 0; i < nr; i++) row_offsets(cnt, T, nr, i, rp);
#pragma omp single
        for (int64_t i = 0; i < nr; i++) rp[i + 1] += rp[i];
#pragma omp for schedule(static)
        for (int t = 0; t < T; t++) scatter_range(M, cut, t, cnt + (size_t)t * (size_t)nr, nr, rp, ci, val, map);
    }
    return 0;
}

/* ---- full symmetric CSR(Q) ---------------------------------------------------------------------------------------------------
 * An entry (i, j) of the stored matrix counts when it is on the stored side or the diagonal. */
#define KEEP_CSR(st, i, j) (((st) < 0) ? ((j) <= (i)) : ((j) >= (i)))      /* CSR row i keeps (i,j): own triangle incl. diagonal */
#define KEEP_MIR(st, i, j) (((st) < 0) ? ((i) > (j)) : ((i) < (j)))        /* CSC column j entry (i,j) mirrors into row j as (j,i) */

int64_t sym_full_nnz(const cholmod_sparse *Q) {
    const int64_t nnz = idx_at(Q->p, Q->itype, (int64_t)Q->ncol);
    const int st = Q->stype;
    if (st == 0) return nnz;
    const void *Qp = Q->p, *Qi = Q->i; const int it = Q->itype;
    int64_t c = 0;
    for (int64_t j = 0; j < (int64_t)Q->ncol; j++)
        for (int64_t k = idx_at(Qp, it, j), e = idx_at(Qp, it, j + 1); k < e; k++) {
            const int64_t i = idx_at(Qi, it, k);
            if (st < 0) c += (i >= j) + (i > j); else c += (i <= j) + (i < j);      /* the stored triangle once, its strict part mirrored */
        }
    return c;
}
/* R: the CSR of the stored matrix (all its entries) */
typedef struct { const int32_t *rp, *ci, *map; const double *val; } StoredCsr;
/* rows [i0, i1): their entry counts into rp[i + 1] */
static void full_count_rows(const cholmod_sparse *Q, const StoredCsr *R, int64_t i0, int64_t i1, int32_t *rp) {
    const int st = Q->stype, it = Q->itype;
    const void *Qp = Q->p, *Qi = Q->i;
    for (int64_t i = i0; i < i1; i++) {
        int32_t c = 0;
        for (int32_t k = R->rp[i]; k < R->rp[i + 1]; k++) c += KEEP_CSR(st, i, (int64_t)R->ci[k]);
        const int64_t b = idx_at(Qp, it, i), e = idx_at(Qp, it, i + 1);
        for (int64_t k = b; k < e; k++) c += KEEP_MIR(st, idx_at(Qi, it, k), i);
        rp[i + 1] = c;
    }
}
/* rows [i0, i1), the first of them at offset s: lower stored, the CSR row (columns <= i) and then the mirrored column below the
 * diagonal; upper stored, the mirrored column above the diagonal and then the CSR row (columns >= i).  Writes rp[i0 .. i1 - 1] and
 * returns the offset behind the last row. */
static int32_t full_fill_rows(const cholmod_sparse *Q, const StoredCsr *R, int64_t i0, int64_t i1, int32_t s, int32_t *rp, int32_t *ci, double *val, int32_t *map) {
    const int st = Q->stype, it = Q->itype;
    const void *Qp = Q->p, *Qi = Q->i;
    const double *x = Q->x, *Rval = R->val;
    const int32_t *Rrp = R->rp, *Rci = R->ci, *Rmap = R->map;
    for (int64_t i = i0; i < i1; i++) {
        rp[i] = s;
        for (int half = 0; half < 2; half++) {
            if ((half == 0) == (st < 0)) {
                for (int32_t k = Rrp[i], ke = Rrp[i + 1]; k < ke; k++)
                    if (KEEP_CSR(st, i, (int64_t)Rci[k])) { ci[s] = Rci[k]; val[s] = Rval[k]; if (map) map[s] = Rmap[k]; s++; }
            } else {
                const int64_t b = idx_at(Qp, it, i), e = idx_at(Qp, it, i + 1);
                for (int64_t k = b; k < e; k++) {
                    const int64_t r = idx_at(Qi, it, k);
                    if (KEEP_MIR(st, r, i)) { ci[s] = (int32_t)r; val[s] = x[k]; if (map) map[s] = (int32_t)k; s++; }
                }
            }
        }
    }
    return s;
}
int sym_to_full_csr(const cholmod_sparse *Q, int32_t *rp, int32_t *ci, double *val, int32_t *map, int threads, ConvScratch *W) {
    const int64_t n = (int64_t)Q->ncol, nnzs = idx_at(Q->p, Q->itype, n);
    if (Q->stype == 0) {      /* symmetric: transpose == itself */
        csc_as_csr_of_transpose(Q, rp, ci, val, threads);
        if (map) for (int64_t k = 0; k < nnzs; k++) map[k] = (int32_t)k;
        return 0;
    }
    int32_t *Rrp = conv_buf(&W->rrp, ((size_t)n + 1) * sizeof(int32_t)), *Rci = conv_buf(&W->rci, (size_t)nnzs * sizeof(int32_t));
    int32_t *Rmap = map ? conv_buf(&W->rmap, (size_t)nnzs * sizeof(int32_t)) : NULL;
    double *Rval = conv_buf(&W->rval, (size_t)nnzs * sizeof(double));
    if (!Rrp || !Rci || !Rval || (map && !Rmap) || csc_to_csr(Q, Rrp, Rci, Rval, Rmap, threads, W)) return -1;
    const StoredCsr R = {Rrp, Rci, Rmap, Rval};
    const int T = nnzs > PAR_MIN_NNZ ? team_size(threads) : 1;
    if (T == 1 && 2 * nnzs < (int64_t)INT32_MAX) {      /* the count cannot reach the limit: one pass with a running offset */
        rp[n] = full_fill_rows(Q, &R, 0, n, 0, rp, ci, val, map);
        return 0;
    }
    rp[0] = 0;
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) full_count_rows(Q, &R, n * t / T, n * (t + 1) / T, rp);
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) { total += rp[i + 1]; if (total >= (int64_t)INT32_MAX) return -1; rp[i + 1] = (int32_t)total; }
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) full_fill_rows(Q, &R, n * t / T, n * (t + 1) / T, rp[n * t / T], rp, ci, val, map);
    return 0;
}

/* ---- owned triples and the row partition --------------------------------------------------------------------------------- */
void host_csr_free(HostCsr *h) { free(h->rp); free(h->ci); free(h->val); memset(h, 0, sizeof(*h)); }

/* the share [*first, *first + *len) of `count` rows: ceil(count / world) per rank, start and end clipped to count */
static void rank_rows(int64_t count, int rank, int world, int32_t *first, int32_t *len) {
    const int64_t per = (count + world - 1) / world;
    int64_t r0 = (int64_t)rank * per; if (r0 > count) r0 = count;
    int64_t r1 = r0 + per; if (r1 > count) r1 = count;
    *first = (int32_t)r0; *len = (int32_t)(r1 - r0);
}
/* rows [r0, r0 + len) of M: row pointers of its own over M's ci and val */
static int row_slice(const HostCsr *M, int32_t r0, int32_t len, HostCsr *out) {
    out->nrows = len; out->ncols = M->ncols;
    out->rp = malloc(((size_t)len + 1) * sizeof(int32_t));
    if (!out->rp) return -1;
    for (int32_t i = 0; i <= len; i++) out->rp[i] = M->rp[r0 + i] - M->rp[r0];
    out->nnz = out->rp[len]; out->ci = M->ci + M->rp[r0]; out->val = M->val + M->rp[r0];
    return 0;
}
/* columns [c0, c0 + len) of M, renumbered from 0, every row */
static int col_slice(const HostCsr *M, int32_t c0, int32_t len, HostCsr *out) {
    const int32_t c1 = c0 + len;
    int64_t tn = 0;
    for (int64_t k = 0; k < M->nnz; k++) tn += (M->ci[k] >= c0 && M->ci[k] < c1);
    out->nrows = M->nrows; out->ncols = len; out->nnz = tn;
    out->rp = malloc(((size_t)M->nrows + 1) * sizeof(int32_t));
    out->ci = malloc((size_t)(tn ? tn : 1) * sizeof(int32_t)); out->val = malloc((size_t)(tn ? tn : 1) * sizeof(double));
    if (!out->rp || !out->ci || !out->val) return -1;
    int64_t pos = 0;
    for (int32_t j = 0; j < M->nrows; j++) {
        out->rp[j] = (int32_t)pos;
        for (int32_t k = M->rp[j]; k < M->rp[j + 1]; k++)
            if (M->ci[k] >= c0 && M->ci[k] < c1) { out->ci[pos] = M->ci[k] - c0; out->val[pos] = M->val[k]; pos++; }
    }
    out->rp[M->nrows] = (int32_t)pos;
    return 0;
}
int cut_row_partition(const HostCsr *Ar, const HostCsr *At, const HostCsr *Qf, int rank, int world, RowPartition *P) {
    memset(P, 0, sizeof(*P));
    rank_rows(Ar->nrows, rank, world, &P->m0, &P->mloc);
    rank_rows(Qf->nrows, rank, world, &P->n0, &P->nloc);
    if (row_slice(Ar, P->m0, P->mloc, &P->Al) || row_slice(Qf, P->n0, P->nloc, &P->Ql) || col_slice(At, P->m0, P->mloc, &P->Tl)) {
        row_partition_free(P);
        return -1;
    }
    return 0;
}
void row_partition_free(RowPartition *P) {
    free(P->Al.rp); free(P->Ql.rp); host_csr_free(&P->Tl);
    memset(P, 0, sizeof(*P));
}
