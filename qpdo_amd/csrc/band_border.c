/*
 * band_border.c -- detection of a BORDERED band (qpdo_amd_band_border; contract: include/qpdo_amd_ext.h): a chain-structured QP with a few
 * trailing variables that appear everywhere -- a global slack, a free final time, a shared parameter.  K = Q + sigma I + A'DA is then
 *
 *     K = [ B   C ]    B: n_core x n_core, half-bandwidth <= 127      (the core variables)
 *         [ C'  D ]    C: n_core x c, D: c x c                        (the trailing c border variables)
 *
 * and the band solver takes it by block elimination (dev/band.inc, the bordered mode).  Pure host code, no HIP, a sibling of band_order.c;
 * tests/band_border_driver.c links this translation unit alone.
 *
 * The rule, T = 127 (BAND_MAX_B): n_core starts at n;
 *   a stored entry (i, j) of Q with |i - j| > T            n_core <= max(i, j)
 *   a row of A with ascending columns c1 < c2 < ...        n_core <= the first column that exceeds c1 + T
 * (every column of the row below that one is within T of every other).  c = n - n_core; b_core = the half-bandwidth of the pattern
 * restricted to the columns < n_core, at least 3 as band_detect's.  Q's stype is honoured as qpdo_setup honours it, explicit zeros count.
 *
 * The rows of A come from its CSC arrays without a conversion: the columns are visited in ascending order, so the first entry a row
 * shows is its first column, and one int32 per row (that column) is all the pass keeps.  Two passes over the pattern, O(nnz).
 */
#include <stdint.h>
#include <stdlib.h>

#include "qpdo.h"
#include "qpdo_amd_ext.h"

#define BAND_BORDER_T 127                /* BAND_MAX_B of dev/band.inc */

static inline int64_t bb_idx(const void *a, int itype, int64_t k) {
    return itype == 0 ? (int64_t)((const int32_t *)a)[k] : (int64_t)((const int64_t *)a)[k];
}
/* is the stored entry (i, j) of Q one the setup reads?  (stype -1: the lower triangle, +1: the upper, 0: all) */
static inline int bb_q_entry(int stype, int64_t i, int64_t j) { return stype == 0 || (stype < 0 ? i >= j : i <= j); }

int qpdo_amd_band_border(const cholmod_sparse *Q, const cholmod_sparse *A, long max_border, long *info4) {
    if (!Q || !Q->p || !info4 || (Q->itype != 0 && Q->itype != 2) || Q->nrow != Q->ncol || Q->ncol >= (size_t)INT32_MAX) return -1;
    if (A && (!A->p || (A->itype != 0 && A->itype != 2) || A->ncol != Q->ncol || A->nrow >= (size_t)INT32_MAX)) return -1;
    if (A && A->nrow == 0) A = NULL;
    const int64_t n = (int64_t)Q->ncol, m = A ? (int64_t)A->nrow : 0;
    int64_t n_core = n, b = 0;
    int32_t *first = NULL;                                   /* first[r] = the first column of row r of A, -1: none seen yet */
    if (A) {
        first = malloc((size_t)m * sizeof(int32_t));
        if (!first) return -1;
        for (int64_t r = 0; r < m; r++) first[r] = -1;
    }
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = bb_idx(Q->p, Q->itype, j); k < bb_idx(Q->p, Q->itype, j + 1); k++) {
            const int64_t i = bb_idx(Q->i, Q->itype, k);
            if (!bb_q_entry(Q->stype, i, j)) continue;
            const int64_t s = i > j ? i - j : j - i, hi = i > j ? i : j;
            if (s > BAND_BORDER_T && hi < n_core) n_core = hi;
        }
    /* (columns ascending: the first column of a row that exceeds c1 + T is the first one this loop meets, and no later one is smaller) */
    for (int64_t j = 0; A && j < n_core; j++)
        for (int64_t k = bb_idx(A->p, A->itype, j); k < bb_idx(A->p, A->itype, j + 1); k++) {
            const int64_t r = bb_idx(A->i, A->itype, k);
            if (first[r] < 0) first[r] = (int32_t)j;
            else if (j - first[r] > BAND_BORDER_T) { n_core = j; break; }
        }
    /* the core's half-bandwidth: entries with both indices below n_core (first[] holds the first column of every row that has one there) */
    for (int64_t j = 0; j < n_core; j++) {
        for (int64_t k = bb_idx(Q->p, Q->itype, j); k < bb_idx(Q->p, Q->itype, j + 1); k++) {
            const int64_t i = bb_idx(Q->i, Q->itype, k);
            if (i >= n_core || !bb_q_entry(Q->stype, i, j)) continue;
            const int64_t s = i > j ? i - j : j - i;
            if (s > b) b = s;
        }
        for (int64_t k = A ? bb_idx(A->p, A->itype, j) : 0; A && k < bb_idx(A->p, A->itype, j + 1); k++) {
            const int64_t s = j - first[bb_idx(A->i, A->itype, k)];
            if (s > b) b = s;
        }
    }
    free(first);
    const int64_t c = n - n_core;
    info4[0] = (long)n_core; info4[1] = (long)c; info4[2] = (long)(b < 3 ? 3 : b);
    info4[3] = c > max_border ? 1 : 0;                       /* reason: 1 = more border columns than max_border */
    return 0;
}
