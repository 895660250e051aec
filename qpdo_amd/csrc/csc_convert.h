/*
 * csc_convert.h -- the one host conversion from the caller's CSC matrices (cholmod_sparse, int32 or int64 indices) to the
 * three int32 CSR images every entry point puts on the device: CSR(A), CSR(A') and the full symmetric CSR(Q).
 *
 * The ordering contract (bit-for-bit parity with the oracle depends on the order in which each row's products are summed;
 * the device transposition of dev/transpose.inc produces the same arrays):
 *   - rows come out column-sorted for column-sorted input;
 *   - row i of the full Q from a lower triangle (stype -1) is CSR row i of the triangle (columns <= i, ascending) followed by
 *     the stored column i below the diagonal (ascending rows = ascending columns of the mirror); from an upper triangle
 *     (stype +1) the stored column i above the diagonal, then CSR row i (columns >= i);
 *   - entries on the wrong side of the stored triangle are ignored, as CHOLMOD does for stype != 0.
 *
 * Every function writes into arrays of the caller.  `map` (optional, may be NULL): map[s] = position in the caller's CSC
 * values that entry s of the CSR image was taken from.  `threads`: T > 0 runs on T OpenMP threads, asked for explicitly;
 * T <= 0 takes min(16, cores) and stays serial below 200000 entries.  The output is the same for every T; T = 1 never enters
 * the OpenMP runtime (the batch and fleet paths call it from host threads of their own).
 */
#ifndef QPDO_CSC_CONVERT_H
#define QPDO_CSC_CONVERT_H

#include <stddef.h>
#include <stdint.h>

#include "qpdo.h"

#ifdef __cplusplus
extern "C" {
#endif
/* internal to libqpdo_amd.so: none of these names is exported */
#pragma GCC visibility push(hidden)

/* the 32/64-bit index read (itype 0: int32, otherwise int64) */
static inline int64_t idx_at(const void *a, int itype, int64_t k) {
    return itype == 0 ? (int64_t)((const int32_t *)a)[k] : (int64_t)((const int64_t *)a)[k];
}

/* temporaries of the conversions; the caller's, grow-only, kept between calls.  All zero is the empty state. */
typedef struct { void *p; size_t cap; } ConvBuf;
typedef struct {
    ConvBuf cnt, cut;               /* csc_to_csr: per-thread row counts (T x nrows), column ranges (T + 1) */
    ConvBuf rrp, rci, rval, rmap;   /* sym_to_full_csr: CSR of the stored matrix */
} ConvScratch;
void conv_scratch_init(ConvScratch *W);
void conv_scratch_free(ConvScratch *W);

/* CSR of the r x c matrix itself: rp[r + 1], ci / val / map[nnz].  Returns 0, or -1 when the scratch cannot grow. */
int csc_to_csr(const cholmod_sparse *M, int32_t *rp, int32_t *ci, double *val, int32_t *map, int threads, ConvScratch *W);
/* CSR of the c x r transpose: the CSC arrays narrowed to 32 bits.  rp[c + 1], ci / val[nnz]. */
void csc_as_csr_of_transpose(const cholmod_sparse *M, int32_t *rp, int32_t *ci, double *val, int threads);
/* entries of the full symmetric Q: the stored triangle once, its strict part mirrored (stype 0: the stored entries) */
int64_t sym_full_nnz(const cholmod_sparse *Q);
/* full symmetric CSR of Q from stype -1 / +1 / 0: rp[n + 1], ci / val / map with room for sym_full_nnz(Q) entries (at most twice
 * the stored ones).  Returns 0, or -1 -- before ci / val / map are written -- when the count reaches INT32_MAX or the scratch
 * cannot grow.  stype 0: the narrowing copy; map[s] = s. */
int sym_to_full_csr(const cholmod_sparse *Q, int32_t *rp, int32_t *ci, double *val, int32_t *map, int threads, ConvScratch *W);

/* ---- an owned CSR triple, and the row partition of the three images over `world` ranks ------------------------------- */
typedef struct { int32_t nrows, ncols; int64_t nnz; int32_t *rp, *ci; double *val; } HostCsr;
void host_csr_free(HostCsr *h);
/* Rank `rank` holds rows [m0, m0 + mloc) of A, with ceil(m / world) rows per rank clipped to m, and rows [n0, n0 + nloc) of Q
 * likewise.  Al and Ql are those rows of Ar and Qf: row pointers of their own, rebased to 0; ci and val point INTO Ar / Qf.
 * Tl is At restricted to the columns [m0, m0 + mloc), renumbered from 0, in arrays of its own. */
typedef struct { int32_t m0, mloc, n0, nloc; HostCsr Al, Tl, Ql; } RowPartition;
int cut_row_partition(const HostCsr *Ar, const HostCsr *At, const HostCsr *Qf, int rank, int world, RowPartition *out);      /* 0, or -1: no memory */
void row_partition_free(RowPartition *P);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
