/* Stand-alone caller of qpdo_amd/csrc/csc_convert.c (no device library, no HIP): reads records of raw arrays from argv[1], converts
 * them and writes the results to argv[2].  One ConvScratch serves every record, so the grow-only scratch is reused across sizes.
 * Built and run by tests/test_csc_convert_cpu.py, also with -fsanitize=address,undefined.
 *
 * record : int64 {op, threads, world, nmat}, then nmat matrices
 * matrix : int64 {nrow, ncol, nnz, itype, stype}, p[ncol + 1], i[nnz] (int32 for itype 0, int64 for itype 2), x[nnz] doubles
 * op 0   : CSR(M) and CSR(M')  -> int64 rc; rp[nrow + 1] ci[nnz] val[nnz] map[nnz]; rp[ncol + 1] ci[nnz] val[nnz]
 * op 1   : full symmetric CSR  -> int64 {count, rc}; when rc == 0: rp[n + 1] ci[count] val[count] map[count]
 * op 2   : matrices A, Q; the row partition over `world` ranks -> per rank int32 {m0, mloc, n0, nloc}, then Al, Tl, Ql each as
 *          rp[nrows + 1] ci[nnz] val[nnz]
 * Every output array is allocated at exactly its stated size, so a write past it is a sanitizer report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "csc_convert.h"

static FILE *fin, *fout;
static void die(const char *what) { fprintf(stderr, "csc_convert_driver: %s\n", what); exit(2); }
static void *xmalloc(size_t bytes) { void *p = malloc(bytes ? bytes : 1); if (!p) die("out of memory"); return p; }
static void get(void *dst, size_t bytes) { if (bytes && fread(dst, 1, bytes, fin) != bytes) die("short input"); }
static void put(const void *src, size_t bytes) { if (bytes && fwrite(src, 1, bytes, fout) != bytes) die("short write"); }

static void read_matrix(cholmod_sparse *M) {
    int64_t h[5];
    get(h, sizeof(h));
    memset(M, 0, sizeof(*M));
    M->nrow = (size_t)h[0]; M->ncol = (size_t)h[1]; M->nzmax = (size_t)h[2]; M->itype = (int)h[3]; M->stype = (int)h[4];
    M->xtype = 1; M->sorted = 1; M->packed = 1;
    const size_t w = M->itype == 0 ? 4 : 8;
    M->p = xmalloc((M->ncol + 1) * w); M->i = xmalloc(M->nzmax * w); M->x = xmalloc(M->nzmax * 8);
    get(M->p, (M->ncol + 1) * w); get(M->i, M->nzmax * w); get(M->x, M->nzmax * 8);
}
static void free_matrix(cholmod_sparse *M) { free(M->p); free(M->i); free(M->x); }
static void put_csr(const HostCsr *h) { put(h->rp, ((size_t)h->nrows + 1) * 4); put(h->ci, (size_t)h->nnz * 4); put(h->val, (size_t)h->nnz * 8); }

/* an image in arrays of exactly cap entries */
static void alloc_csr(HostCsr *h, size_t nrows, size_t ncols, size_t cap) {
    h->nrows = (int32_t)nrows; h->ncols = (int32_t)ncols; h->nnz = (int64_t)cap;
    h->rp = xmalloc((nrows + 1) * 4); h->ci = xmalloc(cap * 4); h->val = xmalloc(cap * 8);
}

int main(int argc, char **argv) {
    if (argc != 3) die("usage: csc_convert_driver IN OUT");
    fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
    if (!fin || !fout) die("cannot open the files");
    ConvScratch W;
    conv_scratch_init(&W);
    int64_t hdr[4];
    long records = 0;
    while (fread(hdr, 1, sizeof(hdr), fin) == sizeof(hdr)) {
        const int op = (int)hdr[0], threads = (int)hdr[1], world = (int)hdr[2];
        cholmod_sparse M[2];
        if (hdr[3] < 1 || hdr[3] > 2) die("bad record");
        for (int k = 0; k < hdr[3]; k++) read_matrix(&M[k]);
        const size_t nnz = M[0].nzmax;
        if (op == 0) {
            HostCsr R, T;
            alloc_csr(&R, M[0].nrow, M[0].ncol, nnz); alloc_csr(&T, M[0].ncol, M[0].nrow, nnz);
            int32_t *map = xmalloc(nnz * 4);
            const int64_t rc = csc_to_csr(&M[0], R.rp, R.ci, R.val, map, threads, &W);
            csc_as_csr_of_transpose(&M[0], T.rp, T.ci, T.val, threads);
            put(&rc, 8); put_csr(&R); put(map, nnz * 4); put_csr(&T);
            host_csr_free(&R); host_csr_free(&T); free(map);
        } else if (op == 1) {
            int64_t out[2];
            out[0] = sym_full_nnz(&M[0]);
            HostCsr F;
            alloc_csr(&F, M[0].ncol, M[0].ncol, (size_t)out[0]);
            int32_t *map = xmalloc((size_t)out[0] * 4);
            out[1] = sym_to_full_csr(&M[0], F.rp, F.ci, F.val, map, threads, &W);
            put(out, 16);
            if (out[1] == 0) { put_csr(&F); put(map, (size_t)out[0] * 4); }
            host_csr_free(&F); free(map);
        } else if (op == 2) {
            HostCsr Ar, At, Qf;
            alloc_csr(&Ar, M[0].nrow, M[0].ncol, nnz); alloc_csr(&At, M[0].ncol, M[0].nrow, nnz);
            alloc_csr(&Qf, M[1].ncol, M[1].ncol, (size_t)sym_full_nnz(&M[1]));
            if (csc_to_csr(&M[0], Ar.rp, Ar.ci, Ar.val, NULL, threads, &W)) die("csc_to_csr failed");
            csc_as_csr_of_transpose(&M[0], At.rp, At.ci, At.val, threads);
            if (sym_to_full_csr(&M[1], Qf.rp, Qf.ci, Qf.val, NULL, threads, &W)) die("sym_to_full_csr failed");
            for (int rank = 0; rank < world; rank++) {
                RowPartition P;
                if (cut_row_partition(&Ar, &At, &Qf, rank, world, &P)) die("cut_row_partition failed");
                const int32_t r[4] = {P.m0, P.mloc, P.n0, P.nloc};
                put(r, sizeof(r)); put_csr(&P.Al); put_csr(&P.Tl); put_csr(&P.Ql);
                row_partition_free(&P);
            }
            host_csr_free(&Ar); host_csr_free(&At); host_csr_free(&Qf);
        } else die("unknown op");
        for (int k = 0; k < hdr[3]; k++) free_matrix(&M[k]);
        records++;
    }
    conv_scratch_free(&W);
    if (fclose(fout)) die("close failed");
    fclose(fin);
    printf("converted %ld records\n", records);
    return 0;
}
