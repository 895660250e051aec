/* A stand-alone caller of qpdo_amd/csrc/band_border.c (that translation unit alone: no device library, no HIP).  Built and run by
 * tests/test_band_border_cpu.py, also with -fsanitize=address,undefined.
 *
 *   band_border_driver detect IN OUT   IN: int64 words -- the number of cases, then per case {itype, stype, n, m, nnz(Q), nnz(A),
 *                                      max_border}, Q's column pointers and row indices, A's column pointers and row indices.  The
 *                                      matrices are rebuilt with int32 or int64 indices as itype says; m = 0 passes A with no rows,
 *                                      m = -1 passes A = NULL.  OUT: per case {rc, info4[4], the second call gave the same output}.
 *   band_border_driver args            the refusals; prints FAIL lines, exit 1 on any.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpdo.h"
#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s\n", what); failures++; } } while (0)

static void *index_array(const int64_t *src, int64_t cnt, int itype) {
    if (itype == 2) { int64_t *a = malloc((size_t)(cnt + 1) * sizeof(int64_t)); memcpy(a, src, (size_t)cnt * sizeof(int64_t)); return a; }
    int32_t *a = malloc((size_t)(cnt + 1) * sizeof(int32_t));
    for (int64_t k = 0; k < cnt; k++) a[k] = (int32_t)src[k];
    return a;
}
static int run_detect(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) { perror(in_path); return 2; }
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    int64_t *w = malloc((size_t)bytes + 8);
    if (fread(w, 1, (size_t)bytes, f) != (size_t)bytes) { fclose(f); free(w); return 2; }
    fclose(f);
    FILE *o = fopen(out_path, "wb");
    if (!o) { perror(out_path); free(w); return 2; }
    const int64_t *p = w;
    const int64_t ncases = *p++;
    for (int64_t c = 0; c < ncases; c++) {
        const int itype = (int)p[0], stype = (int)p[1];
        const int64_t n = p[2], m = p[3], qnnz = p[4], annz = p[5], max_border = p[6];
        p += 7;
        cholmod_sparse Q, A;
        memset(&Q, 0, sizeof(Q)); memset(&A, 0, sizeof(A));
        Q.nrow = Q.ncol = (size_t)n; Q.nzmax = (size_t)qnnz; Q.stype = stype; Q.itype = itype; Q.xtype = 1; Q.packed = 1;
        A.nrow = (size_t)(m < 0 ? 0 : m); A.ncol = (size_t)n; A.nzmax = (size_t)annz; A.itype = itype; A.xtype = 1; A.packed = 1;
        Q.p = index_array(p, n + 1, itype); p += n + 1;
        Q.i = index_array(p, qnnz, itype); p += qnnz;
        A.p = index_array(p, n + 1, itype); p += n + 1;
        A.i = index_array(p, annz, itype); p += annz;
        long i1[4] = {-1, -1, -1, -1}, i2[4] = {-2, -2, -2, -2};
        const cholmod_sparse *Ap = m < 0 ? NULL : &A;
        const int rc = qpdo_amd_band_border(&Q, Ap, (long)max_border, i1), rc2 = qpdo_amd_band_border(&Q, Ap, (long)max_border, i2);
        int64_t head[6] = {rc, i1[0], i1[1], i1[2], i1[3], rc == rc2 && !memcmp(i1, i2, sizeof(i1))};
        fwrite(head, sizeof(int64_t), 6, o);
        free(Q.p); free(Q.i); free(A.p); free(A.i);
    }
    fclose(o); free(w);
    return 0;
}
static int run_args(void) {
    long info[4] = {7, 7, 7, 7};
    int32_t p0[1] = {0};
    cholmod_sparse Q, A;
    memset(&Q, 0, sizeof(Q)); memset(&A, 0, sizeof(A));
    Q.p = p0; Q.i = p0; Q.stype = -1;
    EXPECT(qpdo_amd_band_border(NULL, NULL, 4, info) == -1, "no Q is refused");
    EXPECT(qpdo_amd_band_border(&Q, NULL, 4, NULL) == -1, "no info4 is refused");
    EXPECT(qpdo_amd_band_border(&Q, NULL, 4, info) == 0 && info[0] == 0 && info[1] == 0 && info[2] == 3 && info[3] == 0, "n = 0: no core, no border");
    Q.itype = 1;
    EXPECT(qpdo_amd_band_border(&Q, NULL, 4, info) == -1, "an unknown itype is refused");
    Q.itype = 0; Q.nrow = 2; Q.ncol = 3;
    EXPECT(qpdo_amd_band_border(&Q, NULL, 4, info) == -1, "a Q that is not square is refused");
    Q.nrow = Q.ncol = 0; A.p = p0; A.i = p0; A.nrow = 1; A.ncol = 5;
    EXPECT(qpdo_amd_band_border(&Q, &A, 4, info) == -1, "an A with another number of columns is refused");
    printf(failures ? "%d FAILURES\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "detect")) return run_detect(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "args")) return run_args();
    fprintf(stderr, "usage: %s detect IN OUT | args\n", argv[0]);
    return 2;
}
