/* A stand-alone caller of qpdo_amd/csrc/band_order.c (that translation unit alone: no device library, no HIP).  Built and run by
 * tests/test_band_order_cpu.py, also with -fsanitize=address,undefined.
 *
 *   band_order_driver order IN OUT   IN: int64 words -- the number of cases, then per case {itype, stype, n, m, nnz(Q), nnz(A)},
 *                                    Q's column pointers and row indices, A's column pointers and row indices.  The matrices are
 *                                    rebuilt with int32 or int64 indices as itype says.  OUT: per case {rc, info4[4], the second
 *                                    call gave the same output (1 / 0), band_order_bandwidth of the caller's order, of newold},
 *                                    newold[n].
 *   band_order_driver config         the refusals of qpdo_amd_band_order_config and of a setup's snapshot; prints FAIL lines, exit 1 on any.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "band_order.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s\n", what); failures++; } } while (0)

static void *index_array(const int64_t *src, int64_t cnt, int itype) {
    if (itype == 2) { int64_t *a = malloc((size_t)(cnt + 1) * sizeof(int64_t)); memcpy(a, src, (size_t)cnt * sizeof(int64_t)); return a; }
    int32_t *a = malloc((size_t)(cnt + 1) * sizeof(int32_t));
    for (int64_t k = 0; k < cnt; k++) a[k] = (int32_t)src[k];
    return a;
}
static int run_order(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) { perror(in_path); return 2; }
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    int64_t *w = malloc((size_t)bytes + 8);
    if (fread(w, 1, (size_t)bytes, f) != (size_t)bytes) { fclose(f); return 2; }
    fclose(f);
    FILE *o = fopen(out_path, "wb");
    if (!o) { perror(out_path); return 2; }
    const int64_t *p = w;
    const int64_t ncases = *p++;
    for (int64_t c = 0; c < ncases; c++) {
        const int itype = (int)p[0], stype = (int)p[1];
        const int64_t n = p[2], m = p[3], qnnz = p[4], annz = p[5];
        p += 6;
        cholmod_sparse Q, A;
        memset(&Q, 0, sizeof(Q)); memset(&A, 0, sizeof(A));
        Q.nrow = Q.ncol = (size_t)n; Q.nzmax = (size_t)qnnz; Q.stype = stype; Q.itype = itype; Q.xtype = 1; Q.sorted = 1; Q.packed = 1;
        A.nrow = (size_t)m; A.ncol = (size_t)n; A.nzmax = (size_t)annz; A.itype = itype; A.xtype = 1; A.sorted = 1; A.packed = 1;
        Q.p = index_array(p, n + 1, itype); p += n + 1;
        Q.i = index_array(p, qnnz, itype); p += qnnz;
        A.p = index_array(p, n + 1, itype); p += n + 1;
        A.i = index_array(p, annz, itype); p += annz;
        long *no1 = malloc((size_t)(n + 1) * sizeof(long)), *no2 = malloc((size_t)(n + 1) * sizeof(long));
        int32_t *oldnew = malloc((size_t)(n + 1) * sizeof(int32_t));
        long i1[4] = {-1, -1, -1, -1}, i2[4] = {-2, -2, -2, -2};
        const int rc = qpdo_amd_band_order(&Q, &A, no1, i1), rc2 = qpdo_amd_band_order(&Q, &A, no2, i2);
        const int same = rc == rc2 && !memcmp(i1, i2, sizeof(i1)) && !memcmp(no1, no2, (size_t)n * sizeof(long));
        for (int64_t k = 0; k < n; k++) if (no1[k] >= 0 && no1[k] < n) oldnew[no1[k]] = (int32_t)k;
        int64_t head[8] = {rc, i1[0], i1[1], i1[2], i1[3], same, band_order_bandwidth(&Q, &A, NULL), rc ? -1 : band_order_bandwidth(&Q, &A, oldnew)};
        fwrite(head, sizeof(int64_t), 8, o);
        for (int64_t k = 0; k < n; k++) { const int64_t v = no1[k]; fwrite(&v, sizeof(v), 1, o); }
        free(no1); free(no2); free(oldnew); free(Q.p); free(Q.i); free(A.p); free(A.i);
    }
    fclose(o); free(w);
    return 0;
}
static int run_config(void) {
    char msg[256] = "";
    int mode = -1; int32_t *no = NULL;
    const long perm[5] = {4, 2, 0, 1, 3}, twice[5] = {4, 2, 0, 2, 3}, range[5] = {4, 2, 0, 5, 3}, neg[5] = {4, 2, 0, -1, 3};
    EXPECT(qpdo_amd_band_order_config(4, NULL, 0) == -1 && qpdo_amd_band_order_config(-1, NULL, 0) == -1, "an unknown mode is refused");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, twice, 5) == -1, "a repeated index is refused");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, range, 5) == -1, "an index >= n is refused");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, neg, 5) == -1, "a negative index is refused");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, NULL, 5) == -1, "a given order without newold is refused");
    /* the refused calls left the default: the environment decides */
    unsetenv("QPDO_BAND_ORDER");
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_NATURAL && !no, "default: natural");
    setenv("QPDO_BAND_ORDER", "rcm", 1);
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_RCM && !no, "QPDO_BAND_ORDER=rcm");
    setenv("QPDO_BAND_ORDER", "0", 1);
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_NATURAL, "QPDO_BAND_ORDER=0");
    setenv("QPDO_BAND_ORDER", "amd", 1);
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == -1 && strstr(msg, "QPDO_BAND_ORDER=amd"), "an unknown QPDO_BAND_ORDER fails the setup");
    /* an explicit mode overrides the variable */
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_NATURAL, NULL, 0) == 0, "natural is accepted");
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_NATURAL, "config overrides the environment");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, perm, 5) == 0, "a permutation is accepted");
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_GIVEN && no, "a given order reaches the setup");
    if (no) { int ok = 1; for (int k = 0; k < 5; k++) ok = ok && no[k] == perm[k]; EXPECT(ok, "... as a copy of newold"); free(no); no = NULL; }
    EXPECT(band_order_snapshot(6, &mode, &no, msg, sizeof(msg)) == -1 && !no && strstr(msg, "5 entries") && strstr(msg, "6 variables"),
           "a workspace of another n fails with a message that names both");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, twice, 5) == -1, "a refused call ...");
    EXPECT(band_order_snapshot(5, &mode, &no, msg, sizeof(msg)) == 0 && mode == QPDO_AMD_BAND_ORDER_GIVEN && no && no[0] == 4, "... leaves the configuration as it was");
    free(no); no = NULL;
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_GIVEN, perm, 0) == 0, "an empty order is a permutation");
    EXPECT(qpdo_amd_band_order_config(QPDO_AMD_BAND_ORDER_ENV, NULL, 0) == 0, "back to the default (frees the copy)");
    EXPECT(qpdo_amd_band_order(NULL, NULL, NULL, NULL) == -1, "qpdo_amd_band_order without a matrix is refused");
    printf(failures ? "%d FAILURES\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "order")) return run_order(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "config")) return run_config();
    fprintf(stderr, "usage: %s order IN OUT | config\n", argv[0]);
    return 2;
}
