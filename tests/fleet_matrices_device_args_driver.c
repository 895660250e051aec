/* The fleet's device matrix-update entry points (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no
 * device is needed: the packed value layout is host arithmetic and must be the cumulative sums of the stored entry counts (either itype,
 * an item without A entries and one whose Q stores nothing included), and the calls on a NULL fleet must be refused under their own names.
 * Built and run by tests/test_fleet_matrices_device_cpu.py, also with -fsanitize=address,undefined on the host driver and on this file. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

/* the layout reads p[ncol] of Q and of A alone: `ncol` columns with `per_col` entries each, column pointers of either index type */
typedef struct { cholmod_sparse M; void *p; } Mat;
static void mat_make(Mat *X, size_t nrow, size_t ncol, size_t per_col, int itype, int stype) {
    memset(X, 0, sizeof(*X));
    if (itype == 2) { long *p = malloc((ncol + 1) * sizeof(long)); for (size_t j = 0; j <= ncol; j++) p[j] = (long)(j * per_col); X->p = p; }
    else { int *p = malloc((ncol + 1) * sizeof(int)); for (size_t j = 0; j <= ncol; j++) p[j] = (int)(j * per_col); X->p = p; }
    X->M.nrow = nrow; X->M.ncol = ncol; X->M.nzmax = per_col > 0 ? ncol * per_col : 1; X->M.p = X->p; X->M.itype = itype; X->M.stype = stype;
    X->M.xtype = 1; X->M.sorted = 1; X->M.packed = 1;
}

int main(void) {
    /* item:        0 (int, lower)   1 (long, m = 0)   2 (int, Q stores nothing)   3 (long, full Q) */
    const size_t ns[4] = { 2, 30, 12, 40 }, ms[4] = { 3, 0, 20, 60 }, qper[4] = { 1, 4, 0, 7 }, aper[4] = { 2, 0, 5, 9 };
    const int itypes[4] = { 0, 2, 0, 2 }, stypes[4] = { -1, 1, -1, 0 };
    Mat Q[4], A[4];
    QPDOData d[4];
    const QPDOData *items[4], *with_null[2];
    long qoff[5], aoff[5], big[5];
    memset(d, 0, sizeof(d));
    for (int i = 0; i < 4; i++) {
        mat_make(&Q[i], ns[i], ns[i], qper[i], itypes[i], stypes[i]);
        mat_make(&A[i], ms[i], ns[i], aper[i], itypes[i], 0);
        d[i].n = ns[i]; d[i].m = ms[i]; d[i].Q = &Q[i].M; d[i].A = &A[i].M; items[i] = &d[i];
    }
    with_null[0] = &d[0]; with_null[1] = NULL;
    for (int i = 0; i < 5; i++) qoff[i] = aoff[i] = big[i] = -7;

    EXPECT(qpdo_amd_fleet_packed_matrix_layout(4, items, qoff, aoff) == 0, "packed_matrix_layout");
    EXPECT(qoff[0] == 0 && qoff[1] == 2 && qoff[2] == 122 && qoff[3] == 122 && qoff[4] == 402, "Q offsets (a Q that stores nothing occupies nothing)");
    EXPECT(aoff[0] == 0 && aoff[1] == 4 && aoff[2] == 4 && aoff[3] == 64 && aoff[4] == 424, "A offsets (the m = 0 item occupies nothing)");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(1, items, big, big + 2) == 0 && big[0] == 0 && big[1] == 2 && big[2] == 0 && big[3] == 4 && big[4] == -7,
           "count + 1 entries are written, no more");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(0, items, qoff, aoff) != 0, "count 0");
    REFUSED_WITH("qpdo_amd_fleet_packed_matrix_layout: count must be positive", "count 0 message");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(4, NULL, qoff, aoff) != 0, "NULL data");
    REFUSED_WITH("qpdo_amd_fleet_packed_matrix_layout: NULL data array", "NULL data message");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(4, items, NULL, aoff) != 0, "NULL qoff");
    REFUSED_WITH("qpdo_amd_fleet_packed_matrix_layout: NULL output", "NULL qoff message");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(4, items, qoff, NULL) != 0, "NULL aoff");
    REFUSED_WITH("qpdo_amd_fleet_packed_matrix_layout: NULL output", "NULL aoff message");
    EXPECT(qpdo_amd_fleet_packed_matrix_layout(2, with_null, qoff, aoff) != 0, "NULL item");
    REFUSED_WITH("qpdo_amd_fleet_packed_matrix_layout: NULL item", "NULL item message");

    EXPECT(qpdo_amd_fleet_get_packed_matrix_layout(NULL, qoff, aoff) != 0, "get_packed_matrix_layout(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_get_packed_matrix_layout: NULL fleet", "get_packed_matrix_layout message");
    EXPECT(qpdo_amd_fleet_update_matrices_dev(NULL, NULL, NULL, NULL, 402, 424, NULL) != 0, "update_matrices_dev(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_update_matrices_dev: NULL fleet", "update_matrices_dev message");
    EXPECT(qpdo_amd_fleet_update_matrices_dev(NULL, (const double *)qoff, (const double *)aoff, (const int *)big, 0, 0, NULL) != 0, "update_matrices_dev(NULL, arrays)");
    REFUSED_WITH("qpdo_amd_fleet_update_matrices_dev: NULL fleet", "update_matrices_dev message with arrays");

    for (int i = 0; i < 4; i++) { free(Q[i].p); free(A[i].p); }
    if (failures) return 1;
    printf("fleet device matrix-update argument checks: all refused before any device call\n");
    return 0;
}
