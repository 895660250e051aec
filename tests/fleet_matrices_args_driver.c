/* The argument checks of the fleet's matrix-update entry points (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller:
 * every call here must be refused before the library touches a device, with a message in qpdo_amd_last_error().  Built and run by
 * tests/test_fleet_matrices_cpu.py, also with -fsanitize=address,undefined on the host driver and on this file. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

/* a diagonal QP in n variables with one row per variable; lower_above: l[1] > u[1] */
typedef struct { QPDOData d; cholmod_sparse Q, A; long *p, *i; double *x, *q, *l, *u; } Prob;
static void prob_make(Prob *P, size_t n, int lower_above) {
    memset(P, 0, sizeof(*P));
    P->p = malloc((n + 1) * sizeof(long)); P->i = malloc(n * sizeof(long)); P->x = malloc(n * sizeof(double));
    P->q = malloc(n * sizeof(double)); P->l = malloc(n * sizeof(double)); P->u = malloc(n * sizeof(double));
    for (size_t k = 0; k < n; k++) { P->p[k] = (long)k; P->i[k] = (long)k; P->x[k] = 1.0 + (double)k; P->q[k] = -1.0; P->l[k] = -1.0; P->u[k] = 1.0; }
    P->p[n] = (long)n;
    if (lower_above) P->l[1] = 2.0;
    cholmod_sparse M;
    memset(&M, 0, sizeof(M));
    M.nrow = n; M.ncol = n; M.nzmax = n; M.p = P->p; M.i = P->i; M.x = P->x; M.itype = 2; M.xtype = 1; M.dtype = 0; M.sorted = 1; M.packed = 1;
    P->Q = M; P->Q.stype = -1;
    P->A = M; P->A.stype = 0;
    P->d.n = n; P->d.m = n; P->d.Q = &P->Q; P->d.A = &P->A; P->d.q = P->q; P->d.c = 0.0; P->d.l = P->l; P->d.u = P->u;
}
static void prob_free(Prob *P) { free(P->p); free(P->i); free(P->x); free(P->q); free(P->l); free(P->u); }

int main(void) {
    QPDOSettings st, bad;
    QPDOAmdFleetMatrixStats ms;
    Prob ok, big, crossed;
    qpdo_set_default_settings(&st);
    st.verbose = 0;
    prob_make(&ok, 8, 0); prob_make(&big, 1500, 0); prob_make(&crossed, 8, 1);
    const QPDOData *one[1] = { &ok.d };
    const QPDOData *with_big[2] = { &ok.d, &big.d };
    const QPDOData *with_crossed[2] = { &ok.d, &crossed.d };
    const QPDOData *with_null[2] = { &ok.d, NULL };
    const cholmod_sparse *mats[1] = { &ok.A };
    const long F = QPDO_AMD_FLEET_MATRIX_UPDATES;

    EXPECT(qpdo_amd_fleet_create_ex(1, one, &st, 2L) == NULL, "flag bit 1"); REFUSED_WITH("unknown flag bits", "flag bit 1 message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &st, F | 4L) == NULL, "flag bit 2 beside the known one"); REFUSED_WITH("unknown flag bits", "flag bit 2 message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &st, -1L) == NULL, "all flag bits"); REFUSED_WITH("unknown flag bits", "all flag bits message");
    EXPECT(qpdo_amd_fleet_create_ex(0, one, &st, F) == NULL, "count 0"); REFUSED_WITH("count must be positive", "count 0 message");
    EXPECT(qpdo_amd_fleet_create_ex(1, NULL, &st, F) == NULL, "NULL data"); REFUSED_WITH("NULL data array", "NULL data message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, NULL, F) == NULL, "NULL settings"); REFUSED_WITH("NULL settings", "NULL settings message");
    bad = st; bad.rho = 2.0;
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &bad, F) == NULL, "invalid settings"); REFUSED_WITH("invalid settings", "invalid settings message");
    EXPECT(qpdo_amd_fleet_create_ex(2, with_big, &st, F) == NULL, "n = 1500"); REFUSED_WITH("item 1 does not fit the fused kernel", "n = 1500 message");
    EXPECT(qpdo_amd_fleet_create_ex(2, with_null, &st, 0L) == NULL, "NULL item"); REFUSED_WITH("item 1 does not fit the fused kernel", "NULL item message");
    EXPECT(qpdo_amd_fleet_create_ex(2, with_crossed, &st, F) == NULL, "l > u"); REFUSED_WITH("item 1 has a lower bound above its upper bound", "l > u message");

    EXPECT(qpdo_amd_fleet_update_matrices(NULL, mats, mats) != 0, "update_matrices(NULL)"); REFUSED_WITH("qpdo_amd_fleet_update_matrices: NULL fleet", "update_matrices message");
    EXPECT(qpdo_amd_fleet_update_matrices(NULL, NULL, NULL) != 0, "update_matrices(NULL, NULL, NULL)"); REFUSED_WITH("NULL fleet", "update_matrices message");
    EXPECT(qpdo_amd_fleet_get_matrix_stats(NULL, &ms) != 0, "get_matrix_stats(NULL)"); REFUSED_WITH("qpdo_amd_fleet_get_matrix_stats: NULL fleet", "get_matrix_stats message");

    prob_free(&ok); prob_free(&big); prob_free(&crossed);
    if (failures) return 1;
    printf("fleet matrix-update argument checks: all refused before any device call\n");
    return 0;
}
