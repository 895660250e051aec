/* qpdo_amd_rhs_group, qpdo_amd_get_group_stats and qpdo_amd_spmv_group (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C
 * caller, as far as no workspace is needed: every check that comes before the backend is touched, by message -- each refused call below
 * carries a NULL workspace behind the fault under test, so the message shows that the check came first.  Built and run by
 * tests/test_workspace_group_cpu.py, also with -fsanitize=address,undefined on the host driver and on this file. */
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double v[8] = { 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0 }, y[8] = { 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0 };
    QPDOAmdGroupStats gs = { -5, -5, -5, -5 };

    EXPECT(sizeof(QPDOAmdGroupStats) == 32, "the group stats struct is 32 bytes");
    EXPECT(qpdo_amd_rhs_group(NULL) == -1, "rhs_group(NULL) is -1");

    EXPECT(qpdo_amd_get_group_stats(NULL, &gs) != 0 && gs.group == -5 && gs.groups_run == -5 && gs.rounds_total == -5 && gs.scratch_bytes == -5,
           "get_group_stats(NULL) leaves the struct untouched");
    REFUSED_WITH("qpdo_amd_get_group_stats: NULL workspace", "get_group_stats message");

    /* nvec out of range */
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 0, 0u, v, y) != 0, "nvec 0");
    REFUSED_WITH("qpdo_amd_spmv_group: nvec must be 1 .. 8", "nvec 0 message");
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 9, 1u, v, y) != 0, "nvec 9");
    REFUSED_WITH("qpdo_amd_spmv_group: nvec must be 1 .. 8", "nvec 9 message");
    EXPECT(qpdo_amd_spmv_group(NULL, 0, -1, 1u, v, y) != 0, "nvec -1");
    REFUSED_WITH("nvec must be 1 .. 8", "negative nvec message");
    /* a mask bit >= nvec */
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 3, 0x8u, v, y) != 0, "mask bit 3 with nvec 3");
    REFUSED_WITH("qpdo_amd_spmv_group: live_mask names a vector >= nvec", "mask message");
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 8, 0x100u, v, y) != 0, "mask bit 8 with nvec 8");
    REFUSED_WITH("live_mask names a vector >= nvec", "mask message at nvec 8");
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 1, 0x80000000u, v, y) != 0, "mask bit 31 with nvec 1");
    REFUSED_WITH("live_mask names a vector >= nvec", "mask message, top bit");
    /* which */
    EXPECT(qpdo_amd_spmv_group(NULL, 3, 2, 3u, v, y) != 0, "which 3");
    REFUSED_WITH("qpdo_amd_spmv_group: which is 0 (A), 1 (A') or 2 (Q)", "which message");
    /* NULL pointers -- v before y */
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 2, 3u, NULL, NULL) != 0, "NULL v");
    REFUSED_WITH("qpdo_amd_spmv_group: v is NULL", "v message");
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 2, 3u, v, NULL) != 0, "NULL y");
    REFUSED_WITH("qpdo_amd_spmv_group: y is NULL", "y message");
    /* NULL workspace: the last of the checks */
    EXPECT(qpdo_amd_spmv_group(NULL, 0, 2, 3u, v, y) != 0, "NULL workspace");
    REFUSED_WITH("qpdo_amd_spmv_group: NULL workspace", "workspace message");
    EXPECT(y[0] == 7.0 && y[3] == 7.0 && y[7] == 7.0, "a refused call leaves y untouched");

    if (failures) return 1;
    printf("workspace group argument checks: all refused before any device call\n");
    return 0;
}
