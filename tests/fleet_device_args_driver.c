/* The fleet's device entry points (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no device is needed:
 * the packed layout is host arithmetic and must be the cumulative sums (an m = 0 item included), and every call on a NULL fleet must be
 * refused under its own name.  Built and run by tests/test_fleet_device_cpu.py, also with -fsanitize=address,undefined on the host
 * driver and on this file. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    /* the layout reads n and m alone */
    const size_t ns[4] = { 2, 30, 12, 40 }, ms[4] = { 3, 0, 20, 60 };
    QPDOData d[4];
    const QPDOData *items[4], *with_null[2];
    long noff[5], moff[5], big[5];
    QPDOInfo info[1];
    QPDOAmdFleetDevStats ds;
    memset(d, 0, sizeof(d));
    for (int i = 0; i < 4; i++) { d[i].n = ns[i]; d[i].m = ms[i]; items[i] = &d[i]; }
    with_null[0] = &d[0]; with_null[1] = NULL;
    for (int i = 0; i < 5; i++) noff[i] = moff[i] = big[i] = -7;

    EXPECT(qpdo_amd_fleet_packed_layout(4, items, noff, moff) == 0, "packed_layout");
    EXPECT(noff[0] == 0 && noff[1] == 2 && noff[2] == 32 && noff[3] == 44 && noff[4] == 84, "n offsets");
    EXPECT(moff[0] == 0 && moff[1] == 3 && moff[2] == 3 && moff[3] == 23 && moff[4] == 83, "m offsets (the m = 0 item occupies nothing)");
    EXPECT(qpdo_amd_fleet_packed_layout(1, items, big, big + 2) == 0 && big[0] == 0 && big[1] == 2 && big[2] == 0 && big[3] == 3 && big[4] == -7,
           "count + 1 entries are written, no more");
    EXPECT(qpdo_amd_fleet_packed_layout(0, items, noff, moff) != 0, "count 0"); REFUSED_WITH("qpdo_amd_fleet_packed_layout: count must be positive", "count 0 message");
    EXPECT(qpdo_amd_fleet_packed_layout(4, NULL, noff, moff) != 0, "NULL data"); REFUSED_WITH("qpdo_amd_fleet_packed_layout: NULL data array", "NULL data message");
    EXPECT(qpdo_amd_fleet_packed_layout(4, items, NULL, moff) != 0, "NULL noff"); REFUSED_WITH("qpdo_amd_fleet_packed_layout: NULL output", "NULL noff message");
    EXPECT(qpdo_amd_fleet_packed_layout(4, items, noff, NULL) != 0, "NULL moff"); REFUSED_WITH("qpdo_amd_fleet_packed_layout: NULL output", "NULL moff message");
    EXPECT(qpdo_amd_fleet_packed_layout(2, with_null, noff, moff) != 0, "NULL item"); REFUSED_WITH("qpdo_amd_fleet_packed_layout: NULL item", "NULL item message");

    EXPECT(qpdo_amd_fleet_get_packed_layout(NULL, noff, moff) != 0, "get_packed_layout(NULL)"); REFUSED_WITH("qpdo_amd_fleet_get_packed_layout: NULL fleet", "get_packed_layout message");
    EXPECT(qpdo_amd_fleet_device(NULL) == -1, "device(NULL)"); REFUSED_WITH("qpdo_amd_fleet_device: NULL fleet", "device message");
    EXPECT(qpdo_amd_fleet_update_dev(NULL, NULL, NULL, NULL, NULL, 84, 83, NULL) != 0, "update_dev(NULL)"); REFUSED_WITH("qpdo_amd_fleet_update_dev: NULL fleet", "update_dev message");
    EXPECT(qpdo_amd_fleet_warm_start_dev(NULL, NULL, NULL, NULL, 84, 83, NULL) != 0, "warm_start_dev(NULL)"); REFUSED_WITH("qpdo_amd_fleet_warm_start_dev: NULL fleet", "warm_start_dev message");
    EXPECT(qpdo_amd_fleet_warm_start_last_dev(NULL, NULL) != 0, "warm_start_last_dev(NULL)"); REFUSED_WITH("qpdo_amd_fleet_warm_start_last_dev: NULL fleet", "warm_start_last_dev message");
    EXPECT(qpdo_amd_fleet_solve_dev(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 84, 83, NULL) != 0, "solve_dev(NULL)"); REFUSED_WITH("qpdo_amd_fleet_solve_dev: NULL fleet", "solve_dev message");
    EXPECT(qpdo_amd_fleet_fetch_last(NULL, NULL, NULL, info) != 0, "fetch_last(NULL)"); REFUSED_WITH("qpdo_amd_fleet_fetch_last: NULL fleet", "fetch_last message");
    EXPECT(qpdo_amd_fleet_sync(NULL, &ds) != 0, "sync(NULL)"); REFUSED_WITH("qpdo_amd_fleet_sync: NULL fleet", "sync message");

    if (failures) return 1;
    printf("fleet device-call argument checks: all refused before any device call\n");
    return 0;
}
