/* The fleet's adjoint entry points (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no device is needed:
 * the calls on a NULL fleet are refused under their own names whatever else is passed, and qpdo_amd_fleet_create_ex knows the flag
 * QPDO_AMD_FLEET_ADJOINT alone and beside QPDO_AMD_FLEET_MATRIX_UPDATES (the argument checks behind the flag check are reached) and still
 * refuses every other bit.  Built and run by tests/test_fleet_adjoint_cpu.py, also with -fsanitize=address,undefined on the host driver and
 * on this file. */
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double v[4] = { 1.0, 2.0, 3.0, 4.0 };
    int act[4];
    long st[3];
    QPDOAmdFleetAdjointStats as = { -5, -5 };
    QPDOSettings settings;
    QPDOData d;
    const QPDOData *one[1];
    memset(&d, 0, sizeof(d));
    one[0] = &d;
    qpdo_set_default_settings(&settings);

    EXPECT(qpdo_amd_fleet_adjoint_dev(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 20, 0, 0, 0, 0, NULL) != 0, "adjoint_dev(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_dev: NULL fleet", "adjoint_dev message");
    EXPECT(qpdo_amd_fleet_adjoint_dev(NULL, v, v, v, v, v, v, v, act, st, v, 1e-9, 20, 4, 4, 4, 4, NULL) != 0, "adjoint_dev(NULL, arrays)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_dev: NULL fleet", "adjoint_dev message with arrays");
    EXPECT(qpdo_amd_fleet_adjoint_dev(NULL, v, NULL, v, v, v, NULL, NULL, NULL, NULL, NULL, -1.0, 0, 4, 4, 0, 0, NULL) != 0, "adjoint_dev(NULL, bad knobs)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_dev: NULL fleet", "adjoint_dev message with bad knobs");
    EXPECT(qpdo_amd_fleet_get_adjoint_stats(NULL, &as) != 0 && as.adjoint_calls == -5 && as.resident_extra_bytes == -5, "get_adjoint_stats(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_get_adjoint_stats: NULL fleet", "get_adjoint_stats message");

    /* the flag is known: the checks behind the flag check answer */
    EXPECT(qpdo_amd_fleet_create_ex(0, one, &settings, QPDO_AMD_FLEET_ADJOINT) == NULL, "count 0 with the adjoint flag");
    REFUSED_WITH("count must be positive", "count 0 message");
    EXPECT(qpdo_amd_fleet_create_ex(1, NULL, &settings, QPDO_AMD_FLEET_ADJOINT | QPDO_AMD_FLEET_MATRIX_UPDATES) == NULL, "NULL data with both flags");
    REFUSED_WITH("NULL data array", "NULL data message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, NULL, QPDO_AMD_FLEET_ADJOINT) == NULL, "NULL settings with the adjoint flag");
    REFUSED_WITH("NULL settings", "NULL settings message");
    /* ... and every other bit is still refused */
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &settings, QPDO_AMD_FLEET_ADJOINT | 16L) == NULL, "an unknown bit beside the adjoint flag");
    REFUSED_WITH("unknown flag bits", "unknown bit message");
    REFUSED_WITH("QPDO_AMD_FLEET_ADJOINT", "the message names the new flag");
    EXPECT(QPDO_AMD_FLEET_ADJOINT != QPDO_AMD_FLEET_MATRIX_UPDATES && (QPDO_AMD_FLEET_ADJOINT & (QPDO_AMD_FLEET_ADJOINT - 1)) == 0, "one bit of its own");

    if (failures) return 1;
    printf("fleet adjoint argument checks: all refused before any device call\n");
    return 0;
}
