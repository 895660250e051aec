/* The fleet's many-right-hand-side entry points (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no device
 * is needed: the calls on a NULL fleet are refused under their own names whatever else is passed.  The nrhs < 1 check itself is NOT
 * covered here: it stands behind the NULL-fleet check and a fleet cannot be created without a device, so its message is exercised by the
 * GPU refusal test (tests/_fleet_sensitivity_worker.py); this file only shows that a NULL fleet answers first when nrhs is 0 or negative.
 * Further: qpdo_amd_fleet_rhs_group(NULL) is -1, the stats struct has its three members, the
 * older structs keep their sizes, and qpdo_amd_fleet_create_ex has NO new flag: it knows QPDO_AMD_FLEET_ADJOINT and
 * QPDO_AMD_FLEET_MATRIX_UPDATES and still refuses bit 16.  Built and run by tests/test_fleet_sensitivity_cpu.py, also with
 * -fsanitize=address,undefined on the host driver and on this file. */
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double v[8] = { 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0 };
    int act[4];
    long st[6];
    QPDOAmdFleetSensitivityStats ss = { -5, -5, -5 };
    QPDOSettings settings;
    QPDOData d;
    const QPDOData *one[1];
    memset(&d, 0, sizeof(d));
    one[0] = &d;
    qpdo_set_default_settings(&settings);

    EXPECT(qpdo_amd_fleet_adjoint_multi_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 20, 0, 0, 0, 0, NULL) != 0, "adjoint_multi_dev(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_multi_dev: NULL fleet", "adjoint_multi_dev message");
    EXPECT(qpdo_amd_fleet_adjoint_multi_dev(NULL, 2, v, v, v, v, v, v, v, act, st, v, 1e-9, 20, 4, 4, 4, 4, NULL) != 0, "adjoint_multi_dev(NULL, arrays)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_multi_dev: NULL fleet", "adjoint_multi_dev message with arrays");
    EXPECT(qpdo_amd_fleet_adjoint_multi_dev(NULL, 0, v, NULL, v, v, v, NULL, NULL, NULL, NULL, NULL, -1.0, 0, 4, 4, 0, 0, NULL) != 0, "adjoint_multi_dev(NULL, nrhs 0)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_multi_dev: NULL fleet", "adjoint_multi_dev message with nrhs 0 and bad knobs");
    EXPECT(qpdo_amd_fleet_adjoint_multi_dev(NULL, -7, v, NULL, v, v, v, NULL, NULL, NULL, NULL, NULL, 1e-9, 20, 4, 4, 0, 0, NULL) != 0, "adjoint_multi_dev(NULL, nrhs -7)");
    REFUSED_WITH("qpdo_amd_fleet_adjoint_multi_dev: NULL fleet", "adjoint_multi_dev message with a negative nrhs");

    EXPECT(qpdo_amd_fleet_tangent_dev(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 20, 0, 0, 0, 0, NULL) != 0, "tangent_dev(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_tangent_dev: NULL fleet", "tangent_dev message");
    EXPECT(qpdo_amd_fleet_tangent_dev(NULL, 2, v, v, v, v, v, v, v, act, st, v, 1e-9, 20, 4, 4, 4, 4, NULL) != 0, "tangent_dev(NULL, arrays)");
    REFUSED_WITH("qpdo_amd_fleet_tangent_dev: NULL fleet", "tangent_dev message with arrays");
    EXPECT(qpdo_amd_fleet_tangent_dev(NULL, 0, v, NULL, NULL, NULL, NULL, v, v, NULL, NULL, NULL, 0.0, -1, 4, 4, 0, 0, NULL) != 0, "tangent_dev(NULL, nrhs 0)");
    REFUSED_WITH("qpdo_amd_fleet_tangent_dev: NULL fleet", "tangent_dev message with nrhs 0 and bad knobs");

    EXPECT(qpdo_amd_fleet_rhs_group(NULL) == -1, "rhs_group(NULL)");
    EXPECT(qpdo_amd_fleet_get_sensitivity_stats(NULL, &ss) != 0 && ss.calls == -5 && ss.rhs_total == -5 && ss.scratch_bytes == -5, "get_sensitivity_stats(NULL)");
    REFUSED_WITH("qpdo_amd_fleet_get_sensitivity_stats: NULL fleet", "get_sensitivity_stats message");

    /* the struct sizes of the ABI */
    EXPECT(sizeof(QPDOAmdFleetSensitivityStats) == 3 * sizeof(long), "QPDOAmdFleetSensitivityStats: three longs");
    EXPECT(sizeof(QPDOAmdFleetAdjointStats) == 2 * sizeof(long), "QPDOAmdFleetAdjointStats keeps its size");
    EXPECT(sizeof(QPDOAmdFleetDevStats) == 5 * sizeof(long), "QPDOAmdFleetDevStats keeps its size");

    /* no new create flag: the two known ones pass the flag check (the checks behind it answer), bit 16 is refused */
    EXPECT(qpdo_amd_fleet_create_ex(0, one, &settings, QPDO_AMD_FLEET_ADJOINT | QPDO_AMD_FLEET_MATRIX_UPDATES) == NULL, "count 0 with both flags");
    REFUSED_WITH("count must be positive", "count 0 message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &settings, QPDO_AMD_FLEET_ADJOINT | 16L) == NULL, "bit 16 beside the adjoint flag");
    REFUSED_WITH("unknown flag bits", "unknown bit message");
    EXPECT(qpdo_amd_fleet_create_ex(1, one, &settings, 16L) == NULL, "bit 16 alone");
    REFUSED_WITH("unknown flag bits", "unknown bit message, alone");

    if (failures) return 1;
    printf("fleet sensitivity argument checks: all refused before any device call\n");
    return 0;
}
