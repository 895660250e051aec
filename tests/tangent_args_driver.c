/* qpdo_amd_tangent and qpdo_amd_get_tangent_stats (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no
 * workspace is needed: every argument check that comes before the backend is touched, by message and IN THE HEADER'S ORDER -- each call
 * below carries the fault under test and every fault BEHIND it in the order, so the message shows which check came first.  Built and run by
 * tests/test_workspace_tangent_cpu.py, also with -fsanitize=address,undefined on the host driver and on this file. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double v[4] = { 1.0, 2.0, 3.0, 4.0 }, out[4] = { 7.0, 7.0, 7.0, 7.0 };
    QPDOAmdTangentStats ts = { -5, -5, -5, -5, -5, -5.0 };

    EXPECT(sizeof(QPDOAmdTangentStats) == 48 && sizeof(QPDOAmdAdjointStats) == 48, "the two stats structs are 48 bytes each");
    /* 1. nrhs < 1 (with a bad tol, bad max_sweeps, NULL outputs, no tangent and a NULL workspace behind it) */
    EXPECT(qpdo_amd_tangent(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0.0, 0) != 0, "nrhs 0");
    REFUSED_WITH("qpdo_amd_tangent: nrhs must be at least 1", "nrhs message");
    EXPECT(qpdo_amd_tangent(NULL, -3, v, NULL, NULL, NULL, NULL, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "nrhs -3");
    REFUSED_WITH("nrhs must be at least 1", "negative nrhs message");
    /* 2. tol */
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0.0, 0) != 0, "tol 0");
    REFUSED_WITH("qpdo_amd_tangent: tol is not a positive finite number", "tol 0 message");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, -1e-9, 0) != 0, "tol < 0");
    REFUSED_WITH("tol is not a positive finite number", "negative tol message");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NAN, 0) != 0, "tol NaN");
    REFUSED_WITH("tol is not a positive finite number", "NaN tol message");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, INFINITY, 0) != 0, "tol inf");
    REFUSED_WITH("tol is not a positive finite number", "infinite tol message");
    /* 3. max_sweeps */
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 0) != 0, "max_sweeps 0");
    REFUSED_WITH("qpdo_amd_tangent: max_sweeps must be at least 1", "max_sweeps message");
    /* 4. NULL dx, dy -- in that order */
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL dx");
    REFUSED_WITH("qpdo_amd_tangent: dx is NULL", "dx message");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL dy");
    REFUSED_WITH("qpdo_amd_tangent: dy is NULL", "dy message");
    /* 5. no tangent passed */
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "no tangent");
    REFUSED_WITH("qpdo_amd_tangent: no tangent passed", "no tangent message");
    /* 6. tQx without Q */
    EXPECT(qpdo_amd_tangent(NULL, 1, v, NULL, NULL, NULL, v, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "tQx without Q");
    REFUSED_WITH("qpdo_amd_tangent: tQx needs Q", "tQx message");
    /* 7. NULL workspace: with each of the five arrays alone */
    EXPECT(qpdo_amd_tangent(NULL, 1, v, NULL, NULL, NULL, NULL, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL workspace, tq");
    REFUSED_WITH("qpdo_amd_tangent: NULL workspace", "workspace message (tq)");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, v, NULL, NULL, NULL, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL workspace, tl");
    REFUSED_WITH("qpdo_amd_tangent: NULL workspace", "workspace message (tl)");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, v, NULL, NULL, NULL, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL workspace, tu");
    REFUSED_WITH("qpdo_amd_tangent: NULL workspace", "workspace message (tu)");
    EXPECT(qpdo_amd_tangent(NULL, 1, NULL, NULL, NULL, NULL, NULL, v, out, out, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL workspace, tAx");
    REFUSED_WITH("qpdo_amd_tangent: NULL workspace", "workspace message (tAx)");
    EXPECT(out[0] == 7.0 && out[1] == 7.0 && out[2] == 7.0 && out[3] == 7.0, "a refused call leaves the outputs untouched");

    EXPECT(qpdo_amd_get_tangent_stats(NULL, &ts) != 0 && ts.calls == -5 && ts.scratch_bytes == -5 && ts.last_seconds == -5.0, "get_tangent_stats(NULL)");
    REFUSED_WITH("qpdo_amd_get_tangent_stats: NULL workspace", "get_tangent_stats message");

    if (failures) return 1;
    printf("workspace tangent argument checks: all refused before any device call\n");
    return 0;
}
