/* qpdo_amd_adjoint and qpdo_amd_get_adjoint_stats (include/qpdo_amd_ext.h, qpdo_amd/csrc/qpdo_api.c) from a plain-C caller, as far as no
 * workspace is needed: every argument check that comes before the backend is touched, by message and IN THE HEADER'S ORDER -- each call
 * below carries the fault under test and every fault BEHIND it in the order, so the message shows which check came first.  Built and run by
 * tests/test_workspace_adjoint_cpu.py, also with -fsanitize=address,undefined on the host driver and on this file. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double v[4] = { 1.0, 2.0, 3.0, 4.0 }, out[4] = { 7.0, 7.0, 7.0, 7.0 };
    QPDOAmdAdjointStats as = { -5, -5, -5, -5, -5, -5.0 };

    /* 1. nrhs < 1 (with a bad tol, bad max_sweeps, NULL arrays, dQx without Q and a NULL workspace behind it) */
    EXPECT(qpdo_amd_adjoint(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 0.0, 0) != 0, "nrhs 0");
    REFUSED_WITH("qpdo_amd_adjoint: nrhs must be at least 1", "nrhs message");
    EXPECT(qpdo_amd_adjoint(NULL, -3, v, NULL, out, out, out, NULL, NULL, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "nrhs -3");
    REFUSED_WITH("nrhs must be at least 1", "negative nrhs message");
    /* 2. tol */
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 0.0, 0) != 0, "tol 0");
    REFUSED_WITH("qpdo_amd_adjoint: tol is not a positive finite number", "tol 0 message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, -1e-9, 0) != 0, "tol < 0");
    REFUSED_WITH("tol is not a positive finite number", "negative tol message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, NAN, 0) != 0, "tol NaN");
    REFUSED_WITH("tol is not a positive finite number", "NaN tol message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, INFINITY, 0) != 0, "tol inf");
    REFUSED_WITH("tol is not a positive finite number", "infinite tol message");
    /* 3. max_sweeps */
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 0) != 0, "max_sweeps 0");
    REFUSED_WITH("qpdo_amd_adjoint: max_sweeps must be at least 1", "max_sweeps message");
    /* 4. NULL gx, dq, dl, du -- in that order */
    EXPECT(qpdo_amd_adjoint(NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL gx");
    REFUSED_WITH("qpdo_amd_adjoint: gx is NULL", "gx message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, v, NULL, NULL, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL dq");
    REFUSED_WITH("qpdo_amd_adjoint: dq is NULL", "dq message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, v, NULL, out, NULL, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL dl");
    REFUSED_WITH("qpdo_amd_adjoint: dl is NULL", "dl message");
    EXPECT(qpdo_amd_adjoint(NULL, 1, v, NULL, out, out, NULL, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL du");
    REFUSED_WITH("qpdo_amd_adjoint: du is NULL", "du message");
    /* 5. dQx without Q */
    EXPECT(qpdo_amd_adjoint(NULL, 1, v, NULL, out, out, out, NULL, out, NULL, NULL, NULL, NULL, 1e-9, 20) != 0, "dQx without Q");
    REFUSED_WITH("qpdo_amd_adjoint: dQx needs Q", "dQx message");
    /* 6. NULL workspace */
    EXPECT(qpdo_amd_adjoint(NULL, 1, v, v, out, out, out, NULL, NULL, out, NULL, NULL, NULL, 1e-9, 20) != 0, "NULL workspace");
    REFUSED_WITH("qpdo_amd_adjoint: NULL workspace", "workspace message");
    EXPECT(out[0] == 7.0 && out[1] == 7.0 && out[2] == 7.0 && out[3] == 7.0, "a refused call leaves the outputs untouched");

    EXPECT(qpdo_amd_get_adjoint_stats(NULL, &as) != 0 && as.calls == -5 && as.scratch_bytes == -5 && as.last_seconds == -5.0, "get_adjoint_stats(NULL)");
    REFUSED_WITH("qpdo_amd_get_adjoint_stats: NULL workspace", "get_adjoint_stats message");

    if (failures) return 1;
    printf("workspace adjoint argument checks: all refused before any device call\n");
    return 0;
}
