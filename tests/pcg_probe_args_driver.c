/* The argument checks of the two PCG test entries (include/qpdo_amd_ext.h: qpdo_amd_pcg_probe, qpdo_amd_download_compact; made in
 * qpdo_amd/csrc/qpdo_api.c) from a plain-C caller: every call here must be refused before the library touches a device, with a message in
 * qpdo_amd_last_error().  Built and run by tests/test_pcg_checks_cpu.py, also with -fsanitize=address,undefined on the host driver and on
 * this file. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "qpdo_amd_ext.h"

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL: %s (last error: %s)\n", what, qpdo_amd_last_error()); failures++; } } while (0)
#define REFUSED_WITH(sub, what) EXPECT(strstr(qpdo_amd_last_error(), sub) != NULL, what)

int main(void) {
    double dw[2] = {1.0, 0.0}, v[2] = {1.0, 2.0}, out[2] = {7.0, 7.0}, info[QPDO_AMD_PCG_INFO_LEN];
    long long g[7];
    memset(info, 0, sizeof(info));

    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, v, out, 2, info) == -1, "mode 2"); REFUSED_WITH("mode is 0", "mode 2 message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, v, out, -1, info) == -1, "mode -1"); REFUSED_WITH("mode is 0", "mode -1 message");
    EXPECT(qpdo_amd_pcg_probe(NULL, NULL, 1.0, v, out, 0, info) == -1, "NULL dw"); REFUSED_WITH("NULL vector", "NULL dw message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, NULL, out, 0, info) == -1, "NULL v"); REFUSED_WITH("NULL vector", "NULL v message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, v, NULL, 1, info) == -1, "NULL out"); REFUSED_WITH("NULL vector", "NULL out message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, v, out, 1, NULL) == -1, "NULL info"); REFUSED_WITH("NULL vector", "NULL info message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, NAN, v, out, 1, info) == -1, "NaN sigma"); REFUSED_WITH("sigma is NaN", "NaN sigma message");
    EXPECT(qpdo_amd_pcg_probe(NULL, dw, 1.0, v, out, 0, info) == -1, "NULL workspace"); REFUSED_WITH("NULL workspace", "NULL workspace message");
    EXPECT(out[0] == 7.0 && out[1] == 7.0 && info[0] == 0.0, "a refused call writes nothing");

    EXPECT(qpdo_amd_download_compact(NULL, -1, g, 7) == -1, "which -1"); REFUSED_WITH("unknown array", "which -1 message");
    EXPECT(qpdo_amd_download_compact(NULL, 58, g, 7) == -1, "which 58"); REFUSED_WITH("unknown array", "which 58 message");
    EXPECT(qpdo_amd_download_compact(NULL, 16 + 6, g, 7) == -1, "part 6"); REFUSED_WITH("unknown array", "part 6 message");
    EXPECT(qpdo_amd_download_compact(NULL, 0, g, -7) == -1, "count < 0"); REFUSED_WITH("negative count", "count < 0 message");
    EXPECT(qpdo_amd_download_compact(NULL, 0, NULL, 7) == -1, "NULL destination"); REFUSED_WITH("NULL destination", "NULL destination message");
    EXPECT(qpdo_amd_download_compact(NULL, 48, g, 5) == -1, "NULL workspace"); REFUSED_WITH("NULL workspace", "NULL workspace message (download)");

    if (failures) return 1;
    printf("pcg probe argument checks: all refused before any device call\n");
    return 0;
}
