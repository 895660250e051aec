/* The LDS plan of the fused small-QP kernels (qpdo_amd/csrc/small_lds.h) on the CPU: includes that header alone, links nothing.
 *
 *   small_lds_driver [n m]...
 *
 * sweeps n = 1..1024, m = 0..1024 and both column-buffer counts, checks the layout's invariants for every triple (a violation is printed
 * and counted), prints the FNV-1a checksum of (fixed bytes, union bytes, packed-fits, vector offset, vector bytes) over the sweep, and one
 * "row" line per (n, m) argument and column-buffer count.  tests/test_small_lds_cpu.py compares those with tests/golden/small_lds_table.json. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "small_lds.h"

static long bad = 0;
#define CHECK(cond) do { if (!(cond)) { if (bad++ < 20) printf("violated at n=%d m=%d sets=%d: %s\n", n, m, sets, #cond); } } while (0)

static uint64_t hash = 1469598103934665603ULL;
static void fnv(uint64_t v) { for (int b = 0; b < 8; b++) { hash ^= (v >> (8 * b)) & 0xff; hash *= 1099511628211ULL; } }

typedef struct { size_t fixed, un, fits, voff, vbytes; } Row;
static Row row_of(int n, int m, int sets) {
    Row r; int fits = 0;
    const SmallLds L = small_lds_layout(n, m, sets);
    r.fixed = L.U; r.un = small_lds_union_bytes(&L, 1, &fits); r.fits = (size_t)fits;
    r.voff = small_lds_vec(r.fixed + r.un, n, m, &r.vbytes);
    return r;
}

enum { NMAX = 1024, MMAX = 1024 };
static size_t prev_fixed[MMAX + 1][2], prev_ls[MMAX + 1][2], prev_k[MMAX + 1][2];      /* the values at n - 1 */

static void check(int n, int m, int sets) {
    const SmallLds L = small_lds_layout(n, m, sets);
    const size_t N = (size_t)n, M = (size_t)m, big = N > M ? N : M;
    size_t np2 = 1; while (np2 < 2 * M) np2 *= 2;
    /* the documented order, nothing on top of anything else */
    CHECK(L.xs == 0 && L.xs + 8 * N <= L.colbuf && L.colbuf + 8 * N <= L.tk && L.tk + 8 * 2 * N <= L.gbuf);
    CHECK(L.gbuf == 8 * (size_t)sets * 8 * N);                                /* `sets` sets of 8n doubles, xs, colbuf and tk among them */
    CHECK(L.gbuf + 8 * (big / 4 + 4) <= L.d_s);                               /* gbuf: max(n, m)/4 + 4 group sums */
    CHECK(L.d_s + 8 * M <= L.rp_s && L.rp_s + 4 * (M + 1) <= L.U);
    CHECK(L.ls_delta == L.U && L.ls_delta + 8 * 2 * M <= L.ls_alpha && L.ls_alpha + 8 * 2 * M <= L.skey);
    CHECK(L.skey + 8 * np2 <= L.sidx && L.sidx + 4 * np2 <= L.jflag && L.jflag + 2 * M <= L.ls_end);
    CHECK(L.ls_end <= SMALL_LDS_SPAN);                                        /* the buffer the offsets are read off is long enough */
    /* every region aligned to its element type (the dynamic LDS starts 16-byte aligned) */
    CHECK(L.colbuf % 8 == 0 && L.tk % 8 == 0 && L.gbuf % 8 == 0 && L.d_s % 8 == 0 && L.rp_s % 4 == 0 && L.U % 8 == 0);
    CHECK(L.ls_alpha % 8 == 0 && L.skey % 8 == 0 && L.sidx % 4 == 0);
    CHECK(L.kbytes == N * (N + 1) / 2 * 8);
    /* the linesearch's regions and the dot products' group arrays end inside U, whichever size is reported for it */
    int fits0 = -1, fits1 = -1;
    const size_t u0 = small_lds_union_bytes(&L, 0, &fits0), u1 = small_lds_union_bytes(&L, 1, &fits1);
    CHECK(fits0 == 0 && (fits1 == 0 || fits1 == 1));
    CHECK(L.ls_end <= L.U + u0 && L.gdots_bytes <= u0 && L.ls_end <= L.U + u1 && L.gdots_bytes <= u1);
    CHECK(fits1 ? (u1 >= L.kbytes && L.U + u1 <= SMALL_LDS_BUDGET) : u1 == u0);
    CHECK(fits1 || L.U + (L.kbytes > u0 ? L.kbytes : u0) > SMALL_LDS_BUDGET);
    /* the vector area: 16-byte aligned behind everything else, its three arrays end 16 bytes before the reported total */
    size_t vbytes = 0;
    const size_t voff = small_lds_vec(L.U + u1, n, m, &vbytes);
    CHECK(voff % 16 == 0 && voff >= L.U + u1 && voff < L.U + u1 + 16);
    CHECK(voff + 8 * ((size_t)NV_COUNT * N + (size_t)MV_COUNT * M) + 4 * 3 * M + 16 == voff + vbytes);
    /* an item carves by its own (n, m) inside a launch sized for (nmax, mmax): nothing may shrink as n or m grows */
    if (m > 0) CHECK(prev_fixed[m - 1][sets - 1] <= L.U && prev_ls[m - 1][sets - 1] <= u0 && prev_k[m - 1][sets - 1] <= L.kbytes);
    if (n > 1) { const SmallLds P = small_lds_layout(n - 1, m, sets); CHECK(P.U <= L.U && small_lds_union_bytes(&P, 0, NULL) <= u0 && P.kbytes <= L.kbytes); }
    prev_fixed[m][sets - 1] = L.U; prev_ls[m][sets - 1] = u0; prev_k[m][sets - 1] = L.kbytes;
}

int main(int argc, char **argv) {
    long triples = 0;
    for (int n = 1; n <= NMAX; n++) for (int m = 0; m <= MMAX; m++) for (int sets = 1; sets <= 2; sets++) {
        check(n, m, sets);
        const Row r = row_of(n, m, sets);
        fnv(r.fixed); fnv(r.un); fnv(r.fits); fnv(r.voff); fnv(r.vbytes);
        triples++;
    }
    /* the column-buffer rule: two sets only for the latency kernel on a packed factor -- and, by the kernel's expression, for the latency
     * kernel outside a fleet with K in global memory, which no launch reaches */
    for (int lat = 0; lat <= 1; lat++) for (int fleet = 0; fleet <= 1; fleet++) for (int lay = K_GLOBAL; lay <= K_BAND; lay++) {
        const int want = (lat && (lay == K_PACKED || (!fleet && lay == K_GLOBAL))) ? 2 : 1;
        if (small_lds_colbuf_sets(lat, fleet, lay) != want) { printf("violated: column-buffer sets of lat=%d fleet=%d layout=%d\n", lat, fleet, lay); bad++; }
    }
    for (int a = 1; a + 1 < argc; a += 2) for (int sets = 1; sets <= 2; sets++) {
        const int n = atoi(argv[a]), m = atoi(argv[a + 1]);
        const Row r = row_of(n, m, sets);
        printf("row %d %d %d %zu %zu %zu %zu %zu\n", n, m, sets, r.fixed, r.un, r.fits, r.voff, r.vbytes);
    }
    printf("swept %ld triples, %ld violations, fnv1a64 %016llx\n", triples, bad, (unsigned long long)hash);
    return bad ? 1 : 0;
}
