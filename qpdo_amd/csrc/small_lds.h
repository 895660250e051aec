/* small_lds.h -- THE plan of one workgroup's dynamic LDS in the fused small-QP kernels (qpdo_small.hip, dev/small_fleet.inc).
 *
 * The kernels carve their pointers from it, the host sizes its launches from it, and tests/small_lds_driver.c sweeps it on the CPU:
 * plain C, no HIP, no other header of the project.  All offsets are bytes from the start of the dynamic LDS (16-byte aligned).
 *
 *   [xs: n][colbuf: n][tk: 2n][the rest of the column buffers, 8n per set in all][gbuf][d_s: m][rp_s: m + 1 ints, padded to 4][U][vectors]
 *
 *   xs .. gbuf   doubles.  xs: the triangular solves' vector; with colbuf, tk and the rest: l and l*d of four columns during a
 *                factorization (8n doubles, ONE set), twice that for the factorization with look-ahead (TWO sets: small_lds_colbuf_sets).
 *   gbuf         max(n, m)/4 + 4 group sums of a 4-way grouped dot product, rounded up to an even count
 *   d_s, rp_s    the weights of the rows of A and CSR(A)'s row pointers
 *   U            ONE region shared by K -- the packed factor n (n + 1)/2 if the launch's plan found room for it, else the item's band image
 *                n (b + 1) if those of all items fit, else nothing: K in global memory -- and the linesearch scratch, which runs after the
 *                pass's solve and may overwrite K: delta (2m doubles), alpha (2m doubles), the sort's keys (64 bit) and indices (32 bit),
 *                both padded to the bitonic sort's power of two >= 2m, one flag byte per breakpoint.  The four group arrays of the
 *                linesearch's dot products (2 (m/4 + 4) + 2 (n/4 + 4) doubles) are staged there too: U is never smaller than that.
 *   vectors      a launch that has room keeps the item's work vectors behind U, at the next multiple of 16 bytes (small_lds_vec):
 *                [nv: NV_COUNT n doubles][mv: MV_COUNT m doubles][iv: 3m ints], 16 bytes of slack.
 *
 * A launch is sized for (nmax, mmax) and every workgroup carves by its own item's (n, m): the fixed part and the union size grow with n and
 * with m, so an item's regions end inside the launch's. */
#ifndef QPDO_SMALL_LDS_H
#define QPDO_SMALL_LDS_H

#include <stddef.h>

#if defined(__HIPCC__)
#define SMALL_LDS_HD __host__ __device__
#else
#define SMALL_LDS_HD
#endif
#define SMALL_LDS_FN SMALL_LDS_HD static inline __attribute__((always_inline))

/* what one workgroup may ask for: the CU's 160 KB less 1 KB for the kernels' static LDS (reduction scratch only) */
#define SMALL_LDS_BUDGET ((size_t)(160 * 1024 - 1024))

/* the item's work vectors (the solve's names; the adjoint reuses the area) */
enum { NV_X = 0, NV_XBAR, NV_QX, NV_ATY, NV_DF, NV_RD, NV_RDI, NV_RHS, NV_DX, NV_QDX, NV_ATDY, NV_D, NV_DINV, NV_T, NV_COUNT };
enum { MV_Y = 0, MV_YBAR, MV_AX, MV_MU, MV_ISQ, MV_W, MV_RP, MV_RPOLD, MV_RPI, MV_DY, MV_ADX, MV_DW, MV_E, MV_EINV, MV_ATS, MV_T, MV_DWF, MV_COUNT };

/* where K lives, one layout per launch (= QPDO_AMD_SMALL_K_*, qpdo_amd_ext.h) */
enum { K_GLOBAL = 0, K_PACKED = 1, K_BAND = 2 };

/* Sets of column buffers (8n doubles each) in front of gbuf.  Two for the factorization with look-ahead: the latency kernel (lat) on a
 * packed factor.  A band launch and a fleet whose factor is not packed have no look-ahead: one, as the batch kernel.
 * (lat, not fleet, K_GLOBAL) gives two, but no launch is made in that combination -- the host never sizes one: small_launch_sets. */
SMALL_LDS_FN int small_lds_colbuf_sets(int lat, int fleet, int layout) {
    return (lat && (fleet ? layout == K_PACKED : layout != K_BAND)) ? 2 : 1;
}

/* THE carve-up, written once, as the declarations of the regions' pointers: xs, colbuf, tk, gbuf, d_s, rp_s, Klds (the start of U),
 * ls_delta, ls_alpha, skey, sidx, jflag and ls_end (one flag byte per breakpoint, padded to 16).  dyn: the start of the dynamic LDS,
 * a double *; n, m: the item's own; sets: small_lds_colbuf_sets.  The kernels expand it in place -- statements, not a function: what the
 * compiler sees in k_small_solve (held to 128 VGPRs, with 88 vector spills) must not move -- and small_lds_layout below reads the offsets off it. */
#define SMALL_LDS_CARVE(dyn, n, m, sets) \
    double *xs = (dyn), *colbuf = (dyn) + (n), *tk = (dyn) + 2 * (size_t)(n), *gbuf = (dyn) + ((sets) == 2 ? 16 : 8) * (size_t)(n); \
    double *d_s = gbuf + (((size_t)((n) > (m) ? (n) : (m)) / 4 + 4 + 1) & ~(size_t)1); \
    int *rp_s = (int *)(d_s + (m)); \
    double *Klds = (double *)(rp_s + (((size_t)(m) + 1 + 3) & ~(size_t)3)); \
    double *ls_delta = Klds, *ls_alpha = ls_delta + 2 * (size_t)(m); \
    size_t np2s = 1; while (np2s < 2 * (size_t)(m)) np2s <<= 1;          /* the bitonic sort pads 2m to a power of two */ \
    unsigned long long *skey = (unsigned long long *)(ls_alpha + 2 * (size_t)(m)); \
    unsigned int *sidx = (unsigned int *)(skey + np2s); \
    unsigned char *jflag = (unsigned char *)(sidx + np2s), *ls_end = jflag + ((2 * (size_t)(m) + 15) & ~(size_t)15)

/* The same carve-up as byte offsets from the start of the dynamic LDS, and the sizes that go with it: what the host sizes launches from
 * and the CPU test sweeps.  (Host only: the offsets are read off a carve of a buffer that is never touched and that is long enough for
 * every n, m <= 1024 -- 204848 bytes at n = m = 1024 with two sets.) */
#define SMALL_LDS_SPAN ((size_t)256 * 1024)
typedef struct SmallLds {
    size_t xs, colbuf, tk, gbuf, d_s, rp_s, U;             /* the fixed regions; U: start of the union region = bytes of the fixed part */
    size_t ls_delta, ls_alpha, skey, sidx, jflag, ls_end;  /* the linesearch's regions inside U and their end */
    size_t gdots_bytes;                                    /* U holds at least the four dot-product group arrays */
    size_t kbytes;                                         /* the packed factor, from U */
} SmallLds;
static inline SmallLds small_lds_layout(int n, int m, int sets) {
    static double span[SMALL_LDS_SPAN / sizeof(double)];
    SMALL_LDS_CARVE(span, n, m, sets);
    const char *b = (const char *)span;
    SmallLds L;
#define SMALL_LDS_OFF(f, p) L.f = (size_t)((const char *)(p) - b)
    SMALL_LDS_OFF(xs, xs); SMALL_LDS_OFF(colbuf, colbuf); SMALL_LDS_OFF(tk, tk); SMALL_LDS_OFF(gbuf, gbuf); SMALL_LDS_OFF(d_s, d_s);
    SMALL_LDS_OFF(rp_s, rp_s); SMALL_LDS_OFF(U, Klds); SMALL_LDS_OFF(ls_delta, ls_delta); SMALL_LDS_OFF(ls_alpha, ls_alpha);
    SMALL_LDS_OFF(skey, skey); SMALL_LDS_OFF(sidx, sidx); SMALL_LDS_OFF(jflag, jflag); SMALL_LDS_OFF(ls_end, ls_end);
#undef SMALL_LDS_OFF
    L.gdots_bytes = 8 * (2 * ((size_t)m / 4 + 4) + 2 * ((size_t)n / 4 + 4));
    L.kbytes = (size_t)n * ((size_t)n + 1) / 2 * 8;
    return L;
}

/* Bytes of U for a launch whose largest item is L's (n, m).  try_packed: the packed factor goes there if fixed part + U stay inside the
 * budget (*packed_fits, optional: whether it does); otherwise the linesearch scratch alone -- a band launch widens that to its largest band
 * image itself (small_plan). */
static inline size_t small_lds_union_bytes(const SmallLds *L, int try_packed, int *packed_fits) {
    size_t ls = L->ls_end - L->U;
    if (L->gdots_bytes > ls) ls = L->gdots_bytes;
    const int ok = try_packed && (L->U + (L->kbytes > ls ? L->kbytes : ls) <= SMALL_LDS_BUDGET);
    if (packed_fits) *packed_fits = ok;
    return (ok && L->kbytes > ls) ? L->kbytes : ls;
}

/* the work vectors of an item of (n, m) behind `lds` bytes: their offset; *vbytes: their size */
SMALL_LDS_FN size_t small_lds_vec(size_t lds, int n, int m, size_t *vbytes) {
    *vbytes = ((size_t)NV_COUNT * (size_t)n + (size_t)MV_COUNT * (size_t)m) * 8 + 3 * (size_t)m * 4 + 16;
    return (lds + 15) & ~(size_t)15;
}

#endif
