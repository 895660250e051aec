// band.inc -- part of qpdo_dev.hip (one translation unit; included in order): a BAND direct solver for Newton matrices that are banded.
// ------------------------------------------------------------------------------------------------
// The reference hands K = Q + sigma I + A'DA to CHOLMOD in NATURAL order (cholmod_interface.c:35-52,107-123): on a chain-structured QP
// (MPC, splines, trajectories) K is banded and the sparse factorization costs O(n b^2) -- which is why the reference solves such problems
// trivially at any n.  Here K with half-bandwidth b <= 127 (b = max over the rows of A of their column span, and of Q's bandwidth: the
// pattern of A'DA lies inside it for every D) gets the same treatment: lower band storage (b + 1 doubles per column), a natural-order
// LDL' that never leaves the band (no pivoting, no fill outside it), band triangular solves.  One workgroup sweeps the columns; the part
// of the matrix a step touches -- b + 4 columns -- lives in a ring in LDS, columns stream in from and out to HBM once.
// Storage: Kb[j * (b+1) + t] = K(j + t, j), 0 <= t <= b (zero beyond the matrix).  After the factorization the same array holds D on the
// diagonal slots and the unit-lower L below; Lt[i * (b+1) + t] = L(i, i - t) is the row-band copy the backward solve streams.
// ------------------------------------------------------------------------------------------------
static const int BAND_MAX_B = 127;

// half-bandwidth: rows of A are column-sorted (span = last - first column); Q is scanned entry by entry
__global__ void k_band_span_A(int m, const int *__restrict__ rp, const int *__restrict__ ci, int *__restrict__ out) {
    int mx = 0;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) {
        const int b = rp[r], e = rp[r + 1];
        if (e > b) { const int s = ci[e - 1] - ci[b]; mx = s > mx ? s : mx; }
    }
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_down(mx, o, 64); mx = t > mx ? t : mx; }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(out, mx);
}
__global__ void k_band_span_Q(int n, const int *__restrict__ rp, const int *__restrict__ ci, int *__restrict__ out) {
    int mx = 0;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
        for (int k = rp[r]; k < rp[r + 1]; k++) { const int s = ci[k] > r ? ci[k] - r : r - ci[k]; mx = s > mx ? s : mx; }
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_down(mx, o, 64); mx = t > mx ? t : mx; }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(out, mx);
}
// assembly: one wave per column j, accumulator of b + 1 doubles in LDS; Q first, then the weighted rows of A that touch column j in
// ascending order, sigma_f last -- the per-element order of k_dense_assemble, so the band holds the very values the dense matrix would.
// Columns n .. np-1 (np = n rounded up to 4) are identity padding: the factorization takes four columns per step.
// PERM (a variable order of the band solver, dev/host_band.inc): the wave of column pj assembles the caller's column j = newold[pj], and an
// entry with the caller's row i lands at oldnew[i] - pj when that is in 0 .. b -- the band of P K P', each element summed in the order
// above, so it holds the very bits the natural-order band of K holds for the same entries.  PERM = false is the code without an order.
template <bool PERM>
__device__ __forceinline__ void band_assemble_body(int n, int np, int b, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                   const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                   const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                   const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                   double *__restrict__ Kb, const int *__restrict__ newold, const int *__restrict__ oldnew,
                                                   double (*acc_s)[128]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, B1 = b + 1;
    double *acc = acc_s[wave];
    for (int pj = blockIdx.x * 4 + wave; pj < np; pj += gridDim.x * 4) {
        double *col = Kb + (size_t)pj * B1;
        if (pj >= n) { for (int t = lane; t <= b; t += 64) col[t] = (t == 0) ? 1.0 : 0.0; continue; }
        const int j = PERM ? newold[pj] : pj;
        acc[lane] = 0.0; acc[lane + 64] = 0.0;
        __builtin_amdgcn_wave_barrier();
        for (int k = qrp[j] + lane; k < qrp[j + 1]; k += 64) { const int c = PERM ? oldnew[qci[k]] : qci[k]; if (c >= pj && c - pj <= b) acc[c - pj] += qval[k]; }
        __builtin_amdgcn_wave_barrier();
        for (int t = trp[j]; t < trp[j + 1]; t++) {                   // (uniform over the wave)
            const int r = tci[t];
            const double wgt = dw[r];
            if (wgt == 0.0) continue;
            const double vj = wgt * tval[t];
            for (int e = arp[r] + lane; e < arp[r + 1]; e += 64) { const int i = PERM ? oldnew[aci[e]] : aci[e]; if (i >= pj && i - pj <= b) acc[i - pj] += vj * aval[e]; }
            __builtin_amdgcn_wave_barrier();                          // one wave: its LDS operations are served in order
        }
        if (lane == 0) acc[0] += sigma_f;
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t <= b; t += 64) col[t] = (pj + t < n) ? acc[t] : 0.0;
        __builtin_amdgcn_wave_barrier();
    }
}
__global__ __launch_bounds__(256) void k_band_assemble(int n, int np, int b, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                      const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                      const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                      const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                      double *__restrict__ Kb) {
    __shared__ double acc_s[4][128];
    band_assemble_body<false>(n, np, b, qrp, qci, qval, trp, tci, tval, arp, aci, aval, dw, sigma_f, Kb, nullptr, nullptr, acc_s);
}
__global__ __launch_bounds__(256) void k_band_assemble_perm(int n, int np, int b, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                           const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                           const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                           const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                           double *__restrict__ Kb, const int *__restrict__ newold, const int *__restrict__ oldnew) {
    __shared__ double acc_s[4][128];
    band_assemble_body<true>(n, np, b, qrp, qci, qval, trp, tci, tval, arp, aci, aval, dw, sigma_f, Kb, newold, oldnew, acc_s);
}
// natural-order LDL' inside the band, four columns per step (the leading 4 x 4 block is factored redundantly by every thread, the panel
// rows and the trailing window are updated in parallel: the scheme of the fused small-problem kernel, on a window that slides).  The ring
// holds columns k .. k + b + 3; K(i, j) sits at ring[(j mod RC) * B1 + (i - j)].  Requires b >= 3 and np a multiple of 4 (host).
// Workgroup barrier for LDS traffic ONLY.  __syncthreads() waits for every outstanding vector-memory operation of the wave first
// (s_waitcnt vmcnt(0)): in these two kernels that is an HBM round trip per step -- the loads a step issues for LATER steps and the
// stores of finished columns are all still in flight at its barriers, and waiting for them there is what made every prefetch scheme
// measure the same.  The data the barriers order lives in LDS (lgkmcnt); registers filled by global loads are waited for by the
// compiler where they are used.
#define BAND_SYNC() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// 1/d: hardware reciprocal + two Newton steps (accurate to an ulp or two for the pivots of a scaled SPD matrix, NOT the correctly rounded
// IEEE quotient: the band factor agrees with the dense path's within rounding, not bit for bit; the IEEE division sequence is ~250
// dependent cycles and four of them in a row are most of a narrow band's step)
__device__ __forceinline__ double band_recip(double d) {
    double inv = __builtin_amdgcn_rcp(d);
    inv = fma(fma(-d, inv, 1.0), inv, inv);
    inv = fma(fma(-d, inv, 1.0), inv, inv);
    return inv;
}
// BAND_NT threads, half-bandwidth up to BMAX (instantiated <256, 127>).
template <int BAND_NT, int BMAX>
__global__ __launch_bounds__(BAND_NT) void k_band_factor(int np, int b, double *__restrict__ Kb, double *__restrict__ Lt, int *__restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double band_lds[];
    const int B1 = b + 1, RC = b + 4, FW = b + 4;
    double *ring = band_lds;
    double *F = ring + (size_t)RC * B1;
    double *L0 = F, *L1 = F + FW, *L2 = F + 2 * FW, *L3 = F + 3 * FW, *T0 = F + 4 * FW, *T1 = F + 5 * FW, *T2 = F + 6 * FW, *T3 = F + 7 * FW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = BAND_NT / 64;
    for (int e = tid; e < RC * B1; e += BAND_NT) { const int c = e / B1, t = e - c * B1; ring[e] = (c < np) ? Kb[(size_t)c * B1 + t] : 0.0; }
    // this thread's share of a group of four columns (streamed in and out once per step): column-in-group and band offset, fixed for the
    // whole sweep -- no integer division inside the loop (one runtime division is ~40 instructions; the first version of this kernel
    // spent most of a narrow band's step on them, and on the modulo of the ring addressing: 3100 cycles per step at b = 3)
    constexpr int PFN = (4 * (BMAX + 1) + BAND_NT - 1) / BAND_NT;
    int g_cl[PFN], g_t[PFN];
#pragma unroll
    for (int u = 0; u < PFN; u++) { const int e = tid + u * BAND_NT; g_cl[u] = e < 4 * B1 ? e / B1 : -1; g_t[u] = e < 4 * B1 ? e - g_cl[u] * B1 : 0; }
    // The four columns that enter the window at the end of step s are loaded PFD steps ahead into a register queue: a narrow band's step is
    // a few hundred cycles of arithmetic, an HBM round trip a few thousand.
    constexpr int PFD = 3;
    double pfq[PFD + 1][PFN];
    auto issue = [&](int kk, double *dst) {
#pragma unroll
        for (int u = 0; u < PFN; u++) {
            dst[u] = 0.0;
            if (g_cl[u] >= 0) { const int c = kk + RC + g_cl[u]; if (c < np) dst[u] = Kb[(size_t)c * B1 + g_t[u]]; }
        }
    };
#pragma unroll
    for (int q = 0; q < PFD; q++) issue(4 * q, pfq[q]);
    BAND_SYNC();
    int sk = 0;                                       // slot of column k in the ring (k mod RC, kept incrementally)
    // K is symmetric positive definite whenever the reference's factorization exists; a pivot that is not a positive finite number
    // (settings->proximal = 0 on a Q + A'DA that is singular along a direction, or a NaN in the data) is latched for the host, which
    // redoes the pass with another solver instead of walking on with inf / NaN in dx (the reciprocals below have no check of their own)
    bool bad_pivot = false;
    // One step; pf_out: the register set whose columns enter the ring at the end of this step (loaded PFD steps ago), pf_in: the set this
    // step's loads go to.  The sets are addressed STATICALLY (the outer loop below is unrolled over them): rotating a queue with register
    // moves would read the destinations of loads still in flight and make every step wait for them (s_waitcnt vmcnt(0) at the loop head).
    auto step = [&](const int k, double *pf_out, double *pf_in) {
        issue(k + 4 * PFD, pf_in);
        // pc[u][o] = K(k + o, k + u): column k + u of the ring, addressed by the row offset from k
        double *pc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { int sl = sk + u; if (sl >= RC) sl -= RC; pc[u] = ring + (size_t)sl * B1 - u; }
        const double d0 = pc[0][0], inv0 = band_recip(d0);
        const double l10 = pc[0][1] * inv0, l20 = pc[0][2] * inv0, l30 = pc[0][3] * inv0;
        const double t10 = l10 * d0, t20 = l20 * d0, t30 = l30 * d0;
        const double d1 = pc[1][1] - l10 * t10, inv1 = band_recip(d1);
        const double l21 = (pc[1][2] - l20 * t10) * inv1, l31 = (pc[1][3] - l30 * t10) * inv1;
        const double t21 = l21 * d1, t31 = l31 * d1;
        const double d2 = (pc[2][2] - l20 * t20) - l21 * t21, inv2 = band_recip(d2);
        const double l32 = ((pc[2][3] - l30 * t20) - l31 * t21) * inv2, t32 = l32 * d2;
        const double d3 = ((pc[3][3] - l30 * t30) - l31 * t31) - l32 * t32;
        const double inv3 = band_recip(d3);
        bad_pivot = bad_pivot || !(d0 > 0.0 && d0 < 1e300) || !(d1 > 0.0 && d1 < 1e300) || !(d2 > 0.0 && d2 < 1e300) || !(d3 > 0.0 && d3 < 1e300);
        const int olast = (k + 3 + b < np - 1) ? 3 + b : np - 1 - k;          // offset of the last row the four pivot columns reach
        for (int o = 4 + tid; o <= olast; o += BAND_NT) {
            const double r0 = pc[0][o <= b ? o : b], r1 = pc[1][o - 1 <= b ? o : b + 1], r2 = pc[2][o - 2 <= b ? o : b + 2], a3 = pc[3][o];
            const double a0 = (o <= b) ? r0 : 0.0, a1 = (o - 1 <= b) ? r1 : 0.0, a2 = (o - 2 <= b) ? r2 : 0.0;
            const double l0 = a0 * inv0;
            const double v1 = a1 - l0 * t10;
            const double l1 = v1 * inv1;
            const double v2 = (a2 - l0 * t20) - l1 * t21;
            const double l2 = v2 * inv2;
            const double v3 = ((a3 - l0 * t30) - l1 * t31) - l2 * t32;
            const double l3 = v3 * inv3;
            if (o <= b) pc[0][o] = l0;
            if (o - 1 <= b) pc[1][o] = l1;
            if (o - 2 <= b) pc[2][o] = l2;
            pc[3][o] = l3;
            L0[o] = l0; L1[o] = l1; L2[o] = l2; L3[o] = l3;
            T0[o] = l0 * d0; T1[o] = l1 * d1; T2[o] = l2 * d2; T3[o] = l3 * d3;
        }
        BAND_SYNC();
        if (tid == 0) {                                // (inputs of every thread above: overwritten after the barrier)
            pc[0][1] = l10; pc[0][2] = l20; pc[0][3] = l30;
            pc[1][1] = d1;  pc[1][2] = l21; pc[1][3] = l31;
            pc[2][2] = d2;  pc[2][3] = l32; pc[3][3] = d3;
        }
        // trailing window: columns at offsets oj = 4 .. olast, rows oj .. olast (rows beyond see no pivot column of this step)
        for (int oj = 4 + wave; oj <= olast; oj += nw) {
            const double t0 = T0[oj], t1 = T1[oj], t2 = T2[oj], t3 = T3[oj];
            int sl = sk + oj; if (sl >= RC) sl -= RC;
            double *colp = ring + (size_t)sl * B1 - oj;
            for (int oi = oj + lane; oi <= olast; oi += 64) {
                double w = colp[oi] - L0[oi] * t0;
                w = w - L1[oi] * t1;
                w = w - L2[oi] * t2;
                colp[oi] = w - L3[oi] * t3;
            }
        }
        BAND_SYNC();
        // the four finished columns leave (L below the diagonal, D on it; row-band copy for the backward solve), the queued ones enter
#pragma unroll
        for (int u = 0; u < PFN; u++) {
            if (g_cl[u] >= 0) {
                const int cl = g_cl[u], t = g_t[u], c = k + cl;
                int sl = sk + cl; if (sl >= RC) sl -= RC;
                double *slot = ring + (size_t)sl * B1 + t;
                const double v = *slot;
                Kb[(size_t)c * B1 + t] = v;
                if (t > 0 && c + t < np) Lt[(size_t)(c + t) * B1 + t] = v;
                *slot = pf_out[u];
            }
        }
        sk += 4; if (sk >= RC) sk -= RC;
        BAND_SYNC();
    };
    static_assert(PFD == 3, "the unrolled schedule below assumes a queue of four register sets");
    for (int k = 0; k < np; k += 16) {
        step(k, pfq[0], pfq[3]);
        if (k + 4 < np) step(k + 4, pfq[1], pfq[0]);
        if (k + 8 < np) step(k + 8, pfq[2], pfq[1]);
        if (k + 12 < np) step(k + 12, pfq[3], pfq[2]);
    }
    if (bad_pivot && tid == 0) atomicOr(err, 2);       // (C_CHAIN_ERR, bit 1: the device skips this pass's iterate update, the host reads the latch with the step)
}
// Both triangular solves and the diagonal scaling.  The recurrence x_j -> x_{j+1} is sequential: ONE wave carries it -- lane l keeps the rows of
// the sliding window that are congruent to l (three per lane: b <= 127), x_j is broadcast with v_readlane -- at ~50 cycles per column, which
// only works if no step waits for memory: the three other waves of the workgroup stream the band (Lb forward, the row-band copy Lt
// backward) into a four-deep LDS ring of 32-column chunks two chunks ahead of the compute wave, one workgroup barrier per chunk.  (A first
// version had the compute wave load its own multipliers eight steps ahead: 410 cycles per column, an HBM round trip per group.)
#define BAND_SC 32
__device__ __forceinline__ double band_rl64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
// (the body of k_band_solve; k_band_solve_multi runs it once per workgroup on a column of its own)
// PERM (a variable order, see band_assemble_body): rhs and x are in the caller's order -- entry i of the solver's order is read from
// rhs[perm[i]] and delivered to x[perm[i]], perm = newold; the gather and the scatter ARE the sweep's first loads and last stores, no
// launch and no vector of their own.  z stays in the solver's order.  PERM = false is the code without an order.
template <bool PERM>
__device__ __forceinline__ void band_solve_body(int n, int b, const double *__restrict__ Lb, const double *__restrict__ Lt, const double *__restrict__ rhs,
                                                double *__restrict__ z, double *__restrict__ x, const int *__restrict__ perm) {
    extern __shared__ __attribute__((aligned(16))) double band_sbuf[];       // 4 x (BAND_SC * B1)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, B1 = b + 1, CH = BAND_SC * B1;
    const int nchunks = (n + BAND_SC - 1) / BAND_SC;
    const long long total = (long long)n * B1;
    auto ld = [&](const double *v, int i) { return (i >= 0 && i < n) ? v[i] : 0.0; };
    auto ld_rhs = [&](int i) { return (i >= 0 && i < n) ? rhs[PERM ? perm[i] : i] : 0.0; };
    auto copy_chunk = [&](const double *src, int c, int t0, int nt) {          // columns c*SC .. c*SC + SC - 1 of the band: CH contiguous doubles
        if (c < 0 || c >= nchunks) return;
        double *dst = band_sbuf + (size_t)(c & 3) * CH;
        const long long base = (long long)c * CH;
        for (int e = t0; e < CH; e += nt) dst[e] = (base + e < total) ? src[base + e] : 0.0;
    };
    // the loader waves' pipeline: a chunk is LOADED (global -> registers) in one iteration and STORED (registers -> ring) in the next, so that
    // the barrier that ends an iteration never waits for an HBM round trip
    constexpr int LRN = (BAND_SC * (BAND_MAX_B + 1) + 191) / 192;
    double lr[LRN];
    auto chunk_load = [&](const double *src, int c) {
        const long long base = (long long)c * CH;
#pragma unroll
        for (int u = 0; u < LRN; u++) { const int e = tid - 64 + u * 192; lr[u] = (c >= 0 && c < nchunks && e < CH && base + e < total) ? src[base + e] : 0.0; }
    };
    auto chunk_store = [&](int c) {
        if (c < 0 || c >= nchunks) return;
        double *dst = band_sbuf + (size_t)(c & 3) * CH;
#pragma unroll
        for (int u = 0; u < LRN; u++) { const int e = tid - 64 + u * 192; if (e < CH) dst[e] = lr[u]; }
    };
    constexpr int STEPS = 8;
    // ---- L z = rhs, z /= D -------------------------------------------------------------------------------------------------------
    copy_chunk(Lb, 0, tid, 256); copy_chunk(Lb, 1, tid, 256);
    if (wave != 0) chunk_load(Lb, 2);
    BAND_SYNC();
    double s0 = ld_rhs(lane), s1 = ld_rhs(64 + lane), s2 = ld_rhs(128 + lane);
    for (int g = 0; g < nchunks; g++) {
        if (wave != 0) { chunk_store(g + 2); chunk_load(Lb, g + 3); }
        else {
            const int jb = (g >> 1) * 64, jl0 = (g & 1) * BAND_SC;
            const double *buf = band_sbuf + (size_t)(g & 3) * CH;
            for (int q = 0; q < BAND_SC; q += STEPS) {
                double c0[STEPS], c1[STEPS], c2[STEPS];
#pragma unroll
                for (int u = 0; u < STEPS; u++) {
                    const int jl = jl0 + q + u;
                    const double *col = buf + (size_t)(q + u) * B1;
                    const int o0 = lane - jl, o1 = o0 + 64, o2 = o0 + 128;
                    c0[u] = (o0 > 0 && o0 <= b) ? col[o0] : 0.0; c1[u] = (o1 <= b) ? col[o1] : 0.0; c2[u] = (o2 <= b) ? col[o2] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < STEPS; u++) {                  // (columns past the matrix are zeros in the ring: no effect)
                    const double xj = band_rl64(s0, jl0 + q + u);
                    s0 = s0 - c0[u] * xj; s1 = s1 - c1[u] * xj; s2 = s2 - c2[u] * xj;
                }
            }
            if ((g & 1) == 1 || g == nchunks - 1) {               // rows jb .. jb + 63 are final: divide by D (the t = 0 entries of their columns)
                const int gc = (lane < BAND_SC) ? (jb / BAND_SC) : (jb / BAND_SC + 1);
                const double dd = (jb + lane < n) ? band_sbuf[(size_t)(gc & 3) * CH + (size_t)(lane & (BAND_SC - 1)) * B1] : 1.0;
                if (jb + lane < n) z[jb + lane] = s0 / dd;
                s0 = s1; s1 = s2; s2 = ld_rhs(jb + 192 + lane);
            }
        }
        BAND_SYNC();
    }
    __threadfence_block();
    // ---- L' x = z, columns descending: row j of L (the row-band copy Lt) holds the multipliers of the rows above it -----------------
    copy_chunk(Lt, nchunks - 1, tid, 256); copy_chunk(Lt, nchunks - 2, tid, 256);
    if (wave != 0) chunk_load(Lt, nchunks - 3);
    BAND_SYNC();
    const int jb_last = ((nchunks - 1) >> 1) * 64;
    s0 = ld(z, jb_last + lane); s1 = ld(z, jb_last - 64 + lane); s2 = ld(z, jb_last - 128 + lane);
    for (int g = nchunks - 1; g >= 0; g--) {
        if (wave != 0) { chunk_store(g - 2); chunk_load(Lt, g - 3); }
        else {
            const int jb = (g >> 1) * 64, jl0 = (g & 1) * BAND_SC;
            const double *buf = band_sbuf + (size_t)(g & 3) * CH;
            for (int q = BAND_SC - 1; q >= 0; q -= STEPS) {
                double c0[STEPS], c1[STEPS], c2[STEPS];
#pragma unroll
                for (int u = 0; u < STEPS; u++) {
                    const int jl = jl0 + q - u;
                    const double *row = buf + (size_t)(q - u) * B1;
                    const int o0 = jl - lane, o1 = o0 + 64, o2 = o0 + 128;
                    c0[u] = (o0 > 0 && o0 <= b) ? row[o0] : 0.0; c1[u] = (o1 <= b) ? row[o1] : 0.0; c2[u] = (o2 <= b) ? row[o2] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < STEPS; u++) {
                    const double xj = band_rl64(s0, jl0 + q - u);
                    s0 = s0 - c0[u] * xj; s1 = s1 - c1[u] * xj; s2 = s2 - c2[u] * xj;
                }
            }
            if ((g & 1) == 0) {                                    // rows jb .. jb + 63 are final
                if (jb + lane < n) x[PERM ? perm[jb + lane] : jb + lane] = s0;
                s0 = s1; s1 = s2; s2 = ld(z, jb - 192 + lane);
            }
        }
        BAND_SYNC();
    }
}
__global__ __launch_bounds__(256) void k_band_solve(int n, int b, const double *__restrict__ Lb, const double *__restrict__ Lt,
                                                    const double *__restrict__ rhs, double *__restrict__ z, double *__restrict__ x) {
    band_solve_body<false>(n, b, Lb, Lt, rhs, z, x, nullptr);
}
__global__ __launch_bounds__(256) void k_band_solve_perm(int n, int b, const double *__restrict__ Lb, const double *__restrict__ Lt,
                                                         const double *__restrict__ rhs, double *__restrict__ z, double *__restrict__ x,
                                                         const int *__restrict__ perm) {
    band_solve_body<true>(n, b, Lb, Lt, rhs, z, x, perm);
}
// the group path's solve (dev/adjoint.inc adj_sweeps_group): one workgroup per live right-hand side, each running k_band_solve's two sweeps
// on columns of its own (rhs and x: ldx apart, z: np apart) -- the columns advance together on different CUs for the time of one solve
__global__ __launch_bounds__(256) void k_band_solve_group(int n, int np, int b, const double *__restrict__ Lb, const double *__restrict__ Lt,
                                                          const double *rhs, long long ldx, double *z, double *x) {
    const long long s = blockIdx.x;
    band_solve_body<false>(n, b, Lb, Lt, rhs + s * ldx, z + s * np, x + s * ldx, nullptr);
}
__global__ __launch_bounds__(256) void k_band_solve_group_perm(int n, int np, int b, const double *__restrict__ Lb, const double *__restrict__ Lt,
                                                               const double *rhs, long long ldx, double *z, double *x, const int *__restrict__ perm) {
    const long long s = blockIdx.x;
    band_solve_body<true>(n, b, Lb, Lt, rhs + s * ldx, z + s * np, x + s * ldx, perm);
}

// ---- chain QPs with a few dense coupling rows (QPDO_BAND_COUPLING; host side: dev/host_band.inc) ------------------------------------------
// A row of A that touches the whole horizon (a budget, a terminal average, a conservation equality) makes A'DA a full matrix, but K is
// still band plus low rank: K = B + U W U', B = Q + sigma I + A_b' D_b A_b over the remaining rows, the columns of U = the coupling rows
// with a nonzero weight, W = their weights.  B gets the band factorization above; the solve is Woodbury's,
//   x = z0 - Z S^-1 (U' z0),   z0 = B^-1 v,   Z = B^-1 U,   S = W^-1 + U' Z  (k x k, symmetric positive definite),
// inside the residual-checked refinement of the low-rank path (host_dense.inc dense_refine_checked).  The coupling rows keep fixed slots
// 0 .. r-1 (ascending row number); a 64-bit mask names the slots a launch works on, in ascending order.
static const int BC_MAX = 64;               // coupling rows a workspace accepts (one bit of the slot masks each)
__device__ __forceinline__ int bc_nth_slot(u64 mask, int j) {                 // the j-th set bit of mask
    for (int i = 0; i < j; i++) mask &= mask - 1;
    return __ffsll((unsigned long long)mask) - 1;
}
// One pass over the row pointers: the rows whose column span exceeds BAND_MAX_B are counted and listed in ascending order (the first cap
// of them), out = {their count, the largest span of the other rows, the largest span of all rows}.  One workgroup, contiguous chunk of
// rows per thread, k_wb_select's scheme: plain stores in a fixed order.
__global__ __launch_bounds__(1024) void k_bc_classify(int m, const int *__restrict__ rp, const int *__restrict__ ci, int cap, int *__restrict__ rows,
                                                      int *__restrict__ out) {
    __shared__ int sums[1024], mxc[1024], mxa[1024];
    const int chunk = (m + 1023) / 1024;
    const int beg = min(threadIdx.x * chunk, m), end = min(beg + chunk, m);
    int c = 0, core = 0, all = 0;
    for (int i = beg; i < end; i++) {
        const int s = rp[i + 1] > rp[i] ? ci[rp[i + 1] - 1] - ci[rp[i]] : 0;
        all = s > all ? s : all;
        if (s > BAND_MAX_B) c++; else core = s > core ? s : core;
    }
    sums[threadIdx.x] = c; mxc[threadIdx.x] = core; mxa[threadIdx.x] = all;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0, a = 0, b = 0;
        for (int i = 0; i < 1024; i++) { const int t = sums[i]; sums[i] = run; run += t; a = mxc[i] > a ? mxc[i] : a; b = mxa[i] > b ? mxa[i] : b; }
        out[0] = run; out[1] = a; out[2] = b;
    }
    __syncthreads();
    int pos = sums[threadIdx.x];
    for (int i = beg; i < end; i++)
        if (rp[i + 1] > rp[i] && ci[rp[i + 1] - 1] - ci[rp[i]] > BAND_MAX_B) { if (pos < cap) rows[pos] = i; pos++; }
}
// core weights: d with the coupling rows zeroed (k_band_assemble skips zero-weight rows, so B is assembled from the other rows alone);
// info[0] |= 1 where they differ from the weights of the kept band factor, info[1] = k, the number of coupling rows with a nonzero
// weight, info[2], info[3] = their slots as a 64-bit mask.  info[0] is zeroed by the host before the launch.
__global__ void k_bc_prepare(int m, int r, const int *__restrict__ rows, const double *__restrict__ dw, double *__restrict__ dcore,
                             const double *__restrict__ dfact, int *__restrict__ info) {
    __shared__ int rs[BC_MAX];
    for (int a = threadIdx.x; a < r; a += blockDim.x) rs[a] = rows[a];
    __syncthreads();
    int moved = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        int lo = 0, hi = r;                                                   // (rs ascending)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (rs[mid] < i) lo = mid + 1; else hi = mid; }
        const double dc = (lo < r && rs[lo] == i) ? 0.0 : dw[i];
        dcore[i] = dc;
        moved |= dc != dfact[i];
    }
    if (__any(moved) && (threadIdx.x & 63) == 0) atomicOr(&info[0], 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        u64 act = 0; int k = 0;
        for (int a = 0; a < r; a++) if (dw[rs[a]] != 0.0) { act |= 1ull << a; k++; }
        info[1] = k; info[2] = (int)(u32)act; info[3] = (int)(u32)(act >> 32);
    }
}
// Z(:, s) = B^-1 (coupling row s as a dense column) for the slots s of `todo`: one workgroup per slot, each running k_band_solve's two
// sweeps on columns of its own (U: the right-hand side, T: the forward sweep's result; np entries each) -- the columns advance together on
// different CUs for the time of one solve.
__global__ __launch_bounds__(256) void k_band_solve_multi(int n, int np, int b, const double *__restrict__ Lb, const double *__restrict__ Lt, u64 todo,
                                                          const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                                          const double *__restrict__ aval, double *U, double *T, double *Z) {
    const int s = bc_nth_slot(todo, blockIdx.x), row = rows[s];
    double *u = U + (size_t)s * np;
    for (int i = threadIdx.x; i < np; i += 256) u[i] = 0.0;
    __syncthreads();
    for (int e = arp[row] + threadIdx.x; e < arp[row + 1]; e += 256) u[aci[e]] = aval[e];
    __syncthreads();
    band_solve_body<false>(n, b, Lb, Lt, u, T + (size_t)s * np, Z + (size_t)s * np, nullptr);
}
// S(a, c) = [a == c] / d_a + A(row_a, :) Z(:, slot_c) over the active slots, a <= c and its mirror image (k_wb_G's scheme; leading
// dimension BC_MAX)
__global__ __launch_bounds__(64) void k_bc_S(u64 act, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                             const double *__restrict__ aval, const double *__restrict__ dw, const double *__restrict__ Z, int np,
                                             double *__restrict__ S) {
    const int a = blockIdx.x, c = blockIdx.y;
    if (a > c) return;
    const int r = rows[bc_nth_slot(act, a)];
    const double *zc = Z + (size_t)bc_nth_slot(act, c) * np;
    double sacc = 0.0;
    for (int e = arp[r] + threadIdx.x; e < arp[r + 1]; e += 64) sacc += aval[e] * zc[aci[e]];
    sacc = wave_sum(sacc);
    if (threadIdx.x == 0) {
        if (a == c) sacc = 1.0 / dw[r] + sacc;
        S[a * BC_MAX + c] = sacc; S[c * BC_MAX + a] = sacc;
    }
}
// S = L D L' in one workgroup's LDS, no pivoting (S is symmetric positive definite); SL: L below the diagonal, D on it.  A pivot that is
// not a positive finite number is latched like one of the band factorization (bit 1 of C_CHAIN_ERR).
__global__ __launch_bounds__(256) void k_bc_factor_S(int k, const double *__restrict__ S, double *__restrict__ SL, int *__restrict__ err) {
    __shared__ double M[BC_MAX * BC_MAX];
    const int tid = threadIdx.x;
    for (int e = tid; e < k * k; e += 256) { const int i = e / k, j = e - i * k; M[i * BC_MAX + j] = S[i * BC_MAX + j]; }
    __syncthreads();
    bool bad_pivot = false;
    for (int j = 0; j < k; j++) {
        const double dj = M[j * BC_MAX + j];
        bad_pivot = bad_pivot || !(dj > 0.0 && dj < 1e300);
        // column j: the multipliers below the diagonal, their products with d_j in row j above it (scratch: the upper triangle)
        for (int i = j + 1 + tid; i < k; i += 256) { const double w = M[i * BC_MAX + j]; M[j * BC_MAX + i] = w; M[i * BC_MAX + j] = w / dj; }
        __syncthreads();
        const int nn = k - j - 1;
        for (int e = tid; e < nn * nn; e += 256) {
            const int i = j + 1 + e / nn, c = j + 1 + e % nn;
            if (c <= i) M[i * BC_MAX + c] = M[i * BC_MAX + c] - M[i * BC_MAX + j] * M[j * BC_MAX + c];
        }
        __syncthreads();
    }
    for (int e = tid; e < k * k; e += 256) { const int i = e / k, j = e - i * k; if (j <= i) SL[i * BC_MAX + j] = M[i * BC_MAX + j]; }
    if (bad_pivot && tid == 0) atomicOr(err, 2);
}
// t = (L D L')^-1 v for the k x k factor in M (leading dimension BC_MAX; L below the diagonal, D on it), by the workgroup's first wave: lane
// a keeps entry a, the pivot entry is broadcast with v_readlane.  (Behind the barrier that publishes M and v.)
__device__ __forceinline__ void bc_tri_solve(int k, const double *M, const double *v, double *__restrict__ t) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave != 0) return;
    const bool in = lane < k;
    double val = in ? v[lane] : 0.0;
    for (int j = 0; j < k; j++) {
        const double vj = band_rl64(val, j);
        if (in && lane > j) val = val - M[lane * BC_MAX + j] * vj;
    }
    if (in) val = val / M[lane * BC_MAX + lane];
    for (int j = k - 1; j > 0; j--) {
        const double xj = band_rl64(val, j);
        if (lane < j) val = val - M[j * BC_MAX + lane] * xj;
    }
    if (in) t[lane] = val;
}
// t = S^-1 (U' z0): the k dot products A(row_a, :) z0, one wave each in turn, then both triangular solves by one wave (lane a keeps
// entry a, the pivot entry is broadcast with v_readlane).  ONE body: k_bc_t runs it on the workspace's z0 and t, k_bc_t_group (the
// sensitivity calls' groups, dev/adjoint.inc) once per workgroup on a column of its own.  M: BC_MAX * BC_MAX doubles of LDS, v: BC_MAX.
__device__ __forceinline__ void bc_t_body(int k, u64 act, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                          const double *__restrict__ aval, const double *__restrict__ z0, const double *__restrict__ SL, double *__restrict__ t,
                                          double *M, double *v) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < k * k; e += 1024) { const int i = e / k, j = e - i * k; if (j <= i) M[i * BC_MAX + j] = SL[i * BC_MAX + j]; }
    for (int a = wave; a < k; a += 16) {
        const int r = rows[bc_nth_slot(act, a)];
        double sacc = 0.0;
        for (int e = arp[r] + lane; e < arp[r + 1]; e += 64) sacc += aval[e] * z0[aci[e]];
        sacc = wave_sum(sacc);
        if (lane == 0) v[a] = sacc;
    }
    __syncthreads();
    bc_tri_solve(k, M, v, t);
}
__global__ __launch_bounds__(1024) void k_bc_t(int k, u64 act, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                               const double *__restrict__ aval, const double *__restrict__ z0, const double *__restrict__ SL,
                                               double *__restrict__ t) {
    __shared__ double M[BC_MAX * BC_MAX], v[BC_MAX];
    bc_t_body(k, act, rows, arp, aci, aval, z0, SL, t, M, v);
}
// (one workgroup per live column: z0 ldx apart, t BC_MAX apart, both compact over the live right-hand sides)
__global__ __launch_bounds__(1024) void k_bc_t_group(int k, u64 act, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                                     const double *__restrict__ aval, const double *__restrict__ z0, long long ldx,
                                                     const double *__restrict__ SL, double *__restrict__ t) {
    __shared__ double M[BC_MAX * BC_MAX], v[BC_MAX];
    const long long s = blockIdx.x;
    bc_t_body(k, act, rows, arp, aci, aval, z0 + s * ldx, SL, t + s * BC_MAX, M, v);
}
// out = z0 - Z(:, active slots) t.  ONE body, as above: k_bc_apply_group's grid.y is the live column (z0 and out ldx apart, t BC_MAX apart)
__device__ __forceinline__ void bc_apply_body(int n, int np, int k, u64 act, const double *__restrict__ Z, const double *__restrict__ t,
                                              const double *__restrict__ z0, double *__restrict__ out, double *ts, int *sl) {
    for (int a = threadIdx.x; a < k; a += blockDim.x) { ts[a] = t[a]; sl[a] = bc_nth_slot(act, a); }
    __syncthreads();
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        double sacc = 0.0;
        for (int a = 0; a < k; a++) sacc += Z[(size_t)sl[a] * np + j] * ts[a];
        out[j] = z0[j] - sacc;
    }
}
__global__ void k_bc_apply(int n, int np, int k, u64 act, const double *__restrict__ Z, const double *__restrict__ t, const double *__restrict__ z0,
                           double *__restrict__ out) {
    __shared__ double ts[BC_MAX]; __shared__ int sl[BC_MAX];
    bc_apply_body(n, np, k, act, Z, t, z0, out, ts, sl);
}
__global__ void k_bc_apply_group(int n, int np, int k, u64 act, const double *__restrict__ Z, const double *__restrict__ t, const double *__restrict__ z0,
                                 double *__restrict__ out, long long ldx) {
    __shared__ double ts[BC_MAX]; __shared__ int sl[BC_MAX];
    const long long s = blockIdx.y;
    bc_apply_body(n, np, k, act, Z, t + s * BC_MAX, z0 + s * ldx, out + s * ldx, ts, sl);
}

// ---- chain QPs with a few coupling VARIABLES (QPDO_BAND_BORDER; host side: dev/host_band.inc band_border_refresh) ----------------------------
// Variables that appear everywhere -- a global slack, a free final time, a shared parameter -- give K a dense row and column each, and no
// order narrows an arrowhead.  Numbered last, they leave K = [B C; C' D]: B (nc x nc, the core variables) banded, C nc x c, D c x c, c <=
// BC_MAX.  Block elimination is an exact LDL' of the SPD K in that order -- nothing cancels, so unlike the Woodbury solve of the coupling
// rows it needs no residual check around it:
//   refresh   B = L D L' (k_band_assemble / k_band_factor on n = nc: the assembly drops what lands at a row >= n, so Kb holds the bits of
//             the plain band workspace of the core-only problem), [C; D] (k_bb_assemble), Z = B^-1 C (k_band_solve_group, a workgroup
//             per column), S = D - C'Z (k_bb_S), S = L D L' in LDS (k_bc_factor_S);
//   solve     z0 = B^-1 rhs_1 (k_band_solve), t = S^-1 (rhs_2 - C'z0) (k_bb_t), x_1 = z0 - Z t, x_2 = t (k_bb_apply).
// C, Z and the forward results: columns np apart (np = nc rounded up to 4); D, S and its factor: leading dimension BC_MAX.
// Every sum below has a fixed order: the same call twice gives the same bits.

// Column jb of [C; D] = column v = nc + jb of K, one workgroup per border column, plain stores.  Rows of A are column-sorted, so the border
// entries of a row are its tail: A(r, v) is found by walking back from the row's end while the column is >= nc (at most c steps).
//   core rows i < nc, a thread per element: Q(i, v), then the weighted rows of A that hold both i and v in ascending order -- the
//     per-element order and the products (w A(r, v)) A(r, i) of band_assemble_body on column v; rows i = nc .. np-1 of C are zero;
//   border rows a >= jb, a wave per element (a border variable may sit in every row of A): lane l sums the rows l, l + 64, ... of its
//     variable's list, ascending, the lanes are summed by wave_sum's tree; Q(u, v) first, sigma_f on the diagonal last.  The element goes
//     to D(a, jb) and D(jb, a): D is symmetric bit for bit.
__global__ __launch_bounds__(1024) void k_bb_assemble(int nc, int np, int c, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                      const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                      const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                      const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                      double *__restrict__ Cm, double *__restrict__ Dm) {
    const int jb = blockIdx.x, v = nc + jb, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *col = Cm + (size_t)jb * np;
    // (w A(r, v)) a_ri added to acc when row r holds v; rows without v, or without weight, add nothing
    auto row_term = [&](int r, double a_ri, double &acc) {
        const double wgt = dw[r];
        if (wgt == 0.0) return;
        for (int e = arp[r + 1] - 1; e >= arp[r] && aci[e] >= nc; e--)
            if (aci[e] == v) { acc += (wgt * aval[e]) * a_ri; break; }
    };
    for (int i = threadIdx.x; i < np; i += 1024) {
        double acc = 0.0;
        if (i < nc) {
            for (int k = qrp[i]; k < qrp[i + 1]; k++) if (qci[k] == v) acc += qval[k];
            for (int t = trp[i]; t < trp[i + 1]; t++) row_term(tci[t], tval[t], acc);
        }
        col[i] = acc;
    }
    for (int a = jb + wave; a < c; a += 16) {
        const int u = nc + a;
        double qacc = 0.0, acc = 0.0;
        for (int k = qrp[u] + lane; k < qrp[u + 1]; k += 64) if (qci[k] == v) qacc += qval[k];
        for (int t = trp[u] + lane; t < trp[u + 1]; t += 64) row_term(tci[t], tval[t], acc);
        qacc = wave_sum(qacc); acc = wave_sum(acc);
        if (lane == 0) {
            double e = qacc + acc;
            if (a == jb) e += sigma_f;
            Dm[a * BC_MAX + jb] = e; Dm[jb * BC_MAX + a] = e;
        }
    }
}
// S(a, j) = D(a, j) - C(:, a)'Z(:, j), a >= j and its mirror image; one workgroup per element: thread l sums the rows l, l + 256, ...
// ascending, the threads are summed by wave_sum's tree and the four waves in order
__global__ __launch_bounds__(256) void k_bb_S(int nc, int np, const double *__restrict__ Cm, const double *__restrict__ Z, const double *__restrict__ Dm,
                                              double *__restrict__ S) {
    __shared__ double part[4];
    const int a = blockIdx.x, j = blockIdx.y;
    if (a < j) return;
    const double *ca = Cm + (size_t)a * np, *zj = Z + (size_t)j * np;
    double sacc = 0.0;
    for (int i = threadIdx.x; i < nc; i += 256) sacc += ca[i] * zj[i];
    sacc = wave_sum(sacc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sacc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = Dm[a * BC_MAX + j] - (((part[0] + part[1]) + part[2]) + part[3]);
        S[a * BC_MAX + j] = s; S[j * BC_MAX + a] = s;
    }
}
// t = S^-1 (rhs_2 - C'z0): the c dot products C(:, a)'z0, one wave each in turn (lane l sums the rows l, l + 64, ... ascending, then
// wave_sum's tree), then both triangular solves by one wave (bc_tri_solve).  One workgroup.
__global__ __launch_bounds__(1024) void k_bb_t(int nc, int np, int c, const double *__restrict__ Cm, const double *__restrict__ z0,
                                               const double *__restrict__ rhs2, const double *__restrict__ SL, double *__restrict__ t) {
    __shared__ double M[BC_MAX * BC_MAX], v[BC_MAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < c * c; e += 1024) { const int i = e / c, j = e - i * c; if (j <= i) M[i * BC_MAX + j] = SL[i * BC_MAX + j]; }
    for (int a = wave; a < c; a += 16) {
        const double *ca = Cm + (size_t)a * np;
        double sacc = 0.0;
        for (int i = lane; i < nc; i += 64) sacc += ca[i] * z0[i];
        sacc = wave_sum(sacc);
        if (lane == 0) v[a] = rhs2[a] - sacc;
    }
    __syncthreads();
    bc_tri_solve(c, M, v, t);
}
// in place on x = [z0; .]: x_1 = z0 - Z t (the columns in ascending order), x_2 = t
__global__ void k_bb_apply(int nc, int np, int c, const double *__restrict__ Z, const double *__restrict__ t, double *x) {
    __shared__ double ts[BC_MAX];
    for (int a = threadIdx.x; a < c; a += blockDim.x) ts[a] = t[a];
    __syncthreads();
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nc + c; j += gridDim.x * blockDim.x) {
        if (j >= nc) { x[j] = ts[j - nc]; continue; }
        double sacc = 0.0;
        for (int a = 0; a < c; a++) sacc += Z[(size_t)a * np + j] * ts[a];
        x[j] = x[j] - sacc;
    }
}
