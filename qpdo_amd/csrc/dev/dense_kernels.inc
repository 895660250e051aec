// dense_kernels.inc -- part of qpdo_dev.hip (one translation unit; included in order): dense LDL' kernels: assembly, diagonal block, panel, trailing update, chained and multi-RHS solves, low-rank update
// ================================================================================================
// Dense direct solver for K = Q + sigma_f I + A' diag(d) A  (reference N2/N4: cholmod_interface.c:8-52,
// 98-102).  With CHOLMOD's natural ordering and percent-level fill the normal-equations term is
// structurally dense, i.e. the supernodal factorization degenerates to ONE dense front of order n;
// this is that front: blocked right-looking LDL' (no pivoting, as CHOLMOD_LDLt on an SPD matrix) whose
// trailing update runs on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  Used when n <= dense_max_n.
// Storage: column-major lower triangle K[i + j*ld], ld = n rounded up to 64; the padding carries an
// identity so every block is full.  W (ld x 64) holds the scaled panel L*D of the current step.
// ================================================================================================
static const int DNB = 64;
static const unsigned long long CH_SENT = 0x7FF4DEADBEEF0001ULL;      // the polled vectors of the chained solves: "not yet written"
typedef double dvec4 __attribute__((ext_vector_type(4)));

#ifndef DENSE_ASM_PF
#define DENSE_ASM_PF 8
#endif
// one wave per column j: acc (LDS) gathers Q(:,j) and sum_r d_r a_rj a_r(:) for rows >= j.
// Sequential over r inside the wave, so the summation order is fixed (reproducible).
// The accumulator holds `tile` rows at a time (host: as many as fit in LDS, ~19 000): a column with more rows below the diagonal is
// assembled in row tiles [lo, lo + tile), each walking the column's weighted rows again and keeping only the entries that fall into
// the tile -- every element still receives its contributions in ascending row order, so the tiled and the untiled assembly give the
// same bits, and the order of the direct solver is bounded by HBM (an n x n matrix), not by LDS.
// (launch-ahead route: the product A't of the step's right-hand side rides on this launch -- blocks [g0, gridDim.x) --, through
// spmv_rows, the row loop of k_spmv, so the same bits; it writes the padded right-hand side itself)
struct AsmRhs { int on, g0, tpr, nrows; const int *rp, *ci; const double *val, *x, *rdi; double *atdy, *rhs; };
__global__ __launch_bounds__(64) void k_dense_assemble(int n, int ld, int tile, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                       const double *__restrict__ qval, const int *__restrict__ trp,
                                                       const int *__restrict__ tci, const double *__restrict__ tval,
                                                       const int *__restrict__ arp, const int *__restrict__ aci,
                                                       const double *__restrict__ aval, const double *__restrict__ dw,
                                                       double sigma_f, double *__restrict__ K,
                                                       const double *__restrict__ rb, double *__restrict__ rx, unsigned long long *__restrict__ rs1,
                                                       unsigned long long *__restrict__ rs2, const Ctrl *spec = nullptr, double sigma_f1 = 0.0,
                                                       AsmRhs ar = AsmRhs{}) {
    extern __shared__ __attribute__((aligned(16))) double acc_base[];
    __shared__ int l_e0[64], l_e1[64]; __shared__ double l_w[64];
    const int lane = threadIdx.x;
    // launch-ahead (vector.inc SpecArgs): leave if this pass is not a Newton step; sigma_f as qdev_newton_step sets it: the caller's
    // sigma_f is that of branches 0 and 2 (cholmod_interface.c:11-13), branch 1 keeps the factor's (sigma_f1)
    if (spec) { if (spec->cnt[C_SPEC_SKIP]) return; if (spec->cnt[C_SPEC_BRANCH] == 1) sigma_f = sigma_f1; }
    if (ar.on && (int)blockIdx.x >= ar.g0) {
        EpiRhsX e{ar.rdi, ar.atdy, ar.rhs, rx};
        spmv_rows((int)blockIdx.x - ar.g0, (int)gridDim.x - ar.g0, ar.tpr, ar.nrows, ar.rp, ar.ci, ar.val, ar.x, e, 64);
        return;
    }
    const int nblk = ar.on ? ar.g0 : (int)gridDim.x;                 // blocks of the assembly proper
    // (the one-launch factorization takes its right-hand side along: what k_dense_load_rhs does, without a launch of its own)
    if (rb) for (int i = blockIdx.x * 64 + lane; i < ld; i += nblk * 64) { rx[i] = i < n ? rb[i] : 0.0; rs1[i] = CH_SENT; rs2[i] = CH_SENT; }
    else if (ar.on) for (int i = blockIdx.x * 64 + lane; i < ld; i += nblk * 64) { if (i >= n) rx[i] = 0.0; rs1[i] = CH_SENT; rs2[i] = CH_SENT; }
    for (int j = blockIdx.x; j < ld; j += nblk) {
        double *col = K + (size_t)j * ld;
        if (j >= n) {                                  // identity padding
            for (int i = j + lane; i < ld; i += 64) col[i] = (i == j) ? 1.0 : 0.0;
            continue;
        }
      for (int lo = j; lo < n; lo += tile) {
        const int hi = (lo + tile < n) ? lo + tile : n;          // this pass assembles rows [lo, hi) of column j
        double *acc = acc_base - lo;                             // acc[i], lo <= i < hi
        for (int i = lo + lane; i < hi; i += 64) acc[i] = 0.0;
        __syncthreads();
        for (int k = qrp[j] + lane; k < qrp[j + 1]; k += 64) { const int i = qci[k]; if (i >= lo && i < hi) acc[i] += qval[k]; }
        __syncthreads();
        // Rows r of A with an entry in column j, in ascending order.  Finding the weighted ones is a chain of dependent
        // loads per row (row index -> weight -> row pointers); 64 rows at a time take that chain in parallel, one per lane,
        // and the weighted rows are compacted in order (ballot) into a small LDS list.  Their entries are then added row by
        // row -- the accumulation order per element is the row order, as before -- with the first 64 entries of the next
        // row already in flight.  (Walking the rows one by one cost ~1 us of exposed latency per row: 2.1 ms per assembly
        // at n = 1e4, most of it on the 63 % of rows whose weight is zero.)
        const int t0 = trp[j], t1 = trp[j + 1];
        for (int tb = t0; tb < t1; tb += 64) {
            const int t = tb + lane;
            int e0 = 0, e1 = 0; double w = 0.0; bool act = false;
            if (t < t1) {
                const int r = tci[t];
                const double wgt = dw[r];
                if (wgt != 0.0) { act = true; w = wgt * tval[t]; e0 = arp[r]; e1 = arp[r + 1]; }
            }
            const unsigned long long mask = __ballot(act);
            const int cnt = __popcll(mask);
            if (act) { const int pos = __popcll(mask & ((1ull << lane) - 1ull)); l_e0[pos] = e0; l_e1[pos] = e1; l_w[pos] = w; }
            __builtin_amdgcn_wave_barrier();
            // first 128 entries of the next PF rows in flight (register ring), the rest of a longer row on demand
            constexpr int PF = DENSE_ASM_PF;
            int pi[PF], pj[PF]; double pv[PF], pw[PF];
            auto fetch = [&](int u, int q) {
                pi[u] = -1; pj[u] = -1; pv[u] = 0.0; pw[u] = 0.0;
                if (q < cnt) {
                    const int e = l_e0[q] + lane, e1 = l_e1[q];
                    if (e < e1) { pi[u] = aci[e]; pv[u] = aval[e]; }
                    if (e + 64 < e1) { pj[u] = aci[e + 64]; pw[u] = aval[e + 64]; }
                }
            };
#pragma unroll
            for (int u = 0; u < PF; u++) fetch(u, u);
            for (int q0 = 0; q0 < cnt; q0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; u++) {
                    const int q = q0 + u;
                    if (q < cnt) {
                        const int b0 = l_e0[q], b1 = l_e1[q]; const double wq = l_w[q];
                        const int i0 = pi[u], i1 = pj[u]; const double v0 = pv[u], v1 = pw[u];
                        fetch(u, q + PF);
                        if (i0 >= lo && i0 < hi) acc[i0] += wq * v0;
                        if (i1 >= lo && i1 < hi) acc[i1] += wq * v1;
                        for (int e = b0 + 128 + lane; e < b1; e += 64) { const int i = aci[e]; if (i >= lo && i < hi) acc[i] += wq * aval[e]; }
                        // one wave: its LDS operations are issued and served in order, so the read-modify-writes of
                        // consecutive rows are ordered without a hardware barrier; the compiler must only keep the order
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();                      // (the row list is rewritten by the next batch of 64 rows)
        }
        __syncthreads();
        if (lane == 0 && lo == j) acc[j] += sigma_f;
        __syncthreads();
        for (int i = lo + lane; i < hi; i += 64) col[i] = acc[i];
        __syncthreads();
      }
        for (int i = n + lane; i < ld; i += 64) col[i] = 0.0;
    }
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane); hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}
// ---- hand-off between workgroups inside one launch (k_mid_factor): 8-byte agent-scope accesses on both sides --------------------
__device__ __forceinline__ double ld_agent(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent(double *p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDL' of a 64x64 diagonal block, eliminated in four 16-column sub-panels (diag64_lds_v2 below); the rest of the block is updated on
// the matrix cores (C -= X L'), and the inverse of the whole block is assembled from the four 16x16 inverses by block forward
// substitution, also on the matrix cores.  The block sits in LDS throughout:
//   T  [64][65]   the block; on exit strictly lower = L, diagonal = D
//   Ic [10][16][16]  lower 16x16 blocks of L^-1, block (bi, bj) at bi (bi + 1) / 2 + bj, element (r, c) at r*16 + (c ^ r) (bank swizzle)
//   cb [64]       with the first 64 doubles of Xs: the two column buffers of the sub-panel elimination
//   Xs [64][17]   X = L D of the current 16-column sub-panel (rows >= 16 only)
// 62 976 bytes.
static const int DG_TS = DNB + 1;
static const int DG_LDS = DNB * DG_TS + 10 * 256 + 64 + DNB * 17;          // doubles
__device__ __forceinline__ int ic_at(int bi, int bj, int r, int c) { return (bi * (bi + 1) / 2 + bj) * 256 + r * 16 + (c ^ r); }
__device__ __forceinline__ double diag64_inv(const double *Ic, int r, int c) {          // (L^-1)[r][c] of the whole block
    const int bi = r >> 4, bj = c >> 4;
    return bi < bj ? 0.0 : Ic[ic_at(bi, bj, r & 15, c & 15)];
}
// 16x16x16 product on one wave: acc += A B with A(r, k) = fa(r, k), B(k, c) = fb(k, c)
template <class FA, class FB>
__device__ __forceinline__ dvec4 mfma16(FA fa, FB fb, dvec4 acc, int li, int lk) {
#pragma unroll
    for (int k0 = 0; k0 < 16; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(li, k0 + lk), fb(k0 + lk, li), acc, 0, 0, 0);
    return acc;
}
#ifdef DG_TIMING
__device__ long long g_dg_t[32];
#define DG_T(i) do { if (threadIdx.x == 0) g_dg_t[i] = wall_clock64(); } while (0)
#define DG_T2(i, cond) do { if (cond) g_dg_t[i] = wall_clock64(); } while (0)
#else
#define DG_T(i) do { } while (0)
#define DG_T2(i, cond) do { } while (0)
#endif
#ifndef DIAG_READLANE_ONLY
#define DIAG_LDS_BCAST 1      // (lab switch: -DDIAG_READLANE_ONLY keeps every broadcast on v_readlane, 2.3 instead of 2.0 us per sub-panel)
#endif
// ---- the 16-column sub-panels eliminated IN REGISTERS ---------------------------------------------------------------------------------
// Wave 0 holds the whole 64-row x 16-column sub-panel, one row per lane and 16 registers: the pivot and the 15-j entries of column j
// that the step needs are the register r[j] of lanes o+j .. o+15, taken with v_readlane into SGPRs -- no LDS round trip, and as scalar
// operands they serve all 64 lanes, so the rows BELOW the sub-block are eliminated by the very same instructions.  A step is a
// reciprocal (v_rcp + two Newton steps), 2 (16 - j) readlanes and 15 - j FMAs.  Meanwhile the idle waves invert the 16 x 16 unit-lower factors the same way (row k of the
// running inverse broadcast by readlane) and form the off-diagonal blocks of L^-1 on the matrix cores as soon as their operands are
// final, so only the last block row of the inverse is left when the factorization ends.  (Rounds 2-4 published each column through
// LDS instead, ~165 ns per pivot for the 16 rows of the sub-block alone, and then ran an MFMA phase for the rows below: LAB_NOTES.)
// NW waves may share the work: the columns of the inverse are independent of each other, wave w of the team takes columns w, w + NW, ...
template <int NW, int w>
__device__ __forceinline__ void tri16_inv_wave(const double *T, double *Ic, int s, int l) {
    // inverse of the unit-lower 16 x 16 block (s, s) of L: lanes 0-15 hold row i of L (a[k], k < i) and row i of the running inverse
    constexpr int TS = DG_TS;
    const int o = 16 * s, i = l & 15;
    double a[16], mrow[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { const double t = T[(o + i) * TS + o + k]; a[k] = (k < i) ? t : 0.0; mrow[k] = (k == i) ? 1.0 : 0.0; }
#pragma unroll
    for (int k = 0; k < 15; k++) {
        // row k of the inverse is final: rows i > k take  M(i, c) -= L(i, k) M(k, c), c <= k  (a[k] = 0 for i <= k)
#pragma unroll
        for (int c = 0; c <= k; c++) if (NW == 1 || (c % NW) == w) { const double mk = lane_bcast(mrow[c], k); mrow[c] = fma(-a[k], mk, mrow[c]); }
    }
    if (l < 16) {
#pragma unroll
        for (int c = 0; c < 16; c++) if (NW == 1 || (c % NW) == w) Ic[ic_at(s, s, i, c)] = (c <= i) ? mrow[c] : 0.0;
    }
}
// product chain of one off-diagonal block of L^-1:  X(bi, bj) = - X(bi, bi) sum_{k = bj}^{bi - 1} L(bi, k) X(k, bj)  (one wave)
__device__ __forceinline__ void inv_block_wave(const double *T, double *Ic, int bi, int bj, int li, int lk) {
    constexpr int TS = DG_TS;
    dvec4 acc = (dvec4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = bj; k < bi; k++)
        acc = mfma16([&](int r, int kk) { return T[(bi * 16 + r) * TS + k * 16 + kk]; },
                     [&](int kk, int c) { return Ic[ic_at(k, bj, kk, c)]; }, acc, li, lk);
#pragma unroll
    for (int v = 0; v < 4; v++) Ic[ic_at(bi, bj, lk + 4 * v, li)] = acc[v];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    dvec4 a2 = (dvec4){0.0, 0.0, 0.0, 0.0};
    a2 = mfma16([&](int r, int kk) { return Ic[ic_at(bi, bi, r, kk)]; },
                [&](int kk, int c) { return Ic[ic_at(bi, bj, kk, c)]; }, a2, li, lk);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int v = 0; v < 4; v++) Ic[ic_at(bi, bj, lk + 4 * v, li)] = -a2[v];
}
// nsub: 16-column sub-panels that hold matrix columns (the rest of the block is the identity padding of the last block of a matrix
// whose order is not a multiple of 64: nothing to eliminate there, its part of L^-1 is the identity).
__device__ __forceinline__ void diag64_lds_v2(double *T, double *Ic, double *Xs, int tid, int nsub = 4) {
    const int wave = tid >> 6, l = tid & 63;
    const int li = l & 15, lk = l >> 4;
    constexpr int TS = DG_TS;
#pragma unroll 1
    for (int s = 0; s < nsub; s++) {
        const int o = 16 * s;
        if (wave == 0) {
            double r[16], dd[16];
#ifdef DIAG_LDS_BCAST
            double *cbq = Ic + 10 * 256;                                     // the 128 doubles behind the inverse blocks (cb + the head of Xs: rows < 16 of Xs are never used)
#endif
#pragma unroll
            for (int c = 0; c < 16; c++) r[c] = T[l * TS + o + c];           // (lanes above the sub-panel carry entries of the upper triangle: never stored)
#ifdef DIAG_LDS_BCAST
            // Step j = a reciprocal chain (pivot by v_readlane, v_rcp + two Newton steps, s = a / d) and rank-1 updates of the columns behind it.
            // Only column j + 1 -- the next pivot's -- needs its update now (one v_readlane pair); the updates of columns >= j + 2 are
            // DEFERRED by one step: column j goes to LDS once, its entries come back as broadcast reads (two per instruction instead of two
            // v_readlane per entry) that have a whole step to land, and the FMAs that use them fill the issue slots of the next reciprocal chain.
            double vp[16], sp = 0.0;
#pragma unroll
            for (int c = 0; c < 16; c++) vp[c] = 0.0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                double vn[16];
                if (j < 14) {
                    cbq[(j & 1) * 64 + l] = r[j];
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
                    for (int c = j + 2; c < 16; c++) vn[c] = cbq[(j & 1) * 64 + o + c];
                }
                const double dj = lane_bcast(r[j], o + j);
                double inv = __builtin_amdgcn_rcp(dj);
                inv = fma(fma(-dj, inv, 1.0), inv, inv);
                inv = fma(fma(-dj, inv, 1.0), inv, inv);
                dd[j] = dj;
                const double sj = r[j] * inv;
                if (j < 15) { const double vc = lane_bcast(r[j], o + j + 1); r[j + 1] = fma(-sj, vc, r[j + 1]); }
                if (j >= 1) {
#pragma unroll
                    for (int c = j + 1; c < 16; c++) r[c] = fma(-sp, vp[c], r[c]);
                }
                r[j] = (l > o + j) ? sj : r[j];
                sp = sj;
                if (j < 14) {
#pragma unroll
                    for (int c = j + 2; c < 16; c++) vp[c] = vn[c];
                }
            }
#else
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const double dj = lane_bcast(r[j], o + j);
                double inv = __builtin_amdgcn_rcp(dj);
                inv = fma(fma(-dj, inv, 1.0), inv, inv);
                inv = fma(fma(-dj, inv, 1.0), inv, inv);
                dd[j] = dj;
                const double sj = r[j] * inv;
#pragma unroll
                for (int c = j + 1; c < 16; c++) { const double vc = lane_bcast(r[j], o + c); r[c] = fma(-sj, vc, r[c]); }
                r[j] = (l > o + j) ? sj : r[j];
            }
#endif
            if (l >= o) {
#pragma unroll
                for (int c = 0; c < 16; c++) if (l - o >= c) T[l * TS + o + c] = r[c];       // L below the diagonal, D on it
            }
            if (l >= o + 16) {
#pragma unroll
                for (int c = 0; c < 16; c++) Xs[l * 17 + c] = r[c] * dd[c];                  // X = L D for the update of the rest of the block
            }
        } else if (s > 0) {
            // in the shadow of sub-panel s: the inverse of the unit-lower block (s-1, s-1) [wave 1] and, during the last sub-panel, the
            // blocks of L^-1 whose operands are final by then: X(1,0) [wave 2], X(2,1) [wave 1, behind its X(2,2)]
            if (wave == 1) {
                tri16_inv_wave<1, 0>(T, Ic, s - 1, l);
                if (s == 3) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); inv_block_wave(T, Ic, 2, 1, li, lk); }
            } else if (wave == 2 && s == 3) inv_block_wave(T, Ic, 1, 0, li, lk);
        }
        DG_T2(16 + 2 * s, wave == 0 && l == 0);
        __syncthreads();
        DG_T(17 + 2 * s);
        if (s == nsub - 1) break;
        // the rest of the block: C(bi, bj) -= X(bi) L(bj)', s < bj <= bi < nsub, dealt over the waves
        {
            int q = 0;
#pragma unroll 1
            for (int bi = s + 1; bi < nsub; bi++)
#pragma unroll 1
                for (int bj = s + 1; bj <= bi; bj++, q++) {
                    if ((q & 3) != wave) continue;
                    dvec4 acc = (dvec4){0.0, 0.0, 0.0, 0.0};
                    acc = mfma16([&](int r, int k) { return Xs[(bi * 16 + r) * 17 + k]; },
                                 [&](int k, int c) { return T[(bj * 16 + c) * TS + o + k]; }, acc, li, lk);
#pragma unroll
                    for (int v = 0; v < 4; v++) { double *t = &T[(bi * 16 + lk + 4 * v) * TS + bj * 16 + li]; *t = *t - acc[v]; }
                }
        }
        __syncthreads();
        DG_T(4 + 3 * s);
    }
    if (nsub == 4) {
        // what is left of the inverse: X(3,3) [its columns dealt over waves 0-2], X(2,0) [wave 3: needs X(1,0), X(2,2)]; then block row 3
        if (wave == 0) tri16_inv_wave<3, 0>(T, Ic, 3, l);
        else if (wave == 1) tri16_inv_wave<3, 1>(T, Ic, 3, l);
        else if (wave == 2) tri16_inv_wave<3, 2>(T, Ic, 3, l);
        else inv_block_wave(T, Ic, 2, 0, li, lk);
        __syncthreads();
        DG_T(24);
        if (wave < 3) inv_block_wave(T, Ic, 3, 2 - wave, li, lk);          // X(3,2), X(3,1), X(3,0): column bj = 2 - wave needs X(k, bj), k < 3 (all final)
        __syncthreads();
        DG_T(25);
        return;
    }
    // a padded block: identity blocks of L^-1 for the padding, the last factored 16 x 16 inverse, then the blocks below the diagonal by
    // block diagonals
    for (int e = tid; e < 10 * 256; e += 256) {
        const int blk = e >> 8, r = (e >> 4) & 15, c = e & 15;
        int bi = 0; while ((bi + 1) * (bi + 2) / 2 <= blk) bi++;
        const int bj = blk - bi * (bi + 1) / 2;
        if (bi >= nsub) Ic[ic_at(bi, bj, r, c)] = (bi == bj && r == c) ? 1.0 : 0.0;
    }
    if (wave == 0) tri16_inv_wave<1, 0>(T, Ic, nsub - 1, l);
    __syncthreads();
#pragma unroll 1
    for (int dgl = 1; dgl < nsub; dgl++) {
        const int bi = dgl + wave, bj = wave;
        if (bi < nsub) inv_block_wave(T, Ic, bi, bj, li, lk);
        __syncthreads();
    }
}
// load block kb into LDS, factor, write L (strictly lower part of K), D, L^-1 (column-major: Li[c*64 + r] = (L^-1)[r][c], for the
// panel solve and the forward solves) and its transpose (LiT[r*64 + c], backward solves)
__device__ __forceinline__ void diag64_block(double *S, double *__restrict__ K, int ld, int kb, double *__restrict__ Dg, double *__restrict__ Linv,
                             double *__restrict__ LinvT, int tid) {
    double *T = S, *Ic = S + DNB * DG_TS, *Xs = Ic + 10 * 256 + 64;
    const size_t base = (size_t)kb * DNB + (size_t)kb * DNB * ld;
    const int r = tid & 63, c0 = tid >> 6;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) { const int c = c0 + 4 * e; T[r * DG_TS + c] = K[base + r + (size_t)c * ld]; }
    DG_T(0);
    __syncthreads();
    DG_T(1);
    diag64_lds_v2(T, Ic, Xs, tid);
    DG_T(14);
    double *o1 = Linv + (size_t)kb * DNB * DNB, *o2 = LinvT + (size_t)kb * DNB * DNB;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int c = c0 + 4 * e;
        if (r > c) K[base + r + (size_t)c * ld] = T[r * DG_TS + c];
        o1[(size_t)c * DNB + r] = diag64_inv(Ic, r, c);
        o2[(size_t)c * DNB + r] = diag64_inv(Ic, c, r);
    }
    if (tid < DNB) Dg[kb * DNB + tid] = T[tid * DG_TS + tid];
    DG_T(15);
}
__global__ __launch_bounds__(256) void k_ldl_diag_blocked(double *__restrict__ K, int ld, int kb, double *__restrict__ Dg, double *__restrict__ Linv,
                                                          double *__restrict__ LinvT) {
    __shared__ double S[DG_LDS];
    diag64_block(S, K, ld, kb, Dg, Linv, LinvT, threadIdx.x);
}
// panel below the diagonal block on the matrix cores: X = A L_kk^-T  =>  W = X (= L D), L = X / D.  L is also written
// transposed into the upper triangle of K so that the backward solve reads contiguous columns.
// One workgroup per 64-row tile.  S: 2*32*80 doubles of LDS.
__device__ __forceinline__ void ldl_panel_tile(double *S, double *__restrict__ K, int ld, int kb, int ti, int wcol, const double *__restrict__ Dg,
                                               const double *__restrict__ Linv, double *__restrict__ W) {
    // 40 KB of LDS (two 32-deep k chunks through the same buffers) so that the tiles of a panel find room beside the trailing
    // update's workgroups; the three outputs leave through an LDS image of the tile and are written along contiguous rows
    // (the per-lane stores of the accumulator layout hit 16 columns x 32 B per instruction: 54 us per panel under load, now 34).
    constexpr int KC = 32;
    double (*As)[80] = reinterpret_cast<double (*)[80]>(S);
    double (*Bs)[80] = reinterpret_cast<double (*)[80]>(S + KC * 80);
    const int tid = threadIdx.x;
    const double *Li = Linv + (size_t)kb * DNB * DNB;
    const int wave = tid >> 6, l = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int li = l & 15, lk = l >> 4;
    dvec4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc[m][q] = (dvec4){0.0, 0.0, 0.0, 0.0};
    for (int h = 0; h < DNB / KC; h++) {
        __syncthreads();                                           // (also: a previous tile of this workgroup is done with S)
        for (int idx = tid; idx < KC * DNB; idx += 256) {
            const int r = idx % DNB, k = idx / DNB, kg = h * KC + k;
            As[k][r] = K[(size_t)ti * DNB + r + ((size_t)kb * DNB + kg) * ld];      // A[row r][k]
            Bs[k][r] = Li[(size_t)kg * DNB + r];                                      // B[k][col r] = (L^-1)[r][k]
        }
        __syncthreads();
#pragma unroll 4
        for (int k0 = 0; k0 < KC; k0 += 4) {
            const double a0 = As[k0 + lk][wr + li], a1 = As[k0 + lk][wr + 16 + li];
            const double b0 = Bs[k0 + lk][wc + li], b1 = Bs[k0 + lk][wc + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    __syncthreads();
    // X = A L_kk^-T as a [col][row] image (row stride 65: conflict-free along rows and along columns)
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int v = 0; v < 4; v++) S[(wc + q * 16 + li) * (DNB + 1) + wr + m * 16 + lk + 4 * v] = acc[m][q][v];
    __syncthreads();
    const int lr = tid & 63, c0 = tid >> 6;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int col = c0 + 4 * e;
        const double x = S[col * (DNB + 1) + lr];
        W[(size_t)ti * DNB + lr + ((size_t)wcol * DNB + col) * ld] = x;                   // W = L D
        K[(size_t)ti * DNB + lr + ((size_t)kb * DNB + col) * ld] = x / Dg[kb * DNB + col];                                // L
    }
    const double dl = Dg[kb * DNB + lr];
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {                                                  // L' in the (otherwise unused) upper triangle
        const int row = c0 + 4 * e;                                                      // tile row -> column of the transposed copy
        K[(size_t)kb * DNB + lr + ((size_t)ti * DNB + row) * ld] = S[lr * (DNB + 1) + row] / dl;
    }
}
__global__ __launch_bounds__(256) void k_ldl_panel(double *__restrict__ K, int ld, int kb, int wcol, const double *__restrict__ Dg,
                                                   const double *__restrict__ Linv, double *__restrict__ W) {
    __shared__ double S[2 * 32 * 80];
    ldl_panel_tile(S, K, ld, kb, kb + 1 + blockIdx.x, wcol, Dg, Linv, W);
}
// update on the matrix cores: C(ti,tj) -= sum_{q<nkb} W(ti, wcol0+q) * L(tj, kb0+q)'  for tj in [tj_lo, tj_hi), ti >= tj.
// nkb = 1 updates the rest of the current 256-wide outer panel, nkb = 4 the trailing matrix (one read-modify-write
// of C per 256 eliminated columns instead of per 64).  Software pipelined: the k dimension is cut into 16-deep
// chunks held in double-buffered LDS tiles; the global loads of chunk c+1 are in flight while the MFMAs of chunk c
// run (one barrier per chunk; 40 KB LDS => four workgroups per CU).
static const int SY_KC = 16;
static const int SY_STRIP = 8;
// number of tiles of the trapezoid {C columns, R rows, column <= row} (host side of the 1-D order below)
static inline int syrk_tiles(int R, int C) {
    int tot = 0;
    for (int s0 = 0; s0 < C; s0 += SY_STRIP) {
        const int w = (C - s0 < SY_STRIP) ? C - s0 : SY_STRIP, h = R - s0;
        tot += (h >= w) ? w * (w + 1) / 2 + (h - w) * w : h * (h + 1) / 2;
    }
    return tot;
}
// S: max(4 * SY_KC * 80, 64 * 65) doubles of LDS.
__device__ __forceinline__ void ldl_syrk_tile(double *S, double *__restrict__ K, int ld, const double *__restrict__ W, int kb0, int nkb, int wcol0,
                                              int ti, int tj) {
    // one LDS array: A tiles [buf][k][row] at S + buf*T, B tiles at S + (2+buf)*T, T = SY_KC*80 (row stride 80 doubles: the
    // two k-rows of a half-wave hit disjoint banks); reused as the [col][row] image of the C tile in the epilogue
    constexpr int T = SY_KC * 80;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, l = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int li = l & 15, lk = l >> 4;
    const int lr = tid & 63, lk0 = tid >> 6;                      // this thread stages rows lr, k = lk0 + 4 e
    const int nch = nkb * (DNB / SY_KC);
    const double *Wp = W + (size_t)ti * DNB + lr, *Kp = K + (size_t)tj * DNB + lr;
    double ra0[SY_KC / 4], rb0[SY_KC / 4], ra1[SY_KC / 4], rb1[SY_KC / 4];
    auto gload = [&](int ch, double (&ra)[SY_KC / 4], double (&rb)[SY_KC / 4]) {
        const int q = ch / (DNB / SY_KC), h = ch % (DNB / SY_KC);
        const size_t wc0 = ((size_t)(wcol0 + q) * DNB + (size_t)h * SY_KC) * ld, kc0 = ((size_t)(kb0 + q) * DNB + (size_t)h * SY_KC) * ld;
#pragma unroll
        for (int e = 0; e < SY_KC / 4; e++) { const size_t ko = (size_t)(lk0 + 4 * e) * ld; ra[e] = Wp[wc0 + ko]; rb[e] = Kp[kc0 + ko]; }
    };
    auto lstore = [&](int buf, const double (&ra)[SY_KC / 4], const double (&rb)[SY_KC / 4]) {
        double *A = S + buf * T, *B = S + (2 + buf) * T;
#pragma unroll
        for (int e = 0; e < SY_KC / 4; e++) { A[(lk0 + 4 * e) * 80 + lr] = ra[e]; B[(lk0 + 4 * e) * 80 + lr] = rb[e]; }
    };
    dvec4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc[m][q] = (dvec4){0.0, 0.0, 0.0, 0.0};
    auto chunk = [&](int buf) {
        const double *A = S + buf * T, *B = S + (2 + buf) * T;
#pragma unroll
        for (int k0 = 0; k0 < SY_KC; k0 += 4) {
            const double a0 = A[(k0 + lk) * 80 + wr + li], a1 = A[(k0 + lk) * 80 + wr + 16 + li];
            const double b0 = B[(k0 + lk) * 80 + wc + li], b1 = B[(k0 + lk) * 80 + wc + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    };
    // Chunk c is computed from LDS buffer c&1 while the loads of chunk c+1 (issued one iteration ago) land in one register set and
    // those of chunk c+2 are issued into the other: a load has two chunk times to arrive, not one (the loop ran at the L2/MALL
    // latency, not at the MFMA rate).  nch is a multiple of DNB / SY_KC >= 2, the loop is unrolled by two so the sets are static.
    __syncthreads();                                               // a previous tile of this workgroup is done with S
    gload(0, ra0, rb0); lstore(0, ra0, rb0);
    gload(1, ra1, rb1);
    __syncthreads();
    for (int ch = 0; ch + 2 < nch; ch += 2) {
        gload(ch + 2, ra0, rb0);
        chunk(0);
        lstore(1, ra1, rb1);
        __syncthreads();
        gload(ch + 3, ra1, rb1);                                  // nch is even: chunk ch + 3 exists
        chunk(1);
        lstore(0, ra0, rb0);
        __syncthreads();
    }
    chunk(0);
    lstore(1, ra1, rb1);
    __syncthreads();
    chunk(1);
    __syncthreads();
    // C -= acc, coalesced: the accumulators (4 rows x 16 columns per wave instruction) go through LDS as a [col][row]
    // image so that the global read-modify-write runs along the contiguous rows
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int v = 0; v < 4; v++) S[(wc + q * 16 + li) * (DNB + 1) + wr + m * 16 + lk + 4 * v] = acc[m][q][v];
    __syncthreads();
    double *Cp = K + (size_t)ti * DNB + lr + (size_t)tj * DNB * ld;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int col = lk0 + 4 * e;
        double *cp = Cp + (size_t)col * ld;
        *cp = *cp - S[col * (DNB + 1) + lr];
    }
}
__global__ __launch_bounds__(256, 4) void k_ldl_syrk(double *__restrict__ K, int ld, const double *__restrict__ W, int kb0, int nkb, int wcol0,
                                                     int tj_lo, int tj_hi, int nb_swz) {
    int ti, tj;
    if (nb_swz > 0) {
        // 1-D grid over the tiles of the trapezoid {tj_lo <= tj < tj_hi, tj <= ti < nb}, in an order made for the eight L2s: workgroups
        // are dealt round-robin over the XCDs, so XCD x takes the x-th eighth of the order, and the order runs through strips of
        // SY_STRIP tile columns row by row -- the ~112 tiles an XCD works on at a time form a 14 x 8 patch that shares 22 operand
        // panels (2.8 MB of its 4 MB L2).  With the 2-D grid every tile of an XCD had its own W panel: 51 % L2 hits (r02 counters).
        const int cpx = gridDim.x >> 3;
        int t = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
        const int R = nb_swz - tj_lo, C = tj_hi - tj_lo;
        int s0 = 0, found = 0, r = 0, c = 0;
        for (; s0 < C; s0 += SY_STRIP) {
            const int w = (C - s0 < SY_STRIP) ? C - s0 : SY_STRIP, h = R - s0;
            const int head = (h >= w) ? w * (w + 1) / 2 : h * (h + 1) / 2;
            const int cnt = (h >= w) ? head + (h - w) * w : head;
            if (t < cnt) {
                if (t < head) { r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f); while (r * (r + 1) / 2 > t) r--; while ((r + 1) * (r + 2) / 2 <= t) r++; c = t - r * (r + 1) / 2; }
                else { r = w + (t - head) / w; c = (t - head) % w; }
                found = 1;
                break;
            }
            t -= cnt;
        }
        if (!found) return;
        ti = tj_lo + s0 + r; tj = tj_lo + s0 + c;
    } else {
        ti = tj_lo + blockIdx.x; tj = tj_lo + blockIdx.y;
        if (tj >= tj_hi || tj > ti) return;
    }
    constexpr int SZ = (4 * SY_KC * 80 > DNB * (DNB + 1)) ? 4 * SY_KC * 80 : DNB * (DNB + 1);
    __shared__ double S[SZ];
    ldl_syrk_tile(S, K, ld, W, kb0, nkb, wcol0, ti, tj);
}
// forward step kb: z_k = L_kk^-1 x_k (matrix-vector with the stored inverse: no serial chain), wave 0 publishes
// it, then wave b updates the 64 rows of block kb+1+b:  x_i -= L(i, kb) z_k.
__global__ __launch_bounds__(64) void k_ldl_fwd(const double *__restrict__ K, int ld, int kb, const double *__restrict__ Linv,
                                                double *__restrict__ x, double *__restrict__ z) {
    __shared__ double xs[DNB], zs[DNB];
    const int l = threadIdx.x;
    xs[l] = x[kb * DNB + l];
    __syncthreads();
    const double *Li = Linv + (size_t)kb * DNB * DNB;
    double v = 0.0;
    for (int c = 0; c < DNB; c++) v += Li[(size_t)c * DNB + l] * xs[c];
    zs[l] = v;
    if (blockIdx.x == 0) z[kb * DNB + l] = v;
    __syncthreads();
    const int r = (kb + 1 + blockIdx.x) * DNB + l;
    if (r >= ld) return;
    const double *row = K + r + (size_t)kb * DNB * ld;
    double sacc = x[r];
    for (int c = 0; c < DNB; c++) sacc -= row[(size_t)c * ld] * zs[c];
    x[r] = sacc;
}
// backward step kb: x_k = L_kk^-T y_k, publish, then wave j (< kb) updates y_j -= L(kb, j)' x_k through an LDS
// transpose of the 64x64 tile.
__global__ __launch_bounds__(64) void k_ldl_bwd(const double *__restrict__ K, int ld, int kb, const double *__restrict__ Linv,
                                                double *__restrict__ y, double *__restrict__ xout) {
    __shared__ double xs[DNB], ys[DNB];
    __shared__ double tile[DNB][DNB + 1];
    const int l = threadIdx.x;
    ys[l] = y[kb * DNB + l];
    const double *Li = Linv + (size_t)kb * DNB * DNB;
    for (int c = 0; c < DNB; c++) tile[l][c] = Li[(size_t)c * DNB + l];        // tile[r][c] = (L^-1)[r][c]
    __syncthreads();
    double v = 0.0;
    for (int r = 0; r < DNB; r++) v += tile[r][l] * ys[r];                      // (L^-T y)_l = sum_r (L^-1)[r][l] y_r
    xs[l] = v;
    if (blockIdx.x == 0) xout[kb * DNB + l] = v;
    __syncthreads();
    const int j = blockIdx.x;                            // 0 .. kb-1
    if (kb == 0 || j >= kb) return;
    for (int c = 0; c < DNB; c++) tile[l][c] = K[(size_t)kb * DNB + l + ((size_t)j * DNB + c) * ld];   // rows contiguous across lanes
    __syncthreads();
    double sacc = y[j * DNB + l];
    for (int r = 0; r < DNB; r++) sacc -= tile[r][l] * xs[r];
    y[j * DNB + l] = sacc;
}
// ---- triangular solves as ONE launch per direction ------------------------------------------------------
// Workgroup b owns block row b.  Forward: x_b - sum_{k<b} L(b,k) z_k, then z_b = L_bb^-1 (.), published to z; the
// consumers poll z itself (pre-filled with a signalling-NaN pattern no arithmetic produces) with device-scope
// loads, so one cross-XCD round trip separates consecutive steps instead of a kernel launch (157 dependent
// launches of ~11.5 us at n = 1e4).  Backward is the same kernel on the transposed tiles the panel kernel left in
// the upper triangle, with the block order reversed.  Workgroup b waits only on workgroups dispatched before it,
// so the grid drains for any dispatch width; a bounded spin turns a lost producer into NaNs + C_CHAIN_ERR.
static const int CH_SPIN_MAX = 1 << 22;
__global__ void k_fill_sentinel(int n, double *__restrict__ a, double *__restrict__ b) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        reinterpret_cast<unsigned long long *>(a)[i] = CH_SENT; reinterpret_cast<unsigned long long *>(b)[i] = CH_SENT;
    }
}
template <bool FWD>
__global__ __launch_bounds__(256) void k_ldl_chain(const double *__restrict__ K, int ld, int nb, const double *__restrict__ Li,
                                                   const double *__restrict__ Dg, const double *__restrict__ rhs, double *pub,
                                                   double *__restrict__ yout, int nout, Ctrl *ctrl, int spec = 0) {
    __shared__ double part[4][DNB];
    __shared__ double tot[DNB];
    if (spec && ctrl->cnt[C_SPEC_SKIP]) return;                     // launch-ahead (vector.inc SpecArgs): this pass is not a Newton step
    // grid (nrhs, nb): blockIdx.x = right-hand side (columns ld apart), blockIdx.y = position in the chain.  With the
    // right-hand side as the fast grid dimension the chains of all columns advance together and a workgroup still
    // depends only on workgroups dispatched before it.
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int ndep = blockIdx.y;                                    // blocks this one waits for
    const int b = FWD ? (int)blockIdx.y : nb - 1 - (int)blockIdx.y;
    rhs += (size_t)blockIdx.x * ld; pub += (size_t)blockIdx.x * ld; if (yout) yout += (size_t)blockIdx.x * ld;
    double li[16], cur[16], nxt[16];
    const double *Lb = Li + (size_t)b * DNB * DNB + (size_t)(w * 16) * DNB + l;
#pragma unroll
    for (int q = 0; q < 16; q++) li[q] = Lb[(size_t)q * DNB];
    const double *Kb = K + (size_t)b * DNB + l + (size_t)(w * 16) * ld;      // tile (b,k): + k*64*ld, element (l, w*16+q): + q*ld
    auto kof = [&](int j) { return FWD ? j : nb - 1 - j; };
    if (ndep > 0) {
        const double *t = Kb + (size_t)kof(0) * DNB * ld;
#pragma unroll
        for (int q = 0; q < 16; q++) cur[q] = t[(size_t)q * ld];
    }
    double acc = 0.0;
    bool lost = false;
    for (int j = 0; j < ndep; j++) {
        if (j + 1 < ndep) {
            const double *t = Kb + (size_t)kof(j + 1) * DNB * ld;
#pragma unroll
            for (int q = 0; q < 16; q++) nxt[q] = t[(size_t)q * ld];
        }
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(pub) + (size_t)kof(j) * DNB + w * 16 + (l & 15);
        unsigned long long bits = CH_SENT;
        int spins = 0;
        for (;;) {
            if (l < 16) bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all(l >= 16 || bits != CH_SENT)) break;
            if (++spins > CH_SPIN_MAX) { lost = true; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        const double v = lost ? __longlong_as_double(0x7FF8000000000000LL) : __longlong_as_double((long long)bits);
#pragma unroll
        for (int q = 0; q < 16; q++) acc += cur[q] * lane_bcast(v, q);
#pragma unroll
        for (int q = 0; q < 16; q++) cur[q] = nxt[q];
    }
    part[w][l] = acc;
    __syncthreads();
    if (w == 0) tot[l] = rhs[(size_t)b * DNB + l] - ((part[0][l] + part[1][l]) + (part[2][l] + part[3][l]));
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; q++) s += li[q] * tot[w * 16 + q];
    part[w][l] = s;                                                 // the first use of part ended before the barrier above
    __syncthreads();
    if (w == 0) {
        double r = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
        unsigned long long rb = (unsigned long long)__double_as_longlong(r);
        if (rb == CH_SENT) rb = 0x7FF8000000000000ULL;
        if (FWD) yout[(size_t)b * DNB + l] = r / Dg[(size_t)b * DNB + l];
        else if (yout && b * DNB + l < nout) yout[(size_t)b * DNB + l] = r;      // backward: optional plain copy of the solution (first nout entries)
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(pub) + (size_t)b * DNB + l, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the value IS the payload: nothing to release, and a release here is an L2 write-back per step)
    }
    if (lost && tid == 0) atomicOr(&ctrl->cnt[C_CHAIN_ERR], 1);
}

// ---- the low-rank factor update ---------------------------------------------------------------------------
// The reference keeps its factor current with rank-<=100 LDL' up/downdates when few rows enter or leave
// (cholmod_interface.c:57-93, newton.c:21-30).  Here the factor K0 = L D L' of the last full factorization
// is kept and the change K = K0 + U' W U (U = the rows of A whose weight d_i moved since then, W = diag(d - d_fact))
// is applied in the solve:  K^-1 r = z0 - Z (I + W G)^-1 W U z0,  z0 = K0^-1 r,  Z = K0^-1 U',  G = U Z.
// Z gains one column per new row (chained solves, one chain per column, all advancing together), G one row and column;
// the (<= WB_MAX)^2 system is solved in LDS.  Same linear system as the reference's updated factor.
static const int WB_MAX = 256;          // rows in the low-rank set; beyond WB_LDS_MAX the small system is eliminated in global memory
static const int WB_LDS_MAX = 128;
static const double WB_MIN_PIVOT = 1e-6;      // smallest |pivot| of I + W G accepted (refinement recovers a few digits, not a singular downdate)
// rows whose weight moved since the factorization and that hold no slot yet get the next slots, in row order
__global__ __launch_bounds__(1024) void k_wb_select(int m, const double *__restrict__ dw, const double *__restrict__ dfact, int *__restrict__ slot,
                                                    int *__restrict__ rows, int k_old, int *__restrict__ cnt) {
    __shared__ int sums[1024];
    const int chunk = (m + 1023) / 1024;
    const int beg = threadIdx.x * chunk, end = min(beg + chunk, m);
    int c = 0;
    for (int i = beg; i < end; i++) c += (dw[i] != dfact[i] && slot[i] < 0);
    sums[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < 1024; i++) { int t = sums[i]; sums[i] = run; run += t; } cnt[0] = k_old + run; }
    __syncthreads();
    int pos = k_old + sums[threadIdx.x];
    for (int i = beg; i < end; i++)
        if (dw[i] != dfact[i] && slot[i] < 0) { if (pos < WB_MAX) { rows[pos] = i; slot[i] = pos; } pos++; }
}
// right-hand side columns: X(:, k_old + b) = row rows[k_old + b] of A as a dense vector (zero for the padding columns)
__global__ __launch_bounds__(256) void k_wb_rhs(int ld, int k_old, int k_new, const int *__restrict__ rows, const int *__restrict__ arp,
                                                const int *__restrict__ aci, const double *__restrict__ aval, double *__restrict__ X) {
    double *col = X + (size_t)(k_old + blockIdx.x) * ld;
    for (int i = threadIdx.x; i < ld; i += blockDim.x) col[i] = 0.0;
    __syncthreads();
    if ((int)blockIdx.x >= k_new) return;
    const int r = rows[k_old + blockIdx.x];
    for (int e = arp[r] + threadIdx.x; e < arp[r + 1]; e += blockDim.x) col[aci[e]] = aval[e];
}
// G(a,b) = A(rows[a],:) Z(:,b) for the new columns b (and, by symmetry, the new rows)
__global__ __launch_bounds__(64) void k_wb_G(int k_old, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                             const double *__restrict__ aval, const double *__restrict__ Z, int ld, double *__restrict__ G) {
    const int a = blockIdx.x, b = k_old + blockIdx.y;
    if (a > b) return;
    const int r = rows[a];
    const double *zc = Z + (size_t)b * ld;
    double sacc = 0.0;
    for (int e = arp[r] + threadIdx.x; e < arp[r + 1]; e += 64) sacc += aval[e] * zc[aci[e]];
    sacc = wave_sum(sacc);
    if (threadIdx.x == 0) { G[a * WB_MAX + b] = sacc; G[b * WB_MAX + a] = sacc; }
}
// v_a = A(rows[a],:) z0,  w_a = d - d_fact at that row
__global__ __launch_bounds__(64) void k_wb_v(const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ aci,
                                             const double *__restrict__ aval, const double *__restrict__ z0, const double *__restrict__ dw,
                                             const double *__restrict__ dfact, double *__restrict__ v, double *__restrict__ w) {
    const int a = blockIdx.x, r = rows[a];
    double sacc = 0.0;
    for (int e = arp[r] + threadIdx.x; e < arp[r + 1]; e += 64) sacc += aval[e] * z0[aci[e]];
    sacc = wave_sum(sacc);
    if (threadIdx.x == 0) { v[a] = sacc; w[a] = dw[r] - dfact[r]; }
}
// t = (I + W G)^-1 W v by Gauss-Jordan elimination with partial pivoting: in LDS for k <= WB_LDS_MAX, in the global scratch
// Mg (L2-resident, ~0.5 MB) beyond; one workgroup, __syncthreads orders its global writes as well
__global__ __launch_bounds__(1024) void k_wb_lu(int k, const double *__restrict__ G, const double *__restrict__ w, const double *__restrict__ v,
                                                double *__restrict__ t, double *Mg) {
    extern __shared__ double smr[];
    const int S = k + 2;                                  // row stride: k columns + right-hand side (+1 keeps it even/odd mixed)
    double *M = k <= WB_LDS_MAX ? smr : Mg;
    __shared__ double red_v[16]; __shared__ int red_i[16]; __shared__ int piv_s; __shared__ double piv_inv, piv_min;
    const int tid = threadIdx.x;
    if (tid == 0) piv_min = 1.0;
    for (int e = tid; e < k * (k + 1); e += 1024) {
        const int a = e / (k + 1), b = e % (k + 1);
        M[a * S + b] = b < k ? ((a == b ? 1.0 : 0.0) + w[a] * G[a * WB_MAX + b]) : w[a] * v[a];
    }
    __syncthreads();
    for (int j = 0; j < k; j++) {
        // pivot: largest |M[r][j]|, r >= j (ties -> smallest r)
        double best = -1.0; int bi = j;
        for (int r = j + tid; r < k; r += 1024) { const double x = fabs(M[r * S + j]); if (x > best) { best = x; bi = r; } }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_down(best, off); const int oi = __shfl_down(bi, off);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            double bb = red_v[0]; int ii = red_i[0];
            for (int q = 1; q < 16; q++) if (red_v[q] > bb || (red_v[q] == bb && red_i[q] < ii)) { bb = red_v[q]; ii = red_i[q]; }
            piv_s = ii; piv_inv = 1.0 / M[ii * S + j];
            if (!(bb >= piv_min)) piv_min = bb;            // NaN-propagating minimum of |pivot|
        }
        __syncthreads();
        const int p = piv_s; const double pinv = piv_inv;
        if (p != j) for (int c = j + tid; c <= k; c += 1024) { const double x = M[j * S + c]; M[j * S + c] = M[p * S + c]; M[p * S + c] = x; }
        __syncthreads();
        // eliminate column j from every other row; columns j+1..k (k = right-hand side)
        const int ncol = k - j;                            // columns j+1 .. k
        for (int e = tid; e < k * ncol; e += 1024) {
            const int r = e / ncol, c = j + 1 + e % ncol;
            if (r != j) M[r * S + c] -= (M[r * S + j] * pinv) * M[j * S + c];
        }
        __syncthreads();
        for (int c = j + 1 + tid; c <= k; c += 1024) M[j * S + c] *= pinv;
        __syncthreads();
    }
    for (int a = tid; a < k; a += 1024) t[a] = M[a * S + k];
    if (tid == 0) t[WB_MAX] = piv_min;                     // M = I at k = 0 weight change: pivots near 1 mean a benign update
}
// dx = z0 - Z t
__global__ void k_wb_apply(int n, int ld, int k, const double *__restrict__ Z, const double *__restrict__ t, const double *__restrict__ z0,
                           double *__restrict__ dx) {
    __shared__ double ts[WB_MAX];
    for (int a = threadIdx.x; a < k; a += blockDim.x) ts[a] = t[a];
    __syncthreads();
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        double sacc = 0.0;
        for (int a = 0; a < k; a++) sacc += Z[(size_t)a * ld + j] * ts[a];
        dx[j] = z0[j] - sacc;
    }
}
// right-hand side padded to ld; s1, s2 (optional): the two polled vectors of the chained solves, filled with the sentinel
__global__ void k_dense_load_rhs(int n, int ld, const double *__restrict__ b, double *__restrict__ x, double *__restrict__ s1, double *__restrict__ s2) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += gridDim.x * blockDim.x) {
        x[i] = i < n ? b[i] : 0.0;
        if (s1) { reinterpret_cast<unsigned long long *>(s1)[i] = CH_SENT; reinterpret_cast<unsigned long long *>(s2)[i] = CH_SENT; }
    }
}
// k_dense_load_rhs for the columns of a group (blockIdx.y = column, ld apart in every array): b's column (ldb apart) padded to ld, the
// sentinels of the column's two polled vectors refilled
__global__ void k_dense_load_rhs_group(int n, int ld, const double *__restrict__ b, long long ldb, double *__restrict__ x, double *__restrict__ s1,
                                       double *__restrict__ s2) {
    const long long col = blockIdx.y;
    b += col * ldb; x += col * ld; s1 += col * ld; s2 += col * ld;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += gridDim.x * blockDim.x) {
        x[i] = i < n ? b[i] : 0.0;
        reinterpret_cast<unsigned long long *>(s1)[i] = CH_SENT; reinterpret_cast<unsigned long long *>(s2)[i] = CH_SENT;
    }
}
__global__ void k_dense_scale_d(int ld, const double *__restrict__ z, const double *__restrict__ Dg, double *__restrict__ y) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += gridDim.x * blockDim.x) y[i] = z[i] / Dg[i];
}

