// band_wide.inc -- part of qpdo_dev.hip (one translation unit; included in order): the band direct solver for half-bandwidths 128 .. 1023.
// ------------------------------------------------------------------------------------------------
// k_band_factor (dev/band.inc) keeps a window of b + 4 columns in LDS, which ends at b = 127.  Beyond that the band is held as 64 x 64 tiles
// and factored block column by block column on the fp64 matrix cores, with the dense path's device functions (diag64_lds_v2,
// mfma_64x64x32): np = n rounded up to 64, nbc = np / 64 block columns, w = (b + 63) / 64 tiles below the diagonal one (2 <= w <= 16).
//   Wb[(J (w+1) + s) 4096 + c 64 + r] = tile (J + s, J), element (r, c); rows and columns n .. np-1 are identity padding, tiles whose
//                                       block row is >= nbc are zero.  After the factorization: unit-lower L (diagonal tiles: 1 on the
//                                       diagonal, 0 above it).  An element outside the band (i - j > b) is an exact zero before and after.
//   Wdiag[J 4096 + c 64 + r]          = the diagonal tile (J, J) while it is still being updated: what launch k reads of block column k is
//                                       written by no workgroup of launch k (L_kk goes to Wb, its input stays here)
//   Wd[np] = D;  Li / LiT[J 4096 + c 64 + r] = (L_JJ^-1)[r][c] / [c][r], as the dense path keeps Linv / LinvT
// Right-looking, two launches per block column k, no workgroup waits for another inside a launch (no flags, no polling), no atomics on
// doubles, every sum in a fixed order:
//   k_bw_panel(k):  min(w, nbc-1-k) workgroups (at least one).  EACH eliminates the diagonal tile (redundantly: no hand-off);
//                   workgroup 0 writes L_kk, D, the inverses and latches a bad pivot (C_CHAIN_ERR bit 1, as k_band_factor does);
//                   workgroup s forms L_{k+s+1,k} = A_{k+s+1,k} L_kk^-T D^-1 (the product with the explicit inverse, as k_ldl_panel).
//   k_bw_update(k): tile (k+i, k+j) -= L_{k+i,k} D_k L_{k+j,k}', 1 <= j <= i <= min(w, nbc-1-k): one workgroup per tile (<= 136).
// A bad pivot leaves the later launches computing on garbage; nothing spins, the host sees the latch with the step.
// ------------------------------------------------------------------------------------------------
static const int BAND_WIDE_MAX_B = 1023;
static const int BW_MAX_W = (BAND_WIDE_MAX_B + 63) / 64;          // 16
static const int BW_T = DNB * DNB;                                 // doubles per tile

// assembly: one wave per column j, accumulator of 64 (w + 1) doubles in LDS (the column's part of its w + 1 tiles); k_band_assemble's
// per-element order -- Q first, then the weighted rows of A that touch column j in ascending order, sigma_f last -- so the tiles hold the
// very values the dense and the narrow-band matrices would.
// PERM: band_assemble_body's rule (dev/band.inc) -- column pj of the tiles is the caller's column newold[pj], the caller's row i lands in row
// oldnew[i]; PERM = false is the code without an order.
template <bool PERM>
__device__ __forceinline__ void bw_assemble_body(int n, int np, int b, int w, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                 const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                 const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                 const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                 double *__restrict__ Wb, double *__restrict__ Wdiag, const int *__restrict__ newold,
                                                 const int *__restrict__ oldnew, double (*acc_s)[DNB * (BW_MAX_W + 1)]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, len = DNB * (w + 1);
    double *acc = acc_s[wave];
    for (int pj = blockIdx.x * 4 + wave; pj < np; pj += gridDim.x * 4) {
        const int J = pj >> 6, c = pj & 63, r0 = J * DNB;           // acc[i - r0] = K(i, pj), r0 <= i < r0 + len (pj - r0 + b < len)
        double *tiles = Wb + (size_t)J * (w + 1) * BW_T + (size_t)c * DNB, *dcol = Wdiag + (size_t)J * BW_T + (size_t)c * DNB;
        for (int t = lane; t < len; t += 64) acc[t] = 0.0;
        __builtin_amdgcn_wave_barrier();
        if (pj < n) {
            const int j = PERM ? newold[pj] : pj;
            for (int k = qrp[j] + lane; k < qrp[j + 1]; k += 64) { const int i = PERM ? oldnew[qci[k]] : qci[k]; if (i >= pj && i - pj <= b) acc[i - r0] += qval[k]; }
            __builtin_amdgcn_wave_barrier();
            for (int t = trp[j]; t < trp[j + 1]; t++) {               // (uniform over the wave)
                const int r = tci[t];
                const double wgt = dw[r];
                if (wgt == 0.0) continue;
                const double vj = wgt * tval[t];
                for (int e = arp[r] + lane; e < arp[r + 1]; e += 64) { const int i = PERM ? oldnew[aci[e]] : aci[e]; if (i >= pj && i - pj <= b) acc[i - r0] += vj * aval[e]; }
                __builtin_amdgcn_wave_barrier();                      // one wave: its LDS operations are served in order
            }
            if (lane == 0) acc[c] += sigma_f;
        } else if (lane == 0) acc[c] = 1.0;                           // identity padding
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < len; t += 64) {
            const int i = r0 + t;
            const double v = (i >= pj && i - pj <= b && (i < n || i == pj)) ? acc[t] : 0.0;
            if (t < DNB) { dcol[t] = v; tiles[t] = 0.0; }
            else tiles[(size_t)(t >> 6) * BW_T + (t & 63)] = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
}
__global__ __launch_bounds__(256) void k_bw_assemble(int n, int np, int b, int w, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                    const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                    const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                    const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                    double *__restrict__ Wb, double *__restrict__ Wdiag) {
    __shared__ double acc_s[4][DNB * (BW_MAX_W + 1)];
    bw_assemble_body<false>(n, np, b, w, qrp, qci, qval, trp, tci, tval, arp, aci, aval, dw, sigma_f, Wb, Wdiag, nullptr, nullptr, acc_s);
}
__global__ __launch_bounds__(256) void k_bw_assemble_perm(int n, int np, int b, int w, const int *__restrict__ qrp, const int *__restrict__ qci,
                                                         const double *__restrict__ qval, const int *__restrict__ trp, const int *__restrict__ tci,
                                                         const double *__restrict__ tval, const int *__restrict__ arp, const int *__restrict__ aci,
                                                         const double *__restrict__ aval, const double *__restrict__ dw, double sigma_f,
                                                         double *__restrict__ Wb, double *__restrict__ Wdiag, const int *__restrict__ newold,
                                                         const int *__restrict__ oldnew) {
    __shared__ double acc_s[4][DNB * (BW_MAX_W + 1)];
    bw_assemble_body<true>(n, np, b, w, qrp, qci, qval, trp, tci, tval, arp, aci, aval, dw, sigma_f, Wb, Wdiag, newold, oldnew, acc_s);
}
// S: DG_LDS doubles for the elimination of the diagonal tile + the two [32][80] operand images of the panel product (reused as the
// [col][row] image of the result)
static const int BW_PANEL_LDS = DG_LDS + 2 * 32 * 80;                // doubles
__global__ __launch_bounds__(256) void k_bw_panel(int k, int w, int nbc, double *__restrict__ Wb, const double *__restrict__ Wdiag,
                                                  double *__restrict__ Wd, double *__restrict__ Li, double *__restrict__ LiT, int *__restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double bw_lds[];
    double *T = bw_lds, *Ic = T + DNB * DG_TS, *Xs = Ic + 10 * 256 + 64, *P = bw_lds + DG_LDS;
    double (*As)[80] = reinterpret_cast<double (*)[80]>(P);
    double (*Bs)[80] = reinterpret_cast<double (*)[80]>(P + 32 * 80);
    const int tid = threadIdx.x, lr = tid & 63, c0 = tid >> 6, s = blockIdx.x + 1;
    const bool has_tile = k + s < nbc;                                 // (false only for the lone workgroup of the last block column)
    double *tile = Wb + ((size_t)k * (w + 1) + s) * BW_T;
    // this workgroup's tile of the panel: in flight during the elimination (element (lr, c0 + 4 e))
    double a[DNB / 4];
    if (has_tile) {
#pragma unroll
        for (int e = 0; e < DNB / 4; e++) a[e] = tile[(size_t)(c0 + 4 * e) * DNB + lr];
    }
    const double *dt = Wdiag + (size_t)k * BW_T;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) { const int c = c0 + 4 * e; T[lr * DG_TS + c] = dt[(size_t)c * DNB + lr]; }
    __syncthreads();
    diag64_lds_v2(T, Ic, Xs, tid);
    if (blockIdx.x == 0) {
        double *o0 = Wb + (size_t)k * (w + 1) * BW_T, *o1 = Li + (size_t)k * BW_T, *o2 = LiT + (size_t)k * BW_T;
#pragma unroll 4
        for (int e = 0; e < DNB / 4; e++) {
            const int c = c0 + 4 * e;
            o0[(size_t)c * DNB + lr] = lr > c ? T[lr * DG_TS + c] : (lr == c ? 1.0 : 0.0);
            o1[(size_t)c * DNB + lr] = diag64_inv(Ic, lr, c);
            o2[(size_t)c * DNB + lr] = diag64_inv(Ic, c, lr);
        }
        if (tid < DNB) {
            const double dd = T[tid * DG_TS + tid];
            Wd[(size_t)k * DNB + tid] = dd;
            if (!(dd > 0.0 && dd < 1e300)) atomicOr(err, 2);           // (C_CHAIN_ERR, bit 1: the host reads the latch with the step)
        }
    }
    if (!has_tile) return;
    // X = A L_kk^-T on the matrix cores, two 32-deep halves of k through the same images: As[k][row] = A(row, k), Bs[k][col] = (L^-1)(col, k)
    const int wave = tid >> 6, l = tid & 63, wr = (wave >> 1) * 32, wc = (wave & 1) * 32, li = l & 15, lk = l >> 4;
    dvec4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc[m][q] = (dvec4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h) __syncthreads();                                        // the first half product is done with the images
#pragma unroll
        for (int e8 = 0; e8 < 8; e8++) {
            const int e = 8 * h + e8, kk = c0 + 4 * e, kh = kk - 32 * h;
            As[kh][lr] = a[e];
            Bs[kh][lr] = diag64_inv(Ic, lr, kk);
        }
        __syncthreads();
        mfma_64x64x32(As, Bs, acc, wr, wc, li, lk);
    }
    __syncthreads();
    // L = X / D through a [col][row] image (row stride 65), written along the contiguous rows of the tile
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int v = 0; v < 4; v++) P[(wc + q * 16 + li) * (DNB + 1) + wr + m * 16 + lk + 4 * v] = acc[m][q][v];
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int c = c0 + 4 * e;
        tile[(size_t)c * DNB + lr] = P[c * (DNB + 1) + lr] / T[c * DG_TS + c];
    }
}
// S: the [k][row] images of L_{k+i,k} D_k and of L_{k+j,k} ([64][80] each); the first is reused as the [col][row] image of the product
static const int BW_UPDATE_LDS = 2 * 64 * 80;                         // doubles
__global__ __launch_bounds__(256) void k_bw_update(int k, int w, double *__restrict__ Wb, double *__restrict__ Wdiag, const double *__restrict__ Wd) {
    extern __shared__ __attribute__((aligned(16))) double bw_lds[];
    double (*Ah)[80] = reinterpret_cast<double (*)[80]>(bw_lds);
    double (*Bh)[80] = reinterpret_cast<double (*)[80]>(bw_lds + 64 * 80);
    // blockIdx.x = i (i - 1) / 2 + (j - 1), 1 <= j <= i
    int i = 1;
    while (i * (i + 1) / 2 <= (int)blockIdx.x) i++;
    const int j = (int)blockIdx.x - i * (i - 1) / 2 + 1;
    const int tid = threadIdx.x, lr = tid & 63, c0 = tid >> 6;
    const double *Lik = Wb + ((size_t)k * (w + 1) + i) * BW_T, *Ljk = Wb + ((size_t)k * (w + 1) + j) * BW_T, *dk = Wd + (size_t)k * DNB;
    double *C = (i == j) ? Wdiag + (size_t)(k + j) * BW_T : Wb + ((size_t)(k + j) * (w + 1) + (i - j)) * BW_T;
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int kk = c0 + 4 * e;
        Ah[kk][lr] = Lik[(size_t)kk * DNB + lr] * dk[kk];
        Bh[kk][lr] = Ljk[(size_t)kk * DNB + lr];
    }
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, wr = (wave >> 1) * 32, wc = (wave & 1) * 32, li = l & 15, lk = l >> 4;
    dvec4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++) acc[m][q] = (dvec4){0.0, 0.0, 0.0, 0.0};
    mfma_64x64x32(Ah, Bh, acc, wr, wc, li, lk);
    mfma_64x64x32(Ah + 32, Bh + 32, acc, wr, wc, li, lk);
    __syncthreads();
    double *P = bw_lds;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int v = 0; v < 4; v++) P[(wc + q * 16 + li) * (DNB + 1) + wr + m * 16 + lk + 4 * v] = acc[m][q][v];
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < DNB / 4; e++) {
        const int c = c0 + 4 * e;
        double *cp = C + (size_t)c * DNB + lr;
        *cp = *cp - P[c * (DNB + 1) + lr];
    }
}
// Both triangular solves and the diagonal scaling, one workgroup.  Left-looking over the block columns: t_J = r_J - sum_s L_{J,J-s} z_{J-s}
// (the last w results sit in an LDS window), z_J = L_JJ^-1 t_J with the stored inverse, out = z_J / D; the backward sweep mirrors it with
// the tiles of block column J read along their columns and LiT.  Which tiles a step reads does not depend on the chain, so every wave
// loads its next tile (64 doubles per lane) while it multiplies the current one -- across the steps' barriers too -- and the inverse and
// the right-hand side of step J + 1 are loaded during step J.  Wave v takes the tiles s = v + 1, v + 5, ...; partial sums are added in a
// fixed order.
// PERM (a variable order): the forward sweep's `in` and the backward sweep's `out` are in the caller's order, entry i of the solver's order at
// perm[i] (band_solve_body's rule, dev/band.inc)
template <bool FWD, bool PERM>
__device__ __forceinline__ void bw_sweep(int nbc, int w, const double *__restrict__ Wb, const double *__restrict__ inv, const double *__restrict__ Wd,
                                         const double *__restrict__ in, int nin, double *__restrict__ out, int nout, double (*win)[DNB],
                                         double (*part)[DNB], double (*part2)[DNB], double *tot, const int *__restrict__ perm) {
    const int tid = threadIdx.x, v = tid >> 6, l = tid & 63;
    auto lim = [&](int J) { const int r = FWD ? J : nbc - 1 - J; return r < w ? r : w; };
    auto tile_of = [&](int J, int s) { return FWD ? Wb + ((size_t)(J - s) * (w + 1) + s) * BW_T : Wb + ((size_t)J * (w + 1) + s) * BW_T; };
    double cur[DNB], nxt[DNB], li[16], li_n[16];
    auto load_tile = [&](double (&buf)[DNB], int J, int s) {
        if (J < 0 || J >= nbc || s > lim(J)) return;
        const double *t = tile_of(J, s);
        if (FWD) {
#pragma unroll
            for (int c = 0; c < DNB; c++) buf[c] = t[(size_t)c * DNB + l];          // row l of the tile
        } else {
#pragma unroll
            for (int r = 0; r < DNB; r++) buf[r] = t[(size_t)l * DNB + r];          // column l of the tile
        }
    };
    auto load_inv = [&](double (&buf)[16], int J) {
        if (J < 0 || J >= nbc) return;
#pragma unroll
        for (int q = 0; q < 16; q++) buf[q] = inv[(size_t)J * BW_T + (size_t)(v * 16 + q) * DNB + l];
    };
    const int J0 = FWD ? 0 : nbc - 1, dJ = FWD ? 1 : -1;
    load_tile(cur, J0, v + 1);
    load_inv(li, J0);
    double rin = (J0 * DNB + l < nin) ? in[(PERM && FWD) ? (size_t)perm[J0 * DNB + l] : (size_t)J0 * DNB + l] : 0.0;
    for (int J = J0; J >= 0 && J < nbc; J += dJ) {
        const int Jn = J + dJ;
        load_inv(li_n, Jn);
        const double rin_n = (Jn >= 0 && Jn * DNB + l < nin) ? in[(PERM && FWD) ? (size_t)perm[Jn * DNB + l] : (size_t)Jn * DNB + l] : 0.0;
        const double dd = FWD ? Wd[(size_t)J * DNB + l] : 1.0;
        double acc = 0.0;
        for (int s = v + 1;; s += 4) {
            const bool last = s + 4 > lim(J);
            if (last) load_tile(nxt, Jn, v + 1); else load_tile(nxt, J, s + 4);
            if (s <= lim(J)) {
                const double *zz = win[(FWD ? J - s : J + s) % (BW_MAX_W + 1)];
#pragma unroll
                for (int c = 0; c < DNB; c++) acc += cur[c] * zz[c];
            }
#pragma unroll
            for (int c = 0; c < DNB; c++) cur[c] = nxt[c];
            if (last) break;
        }
        part[v][l] = acc;
        __syncthreads();
        if (v == 0) tot[l] = rin - ((part[0][l] + part[1][l]) + (part[2][l] + part[3][l]));
        __syncthreads();
        double sacc = 0.0;
#pragma unroll
        for (int q = 0; q < 16; q++) sacc += li[q] * tot[v * 16 + q];
        part2[v][l] = sacc;
        __syncthreads();
        if (v == 0) {
            const double z = (part2[0][l] + part2[1][l]) + (part2[2][l] + part2[3][l]);
            win[J % (BW_MAX_W + 1)][l] = z;
            if (J * DNB + l < nout) out[(PERM && !FWD) ? (size_t)perm[J * DNB + l] : (size_t)J * DNB + l] = FWD ? z / dd : z;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) li[q] = li_n[q];
        rin = rin_n;
    }
}
// rhs and x hold n entries, z np
__global__ __launch_bounds__(256) void k_bw_solve(int n, int nbc, int w, const double *__restrict__ Wb, const double *__restrict__ Li,
                                                  const double *__restrict__ LiT, const double *__restrict__ Wd, const double *__restrict__ rhs,
                                                  double *__restrict__ z, double *__restrict__ x) {
    __shared__ double win[BW_MAX_W + 1][DNB], part[4][DNB], part2[4][DNB], tot[DNB];
    bw_sweep<true, false>(nbc, w, Wb, Li, Wd, rhs, n, z, nbc * DNB, win, part, part2, tot, nullptr);
    __threadfence_block();
    __syncthreads();
    bw_sweep<false, false>(nbc, w, Wb, LiT, Wd, z, nbc * DNB, x, n, win, part, part2, tot, nullptr);
}
// the same under a variable order: rhs and x in the caller's order, perm = newold
__global__ __launch_bounds__(256) void k_bw_solve_perm(int n, int nbc, int w, const double *__restrict__ Wb, const double *__restrict__ Li,
                                                       const double *__restrict__ LiT, const double *__restrict__ Wd, const double *__restrict__ rhs,
                                                       double *__restrict__ z, double *__restrict__ x, const int *__restrict__ perm) {
    __shared__ double win[BW_MAX_W + 1][DNB], part[4][DNB], part2[4][DNB], tot[DNB];
    bw_sweep<true, true>(nbc, w, Wb, Li, Wd, rhs, n, z, nbc * DNB, win, part, part2, tot, perm);
    __threadfence_block();
    __syncthreads();
    bw_sweep<false, true>(nbc, w, Wb, LiT, Wd, z, nbc * DNB, x, n, win, part, part2, tot, perm);
}
// the group path's solve (dev/adjoint.inc adj_sweeps_group): one workgroup per live right-hand side, each running k_bw_solve's two sweeps on
// columns of its own (rhs and x: ldx apart, z: np = 64 nbc apart) -- to k_bw_solve what k_band_solve_group is to k_band_solve.  Per column
// it is the single kernel's code.  (No kernel that loads a tile once for all columns: the chain is latency bound, DESIGN.md 3.7.1.)
__global__ __launch_bounds__(256) void k_bw_solve_group(int n, int nbc, int w, const double *__restrict__ Wb, const double *__restrict__ Li,
                                                        const double *__restrict__ LiT, const double *__restrict__ Wd, const double *rhs, long long ldx,
                                                        double *z, double *x) {
    __shared__ double win[BW_MAX_W + 1][DNB], part[4][DNB], part2[4][DNB], tot[DNB];
    const long long s = blockIdx.x, np = (long long)nbc * DNB;
    bw_sweep<true, false>(nbc, w, Wb, Li, Wd, rhs + s * ldx, n, z + s * np, nbc * DNB, win, part, part2, tot, nullptr);
    __threadfence_block();
    __syncthreads();
    bw_sweep<false, false>(nbc, w, Wb, LiT, Wd, z + s * np, nbc * DNB, x + s * ldx, n, win, part, part2, tot, nullptr);
}
__global__ __launch_bounds__(256) void k_bw_solve_group_perm(int n, int nbc, int w, const double *__restrict__ Wb, const double *__restrict__ Li,
                                                             const double *__restrict__ LiT, const double *__restrict__ Wd, const double *rhs, long long ldx,
                                                             double *z, double *x, const int *__restrict__ perm) {
    __shared__ double win[BW_MAX_W + 1][DNB], part[4][DNB], part2[4][DNB], tot[DNB];
    const long long s = blockIdx.x, np = (long long)nbc * DNB;
    bw_sweep<true, true>(nbc, w, Wb, Li, Wd, rhs + s * ldx, n, z + s * np, nbc * DNB, win, part, part2, tot, perm);
    __threadfence_block();
    __syncthreads();
    bw_sweep<false, true>(nbc, w, Wb, LiT, Wd, z + s * np, nbc * DNB, x + s * ldx, n, win, part, part2, tot, perm);
}
