// adjoint.inc -- part of qpdo_dev.hip (one translation unit; included in order): qpdo_amd_adjoint -- the gradients of a workspace's solution
// w.r.t. q, l, u, Q, A (include/qpdo_amd_ext.h; DESIGN.md 3.7).  The method is the fleet's (qpdo_small.hip k_small_fleet_adjoint), device
// wide: at the x, y the solve delivered the rows are classified (t = Ax + y against the bounds), and
//   [ Q  A_S' ; A_S  0 ] [vx ; vy] = [gx ; gy_S]
// is solved in the workspace's SCALED space -- Qs = c D Q D, As = E A D, vxs = D^-1 vx, vys = c E^-1 vy, gxs = c D gx, gys = E gy: the same
// system in the stored matrices -- by block elimination on the regularised matrix:
//   K dvx = rx + As_S' W ry,   dvy = W (As_S dvx - ry),   K = Qs + sigma I + As_S' W As_S,
// repeated on the residual (rx, ry) of the TRUE system.  K is the Newton matrix with weights W on the flagged rows: it is factored ONCE per
// call by the workspace's own direct solver (dense_factor / band_factor) and solved by dense_solve / band_solve; the products are the
// workspace's SpMV.  The kernels here are streams over n, m or nnz.  Every reduction is a maximum or an integer count (exact and order
// free on the control block, helpers.inc block_max_to), so two calls on one solve deliver the same bits.
#define ADJ_SIGMA_REL 1e-10
#define ADJ_ROW_WEIGHT 1e10
#define ADJ_DBL_MAX 1.7976931348623157e308
static const int ADJ_LPR = 16;                    // lanes per matrix row in the row-wise kernels (rows of A, A', Q: tens of entries)
enum { ADJ_N_XU = 0, ADJ_N_GXS, ADJ_N_VX, ADJ_N_RX, ADJ_N_T1, ADJ_N_T2, ADJ_N_COUNT };
enum { ADJ_M_YU = 0, ADJ_M_GYS, ADJ_M_VY, ADJ_M_RY, ADJ_M_WRY, ADJ_M_AV, ADJ_M_A2, ADJ_M_COUNT };

__device__ __forceinline__ double adj_abs(double v) { return v < 0 ? -v : v; }
static inline int adj_grid_rows(long long nrows) { return vgrid(nrows * ADJ_LPR); }

// zero the slots a right-hand side uses: N_A = ||gx||, N_B = ||gy_S||, N_C / N_D = the sweep's two residual norms, C_VIOL = the
// non-finite marker (all: a new right-hand side; else: the two residual norms of the next sweep)
__global__ void k_adj_ctrl_clear(Ctrl *c, int all) {
    const int t = threadIdx.x;
    if (blockIdx.x) return;
    if (t == 0) c->nrm[N_C] = 0ull;
    if (t == 1) c->nrm[N_D] = 0ull;
    if (all && t == 2) c->nrm[N_A] = 0ull;
    if (all && t == 3) c->nrm[N_B] = 0ull;
    if (all && t == 4) c->cnt[C_VIOL] = 0;
}
// once per call, n side: xs = D^-1 x; the largest |diagonal entry| of Qs into N_C (from qdiag when the workspace holds it)
__global__ void k_adj_scale_x(int n, int scaled, const double *__restrict__ Dinv, const double *__restrict__ xu, const double *__restrict__ qdiag,
                              const int *__restrict__ Qrp, const int *__restrict__ Qci, const double *__restrict__ Qval, double *__restrict__ xs, Ctrl *ctrl) {
    __shared__ double sm[32];
    double mqd = 0.0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        xs[j] = scaled ? xu[j] * Dinv[j] : xu[j];
        if (qdiag) { const double a = adj_abs(qdiag[j]); mqd = a > mqd ? a : mqd; }
        else for (int k = Qrp[j]; k < Qrp[j + 1]; k++) if (Qci[k] == j) { const double a = adj_abs(Qval[k]); mqd = a > mqd ? a : mqd; }
    }
    block_max_to(mqd, &ctrl->nrm[N_C], sm);
}
// once per call, m side (Av = As xs is there): the flags from t = Axs + E y against the stored (scaled) bounds, the rows' squared norms,
// the number of flagged rows into C_MUCH.  ADJ_LPR lanes per row; the lanes' partial sums are folded in a fixed order.
__global__ void k_adj_classify(int m, int scaled, const double *__restrict__ E, const double *__restrict__ yu, const double *__restrict__ l,
                               const double *__restrict__ u, const double *__restrict__ Av, const int *__restrict__ Arp, const double *__restrict__ Aval,
                               int *__restrict__ flag, double *__restrict__ a2out, Ctrl *ctrl) {
    __shared__ int smi[32];
    const int lane = threadIdx.x & (ADJ_LPR - 1);
    const int groups = gridDim.x * (blockDim.x / ADJ_LPR);
    int cnt = 0;
    const int rounds = (m + groups - 1) / groups;          // (every lane takes part in every shuffle)
    for (int it = 0; it < rounds; it++) {
        const int i = it * groups + blockIdx.x * (blockDim.x / ADJ_LPR) + (threadIdx.x / ADJ_LPR);
        double a2 = 0.0;
        if (i < m) for (int k = Arp[i] + lane; k < Arp[i + 1]; k += ADJ_LPR) { const double a = Aval[k]; a2 += a * a; }
#pragma unroll
        for (int o = ADJ_LPR / 2; o > 0; o >>= 1) a2 += __shfl_down(a2, o, ADJ_LPR);
        if (i < m && lane == 0) {
            const double e = scaled ? E[i] : 1.0, yi = yu[i];
            const double t = Av[i] + (scaled ? e * yi : yi);
            const double lo = l[i], up = u[i];
            int f = 0;
            if (up < e * QPDO_INFTY_D && t >= up) f = 1;
            else if (lo > -e * QPDO_INFTY_D && t <= lo) f = -1;
            flag[i] = f; cnt += (f != 0);
            a2out[i] = a2;
        }
    }
    const int tot = block_sum_int(cnt, smi);
    if (threadIdx.x == 0 && tot) atomicAdd(&ctrl->cnt[C_MUCH], tot);
}
// once per call, after s is known: the factorization's weights d_i = W_i = 1e10 s / ||row i of As||^2 on flagged rows, 0 elsewhere
__global__ void k_adj_weights(int m, double s, const int *__restrict__ flag, const double *__restrict__ a2, double *__restrict__ W) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const double v = a2[i];
        W[i] = (flag[i] && v > 0.0) ? (ADJ_ROW_WEIGHT * s) / v : 0.0;
    }
}
// dense route: the pivots of the fresh factor; one that is not a positive finite number sets C_DINF
__global__ void k_adj_check_pivots(int n, const double *__restrict__ Dg, Ctrl *ctrl) {
    int bad = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) { const double dj = Dg[j]; bad |= !(dj > 0.0 && dj <= ADJ_DBL_MAX); }
    if (bad) ctrl->cnt[C_DINF] = 1;
}
// ---- the four vector kernels of the sweep loop: ONE body each, run by the single call's kernel on the control block's slots and by the
// group's kernel (grid.y = the right-hand side, vectors a fixed stride apart, masked by `live`) on that right-hand side's slots of the
// group control array -- the same expressions in the same order for both.
// per right-hand side: gxs = c D gx, gys = E gy on flagged rows (0 elsewhere: gy of an inactive row is never read), vx = vy = 0,
// ||gx||inf -> nA, ||gy_S||inf -> nB, a non-finite entry among those used -> viol
__device__ __forceinline__ void adj_rhs_body(int n, int m, int scaled, double c, const double *__restrict__ D, const double *__restrict__ E,
                                             const double *__restrict__ gx, const double *__restrict__ gy, const int *__restrict__ flag, double *__restrict__ gxs,
                                             double *__restrict__ gys, double *__restrict__ vx, double *__restrict__ vy, u64 *nA, u64 *nB, int *viol, double *sm) {
    double mgx = 0.0, mgy = 0.0; int nonfin = 0;
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int j = t0; j < n; j += stride) {
        const double g = gx[j];
        gxs[j] = scaled ? c * (D[j] * g) : g;
        vx[j] = 0.0;
        const double ag = adj_abs(g);
        mgx = ag > mgx ? ag : mgx;
        if (!(ag <= ADJ_DBL_MAX)) nonfin = 1;
    }
    for (int i = t0; i < m; i += stride) {
        double g = 0.0;
        if (flag[i] && gy) { g = gy[i]; const double ag = adj_abs(g); mgy = ag > mgy ? ag : mgy; if (!(ag <= ADJ_DBL_MAX)) nonfin = 1; }
        gys[i] = scaled ? E[i] * g : g;
        vy[i] = 0.0;
    }
    block_max_to(mgx, nA, sm);
    block_max_to(mgy, nB, sm + 16);
    if (nonfin) *viol = 1;
}
__global__ void k_adj_rhs(int n, int m, int scaled, double c, const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ gx,
                          const double *__restrict__ gy, const int *__restrict__ flag, double *__restrict__ gxs, double *__restrict__ gys, double *__restrict__ vx,
                          double *__restrict__ vy, Ctrl *ctrl) {
    __shared__ double sm[32];
    adj_rhs_body(n, m, scaled, c, D, E, gx, gy, flag, gxs, gys, vx, vy, &ctrl->nrm[N_A], &ctrl->nrm[N_B], &ctrl->cnt[C_VIOL], sm);
}
__global__ void k_adj_rhs_group(int n, int m, int scaled, double c, const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ gx,
                                const double *__restrict__ gy, const int *__restrict__ flag, double *__restrict__ gxs, double *__restrict__ gys, double *__restrict__ vx,
                                double *__restrict__ vy, unsigned live, AdjGrpCtrl *gc) {
    __shared__ double sm[32];
    const size_t g = blockIdx.y;
    if (!((live >> g) & 1u)) return;
    adj_rhs_body(n, m, scaled, c, D, E, gx + g * n, gy ? gy + g * m : nullptr, flag, gxs + g * n, gys + g * m, vx + g * n, vy + g * m, &gc[g].nrm[0], &gc[g].nrm[1],
                 &gc[g].nonfin, sm);
}
// per sweep, behind t1 = Qs vx, Av = As vx, t2 = As' vy: rx = (gxs - t1) - t2, ry = gys - Av on flagged rows, wry = W ry; the two
// inf-norms in unscaled terms (||rx D^-1|| -> nC, the host multiplies by 1 / c; ||ry E^-1|| -> nD); a non-finite one -> viol
__device__ __forceinline__ void adj_resid_body(int n, int m, int scaled, const double *__restrict__ Dinv, const double *__restrict__ Einv,
                                               const double *__restrict__ gxs, const double *__restrict__ t1, const double *__restrict__ t2,
                                               const double *__restrict__ gys, const double *__restrict__ Av, const int *__restrict__ flag,
                                               const double *__restrict__ W, double *__restrict__ rx, double *__restrict__ ry, double *__restrict__ wry, u64 *nC,
                                               u64 *nD, int *viol, double *sm) {
    double m1 = 0.0, m2 = 0.0; int nonfin = 0;
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int j = t0; j < n; j += stride) {
        const double r = (gxs[j] - t1[j]) - t2[j];
        rx[j] = r;
        const double a = adj_abs(scaled ? r * Dinv[j] : r);
        m1 = a > m1 ? a : m1;
        if (!(a <= ADJ_DBL_MAX)) nonfin = 1;
    }
    for (int i = t0; i < m; i += stride) {
        const double r = flag[i] ? gys[i] - Av[i] : 0.0;
        ry[i] = r; wry[i] = W[i] * r;
        const double a = adj_abs(scaled ? r * Einv[i] : r);
        m2 = a > m2 ? a : m2;
        if (!(a <= ADJ_DBL_MAX)) nonfin = 1;
    }
    block_max_to(m1, nC, sm);
    block_max_to(m2, nD, sm + 16);
    if (nonfin) *viol = 1;
}
__global__ void k_adj_resid(int n, int m, int scaled, const double *__restrict__ Dinv, const double *__restrict__ Einv, const double *__restrict__ gxs,
                            const double *__restrict__ t1, const double *__restrict__ t2, const double *__restrict__ gys, const double *__restrict__ Av,
                            const int *__restrict__ flag, const double *__restrict__ W, double *__restrict__ rx, double *__restrict__ ry,
                            double *__restrict__ wry, Ctrl *ctrl) {
    __shared__ double sm[32];
    adj_resid_body(n, m, scaled, Dinv, Einv, gxs, t1, t2, gys, Av, flag, W, rx, ry, wry, &ctrl->nrm[N_C], &ctrl->nrm[N_D], &ctrl->cnt[C_VIOL], sm);
}
__global__ void k_adj_resid_group(int n, int m, int scaled, const double *__restrict__ Dinv, const double *__restrict__ Einv, const double *__restrict__ gxs,
                                  const double *__restrict__ t1, const double *__restrict__ t2, const double *__restrict__ gys, const double *__restrict__ Av,
                                  const int *__restrict__ flag, const double *__restrict__ W, double *__restrict__ rx, double *__restrict__ ry,
                                  double *__restrict__ wry, unsigned live, AdjGrpCtrl *gc) {
    __shared__ double sm[32];
    const size_t g = blockIdx.y;
    if (!((live >> g) & 1u)) return;
    adj_resid_body(n, m, scaled, Dinv, Einv, gxs + g * n, t1 + g * n, t2 + g * n, gys + g * m, Av + g * m, flag, W, rx + g * n, ry + g * m, wry + g * m,
                   &gc[g].nrm[2], &gc[g].nrm[3], &gc[g].nonfin, sm);
}
// the solve's right-hand side: rhs = rx + As' wry (t2 holds the product)
__device__ __forceinline__ void adj_solve_rhs_body(int n, const double *__restrict__ rx, const double *__restrict__ t2, double *__restrict__ rhs) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) rhs[j] = rx[j] + t2[j];
}
__global__ void k_adj_solve_rhs(int n, const double *__restrict__ rx, const double *__restrict__ t2, double *__restrict__ rhs) { adj_solve_rhs_body(n, rx, t2, rhs); }
// (the group's right-hand sides are COMPACT: that of live vector g is column slot(g) = the number of live vectors below g)
__device__ __forceinline__ size_t adj_slot(unsigned live, size_t g) { return (size_t)__popc(live & ((1u << g) - 1u)); }
__global__ void k_adj_solve_rhs_group(int n, const double *__restrict__ rx, const double *__restrict__ t2, double *__restrict__ rhs, unsigned live) {
    const size_t g = blockIdx.y;
    if (!((live >> g) & 1u)) return;
    adj_solve_rhs_body(n, rx + g * n, t2 + g * n, rhs + adj_slot(live, g) * n);
}
// behind Av = As dvx: vy += W (Av - ry), vx += dvx
__device__ __forceinline__ void adj_update_body(int n, int m, const double *__restrict__ dvx, const double *__restrict__ Av, const double *__restrict__ ry,
                                                const double *__restrict__ W, double *__restrict__ vx, double *__restrict__ vy) {
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = t0; i < m; i += stride) vy[i] = vy[i] + W[i] * (Av[i] - ry[i]);
    for (int j = t0; j < n; j += stride) vx[j] = vx[j] + dvx[j];
}
__global__ void k_adj_update(int n, int m, const double *__restrict__ dvx, const double *__restrict__ Av, const double *__restrict__ ry,
                             const double *__restrict__ W, double *__restrict__ vx, double *__restrict__ vy) {
    adj_update_body(n, m, dvx, Av, ry, W, vx, vy);
}
// (dvx: the solve's columns, compact and ldx apart)
__global__ void k_adj_update_group(int n, int m, const double *__restrict__ dvx, long long ldx, const double *__restrict__ Av, const double *__restrict__ ry,
                                   const double *__restrict__ W, double *__restrict__ vx, double *__restrict__ vy, unsigned live) {
    const size_t g = blockIdx.y;
    if (!((live >> g) & 1u)) return;
    adj_update_body(n, m, dvx + adj_slot(live, g) * (size_t)ldx, Av + g * m, ry + g * m, W, vx + g * n, vy + g * m);
}
// the group control array: all = 1 zeroes every slot of every right-hand side (a new group), else the two residual norms of the next sweep
__global__ void k_adj_grp_clear(AdjGrpCtrl *gc, int G, int all) {
    const int g = threadIdx.x >> 3, t = threadIdx.x & 7;
    if (blockIdx.x || g >= G) return;
    if (t == 2 || t == 3) gc[g].nrm[t] = 0ull;
    if (all && t < 2) gc[g].nrm[t] = 0ull;
    if (all && t == 4) gc[g].nonfin = 0;
}
// the read-back of a group's sweep: k_ctrl_publish with the group control array written to ITS pinned copy before the sequence word
__global__ __launch_bounds__(128) void k_adj_grp_publish(const Ctrl *__restrict__ c, Ctrl *host, const AdjGrpCtrl *__restrict__ gc, AdjGrpCtrl *hgc, int G, u64 *hseq,
                                                         u64 seq) {
    const u64 *src = (const u64 *)c; u64 *dst = (u64 *)host;
    const u64 *gsrc = (const u64 *)gc; u64 *gdst = (u64 *)hgc;
    const int t = threadIdx.x;
    if (t < (int)(sizeof(Ctrl) / 8)) dst[t] = src[t];
    else if (t >= 64 && t - 64 < G * (int)(sizeof(AdjGrpCtrl) / 8)) gdst[t - 64] = gsrc[t - 64];
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(hseq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// back to the caller's space: vx = D vxs, vy = E vys / c; dq = -vx, du = vy on +1 rows, dl = vy on -1 rows, every other entry +0.0
__global__ void k_adj_grad_vec(int n, int m, int scaled, double cinv, const double *__restrict__ D, const double *__restrict__ E, const int *__restrict__ flag,
                               const double *__restrict__ vx, const double *__restrict__ vy, double *__restrict__ vxu, double *__restrict__ vyu,
                               double *__restrict__ dq, double *__restrict__ dl, double *__restrict__ du) {
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int j = t0; j < n; j += stride) { const double v = scaled ? D[j] * vx[j] : vx[j]; vxu[j] = v; dq[j] = -v; }
    for (int i = t0; i < m; i += stride) {
        const int f = flag[i];
        double v = 0.0;
        if (f) { v = vy[i]; if (scaled) { v = E[i] * v; v = v * cinv; } }
        vyu[i] = v;
        du[i] = f > 0 ? v : 0.0; dl[i] = f < 0 ? v : 0.0;
    }
}
// dL/dA over the rows of CSR(A') (= the caller's CSC arrays of A, so entry k is the caller's entry k): -(y_i vx_j + vy_i x_j) on a flagged
// row i, +0.0 elsewhere
__global__ void k_adj_grad_A(int n, const int *__restrict__ Trp, const int *__restrict__ Tci, const int *__restrict__ flag, const double *__restrict__ xu,
                             const double *__restrict__ yu, const double *__restrict__ vxu, const double *__restrict__ vyu, double *__restrict__ dA) {
    const int lane = threadIdx.x & (ADJ_LPR - 1);
    const int groups = gridDim.x * (blockDim.x / ADJ_LPR);
    for (int j = blockIdx.x * (blockDim.x / ADJ_LPR) + (threadIdx.x / ADJ_LPR); j < n; j += groups) {
        const double vxj = vxu[j], xj = xu[j];
        for (int k = Trp[j] + lane; k < Trp[j + 1]; k += ADJ_LPR) { const int i = Tci[k]; dA[k] = flag[i] ? -(yu[i] * vxj + vyu[i] * xj) : 0.0; }
    }
}
// dL/dQ over the rows of the full CSR(Q).  mapQ == null (stype 0): entry k of row r IS the caller's entry k, row cc of column r.
// Otherwise the stored entry is written from the lower-triangle image (its mirror names the same stored entry); dQ was zero-filled.
__global__ void k_adj_grad_Q(int n, const int *__restrict__ Qrp, const int *__restrict__ Qci, const u32 *__restrict__ mapQ, const double *__restrict__ xu,
                             const double *__restrict__ vxu, double *__restrict__ dQ) {
    const int lane = threadIdx.x & (ADJ_LPR - 1);
    const int groups = gridDim.x * (blockDim.x / ADJ_LPR);
    for (int r = blockIdx.x * (blockDim.x / ADJ_LPR) + (threadIdx.x / ADJ_LPR); r < n; r += groups) {
        const double vr = vxu[r], xr = xu[r];
        for (int k = Qrp[r] + lane; k < Qrp[r + 1]; k += ADJ_LPR) {
            const int cc = Qci[k];
            if (!mapQ) dQ[k] = -(vxu[cc] * xr);
            else if (r == cc) dQ[mapQ[k]] = -(vr * xr);
            else if (r > cc) dQ[mapQ[k]] = -(vr * xu[cc] + vxu[cc] * xr);
        }
    }
}
// ---- qpdo_amd_tangent: the right-hand side of the tangent system, formed from the caller's perturbations and the UNSCALED x, y ------------
// rx_j = -(tq_j + (tQ x)_j + (tA_S' y_S)_j) over the rows of the full CSR(Q) and of CSR(A') (whose value order is the caller's CSC order of
// A).  tQ is read through mapQ (stype +-1: the stored entry a Qf entry came from) or straight (mapQ == null, stype 0: entry k of row j of Qf
// IS the caller's entry k of column j).  ADJ_LPR lanes per row: lane L adds the entries Qrp[j] + L, + ADJ_LPR, ... of tQ and then the
// entries Trp[j] + L, + ADJ_LPR, ... of tA to ONE partial sum in that order, the 16 partial sums are folded 8, 4, 2, 1 (lane L += lane
// L + o), and lane 0 adds tq_j to the fold.  An entry of tA on an unflagged row is branched past (it may hold NaN).  A null tq, tQ or tA
// is a zero perturbation.  Every lane takes part in every shuffle.
__global__ void k_tan_rhs_x(int n, const double *__restrict__ tq, const int *__restrict__ Qrp, const int *__restrict__ Qci, const u32 *__restrict__ mapQ,
                            const double *__restrict__ tQ, const int *__restrict__ Trp, const int *__restrict__ Tci, const double *__restrict__ tA,
                            const int *__restrict__ flag, const double *__restrict__ xu, const double *__restrict__ yu, double *__restrict__ rx) {
    const int lane = threadIdx.x & (ADJ_LPR - 1);
    const int groups = gridDim.x * (blockDim.x / ADJ_LPR);
    const int rounds = (n + groups - 1) / groups;
    for (int it = 0; it < rounds; it++) {
        const int j = it * groups + blockIdx.x * (blockDim.x / ADJ_LPR) + (threadIdx.x / ADJ_LPR);
        double s = 0.0;
        if (j < n) {
            if (tQ) for (int k = Qrp[j] + lane; k < Qrp[j + 1]; k += ADJ_LPR) s += tQ[mapQ ? mapQ[k] : (u32)k] * xu[Qci[k]];
            if (tA) for (int k = Trp[j] + lane; k < Trp[j + 1]; k += ADJ_LPR) { const int i = Tci[k]; if (flag[i]) s += tA[k] * yu[i]; }
        }
#pragma unroll
        for (int o = ADJ_LPR / 2; o > 0; o >>= 1) s += __shfl_down(s, o, ADJ_LPR);
        if (j < n && lane == 0) rx[j] = -((tq ? tq[j] : 0.0) + s);
    }
}
// ry_i = tb_i - (tA x)_i on flagged rows (tb = tu on +1 rows, tl on -1 rows), a plain 0 elsewhere, over the rows of CSR(A); tA is read
// through mapA (the caller's CSC position of an entry of CSR(A)).  The lane split and the fold are k_tan_rhs_x's; lane 0 subtracts the
// fold from tb_i.  Nothing of an unflagged row is read, nor tl on a +1 row, nor tu on a -1 row.
__global__ void k_tan_rhs_y(int m, const double *__restrict__ tl, const double *__restrict__ tu, const int *__restrict__ Arp, const int *__restrict__ Aci,
                            const u32 *__restrict__ mapA, const double *__restrict__ tA, const int *__restrict__ flag, const double *__restrict__ xu,
                            double *__restrict__ ry) {
    const int lane = threadIdx.x & (ADJ_LPR - 1);
    const int groups = gridDim.x * (blockDim.x / ADJ_LPR);
    const int rounds = (m + groups - 1) / groups;
    for (int it = 0; it < rounds; it++) {
        const int i = it * groups + blockIdx.x * (blockDim.x / ADJ_LPR) + (threadIdx.x / ADJ_LPR);
        const int f = i < m ? flag[i] : 0;
        double s = 0.0;
        if (f && tA) for (int k = Arp[i] + lane; k < Arp[i + 1]; k += ADJ_LPR) s += tA[mapA[k]] * xu[Aci[k]];
#pragma unroll
        for (int o = ADJ_LPR / 2; o > 0; o >>= 1) s += __shfl_down(s, o, ADJ_LPR);
        if (i < m && lane == 0) {
            double r = 0.0;
            if (f) { const double *tb = f > 0 ? tu : tl; r = (tb ? tb[i] : 0.0) - s; }
            ry[i] = r;
        }
    }
}
// back to the caller's space, with k_adj_grad_vec's arithmetic: dx = D vxs, dy = E vys / c on flagged rows, an exact +0.0 elsewhere
__global__ void k_tan_out(int n, int m, int scaled, double cinv, const double *__restrict__ D, const double *__restrict__ E, const int *__restrict__ flag,
                          const double *__restrict__ vx, const double *__restrict__ vy, double *__restrict__ dx, double *__restrict__ dy) {
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int j = t0; j < n; j += stride) dx[j] = scaled ? D[j] * vx[j] : vx[j];
    for (int i = t0; i < m; i += stride) {
        double v = 0.0;
        if (flag[i]) { v = vy[i]; if (scaled) { v = E[i] * v; v = v * cinv; } }
        dy[i] = v;
    }
}

static int adjoint_refuse(const char *msg) { snprintf(g_err, sizeof(g_err), "qpdo_amd_adjoint: %s", msg); return -1; }

int qdev_get_adjoint_stats(QpdoDev *d, QdevAdjointStats *out) { *out = d->adj; return 0; }
int qdev_get_tangent_stats(QpdoDev *d, QdevTangentStats *out) { *out = d->tan; return 0; }

// the workspaces the two calls take: one GPU, the dense LDL' or the band LDL' as the workspace's solver -- the band of every kind: b <= 127,
// the tiled wide band (128 .. 1023), either under an adopted variable order, and b <= 127 with coupling rows.  who: the entry point's
// name, which the message begins with
static const char *adj_kind_refusal(const QpdoDev *d) {
    if (d->comm.active) return "row-partitioned workspaces are not supported (solve the QP on one GPU, or take finite differences of qpdo_solve)";
    if (d->hybrid) return "the workspace starts its solves with PCG (the hybrid of an automatically chosen dense solver from n = 8192, QPDO_HYBRID); set up with QPDO_LINSOLVE=dense";
    if (d->linsolve != 1 && d->linsolve != 3)
        return "the workspace's solver is PCG; the adjoint needs a direct solver: set up with QPDO_LINSOLVE=dense (n <= 40000) or QPDO_LINSOLVE=band";
    return nullptr;
}
int qdev_adjoint_check_kind(QpdoDev *d, const char *who) {
    const char *msg = adj_kind_refusal(d);
    if (!msg) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
    return -1;
}
// The group size of the two calls on this workspace as it stands: the right-hand sides that go through every launch of the sweep loop at
// once.  0: a workspace the calls refuse.  1 (the right-hand sides follow one another): a matrix on the slab kernel -- a slab multi-vector
// product does not exist --, and the dense route on the stepwise solves (QPDO_DENSE_SOLVE=steps, or after a lost producer), and
// the band solver's bordered mode (QPDO_BAND_BORDER), which has no group kernels.  Otherwise QPDO_AMD_RHS_GROUP as read at setup, 8 by default.
int qdev_rhs_group(QpdoDev *d) {
    if (adj_kind_refusal(d)) return 0;
    if (d->Qf.use_slab || d->Ar.use_slab || d->At.use_slab) return 1;
    if (d->linsolve == 1 && !d->dense_chain) return 1;
    if (d->linsolve == 3 && d->bb_c > 0) return 1;
    return d->rhs_group_cfg;
}
int qdev_get_group_stats(QpdoDev *d, QdevGroupStats *out) { *out = d->grp; out->group = qdev_rhs_group(d); return 0; }

// the last of the two calls' checks: the caller's Q (passed with dQx / tQx, `arr`) against the setup's pattern.  The first time a Q is
// seen it is compared on the device and, for stype +-1, mapQ is built (upd_first_Q: whichever of qpdo_amd_update_matrices, the adjoint
// and the tangent comes first builds it); later calls compare the column pointers.  Nothing is adopted from a refused call.
static int adj_check_Q(QpdoDev *d, const QdevCsc *Q, const char *who, const char *arr) {
    u32 *newMapQ = nullptr; double *newStage = nullptr;
    int rc = 0, differs = 0;
    const bool firstQ = d->upd_Qp.empty();
    if (!firstQ && !upd_colptr_same(Q, d->upd_Qp)) differs = 1;
    if (firstQ) {
        TempAllocs tmp;
        rc = upd_first_Q(d, tmp, Q, &differs, &newMapQ, &newStage);
        if (!rc) { hipError_t e = hipGetLastError(); if (e != hipSuccess) rc = set_err(e, "adjoint checks", __LINE__); }
        tmp.release(d->stream);
        h2d_staging_release(d);
    }
    if (!rc && differs) {
        snprintf(g_err, sizeof(g_err), "%s: the pattern of Q differs from the one given to qpdo_setup (%s follows the setup's stored entries)", who, arr);
        rc = -1;
    }
    if (rc) { upd_free(d, newMapQ); upd_free(d, newStage); return rc; }
    if (newMapQ) { d->mapQ = newMapQ; d->qstage = newStage; }
    if (firstQ) upd_colptr(Q, d->upd_Qp);
    return 0;
}

// ---- ONE sweep driver for qdev_adjoint and qdev_tangent ------------------------------------------------------------------------------------
// AdjCall: what one call of either kind holds between adj_begin and adj_end -- the work vectors, the scaling, what is kept of the workspace.
extern "C++" {
struct AdjCall {
    int n = 0, m = 0, scaled = 0, kind = 0, gnm = 1;
    double sc_c = 1.0, sc_cinv = 1.0;
    double *xu = nullptr, *gxs = nullptr, *vx = nullptr, *rx = nullptr, *t1 = nullptr, *t2 = nullptr;
    double *yu = nullptr, *gys = nullptr, *vy = nullptr, *ry = nullptr, *wry = nullptr, *Av = nullptr, *a2 = nullptr;
    int *flag = nullptr;
    DirectKeep keep; QdevStats st_keep;
    int code3 = 0, kact = 0;
    long sweeps_total = 0;
    // G: the right-hand sides a group carries.  The per-right-hand-side vectors are five n-vectors at bn and five m-vectors at bm, G slabs
    // each: vector v of right-hand side k at bn + (v G + k) n.  G = 1: the single call's vectors inside adj_n / adj_m.  The named pointers
    // above are those of the right-hand side adj_point chose last; at k = 0 they are the bases the group kernels take.
    int G = 1;
    double *bn = nullptr, *bm = nullptr;
    // the group's solve: the right-hand sides (n apart) and the solutions (ldx apart), compact over the live right-hand sides; the dense
    // route's padded columns, polled vectors and forward results (ld apart), the band route's forward results (np apart) and, with coupling
    // rows, the Woodbury application's z0 columns (ldx apart) and t columns (BC_MAX apart)
    double *srhs = nullptr, *sdvx = nullptr, *sx = nullptr, *spub1 = nullptr, *schy = nullptr, *spub2 = nullptr, *sz = nullptr, *sz0 = nullptr, *st = nullptr;
    long long ldx = 0;
};
}
static void adj_point(AdjCall &c, int k) {
    const size_t n = (size_t)c.n, m = (size_t)c.m, G = (size_t)c.G, kk = (size_t)k;
    c.gxs = c.bn + (0 * G + kk) * n; c.vx = c.bn + (1 * G + kk) * n; c.rx = c.bn + (2 * G + kk) * n; c.t1 = c.bn + (3 * G + kk) * n; c.t2 = c.bn + (4 * G + kk) * n;
    c.gys = c.bm + (0 * G + kk) * m; c.vy = c.bm + (1 * G + kk) * m; c.ry = c.bm + (2 * G + kk) * m; c.wry = c.bm + (3 * G + kk) * m; c.Av = c.bm + (4 * G + kk) * m;
}
// the work vectors (allocated by the first call of either kind: a host allocation, which may wait for earlier device work; booked in that
// kind's scratch_bytes)
static int adj_vectors(QpdoDev *d, AdjCall &c, long nrhs, int64_t *booked) {
    const int n = d->n, m = d->m;
    if (!d->adj_n) {
        int rc = upd_alloc(d, &d->adj_n, (size_t)ADJ_N_COUNT * n);
        if (!rc) rc = upd_alloc(d, &d->adj_m, (size_t)ADJ_M_COUNT * m);
        if (!rc) rc = upd_alloc(d, &d->adj_flag, (size_t)m);
        if (rc) return rc;
        *booked += ((int64_t)ADJ_N_COUNT * n + (int64_t)ADJ_M_COUNT * m) * 8 + (int64_t)m * 4;
    }
    c.n = n; c.m = m; c.kind = d->linsolve;
    static_assert(ADJ_N_GXS == 1 && ADJ_N_VX == 2 && ADJ_N_RX == 3 && ADJ_N_T1 == 4 && ADJ_N_T2 == 5, "adj_point's order of the n-vectors");
    static_assert(ADJ_M_GYS == 1 && ADJ_M_VY == 2 && ADJ_M_RY == 3 && ADJ_M_WRY == 4 && ADJ_M_AV == 5, "adj_point's order of the m-vectors");
    c.xu = d->adj_n + (size_t)ADJ_N_XU * n; c.yu = d->adj_m + (size_t)ADJ_M_YU * m; c.a2 = d->adj_m + (size_t)ADJ_M_A2 * m;
    c.G = 1; c.bn = d->adj_n + (size_t)ADJ_N_GXS * n; c.bm = d->adj_m + (size_t)ADJ_M_GYS * m;
    adj_point(c, 0);
    c.flag = d->adj_flag;
    c.scaled = d->scaled;
    c.sc_c = c.scaled ? d->sc_c : 1.0; c.sc_cinv = c.scaled ? d->sc_cinv : 1.0;
    c.gnm = vgrid(n > m ? n : m);
    // a call with nrhs > 1 where the workspace's group size is above 1: the group's vectors (allocated by the first such call of either
    // kind: host allocations, which may wait for earlier device work; booked in the group's scratch_bytes alone).  xu, yu, a2 and the
    // flags stay the single call's.
    const int G = nrhs > 1 ? qdev_rhs_group(d) : 1;
    if (G <= 1) return 0;
    const int Gc = d->rhs_group_cfg;
    const size_t ld = (size_t)((n + DNB - 1) / DNB * DNB), ldx = c.kind == 3 ? (size_t)n : ld;      // (ld: dense_alloc's; it covers band_alloc's np)
    if (!d->grp_hctrl) {
        static_assert(sizeof(AdjGrpCtrl) == 40 && SPMV_GROUP_MAX * sizeof(AdjGrpCtrl) / 8 <= 64 && sizeof(Ctrl) / 8 <= 64, "k_adj_grp_publish copies both blocks with two waves");
        const size_t sol = (size_t)Gc * ((size_t)n + 5 * ld);                 // (the larger of the two routes' layouts: the solver may change, the buffers stay)
        int rc = upd_alloc(d, &d->grp_n, (size_t)5 * Gc * n);
        if (!rc) rc = upd_alloc(d, &d->grp_m, (size_t)5 * Gc * m);
        if (!rc) rc = upd_alloc(d, &d->grp_sol, sol);
        if (!rc) rc = upd_alloc(d, &d->grp_ctrl, (size_t)SPMV_GROUP_MAX);
        if (rc) return rc;
        HIPCHK(hipHostMalloc((void **)&d->grp_hctrl, SPMV_GROUP_MAX * sizeof(AdjGrpCtrl), hipHostMallocCoherent));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve_group), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
        if (d->bo_newold) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve_group_perm), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
        d->grp.scratch_bytes += (int64_t)(((size_t)5 * Gc * ((size_t)n + m) + sol) * 8 + SPMV_GROUP_MAX * sizeof(AdjGrpCtrl));
    }
    // the band route's columns inside the per-column share n + 5 ld of grp_sol: right-hand side n, solution n, then three parts of ld -- the
    // forward result (np <= ld: band_alloc rounds n up to 4, band_wide_alloc to DNB as ld is) and, with coupling rows, z0 (n) and t (BC_MAX)
    static_assert(BC_MAX <= DNB, "a column's t fits the ld entries set aside for it");
    if (c.kind == 3 && (size_t)d->band_np > ld) return set_err(hipErrorInvalidValue, "adjoint group: the band solve's columns do not fit the group's solve buffer", __LINE__);
    c.G = G; c.bn = d->grp_n; c.bm = d->grp_m;
    adj_point(c, 0);
    double *p = d->grp_sol;
    c.ldx = (long long)ldx;
    c.srhs = p; p += (size_t)Gc * n;
    c.sdvx = p; p += (size_t)Gc * ldx;
    if (c.kind == 3) { c.sz = p; c.sz0 = p + (size_t)Gc * ld; c.st = p + (size_t)2 * Gc * ld; }
    else { c.sx = p; c.spub1 = p + (size_t)Gc * ld; c.schy = p + (size_t)2 * Gc * ld; c.spub2 = p + (size_t)3 * Gc * ld; }
    return 0;
}
// once per call: what the call overwrites of the workspace is kept (host_probe.inc direct_keep_*), the counters too; x, y go up; the scaled
// x, the flags, s, W, the forced factorization, the pivot check.  Returns nonzero on an error of the runtime (adj_end still follows).
static int adj_begin(QpdoDev *d, AdjCall &c, const double *x, const double *y) {
    const int n = c.n, m = c.m;
    c.st_keep = d->st;
    { int rc = direct_keep_save(d, c.keep, true); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(c.xu, x, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    if (m) HIPCHK(hipMemcpyAsync(c.yu, y, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
    LAUNCH(k_adj_scale_x, vgrid(n), n, c.scaled, (const double *)d->Dinv, (const double *)c.xu, d->qdiag_valid ? (const double *)d->qdiag : (const double *)nullptr,
           (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val, c.t1, d->ctrl);
    if (m) {
        launch_spmv(d, d->Ar, c.t1, EpiStore{c.Av}, false);
        LAUNCH(k_adj_classify, adj_grid_rows(m), m, c.scaled, (const double *)d->E, (const double *)c.yu, (const double *)d->l, (const double *)d->u, (const double *)c.Av,
               (const int *)d->Ar.rp, (const double *)d->Ar.val, c.flag, c.a2, d->ctrl);
    }
    int rc = read_ctrl(d);
    if (rc) return rc;
    const double mqd = nrm_of(d->hctrl, N_C);
    const double s = mqd > 0.0 ? mqd : 1.0;
    c.kact = d->hctrl->cnt[C_MUCH];
    d->sigma_f = ADJ_SIGMA_REL * s;
    if (m) LAUNCH(k_adj_weights, vgrid(m), m, s, (const int *)c.flag, (const double *)c.a2, d->d);
    // forced: a fresh factorization of (sigma_f, d), whatever the low-rank and up/downdate routes would do with a kept factor
    if (c.kind == 3) rc = band_factor(d, true);
    else {
        rc = dense_factor(d);
        if (!rc) LAUNCH(k_adj_check_pivots, vgrid(n), n, (const double *)d->Dg, d->ctrl);
    }
    return rc;
}
// THE acceptance of a right-hand side after a sweep, for both sweep drivers.  nrm: its four maxima in the control block's order N_A .. N_D
// (||gx||, ||gy_S||, the sweep's two residual norms) as bit patterns; viol: its non-finite marker.  *rel: the relative residual.
static bool adj_accept(const u64 *nrm, int viol, double sc_cinv, double tol, double *rel) {
    double v[4]; memcpy(v, nrm, sizeof(v));
    const double gnorm = fmax(v[0], v[1]);
    const double rn = fmax(v[2] * sc_cinv, v[3]);
    *rel = gnorm > 0.0 ? rn / gnorm : rn;
    return !viol && rn <= tol * gnorm;
}
// read_ctrl with the first cnt slots of the group control array brought along into d->grp_hctrl: one publication, or a second copy
static int read_ctrl_group(QpdoDev *d, int cnt) {
    if (!d->ctrl_publish) {
        HIPCHK(hipMemcpyAsync(d->grp_hctrl, d->grp_ctrl, (size_t)cnt * sizeof(AdjGrpCtrl), hipMemcpyDeviceToHost, d->stream));
        return read_ctrl(d);
    }
    const u64 seq = ++d->pub_seq;
    hipLaunchKernelGGL(k_adj_grp_publish, dim3(1), dim3(128), 0, d->stream, (const Ctrl *)d->ctrl, d->hctrl, (const AdjGrpCtrl *)d->grp_ctrl, d->grp_hctrl, cnt, d->hseq, seq);
    { int rc = ctrl_wait(d, d->hseq, seq); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    return 0;
}
// per right-hand side: the UNSCALED right-hand side is in (c.rx, c.ry) -- both are rewritten by the first sweep's residual after k_adj_rhs
// has read them; have_ry false: ry is zero and not read --; k_adj_rhs, the sweeps, the acceptance.  On return with *code == 0 the scaled
// solution is in (c.vx, c.vy) and c.rx, c.ry, c.t1, c.t2, c.wry, c.Av are free.  A code 3 is latched in c.code3: the right-hand sides
// behind it are not run.
static int adj_sweeps(QpdoDev *d, AdjCall &c, bool have_ry, double tol, long max_sweeps, int *code_out, long *sweep_out, double *rel_out) {
    const int n = c.n, m = c.m, scaled = c.scaled;
    const double nan = __builtin_nan("");
    int code = c.code3 ? 3 : 1, rc = 0; long sweep = 0; double rel = nan;
    if (!c.code3) {
        LAUNCH(k_adj_ctrl_clear, 1, d->ctrl, 1);
        LAUNCH(k_adj_rhs, c.gnm, n, m, scaled, c.sc_c, (const double *)d->D, (const double *)d->E, (const double *)c.rx, have_ry ? (const double *)c.ry : (const double *)nullptr,
               (const int *)c.flag, c.gxs, c.gys, c.vx, c.vy, d->ctrl);
        for (;; sweep++) {
            if (sweep) LAUNCH(k_adj_ctrl_clear, 1, d->ctrl, 0);
            launch_spmv(d, d->Qf, c.vx, EpiStore{c.t1}, false);
            if (m) { launch_spmv(d, d->Ar, c.vx, EpiStore{c.Av}, false); launch_spmv(d, d->At, c.vy, EpiStore{c.t2}, false); }
            else HIPCHK(hipMemsetAsync(c.t2, 0, (size_t)n * 8, d->stream));
            LAUNCH(k_adj_resid, c.gnm, n, m, scaled, (const double *)d->Dinv, (const double *)d->Einv, (const double *)c.gxs, (const double *)c.t1, (const double *)c.t2,
                   (const double *)c.gys, (const double *)c.Av, (const int *)c.flag, (const double *)d->d, c.rx, c.ry, c.wry, d->ctrl);
            rc = read_ctrl(d); if (rc) break;
            d->grp.rounds_total++;
            if (d->hctrl->cnt[C_CHAIN_ERR] || d->hctrl->cnt[C_DINF]) { c.code3 = 1; code = 3; break; }
            if (adj_accept(d->hctrl->nrm + N_A, d->hctrl->cnt[C_VIOL], c.sc_cinv, tol, &rel)) { code = 0; break; }
            if (sweep >= max_sweeps) break;
            if (m) launch_spmv(d, d->At, c.wry, EpiStore{c.t2}, false);
            LAUNCH(k_adj_solve_rhs, vgrid(n), n, (const double *)c.rx, (const double *)c.t2, d->rhs);
            // (coupling rows: ONE Woodbury application on the fresh factors of B and S, not band_solve's checked refinement -- this loop is
            // the refinement on the true system, and an inexact inner solve costs sweeps or ends as code 1, never as code 3)
            rc = c.kind != 3 ? dense_solve(d) : d->bc_k > 0 ? band_coupled_apply(d, d->rhs, d->dx) : band_solve(d); if (rc) break;
            if (m) launch_spmv(d, d->Ar, d->dx, EpiStore{c.Av}, false);
            LAUNCH(k_adj_update, c.gnm, n, m, (const double *)d->dx, (const double *)c.Av, (const double *)c.ry, (const double *)d->d, c.vx, c.vy);
        }
        if (rc) return rc;
        c.sweeps_total += sweep;
        d->grp.groups_run++;
    }
    *code_out = code; *sweep_out = code == 3 ? 0 : sweep; *rel_out = code == 0 ? rel : nan;
    return 0;
}
// The same for the cnt <= c.G right-hand sides of a group (G > 1; the unscaled right-hand sides in slabs 0 .. cnt - 1 of rx, ry): every
// launch of the sweep loop is made once for the right-hand sides still in the sweeps (`live`), with one read-back per sweep -- the
// control block (the call's code-3 latch) and the group control array (per right-hand side the four maxima and the non-finite marker)
// in one publication or two copies.  Every right-hand side receives adj_sweeps' operations in adj_sweeps' order: the vector kernels run
// the single kernels' bodies, the products k_spmv's row loop per vector, the solves the single solve's kernel per column.  A right-hand
// side leaves at its own sweep count -- accepted, or code 1 at max_sweeps -- and from then on no launch reads or writes its vectors: its
// solution stays in its slab of (vx, vy).  The solves' columns are compact over the live right-hand sides: a column that left is neither
// produced nor polled.  A code 3 hits the right-hand sides still in the sweeps, and the latch those behind them.
static int adj_sweeps_group(QpdoDev *d, AdjCall &c, int cnt, bool have_ry, double tol, long max_sweeps, int *code_out, long *sweep_out, double *rel_out) {
    const int n = c.n, m = c.m, scaled = c.scaled, G = c.G;
    const double nan = __builtin_nan("");
    for (int k = 0; k < cnt; k++) { code_out[k] = c.code3 ? 3 : 1; sweep_out[k] = 0; rel_out[k] = nan; }
    if (c.code3) return 0;
    adj_point(c, 0);                                       // the bases of the group's vectors
    AdjGrpCtrl *gc = d->grp_ctrl; const AdjGrpCtrl *hg = d->grp_hctrl;
    unsigned live = (1u << cnt) - 1u;
    int rc = 0; long sweep = 0;
    const dim3 gv(c.gnm, cnt), gvn(vgrid(n), cnt);
    LAUNCH(k_adj_grp_clear, 1, gc, G, 1);
    LAUNCH(k_adj_rhs_group, gv, n, m, scaled, c.sc_c, (const double *)d->D, (const double *)d->E, (const double *)c.rx, have_ry ? (const double *)c.ry : (const double *)nullptr,
           (const int *)c.flag, c.gxs, c.gys, c.vx, c.vy, live, gc);
    for (;; sweep++) {
        if (sweep) LAUNCH(k_adj_grp_clear, 1, gc, G, 0);
        launch_spmv_group(d, d->Qf, c.vx, n, false, c.t1, n, live);
        if (m) { launch_spmv_group(d, d->Ar, c.vx, n, false, c.Av, m, live); launch_spmv_group(d, d->At, c.vy, m, false, c.t2, n, live); }
        else HIPCHK(hipMemsetAsync(c.t2, 0, (size_t)G * n * 8, d->stream));      // (t2 is scratch: a right-hand side that left does not read it again)
        LAUNCH(k_adj_resid_group, gv, n, m, scaled, (const double *)d->Dinv, (const double *)d->Einv, (const double *)c.gxs, (const double *)c.t1, (const double *)c.t2,
               (const double *)c.gys, (const double *)c.Av, (const int *)c.flag, (const double *)d->d, c.rx, c.ry, c.wry, live, gc);
        rc = read_ctrl_group(d, cnt); if (rc) break;
        d->grp.rounds_total++;
        if (d->hctrl->cnt[C_CHAIN_ERR] || d->hctrl->cnt[C_DINF]) {
            c.code3 = 1;
            for (int k = 0; k < cnt; k++) if ((live >> k) & 1u) { code_out[k] = 3; sweep_out[k] = 0; rel_out[k] = nan; }
            live = 0;
            break;
        }
        for (int k = 0; k < cnt; k++) {
            if (!((live >> k) & 1u)) continue;
            double rel = nan;
            const bool ok = adj_accept(hg[k].nrm, hg[k].nonfin, c.sc_cinv, tol, &rel);
            if (!ok && sweep < max_sweeps) continue;
            code_out[k] = ok ? 0 : 1; sweep_out[k] = sweep; rel_out[k] = ok ? rel : nan;
            c.sweeps_total += sweep;
            live &= ~(1u << k);
        }
        if (!live) break;
        if (m) launch_spmv_group(d, d->At, c.wry, m, false, c.t2, n, live);
        LAUNCH(k_adj_solve_rhs_group, gvn, n, (const double *)c.rx, (const double *)c.t2, c.srhs, live);
        const int nl = __builtin_popcount(live);
        if (c.kind == 3 && d->band_b > BAND_MAX_B) {
            const int nbc = d->band_np / DNB;
            if (d->bo_newold)
                hipLaunchKernelGGL(k_bw_solve_group_perm, dim3(nl), dim3(256), 0, d->stream, n, nbc, d->bw_w, (const double *)d->bw_Wb, (const double *)d->bw_Li,
                                   (const double *)d->bw_LiT, (const double *)d->bw_Wd, (const double *)c.srhs, (long long)n, c.sz, c.sdvx, (const int *)d->bo_newold);
            else
                hipLaunchKernelGGL(k_bw_solve_group, dim3(nl), dim3(256), 0, d->stream, n, nbc, d->bw_w, (const double *)d->bw_Wb, (const double *)d->bw_Li,
                                   (const double *)d->bw_LiT, (const double *)d->bw_Wd, (const double *)c.srhs, (long long)n, c.sz, c.sdvx);
        } else if (c.kind == 3 && d->bc_k > 0) {
            // band_coupled_apply per live column: the single kernels' bodies on columns of their own
            const size_t lds = (size_t)4 * BAND_SC * (d->band_b + 1) * sizeof(double);
            hipLaunchKernelGGL(k_band_solve_group, dim3(nl), dim3(256), lds, d->stream, n, d->band_np, d->band_b, (const double *)d->Kb, (const double *)d->Lt,
                               (const double *)c.srhs, (long long)n, c.sz, c.sz0);
            hipLaunchKernelGGL(k_bc_t_group, dim3(nl), dim3(1024), 0, d->stream, d->bc_k, d->bc_act, (const int *)d->bc_rows, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                               (const double *)d->Ar.val, (const double *)c.sz0, (long long)n, (const double *)d->bc_SL, c.st);
            LAUNCH(k_bc_apply_group, dim3(vgrid(n), nl), n, d->band_np, d->bc_k, d->bc_act, (const double *)d->bc_Z, (const double *)c.st, (const double *)c.sz0, c.sdvx,
                   (long long)n);
        } else if (c.kind == 3) {
            const size_t lds = (size_t)4 * BAND_SC * (d->band_b + 1) * sizeof(double);
            if (d->bo_newold)
                hipLaunchKernelGGL(k_band_solve_group_perm, dim3(nl), dim3(256), lds, d->stream, n, d->band_np, d->band_b, (const double *)d->Kb, (const double *)d->Lt,
                                   (const double *)c.srhs, (long long)n, c.sz, c.sdvx, (const int *)d->bo_newold);
            else
                hipLaunchKernelGGL(k_band_solve_group, dim3(nl), dim3(256), lds, d->stream, n, d->band_np, d->band_b, (const double *)d->Kb, (const double *)d->Lt,
                                   (const double *)c.srhs, (long long)n, c.sz, c.sdvx);
        } else {
            const int ld = d->dense_ld;
            LAUNCH(k_dense_load_rhs_group, dim3(vgrid(ld), nl), n, ld, (const double *)c.srhs, (long long)n, c.sx, c.spub1, c.spub2);
            // the single solve's kernel on the grid (columns, block rows).  (One workgroup per block row that reads each tile once for all
            // columns was built and measured 1.24x - 1.33x slower per call at n = 1000 and n = 1e4: docs/LAB_NOTES.md.)
            launch_ldl_chain<true>(d, nl, c.sx, c.spub1, c.schy, ld);
            launch_ldl_chain<false>(d, nl, c.schy, c.spub2, c.sdvx, n);
        }
        if (m) launch_spmv_group(d, d->Ar, c.sdvx, c.ldx, true, c.Av, m, live);
        LAUNCH(k_adj_update_group, gv, n, m, (const double *)c.sdvx, c.ldx, (const double *)c.Av, (const double *)c.ry, (const double *)d->d, c.vx, c.vy, live);
    }
    if (rc) return rc;
    d->grp.groups_run++;
    return 0;
}
// the end of a call: the flags out (all 0 after a code 3), the code-3 latch cleared as qdev_direct_solve does (nothing is redone), the
// control block, the counters and what adj_begin kept put back.  rc: what the call met so far; returned, or the restore's own error.
static int adj_end(QpdoDev *d, AdjCall &c, int *active, int rc) {
    if (!rc && active && c.m) {
        if (c.code3) memset(active, 0, (size_t)c.m * sizeof(int));
        else HIPCHK(hipMemcpyAsync(active, c.flag, (size_t)c.m * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    }
    if (c.code3) {
        LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
        d->dense_valid = 0; d->dense_factored = 0; d->wb_k = 0; d->mid_fwd_valid = 0; d->bc_factored = 0;
    }
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    d->ctrl_clean = 0;
    d->st = c.st_keep;
    { int rck = direct_keep_restore(d, c.keep); if (rck && !rc) rc = rck; }
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}
static void adj_book(QdevAdjointStats &st, long nrhs, long sweeps_total, const struct timespec &ts0) {
    struct timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1);
    st.calls++; st.factorizations++; st.rhs_total += nrhs; st.sweeps_total += sweeps_total;
    st.last_seconds = (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec);
}

int qdev_adjoint(QpdoDev *d, const double *x, const double *y, long nrhs, const double *gx, const double *gy, double *dq, double *dl, double *du,
                 const QdevCsc *Q, double *dQx, double *dAx, int *active, long *status, double *res, double tol, long max_sweeps) {
    HIPCHK(hipSetDevice(d->device));
    struct timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
    const int n = d->n, m = d->m;
    // ---- checks: nothing is launched or written before they pass ------------------------------------------------------------------
    { int rck = qdev_adjoint_check_kind(d, "qpdo_amd_adjoint"); if (rck) return rck; }
    const bool wantQ = dQx != nullptr, wantA = dAx != nullptr;
    if (wantQ) { int rck = adj_check_Q(d, Q, "qpdo_amd_adjoint", "dQx"); if (rck) return rck; }
    // ---- the checks passed --------------------------------------------------------------------------------------------------------
    const long long nnzA = d->At.nnz, nnzQf = d->Qf.nnz, nnzQ = wantQ ? (long long)Q->nnz : 0;
    AdjCall c;
    { int rck = adj_vectors(d, c, nrhs, &d->adj.scratch_bytes); if (rck) return rck; }
    if (wantA && !d->adj_dA) { int rc = upd_alloc(d, &d->adj_dA, (size_t)nnzA); if (rc) return rc; d->adj.scratch_bytes += nnzA * 8; }
    if (wantQ && !d->adj_dQ) { int rc = upd_alloc(d, &d->adj_dQ, (size_t)nnzQ); if (rc) return rc; d->adj.scratch_bytes += nnzQ * 8; }
    const double nan = __builtin_nan("");
    int rc = adj_begin(d, c, x, y);
    // ---- the right-hand sides on the one factor, in groups of up to c.G (G = 1: one after the other) ---------------------------------------
    for (long r0 = 0; r0 < nrhs && !rc; r0 += c.G) {
        const int cnt = (int)(nrhs - r0 < c.G ? nrhs - r0 : c.G);
        int code[SPMV_GROUP_MAX]; long sweep[SPMV_GROUP_MAX]; double rel[SPMV_GROUP_MAX];
        for (int k = 0; k < cnt && !c.code3; k++) {
            const long r = r0 + k;
            adj_point(c, k);
            HIPCHK(hipMemcpyAsync(c.rx, gx + (size_t)r * n, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
            if (m && gy) HIPCHK(hipMemcpyAsync(c.ry, gy + (size_t)r * m, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
        }
        rc = c.G == 1 ? adj_sweeps(d, c, gy != nullptr, tol, max_sweeps, code, sweep, rel) : adj_sweeps_group(d, c, cnt, gy != nullptr, tol, max_sweeps, code, sweep, rel);
        if (rc) break;
        bool any = false;
        for (int k = 0; k < cnt; k++) {
            const long r = r0 + k;
            double *dqr = dq + (size_t)r * n, *dlr = dl + (size_t)r * m, *dur = du + (size_t)r * m;
            double *dQr = wantQ ? dQx + (size_t)r * nnzQ : nullptr, *dAr = wantA ? dAx + (size_t)r * nnzA : nullptr;
            if (status) { status[3 * r] = code[k]; status[3 * r + 1] = sweep[k]; status[3 * r + 2] = c.kact; }
            if (res) res[r] = rel[k];
            if (code[k] != 0) {
                for (int j = 0; j < n; j++) dqr[j] = nan;
                for (int i = 0; i < m; i++) { dlr[i] = nan; dur[i] = nan; }
                for (long long e = 0; e < nnzQ; e++) dQr[e] = nan;
                if (wantA) for (long long e = 0; e < nnzA; e++) dAr[e] = nan;
                continue;
            }
            any = true;
            adj_point(c, k);
            // the unscaled vx into rx, vy into ry (the sweeps are over); dq in t1, dl in wry, du in Av
            LAUNCH(k_adj_grad_vec, c.gnm, n, m, c.scaled, c.sc_cinv, (const double *)d->D, (const double *)d->E, (const int *)c.flag, (const double *)c.vx, (const double *)c.vy,
                   c.rx, c.ry, c.t1, c.wry, c.Av);
            HIPCHK(hipMemcpyAsync(dqr, c.t1, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
            if (m) { HIPCHK(hipMemcpyAsync(dlr, c.wry, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipMemcpyAsync(dur, c.Av, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream)); }
            if (wantA && nnzA) {
                LAUNCH(k_adj_grad_A, adj_grid_rows(n), n, (const int *)d->At.rp, (const int *)d->At.ci, (const int *)c.flag, (const double *)c.xu, (const double *)c.yu,
                       (const double *)c.rx, (const double *)c.ry, d->adj_dA);
                HIPCHK(hipMemcpyAsync(dAr, d->adj_dA, (size_t)nnzA * 8, hipMemcpyDeviceToHost, d->stream));
            }
            if (wantQ && nnzQ) {
                const bool mapped = Q->stype != 0;
                if (mapped) HIPCHK(hipMemsetAsync(d->adj_dQ, 0, (size_t)nnzQ * 8, d->stream));
                if (nnzQf) LAUNCH(k_adj_grad_Q, adj_grid_rows(n), n, (const int *)d->Qf.rp, (const int *)d->Qf.ci, mapped ? (const u32 *)d->mapQ : (const u32 *)nullptr,
                                  (const double *)c.xu, (const double *)c.rx, d->adj_dQ);
                HIPCHK(hipMemcpyAsync(dQr, d->adj_dQ, (size_t)nnzQ * 8, hipMemcpyDeviceToHost, d->stream));
            }
        }
        if (any) HIPCHK(hipStreamSynchronize(d->stream));
    }
    rc = adj_end(d, c, active, rc);
    if (rc) return rc;
    adj_book(d->adj, nrhs, c.sweeps_total, ts0);
    return 0;
}

// qpdo_amd_tangent (include/qpdo_amd_ext.h): the adjoint's call with the right-hand side formed on the device -- the caller's perturbations
// go up into the tangent's own staging, k_tan_rhs_x / k_tan_rhs_y write the unscaled (rx, ry) where the adjoint's upload puts (gx, gy),
// and adj_sweeps takes it from there.  The right-hand sides follow one another on the one factor, as in the adjoint.
int qdev_tangent(QpdoDev *d, const double *x, const double *y, long nrhs, const double *tq, const double *tl, const double *tu, const QdevCsc *Q,
                 const double *tQx, const double *tAx, double *dx, double *dy, int *active, long *status, double *res, double tol, long max_sweeps) {
    HIPCHK(hipSetDevice(d->device));
    struct timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
    const int n = d->n, m = d->m;
    // ---- checks: nothing is launched or written before they pass ------------------------------------------------------------------
    { int rck = qdev_adjoint_check_kind(d, "qpdo_amd_tangent"); if (rck) return rck; }
    if (tQx) { int rck = adj_check_Q(d, Q, "qpdo_amd_tangent", "tQx"); if (rck) return rck; }
    // ---- the checks passed --------------------------------------------------------------------------------------------------------
    const long long nnzA = d->At.nnz, nnzQ = tQx ? (long long)Q->nnz : 0;
    const bool useQ = tQx && nnzQ && d->Qf.nnz, useA = tAx && m && nnzA, useL = tl && m, useU = tu && m;
    AdjCall c;
    { int rck = adj_vectors(d, c, nrhs, &d->tan.scratch_bytes); if (rck) return rck; }
    if (useA && !d->mapA) {                                    // (the map qpdo_amd_update_matrices builds on its first call; whichever comes first)
        TempAllocs tmp; u32 *newMapA = nullptr;
        int rc = upd_first_mapA(d, tmp, &newMapA, "qpdo_amd_tangent");
        if (!rc) { hipError_t e = hipGetLastError(); if (e != hipSuccess) rc = set_err(e, "tangent map", __LINE__); }
        tmp.release(d->stream);
        if (rc) { upd_free(d, newMapA); return rc; }
        d->mapA = newMapA;
    }
    struct { bool use; double **buf; size_t len; } stage[] = {{tq != nullptr, &d->tan_q, (size_t)n}, {useL, &d->tan_l, (size_t)m}, {useU, &d->tan_u, (size_t)m},
                                                             {useQ, &d->tan_Q, (size_t)nnzQ}, {useA, &d->tan_A, (size_t)nnzA}};
    for (auto &s : stage)
        if (s.use && !*s.buf) { int rc = upd_alloc(d, s.buf, s.len); if (rc) return rc; d->tan.scratch_bytes += (int64_t)s.len * 8; }
    const double nan = __builtin_nan("");
    int rc = adj_begin(d, c, x, y);
    for (long r0 = 0; r0 < nrhs && !rc; r0 += c.G) {
        const int cnt = (int)(nrhs - r0 < c.G ? nrhs - r0 : c.G);
        int code[SPMV_GROUP_MAX]; long sweep[SPMV_GROUP_MAX]; double rel[SPMV_GROUP_MAX];
        for (int k = 0; k < cnt && !c.code3; k++) {          // (one staging for the caller's arrays: the formation kernels of right-hand side k run behind its copies)
            const long r = r0 + k;
            adj_point(c, k);
            if (tq) HIPCHK(hipMemcpyAsync(d->tan_q, tq + (size_t)r * n, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
            if (useL) HIPCHK(hipMemcpyAsync(d->tan_l, tl + (size_t)r * m, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
            if (useU) HIPCHK(hipMemcpyAsync(d->tan_u, tu + (size_t)r * m, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
            if (useQ) HIPCHK(hipMemcpyAsync(d->tan_Q, tQx + (size_t)r * nnzQ, (size_t)nnzQ * 8, hipMemcpyHostToDevice, d->stream));
            if (useA) HIPCHK(hipMemcpyAsync(d->tan_A, tAx + (size_t)r * nnzA, (size_t)nnzA * 8, hipMemcpyHostToDevice, d->stream));
            LAUNCH(k_tan_rhs_x, adj_grid_rows(n), n, tq ? (const double *)d->tan_q : (const double *)nullptr, (const int *)d->Qf.rp, (const int *)d->Qf.ci,
                   Q && Q->stype != 0 ? (const u32 *)d->mapQ : (const u32 *)nullptr, useQ ? (const double *)d->tan_Q : (const double *)nullptr,
                   (const int *)d->At.rp, (const int *)d->At.ci, useA ? (const double *)d->tan_A : (const double *)nullptr, (const int *)c.flag,
                   (const double *)c.xu, (const double *)c.yu, c.rx);
            if (m) LAUNCH(k_tan_rhs_y, adj_grid_rows(m), m, useL ? (const double *)d->tan_l : (const double *)nullptr, useU ? (const double *)d->tan_u : (const double *)nullptr,
                          (const int *)d->Ar.rp, (const int *)d->Ar.ci, (const u32 *)d->mapA, useA ? (const double *)d->tan_A : (const double *)nullptr,
                          (const int *)c.flag, (const double *)c.xu, c.ry);
        }
        rc = c.G == 1 ? adj_sweeps(d, c, m > 0, tol, max_sweeps, code, sweep, rel) : adj_sweeps_group(d, c, cnt, m > 0, tol, max_sweeps, code, sweep, rel);
        if (rc) break;
        bool any = false;
        for (int k = 0; k < cnt; k++) {
            const long r = r0 + k;
            double *dxr = dx + (size_t)r * n, *dyr = dy + (size_t)r * m;
            if (status) { status[3 * r] = code[k]; status[3 * r + 1] = sweep[k]; status[3 * r + 2] = c.kact; }
            if (res) res[r] = rel[k];
            if (code[k] != 0) {
                for (int j = 0; j < n; j++) dxr[j] = nan;
                for (int i = 0; i < m; i++) dyr[i] = nan;
                continue;
            }
            any = true;
            adj_point(c, k);
            // the unscaled dx into rx, dy into ry (the sweeps are over)
            LAUNCH(k_tan_out, c.gnm, n, m, c.scaled, c.sc_cinv, (const double *)d->D, (const double *)d->E, (const int *)c.flag, (const double *)c.vx, (const double *)c.vy,
                   c.rx, c.ry);
            HIPCHK(hipMemcpyAsync(dxr, c.rx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
            if (m) HIPCHK(hipMemcpyAsync(dyr, c.ry, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
        }
        if (any) HIPCHK(hipStreamSynchronize(d->stream));
    }
    rc = adj_end(d, c, active, rc);
    if (rc) return rc;
    adj_book(d->tan, nrhs, c.sweeps_total, ts0);
    return 0;
}

