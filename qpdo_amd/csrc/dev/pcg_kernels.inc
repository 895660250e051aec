// pcg_kernels.inc -- part of qpdo_dev.hip (one translation unit; included in order): PCG and deflation kernels
// ------------------------------------------------------------------------------------------------
// Jacobi-PCG on K = Q + sigma_f I + A' diag(d) A.  Every kernel leaves immediately once the
// device-side `done` latch is set, so the host may launch iterations in batches and still stop
// at exactly the iteration that met the tolerance.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pcg_init(int n, const double *__restrict__ b, const double *__restrict__ dg,
                                                  double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                  double *__restrict__ p, double *__restrict__ p_rz, double *__restrict__ p_bb) {
    __shared__ double sm[32];
    double a = 0.0, c = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double bi = b[i], zi = bi / dg[i];
        x[i] = 0.0; r[i] = bi; z[i] = zi; p[i] = zi;
        a += bi * zi; c += bi * bi;
    }
    double ta = block_sum(a, sm), tc = block_sum(c, sm + 16);
    if (threadIdx.x == 0) { p_rz[blockIdx.x] = ta; p_bb[blockIdx.x] = tc; }
}
__global__ __launch_bounds__(256) void k_pcg_init2(const double *__restrict__ p_rz, int cnt_rz, const double *__restrict__ p_bb, int cnt, Ctrl *ctrl) {
    __shared__ double sm[32];
    double rz = reduce_partials(p_rz, cnt_rz, sm), bb = reduce_partials(p_bb, cnt, sm + 16);
    if (threadIdx.x == 0) {
        ctrl->val[V_RZ] = rz; ctrl->val[V_BNORM] = sqrt(bb);
        ctrl->cnt[C_PCG_DONE] = (bb == 0.0) ? 1 : 0;
        ctrl->cnt[C_PCG_IT] = 0;
    }
}
// x += alpha p ; r -= alpha Kp ; z = r/diag ; partial r.z, r.r
// p_rinf: per-block maxima of |Dinv_i r_i| (Dinv == NULL: |r_i|) -- the residual of the Newton system measured the way the
// reference measures the inner dual residual (termination.c:58-77, before the cinv factor), for the absolute stopping rule
__global__ __launch_bounds__(256) void k_pcg_update(int n, const Ctrl *__restrict__ ctrl, const double *__restrict__ p_pKp, int pcnt,
                                                    const double *__restrict__ p, const double *__restrict__ Kp,
                                                    const double *__restrict__ dg, double *__restrict__ x, double *__restrict__ r,
                                                    double *__restrict__ z, double *__restrict__ p_rz, double *__restrict__ p_rr,
                                                    const double *__restrict__ Dinv, double *__restrict__ p_rinf) {
    __shared__ double sm[48];
    if (ctrl->cnt[C_PCG_DONE]) return;
    const double pKp = reduce_partials(p_pKp, pcnt, sm);
    const double alpha = ctrl->val[V_RZ] / pKp;
    double a = 0.0, c = 0.0, mx = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Kp[i];
        r[i] = ri;
        const double zi = ri / dg[i];
        z[i] = zi;
        a += ri * zi; c += ri * ri;
        const double s = fabs(Dinv ? Dinv[i] * ri : ri);
        mx = s > mx ? s : mx;
    }
    double ta = block_sum(a, sm), tc = block_sum(c, sm + 16);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sm[32 + (threadIdx.x >> 6)] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[32];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) t = sm[32 + w] > t ? sm[32 + w] : t;
        p_rz[blockIdx.x] = ta; p_rr[blockIdx.x] = tc; p_rinf[blockIdx.x] = t;
    }
}
// scalar step: convergence latch, beta, rz roll-over (single block)
// Stopping rule: relative, ||r||_2 <= tol ||rhs||_2, OR absolute, cinv * max_i |Dinv_i r_i| <= abs_floor -- the latter is the
// unscaled inf-norm in which the reference measures the inner dual residual this Newton residual turns into
// (termination.c:58-77); abs_floor = 1e-5 eps_abs sits four orders below the smallest tolerance the driver ever compares that
// norm with (0.1 eps_abs, qpdo.c:408).  Late passes have right-hand sides of 1e-6 and below: the relative rule alone asks
// them for absolute residuals of 1e-18.
// phase 0: both halves (the Jacobi / deflated path).  The Schur-complement mode splits them around its preconditioner application, which
// is a whole inner solve: phase 1 right after the update -- iteration count, residual norms, the convergence latch; the host looks at the
// latch BEFORE it pays for an inner solve whose result a converged iteration would throw away -- and phase 2 after it: beta, rz roll-over.
__global__ __launch_bounds__(256) void k_pcg_scalar(Ctrl *ctrl, const double *__restrict__ p_rz, int cnt_rz, const double *__restrict__ p_rr,
                                                    int cnt, double tol, const double *__restrict__ p_rinf, double cinv, double abs_floor, int phase = 0) {
    __shared__ double sm[48];
    if (ctrl->cnt[C_PCG_DONE]) return;
    if (phase == 2) {
        const double rz2b = reduce_partials(p_rz, cnt_rz, sm);
        if (threadIdx.x == 0) { ctrl->val[V_RR] = rz2b / ctrl->val[V_RZ]; ctrl->val[V_RZ] = rz2b; }
        return;
    }
    const double rz2 = phase == 1 ? 0.0 : reduce_partials(p_rz, cnt_rz, sm), rr = reduce_partials(p_rr, cnt, sm + 16);
    double mx = 0.0;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const double v = p_rinf[i]; mx = v > mx ? v : mx; }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sm[32 + (threadIdx.x >> 6)] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double rinf = sm[32];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) rinf = sm[32 + w] > rinf ? sm[32 + w] : rinf;
        rinf *= cinv;
        ctrl->cnt[C_PCG_IT] += 1;
        ctrl->val[V_RNORM] = sqrt(rr);
        ctrl->val[V_RINF] = rinf;
        if (sqrt(rr) <= tol * ctrl->val[V_BNORM] || rinf <= abs_floor || !(rr == rr)) ctrl->cnt[C_PCG_DONE] = 1;
        if (phase == 0) {
            ctrl->val[V_RR] = rz2 / ctrl->val[V_RZ];     // beta
            ctrl->val[V_RZ] = rz2;
        }
    }
}
__global__ void k_pcg_p(int n, const Ctrl *__restrict__ ctrl, const double *__restrict__ z, double *__restrict__ p) {
    if (ctrl->cnt[C_PCG_DONE]) return;
    const double beta = ctrl->val[V_RR];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = z[i] + beta * p[i];
}


// ------------------------------------------------------------------------------------------------
// Single-reduction (Chronopoulos-Gear) Jacobi-PCG for the inner system of the Schur-complement mode,
//     S' s = v,   S' = D^-1 + A_c Dq^-1 A_c'   (k x k, never formed; rank r owns k_loc of its rows).
// One iteration = ONE vector kernel (k_cgcg_step) + the two products of S' u:
//     p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  u = r ./ diag        (k_cgcg_step)
//     tn = A_c' u (all-reduced over the ranks);  t = tn ./ Dq                              (product 1)
//     w = u ./ d + A_c t                                                                    (product 2)
//     gamma = (r,u);  delta = (w,u) = sum u^2/d + sum tn t;  beta' = gamma/gamma_old;  alpha' = gamma / (delta - beta' gamma / alpha)
// Every scalar is known right after product 1: (r,u), (r,r) and sum u^2/d are local partial sums formed by k_cgcg_step
// BEFORE the product (single GPU: re-reduced in fixed order by the next k_cgcg_step; multi GPU: three doubles appended
// to the n-vector payload of the one all-reduce), and sum tn t is a dot of the replicated n-vector that every rank
// computes identically.  Hence 3 launches per iteration on one GPU (was 5) and exactly one collective per iteration
// on several, with the k-vectors partitioned.  Partial-sum arrays and the (gamma, alpha) state are double-buffered
// by the parity of the host-supplied iteration index j, because blocks of one launch read what another block of the
// same launch must not overwrite.  All reductions run in a fixed order: bitwise reproducible.
// ------------------------------------------------------------------------------------------------
enum { VS_GAM = 11, VS_ALP = 13 };      // ctrl->val slots (two each, by parity) of the inner solver's control block
__global__ __launch_bounds__(256) void k_cgcg_init(int k, const double *__restrict__ b, const double *__restrict__ dg, const double *__restrict__ dc,
                                                   double *__restrict__ x, double *__restrict__ r, double *__restrict__ u, double *__restrict__ p,
                                                   double *__restrict__ s, double *__restrict__ P3 /* [3][2][PGRID], slot 0 written */, Ctrl *ctrl) {
    __shared__ double sm[48];
    double a = 0.0, c = 0.0, e = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        const double bi = b[i], ui = bi / dg[i];
        x[i] = 0.0; r[i] = bi; u[i] = ui; p[i] = 0.0; s[i] = 0.0;
        a += bi * ui; c += bi * bi; e += ui * ui / dc[i];
    }
    const double ta = block_sum(a, sm), tc = block_sum(c, sm + 16), te = block_sum(e, sm + 32);
    if (threadIdx.x == 0) {
        P3[0 * 2 * PGRID + blockIdx.x] = ta; P3[1 * 2 * PGRID + blockIdx.x] = tc; P3[2 * 2 * PGRID + blockIdx.x] = te;
        if (blockIdx.x == 0) { ctrl->cnt[C_PCG_DONE] = 0; ctrl->cnt[C_PCG_IT] = 0; ctrl->val[V_RNORM] = 0.0; }
    }
}
// sums of the three local partial arrays of parity `par` -> out[0..3) (multi GPU: appended to the all-reduce payload)
__global__ __launch_bounds__(256) void k_cgcg_pack3(const int *__restrict__ done, const double *__restrict__ P3, int par, int cnt, double *__restrict__ out) {
    __shared__ double sm[48];
    if (done && *done) return;
    const double a = reduce_partials(P3 + (0 * 2 + par) * PGRID, cnt, sm), c = reduce_partials(P3 + (1 * 2 + par) * PGRID, cnt, sm + 16),
                 e = reduce_partials(P3 + (2 * 2 + par) * PGRID, cnt, sm + 32);
    if (threadIdx.x == 0) { out[0] = a; out[1] = c; out[2] = e; }
}
__global__ __launch_bounds__(256) void k_cgcg_step(int k, int j, Ctrl *ctrl, const double *__restrict__ glob3, double *__restrict__ P3, int pcnt,
                                                   const double *__restrict__ Pf, int fcnt, const double *__restrict__ w, const double *__restrict__ dg,
                                                   const double *__restrict__ dc, double *__restrict__ x, double *__restrict__ r, double *__restrict__ u,
                                                   double *__restrict__ p, double *__restrict__ s, double tol) {
    __shared__ double sm[32];
    // The latch holds (index of the launch that set it) + 1.  Only a latch set by an EARLIER launch ends this one at the top:
    // block 0 of this very launch may set it below while other waves are still here, and a workgroup whose waves split on it
    // would reduce over missing partials.  The in-launch exit further down is uniform -- every block derives rn from the same
    // read-only partial sums.
    { const int dn = ctrl->cnt[C_PCG_DONE]; if (dn && dn <= j) return; }
    const int par = j & 1;
    // The vector operands do not depend on the scalars: the grid covers k with one element per thread (k <= PGRID * 256), so
    // their loads are issued first and are in flight while the partial sums are re-reduced.
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool own = i < k && (int)(gridDim.x * blockDim.x) >= k;
    double ui = 0.0, pi0 = 0.0, wi = 0.0, si0 = 0.0, xi = 0.0, ri0 = 0.0, dgi = 1.0, dci = 1.0;
    if (own) { ui = u[i]; pi0 = p[i]; wi = w[i]; si0 = s[i]; xi = x[i]; ri0 = r[i]; dgi = dg[i]; dci = dc[i]; }
    double gam = 0.0, rr = 0.0, e = 0.0, f = 0.0;
    if (glob3) { gam = glob3[0]; rr = glob3[1]; e = glob3[2]; }
    else for (int q = threadIdx.x; q < pcnt; q += blockDim.x) { gam += P3[(0 * 2 + par) * PGRID + q]; rr += P3[(1 * 2 + par) * PGRID + q]; e += P3[(2 * 2 + par) * PGRID + q]; }
    for (int q = threadIdx.x; q < fcnt; q += blockDim.x) f += Pf[q];
    if (glob3) { double z0 = 0.0, z1 = 0.0, z2 = 0.0; block_sum4(z0, z1, z2, f, sm); }
    else block_sum4(gam, rr, e, f, sm);
    const double delta = e + f;                                  // (w,u) = u' D^-1 u + tn' Dq^-1 tn
    const double rn = sqrt(rr);
    const double bnorm = (j == 0) ? rn : ctrl->val[V_BNORM];
    if (rn <= tol * bnorm || !(rr == rr)) {                      // converged (or NaN: the host tells them apart from V_RNORM)
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl->cnt[C_PCG_DONE] = j + 1; ctrl->val[V_RNORM] = rn; if (j == 0) ctrl->val[V_BNORM] = bnorm; }
        return;
    }
    const double beta = (j == 0) ? 0.0 : gam / ctrl->val[VS_GAM + par];
    const double alpha = (j == 0) ? gam / delta : gam / (delta - beta * gam / ctrl->val[VS_ALP + par]);
    double a = 0.0, c = 0.0, e2 = 0.0, zero = 0.0;
    if (own) {
        const double pi = ui + beta * pi0, si = wi + beta * si0;
        p[i] = pi; s[i] = si;
        x[i] = xi + alpha * pi;
        const double ri = ri0 - alpha * si;
        r[i] = ri;
        const double un = ri / dgi;
        u[i] = un;
        a = ri * un; c = ri * ri; e2 = un * un / dci;
    } else if ((int)(gridDim.x * blockDim.x) < k) {              // (not reached with vgrid(k) for k <= 262144; kept for generality)
        for (int q = i; q < k; q += gridDim.x * blockDim.x) {
            const double uq = u[q];
            const double pq = uq + beta * p[q], sq = w[q] + beta * s[q];
            p[q] = pq; s[q] = sq;
            x[q] += alpha * pq;
            const double rq = r[q] - alpha * sq;
            r[q] = rq;
            const double un = rq / dg[q];
            u[q] = un;
            a += rq * un; c += rq * rq; e2 += un * un / dc[q];
        }
    }
    block_sum4(a, c, e2, zero, sm);
    if (threadIdx.x == 0) {
        const int np = par ^ 1;
        P3[(0 * 2 + np) * PGRID + blockIdx.x] = a; P3[(1 * 2 + np) * PGRID + blockIdx.x] = c; P3[(2 * 2 + np) * PGRID + blockIdx.x] = e2;
        if (blockIdx.x == 0) {
            ctrl->val[VS_GAM + np] = gam; ctrl->val[VS_ALP + np] = alpha;
            ctrl->cnt[C_PCG_IT] += 1; ctrl->val[V_RNORM] = rn;
            if (j == 0) ctrl->val[V_BNORM] = bnorm;
        }
    }
}

// The inner CG's vector step folded into its two products (QPDO_INNER_FOLD=0: k_cgcg_step between them, as before; same bits).
// Product 1 of application j: before its own rows, workgroup b forms the partial sums of the step that the previous launch performed --
// sum r.u, sum r.r, sum u^2/d over the 256-element blocks b, b + gridDim, ... of the k-vectors, with the per-element expressions and the
// block_sum4 tree of k_cgcg_step -- into P3[.][np][block] (P3 == nullptr: the application after k_cgcg_init, whose slot 0 is filled).
struct EpiDivDotSums {
    const double *w; double *out, *p_f;
    int k, np; const double *r, *u, *dc; double *P3;
    double acc = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ bool prologue(double *sm) {
        if (!P3) return true;
        const int nblk = (k + 255) >> 8;
        for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
            const int i = blk * 256 + (int)threadIdx.x;
            double a = 0.0, c = 0.0, e2 = 0.0, zero = 0.0;
            if (threadIdx.x < 256 && i < k) { const double ri = r[i], un = u[i]; a = ri * un; c = ri * ri; e2 = un * un / dc[i]; }
            block_sum4_256(a, c, e2, zero, sm);
            if (threadIdx.x == 0) { P3[(0 * 2 + np) * PGRID + blk] = a; P3[(1 * 2 + np) * PGRID + blk] = c; P3[(2 * 2 + np) * PGRID + blk] = e2; }
        }
        return true;
    }
    __device__ void row(int r_, double s) { const double t = s / w[r_]; out[r_] = t; acc += s * t; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_f[blockIdx.x] = t;
    }
};
// Product 2 of application j - 1 performs step j: at its top every workgroup re-reduces the partial sums P3[.][par][0..pcnt) and
// Pf[0..fcnt) in the order of k_cgcg_step (its first 256 threads are one block of that kernel), derives rn, the convergence test,
// beta and alpha with that kernel's expressions, and leaves alpha and beta in LDS; then, per owned row, w_i = u_i / d_i + (A_c t)_i
// as EpiSchurW and the five updates and u_i = r_i / diag_i in k_cgcg_step's order.  w never goes to memory; u is read by this launch
// for the workgroup's own rows only (its x is t), so it is written in place.  Converged or NaN: every workgroup leaves (the decision
// is the same in all of them), workgroup 0 sets the latch to j + 1.  Only a latch set by an EARLIER launch ends this one at its top,
// so the kernel's own `done` argument is nullptr for this functor.
struct EpiSchurStep {
    int j; Ctrl *ctrl; const double *P3; int pcnt; const double *Pf; int fcnt;
    const double *dg, *dc; double *x, *r, *u, *p, *s; double tol;
    const double *ab = nullptr;                 // alpha, beta in LDS
    __device__ bool skip(int) const { return false; }
    __device__ bool prologue(double *sm) {
        { const int dn = ctrl->cnt[C_PCG_DONE]; if (dn && dn <= j) return false; }
        const int par = j & 1;
        double gam = 0.0, rr = 0.0, e = 0.0, f = 0.0;
        if (threadIdx.x < 256) {
            for (int q = threadIdx.x; q < pcnt; q += 256) { gam += P3[(0 * 2 + par) * PGRID + q]; rr += P3[(1 * 2 + par) * PGRID + q]; e += P3[(2 * 2 + par) * PGRID + q]; }
            for (int q = threadIdx.x; q < fcnt; q += 256) f += Pf[q];
        }
        block_sum4_256(gam, rr, e, f, sm);
        const double delta = e + f;
        const double rn = sqrt(rr);
        const double bnorm = (j == 0) ? rn : ctrl->val[V_BNORM];
        const bool first = blockIdx.x == 0 && threadIdx.x == 0;
        if (rn <= tol * bnorm || !(rr == rr)) {
            if (first) { ctrl->cnt[C_PCG_DONE] = j + 1; ctrl->val[V_RNORM] = rn; if (j == 0) ctrl->val[V_BNORM] = bnorm; }
            return false;
        }
        const double beta = (j == 0) ? 0.0 : gam / ctrl->val[VS_GAM + par];
        const double alpha = (j == 0) ? gam / delta : gam / (delta - beta * gam / ctrl->val[VS_ALP + par]);
        if (threadIdx.x == 0) { sm[16] = alpha; sm[17] = beta; }
        if (first) {
            const int np = par ^ 1;
            ctrl->val[VS_GAM + np] = gam; ctrl->val[VS_ALP + np] = alpha;
            ctrl->cnt[C_PCG_IT] += 1; ctrl->val[V_RNORM] = rn;
            if (j == 0) ctrl->val[V_BNORM] = bnorm;
        }
        ab = sm + 16;
        __syncthreads();
        return true;
    }
    __device__ void row(int i, double acc) {
        const double alpha = ab[0], beta = ab[1];
        const double ui = u[i];
        const double wi = ui / dc[i] + acc;
        const double pi = ui + beta * p[i], si = wi + beta * s[i];
        p[i] = pi; s[i] = si;
        x[i] = x[i] + alpha * pi;
        const double ri = r[i] - alpha * si;
        r[i] = ri;
        u[i] = ri / dg[i];
    }
    __device__ void finish(double *) {}
};

// ------------------------------------------------------------------------------------------------
// Heavy-row deflation of the Jacobi preconditioner.  After a penalty update a handful of rows carry
// weights d_i 1e4..1e6 times the median; they add isolated huge eigenvalues that cost Jacobi-PCG
// thousands of iterations.  M = P + A_h' D_h A_h treats the (<= 64) heaviest rows exactly, with P the
// Jacobi diagonal of the remainder:  M^-1 r = u - P^-1 A_h' S^-1 A_h u,  u = P^-1 r,
// S = D_h^-1 + A_h P^-1 A_h'  (Woodbury; S is <= 64 x 64 and is inverted on the host once per pass).
// The solution of K dx = rhs is unchanged; only the iteration count drops.
// ------------------------------------------------------------------------------------------------
static const int DEFL_MAX = 256;
// hist[b] = #{ i : dmax/2^(b+1) < d_i <= dmax/2^b },  b = 0..31
__global__ __launch_bounds__(256) void k_defl_hist(int m, const double *__restrict__ dw, const Ctrl *ctrl, int *__restrict__ hist) {
    __shared__ int lh[32];
    if (threadIdx.x < 32) lh[threadIdx.x] = 0;
    __syncthreads();
    const double dmax = __longlong_as_double((long long)ctrl->nrm[N_A]);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const double v = dw[i];
        if (v > 0.0) {
            int b = 0; double t = dmax;
            while (b < 31 && v <= t * 0.5) { t *= 0.5; b++; }
            atomicAdd(&lh[b], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}
// ordered selection of rows with d_i > thr (single block): list, indicator flag, remainder weights
__global__ __launch_bounds__(1024) void k_defl_select(int m, const double *__restrict__ dw, double thr, double *__restrict__ flag,
                                                      double *__restrict__ dlight, int *__restrict__ list, int *__restrict__ count) {
    __shared__ int sums[1024];
    const int chunk = (m + 1023) / 1024;
    const int beg = threadIdx.x * chunk, end = min(beg + chunk, m);
    int c = 0;
    for (int i = beg; i < end; i++) c += (dw[i] > thr);
    sums[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < 1024; i++) { int t = sums[i]; sums[i] = run; run += t; } *count = run; }
    __syncthreads();
    int pos = sums[threadIdx.x];
    for (int i = beg; i < end; i++) {
        const bool h = dw[i] > thr;
        flag[i] = h ? 1.0 : 0.0;
        dlight[i] = h ? 0.0 : dw[i];
        if (h) { if (pos < DEFL_MAX) list[pos] = i; pos++; }
    }
}
// S(a,b) = [a==b]/d_a + sum_c A(h_a,c) A(h_b,c) / P_c ; one wave per pair, binary search in the sorted row b
__global__ __launch_bounds__(64) void k_defl_S(int r, const int *__restrict__ list, const int *__restrict__ arp, const int *__restrict__ aci,
                                               const double *__restrict__ aval, const double *__restrict__ P, const double *__restrict__ dw,
                                               double *__restrict__ S) {
    const int a = blockIdx.x, b = blockIdx.y;
    if (a >= r || b > a) return;
    const int ra = list[a], rb = list[b];
    const int b0 = arp[rb], b1 = arp[rb + 1];
    double sacc = 0.0;
    for (int e = arp[ra] + threadIdx.x; e < arp[ra + 1]; e += 64) {
        const int c = aci[e];
        int lo = b0, hi = b1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (aci[mid] < c) lo = mid + 1; else hi = mid; }
        if (lo < b1 && aci[lo] == c) sacc += aval[e] * aval[lo] / P[c];
    }
    sacc = wave_sum(sacc);
    if (threadIdx.x == 0) {
        if (a == b) sacc += 1.0 / dw[ra];
        S[a * DEFL_MAX + b] = sacc; S[b * DEFL_MAX + a] = sacc;
    }
}
// v_a = A(h_a,:) u ; one wave per heavy row
__global__ __launch_bounds__(64) void k_defl_v(const int *__restrict__ done, int r, const int *__restrict__ list, const int *__restrict__ arp,
                                               const int *__restrict__ aci, const double *__restrict__ aval, const double *__restrict__ u,
                                               double *__restrict__ v) {
    if (done && *done) return;
    const int a = blockIdx.x;
    if (a >= r) return;
    const int row = list[a];
    double sacc = 0.0;
    for (int e = arp[row] + threadIdx.x; e < arp[row + 1]; e += 64) sacc += aval[e] * u[aci[e]];
    sacc = wave_sum(sacc);
    if (threadIdx.x == 0) v[a] = sacc;
}
// w = S^-1 v (explicit inverse, row per lane), scattered to the m-vector th at the heavy rows
__global__ __launch_bounds__(256) void k_defl_w(const int *__restrict__ done, int r, const double *__restrict__ Sinv, const double *__restrict__ v,
                                               const int *__restrict__ list, double *__restrict__ th) {
    if (done && *done) return;
    const int a = threadIdx.x;
    if (a >= r) return;
    double sacc = 0.0;
    for (int b = 0; b < r; b++) sacc += Sinv[b * DEFL_MAX + a] * v[b];      // S^-1 is symmetric: read it along the lanes
    th[list[a]] = sacc;
}
struct EpiDeflZ {                          // z = u - (A_h' w) ./ P ; partial r.z
    const double *P, *r; double *z, *p_rz; double acc = 0.0;
    __device__ bool skip(int) const { return false; }
    __device__ void row(int j, double s) { const double zj = z[j] - s / P[j]; z[j] = zj; acc += r[j] * zj; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_rz[blockIdx.x] = t;
    }
};
__global__ void k_copy(int n, const double *__restrict__ a, double *__restrict__ b) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) b[i] = a[i];
}

