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
    const double ta = block_sum(a, sm), tc = block_sum(c, sm + 16), t = block_max(mx, sm + 32);
    if (threadIdx.x == 0) { p_rz[blockIdx.x] = ta; p_rr[blockIdx.x] = tc; p_rinf[blockIdx.x] = t; }
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
    const double rinf = block_max(mx, sm + 32) * cinv;
    if (threadIdx.x == 0) {
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
// Iteration j is step j followed by one application of S' to the new u:
//     p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  u = r ./ diag        (step)
//     tn = A_c' u (all-reduced over the ranks);  t = tn ./ Dq                              (product 1)
//     w = u ./ d + A_c t                                                                    (product 2)
//     gamma = (r,u);  delta = (w,u) = sum u^2/d + sum tn t;  beta = gamma/gamma_old;  alpha = gamma / (delta - beta gamma / alpha_old)
// Every scalar of step j is known right after product 1 of the application before it: (r,u), (r,r) and sum u^2/d are per-block
// partial sums over the 256-element blocks of the k-vectors (single GPU: P3, re-reduced in fixed order by every workgroup of the
// step; several GPUs: their three totals ride at the end of the n-vector payload of the one all-reduce, glob3), and sum tn t (Pf)
// is a dot of the replicated n-vector that every rank computes identically: one collective per iteration, the k-vectors partitioned.
// Partial-sum arrays and the (gamma, alpha) state are double-buffered by the parity of the host-supplied index j, because
// workgroups of one launch read what another workgroup of the same launch must not overwrite.  All reductions run in a fixed
// order: bitwise reproducible, and the same bits from both schedules --
//     three launches: k_cgcg_step, product 1 (EpiDivDot), product 2 (EpiSchurW);
//     two launches (single GPU, either value width of the matrix stream, k <= PGRID * 256): product 2 performs the step behind its rows (EpiSchurStep) and
//     product 1 forms the step's partial sums in front of its own (EpiDivDotSums) --
// because both are built from the same three functions: cgcg_scalars, cgcg_elem, cgcg_sums (+ cgcg_put3).
// ------------------------------------------------------------------------------------------------
enum { VS_GAM = 11, VS_ALP = 13 };      // ctrl->val slots (two each, by parity) of the inner solver's control block
// the three per-element terms of (r,u), (r,r), sum u^2/d
__device__ __forceinline__ void cgcg_sums(double ri, double ui, double dci, double &a, double &c, double &e) { a = ri * ui; c = ri * ri; e = ui * ui / dci; }
// block sums of the three terms (first 256 threads of the workgroup) -> P3[.][par][blk]     (P3: [3 sums][2 parities][PGRID])
__device__ __forceinline__ void cgcg_put3(double a, double c, double e, double *__restrict__ P3, int par, int blk, double *sm) {
    double zero = 0.0;
    block_sum4_256(a, c, e, zero, sm);
    if (threadIdx.x == 0) { P3[(0 * 2 + par) * PGRID + blk] = a; P3[(1 * 2 + par) * PGRID + blk] = c; P3[(2 * 2 + par) * PGRID + blk] = e; }
}
// Element i of the step, operands in registers (the caller decides when they are loaded); leaves the new r_i, u_i in ri, un.
// u32 (or null): the fp32 copy of u that the pair-wide fp32 product stages (spmv.inc, XT = float), written where u is.
__device__ __forceinline__ void cgcg_elem(int i, double alpha, double beta, double ui, double wi, double pi0, double si0, double xi, double ri0, double dgi,
                                          double *x, double *r, double *u, double *p, double *s, double &ri, double &un, float *u32) {
    const double pi = ui + beta * pi0, si = wi + beta * si0;
    p[i] = pi; s[i] = si;
    x[i] = xi + alpha * pi;
    ri = ri0 - alpha * si;
    r[i] = ri;
    un = ri / dgi;
    u[i] = un;
    if (u32) u32[i] = (float)un;
}
// The scalar part of step j, run by every workgroup of the launch that performs it (its first 256 threads reduce; all threads get
// the result).  false: no step -- an EARLIER launch has latched (the latch holds the index of the launch that set it, + 1), or the
// residual has converged or is NaN (the host tells them apart from V_RNORM), which workgroup 0 latches here.  Only an earlier
// launch's latch may end a workgroup at the top: workgroup 0 of this very launch may set it while other waves are still there, and
// a workgroup whose waves split on it would reduce over missing partials; the in-launch exit is uniform, because every workgroup
// derives rn from the same read-only sums.  true: alpha and beta of the step, and workgroup 0 has published gamma, alpha (next
// parity), the iteration count and the norms.  It does so before the element updates of the launch: the slots other workgroups
// still read are those of this parity, and V_BNORM is only written at j == 0, where nobody reads it.
// glob3 (row-partitioned): the three k-sums arrive reduced over the ranks, only f is summed here.  sm: >= 16 doubles.
__device__ __forceinline__ bool cgcg_scalars(int j, Ctrl *ctrl, const double *__restrict__ glob3, const double *P3, int pcnt, const double *__restrict__ Pf, int fcnt,
                                             double tol, double *sm, double &alpha, double &beta) {
    { const int dn = ctrl->cnt[C_PCG_DONE]; if (dn && dn <= j) return false; }
    const int par = j & 1;
    double gam = 0.0, rr = 0.0, e = 0.0, f = 0.0;
    if (threadIdx.x < 256) {
        if (!glob3) for (int q = threadIdx.x; q < pcnt; q += 256) { gam += P3[(0 * 2 + par) * PGRID + q]; rr += P3[(1 * 2 + par) * PGRID + q]; e += P3[(2 * 2 + par) * PGRID + q]; }
        for (int q = threadIdx.x; q < fcnt; q += 256) f += Pf[q];
    }
    if (glob3) { double z0 = 0.0, z1 = 0.0, z2 = 0.0; block_sum4_256(z0, z1, z2, f, sm); gam = glob3[0]; rr = glob3[1]; e = glob3[2]; }
    else block_sum4_256(gam, rr, e, f, sm);
    const double delta = e + f;                                  // (w,u) = u' D^-1 u + tn' Dq^-1 tn
    const double rn = sqrt(rr);
    const double bnorm = (j == 0) ? rn : ctrl->val[V_BNORM];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (rn <= tol * bnorm || !(rr == rr)) {
        if (first) { ctrl->cnt[C_PCG_DONE] = j + 1; ctrl->val[V_RNORM] = rn; if (j == 0) ctrl->val[V_BNORM] = bnorm; }
        return false;
    }
    beta = (j == 0) ? 0.0 : gam / ctrl->val[VS_GAM + par];
    alpha = (j == 0) ? gam / delta : gam / (delta - beta * gam / ctrl->val[VS_ALP + par]);
    if (first) {
        const int np = par ^ 1;
        ctrl->val[VS_GAM + np] = gam; ctrl->val[VS_ALP + np] = alpha;
        ctrl->cnt[C_PCG_IT] += 1; ctrl->val[V_RNORM] = rn;
        if (j == 0) ctrl->val[V_BNORM] = bnorm;
    }
    return true;
}
__global__ __launch_bounds__(256) void k_cgcg_init(int k, const double *__restrict__ b, const double *__restrict__ dg, const double *__restrict__ dc,
                                                   double *__restrict__ x, double *__restrict__ r, double *__restrict__ u, double *__restrict__ p,
                                                   double *__restrict__ s, double *__restrict__ P3 /* slot 0 written */, Ctrl *ctrl,
                                                   float *__restrict__ u32 /* or null: cgcg_elem */) {
    __shared__ double sm[16];
    double a = 0.0, c = 0.0, e = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        const double bi = b[i], ui = bi / dg[i];
        x[i] = 0.0; r[i] = bi; u[i] = ui; p[i] = 0.0; s[i] = 0.0;
        if (u32) u32[i] = (float)ui;
        double ta, tc, te;
        cgcg_sums(bi, ui, dc[i], ta, tc, te);
        a += ta; c += tc; e += te;
    }
    cgcg_put3(a, c, e, P3, 0, blockIdx.x, sm);
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl->cnt[C_PCG_DONE] = 0; ctrl->cnt[C_PCG_IT] = 0; ctrl->val[V_RNORM] = 0.0; }
}
// ---- refinement of the inner solve (schur_inner_solve): the CG above runs on the fp32 copies of the matrices and only proposes
// corrections; these three kernels keep the solution and form the residual that accepts it, all in fp64 ----
// sol = e (first sweep) or sol += e
__global__ __launch_bounds__(256) void k_refine_acc(int k, int first, const double *__restrict__ e, double *__restrict__ sol) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) sol[i] = first ? e[i] : sol[i] + e[i];
}
// rho = b - w, w = S' sol formed with the fp64 matrices, as the right-hand side of the next sweep: k_cgcg_init with rho for b -- the CG
// state of the sweep and the three partial sums of its step 0 in cgcg_put3's fixed order, (rho, rho) among them
__global__ __launch_bounds__(256) void k_refine_init(int k, const double *__restrict__ b, const double *__restrict__ w, const double *__restrict__ dg,
                                                     const double *__restrict__ dc, double *__restrict__ x, double *__restrict__ r, double *__restrict__ u,
                                                     double *__restrict__ p, double *__restrict__ s, double *__restrict__ P3 /* slot 0 written */,
                                                     float *__restrict__ u32 /* or null: cgcg_elem */) {
    __shared__ double sm[16];
    double a = 0.0, c = 0.0, e = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        const double bi = b[i] - w[i], ui = bi / dg[i];
        x[i] = 0.0; r[i] = bi; u[i] = ui; p[i] = 0.0; s[i] = 0.0;
        if (u32) u32[i] = (float)ui;
        double ta, tc, te;
        cgcg_sums(bi, ui, dc[i], ta, tc, te);
        a += ta; c += tc; e += te;
    }
    cgcg_put3(a, c, e, P3, 0, blockIdx.x, sm);
}
// ||rho||_2 from those partial sums -> V_RNORM, and the control block as k_cgcg_init leaves it for the sweep
__global__ __launch_bounds__(256) void k_refine_norm(const double *__restrict__ P3, int cnt, Ctrl *ctrl) {
    __shared__ double sm[16];
    const double rr = reduce_partials(P3 + (1 * 2 + 0) * PGRID, cnt, sm);
    if (threadIdx.x == 0) { ctrl->cnt[C_PCG_DONE] = 0; ctrl->cnt[C_PCG_IT] = 0; ctrl->val[V_RNORM] = sqrt(rr); }
}
// sums of the three local partial arrays of parity `par` -> out[0..3) (multi GPU: appended to the all-reduce payload)
__global__ __launch_bounds__(256) void k_cgcg_pack3(const int *__restrict__ done, const double *__restrict__ P3, int par, int cnt, double *__restrict__ out) {
    __shared__ double sm[48];
    if (done && *done) return;
    const double a = reduce_partials(P3 + (0 * 2 + par) * PGRID, cnt, sm), c = reduce_partials(P3 + (1 * 2 + par) * PGRID, cnt, sm + 16),
                 e = reduce_partials(P3 + (2 * 2 + par) * PGRID, cnt, sm + 32);
    if (threadIdx.x == 0) { out[0] = a; out[1] = c; out[2] = e; }
}
// Step j as a launch of its own; w = S' u from the application before it.
__global__ __launch_bounds__(256) void k_cgcg_step(int k, int j, Ctrl *ctrl, const double *__restrict__ glob3, double *__restrict__ P3, int pcnt,
                                                   const double *__restrict__ Pf, int fcnt, const double *__restrict__ w, const double *__restrict__ dg,
                                                   const double *__restrict__ dc, double *__restrict__ x, double *__restrict__ r, double *__restrict__ u,
                                                   double *__restrict__ p, double *__restrict__ s, double tol, float *__restrict__ u32) {
    __shared__ double sm[16];
    // The vector operands do not depend on the scalars: when the grid covers k with one element per thread (k <= PGRID * 256)
    // their loads are issued first and are in flight while the partial sums are re-reduced.
    const int i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    const bool own = i < k && stride >= k;
    double ui = 0.0, pi0 = 0.0, wi = 0.0, si0 = 0.0, xi = 0.0, ri0 = 0.0, dgi = 1.0, dci = 1.0;
    if (own) { ui = u[i]; pi0 = p[i]; wi = w[i]; si0 = s[i]; xi = x[i]; ri0 = r[i]; dgi = dg[i]; dci = dc[i]; }
    double alpha, beta;
    if (!cgcg_scalars(j, ctrl, glob3, P3, pcnt, Pf, fcnt, tol, sm, alpha, beta)) return;
    double a = 0.0, c = 0.0, e = 0.0, ri, un;
    if (own) {
        cgcg_elem(i, alpha, beta, ui, wi, pi0, si0, xi, ri0, dgi, x, r, u, p, s, ri, un, u32);
        cgcg_sums(ri, un, dci, a, c, e);
    } else if (stride < k) {                                     // (not reached with vgrid(k) for k <= 262144; the fold is off beyond)
        for (int q = i; q < k; q += stride) {
            double ta, tc, te;
            cgcg_elem(q, alpha, beta, u[q], w[q], p[q], s[q], x[q], r[q], dg[q], x, r, u, p, s, ri, un, u32);
            cgcg_sums(ri, un, dc[q], ta, tc, te);
            a += ta; c += tc; e += te;
        }
    }
    cgcg_put3(a, c, e, P3, (j & 1) ^ 1, blockIdx.x, sm);
}

// Product 1 of the two-launch schedule.  Before its own rows, workgroup b forms the partial sums of the step that the launch
// before it performed, over the 256-element blocks b, b + gridDim, ... of the k-vectors (its first 256 threads are one block of
// k_cgcg_step), into P3[.][np][block].  P3 == nullptr: the application after k_cgcg_init, whose slot 0 is filled.
struct EpiDivDotSums {
    const double *w; double *out, *p_f;
    int k, np; const double *r, *u, *dc; double *P3;
    double acc = 0.0;
    float *out32 = nullptr;                     // the fp32 copy of t for the pair-wide fp32 product that follows, or null
    __device__ bool skip(int) const { return false; }
    __device__ bool prologue(double *sm) {
        if (!P3) return true;
        const int nblk = (k + 255) >> 8;
        for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
            const int i = blk * 256 + (int)threadIdx.x;
            double a = 0.0, c = 0.0, e = 0.0;
            if (threadIdx.x < 256 && i < k) cgcg_sums(r[i], u[i], dc[i], a, c, e);
            cgcg_put3(a, c, e, P3, np, blk, sm);
        }
        return true;
    }
    __device__ void row(int r_, double s) { const double t = s / w[r_]; out[r_] = t; if (out32) out32[r_] = (float)t; acc += s * t; }
    __device__ void finish(double *sm) {
        double t = block_sum(acc, sm);
        if (threadIdx.x == 0) p_f[blockIdx.x] = t;
    }
};
// Product 2 of the two-launch schedule: application j - 1 performs step j.  At its top every workgroup runs cgcg_scalars and
// leaves alpha and beta in LDS; then, per owned row, w_i = u_i / d_i + (A_c t)_i as EpiSchurW and the element step.  w never goes
// to memory; u is read by this launch for the workgroup's own rows only (its x is t), so it is written in place.  The kernel's own
// `done` argument is nullptr for this functor: cgcg_scalars decides which latch may end the launch.
struct EpiSchurStep {
    int j; Ctrl *ctrl; const double *P3; int pcnt; const double *Pf; int fcnt;
    const double *dg, *dc; double *x, *r, *u, *p, *s; double tol;
    const double *ab = nullptr;                 // alpha, beta in LDS
    float *u32 = nullptr;                       // cgcg_elem
    __device__ bool skip(int) const { return false; }
    __device__ bool prologue(double *sm) {
        double alpha, beta;
        if (!cgcg_scalars(j, ctrl, nullptr, P3, pcnt, Pf, fcnt, tol, sm, alpha, beta)) return false;
        if (threadIdx.x == 0) { sm[16] = alpha; sm[17] = beta; }
        ab = sm + 16;
        __syncthreads();
        return true;
    }
    __device__ void row(int i, double acc) {
        const double ui = u[i], wi = ui / dc[i] + acc;
        double ri, un;
        cgcg_elem(i, ab[0], ab[1], ui, wi, p[i], s[i], x[i], r[i], dg[i], x, r, u, p, s, ri, un, u32);
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

