// host_probe.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C): measurement and parity entry points -- kernels and solvers driven on their own, for the benchmarks and the tests
static DevCsr *mat_by_id(QpdoDev *d, int which) { return which == 0 ? &d->Ar : which == 1 ? &d->At : &d->Qf; }

int qdev_bench_spmv(QpdoDev *d, int which, int reps, double *avg_seconds, double *alg_bytes) {
    HIPCHK(hipSetDevice(d->device));
    DevCsr *M = mat_by_id(d, which);
    double *xin = (M->ncols == d->n) ? d->pc_p : d->pc_t;
    double *yout = (M->nrows == d->n) ? d->pc_Kp : d->tmp_m;
    LAUNCH(k_fill, vgrid(M->ncols), M->ncols, 1.0, xin);
    launch_spmv(d, *M, xin, EpiStore{yout}, false);     // warm-up
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    for (int r = 0; r < reps; r++) launch_spmv(d, *M, xin, EpiStore{yout}, false);
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    HIPCHK(hipEventSynchronize(d->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    *avg_seconds = (double)ms * 1e-3 / (double)reps;
    *alg_bytes = M->alg_bytes();
    return 0;
}
// r = rhs - K dx into pc_r, its inf-norm into N_B (declared in host_dense.inc, where dense_refine_checked calls it)
static void true_residual(QpdoDev *d) {
    LAUNCH(k_ctrl_set_nrm0, 1, d->ctrl, N_B);
    launch_spmv(d, d->Ar, d->dx, EpiPcgA{d->d, d->tmp_m, nullptr}, false);
    launch_spmv(d, d->Qf, d->dx, EpiPcgQ{d->dx, d->sigma_f, d->pc_Kp}, false);
    launch_spmv(d, d->At, d->tmp_m, EpiResid{d->rhs, d->pc_Kp, d->pc_r, d->ctrl, N_B}, true);
}
// dense factorization of K = Q + sigma_f I + A' diag(d) A with the workspace's CURRENT weights, `reps` times back to back, timed
// with HIP events on the solver's stream (the look-ahead stream joins it before the factor ends).  flops = n^3 / 3 per factor.
// check != NULL: relative residual ||rhs - K x||inf / ||rhs||inf of one solve with the fresh factor (rhs = the diagonal of Q + 1).
int qdev_bench_dense_factor(QpdoDev *d, int reps, double *avg_seconds, double *check) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) return set_err(hipErrorInvalidValue, "dense factor bench: not for partitioned workspaces", __LINE__);
    int rc = dense_alloc(d); if (rc) return rc;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
    rc = dense_factor(d); if (rc) return rc;               // warm-up (allocations, code objects)
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    for (int r = 0; r < reps; r++) { rc = dense_factor(d); if (rc) return rc; }
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    HIPCHK(hipEventSynchronize(d->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    *avg_seconds = (double)ms * 1e-3 / (double)(reps > 0 ? reps : 1);
    d->st.factor_count -= reps + 1;
    if (d->st.onelaunch_factors >= reps + 1) d->st.onelaunch_factors -= reps + 1;
    if (check) {
        const int n = d->n;
        if (!d->qdiag_valid) { LAUNCH(k_extract_diag, vgrid(n), n, d->Qf.rp, d->Qf.ci, d->Qf.val, d->qdiag); d->qdiag_valid = 1; }
        LAUNCH(k_axpy_const, vgrid(n), n, (const double *)d->qdiag, 1.0, d->rhs);
        const int wbk = d->wb_k; d->wb_k = 0;
        rc = dense_solve(d); d->wb_k = wbk; if (rc) return rc;
        LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
        LAUNCH(k_absmax_mul, vgrid(n), n, (const double *)d->rhs, (const double *)nullptr, d->ctrl, N_A);
        true_residual(d);
        rc = read_ctrl(d); if (rc) return rc;
        if (d->hctrl->cnt[C_CHAIN_ERR]) return set_err(hipErrorUnknown, "dense factor bench: a polling kernel lost its producer", __LINE__);
        *check = nrm_of(d->hctrl, N_B) / nrm_of(d->hctrl, N_A);
        d->dense_valid = 0;
    }
    return 0;
}
// ---- the direct solvers as single linear solves (tests: tests/test_gpu_direct_solvers.py) ---------------------------------------
// K x = rhs with K = Q + sigma I + A' diag(dw) A, through the workspace's direct solver as a Newton pass drives it: dense_refresh_factor /
// dense_solve (linsolve 1; the pass's own functions) or band_factor / band_solve (3), no other kernels.  flags bit 0: refactor; clear: a kept factor of
// this sigma is reused -- with the low-rank update for the rows whose weight moved since it when wb_enable is set (more than WB_MAX of
// them refactor), as it is (the caller passes the factored weights) otherwise, unless the workspace itself has marked that factor stale (dense_valid = 0, e.g. an outer
// update of a solve since it was made): then it is refactored, as a Newton pass would; with ud_cap set, up to that many changed rows change the
// kept factor in place (ud_apply) and more of them take the low-rank path or, without it, refactor.  Bit 1: the factorization launch carries the forward
// solve (dense_factor(d, true)).  The workspace's weights, sigma_f and dx are put back afterwards; the kept factor stays for the next
// call and is dropped by the next qdev_begin_solve.  A lost producer of a polling kernel, or a bad band pivot, returns
// QDEV_DIRECT_LOST with the latch cleared -- never a silent redo.
// What a call that drives the direct solver on its own (qdev_direct_solve, qdev_adjoint) overwrites of the workspace: the weights d->d,
// sigma_f, the direction dx and -- with_rhs -- the right-hand side.  direct_keep_save enqueues the copies to the host (the caller
// synchronises the stream before it changes sigma_f's users or lets the vectors go) and marks the factor such a call leaves as not a
// solve's own (direct_hook_used: the next qdev_begin_solve drops it); direct_keep_restore puts everything back and waits.
extern "C++" {
struct DirectKeep { std::vector<double> d, dx, rhs; double sigma_f = 0.0; bool with_rhs = false; };
}
static int direct_keep_save(QpdoDev *d, DirectKeep &k, bool with_rhs) {
    const int n = d->n, m = d->m;
    k.d.resize((size_t)(m > 0 ? m : 1)); k.dx.resize((size_t)(n > 0 ? n : 1)); k.with_rhs = with_rhs;
    if (with_rhs) k.rhs.resize((size_t)(n > 0 ? n : 1));
    if (m) HIPCHK(hipMemcpyAsync(k.d.data(), d->d, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(k.dx.data(), d->dx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (n && with_rhs) HIPCHK(hipMemcpyAsync(k.rhs.data(), d->rhs, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    k.sigma_f = d->sigma_f;
    d->direct_hook_used = 1;
    return 0;
}
static int direct_keep_restore(QpdoDev *d, const DirectKeep &k) {
    const int n = d->n, m = d->m;
    d->sigma_f = k.sigma_f;
    if (m) HIPCHK(hipMemcpyAsync(d->d, k.d.data(), (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(d->dx, k.dx.data(), (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    if (n && k.with_rhs) HIPCHK(hipMemcpyAsync(d->rhs, k.rhs.data(), (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
int qdev_direct_solve(QpdoDev *d, const double *dw, double sigma, const double *rhs, double *x, int flags) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) return set_err(hipErrorInvalidValue, "direct solve: not for row-partitioned workspaces", __LINE__);
    if (d->linsolve != 1 && d->linsolve != 3) return set_err(hipErrorInvalidValue, "direct solve: the workspace's solver is not a direct one (dense or band)", __LINE__);
    const int n = d->n, m = d->m;
    DirectKeep keep;
    { int rck = direct_keep_save(d, keep, false); if (rck) return rck; }
    if (m) HIPCHK(hipMemcpyAsync(d->d, dw, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(d->rhs, rhs, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    d->sigma_f = sigma;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
    if (d->ud_cap) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_UD_REJECT, 0);      // (a latch left by a call that ended early is not this call's)
    const bool refactor = (flags & 1) != 0, carry = (flags & 2) != 0;
    int rc = 0;
    if (d->linsolve == 3) {
        // (a coupled workspace follows moved weights itself -- band_coupled_refresh keeps what still holds -- so it is always asked)
        if (refactor || !d->dense_valid || d->bc_r > 0) rc = band_factor(d, refactor);
        if (!rc) rc = band_solve(d);
    } else {
        // a Newton pass knows whether (sigma_f, d) moved since the factorization; this caller only says "refactor" or not, and where the
        // workspace can follow moved weights (ud_cap, wb_enable) the kept factor is brought up to date with whatever rows did move
        if (refactor || !d->dense_factored || d->sigma_f != d->dense_fact_sigma || d->ud_cap > 0 || d->wb_enable) d->dense_valid = 0;
        if (!d->dense_valid) rc = dense_refresh_factor(d, refactor, carry);
        if (!rc) rc = dense_solve(d);
    }
    if (!rc && n) HIPCHK(hipMemcpyAsync(x, d->dx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (!rc) rc = read_ctrl(d);
    bool lost = false;
    if (!rc && d->hctrl->cnt[C_CHAIN_ERR]) {
        lost = true;
        LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
        d->dense_valid = 0; d->dense_factored = 0; d->wb_k = 0; d->mid_fwd_valid = 0; d->bc_factored = 0;
    }
    { int rck = direct_keep_restore(d, keep); if (rck) return rck; }
    if (rc) return rc;
    if (lost) {
        snprintf(g_err, sizeof(g_err), "direct solve: %s", d->linsolve == 3 ? (d->bc_r > 0 ? "the band factorization or the coupling rows' k x k system met a pivot that is not a positive finite number, or the solve missed its residual check"
                                                                                            : d->bb_c > 0 ? "the band factorization of the core or the border's c x c system met a pivot that is not a positive finite number"
                                                                                            : "the band factorization met a pivot that is not a positive finite number")
                                                                            : "a polling kernel lost its producer");
        return QDEV_DIRECT_LOST;
    }
    return 0;
}
// the factor arrays of the last factorization (layouts: include/qpdo_amd_ext.h, qpdo_amd_download_factor)
int qdev_download_factor(QpdoDev *d, int which, double *dst, long count) {
    HIPCHK(hipSetDevice(d->device));
    const size_t ld = (size_t)d->dense_ld, nb = (size_t)d->dense_nblk, band = (size_t)d->band_np * (size_t)(d->band_b + 1);
    if (which == 6) {
        if (count < 4) return set_err(hipErrorInvalidValue, "download factor: the geometry needs 4 entries", __LINE__);
        dst[0] = d->Kd ? (double)ld : 0.0; dst[1] = d->Kd ? (double)nb : 0.0; dst[2] = (d->Kb || d->bw_Wb) ? (double)d->band_np : 0.0; dst[3] = (d->Kb || d->bw_Wb) ? (double)d->band_b : 0.0;
        return 0;
    }
    if (which >= 9 && which <= 11) {                    // coupled mode (QPDO_BAND_COUPLING)
        if (d->bc_r <= 0) return set_err(hipErrorInvalidValue, "download factor: this workspace has no coupling rows", __LINE__);
        const size_t np = (size_t)d->band_np;           // (0 before the first factorization, like k)
        const size_t len = which == 9 ? 4 : which == 10 ? (size_t)d->bc_r : np * (size_t)d->bc_k;
        if (count < 0 || (size_t)count != len) return set_err(hipErrorInvalidValue, "download factor: count is not the array's length", __LINE__);
        if (which == 9) { dst[0] = (double)d->bc_r; dst[1] = (double)d->bc_k; dst[2] = (double)d->band_b; dst[3] = (double)np; return 0; }
        if (which == 10) { for (int a = 0; a < d->bc_r; a++) dst[a] = (double)d->bc_rows_h[(size_t)a]; return 0; }
        size_t j = 0;                                    // Z: the columns of the weighted coupling rows, in ascending row order
        for (int a = 0; a < d->bc_r; a++)
            if (d->bc_act >> a & 1) HIPCHK(hipMemcpyAsync(dst + np * j++, d->bc_Z + np * (size_t)a, np * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        return 0;
    }
    if (which == 12) {                                  // the variable order of the band solver
        if (!d->bo_newold) return set_err(hipErrorInvalidValue, "download factor: this workspace has adopted no variable order", __LINE__);
        if (count < 0 || count != (long)d->n) return set_err(hipErrorInvalidValue, "download factor: count is not the array's length", __LINE__);
        std::vector<int32_t> no((size_t)(d->n ? d->n : 1));
        int rcn = qdev_band_order_newold(d, no.data()); if (rcn) return rcn;
        for (int k = 0; k < d->n; k++) dst[k] = (double)no[(size_t)k];
        return 0;
    }
    if (which >= 13 && which <= 15) {                   // bordered mode (QPDO_BAND_BORDER)
        if (d->bb_c <= 0) return set_err(hipErrorInvalidValue, "download factor: this workspace has no border variables", __LINE__);
        const size_t np = (size_t)d->band_np, len = which == 13 ? 4 : np * (size_t)d->bb_c;      // (np: 0 before the first factorization)
        if (count < 0 || (size_t)count != len) return set_err(hipErrorInvalidValue, "download factor: count is not the array's length", __LINE__);
        if (which == 13) { dst[0] = (double)d->bb_ncore; dst[1] = (double)d->bb_c; dst[2] = (double)d->band_b; dst[3] = (double)np; return 0; }
        if (len) HIPCHK(hipMemcpyAsync(dst, which == 14 ? d->bb_C : d->bb_Z, len * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        return 0;
    }
    const double *src = nullptr; size_t len = 0;
    if ((which == 4 || which == 5) && d->bw_Wb) return set_err(hipErrorInvalidValue, "download factor: a band wider than 127 is held as tiles (arrays 7 and 8)", __LINE__);
    switch (which) {
        case 0: src = d->Kd; len = ld * ld; break;
        case 1: src = d->Dg; len = ld; break;
        case 2: src = d->Linv; len = nb * DNB * DNB; break;
        case 3: src = d->LinvT; len = nb * DNB * DNB; break;
        case 4: src = d->Kb; len = band; break;
        case 5: src = d->Lt; len = band; break;
        case 7: src = d->bw_Wb; len = (size_t)(d->band_np / DNB) * (size_t)(d->bw_w + 1) * BW_T; break;
        case 8: src = d->bw_Wd; len = (size_t)d->band_np; break;
        default: return set_err(hipErrorInvalidValue, "download factor: unknown array", __LINE__);
    }
    if (!src) return set_err(hipErrorInvalidValue, "download factor: this workspace has not factored with that solver", __LINE__);
    if (count < 0 || (size_t)count != len) return set_err(hipErrorInvalidValue, "download factor: count is not the array's length", __LINE__);
    HIPCHK(hipMemcpyAsync(dst, src, len * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// ---- the PCG path as single linear-algebra steps (tests: tests/test_gpu_pcg_pieces.py) -------------------------------------------------
// K = Q + sigma I + A' diag(dw) A through the functions a Newton pass of a PCG workspace calls.  mode 0: build_compact, then ONE
// pcg_K_apply on p = v with the latch cleared (every launch of the product leaves at once while C_PCG_DONE is set): out = K v, info =
// [kact, cnt] and the cnt per-block partial sums of p.Kp from info[QDEV_PCG_INFO_HEAD] on.  mode 1: ONE pcg_solve of K x = v with the
// relative stopping rule alone: out = x, info = [kact, iters, defl_r, Schur mode delivered, V_RNORM, V_BNORM, inner solves, inner steps,
// class (0 ok, 1 not converged, 2 NaN), outer iterations].  mode 32 / 33: build_compact, then one product of the fp32-stream slab kernel with
// A_c / A_c' (refused where the pass has no fp32 images); 34 / 35: the pair-wide fp32 instance; 36 / 37: the pair-wide half-precision instance
// (refused where the workspace has no half-precision images or no scale), info[1] = the scale's exponent e.  info holds QDEV_PCG_INFO_LEN doubles.  A solve of class 1 or 2 returns QDEV_PCG_NOT_CONVERGED /
// QDEV_PCG_NAN with pcg_verdict's message, never a HIP code.  Whatever the call overwrites -- the weights, sigma_f, dx, rhs, the stopping
// rule, the Schur mode's strikes and batch memory, the counters -- is put back: the next solve runs as on a workspace that never saw it.
static_assert(QDEV_PCG_NOT_CONVERGED == PCG_NOT_CONVERGED && QDEV_PCG_NAN == PCG_NAN, "qpdo_dev.h carries the PCG failure classes");
static_assert(QDEV_PCG_INFO_LEN == QDEV_PCG_INFO_HEAD + PGRID, "info: the head and one slot per partial sum");
int qdev_pcg_probe(QpdoDev *d, const double *dw, double sigma, const double *v, double *out, int mode, double *info) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) return set_err(hipErrorInvalidValue, "pcg probe: not for row-partitioned workspaces", __LINE__);
    if (d->linsolve != 0) return set_err(hipErrorInvalidValue, "pcg probe: the workspace's solver is not PCG", __LINE__);
    if (mode != 0 && mode != 1 && (mode < 32 || mode > 37)) return set_err(hipErrorInvalidValue, "pcg probe: mode is 0 (one K product), 1 (one solve), 32 or 33 (one fp32-stream product), 34 or 35 (one pair-wide fp32 product), 36 or 37 (one pair-wide half-precision product)", __LINE__);
    const int n = d->n, m = d->m;
    std::vector<double> d_keep((size_t)(m > 0 ? m : 1)), dx_keep((size_t)(n > 0 ? n : 1)), rhs_keep((size_t)(n > 0 ? n : 1));
    if (m) HIPCHK(hipMemcpyAsync(d_keep.data(), d->d, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(dx_keep.data(), d->dx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(rhs_keep.data(), d->rhs, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (m) HIPCHK(hipMemcpyAsync(d->d, dw, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(mode != 1 ? d->pc_p : d->rhs, v, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const double sigma_keep = d->sigma_f, abs_keep = d->pcg_abs_now;
    const int off_keep = d->schur_off, strikes_keep = d->schur_strikes, inner_keep = d->schur_last_inner, jac_keep = d->last_jacobi_iters;
    const long long sp_keep = d->schur_passes, dp_keep = d->defl_passes;
    const QdevStats st_keep = d->st;
    const double ev_keep[3] = {d->ev_spmv_ms, d->ev_ac_ms, d->ev_ac_bytes}; const long long evn_keep[2] = {d->ev_spmv_n, d->ev_ac_n};
    d->sigma_f = sigma; d->pcg_abs_now = -1.0;
    for (int i = 0; i < QDEV_PCG_INFO_HEAD; i++) info[i] = 0.0;
    int rc = 0;
    if (mode == 0) {
        if (!d->qdiag_valid) { LAUNCH(k_extract_diag, vgrid(n), n, d->Qf.rp, d->Qf.ci, d->Qf.val, d->qdiag); d->qdiag_valid = 1; }
        rc = build_compact(d);
        int cnt = 0;
        if (!rc) {
            LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_PCG_DONE, 0);
            rc = pcg_K_apply(d, &d->ctrl->cnt[C_PCG_DONE], pcg_part(d).pKp, false, &cnt);
        }
        if (!rc && n) HIPCHK(hipMemcpyAsync(out, d->pc_Kp, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
        if (!rc) HIPCHK(hipMemcpyAsync(info + QDEV_PCG_INFO_HEAD, pcg_part(d).pKp, (size_t)cnt * 8, hipMemcpyDeviceToHost, d->stream));
        if (!rc) HIPCHK(hipStreamSynchronize(d->stream));
        if (!rc) HIPCHK(hipGetLastError());
        info[0] = (double)d->kact; info[1] = (double)cnt;
    } else if (mode >= 32 && mode <= 37) {
        // the slab kernel's fp32-stream instances on their own: out[0 .. k) = A_c32 v (mode 32), out (n) = A_c32' v[0 .. k) (mode 33), A_c32 =
        // the compact values rounded to float, products and sums in double.  Modes 34 / 35: the same two products by the pair-wide
        // instance, v rounded to float as well (the copy is made on the host here; the solver writes it with the vector).  Modes 36 / 37: the
        // pair-wide instance on the half-precision images, out = 2^-e (A_c16 v32) with A_c16 = the values times 2^e rounded to float, then half
        const bool h16 = mode >= 36, x32 = mode >= 34;
        mode = 32 + (mode & 1);
        rc = build_compact(d);
        const int k = d->kact;
        if (!rc && (!schur_f32_ready(d) || k > n)) rc = set_err(hipErrorInvalidValue, "pcg probe: this pass has no fp32 images (both compact matrices under the slab kernel with 16-bit indices, QPDO_PCG_INNER_REFINE or QPDO_PCG_INNER_F32 on, k <= n)", __LINE__);
        if (!rc && x32 && !schur_x32(d)) rc = set_err(hipErrorInvalidValue, "pcg probe: this workspace has no fp32 operand vectors (QPDO_INNER_X32=0, or no fp32 images)", __LINE__);
        if (!rc && h16 && !schur_h16_ready(d)) rc = set_err(hipErrorInvalidValue, "pcg probe: this workspace has no half-precision images or no scale for them (QPDO_INNER_H16=0, QPDO_INNER_X32=0, or max |a_ij| is 0 or not finite)", __LINE__);
        if (!rc && x32) {
            std::vector<float> v32((size_t)n);
            for (int i = 0; i < n; i++) v32[(size_t)i] = (float)v[i];
            HIPCHK(hipMemcpyAsync(mode == 32 ? d->tmp_n32 : d->s_z32, v32.data(), (size_t)(mode == 32 ? n : k) * sizeof(float), hipMemcpyHostToDevice, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
        }
        if (!rc) {
            const StreamWidth width = h16 ? STREAM_H16 : STREAM_F32;
            if (mode == 32) launch_spmv_inner(d, d->Arc, d->pc_p, x32 ? d->tmp_n32 : (const float *)nullptr, EpiStore{d->tc}, false, nullptr, width);
            else launch_spmv_inner(d, d->Atc, d->pc_p, x32 ? d->s_z32 : (const float *)nullptr, EpiStore{d->tmp_n}, false, nullptr, width);
            HIPCHK(hipMemcpyAsync(out, mode == 32 ? d->tc : d->tmp_n, (size_t)(mode == 32 ? k : n) * 8, hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
            HIPCHK(hipGetLastError());
        }
        info[0] = (double)k;
        if (h16) info[1] = (double)d->h16_e;
    } else {
        int iters = 0;
        d->sdiag_from_build = 0;
        rc = pcg_solve(d, &iters);
        if (!rc && n) HIPCHK(hipMemcpyAsync(out, d->dx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
        const bool schur = d->schur_passes != sp_keep;
        info[0] = (double)d->kact; info[1] = (double)iters; info[2] = schur ? 0.0 : (double)d->defl_r; info[3] = schur ? 1.0 : 0.0;
        info[4] = d->hctrl->val[V_RNORM]; info[5] = d->hctrl->val[V_BNORM];
        info[6] = (double)(d->st.inner_solves - st_keep.inner_solves); info[7] = (double)(d->st.inner_steps - st_keep.inner_steps);
        info[8] = rc == 0 ? 0.0 : rc == PCG_NOT_CONVERGED ? 1.0 : rc == PCG_NAN ? 2.0 : -1.0;
        info[9] = (double)d->hctrl->cnt[C_PCG_IT];          // the outer iteration's own count (Schur mode: iters = this + the inner iterations)
        info[10] = (schur && d->sdiag_from_build) ? 1.0 : 0.0;      // the Schur diagonal came from build_compact's one read, not from k_schur_diag
    }
    d->sigma_f = sigma_keep; d->pcg_abs_now = abs_keep;
    d->schur_off = off_keep; d->schur_strikes = strikes_keep; d->schur_last_inner = inner_keep; d->last_jacobi_iters = jac_keep;
    d->schur_passes = sp_keep; d->defl_passes = dp_keep; d->st = st_keep;
    d->ev_spmv_ms = ev_keep[0]; d->ev_ac_ms = ev_keep[1]; d->ev_ac_bytes = ev_keep[2]; d->ev_spmv_n = evn_keep[0]; d->ev_ac_n = evn_keep[1];
    d->ctrl_clean = 0;                     // (the solve used the control block's per-pass slots: the next residual pass clears them itself)
    if (m) HIPCHK(hipMemcpyAsync(d->d, d_keep.data(), (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(d->dx, dx_keep.data(), (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync(d->rhs, rhs_keep.data(), (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return rc;
}
// the compact structures that the last build_compact / pcg_solve left (layouts: include/qpdo_amd_ext.h, qpdo_amd_download_compact);
// count is the number of elements of the array and must match
int qdev_download_compact(QpdoDev *d, int which, void *dst, long count) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) return set_err(hipErrorInvalidValue, "download compact: not for row-partitioned workspaces", __LINE__);
    if (d->linsolve != 0) return set_err(hipErrorInvalidValue, "download compact: the workspace's solver is not PCG", __LINE__);
    const int k = d->kact, words = (d->m + 63) / 64;
    const void *src = nullptr; size_t len = 0, esz = 8;
    if (which == 48) {
        if (count != 5) return set_err(hipErrorInvalidValue, "download compact: the index space's geometry has 5 entries", __LINE__);
        long long *g = (long long *)dst;
        g[0] = d->n; g[1] = d->m; g[2] = k; g[3] = words; g[4] = d->defl_r;
        return 0;
    }
    if (which == 59) {
        if (count != 2) return set_err(hipErrorInvalidValue, "download compact: the half-precision images' state has 2 entries", __LINE__);
        long long *g = (long long *)dst;
        g[0] = (d->h16_set && d->Arc.vsm16 && d->Atc.vsm16) ? 1 : 0; g[1] = g[0] ? d->h16_e : 0;
        return 0;
    }
    if (which >= 0 && which < 48) {
        const int mat = which / 16, part = which % 16;
        if (mat == 2 ? d->defl_r <= 0 : k <= 0) return set_err(hipErrorInvalidValue, "download compact: the last pass did not build that matrix", __LINE__);
        const DevCsr &M = mat == 0 ? d->Arc : mat == 1 ? d->Atc : d->Ath;
        long long nnz = M.nnz;
        if (mat == 2) {                      // (Ath.nnz is the bound the launches are sized by; the count is the last row pointer)
            int e = 0;
            HIPCHK(hipMemcpyAsync(&e, M.rp + M.nrows, sizeof(int), hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
            nnz = e;
        }
        const bool slab = mat != 2 && M.use_slab;
        switch (part) {
            case 0: {
                if (count != 7) return set_err(hipErrorInvalidValue, "download compact: a matrix's geometry has 7 entries", __LINE__);
                long long *g = (long long *)dst;
                g[0] = M.nrows; g[1] = M.ncols; g[2] = nnz; g[3] = slab; g[4] = slab ? M.nslabs : 0; g[5] = slab ? M.W : 0;
                g[6] = (slab && M.ci16 != nullptr) ? 1 : 0;      // (the array is only meaningful, and only read, under the slab kernel)
                return 0;
            }
            case 1: src = M.rp; len = (size_t)M.nrows + 1; esz = 4; break;
            case 2: src = M.ci; len = (size_t)nnz; esz = 4; break;
            case 3: src = M.val; len = (size_t)nnz; break;
            case 4: if (slab && M.ci16) { src = M.ci16; len = (size_t)nnz; esz = 2; } break;
            case 5: if (slab) { src = M.sp; len = (size_t)M.nrows * (size_t)(M.nslabs + 1); esz = 4; } break;
            default: return set_err(hipErrorInvalidValue, "download compact: unknown array", __LINE__);
        }
    } else if (which == 96) {
        // the lazy path: both images marked stale, then one product with each compact matrix that takes the slab kernel (launch_slab
        // rebuilds the image from the CSR, sp and seg by slab_major_build); nothing is copied
        if (count != 0) return set_err(hipErrorInvalidValue, "download compact: the rebuild request carries no array (count 0)", __LINE__);
        if (k <= 0) return set_err(hipErrorInvalidValue, "download compact: the last pass did not build that matrix", __LINE__);
        d->Arc.sm_dirty = d->Atc.sm_dirty = 1;
        const int64_t calls = d->st.spmv_calls, bytes = d->st.spmv_bytes;
        if (d->Arc.use_slab) launch_spmv(d, d->Arc, d->pc_p, EpiStore{d->tc}, false);
        if (d->Atc.use_slab) launch_spmv(d, d->Atc, d->tc, EpiStore{d->tmp_n}, false);
        d->st.spmv_calls = calls; d->st.spmv_bytes = bytes;
        HIPCHK(hipStreamSynchronize(d->stream));
        HIPCHK(hipGetLastError());
        return 0;
    } else if (which >= 64 && which < 96) {
        const int mat = (which - 64) / 16, part = which % 16;
        if (k <= 0) return set_err(hipErrorInvalidValue, "download compact: the last pass did not build that matrix", __LINE__);
        const DevCsr &M = mat == 0 ? d->Arc : d->Atc;
        if (M.use_slab) switch (part) {       // (count 0 where the matrix does not take the slab kernel)
            case 0: src = M.seg; len = (size_t)2 * M.nrows * (size_t)M.nslabs; esz = 4; break;
            case 1: src = M.vsm; len = (size_t)M.nnz; break;
            case 2: if (M.i16sm) { src = M.i16sm; esz = 2; } else { src = M.cism; esz = 4; } len = (size_t)M.nnz; break;
            case 3: if (h16_dst(d, M)) { src = M.vsm16; esz = 2; len = (size_t)M.nnz; } break;      // (count 0 where the image has no half-precision values)
            case 4: if (M.seg_pairs) { src = M.p16sm; esz = 2; len = (size_t)M.nnz; } break;        // (count 0 where the image is not in pair order)
            default: return set_err(hipErrorInvalidValue, "download compact: unknown array", __LINE__);
        }
    } else switch (which) {
        case 49: src = d->rowlist; len = (size_t)k; esz = 4; break;
        case 50: src = d->cidx; len = (size_t)d->m; esz = 4; break;
        case 51: src = d->dc; len = (size_t)k; break;
        case 52: src = d->flag_bits; len = (size_t)words; break;
        case 53: src = d->flag_wprefix; len = (size_t)words; esz = 4; break;
        case 54: src = d->pc_diag; len = (size_t)d->n; break;
        case 55: src = d->s_diag; len = (size_t)k; break;
        case 56: src = d->defl_list; len = (size_t)d->defl_r; esz = 4; break;
        case 57: src = d->defl_Sinv; len = d->defl_Sinv ? (size_t)DEFL_MAX * DEFL_MAX : 0; break;
        case 60: src = d->ls_idx[0]; len = (size_t)2 * d->m; esz = 4; break;      // (the radix path's eight passes end in buffer 0)
        default: return set_err(hipErrorInvalidValue, "download compact: unknown array", __LINE__);
    }
    if (count < 0 || (size_t)count != len) return set_err(hipErrorInvalidValue, "download compact: count is not the array's length", __LINE__);
    if (!len) return 0;
    if (!src) return set_err(hipErrorInvalidValue, "download compact: this workspace does not hold that array", __LINE__);
    HIPCHK(hipMemcpyAsync(dst, src, len * esz, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// the trip shape of a slab instance, for tests that reproduce its summation order (qpdo_amd_slab_trip_shape)
int qdev_slab_trip_shape(int value_bytes, int operand_bytes, int *shape) {
    if (value_bytes == 8 && operand_bytes == 8) return slab_trip_shape<double, double>(shape);
    if (value_bytes == 4 && operand_bytes == 8) return slab_trip_shape<float, double>(shape);
    if (value_bytes == 4 && operand_bytes == 4) return slab_trip_shape<float, float>(shape);
    if (value_bytes == 2 && operand_bytes == 4) return slab_trip_shape<_Float16, float>(shape);
    return -1;
}
int qdev_spmv(QpdoDev *d, int which, const double *v_host, double *y_host) {
    HIPCHK(hipSetDevice(d->device));
    DevCsr *M = mat_by_id(d, which);
    double *xin = (M->ncols == d->n) ? d->pc_p : d->pc_t;
    double *yout = (M->nrows == d->n) ? d->pc_Kp : d->tmp_m;
    if (M->ncols) HIPCHK(hipMemcpyAsync(xin, v_host, (size_t)M->ncols * 8, hipMemcpyHostToDevice, d->stream));
    launch_spmv(d, *M, xin, EpiStore{yout}, false);
    if (M->nrows) HIPCHK(hipMemcpyAsync(y_host, yout, (size_t)M->nrows * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// the group path's product on host vectors (qpdo_amd_spmv_group): nvec vectors up, one k_spmv_group launch on the slabs of live_mask,
// those slabs down.  Its own temporary buffers: nothing of the workspace is written.
int qdev_spmv_group(QpdoDev *d, int which, int nvec, unsigned live_mask, const double *v_host, double *y_host) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) { snprintf(g_err, sizeof(g_err), "qpdo_amd_spmv_group: row-partitioned workspaces are not supported"); return -1; }
    DevCsr *M = mat_by_id(d, which);
    if (M->use_slab) { snprintf(g_err, sizeof(g_err), "qpdo_amd_spmv_group: the matrix is on the slab kernel (a slab multi-vector product does not exist)"); return -1; }
    const size_t nc = (size_t)M->ncols, nr = (size_t)M->nrows;
    TempAllocs tmp; double *xin = nullptr, *yout = nullptr;
    int rc = 0;
    if (tmp.get(&xin, (size_t)nvec * nc + 1) || tmp.get(&yout, (size_t)nvec * nr + 1)) rc = set_err(hipErrorOutOfMemory, "spmv group scratch", __LINE__);
    hipError_t e = hipSuccess;
    if (!rc && nc) e = hipMemcpyAsync(xin, v_host, (size_t)nvec * nc * 8, hipMemcpyHostToDevice, d->stream);
    if (!rc && e == hipSuccess) {
        launch_spmv_group(d, *M, xin, (long long)nc, false, yout, (long long)nr, live_mask);
        for (int g = 0; g < nvec && nr && e == hipSuccess; g++)
            if ((live_mask >> g) & 1u) e = hipMemcpyAsync(y_host + (size_t)g * nr, yout + (size_t)g * nr, nr * 8, hipMemcpyDeviceToHost, d->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (!rc && e != hipSuccess) rc = set_err(e, "spmv group", __LINE__);
    tmp.release(d->stream);
    return rc;
}
int qdev_linesearch(QpdoDev *d, double eta, double beta, const double *delta, const double *alpha, double *tau) {
    HIPCHK(hipSetDevice(d->device));
    const int M2 = 2 * d->m;
    if (M2 == 0) { *tau = -beta / eta; return 0; }
    HIPCHK(hipMemcpyAsync(d->ls_delta, delta, (size_t)M2 * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->ls_alpha, alpha, (size_t)M2 * 8, hipMemcpyHostToDevice, d->stream));
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_NL, 0);
    const int g = vgrid(M2);
    LAUNCH(k_ls_prep_raw, g, M2, d->ls_delta, d->ls_alpha, d->ls_key[0], d->ls_idx[0], d->part + P_A0 * PGRID, d->part + P_B0 * PGRID, d->ctrl);
    // eta, beta enter through the partial slots so that k_ls_scan2 forms a0, b0 exactly as in a Newton step:
    // eta = 0.5*(eta_m + dxQdx) with eta_m = 2*eta, dxQdx = 0
    hipLaunchKernelGGL(k_set_partial, dim3(1), dim3(1), 0, d->stream, d->part + P_ETA_M * PGRID, 2.0 * eta);
    hipLaunchKernelGGL(k_set_partial, dim3(1), dim3(1), 0, d->stream, d->part + P_BETA_M * PGRID, 2.0 * beta);
    hipLaunchKernelGGL(k_set_partial, dim3(1), dim3(1), 0, d->stream, d->part + P_DXQDX * PGRID, 0.0);
    hipLaunchKernelGGL(k_set_partial, dim3(1), dim3(1), 0, d->stream, d->part + P_DXDF * PGRID, 0.0);
    // pm applies to ETA/BETA (1 value) and A0/B0 (g values): run scan2 with pm = g after zero-padding ETA/BETA slots
    if (g > 1) {
        HIPCHK(hipMemsetAsync(d->part + P_ETA_M * PGRID + 1, 0, (size_t)(g - 1) * 8, d->stream));
        HIPCHK(hipMemsetAsync(d->part + P_BETA_M * PGRID + 1, 0, (size_t)(g - 1) * 8, d->stream));
    }
    int rc = linesearch_device(d, g, 1); if (rc) return rc;
    rc = read_ctrl(d); if (rc) return rc;
    *tau = d->hctrl->val[V_TAU];
    return 0;
}


// ---- the workspace's device arrays, for the fused one-workgroup kernel (qpdo_small.hip: qdev_small_resident_*) ------------------------
int qdev_small_view(QpdoDev *d, QdevSmallView *v) {
    if (d->comm.active) return set_err(hipErrorInvalidValue, "qdev_small_view: row-partitioned workspace", __LINE__);
    memset(v, 0, sizeof(*v));
    v->device = d->device; v->stream = (void *)d->stream; v->n = d->n; v->m = d->m;
    v->Arp = d->Ar.rp; v->Aci = d->Ar.ci; v->Aval = d->Ar.val;
    v->Trp = d->At.rp; v->Tci = d->At.ci; v->Tval = d->At.val;
    v->Qrp = d->Qf.rp; v->Qci = d->Qf.ci; v->Qval = d->Qf.val;
    v->q = d->q; v->l = d->l; v->u = d->u;
    v->scaled = d->scaled; v->D = d->D; v->Dinv = d->Dinv; v->E = d->E; v->Einv = d->Einv; v->c = d->sc_c; v->cinv = d->sc_cinv;
    v->st_x = d->x; v->st_xbar = d->xbar; v->st_Qx = d->Qx; v->st_Aty = d->Aty;
    v->st_y = d->y; v->st_ybar = d->ybar; v->st_Ax = d->Ax; v->st_mu = d->mu; v->st_isq = d->isq;
    return 0;
}
