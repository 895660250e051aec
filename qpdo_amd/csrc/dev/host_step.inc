// host_step.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C): the Newton pass -- linesearch driver, the step's launches (one site each, shared by the host-first and the launched-ahead step), Newton step, residual pass -- and the outer-update helpers
// ---- the launches of a step after its linear solve: the host-first step and the launched-ahead one issue them through these ----------
// sort + scan + search of the linesearch in one launch (small problems; the bits of the radix path).  ahead: the launched-ahead step --
// the kernel leaves if the device decided against a Newton step, and A'dy (iteration.c:23 needs it, the search does not) rides on the
// launch as extra workgroups instead of being a launch of its own
static void launch_ls_small(QpdoDev *d, int pm, int pn, bool ahead) {
    LsProd lp{};
    int gS = 0;
    if (ahead) {
        lp = LsProd{d->At.tpr, d->At.nrows, d->At.rp, d->At.ci, d->At.val, d->dy, d->Atdy};
        gS = (d->At.nrows + 1024 / lp.tpr - 1) / (1024 / lp.tpr); if (gS > 128) gS = 128; if (gS < 1) gS = 1;
        d->st.spmv_calls++; d->st.spmv_bytes += (int64_t)d->At.alg_bytes();
    }
    hipLaunchKernelGGL(k_ls_small, dim3(1 + gS), dim3(1024), 0, d->stream, d->ctrl, (const double *)d->part, pm, pn, (const u64 *)d->ls_key[0],
                       (const double *)d->ls_delta, (const double *)d->ls_alpha, 2 * d->m, ahead ? 1 : 0, lp);
}
// the m-side of the linesearch as the epilogue of A dx
static EpiAdxLs epi_adx_ls(QpdoDev *d) {
    EpiAdxLs e{};
    e.m = d->m; e.mu = d->mu; e.isq = d->isq; e.w = d->w; e.l = d->l; e.u = d->u; e.y = d->y; e.active = d->active; e.active_old = d->active_old;
    e.Adx = d->Adx; e.dy = d->dy; e.delta = d->ls_delta; e.alpha = d->ls_alpha; e.key = d->ls_key[0]; e.idx = d->ls_idx[0];
    e.p_eta = d->part + P_ETA_M * PGRID; e.p_beta = d->part + P_BETA_M * PGRID; e.p_a0 = d->part + P_A0 * PGRID; e.p_b0 = d->part + P_B0 * PGRID;
    e.ctrl = d->ctrl;
    return e;
}
// Q dx and A dx in one launch (spmv.inc k_spmv_pair): A's blocks first; Q's block partials are indexed by blockIdx.x, so their
// pointers are shifted back by A's grid -- the same grids, the same partials as the two launches.  skip (launch-ahead, else null): the
// kernel leaves if that word is set
static void launch_adx_qdx_pair(QpdoDev *d, int proximal, double sigma, const int *skip) {
    const int gA = spmv_grid(d->Ar, true), gQ = spmv_grid(d->Qf, true);
    EpiQdx eq{d->dx, d->df, sigma, proximal, d->Qdx, d->part + P_DXQDX * PGRID - gA, d->part + P_DXDF * PGRID - gA};
    hipLaunchKernelGGL((k_spmv_pair<EpiAdxLs, EpiQdx>), dim3(gA + gQ), dim3(BLK), 0, d->stream, gA, d->Ar.tpr, d->Ar.nrows, (const int *)d->Ar.rp,
                       (const int *)d->Ar.ci, (const double *)d->Ar.val, (const double *)d->dx, epi_adx_ls(d), d->Qf.tpr, d->Qf.nrows, (const int *)d->Qf.rp,
                       (const int *)d->Qf.ci, (const double *)d->Qf.val, (const double *)d->dx, eq, skip);
    d->st.spmv_calls += 2; d->st.spmv_bytes += (int64_t)d->Ar.alg_bytes() + (int64_t)d->Qf.alg_bytes();
}
// the five axpys of the iterate update (skipped on the device if a chained solve reported a lost producer)
static void launch_axpy5(QpdoDev *d) {
    const int n = d->n, m = d->m;
    LAUNCH(k_axpy5, vgrid(n > m ? n : m), n, m, d->ctrl, d->x, d->dx, d->Qx, d->Qdx, d->Aty, d->Atdy, d->y, d->dy, d->Ax, d->Adx);
}
// ---- linesearch sort + scan + search (shared by the Newton step and the parity entry point) -----------
static int linesearch_device(QpdoDev *d, int pm, int pn) {
    const int M2 = 2 * d->m;
    if (d->ls_small && M2 <= LS_SMALL_MAX) {       // small problems: sort + scan + search in one launch, same bits as the path below
        launch_ls_small(d, pm, pn, false);
        HIPCHK(hipGetLastError());
        return 0;
    }
    int cur = 0;
    for (int pass = 0; pass < 8; pass++) {
        radix_pass<u64, RS_ITEMS, int>(d, d->ls_key[cur], d->ls_idx[cur], d->ls_key[1 - cur], d->ls_idx[1 - cur], M2, 8 * pass, d->rs_nblocks,
                                       d->rs_hist, d->scan_tsum);
        cur = 1 - cur;
    }
    // 8 passes: result back in buffer 0
    LAUNCH(k_ls_scan1, d->ls_nblk, d->ctrl, d->ls_idx[cur], d->ls_delta, d->ls_alpha, d->ls_pa, d->ls_pb, d->ls_bt, d->ls_nblk);
    LAUNCH(k_ls_scan2, 1, d->ctrl, d->part, pm, pn, d->ls_bt, d->ls_nblk);
    LAUNCH(k_ls_search, vgrid(M2), d->ctrl, d->ls_key[cur], d->ls_pa, d->ls_pb, d->ls_bt, d->ls_nblk);
    LAUNCH(k_ls_final, 1, d->ctrl, d->ls_pa, d->ls_pb, d->ls_bt, d->ls_nblk);
    HIPCHK(hipGetLastError());
    return 0;
}

// the rest of a Newton step after the linear solve: Qdx (+ sigma dx) and the n-side dots, A dx with the m-side of the linesearch fused
// behind it, A'dy, the breakpoint search, the five axpys; with `sync` the control block is read back (tau, the lost-producer latch)
static int newton_finish_step(QpdoDev *d, int proximal, double sigma, bool redo, bool sync) {
    int rc2 = 0;
    if (d->fuse_outer && !d->comm.active && !d->Qf.use_slab && !d->Ar.use_slab && d->m > 0) {
        if (redo) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_NL, 0);      // (the first time it is still zero from k_ctrl_clear_pass)
        launch_adx_qdx_pair(d, proximal, sigma, nullptr);
    } else {
    launch_spmv(d, d->Qf, d->dx, EpiQdx{d->dx, d->df, sigma, proximal, d->Qdx, d->part + P_DXQDX * PGRID, d->part + P_DXDF * PGRID}, true);
    if (redo) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_NL, 0);      // (the first time it is still zero from k_ctrl_clear_pass)
    rc2 = spmv_A(d, d->dx, epi_adx_ls(d), true); if (rc2) return rc2;
    }
    rc2 = spmv_At(d, d->dy, EpiStore{d->Atdy}, false); if (rc2) return rc2;
    rc2 = linesearch_device(d, pgrid_A(d), spmv_pgrid(d->Qf)); if (rc2) return rc2;
    // (a deferred step leaves its five axpys to the residual launch that follows it: k_resid_mn applies them in front of its own work;
    // qdev_finish_step flushes them if the solve ends first)
    if (!sync && d->fuse_resid) { d->axpy_pending = 1; return 0; }
    launch_axpy5(d);
    return sync ? read_ctrl(d) : 0;
}
// The PCG solve of this pass.  The absolute stopping rule needs the proximal term: sigma > 0 pulls an error along a flat direction of
// Q + A'DA back in the next pass; without it (settings->proximal = 0) such an error persists and the trajectory leaves the reference's
// (seen on one of 120 sweep instances), so those solves keep the relative rule alone.
static int pcg_solve_pass(QpdoDev *d, int proximal, int *lin) {
    d->pcg_abs_now = proximal ? d->pcg_abs : -1.0;
    d->cur_proximal = proximal;
    return pcg_solve(d, lin);
}
// A latch in C_CHAIN_ERR means that the device skipped this pass's iterate update; the pass is redone by another solver, which this
// workspace keeps from then on.  Never an error for the caller, never inf / NaN in dx, never silently.  Two producers set the latch:
//  - The one-launch triangular solves poll their producers inside a launch; that relies on workgroups being dispatched in linear-id
//    order, which the HIP model does not promise (and a GPU shared with other processes can stretch).  A lost producer is redone with
//    the stepwise solves (one launch per block step, no polling) on a fresh multi-launch factor.
//  - The band factorization met a pivot that is not a positive finite number (k_band_factor latches bit 1): with settings->proximal = 0
//    the banded Q + A'DA may be singular along a direction.  The dense solver takes over (n <= DENSE_LIMIT_N; it reports such a matrix
//    through its own residual checks), or PCG.
// Called with a freshly read control block; leaves the redone step's control block in d->hctrl.
static int step_redo_if_lost(QpdoDev *d, int proximal, double sigma) {
    if (!d->hctrl->cnt[C_CHAIN_ERR]) return 0;
    const bool band = d->linsolve == 3;
    const int m = d->m;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
    if (band) {
        d->st.band_fallbacks++;
        d->linsolve = (d->n <= DENSE_LIMIT_N && !d->comm.active) ? 1 : 0; d->st.linsolve = d->linsolve; d->dense_valid = 0; d->dense_factored = 0;
    } else if (d->linsolve == 1 && d->dense_chain) {
        d->dense_chain = 0; d->dense_mid = 0; d->wb_enable = 0; d->ud_cap = 0; d->st.chain_fallbacks++;
    } else {
        // the latch is set although no polling kernel can have run in this step (stale): the device skipped this step's iterate update
        // on its account, so it cannot be ignored -- it is cleared and reported, instead of looping to max_iter on a frozen iterate
        return set_err(hipErrorUnknown, "lost-producer latch set without a chained solve in flight (stale latch; step skipped)", __LINE__);
    }
    LAUNCH(k_newton_prep, vgrid(m), m, 3, d->active, d->active_old, d->isq, d->mu, d->res_prim_in, d->d, d->dy);      // dy = t again
    int rc = spmv_At(d, d->dy, EpiRhs{d->res_dual_in, d->Atdy, d->rhs}, false); if (rc) return rc;
    if (d->linsolve == 1) { rc = dense_factor_and_solve(d, band); if (rc) return rc; }      // (after a band: the factorization may carry the right-hand side)
    else { int lin = 0; rc = pcg_solve_pass(d, proximal, &lin); if (rc) return rc; d->st.lin_iters += lin; }
    return newton_finish_step(d, proximal, sigma, true, true);
}

// The reference factors whatever K it is given (cholmod_interface.c:8-30) and never fails for lack of iterations.  Where the dense factor is
// not available -- n > DENSE_LIMIT_N, or a row-partitioned workspace -- a PCG solve that cannot converge is not yet an error:
//   (a) a BANDED Newton matrix (chain-structured QPs; detected now if the workspace was configured with an explicit solver) has an exact
//       direct solver at any order: the band solver takes over for the rest of this workspace's solves (dev/band.inc up to half-bandwidth
//       127, the tiled one of dev/band_wide.inc up to 1023);
//   (b) otherwise the pass is solved again by PLAIN Jacobi-PCG -- Schur-complement mode and heavy-row deflation off, four times the
//       iteration cap: the two accelerations change the preconditioned spectrum and either can be what stalled.
// QPDOAmdStats.pcg_rescues / pcg_rescue_kinds say which fired; if neither helps the first failure's message stands and qpdo_solve ends
// with QPDO_ERROR as before.
static int pcg_rescue(QpdoDev *d, int *lin) {
    char first[sizeof(g_err)]; snprintf(first, sizeof(first), "%s", g_err);
    if (!d->comm.active) {
        if (d->band_b < 0) { int rcb = band_detect(d); if (rcb) return rcb; }
        if (d->band_b > 0 && d->n >= 4 * (d->band_b + 1)) {
            d->linsolve = 3; d->st.linsolve = 3; d->dense_valid = 0;
            int rc = band_factor(d); if (rc) return rc;
            rc = band_solve(d); if (rc) return rc;
            d->st.pcg_rescues++; d->st.pcg_rescue_kinds |= 1; *lin = 0;
            return 0;
        }
    }
    const int deflate0 = d->deflate, maxit0 = d->pcg_maxit;
    d->schur_off = 1; d->deflate = 0; d->pcg_maxit = maxit0 > (1 << 28) ? maxit0 : 4 * maxit0;
    int it2 = 0;
    int rc = pcg_solve(d, &it2);
    d->deflate = deflate0; d->pcg_maxit = maxit0;
    *lin += it2;
    if (rc == 0) { d->st.pcg_rescues++; d->st.pcg_rescue_kinds |= 2; return 0; }
    if (rc == PCG_NOT_CONVERGED || rc == PCG_NAN) {
        char second[sizeof(g_err)]; snprintf(second, sizeof(second), "%s", g_err);
        snprintf(g_err, sizeof(g_err), "%.110s | plain-Jacobi retry: %.110s", first, second);
    }
    return rc;
}

// ---- launch-ahead of the Newton step (mid-size dense route) ---------------------------------------------------
// A pass of that route is a chain of dependent launches of 3-70 us; between the residual launch and the step's first kernels the device
// waited for the host: one read-back round trip plus the launch latencies of the short kernels that follow it (~20 us of ~125 at C1).
// Here the step's launches go into the stream right behind the residual launch.  Whether the pass IS a Newton step, and with which
// factorization branch, is decided on the device by the residual launch's publishing block (vector.inc SpecArgs: the comparisons of
// qpdo_solve on the same numbers); every kernel below looks at that decision first and leaves at once if the answer is no (~2 us each,
// paid on the outer-update passes and the last one).  The host reads the control block while the step runs, makes its own decision as
// before, and qdev_newton_step only books what is already in flight -- after checking that both decisions agree.
// Route: dense one-launch factorization (k_mid_factor) + chained backward solve, every pass refactors (no low-rank path: n < 9000),
// one GPU, the one-launch linesearch, deferred step with the axpys folded into the next residual launch.  Not with QPDO_DENSE_UPDOWN:
// this route refactors every pass by construction, that one exists to keep the factor.  Each launch below is the
// launch site that qdev_newton_step -> dense_factor / dense_solve / newton_finish_step go through, with the guard switched on: the same bits.
static bool ahead_route_ok(const QpdoDev *d) {
    return d->launch_ahead && d->linsolve == 1 && !d->hybrid_active && !d->comm.active && d->defer_step && d->fuse_resid && d->ctrl_publish &&
           d->fuse_outer && d->m > 0 && !d->Qf.use_slab && !d->Ar.use_slab && !d->At.use_slab && d->ls_small && 2 * d->m <= LS_SMALL_MAX &&
           d->Kd && d->dense_mid && d->dense_chain && d->mid_flags && d->dense_nblk <= MID_MAX_NB && !d->wb_enable && !d->ud_cap;
}
static int ahead_enqueue_step(QpdoDev *d, int proximal, double sigma) {
    const auto calls0 = d->st.spmv_calls; const auto bytes0 = d->st.spmv_bytes;
    // qdev_newton_step: the weights and t were made by the residual launch's publishing block (k_newton_prep's work; vector.inc SpecArgs)
    d->ahead_sigma_f02 = proximal ? sigma : 0.0;      // sigma_f of branches 0 and 2; branch 1 keeps the factor's (the assembly picks on the device)
    // dense_factor(d, true): assembly, forming the right-hand side on the way; the one-launch factorization with the forward solve
    launch_dense_assemble(d, ASM_RHS_FORM, d->ahead_sigma_f02);
    launch_mid_factor(d, true, 1);
    // dense_solve: the forward solve came with the factorization; backward chain into dx
    launch_ldl_chain<false>(d, 1, d->ch_y, d->ch_x, d->dx, d->n, 1);
    // newton_finish_step: A dx (+ the m-side of the linesearch) | Q dx, the breakpoint search with A'dy; the axpys ride on the next residual launch
    launch_adx_qdx_pair(d, proximal, sigma, &d->ctrl->cnt[C_SPEC_SKIP]);
    launch_ls_small(d, pgrid_A(d), spmv_pgrid(d->Qf), true);
    HIPCHK(hipGetLastError());
    d->ahead_spmv_calls0 = d->st.spmv_calls - calls0; d->ahead_spmv_bytes0 = d->st.spmv_bytes - bytes0;     // (taken back if the step leaves)
    return 0;
}
// a launched-ahead step left at once (the device decided against it, or saw the latch of a lost producer): un-book it
static void ahead_drop_step(QpdoDev *d) {
    d->ahead_inflight = 0; d->st.ahead_skips++;
    d->st.spmv_calls -= d->ahead_spmv_calls0; d->st.spmv_bytes -= d->ahead_spmv_bytes0;
}
// the launched-ahead step ran: book what qdev_newton_step / dense_solve / newton_finish_step would have booked
static int ahead_adopt_step(QpdoDev *d, int branch, int proximal, double sigma, double *tau_out, int *lin_iters_out) {
    d->ahead_inflight = 0;
    const int dev_branch = d->ahead_branch;            // (as read with this pass's residual norms: qdev_residuals_ahead)
    if (dev_branch != branch) {
        snprintf(g_err, sizeof(g_err), "launch-ahead: the device took factorization branch %d, the host decided %d", dev_branch, branch);
        return -1;
    }
    if (branch == 0 || branch == 2) d->sigma_f = d->ahead_sigma_f02;
    d->ctrl_clean = 1;
    int rc = dense_factor_enqueued(d, true, false); if (rc) return rc;      // (the backward chain has used the carried forward solve)
    d->dsol = d->ch_x;
#ifdef QPDO_TEST_HOOKS
    if (d->chain_inject >= 0 && (long long)d->st.newton_passes == d->chain_inject) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 1);
#endif
    d->dense_last_branch = branch; d->dense_last_sigma = d->sigma_f;
    *lin_iters_out = 0;
    d->axpy_pending = 1;
    d->step_pending = 1; d->pend_proximal = proximal; d->pend_sigma = sigma;
    *tau_out = NAN;
    d->st.newton_passes++; d->st.ahead_steps++;
    return 0;
}

// ---- one Newton step (iteration.c:11-25) ----------------------------------------------------------------
int qdev_newton_step(QpdoDev *d, int branch, int n_changed, int proximal, double sigma, double *tau_out, int *lin_iters_out) {
    HIPCHK(hipSetDevice(d->device));
    if (d->ahead_inflight) return ahead_adopt_step(d, branch, proximal, sigma, tau_out, lin_iters_out);
    const int n = d->n, m = d->m;
    if (branch == 0 || branch == 2) d->sigma_f = proximal ? sigma : 0.0;     // ldlchol beta (cholmod_interface.c:11-13)
    LAUNCH(k_newton_prep, vgrid(m), m, branch, d->active, d->active_old, d->isq, d->mu, d->res_prim_in, d->d, d->dy, d->ctrl);
    d->ctrl_clean = 1;
    int lin = 0, rc = 0;
    rc = spmv_At(d, d->dy, EpiRhs{d->res_dual_in, d->Atdy, d->rhs}, false); if (rc) return rc;
    // the dense factor stays valid only while (sigma_f, d) is unchanged: full refactor (0) always rebuilds,
    // rank update (1) changes d iff rows entered or left, Q-only (2) is unchanged if the previous factor
    // was also Q-only at the same sigma
    if (branch == 0) d->dense_valid = 0;
    else if (branch == 1) { if (n_changed > 0) d->dense_valid = 0; }
    else if (!(d->dense_last_branch == 2 && d->dense_last_sigma == d->sigma_f)) d->dense_valid = 0;
    if (d->linsolve == 3) {
        // band direct solver: the natural-order LDL' of the banded K, refactored whenever (sigma_f, d) moved -- O(n b^2), cheaper than
        // any update of a kept factor
        if (!d->dense_valid) { rc = band_factor(d); if (rc) return rc; }
        rc = band_solve(d); if (rc) return rc;
    } else if (d->linsolve == 1) {
        // (the latch of the polling kernels -- one-launch outer panels, chained solves -- was cleared by this pass's k_ctrl_clear_pass
        // and is read back with the step)
        if (!d->dense_valid) { rc = dense_refresh_factor(d, branch == 0, true); if (rc) return rc; }
        rc = dense_solve(d); if (rc) return rc;
#ifdef QPDO_TEST_HOOKS
        {   // test hook (QPDO_DENSE_CHAIN_INJECT=<pass>): pretend the chained solve of that Newton pass lost a producer
            const int inject = d->chain_inject;
            if (inject >= 0 && d->dense_chain && (long long)d->st.newton_passes == inject) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 1);
        }
#endif
    } else {
        const bool was_hybrid = d->hybrid_active;
        rc = pcg_solve_pass(d, proximal, &lin);
        if (rc == 0 && was_hybrid) d->st.hybrid_pcg_passes++;
        const bool failed = rc == PCG_NOT_CONVERGED || rc == PCG_NAN;      // every numerical failure: budget, cap, stagnation, NaN
        if (failed && d->hybrid_active) {
            // (a workspace whose solver was chosen as "dense" must not end in QPDO_ERROR where the dense solver alone would have succeeded)
            // hybrid: this pass's system is past the point where PCG is the cheaper solver -- the dense factor from here on (same system)
            d->hybrid_active = 0; d->linsolve = 1; d->dense_valid = 0; d->dense_factored = 0; d->wb_k = 0;
            rc = dense_factor_and_solve(d, true); if (rc) return rc;
            lin = 0;
        } else if (failed && d->pcg_dense_fallback && !d->comm.active && n <= DENSE_LIMIT_N) {
            // The reference solves this system with a direct factorization (cholmod_interface.c:35-52,98-102) and does not care how
            // ill-conditioned it is.  A PCG solve that stagnates above 1e-8 -- seen with settings->proximal = 0, where Q + A'DA may be
            // singular to working precision -- is therefore redone by the dense LDL' solver, which this workspace keeps from then on
            // (the same (sigma_f, d) system, so the trajectory is the reference's).  Above the dense limit the error stands.
            d->linsolve = 1; d->dense_valid = 0; d->st.pcg_dense_fallbacks++;
            rc = dense_factor_and_solve(d, true); if (rc) return rc;
            lin = 0;
        } else if (failed && d->pcg_dense_fallback) {
            // no dense factor at this order / on a row partition: the other rescues (band direct solver, plain-Jacobi retry)
            rc = pcg_rescue(d, &lin); if (rc) return rc;
        } else if (rc) return rc;
    }
    d->dense_last_branch = branch; d->dense_last_sigma = d->sigma_f;
    d->st.lin_iters += lin;
    *lin_iters_out = lin;
    if (d->defer_step && (d->linsolve == 1 || d->linsolve == 3) && !d->comm.active) {
        // deferred read-back: everything above is in flight; tau and the lost-producer latch arrive with the next residual pass
        rc = newton_finish_step(d, proximal, sigma, false, false); if (rc) return rc;
        d->step_pending = 1; d->pend_proximal = proximal; d->pend_sigma = sigma;
        *tau_out = NAN;
        d->st.newton_passes++;
        return 0;
    }
    rc = newton_finish_step(d, proximal, sigma, false, true); if (rc) return rc;
    rc = step_redo_if_lost(d, proximal, sigma); if (rc) return rc;
    *tau_out = d->hctrl->val[V_TAU];
    d->st.newton_passes++;
    return 0;
}
int qdev_set_deferred_step(QpdoDev *d, int on) { d->defer_step = on != 0; return 0; }
// completes a deferred step from a control block that has just been read (d->hctrl): redoes it stepwise if a chained solve lost a
// producer.  *redone = 1 tells the caller that the iterate moved after the residual kernels of this pass ran.
static int step_complete_pending(QpdoDev *d, double *tau, int *redone) {
    *redone = 0;
    if (!d->step_pending) return 0;
    d->step_pending = 0;
    const bool lost = d->hctrl->cnt[C_CHAIN_ERR] != 0;
    if (lost) { int rc = step_redo_if_lost(d, d->pend_proximal, d->pend_sigma); if (rc) return rc; *redone = 1; }
    *tau = d->hctrl->val[V_TAU];
    return 0;
}
int qdev_finish_step(QpdoDev *d, int *had_pending, double *tau) {
    HIPCHK(hipSetDevice(d->device));
    *had_pending = d->step_pending;
    if (!d->step_pending) return 0;
    if (d->axpy_pending) { launch_axpy5(d); d->axpy_pending = 0; }
    int rc = read_ctrl(d); if (rc) return rc;
    int redone = 0;
    return step_complete_pending(d, tau, &redone);
}

// The tail of an outer update -- shifting the estimates, the mu-changed weights, the sigma term of Qx, saving res_prim -- is four
// elementwise kernels that depend on nothing of each other; with QPDO_FUSE_OUTER they are collected and launched as ONE (k_outer_tail) by
// the call that ends every outer update (qdev_save_res_prim), or by outer_tail_flush if something else wants the vectors first.
static int outer_tail_launch(QpdoDev *d, int save) {
    if (!d->tail_shift && !d->tail_muchg && !d->tail_sigma && !save) return 0;
    OuterTail t{};
    t.n = d->n; t.m = d->m; t.shift = d->tail_shift; t.muchg = d->tail_muchg; t.sigma = d->tail_sigma; t.save = save && d->m > 0; t.dsig = d->tail_dsig;
    t.x = d->x; t.y = d->y; t.at_scale = d->at_scale; t.isq = d->isq; t.res_prim = d->res_prim; t.changed = d->mu_changed;
    t.xbar = d->xbar; t.ybar = d->ybar; t.d = d->d; t.Qx = d->Qx; t.res_prim_old = d->res_prim_old; t.ctrl = d->ctrl;
    d->tail_shift = d->tail_muchg = d->tail_sigma = 0; d->tail_dsig = 0.0;
    LAUNCH(k_outer_tail, vgrid(d->n > d->m ? d->n : d->m), t);
    HIPCHK(hipGetLastError());
    if (t.save) d->ctrl_clean = 1;
    return 0;
}
static int outer_tail_flush(QpdoDev *d) { return outer_tail_launch(d, 0); }

// ---- residual pass ---------------------------------------------------------------------------------
int qdev_residuals(QpdoDev *d, int proximal, double sigma, QdevResid *out) { return qdev_residuals_ahead(d, proximal, sigma, nullptr, out); }
int qdev_residuals_ahead(QpdoDev *d, int proximal, double sigma, const QdevAhead *ahead, QdevResid *out) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, m = d->m;
    bool go_ahead = ahead && ahead_route_ok(d);
    d->ahead_inflight = 0;
    { int rcf = outer_tail_flush(d); if (rcf) return rcf; }       // (nothing is pending after a complete outer update)
    auto launch_resid = [&]() -> int {
        if (!d->ctrl_clean) LAUNCH(k_ctrl_clear_pass, 1, d->ctrl);          // (a Newton step leaves the slots zeroed: k_newton_prep)
        d->ctrl_clean = 0;
        const int gm = vgrid(m), gn = vgrid(n);
        ResidM a{m, d->scaled, d->sc_cinv, d->Ax, d->y, d->ybar, d->mu, d->l, d->u, d->E, d->Einv, d->res_prim, d->w, d->res_prim_in, d->active, d->active_old};
        ResidN b{n, d->scaled, proximal, sigma, d->Qx, d->q, d->x, d->xbar, d->Aty, d->Dinv, d->df, d->res_dual, d->res_dual_in};
        StepAx st{d->axpy_pending, d->x, d->Qx, d->Aty, d->y, d->Ax, d->dx, d->Qdx, d->Atdy, d->dy, d->Adx};
        d->axpy_pending = 0;
        PubArgs pb{nullptr, nullptr, 0, d->pub_ticket};
        const bool fused_pub = d->ctrl_publish && d->fuse_resid;
        if (fused_pub) { pb.host = d->hctrl; pb.hseq = d->hseq; pb.seq = ++d->pub_seq; }
        SpecArgs sp{};
        if (go_ahead && fused_pub) {
            sp.on = 1; sp.allow_outer = ahead->allow_outer; sp.force_outer = ahead->force_outer; sp.reset_newton = ahead->reset_newton;
            sp.max_rank = ahead->max_rank; sp.eps_abs = ahead->eps_abs; sp.eps_in = ahead->eps_in; sp.infty = ahead->infty; sp.cinv = d->sc_cinv;
            sp.isq = d->isq; sp.d = d->d; sp.dy = d->dy;
        }
        LAUNCH(k_resid_mn, gm + gn, gm, a, b, d->ctrl, st, pb, sp);
        if (sp.on) {
            // the step goes into the stream before the host looks at the norms; the device decides whether it runs
            int rca = ahead_enqueue_step(d, proximal, sigma); if (rca) return rca;
            d->ahead_inflight = 1;
        }
        if (!fused_pub) return read_ctrl(d);
        int rcw = ctrl_wait(d, d->hseq, pb.seq); if (rcw) return rcw;
        HIPCHK(hipGetLastError());
        return 0;
    };
    int rc = launch_resid(); if (rc) return rc;
    out->prev_step_done = 0; out->prev_tau = 0.0;
    if (d->step_pending) {
        // the Newton step of the previous pass completes here (deferred read-back): its tau, and the lost-producer latch of its
        // chained solves -- if that was set the device skipped the iterate update, so the residuals above are those of the OLD
        // iterate; the step is redone stepwise and the residual kernels run again
        int redone = 0;
        rc = step_complete_pending(d, &out->prev_tau, &redone); if (rc) return rc;
        out->prev_step_done = 1;
        if (redone) {
            // (a launched-ahead step of THIS pass left at once: the residual launch saw the latch of the lost producer)
            if (d->ahead_inflight) ahead_drop_step(d);
            d->ctrl_clean = 0; go_ahead = false;
            rc = launch_resid(); if (rc) return rc;
        }
    }
    out->ahead_enqueued = d->ahead_inflight; out->ahead_went = 0; out->ahead_branch = -1;
    if (d->ahead_inflight) {
        out->ahead_went = d->hctrl->cnt[C_SPEC_SKIP] == 0; out->ahead_branch = d->ahead_branch = d->hctrl->cnt[C_SPEC_BRANCH];
        if (!out->ahead_went) ahead_drop_step(d);
    }
    const Ctrl *c = d->hctrl;
    out->res_prim = nrm_of(c, N_PRIM);
    out->res_prim_in = nrm_of(c, N_PRIM_IN);
    out->res_dual = nrm_of(c, N_DUAL);
    out->res_dual_in = nrm_of(c, N_DUAL_IN);
    if (d->scaled) { out->res_dual *= d->sc_cinv; out->res_dual_in *= d->sc_cinv; }   // termination.c:45,72
    out->n_active = c->cnt[C_ACTIVE]; out->n_enter = c->cnt[C_ENTER]; out->n_leave = c->cnt[C_LEAVE];
    return 0;
}

// ---- outer-update helpers ---------------------------------------------------------------------------------
int qdev_primal_infeasibility(QpdoDev *d, double eps_prim_inf, int *is_infeasible) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, m = d->m;
    *is_infeasible = 0;
    // ONE read-back (round 3; was two): the norm of dy, the norm of Dinv .* A'dy and the support-function sum are all enqueued before
    // the host looks at any of them -- none of the three depends on the tolerance eps = eps_prim_inf ||E .* dy||inf, only the test does
    const int g = vgrid(m);
    int rc = 0;
    if (d->fuse_outer && !d->comm.active) {
        // four launches instead of eight (vector.inc "the outer-update sequences with fewer launches"): the same operations on the same grids
        LAUNCH(k_sub_clear, g, m, (const double *)d->y, (const double *)d->ybar, d->dy, d->ctrl);           // qpdo.c:372
        { int rc2 = spmv_At(d, d->dy, EpiStore{d->Atdy}, false); if (rc2) return rc2; }                        // qpdo.c:374
        LAUNCH(k_pinf_all, g + vgrid(n), g, m, n, d->scaled, (const double *)d->dy, (const double *)d->l, (const double *)d->u, (const double *)d->E,
               (const double *)d->Dinv, d->Atdy, d->part + P_OOB * PGRID, d->ctrl);
        if (d->ctrl_publish) {
            const u64 seq = ++d->pub_seq;
            LAUNCH(k_reduce_publish, 1, (const double *)(d->part + P_OOB * PGRID), g, d->ctrl, V_OOB, d->hctrl, d->hseq, seq);
            rc = ctrl_wait(d, d->hseq, seq); if (rc) return rc;
            HIPCHK(hipGetLastError());
        } else {
            LAUNCH(k_reduce_to_ctrl, 1, d->part + P_OOB * PGRID, g, d->ctrl, V_OOB);
            rc = read_ctrl(d); if (rc) return rc;
        }
    } else {
    LAUNCH(k_sub, vgrid(m), m, d->y, d->ybar, d->dy);                                  // qpdo.c:372
    { int rc2 = spmv_At(d, d->dy, EpiStore{d->Atdy}, false); if (rc2) return rc2; }       // qpdo.c:374
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_mul, vgrid(m), m, (const double *)d->dy, d->scaled ? (const double *)d->E : (const double *)nullptr, d->ctrl, N_A);
    LAUNCH(k_pinf_n, vgrid(n), n, d->scaled, d->Dinv, d->Atdy, d->ctrl);
    LAUNCH(k_pinf_m, g, m, d->scaled, d->dy, d->l, d->u, d->E, d->part + P_OOB * PGRID);
    LAUNCH(k_reduce_to_ctrl, 1, d->part + P_OOB * PGRID, g, d->ctrl, V_OOB);
    rc = read_ctrl(d); if (rc) return rc;
    }
    const double eps = eps_prim_inf * nrm_of(d->hctrl, N_A);
    if (eps == 0) return 0;
    const double nAtdy = nrm_of(d->hctrl, N_B), oob = d->hctrl->val[V_OOB];
    if ((nAtdy <= eps) && (oob <= -eps)) {
        *is_infeasible = 1;
        if (d->scaled) LAUNCH(k_pinf_cert, vgrid(m), m, d->sc_cinv, d->E, d->dy);
    }
    return 0;
}
// is_dual_infeasible (termination.c:156-216) and, behind it in the stream, update_mu (iteration.c:127-168) with ONE read-back (round 3;
// was three + one).  Every quantity of the test is enqueued unconditionally -- the early exits of the reference only skip work whose
// results are not looked at --, its decision is formed on the device (k_dinf_decide), and update_mu runs behind it unless the decision
// is "infeasible" (the solve ends there and mu must stay what it was).  do_dinf / do_mu: which of the two the caller's pass needs.
int qdev_dual_infeasibility_and_mu(QpdoDev *d, int do_dinf, int proximal, double sigma, double tau, double eps_dual_inf, int do_mu,
                                   double eps_abs, double theta, double delta, double mu_min, double isq_mu_min, int *is_infeasible, int *n_changed) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, m = d->m;
    *is_infeasible = 0; *n_changed = 0;
    if (!do_dinf && !do_mu) return 0;
    if (do_dinf && d->fuse_outer && !d->comm.active) {
        // eight launches instead of thirteen: the same operations on the same grids (vector.inc)
        const int gn = vgrid(n), gm = vgrid(m);
        LAUNCH(k_sub_clear, gn, n, (const double *)d->x, (const double *)d->xbar, d->dx, d->ctrl);            // qpdo.c:383
        if (!d->Qf.use_slab && !d->Ar.use_slab && m > 0) {
            // Q dx (qpdo.c:385, no sigma) and A dx (qpdo.c:387) in one launch (k_spmv_pair: each product on its own grid, the same lane groups)
            const int gA = spmv_grid(d->Ar, false), gQ = spmv_grid(d->Qf, false);
            hipLaunchKernelGGL((k_spmv_pair<EpiStore, EpiStore>), dim3(gA + gQ), dim3(BLK), 0, d->stream, gA, d->Ar.tpr, d->Ar.nrows, (const int *)d->Ar.rp,
                               (const int *)d->Ar.ci, (const double *)d->Ar.val, (const double *)d->dx, EpiStore{d->Adx}, d->Qf.tpr, d->Qf.nrows, (const int *)d->Qf.rp,
                               (const int *)d->Qf.ci, (const double *)d->Qf.val, (const double *)d->dx, EpiStore{d->Qdx});
            d->st.spmv_calls += 2; d->st.spmv_bytes += (int64_t)d->Ar.alg_bytes() + (int64_t)d->Qf.alg_bytes();
        } else {
        launch_spmv(d, d->Qf, d->dx, EpiStore{d->Qdx}, false);                             // qpdo.c:385 (no sigma)
        { int rc2 = spmv_A(d, d->dx, EpiStore{d->Adx}, false); if (rc2) return rc2; }        // qpdo.c:387
        }
        LAUNCH(k_absmax_pair, gn + (do_mu ? gm : 0), gn, n, (const double *)d->dx, d->scaled ? (const double *)d->D : (const double *)nullptr, m,
               (const double *)d->res_prim, d->ctrl);                                         // ||D dx||inf; iteration.c:130
        LAUNCH(k_dinf_mn, gm + gn, gm, m, n, d->scaled, eps_dual_inf, (const double *)d->Einv, (const double *)d->E, (const double *)d->l,
               (const double *)d->u, d->Adx, proximal, -sigma * tau, (const double *)d->dx, (const double *)d->q, d->Qdx, d->ctrl, d->part + P_QDX * PGRID);
        int rcf = 0;
        if (d->ctrl_publish && m <= MU_ONE_BLOCK_MAX) {
            // decision, update_mu and the publication in one single-block launch (three launches otherwise)
            MuArgs ma{do_mu, m, eps_abs, theta, delta, mu_min, isq_mu_min, d->res_prim, d->res_prim_old, d->mu, d->isq, d->at_scale, d->mu_changed};
            const u64 seq = ++d->pub_seq;
            LAUNCH(k_reduce_decide_mu_publish, 1, (const double *)(d->part + P_QDX * PGRID), gn, d->ctrl, eps_dual_inf, d->scaled, d->scaled ? d->sc_c : 1.0,
                   ma, d->hctrl, d->hseq, seq);
            rcf = ctrl_wait(d, d->hseq, seq); if (rcf) return rcf;
            HIPCHK(hipGetLastError());
        } else {
        LAUNCH(k_reduce_decide, 1, (const double *)(d->part + P_QDX * PGRID), gn, d->ctrl, eps_dual_inf, d->scaled, d->scaled ? d->sc_c : 1.0);
        if (do_mu)
            LAUNCH(k_update_mu, gm, m, eps_abs, theta, delta, mu_min, isq_mu_min, (const Ctrl *)d->ctrl, d->res_prim, d->res_prim_old,
                   d->mu, d->isq, d->at_scale, d->mu_changed, d->ctrl, (const int *)&d->ctrl->cnt[C_DINF]);
        rcf = read_ctrl(d); if (rcf) return rcf;
        }
        if (d->hctrl->cnt[C_DINF]) {
            *is_infeasible = 1;
            if (d->scaled) LAUNCH(k_mul, vgrid(n), n, d->D, d->dx, d->dx);
            return 0;
        }
        if (do_mu) *n_changed = d->hctrl->cnt[C_MUCH];
        return 0;
    }
    if (do_dinf) {
        LAUNCH(k_sub, vgrid(n), n, d->x, d->xbar, d->dx);                                  // qpdo.c:383
        launch_spmv(d, d->Qf, d->dx, EpiStore{d->Qdx}, false);                             // qpdo.c:385 (no sigma)
        { int rc2 = spmv_A(d, d->dx, EpiStore{d->Adx}, false); if (rc2) return rc2; }        // qpdo.c:387
    }
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    if (do_dinf) {
        LAUNCH(k_absmax_mul, vgrid(n), n, (const double *)d->dx, d->scaled ? (const double *)d->D : (const double *)nullptr, d->ctrl, N_C);
        LAUNCH(k_dinf_m, vgrid(m), m, d->scaled, eps_dual_inf, d->Einv, d->E, d->l, d->u, d->Adx, d->ctrl);
        const int g = vgrid(n);
        LAUNCH(k_dinf_n, g, n, proximal, -sigma * tau, d->dx, d->q, d->Qdx, d->ctrl, d->part + P_QDX * PGRID);
        LAUNCH(k_reduce_to_ctrl, 1, d->part + P_QDX * PGRID, g, d->ctrl, V_QDX);
        LAUNCH(k_dinf_decide, 1, d->ctrl, eps_dual_inf, d->scaled, d->scaled ? d->sc_c : 1.0);
    }
    if (do_mu) {
        LAUNCH(k_absmax_mul, vgrid(m), m, (const double *)d->res_prim, (const double *)nullptr, d->ctrl, N_A);     // iteration.c:130
        LAUNCH(k_update_mu, vgrid(m), m, eps_abs, theta, delta, mu_min, isq_mu_min, (const Ctrl *)d->ctrl, d->res_prim, d->res_prim_old,
               d->mu, d->isq, d->at_scale, d->mu_changed, d->ctrl, do_dinf ? (const int *)&d->ctrl->cnt[C_DINF] : (const int *)nullptr);
    }
    int rc = read_ctrl(d); if (rc) return rc;
    if (do_dinf && d->hctrl->cnt[C_DINF]) {
        *is_infeasible = 1;
        if (d->scaled) LAUNCH(k_mul, vgrid(n), n, d->D, d->dx, d->dx);
        return 0;
    }
    if (do_mu) *n_changed = d->hctrl->cnt[C_MUCH];
    return 0;
}
int qdev_dual_infeasibility(QpdoDev *d, int proximal, double sigma, double tau, double eps_dual_inf, int *is_infeasible) {
    int nch = 0;
    return qdev_dual_infeasibility_and_mu(d, 1, proximal, sigma, tau, eps_dual_inf, 0, 0, 0, 0, 0, 0, is_infeasible, &nch);
}
int qdev_shift_estimates(QpdoDev *d) {
    HIPCHK(hipSetDevice(d->device));
    if (d->fuse_outer) { d->tail_shift = 1; return 0; }
    HIPCHK(hipMemcpyAsync(d->xbar, d->x, (size_t)d->n * 8, hipMemcpyDeviceToDevice, d->stream));
    if (d->m) HIPCHK(hipMemcpyAsync(d->ybar, d->y, (size_t)d->m * 8, hipMemcpyDeviceToDevice, d->stream));
    return 0;
}
int qdev_update_mu(QpdoDev *d, double eps_abs, double theta, double delta, double mu_min, double isq_mu_min, int *n_changed) {
    HIPCHK(hipSetDevice(d->device));
    const int m = d->m;
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_mul, vgrid(m), m, (const double *)d->res_prim, (const double *)nullptr, d->ctrl, N_A);     // iteration.c:130
    LAUNCH(k_update_mu, vgrid(m), m, eps_abs, theta, delta, mu_min, isq_mu_min, (const Ctrl *)d->ctrl, d->res_prim, d->res_prim_old,
           d->mu, d->isq, d->at_scale, d->mu_changed, d->ctrl, (const int *)nullptr);
    int rc = read_ctrl(d); if (rc) return rc;
    *n_changed = d->hctrl->cnt[C_MUCH];
    return 0;
}
int qdev_mu_changed_update(QpdoDev *d) {
    HIPCHK(hipSetDevice(d->device));
    if (d->fuse_outer && d->tail_shift) { d->tail_muchg = 1; d->dense_valid = 0; return 0; }
    LAUNCH(k_mu_changed_d, vgrid(d->m), d->m, d->mu_changed, d->at_scale, d->isq, d->d);
    d->dense_valid = 0;
    HIPCHK(hipGetLastError());
    return 0;
}
int qdev_update_sigma(QpdoDev *d, double sigma_new, double sigma_old) {
    HIPCHK(hipSetDevice(d->device));
    if (d->fuse_outer && d->tail_shift && !d->tail_sigma) { d->tail_sigma = 1; d->tail_dsig = sigma_new - sigma_old; return 0; }
    { int rcf = outer_tail_flush(d); if (rcf) return rcf; }
    LAUNCH(k_axpy, vgrid(d->n), d->n, sigma_new - sigma_old, d->x, d->Qx);
    HIPCHK(hipGetLastError());
    return 0;
}
int qdev_save_res_prim(QpdoDev *d) {
    HIPCHK(hipSetDevice(d->device));
    if (d->m && d->fuse_outer) {
        // (the last call of an outer update: the pass slots of the control block are cleared here for the residual launch that follows;
        // whatever the outer update's tail has collected rides along)
        return outer_tail_launch(d, 1);
    }
    { int rcf = outer_tail_flush(d); if (rcf) return rcf; }
    if (d->m) HIPCHK(hipMemcpyAsync(d->res_prim_old, d->res_prim, (size_t)d->m * 8, hipMemcpyDeviceToDevice, d->stream));
    return 0;
}
// store_solution + the objective with ONE device-to-host copy and one synchronisation (the end of every qpdo_solve): the objective's two
// kernels first, then the six vectors and the objective sum as one image into pinned memory; without the pinned buffer: the two calls
int qdev_store_solution_obj(QpdoDev *d, int proximal, double sigma, double c_const, double *sol_x, double *sol_y, double *x, double *y,
                            double *dx, double *dy, double *objective) {
    HIPCHK(hipSetDevice(d->device));
    { int rcf = outer_tail_flush(d); if (rcf) return rcf; }       // (an outer update that was left half-way by an error)
    if (!d->hpack || !d->pack) {
        int rc = qdev_store_solution(d, sol_x, sol_y, x, y, dx, dy); if (rc) return rc;
        return qdev_objective(d, proximal, sigma, c_const, objective);
    }
    const int n = d->n, m = d->m;
    const int g = vgrid(n);
    LAUNCH(k_objective, g, n, proximal, sigma, d->x, d->Qx, d->q, d->part + P_OBJ * PGRID);
    LAUNCH(k_reduce_to_ctrl, 1, d->part + P_OBJ * PGRID, g, d->ctrl, V_OBJ);
    LAUNCH(k_store_solution_packed, vgrid(n > m ? n : m), n, m, d->scaled, d->sc_cinv, (const double *)d->x, (const double *)d->D, d->y, (const double *)d->E,
           (const double *)d->dx, (const double *)d->dy, (const Ctrl *)d->ctrl, d->pack);
    const size_t cnt = 3 * (size_t)n + 3 * (size_t)m + 1;
    HIPCHK(hipMemcpyAsync(d->hpack, d->pack, cnt * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipGetLastError());
    const double *p = d->hpack;
    memcpy(sol_x, p, (size_t)n * 8); memcpy(x, p + n, (size_t)n * 8); memcpy(dx, p + 2 * (size_t)n, (size_t)n * 8);
    p += 3 * (size_t)n;
    if (m) { memcpy(sol_y, p, (size_t)m * 8); memcpy(y, p + m, (size_t)m * 8); memcpy(dy, p + 2 * (size_t)m, (size_t)m * 8); }
    double obj = p[3 * (size_t)m];
    if (d->scaled) obj *= d->sc_cinv;               // (qdev_objective)
    obj += c_const;
    *objective = obj;
    return 0;
}
int qdev_store_solution(QpdoDev *d, double *sol_x, double *sol_y, double *x, double *y, double *dx, double *dy) {
    HIPCHK(hipSetDevice(d->device));
    { int rcf = outer_tail_flush(d); if (rcf) return rcf; }
    const int n = d->n, m = d->m;
    LAUNCH(k_store_solution, vgrid(n > m ? n : m), n, m, d->scaled, d->sc_cinv, d->x, d->D, d->y, d->E, d->tmp_n, d->tmp_m);
    HIPCHK(hipMemcpyAsync(sol_x, d->tmp_n, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(x, d->x, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(dx, d->dx, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (m) {
        HIPCHK(hipMemcpyAsync(sol_y, d->tmp_m, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(y, d->y, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(dy, d->dy, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
