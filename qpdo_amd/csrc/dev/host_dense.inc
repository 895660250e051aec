// host_dense.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C): dense factorization, solves, low-rank update, in-place up/downdate; the one launch site of the assembly, of the one-launch factorization and of the chained solves
// ---- dense direct solve ------------------------------------------------------------------------------
static const int DOUTER = 4;                 // inner 64-blocks per outer panel (256 columns)
static const int DENSE_RESERVE_CUS = 32;     // CUs left out of the look-ahead stream's mask
static int dense_alloc(QpdoDev *d) {
    if (d->Kd) return 0;
    const int ld = (d->n + DNB - 1) / DNB * DNB;
    d->dense_ld = ld; d->dense_nblk = ld / DNB;
    int rc = dev_alloc(d, &d->Kd, (size_t)ld * ld);
    if (!rc) rc = dev_alloc(d, &d->Wd, (size_t)2 * ld * DNB * DOUTER);     // two outer panels of W = L D (look-ahead)
    if (!rc && !d->stream2) {
        // The trailing updates would fill every CU and starve the one-workgroup diagonal kernel of the next panel
        // (it needs 66 KB of LDS on one CU), so their stream leaves a few CUs out of its mask.
        hipDeviceProp_t prop; int ncu = 256;
        if (hipGetDeviceProperties(&prop, d->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
        hipError_t e = hipErrorInvalidValue;
        if (DENSE_RESERVE_CUS < ncu) {
            const int words = (ncu + 31) / 32;
            std::vector<uint32_t> mask((size_t)words, 0u);
            for (int c = 0; c < ncu - DENSE_RESERVE_CUS; c++) mask[c >> 5] |= 1u << (c & 31);
            e = hipExtStreamCreateWithCUMask(&d->stream2, (uint32_t)words, mask.data());
            if (e != hipSuccess) { (void)hipGetLastError(); d->stream2 = nullptr; }
        }
        if (e != hipSuccess) e = hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; i++) { e = hipEventCreateWithFlags(&d->evF[i], hipEventDisableTiming); if (e == hipSuccess) e = hipEventCreateWithFlags(&d->evB[i], hipEventDisableTiming); }
        if (e != hipSuccess) rc = set_err(e, "dense look-ahead stream", __LINE__);
    }
    if (!rc) rc = dev_alloc(d, &d->Dg, (size_t)ld);
    if (!rc) rc = dev_alloc(d, &d->Linv, (size_t)d->dense_nblk * DNB * DNB);
    if (!rc && d->dense_nblk <= MID_MAX_NB) {
        rc = dev_alloc(d, &d->mid_flags, (size_t)(d->dense_nblk + 1) * d->dense_nblk);
        if (!rc) rc = dev_alloc(d, &d->mid_C, (size_t)d->dense_nblk * DNB * DNB);
        if (!rc) rc = dev_alloc(d, &d->mid_dinv, (size_t)ld);
        if (!rc) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mid_factor), hipFuncAttributeMaxDynamicSharedMemorySize, MID_LDS_DOUBLES * 8);
            if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
        }
    }
    if (!rc && (d->wb_enable || d->ud_cap)) rc = dev_alloc(d, &d->d_fact, d->m > 0 ? (size_t)d->m : 1);
    if (!rc && d->ud_cap) {
        rc = dev_alloc(d, &d->ud_a, (size_t)ld * UD_CAP_MAX);
        if (!rc) rc = dev_alloc(d, &d->ud_p, (size_t)ld * UD_CAP_MAX);
        if (!rc) rc = dev_alloc(d, &d->ud_q, (size_t)ld * UD_CAP_MAX);
        if (!rc) rc = dev_alloc(d, &d->ud_G, (size_t)ld * d->dense_nblk);
        if (!rc) rc = dev_alloc(d, &d->ud_Dn, (size_t)ld);
        if (!rc) rc = dev_alloc(d, &d->ud_beta, (size_t)ld);
        if (!rc) rc = dev_alloc(d, &d->ud_rows, (size_t)UD_CAP_MAX);
        if (!rc) rc = dev_alloc(d, &d->ud_cnt, (size_t)2);
    }
    if (!rc && d->wb_enable) {
        const size_t mm = d->m > 0 ? (size_t)d->m : 1;
        if (!rc) rc = dev_alloc(d, &d->wb_Z, (size_t)ld * (WB_MAX + 16));      // + one padding group of right-hand sides
        if (!rc) rc = dev_alloc(d, &d->wb_T, (size_t)ld * (WB_MAX + 16));
        if (!rc) rc = dev_alloc(d, &d->wb_T2, (size_t)ld * (WB_MAX + 16));
        if (!rc) rc = dev_alloc(d, &d->wb_G, (size_t)WB_MAX * WB_MAX);
        if (!rc) rc = dev_alloc(d, &d->wb_M, (size_t)WB_MAX * (WB_MAX + 2));
        if (!rc) rc = dev_alloc(d, &d->wb_v, (size_t)WB_MAX);
        if (!rc) rc = dev_alloc(d, &d->wb_w, (size_t)WB_MAX);
        if (!rc) rc = dev_alloc(d, &d->wb_t, (size_t)WB_MAX + 1);
        if (!rc) rc = dev_alloc(d, &d->wb_slot, mm);
        if (!rc) rc = dev_alloc(d, &d->wb_rows, (size_t)WB_MAX);
        if (!rc) rc = dev_alloc(d, &d->wb_cnt, (size_t)2);
        if (!rc) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb_lu), hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX * (WB_LDS_MAX + 2) * 8);
            if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
        }
    }
    if (!rc) rc = dev_alloc(d, &d->dz, (size_t)ld);
    if (!rc) rc = dev_alloc(d, &d->dxw, (size_t)ld);
    if (!rc) rc = dev_alloc(d, &d->LinvT, (size_t)d->dense_nblk * DNB * DNB);
    if (!rc) rc = dev_alloc(d, &d->ch_y, (size_t)ld);
    if (!rc) rc = dev_alloc(d, &d->ch_x, (size_t)ld);
    if (!rc) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dense_assemble), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
    }
    return rc;
}
// ---- the launches that the host-first Newton step and the launched-ahead one (host_step.inc ahead_enqueue_step) both issue: one site each ----
// Assembly of K = Q + sigma_f I + A' diag(d) A, and what becomes of the right-hand side in the same launch:
enum { ASM_RHS_NONE,        // nothing: the solve loads its own (k_dense_load_rhs)
       ASM_RHS_COPY,        // d->rhs is copied, padded, for the one-launch factorization that follows
       ASM_RHS_FORM };      // launch-ahead: extra workgroups form rhs = -res_dual_in - A't themselves (EpiRhs' work); the launch looks at the
                            // device's decision first (spec) and takes the kept factor's sigma_f in branch 1
static void launch_dense_assemble(QpdoDev *d, int rhs_mode, double sigma_f) {
    const int n = d->n, ld = d->dense_ld;
    const int g = ld < 1024 ? ld : 1024;
    // the assembly's accumulator is an LDS tile of up to DENSE_ASM_TILE_MAX rows (QPDO_DENSE_ASM_TILE: a smaller tile, for the tests
    // of the tiled path at small n); larger orders are assembled in several row tiles per column -- the same bits
    const int asm_tile = n < d->dense_asm_tile ? (n > 0 ? n : 1) : d->dense_asm_tile;
    const bool form = rhs_mode == ASM_RHS_FORM;
    AsmRhs ar{};
    int gR = 0;
    if (form) {
        ar.on = 1; ar.g0 = g; ar.tpr = d->At.tpr; ar.nrows = d->At.nrows; ar.rp = d->At.rp; ar.ci = d->At.ci; ar.val = d->At.val; ar.x = d->dy;
        ar.rdi = d->res_dual_in; ar.atdy = d->Atdy; ar.rhs = d->rhs;
        gR = (d->At.nrows + 64 / ar.tpr - 1) / (64 / ar.tpr); if (gR > 1024) gR = 1024; if (gR < 1) gR = 1;
        d->st.spmv_calls++; d->st.spmv_bytes += (int64_t)d->At.alg_bytes();
    }
    hipLaunchKernelGGL(k_dense_assemble, dim3(g + gR), dim3(64), (size_t)asm_tile * sizeof(double), d->stream, n, ld, asm_tile, d->Qf.rp, d->Qf.ci, d->Qf.val,
                       d->At.rp, d->At.ci, d->At.val, d->Ar.rp, d->Ar.ci, d->Ar.val, (const double *)d->d, sigma_f, d->Kd,
                       rhs_mode == ASM_RHS_COPY ? (const double *)d->rhs : (const double *)nullptr, d->dxw, (unsigned long long *)d->dz, (unsigned long long *)d->ch_x,
                       form ? (const Ctrl *)d->ctrl : (const Ctrl *)nullptr, form ? d->sigma_f : 0.0, ar);
}
// mid-size order: every tile of the lower triangle has a workgroup of its own, the factorization is ONE launch (dev/mid_kernels.inc); with_rhs:
// nb more workgroups carry the forward solve of the right-hand side that the assembly launch left in dxw (padded, with the sentinels of the
// polled vectors); spec = 1: launch-ahead, the kernel leaves if the device decided against a Newton step
static void launch_mid_factor(QpdoDev *d, bool with_rhs, int spec) {
    const int nb = d->dense_nblk;
    hipLaunchKernelGGL(k_mid_factor, dim3(nb * (nb + 1) / 2 + (with_rhs ? nb : 0)), dim3(256), MID_LDS_DOUBLES * 8, d->stream, d->Kd, d->n, d->dense_ld, nb, d->Dg,
                       d->Linv, d->LinvT, with_rhs ? (const double *)d->dxw : (const double *)nullptr, d->dz, d->ch_y, d->mid_flags, ++d->mid_epoch, d->ctrl,
                       d->mid_C, d->mid_dinv, spec);
}
// one chained triangular solve per right-hand side (grid: right-hand side x block row), block rows chained through polled device-scope
// loads: FWD: out = D^-1 L^-1 src (ld entries each), else out = L^-T src (the first nout entries; out may be null); pub: the polled vector
extern "C++" template <bool FWD>
static void launch_ldl_chain(QpdoDev *d, int nrhs, const double *src, double *pub, double *out, int nout, int spec = 0) {
    hipLaunchKernelGGL(k_ldl_chain<FWD>, dim3(nrhs, d->dense_nblk), dim3(256), 0, d->stream, (const double *)d->Kd, d->dense_ld, d->dense_nblk,
                       (const double *)(FWD ? d->Linv : d->LinvT), (const double *)d->Dg, src, pub, out, nout, d->ctrl, spec);
}
// A factorization of the current (sigma_f, d) has just been enqueued: the one place that books it.  fwd_carried: its launch left the
// forward solve of d->rhs in ch_y and no solve has used it yet.  The factor belongs to this weight vector and no row holds a low-rank
// slot: d_fact and wb_slot follow where they exist.  (Neither can fire for a launched-ahead step, which must enqueue nothing the
// host-first step does not: ahead_route_ok requires !wb_enable && !ud_cap.  d_fact exists only if one of the two was set when
// dense_alloc ran, dense_alloc allocates once per workspace, and both are fixed at setup (d->cfg) -- only a lost producer clears them,
// together with dense_chain, which takes the workspace off the launch-ahead route until the configuration is put back as a whole.  A change that lets the configuration be
// read again after the allocation must guard the copy.)
static int dense_factor_enqueued(QpdoDev *d, bool onelaunch, bool fwd_carried) {
    d->mid_fwd_valid = fwd_carried ? 1 : 0;
    if (onelaunch) d->st.onelaunch_factors++;
    d->st.factor_count++;
    d->dense_valid = 1;
    d->dense_factored = 1; d->dense_fact_sigma = d->sigma_f; d->wb_k = 0; d->ud_dirty = 0;
    if (d->d_fact && d->m > 0) HIPCHK(hipMemcpyAsync(d->d_fact, d->d, (size_t)d->m * 8, hipMemcpyDeviceToDevice, d->stream));
    if (d->wb_enable && d->m > 0) HIPCHK(hipMemsetAsync(d->wb_slot, 0xFF, (size_t)d->m * sizeof(int), d->stream));
    return 0;
}
// with_rhs: the caller's next solve is K x = d->rhs -- a mid-size factorization then carries the forward solve along (k_mid_factor)
static int dense_factor(QpdoDev *d, bool with_rhs = false) {
    int rc = dense_alloc(d); if (rc) return rc;
    d->mid_fwd_valid = 0;
    const int n = d->n, ld = d->dense_ld, nb = d->dense_nblk;
    // look-ahead pays from n ~ 7000 up (tools/dense_lookahead_crossover.sh, factor ms with | without: n = 2000: 1.60 | 1.46, 4000: 3.39 | 3.18,
    // 6000: 5.82 | 5.72, 7000: 7.24 | 7.35, 8000: 8.85 | 9.14, 1e4: 13.4 | 14.0, 12288: 22.2 | 23.9): below, the two streams only slow each other
    const bool lookahead = d->dense_lookahead >= 0 ? d->dense_lookahead != 0 : n >= 7000;
    const bool mid = d->dense_mid && d->dense_chain && d->mid_flags && nb <= MID_MAX_NB;
    launch_dense_assemble(d, (mid && with_rhs) ? ASM_RHS_COPY : ASM_RHS_NONE, d->sigma_f);
    if (mid) {
        launch_mid_factor(d, with_rhs, 0);
        HIPCHK(hipGetLastError());
        return dense_factor_enqueued(d, true, with_rhs);
    }
    // Outer panel p (DOUTER block columns): F_p = its factorization (a serial diag -> panel -> narrow update chain that
    // fills few CUs), a_p = trailing update of the NEXT outer panel's columns, b_p = trailing update of everything
    // beyond.  One-deep look-ahead: F_p, a_p on the main stream, b_p on stream2, so that F_{p+1} overlaps b_p.
    //   F_p <- a_{p-1};  a_p, b_p <- F_p, b_{p-1};  W_p lives in buffer p&1 (F_{p+1} <- a_p <- b_{p-1}: its reader is done).
    // Every element of K receives the same updates in the same order as without look-ahead: results are bit-identical.
    auto syrk = [&](hipStream_t st, const double *W, int kb0, int nkb, int wcol0, int tj_lo, int tj_hi) {
        dim3 grid(nb - tj_lo, tj_hi - tj_lo);
        int nb_swz = 0;
        if (nkb > 1) {                                      // wide updates: 1-D grid in the L2-friendly tile order
            const int nt = syrk_tiles(nb - tj_lo, tj_hi - tj_lo);
            grid = dim3((nt + 7) / 8 * 8, 1); nb_swz = nb;
        }
        hipLaunchKernelGGL(k_ldl_syrk, grid, dim3(256), 0, st, d->Kd, ld, W, kb0, nkb, wcol0, tj_lo, tj_hi, nb_swz);
    };
    hipStream_t sc = d->stream;
    bool b_pending = false;
    int p = 0;
    for (int J0 = 0; J0 < nb; J0 += DOUTER, p++) {
        const int Jend = J0 + DOUTER < nb ? J0 + DOUTER : nb;
        double *W = d->Wd + (size_t)(p & 1) * ld * DNB * DOUTER;
        for (int kb = J0; kb < Jend; kb++) {
            hipLaunchKernelGGL(k_ldl_diag_blocked, dim3(1), dim3(256), 0, sc, d->Kd, ld, kb, d->Dg, d->Linv, d->LinvT);
            const int below = nb - kb - 1;
            if (below > 0) {
                hipLaunchKernelGGL(k_ldl_panel, dim3(below), dim3(256), 0, sc, d->Kd, ld, kb, kb - J0, (const double *)d->Dg,
                                   (const double *)d->Linv, W);
                if (kb + 1 < Jend) syrk(sc, W, kb, 1, kb - J0, kb + 1, Jend);      // rest of this outer panel
            }
        }
        if (Jend < nb) {
            const int Jend2 = (lookahead && Jend + DOUTER < nb) ? Jend + DOUTER : nb;
            if (Jend2 < nb) {
                HIPCHK(hipEventRecord(d->evF[p & 1], sc));
                HIPCHK(hipStreamWaitEvent(d->stream2, d->evF[p & 1], 0));
            }
            if (b_pending) HIPCHK(hipStreamWaitEvent(sc, d->evB[(p - 1) & 1], 0));
            b_pending = false;
            syrk(sc, W, J0, Jend - J0, 0, Jend, Jend2);                             // a_p
            if (Jend2 < nb) {
                syrk(d->stream2, W, J0, Jend - J0, 0, Jend2, nb);                          // b_p
                HIPCHK(hipEventRecord(d->evB[p & 1], d->stream2));
                b_pending = true;
            }
        }
    }
    if (b_pending) HIPCHK(hipStreamWaitEvent(sc, d->evB[(p - 1) & 1], 0));
    HIPCHK(hipGetLastError());
    return dense_factor_enqueued(d, false, false);
}
// z0 = K0^-1 src; the result (ld entries) is at d->dsol; dst (optional, n entries) receives a copy
static int dense_solve_core(QpdoDev *d, const double *src, double *dst = nullptr) {
    const int n = d->n, ld = d->dense_ld, nb = d->dense_nblk;
    const bool fwd_done = d->mid_fwd_valid && src == d->rhs && d->dense_chain;      // the factorization's launch left D^-1 L^-1 rhs in ch_y
    d->mid_fwd_valid = 0;
    if (!fwd_done) LAUNCH(k_dense_load_rhs, vgrid(ld), n, ld, src, d->dxw, d->dense_chain ? d->dz : (double *)nullptr, d->ch_x);
    if (d->dense_chain) {          // one launch per direction, block rows chained through polled device-scope loads
        if (!fwd_done) launch_ldl_chain<true>(d, 1, d->dxw, d->dz, d->ch_y, ld);
        launch_ldl_chain<false>(d, 1, d->ch_y, d->ch_x, dst, n);
        d->dsol = d->ch_x;
        return 0;
    }
    for (int kb = 0; kb < nb; kb++) {
        const int below = nb - kb - 1;
        hipLaunchKernelGGL(k_ldl_fwd, dim3(below > 0 ? below : 1), dim3(64), 0, d->stream, (const double *)d->Kd, ld, kb, (const double *)d->Linv, d->dxw, d->dz);
    }
    LAUNCH(k_dense_scale_d, vgrid(ld), ld, (const double *)d->dz, (const double *)d->Dg, d->dz);
    for (int kb = nb - 1; kb >= 0; kb--)
        hipLaunchKernelGGL(k_ldl_bwd, dim3(kb > 0 ? kb : 1), dim3(64), 0, d->stream, (const double *)d->Kd, ld, kb, (const double *)d->Linv, d->dz, d->dxw);
    d->dsol = d->dxw;
    if (dst) HIPCHK(hipMemcpyAsync(dst, d->dsol, (size_t)n * 8, hipMemcpyDeviceToDevice, d->stream));
    return 0;
}
__global__ void k_add_to(int n, const double *__restrict__ a, double *__restrict__ y) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = y[i] + a[i];
}
// r = rhs - K dx on the true K = Q + sigma_f I + A' diag(d) A by three SpMV, into pc_r; its inf-norm into N_B of the control block.
// (Defined in host_probe.inc, beside its other caller: the EpiResid products are instantiated where they first appear outside a
// template, and that place decides where their kernels sit in the code object -- it stays where it has been.)
static void true_residual(QpdoDev *d);
static const double WB_RES_TOL = 1e-13;    // relative inf-norm residual accepted for a low-rank solve
static const int WB_MAX_REFINE = 5;
// Residual check and refinement of a solve whose inner solver is not a fresh factorization (the low-rank path, an up/downdated factor):
// the true residual (true_residual), accepted at WB_RES_TOL relative to |rhs|inf; up to WB_MAX_REFINE
// sweeps, a sweep that does not reduce the residual fourfold ends them and is accepted only near the floor.  inner(it) enqueues sweep
// it: dx (it = 0) or its correction from r (in d->pc_r); guard() is asked after each read-back and ends the sweeps without acceptance.
// The one copy of the acceptance rule; *ok = 0: the caller refactors.
extern "C++" template <class Inner, class Guard>
static int dense_refine_checked(QpdoDev *d, Inner inner, Guard guard, bool *ok) {
    const int n = d->n;
    *ok = false;
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_mul, vgrid(n), n, (const double *)d->rhs, (const double *)nullptr, d->ctrl, N_A);
    double prev = 0.0;
    for (int it = 0; it <= WB_MAX_REFINE; it++) {
        int rc = inner(it); if (rc) return rc;
        true_residual(d);
        bool go = true;
        rc = guard(&go); if (rc) return rc;                  // (reads the control block back)
        const double nb_ = nrm_of(d->hctrl, N_A), nr_ = nrm_of(d->hctrl, N_B);
        if (!go) break;
        if (nr_ <= WB_RES_TOL * nb_) { *ok = true; break; }
        if (it > 0 && !(nr_ < 0.25 * prev)) { *ok = nr_ <= 1e3 * WB_RES_TOL * nb_; break; }      // stalled: accept only near the floor
        prev = nr_;
    }
    return 0;
}
// A solve with a kept factor that carries in-place up/downdates (d->ud_dirty; dev/updown.inc).  A downdate of a heavy row cancels
// digits of D and L (the recurrence itself does: tests/test_dense_updown_cpu.py), so the result is checked exactly as the low-rank path
// checks its own (dense_refine_checked), with the updated factor as the inner solver.  A failed check -- or the latch of a scan that
// refused a row, which arrives with the same read-back -- refactors and solves again.
static int dense_solve_updown(QpdoDev *d) {
    const int n = d->n;
    bool ok = false;
    int rc = dense_refine_checked(d, [&](int it) -> int {
        if (it == 0) return dense_solve_core(d, d->rhs, d->dx);
        int rci = dense_solve_core(d, d->pc_r); if (rci) return rci;
        LAUNCH(k_add_to, vgrid(n), n, (const double *)d->dsol, d->dx);
        return 0;
    }, [&](bool *go) -> int {
        int rcg = read_ctrl(d); if (rcg) return rcg;
        *go = d->hctrl->cnt[C_UD_REJECT] == 0;
        return 0;
    }, &ok);
    if (rc) return rc;
    if (ok) { d->st.updown_solves++; return 0; }
    d->st.updown_rejects++;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_UD_REJECT, 0);
    rc = dense_factor(d); if (rc) return rc;
    return dense_solve_core(d, d->rhs, d->dx);
}
static int dense_solve(QpdoDev *d) {
    const int n = d->n, ld = d->dense_ld, k = d->wb_k;
    if (k == 0 && d->ud_dirty) return dense_solve_updown(d);
    int rc = dense_solve_core(d, d->rhs, k == 0 ? d->dx : (double *)nullptr); if (rc) return rc;
    if (k == 0) return 0;
    // Low-rank path.  One application  e = z0 - Z (I + W G)^-1 W U z0,  z0 = K0^-1 r,  is the solve with the updated
    // matrix in exact arithmetic, but the correction cancels the part of z0 along the new rows: with weights 1/mu
    // up to 1e9 that costs log10(w a'K0^-1 a) digits (measured: 1e-4 relative residual on a 200 x 400 instance).
    // So it is used as the inner solver of an iterative refinement on the true K = Q + sigma I + A' diag(d) A
    // (three SpMV per sweep) until the residual is at the level of a fresh factorization; a sweep that stalls, a
    // NaN or a tiny pivot of I + W G (a downdate removing most of a direction of K0) falls back to refactoring.
    bool ok = false;
    rc = dense_refine_checked(d, [&](int it) -> int {
        if (it > 0) { int rci = dense_solve_core(d, d->pc_r); if (rci) return rci; }
        hipLaunchKernelGGL(k_wb_v, dim3(k), dim3(64), 0, d->stream, (const int *)d->wb_rows, d->Ar.rp, d->Ar.ci, d->Ar.val, (const double *)d->dsol,
                           (const double *)d->d, (const double *)d->d_fact, d->wb_v, d->wb_w);
        hipLaunchKernelGGL(k_wb_lu, dim3(1), dim3(1024), k <= WB_LDS_MAX ? (size_t)k * (k + 2) * 8 : 0, d->stream, k, (const double *)d->wb_G, (const double *)d->wb_w,
                           (const double *)d->wb_v, d->wb_t, d->wb_M);
        if (it == 0) {
            LAUNCH(k_wb_apply, vgrid(n), n, ld, k, (const double *)d->wb_Z, (const double *)d->wb_t, (const double *)d->dsol, d->dx);
        } else {
            LAUNCH(k_wb_apply, vgrid(n), n, ld, k, (const double *)d->wb_Z, (const double *)d->wb_t, (const double *)d->dsol, d->pc_z);
            LAUNCH(k_add_to, vgrid(n), n, (const double *)d->pc_z, d->dx);
        }
        return 0;
    }, [&](bool *go) -> int {
        double minpiv = 0.0;
        HIPCHK(hipMemcpyAsync(&minpiv, d->wb_t + WB_MAX, sizeof(double), hipMemcpyDeviceToHost, d->stream));
        int rcg = read_ctrl(d); if (rcg) return rcg;
        d->st.lowrank_sweeps++;
        *go = minpiv >= WB_MIN_PIVOT;
        return 0;
    }, &ok);
    if (rc) return rc;
    if (ok) { d->st.lowrank_solves++; return 0; }
    d->st.lowrank_rejects++;
    rc = dense_factor(d); if (rc) return rc;
    return dense_solve_core(d, d->rhs, d->dx);
}
// Give every row whose weight differs from the factored one a low-rank slot; new slots get their column of
// Z = K0^-1 U' (one chained solve per column, all columns advancing together) and their row and column of G.  *overflow = 1: more
// than WB_MAX rows differ, the caller refactors.
static int wb_extend(QpdoDev *d, int *overflow) {
    const int ld = d->dense_ld, k_old = d->wb_k;
    *overflow = 0;
    hipLaunchKernelGGL(k_wb_select, dim3(1), dim3(1024), 0, d->stream, d->m, (const double *)d->d, (const double *)d->d_fact, d->wb_slot, d->wb_rows,
                       k_old, d->wb_cnt);
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d->wb_cnt, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (cnt > WB_MAX) { *overflow = 1; return 0; }
    const int k_new = cnt - k_old;
    if (k_new <= 0) return 0;
    double *X = d->wb_Z + (size_t)k_old * ld, *T = d->wb_T + (size_t)k_old * ld;
    hipLaunchKernelGGL(k_wb_rhs, dim3(k_new), dim3(256), 0, d->stream, ld, k_old, k_new, (const int *)d->wb_rows, d->Ar.rp, d->Ar.ci, d->Ar.val, d->wb_Z);
    {
        // the new columns as independent chained solves, all advancing together (grid: right-hand side x block row):
        // X -> z (polled, in T) and y = D^-1 z (in T2), then y -> the solution (polled, back in X)
        double *T2 = d->wb_T2 + (size_t)k_old * ld;
        const int tot = ld * k_new;
        LAUNCH(k_fill_sentinel, vgrid(tot), tot, T, T);
        launch_ldl_chain<true>(d, k_new, X, T, T2, ld);
        LAUNCH(k_fill_sentinel, vgrid(tot), tot, X, X);
        launch_ldl_chain<false>(d, k_new, T2, X, nullptr, 0);
    }
    hipLaunchKernelGGL(k_wb_G, dim3(cnt, k_new), dim3(64), 0, d->stream, k_old, (const int *)d->wb_rows, d->Ar.rp, d->Ar.ci, d->Ar.val,
                       (const double *)d->wb_Z, ld, d->wb_G);
    HIPCHK(hipGetLastError());
    d->wb_k = cnt;
    d->st.lowrank_cols += k_new;
    return 0;
}
// In-place up/downdate of the kept factor (dev/updown.inc) for the rows whose weight differs from the factored one.  *applied = 0: more
// than d->ud_cap rows differ and nothing was touched (the caller takes the path it took without this route); 1: the rows -- possibly
// none -- are in the stream one after another (chained forward solve, scan + tile products, streaming pass), d_fact follows on the
// device, no factorization.  A row whose scan refuses it stops there and behind it: the solve that follows reads the latch.
static int ud_apply(QpdoDev *d, int *applied) {
    const int ld = d->dense_ld, nb = d->dense_nblk;
    *applied = 0;
    int cnt = 0;
    if (d->m > 0) {
        hipLaunchKernelGGL(k_ud_select, dim3(1), dim3(1024), 0, d->stream, d->m, (const double *)d->d, (const double *)d->d_fact, d->ud_cap, d->ud_rows, d->ud_cnt);
        HIPCHK(hipMemcpyAsync(&cnt, d->ud_cnt, sizeof(int), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    if (cnt > d->ud_cap) return 0;
    *applied = 1;
    if (cnt == 0) return 0;
    d->mid_fwd_valid = 0;
    hipLaunchKernelGGL(k_ud_load, dim3(cnt), dim3(256), 0, d->stream, ld, (const int *)d->ud_rows, d->Ar.rp, d->Ar.ci, d->Ar.val, d->ud_a, d->ud_p, d->ud_q);
    for (int k = 0; k < cnt; k++) {
        const double *a = d->ud_a + (size_t)k * ld, *p = d->ud_p + (size_t)k * ld, *q = d->ud_q + (size_t)k * ld;
        launch_ldl_chain<true>(d, 1, a, (double *)p, (double *)q, ld);
        hipLaunchKernelGGL(k_ud_prep, dim3(nb, nb + 1), dim3(256), 0, d->stream, (const double *)d->Kd, ld, nb, (const double *)d->Dg, p, q,
                           (const int *)d->ud_rows, k, (const double *)d->d, (const double *)d->d_fact, d->ud_G, d->ud_Dn, d->ud_beta, d->ctrl);
        hipLaunchKernelGGL(k_ud_apply, dim3(nb, nb), dim3(256), 0, d->stream, d->Kd, ld, nb, d->Dg, d->Linv, d->LinvT, a, p, (const double *)d->ud_G,
                           (const double *)d->ud_Dn, (const double *)d->ud_beta, (const int *)d->ud_rows, k, (const double *)d->d, d->d_fact, (const Ctrl *)d->ctrl);
    }
    HIPCHK(hipGetLastError());
    d->ud_dirty = 1;
    d->st.updown_rows += cnt;              // rows SENT: one that its scan refuses, and the rows behind it, never touch the factor (updown_rejects then counts the pass)
    return 0;
}
// Bring the kept factor up to date with the current (sigma_f, d) when it is not known to be (d->dense_valid = 0) -- the one copy of the
// rule, for the Newton pass and for the test hook that drives the solver as a pass does (host_probe.inc qdev_direct_solve).  As the
// reference: a full factorization where it is forced (branch 0, newton.c:21-33), where there is no factor or sigma_f moved; otherwise
// the rows whose weight moved change the kept factor -- in place for up to ud_cap of them (QPDO_DENSE_UPDOWN; no low-rank slot held: its
// columns belong to the factor as it was), through low-rank slots where wb_enable is set -- and whatever neither route takes (more rows
// than WB_MAX, or no low-rank path) refactors.  carry_fwd: a factorization launch takes the forward solve of d->rhs along.
static int dense_refresh_factor(QpdoDev *d, bool force_full, bool carry_fwd) {
    bool full = force_full || !d->dense_factored || d->sigma_f != d->dense_fact_sigma;
    int rc = 0, updated = 0;
    if (!full && d->ud_cap > 0 && d->wb_k == 0) { rc = ud_apply(d, &updated); if (rc) return rc; }
    if (updated) { d->dense_valid = 1; return 0; }
    if (!d->wb_enable) full = true;
    if (!full) {
        int overflow = 0;
        rc = wb_extend(d, &overflow); if (rc) return rc;
        if (!overflow) { d->dense_valid = 1; return 0; }
    }
    return dense_factor(d, carry_fwd);
}
// a fresh factorization of this pass's matrix, then the solve of K dx = d->rhs with it
static int dense_factor_and_solve(QpdoDev *d, bool carry_fwd) {
    int rc = dense_factor(d, carry_fwd); if (rc) return rc;
    return dense_solve(d);
}
