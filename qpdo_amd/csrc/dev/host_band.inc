// host_band.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side of the band direct solver (dev/band.inc)

// half-bandwidth of every Newton matrix this workspace can produce (pattern of Q + A'A), or -1 when it is not a band worth the name
// QPDO_BAND_COUPLING = R > 0: the rows of A wider than BAND_MAX_B are counted first (k_bc_classify).  1 .. R of them over a core -- Q and the
// other rows -- of half-bandwidth <= BAND_MAX_B: band_b is the core's and bc_r their number (dev/band.inc, the coupled mode); more than
// R: not banded (bc_over keeps the count for setup's message); none, or a core that is too wide: the rule over all rows, as without R.
static int band_detect(QpdoDev *d) {
    d->band_b = -1; d->bc_r = 0; d->bc_over = 0;
    if (d->comm.active || d->n < 8) return 0;
    if (d->bo_newold) {                                  // a variable order: its half-bandwidth was measured where the order was made (band_order.c)
        const int b = d->bo_b < 3 ? 3 : d->bo_b;
        if (b <= BAND_WIDE_MAX_B) d->band_b = b;
        return 0;
    }
    int cls[3] = {0, 0, 0};                             // coupling rows, the largest span of the other rows, of all rows
    if (d->band_coupling > 0 && d->m > 0) {
        int rc = 0;
        if (!d->bc_rows) { rc = dev_alloc(d, &d->bc_rows, (size_t)BC_MAX); if (!rc) rc = dev_alloc(d, &d->bc_info, (size_t)4); if (rc) return rc; }
        hipLaunchKernelGGL(k_bc_classify, dim3(1), dim3(1024), 0, d->stream, d->m, (const int *)d->Ar.rp, (const int *)d->Ar.ci, BC_MAX, d->bc_rows, d->bc_info);
        HIPCHK(hipMemcpyAsync(cls, d->bc_info, sizeof(cls), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    const bool coupled = cls[0] > 0;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_VIOL, 0);
    if (d->m > 0 && !coupled) LAUNCH(k_band_span_A, vgrid(d->m), d->m, (const int *)d->Ar.rp, (const int *)d->Ar.ci, &d->ctrl->cnt[C_VIOL]);
    LAUNCH(k_band_span_Q, vgrid(d->n), d->n, (const int *)d->Qf.rp, (const int *)d->Qf.ci, &d->ctrl->cnt[C_VIOL]);
    int rc = read_ctrl(d); if (rc) return rc;
    int b = d->hctrl->cnt[C_VIOL];                      // (coupled: Q's bandwidth alone)
    if (coupled) {
        if (cls[0] > d->band_coupling) { d->bc_over = cls[0]; return 0; }
        if (b <= BAND_MAX_B && cls[1] <= BAND_MAX_B) {
            d->bc_r = cls[0];
            d->bc_rows_h.resize((size_t)d->bc_r);
            HIPCHK(hipMemcpyAsync(d->bc_rows_h.data(), d->bc_rows, (size_t)d->bc_r * sizeof(int), hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
            if (cls[1] > b) b = cls[1];
        } else if (cls[2] > b) b = cls[2];
    }
    if (b < 3) b = 3;                                   // (the four-column step reads a 4 x 4 leading block)
    if (b <= BAND_WIDE_MAX_B) d->band_b = b;
    return 0;
}
// b > BAND_MAX_B: the tiled storage of dev/band_wide.inc, 8 np (64 (w + 2) + 129) bytes -- 0.9 GB at n = 1e5, b = 1023
static int band_wide_alloc(QpdoDev *d) {
    if (d->bw_Wb) return 0;
    d->band_np = (d->n + DNB - 1) / DNB * DNB;
    d->bw_w = (d->band_b + DNB - 1) / DNB;
    const size_t nbc = (size_t)d->band_np / DNB, tiles = nbc * (size_t)(d->bw_w + 1);
    const size_t bytes = (tiles + 3 * nbc) * BW_T * 8 + 2 * (size_t)d->band_np * 8;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + ((size_t)256 << 20) > free_b) {
        snprintf(g_err, sizeof(g_err), "band solver: n = %d, half-bandwidth %d needs %.2f GB of device memory, %.2f GB are free", d->n, d->band_b,
                 (double)bytes * 1e-9, (double)free_b * 1e-9);
        return -1;
    }
    int rc = dev_alloc(d, &d->bw_Wdiag, nbc * BW_T);
    if (!rc) rc = dev_alloc(d, &d->bw_Wd, (size_t)d->band_np);
    if (!rc) rc = dev_alloc(d, &d->bw_Li, nbc * BW_T);
    if (!rc) rc = dev_alloc(d, &d->bw_LiT, nbc * BW_T);
    if (!rc) rc = dev_alloc(d, &d->band_z, (size_t)d->band_np);
    if (!rc) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bw_panel), hipFuncAttributeMaxDynamicSharedMemorySize, BW_PANEL_LDS * 8);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bw_update), hipFuncAttributeMaxDynamicSharedMemorySize, BW_UPDATE_LDS * 8);
        if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
    }
    if (!rc) rc = dev_alloc(d, &d->bw_Wb, tiles * BW_T);           // (last: its presence says the workspace is complete)
    return rc;
}
// assembly, then two launches per block column (dev/band_wide.inc)
static int band_wide_factor(QpdoDev *d) {
    int rc = band_wide_alloc(d); if (rc) return rc;
    const int n = d->n, np = d->band_np, b = d->band_b, w = d->bw_w, nbc = np / DNB;
    int g = (np + 3) / 4; if (g > 4096) g = 4096;
    if (d->bo_newold)
        hipLaunchKernelGGL(k_bw_assemble_perm, dim3(g), dim3(256), 0, d->stream, n, np, b, w, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                           (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->bw_Wb, d->bw_Wdiag, (const int *)d->bo_newold, (const int *)d->bo_oldnew);
    else
        hipLaunchKernelGGL(k_bw_assemble, dim3(g), dim3(256), 0, d->stream, n, np, b, w, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                           (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->bw_Wb, d->bw_Wdiag);
    for (int k = 0; k < nbc; k++) {
        const int wk = nbc - 1 - k < w ? nbc - 1 - k : w;          // tiles below the diagonal one in block column k
        hipLaunchKernelGGL(k_bw_panel, dim3(wk > 0 ? wk : 1), dim3(256), BW_PANEL_LDS * 8, d->stream, k, w, nbc, d->bw_Wb, (const double *)d->bw_Wdiag,
                           d->bw_Wd, d->bw_Li, d->bw_LiT, &d->ctrl->cnt[C_CHAIN_ERR]);
        if (wk > 0) hipLaunchKernelGGL(k_bw_update, dim3(wk * (wk + 1) / 2), dim3(256), BW_UPDATE_LDS * 8, d->stream, k, w, d->bw_Wb, d->bw_Wdiag, (const double *)d->bw_Wd);
    }
    HIPCHK(hipGetLastError());
    d->dense_valid = 1; d->st.factor_count++;
    return 0;
}
static int band_alloc(QpdoDev *d) {
    if (d->band_b > BAND_MAX_B) return band_wide_alloc(d);
    if (d->Kb) return 0;
    d->band_np = ((d->bb_c > 0 ? d->bb_ncore : d->n) + 3) & ~3;
    const size_t cnt = (size_t)d->band_np * (d->band_b + 1);
    int rc = dev_alloc(d, &d->Kb, cnt);
    if (!rc) rc = dev_alloc(d, &d->Lt, cnt);
    if (!rc) rc = dev_alloc(d, &d->band_z, (size_t)d->band_np);
    if (!rc) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_factor<256, BAND_MAX_B>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e == hipSuccess && d->bo_newold) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve_perm), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e == hipSuccess && d->bc_r > 0) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve_multi), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e == hipSuccess && d->bb_c > 0) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve_group), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
    }
    if (!rc && d->bb_c > 0) {                            // bordered mode: three np x c arrays (C, forward results, Z), the c x c blocks
        const size_t cols = (size_t)d->band_np * (size_t)d->bb_c;
        rc = dev_alloc(d, &d->bb_C, cols);
        if (!rc) rc = dev_alloc(d, &d->bb_T, cols);
        if (!rc) rc = dev_alloc(d, &d->bb_Z, cols);
        if (!rc) rc = dev_alloc(d, &d->bb_D, (size_t)BC_MAX * BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bb_S, (size_t)BC_MAX * BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bb_SL, (size_t)BC_MAX * BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bb_t, (size_t)BC_MAX);
    }
    if (!rc && d->bc_r > 0) {                           // coupled mode: three np x r arrays (right-hand sides, forward results, Z), the k x k system
        const size_t cols = (size_t)d->band_np * (size_t)d->bc_r, mm = (size_t)d->m;
        rc = dev_alloc(d, &d->bc_dcore, mm);
        if (!rc) rc = dev_alloc(d, &d->bc_dfact, mm);
        if (!rc) rc = dev_alloc(d, &d->bc_U, cols);
        if (!rc) rc = dev_alloc(d, &d->bc_T, cols);
        if (!rc) rc = dev_alloc(d, &d->bc_Z, cols);
        if (!rc) rc = dev_alloc(d, &d->bc_S, (size_t)BC_MAX * BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bc_SL, (size_t)BC_MAX * BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bc_t, (size_t)BC_MAX);
        if (!rc) rc = dev_alloc(d, &d->bc_z0, (size_t)d->band_np);
    }
    return rc;
}
// Coupled mode: bring the factor of B, the columns of Z and the factored S up to date with the current (sigma_f, d).  The band factor and
// the columns of Z it produced stay while the core weights and sigma_f are the kept ones (compared on the device, one read-back); a
// coupling row whose weight became nonzero since gets its column of Z now; S is built and factored for the weighted coupling rows.  When
// only coupling weights moved nothing else runs and factor_count does not move.
static int band_coupled_refresh(QpdoDev *d, bool force) {
    int rc = band_alloc(d); if (rc) return rc;
    const int n = d->n, m = d->m, np = d->band_np, b = d->band_b, r = d->bc_r;
    HIPCHK(hipMemsetAsync(d->bc_info, 0, sizeof(int), d->stream));
    LAUNCH(k_bc_prepare, vgrid(m), m, r, (const int *)d->bc_rows, (const double *)d->d, d->bc_dcore, (const double *)d->bc_dfact, d->bc_info);
    int info[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(info, d->bc_info, sizeof(info), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const int k = info[1];
    const u64 act = (u64)(u32)info[2] | (u64)(u32)info[3] << 32;
    if (force || !d->bc_factored || d->sigma_f != d->bc_fact_sigma || info[0]) {
        int g = (np + 3) / 4; if (g > 4096) g = 4096;
        hipLaunchKernelGGL(k_band_assemble, dim3(g), dim3(256), 0, d->stream, n, np, b, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                           (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->bc_dcore, d->sigma_f, d->Kb);
        const size_t lds = ((size_t)(b + 4) * (b + 1) + 8 * (size_t)(b + 4)) * sizeof(double);
        hipLaunchKernelGGL((k_band_factor<256, BAND_MAX_B>), dim3(1), dim3(256), lds, d->stream, np, b, d->Kb, d->Lt, &d->ctrl->cnt[C_CHAIN_ERR]);
        HIPCHK(hipMemcpyAsync(d->bc_dfact, d->bc_dcore, (size_t)m * 8, hipMemcpyDeviceToDevice, d->stream));
        d->bc_factored = 1; d->bc_fact_sigma = d->sigma_f; d->bc_zvalid = 0; d->st.factor_count++;
    }
    const u64 todo = act & ~d->bc_zvalid;
    if (todo) {
        const size_t lds = (size_t)4 * BAND_SC * (b + 1) * sizeof(double);
        hipLaunchKernelGGL(k_band_solve_multi, dim3(__builtin_popcountll(todo)), dim3(256), lds, d->stream, n, np, b, (const double *)d->Kb, (const double *)d->Lt, todo,
                           (const int *)d->bc_rows, (const int *)d->Ar.rp, (const int *)d->Ar.ci, (const double *)d->Ar.val, d->bc_U, d->bc_T, d->bc_Z);
        d->bc_zvalid |= todo;
    }
    if (k > 0) {
        hipLaunchKernelGGL(k_bc_S, dim3(k, k), dim3(64), 0, d->stream, act, (const int *)d->bc_rows, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->d, (const double *)d->bc_Z, np, d->bc_S);
        hipLaunchKernelGGL(k_bc_factor_S, dim3(1), dim3(256), 0, d->stream, k, (const double *)d->bc_S, d->bc_SL, &d->ctrl->cnt[C_CHAIN_ERR]);
    }
    HIPCHK(hipGetLastError());
    d->bc_act = act; d->bc_k = k; d->dense_valid = 1;
    return 0;
}
// Bordered mode (dev/band.inc): the factor of the core B, the border columns [C; D], Z = B^-1 C and the factored S = D - C'Z for the
// current (sigma_f, d).  Five launches behind the assembly, whatever c is; no read-back.  The core goes through the plain band solver's
// two kernels with n = n_core: k_band_assemble drops what lands at a row >= n, so the border variables never reach the band and Kb holds
// the bits of a plain band workspace on the problem without the border columns.
static int band_border_refresh(QpdoDev *d) {
    int rc = band_alloc(d); if (rc) return rc;
    const int nc = d->bb_ncore, np = d->band_np, b = d->band_b, c = d->bb_c;
    int g = (np + 3) / 4; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_band_assemble, dim3(g), dim3(256), 0, d->stream, nc, np, b, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                       (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                       (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->Kb);
    const size_t lds_f = ((size_t)(b + 4) * (b + 1) + 8 * (size_t)(b + 4)) * sizeof(double), lds_s = (size_t)4 * BAND_SC * (b + 1) * sizeof(double);
    hipLaunchKernelGGL((k_band_factor<256, BAND_MAX_B>), dim3(1), dim3(256), lds_f, d->stream, np, b, d->Kb, d->Lt, &d->ctrl->cnt[C_CHAIN_ERR]);
    hipLaunchKernelGGL(k_bb_assemble, dim3(c), dim3(1024), 0, d->stream, nc, np, c, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                       (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                       (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->bb_C, d->bb_D);
    hipLaunchKernelGGL(k_band_solve_group, dim3(c), dim3(256), lds_s, d->stream, nc, np, b, (const double *)d->Kb, (const double *)d->Lt,
                       (const double *)d->bb_C, (long long)np, d->bb_T, d->bb_Z);
    hipLaunchKernelGGL(k_bb_S, dim3(c, c), dim3(256), 0, d->stream, nc, np, (const double *)d->bb_C, (const double *)d->bb_Z, (const double *)d->bb_D, d->bb_S);
    hipLaunchKernelGGL(k_bc_factor_S, dim3(1), dim3(256), 0, d->stream, c, (const double *)d->bb_S, d->bb_SL, &d->ctrl->cnt[C_CHAIN_ERR]);
    HIPCHK(hipGetLastError());
    d->dense_valid = 1; d->st.factor_count++;
    return 0;
}
// force (coupled mode only): factor B again even where the kept factor's weights and sigma_f are the current ones
static int band_factor(QpdoDev *d, bool force = false) {
    if (d->band_b > BAND_MAX_B) return band_wide_factor(d);
    if (d->bb_c > 0) return band_border_refresh(d);
    if (d->bc_r > 0) return band_coupled_refresh(d, force);
    int rc = band_alloc(d); if (rc) return rc;
    const int n = d->n, np = d->band_np, b = d->band_b;
    int g = (np + 3) / 4; if (g > 4096) g = 4096;
    if (d->bo_newold)
        hipLaunchKernelGGL(k_band_assemble_perm, dim3(g), dim3(256), 0, d->stream, n, np, b, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                           (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->Kb, (const int *)d->bo_newold, (const int *)d->bo_oldnew);
    else
        hipLaunchKernelGGL(k_band_assemble, dim3(g), dim3(256), 0, d->stream, n, np, b, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                           (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                           (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->Kb);
    const size_t lds = ((size_t)(b + 4) * (b + 1) + 8 * (size_t)(b + 4)) * sizeof(double);
    // (a one-wave variant for narrow bands -- no workgroup barrier at all -- was measured slower: 76.6 against 57.0 ms at n = 2e5, b = 3)
    hipLaunchKernelGGL((k_band_factor<256, BAND_MAX_B>), dim3(1), dim3(256), lds, d->stream, np, b, d->Kb, d->Lt, &d->ctrl->cnt[C_CHAIN_ERR]);
    d->dense_valid = 1; d->st.factor_count++;
    return 0;
}
// Coupled mode with k = d->bc_k > 0 weighted coupling rows: ONE Woodbury application out = z0 - Z S^-1 (U' z0), z0 = B^-1 v, three
// launches, no read-back and no latch of its own.  band_solve wraps it in the residual-checked refinement of a Newton pass; the
// sensitivity calls (dev/adjoint.inc adj_sweeps) take it as it is -- their sweep loop already refines on the true system.
static int band_coupled_apply(QpdoDev *d, const double *v, double *out) {
    const int n = d->n, np = d->band_np, k = d->bc_k;
    const size_t lds = (size_t)4 * BAND_SC * (d->band_b + 1) * sizeof(double);
    hipLaunchKernelGGL(k_band_solve, dim3(1), dim3(256), lds, d->stream, n, d->band_b, (const double *)d->Kb, (const double *)d->Lt, v, d->band_z, d->bc_z0);
    hipLaunchKernelGGL(k_bc_t, dim3(1), dim3(1024), 0, d->stream, k, d->bc_act, (const int *)d->bc_rows, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                       (const double *)d->Ar.val, (const double *)d->bc_z0, (const double *)d->bc_SL, d->bc_t);
    LAUNCH(k_bc_apply, vgrid(n), n, np, k, d->bc_act, (const double *)d->bc_Z, (const double *)d->bc_t, (const double *)d->bc_z0, out);
    return 0;
}
// d->rhs -> d->dx, both in the caller's order; a workspace with a variable order launches the _perm instance of the same kernel (one launch
// per solve either way: the gather and the scatter are that kernel's first loads and last stores)
static int band_solve(QpdoDev *d) {
    if (d->band_b > BAND_MAX_B) {
        if (d->bo_newold) {
            hipLaunchKernelGGL(k_bw_solve_perm, dim3(1), dim3(256), 0, d->stream, d->n, d->band_np / DNB, d->bw_w, (const double *)d->bw_Wb, (const double *)d->bw_Li,
                               (const double *)d->bw_LiT, (const double *)d->bw_Wd, (const double *)d->rhs, d->band_z, d->dx, (const int *)d->bo_newold);
            return 0;
        }
        hipLaunchKernelGGL(k_bw_solve, dim3(1), dim3(256), 0, d->stream, d->n, d->band_np / DNB, d->bw_w, (const double *)d->bw_Wb, (const double *)d->bw_Li,
                           (const double *)d->bw_LiT, (const double *)d->bw_Wd, (const double *)d->rhs, d->band_z, d->dx);
        return 0;
    }
    const size_t lds = (size_t)4 * BAND_SC * (d->band_b + 1) * sizeof(double);
    if (d->bb_c > 0) {
        // Bordered mode: rhs and dx carry the border entries behind the core's, so nothing is gathered.  z0 = B^-1 rhs_1 goes straight
        // into dx, t = S^-1 (rhs_2 - C'z0), then dx_1 -= Z t and dx_2 = t in place: three launches, a plain direct solve.
        const int nc = d->bb_ncore, np = d->band_np, c = d->bb_c;
        hipLaunchKernelGGL(k_band_solve, dim3(1), dim3(256), lds, d->stream, nc, d->band_b, (const double *)d->Kb, (const double *)d->Lt, (const double *)d->rhs, d->band_z, d->dx);
        hipLaunchKernelGGL(k_bb_t, dim3(1), dim3(1024), 0, d->stream, nc, np, c, (const double *)d->bb_C, (const double *)d->dx, (const double *)d->rhs + nc,
                           (const double *)d->bb_SL, d->bb_t);
        LAUNCH(k_bb_apply, vgrid(d->n), nc, np, c, (const double *)d->bb_Z, (const double *)d->bb_t, d->dx);
        d->st.border_solves++;
        return 0;
    }
    if (d->bc_k > 0) {
        // Coupled mode with k weighted coupling rows: x = z0 - Z S^-1 (U' z0), z0 = B^-1 v, as the inner solver of the refinement on the
        // true K that the dense low-rank path uses (dense_refine_checked: its acceptance rule, its sweeps).  A solve that misses the check,
        // like a latched pivot of B or S, sets the latch of the band fallback: the device skips the pass's iterate update, and the
        // host hands the pass and the rest of the solve to another solver (host_step.inc step_redo_if_lost).
        const int n = d->n, k = d->bc_k;
        bool ok = false, latched = false;
        int rc = dense_refine_checked(d, [&](int it) -> int {
            band_coupled_apply(d, it == 0 ? d->rhs : d->pc_r, it == 0 ? d->dx : d->pc_z);
            if (it > 0) LAUNCH(k_add_to, vgrid(n), n, (const double *)d->pc_z, d->dx);
            return 0;
        }, [&](bool *go) -> int {
            int rcg = read_ctrl(d); if (rcg) return rcg;
            d->st.coupled_sweeps++;
            latched = d->hctrl->cnt[C_CHAIN_ERR] != 0;
            if (d->defl_debug) fprintf(stderr, "[band coupled] pass %lld: k = %d, sweep |r|inf / |rhs|inf = %.3e\n", (long long)d->st.newton_passes, k, nrm_of(d->hctrl, N_B) / nrm_of(d->hctrl, N_A));
            *go = !latched;
            return 0;
        }, &ok);
        if (rc) return rc;
        if (ok) { d->st.coupled_solves++; return 0; }
        if (!latched) { d->st.coupled_rejects++; LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 2); }
        if (d->defl_debug) fprintf(stderr, "[band coupled] pass %lld: k = %d, %s; last sweep |r|inf = %.3e, |rhs|inf = %.3e\n", (long long)d->st.newton_passes, k,
                                   latched ? "bad pivot latched" : "residual check missed", nrm_of(d->hctrl, N_B), nrm_of(d->hctrl, N_A));
        return 0;
    }
    if (d->bo_newold) {
        hipLaunchKernelGGL(k_band_solve_perm, dim3(1), dim3(256), lds, d->stream, d->n, d->band_b, (const double *)d->Kb, (const double *)d->Lt, (const double *)d->rhs,
                           d->band_z, d->dx, (const int *)d->bo_newold);
        return 0;
    }
    hipLaunchKernelGGL(k_band_solve, dim3(1), dim3(256), lds, d->stream, d->n, d->band_b, (const double *)d->Kb, (const double *)d->Lt, (const double *)d->rhs, d->band_z, d->dx);
    return 0;
}
