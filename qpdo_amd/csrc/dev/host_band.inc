// host_band.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side of the band direct solver (dev/band.inc)

// half-bandwidth of every Newton matrix this workspace can produce (pattern of Q + A'A), or -1 when it is not a band worth the name
static int band_detect(QpdoDev *d) {
    d->band_b = -1;
    if (d->comm.active || d->n < 8) return 0;
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_VIOL, 0);
    if (d->m > 0) LAUNCH(k_band_span_A, vgrid(d->m), d->m, (const int *)d->Ar.rp, (const int *)d->Ar.ci, &d->ctrl->cnt[C_VIOL]);
    LAUNCH(k_band_span_Q, vgrid(d->n), d->n, (const int *)d->Qf.rp, (const int *)d->Qf.ci, &d->ctrl->cnt[C_VIOL]);
    int rc = read_ctrl(d); if (rc) return rc;
    int b = d->hctrl->cnt[C_VIOL];
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
    d->band_np = (d->n + 3) & ~3;
    const size_t cnt = (size_t)d->band_np * (d->band_b + 1);
    int rc = dev_alloc(d, &d->Kb, cnt);
    if (!rc) rc = dev_alloc(d, &d->Lt, cnt);
    if (!rc) rc = dev_alloc(d, &d->band_z, (size_t)d->band_np);
    if (!rc) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_factor<256, BAND_MAX_B>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_band_solve), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048);
        if (e != hipSuccess) rc = set_err(e, "hipFuncSetAttribute", __LINE__);
    }
    return rc;
}
static int band_factor(QpdoDev *d) {
    if (d->band_b > BAND_MAX_B) return band_wide_factor(d);
    int rc = band_alloc(d); if (rc) return rc;
    const int n = d->n, np = d->band_np, b = d->band_b;
    int g = (np + 3) / 4; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_band_assemble, dim3(g), dim3(256), 0, d->stream, n, np, b, (const int *)d->Qf.rp, (const int *)d->Qf.ci, (const double *)d->Qf.val,
                       (const int *)d->At.rp, (const int *)d->At.ci, (const double *)d->At.val, (const int *)d->Ar.rp, (const int *)d->Ar.ci,
                       (const double *)d->Ar.val, (const double *)d->d, d->sigma_f, d->Kb);
    const size_t lds = ((size_t)(b + 4) * (b + 1) + 8 * (size_t)(b + 4)) * sizeof(double);
    // (a one-wave variant for narrow bands -- no workgroup barrier at all -- was measured slower: 76.6 against 57.0 ms at n = 2e5, b = 3)
    hipLaunchKernelGGL((k_band_factor<256, BAND_MAX_B>), dim3(1), dim3(256), lds, d->stream, np, b, d->Kb, d->Lt, &d->ctrl->cnt[C_CHAIN_ERR]);
    d->dense_valid = 1; d->st.factor_count++;
    return 0;
}
static int band_solve(QpdoDev *d) {
    if (d->band_b > BAND_MAX_B) {
        hipLaunchKernelGGL(k_bw_solve, dim3(1), dim3(256), 0, d->stream, d->n, d->band_np / DNB, d->bw_w, (const double *)d->bw_Wb, (const double *)d->bw_Li,
                           (const double *)d->bw_LiT, (const double *)d->bw_Wd, (const double *)d->rhs, d->band_z, d->dx);
        return 0;
    }
    const size_t lds = (size_t)4 * BAND_SC * (d->band_b + 1) * sizeof(double);
    hipLaunchKernelGGL(k_band_solve, dim3(1), dim3(256), lds, d->stream, d->n, d->band_b, (const double *)d->Kb, (const double *)d->Lt, (const double *)d->rhs, d->band_z, d->dx);
    return 0;
}
