// host_update.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C) of qpdo_amd_update_matrices --
// new values of Q and A in the setup's pattern, and the workspace back in the state qpdo_setup leaves (DESIGN.md 3.5)

extern "C++" {
template <class T>
static int upd_alloc(QpdoDev *d, T **p, size_t count) {      // long-lived, no zero fill (every entry is written before it is read)
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    d->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}
}
static void upd_free(QpdoDev *d, void *p) {                  // a long-lived buffer whose check failed
    if (!p) return;
    (void)hipStreamSynchronize(d->stream);
    for (size_t i = 0; i < d->allocs.size(); i++) if (d->allocs[i] == p) { d->allocs.erase(d->allocs.begin() + (long)i); break; }
    (void)hipFree(p);
}
// *differs = 1 where a[0..na) != b[0..nb) (both on the device)
static int upd_compare(QpdoDev *d, TempAllocs &tmp, const int *a, const int *b, long long cnt, int *differs) {
    int *flag = nullptr;
    if (tmp.get(&flag, 1)) return set_err(hipErrorOutOfMemory, "update scratch", __LINE__);
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), d->stream));
    if (cnt > 0) hipLaunchKernelGGL(k_cmp_int, dim3(vgrid(cnt)), dim3(BLK), 0, d->stream, cnt, a, b, flag);
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *differs |= h;
    return 0;
}
static void upd_colptr(const QdevCsc *h, std::vector<long long> &out) {
    out.resize((size_t)h->ncols + 1);
    for (size_t j = 0; j <= (size_t)h->ncols; j++) out[j] = h->itype == 0 ? (long long)((const int32_t *)h->p)[j] : (long long)((const int64_t *)h->p)[j];
}
static bool upd_colptr_same(const QdevCsc *h, const std::vector<long long> &ref) {
    if (ref.size() != (size_t)h->ncols + 1) return false;
    for (size_t j = 0; j <= (size_t)h->ncols; j++)
        if ((h->itype == 0 ? (long long)((const int32_t *)h->p)[j] : (long long)((const int64_t *)h->p)[j]) != ref[j]) return false;
    return true;
}
static int upd_grid(long long len) { long long g = (len + BLK - 1) / BLK; return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g); }   // 32 waves per CU
static int pattern_error(const char *which) {
    snprintf(g_err, sizeof(g_err), "qpdo_amd_update_matrices: the pattern of %s differs from the one given to qpdo_setup (a new pattern needs a new setup)", which);
    return -1;
}

// The first time a caller's Q is seen (qdev_update_matrices, qdev_adjoint with dQx): its (p, i) against the workspace's full CSR(Q) on the
// device, *differs |= 1 where the pattern is another one.  stype 0: Qf IS the caller's CSC arrays.  stype +-1: setup's symmetric
// expansion is run again with index payloads, which also gives *mapQ (per entry of Qf, the caller's position of the stored entry it
// came from) and *stage (room for the caller's stored values); both are long-lived allocations that the caller adopts, or hands to
// upd_free when the call is refused.  Writes nothing of the workspace.
static int upd_first_Q(QpdoDev *d, TempAllocs &tmp, const QdevCsc *Q, int *differs, u32 **mapQ, double **stage) {
    const int n = d->n;
    int rc = 0;
    if (Q->stype == 0) {
        DevCsr P;
        if (Q->nnz != d->Qf.nnz) { *differs |= 1; return 0; }
        rc = upload_csc_as_csr_of_transpose(d, tmp, &P, Q, true, false);
        if (!rc) rc = upd_compare(d, tmp, P.rp, d->Qf.rp, (long long)n + 1, differs);
        if (!rc) rc = upd_compare(d, tmp, P.ci, d->Qf.ci, Q->nnz, differs);
        return rc;
    }
    DevCsr S, R; int *cnt = nullptr, *tsum = nullptr, *orp = nullptr, *oci = nullptr; u32 *permR = nullptr, *iota = nullptr;
    rc = upload_csc_as_csr_of_transpose(d, tmp, &S, Q, true, false);
    if (!rc && (tmp.get(&permR, (size_t)S.nnz) || tmp.get(&iota, (size_t)S.nnz) || tmp.get(&cnt, (size_t)n + 1) || tmp.get(&tsum, (size_t)scan_tiles(n)) || tmp.get(&orp, (size_t)n + 1)))
        rc = set_err(hipErrorOutOfMemory, "update scratch", __LINE__);
    if (!rc) rc = dev_transpose(d, tmp, S, &R, true, permR);
    int total = 0;
    if (!rc) {
        hipLaunchKernelGGL(k_sym_count, dim3(vgrid(n)), dim3(BLK), 0, d->stream, n, Q->stype, (const int *)R.rp, (const int *)R.ci, (const int *)S.rp, (const int *)S.ci, cnt);
        dev_scan(d, cnt, n, orp, orp + n, tsum);
        hipError_t e = hipMemcpyAsync(&total, orp + n, sizeof(int), hipMemcpyDeviceToHost, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) rc = set_err(e, "symmetric expansion", __LINE__);
    }
    if (!rc && (long long)total != d->Qf.nnz) { *differs |= 1; return 0; }
    if (!rc && tmp.get(&oci, (size_t)total)) rc = set_err(hipErrorOutOfMemory, "update scratch", __LINE__);
    if (!rc) rc = upd_alloc(d, mapQ, (size_t)total);
    if (!rc) rc = upd_alloc(d, stage, (size_t)S.nnz);
    if (!rc) {
        hipLaunchKernelGGL(k_iota_u32, dim3(vgrid(S.nnz)), dim3(BLK), 0, d->stream, (long long)S.nnz, iota);
        hipLaunchKernelGGL(k_sym_fill<u32>, dim3(2048), dim3(BLK), 0, d->stream, n, Q->stype, (const int *)R.rp, (const int *)R.ci, (const u32 *)permR,
                           (const int *)S.rp, (const int *)S.ci, (const u32 *)iota, (const int *)orp, oci, *mapQ);
        rc = upd_compare(d, tmp, orp, d->Qf.rp, (long long)n + 1, differs);
    }
    if (!rc) rc = upd_compare(d, tmp, oci, d->Qf.ci, total, differs);
    return rc;
}

// The first time the position of CSR(A)'s entries in the caller's CSC arrays is needed (qdev_update_matrices, qdev_tangent with tAx):
// setup's transposition of the CSC arrays again, its permutation kept as *mapA -- a long-lived allocation that the caller adopts, or hands
// to upd_free when the call fails -- and the result compared with the workspace's CSR(A).  who: the entry point's name, for the message.
// Writes nothing of the workspace.
static int upd_first_mapA(QpdoDev *d, TempAllocs &tmp, u32 **mapA, const char *who) {
    DevCsr R;
    int differs = 0;
    int rc = upd_alloc(d, mapA, (size_t)d->At.nnz);
    if (!rc) rc = dev_transpose(d, tmp, d->At, &R, true, *mapA);
    if (!rc) rc = upd_compare(d, tmp, R.rp, d->Ar.rp, (long long)d->m + 1, &differs);
    if (!rc) rc = upd_compare(d, tmp, R.ci, d->Ar.ci, d->Ar.nnz, &differs);
    if (!rc && differs) { snprintf(g_err, sizeof(g_err), "%s: CSR(A) of the workspace is not the transposition of its CSC arrays", who); rc = -1; }
    return rc;
}

// Every piece of workspace state that outlives one solve, back to its value after create_tail + qdev_configure.  The pattern-only
// decisions of setup stay (linsolve's automatic choice, band_b, max_row_nnz_A, the slab tables: band_detect and k_max_row_len read rp / ci
// only); buffers whose contents are only read under a validity flag keep their contents (the dense / band factors, the Woodbury slots).
static int reset_to_setup_state(QpdoDev *d) {
    const size_t n = (size_t)d->n, m = (size_t)d->m;
    d->Ar.sm_dirty = d->At.sm_dirty = d->Qf.sm_dirty = d->Qs.sm_dirty = 1;
    d->Arc.sm_dirty = d->Atc.sm_dirty = 1;
    d->qdiag_valid = 0; d->dense_valid = 0; d->dense_factored = 0; d->mid_fwd_valid = 0;
    d->wb_k = 0; d->dense_fact_sigma = 0.0; d->dense_last_branch = -1; d->dense_last_sigma = -1.0; d->sigma_f = 0.0;
    d->hybrid_active = 0; d->schur_off = 0; d->schur_strikes = 0; d->last_jacobi_iters = 0; d->schur_last_inner = 0; d->pcg_abs_now = -1.0;
    for (int &v : d->sweep_last_inner) v = 0;
    d->ahead_inflight = 0; d->ahead_branch = -1; d->ahead_sigma_f02 = 0.0; d->ahead_spmv_calls0 = 0; d->ahead_spmv_bytes0 = 0;
    d->tail_shift = 0; d->tail_muchg = 0; d->tail_sigma = 0; d->tail_dsig = 0.0;
    d->step_pending = 0; d->axpy_pending = 0; d->ctrl_clean = 0; d->defer_step = 0; d->pend_proximal = 0; d->pend_sigma = 0.0; d->cur_proximal = 1;
    d->kact = 0; d->kg = 0; d->defl_r = 0; d->defl_passes = 0; d->schur_passes = 0;
    // what a solve may have switched (fallbacks of the linear solvers, the hybrid's hand-over)
    d->linsolve = d->cfg.linsolve; d->dense_chain = d->cfg.dense_chain; d->dense_mid = d->cfg.dense_mid; d->dense_lookahead = d->cfg.dense_lookahead;
    d->wb_enable = d->cfg.wb_enable; d->ud_cap = d->cfg.ud_cap; d->deflate = d->cfg.deflate; d->pcg_maxit = d->cfg.pcg_maxit; d->band_b = d->cfg.band_b;
    d->bc_r = d->cfg.bc_r; d->bc_factored = 0; d->bc_k = 0;      // (the coupling rows are the pattern's, like band_b; the kept factor of B is not)
    d->st = QdevStats{}; d->st.linsolve = d->linsolve;
    d->ev_spmv_ms = 0; d->ev_spmv_n = 0; d->ev_ac_ms = 0; d->ev_ac_bytes = 0; d->ev_ac_n = 0;
    // the vectors and control blocks as dev_alloc left them: zero (q, l, u are written by the caller next; D, E by the scaling)
    double *vn[] = {d->x, d->xbar, d->Qx, d->Aty, d->df, d->res_dual, d->res_dual_in, d->rhs, d->dx, d->Qdx, d->Atdy, d->D, d->Dinv,
                    d->pc_r, d->pc_z, d->pc_p, d->pc_Kp, d->pc_diag, d->tmp_n, d->qdiag};
    double *vm[] = {d->y, d->ybar, d->Ax, d->mu, d->isq, d->w, d->res_prim, d->res_prim_old, d->res_prim_in, d->dy, d->Adx, d->d, d->E, d->Einv,
                    d->pc_t, d->at_scale, d->tmp_m, d->s_x, d->s_r, d->s_z, d->s_p, d->s_Sp, d->s_diag, d->s_v, d->s_s, d->s_acc, d->dc, d->tc};
    for (double *p : vn) HIPCHK(hipMemsetAsync(p, 0, n * 8, d->stream));
    if (m) {
        for (double *p : vm) HIPCHK(hipMemsetAsync(p, 0, m * 8, d->stream));
        int *im[] = {d->active, d->active_old, d->mu_changed};
        for (int *p : im) HIPCHK(hipMemsetAsync(p, 0, m * sizeof(int), d->stream));
    }
    HIPCHK(hipMemsetAsync(d->ctrl, 0, sizeof(Ctrl), d->stream));
    HIPCHK(hipMemsetAsync(d->ctrl2, 0, sizeof(Ctrl), d->stream));
    return 0;
}

void qdev_set_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

// setup of a scaled workspace: the unscaled values, before qdev_scale_data rewrites them (one device copy each)
int qdev_keep_raw_values(QpdoDev *d) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) return 0;                              // (row-partitioned workspaces cannot be updated)
    int rc = upd_alloc(d, &d->rawA, (size_t)d->At.nnz);
    if (!rc) rc = upd_alloc(d, &d->rawQ, (size_t)d->Qf.nnz);
    if (rc) return rc;
    if (d->At.nnz) HIPCHK(hipMemcpyAsync(d->rawA, d->At.val, (size_t)d->At.nnz * 8, hipMemcpyDeviceToDevice, d->stream));
    if (d->Qf.nnz) HIPCHK(hipMemcpyAsync(d->rawQ, d->Qf.val, (size_t)d->Qf.nnz * 8, hipMemcpyDeviceToDevice, d->stream));
    return 0;
}

int qdev_update_matrices(QpdoDev *d, const QdevCsc *A, const QdevCsc *Q, const double *q, const double *l, const double *u) {
    HIPCHK(hipSetDevice(d->device));
    if (d->comm.active) { snprintf(g_err, sizeof(g_err), "qpdo_amd_update_matrices: row-partitioned workspaces are not supported (set up anew)"); return -1; }
    HIPCHK(hipStreamSynchronize(d->stream));
    const int n = d->n;
    const bool needA = A || d->rawA;                           // CSR(A) is rewritten (new values, or the raw copy scaled again)
    const bool gatherQ = Q && Q->stype != 0;
    int rc = 0, differs = 0;
    u32 *newMapA = nullptr, *newMapQ = nullptr; double *newStage = nullptr;
    // ---- checks: nothing of the workspace is written before they pass --------------------------------------------------------------
    {
        TempAllocs tmp;
        if (A && A->nnz != d->At.nnz) rc = pattern_error("A");
        if (!rc && A && !d->upd_Ap.empty() && !upd_colptr_same(A, d->upd_Ap)) rc = pattern_error("A");
        if (!rc && A && d->upd_Ap.empty()) {                   // first time: the caller's (p, i) against CSR(A') = the setup's CSC arrays
            DevCsr P;
            rc = upload_csc_as_csr_of_transpose(d, tmp, &P, A, true, false);
            if (!rc) rc = upd_compare(d, tmp, P.rp, d->At.rp, (long long)n + 1, &differs);
            if (!rc) rc = upd_compare(d, tmp, P.ci, d->At.ci, A->nnz, &differs);
            if (!rc && differs) rc = pattern_error("A");
        }
        if (!rc && needA && !d->mapA) rc = upd_first_mapA(d, tmp, &newMapA, "qpdo_amd_update_matrices");
        const bool firstQ = Q && d->upd_Qp.empty();
        if (!rc && Q && !firstQ && !upd_colptr_same(Q, d->upd_Qp)) rc = pattern_error("Q");
        if (!rc && firstQ) rc = upd_first_Q(d, tmp, Q, &differs, &newMapQ, &newStage);
        if (!rc && firstQ && differs) rc = pattern_error("Q");
        if (!rc) { hipError_t e = hipGetLastError(); if (e != hipSuccess) rc = set_err(e, "update checks", __LINE__); }
        tmp.release(d->stream);
        h2d_staging_release(d);
    }
    if (rc) { upd_free(d, newMapA); upd_free(d, newMapQ); upd_free(d, newStage); return rc; }
    // ---- the checks passed: maps, values, state -------------------------------------------------------------------------------------
    if (newMapA) d->mapA = newMapA;
    if (newMapQ) { d->mapQ = newMapQ; d->qstage = newStage; }
    if (A && d->upd_Ap.empty()) upd_colptr(A, d->upd_Ap);
    if (Q && d->upd_Qp.empty()) upd_colptr(Q, d->upd_Qp);
    double *srcA = d->rawA ? d->rawA : d->At.val;
    if (A && A->nnz) rc = h2d_staged(d, srcA, A->x, (size_t)A->nnz * 8);
    if (!rc && Q && Q->nnz) rc = h2d_staged(d, gatherQ ? d->qstage : (d->rawQ ? d->rawQ : d->Qf.val), Q->x, (size_t)Q->nnz * 8);
    if (rc) { h2d_staging_release(d); return rc; }
    const long long nA = needA ? d->At.nnz : 0, nQ = (gatherQ || d->rawQ) ? d->Qf.nnz : 0;
    if (nA || nQ)
        hipLaunchKernelGGL(k_update_values, dim3(upd_grid(nA > nQ ? nA : nQ)), dim3(BLK), 0, d->stream, nA, (const double *)srcA, d->rawA ? d->At.val : (double *)nullptr,
                           (const u32 *)d->mapA, needA ? d->Ar.val : (double *)nullptr, nQ, gatherQ ? (const double *)d->qstage : (const double *)nullptr,
                           (const u32 *)d->mapQ, d->rawQ, d->Qf.val);
    rc = reset_to_setup_state(d);
    if (!rc) rc = h16_refresh_scale(d);          // (new values of A: a new scale of the half-precision images)
    if (!rc) {
        HIPCHK(hipMemcpyAsync(d->q, q, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
        if (d->m) { HIPCHK(hipMemcpyAsync(d->l, l, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream)); HIPCHK(hipMemcpyAsync(d->u, u, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream)); }
        HIPCHK(hipStreamSynchronize(d->stream));
        HIPCHK(hipGetLastError());
    }
    h2d_staging_release(d);
    return rc;
}
