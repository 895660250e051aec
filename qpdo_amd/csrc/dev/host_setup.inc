// host_setup.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C): create/destroy, configuration, scaling, warm start

int qdev_rccl_unique_id(void *out128) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
    memcpy(out128, &id, sizeof(id) < 128 ? sizeof(id) : 128);
    return 0;
}
int qdev_device_count(void) { int c = 0; if (hipGetDeviceCount(&c) != hipSuccess) return 0; return c; }
const char *qdev_last_error(void) { return g_err; }

static int create_tail(QpdoDev *d, int32_t n, int32_t m, const double *q, const double *l, const double *u, const QdevDist *dist, int max_row_nnz_A);
static int band_detect(QpdoDev *d);      // host_band.inc

// qpdo_setup's intake on ONE GPU: the caller's CSC arrays go up as they are; CSR(A) and the full symmetric CSR(Q) are built on the device
int qdev_create_csc(QpdoDev **out, int device, int32_t n, int32_t m, const QdevCsc *A, const QdevCsc *Q, const double *q, const double *l, const double *u) {
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    QpdoDev *d = new QpdoDev();
    d->device = device; d->n = n; d->m = m; d->mloc = m; d->nloc = n;
    QdevDist none; memset(&none, 0, sizeof(none)); none.world = 1; none.mloc = m; none.nloc = n;
    hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete d; return set_err(e, "hipStreamCreate", __LINE__); }
    TempAllocs tmp;
    int rc = upload_csc_as_csr_of_transpose(d, tmp, &d->At, A, false);            // CSR(A') = the CSC arrays of A
    if (!rc) rc = dev_transpose(d, tmp, d->At, &d->Ar, false);                       // CSR(A)
    tmp.release(d->stream);
    if (!rc) {
        if (Q->stype == 0) rc = upload_csc_as_csr_of_transpose(d, tmp, &d->Qf, Q, false);       // full storage of a symmetric matrix: its own transpose
        else {
            DevCsr S, R;
            rc = upload_csc_as_csr_of_transpose(d, tmp, &S, Q, true);
            if (!rc) rc = dev_transpose(d, tmp, S, &R, true);
            int *cnt = nullptr, *tsum = nullptr;
            if (!rc && (tmp.get(&cnt, (size_t)n + 1) || tmp.get(&tsum, (size_t)scan_tiles(n)))) rc = set_err(hipErrorOutOfMemory, "setup scratch", __LINE__);
            if (!rc) {
                d->Qf.nrows = d->Qf.ncols = n;
                rc = dev_alloc(d, &d->Qf.rp, (size_t)n + 1);
            }
            if (!rc) {
                hipLaunchKernelGGL(k_sym_count, dim3(vgrid(n)), dim3(BLK), 0, d->stream, n, Q->stype, (const int *)R.rp, (const int *)R.ci, (const int *)S.rp, (const int *)S.ci, cnt);
                dev_scan(d, cnt, n, d->Qf.rp, d->Qf.rp + n, tsum);
                int total = 0;
                e = hipMemcpyAsync(&total, d->Qf.rp + n, sizeof(int), hipMemcpyDeviceToHost, d->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
                if (e != hipSuccess) rc = set_err(e, "symmetric expansion", __LINE__);
                d->Qf.nnz = total;
            }
            if (!rc) rc = dev_alloc(d, &d->Qf.ci, (size_t)d->Qf.nnz);
            if (!rc) rc = dev_alloc(d, &d->Qf.val, (size_t)d->Qf.nnz);
            if (!rc) {
                hipLaunchKernelGGL(k_sym_fill<double>, dim3(2048), dim3(BLK), 0, d->stream, n, Q->stype, (const int *)R.rp, (const int *)R.ci, (const double *)R.val,
                                   (const int *)S.rp, (const int *)S.ci, (const double *)S.val, (const int *)d->Qf.rp, d->Qf.ci, d->Qf.val);
                d->Qf.tpr = pick_tpr(d->Qf);
            }
        }
    }
    tmp.release(d->stream);
    if (!rc) { e = hipGetLastError(); if (e != hipSuccess) rc = set_err(e, "setup conversions", __LINE__); }
    if (!rc) rc = create_tail(d, n, m, q, l, u, &none, -1);
    h2d_staging_release(d);
    if (rc) { qdev_destroy(d); return rc; }
    d->st.linsolve = 0;
    *out = d;
    return 0;
}

int qdev_create(QpdoDev **out, int device, int32_t n, int32_t m, const QdevCsr *Ar, const QdevCsr *At, const QdevCsr *Qf,
                const double *q, const double *l, const double *u) {
    QdevDist none; memset(&none, 0, sizeof(none));
    none.world = 1; none.mloc = m; none.nloc = n;
    return qdev_create_dist(out, device, n, m, Ar, At, Qf, (const QdevCsr *)nullptr, q, l, u, &none);
}
int qdev_create_dist(QpdoDev **out, int device, int32_t n, int32_t m, const QdevCsr *Ar, const QdevCsr *At, const QdevCsr *Qf,
                     const QdevCsr *Qs, const double *q, const double *l, const double *u, const QdevDist *dist) {
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    QpdoDev *d = new QpdoDev();
    d->device = device; d->n = n; d->m = m;
    d->m0 = dist->m0; d->mloc = dist->mloc; d->n0 = dist->n0; d->nloc = dist->nloc;
    d->comm.rank = dist->rank; d->comm.world = dist->world; d->comm.fn = dist->fn; d->comm.ctx = dist->ctx;
    d->comm.active = dist->world > 1 || dist->force;
    d->comm.mode = d->comm.active ? (dist->fn ? 1 : 2) : 0;
    int rc = 0;
    hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete d; return set_err(e, "hipStreamCreate", __LINE__); }
    if (!rc) rc = upload_csr(d, &d->Ar, Ar);
    if (!rc) rc = upload_csr(d, &d->At, At);
    if (!rc) rc = upload_csr(d, &d->Qf, Qf);
    if (!rc && Qs && d->comm.active) rc = upload_csr(d, &d->Qs, Qs);
    int mx = 0;
    for (int i = 0; i < Ar->nrows; i++) { const int len = Ar->rp[i + 1] - Ar->rp[i]; if (len > mx) mx = len; }
    if (!rc) rc = create_tail(d, n, m, q, l, u, dist, mx);
    h2d_staging_release(d);      // 2 x 64 MB of pinned memory: only the uploads above needed it
    if (rc) { qdev_destroy(d); return rc; }
    d->st.linsolve = 0;
    *out = d;
    return 0;
}
// everything of a workspace but its three matrices (which are on the device when this is called): vectors, control blocks, slab
// tables, communicator, the per-pass compact copies.  max_row_nnz_A < 0: take it from the device arrays.
static int create_tail(QpdoDev *d, int32_t n, int32_t m, const double *q, const double *l, const double *u, const QdevDist *dist, int max_row_nnz_A) {
    int rc = 0;
    hipError_t e = hipSuccess;
#define A_(p, cnt) if (!rc) rc = dev_alloc(d, &d->p, (size_t)(cnt))
    A_(x, n); A_(xbar, n); A_(Qx, n); A_(Aty, n); A_(q, n); A_(df, n); A_(res_dual, n); A_(res_dual_in, n); A_(rhs, n);
    A_(dx, n); A_(Qdx, n); A_(Atdy, n); A_(D, n); A_(Dinv, n);
    A_(pc_r, n); A_(pc_z, n); A_(pc_p, n); A_(pc_Kp, n); A_(pc_diag, n); A_(tmp_n, n);
    A_(y, m); A_(ybar, m); A_(Ax, m); A_(l, m); A_(u, m); A_(mu, m); A_(isq, m); A_(w, m); A_(res_prim, m);
    A_(res_prim_old, m); A_(res_prim_in, m); A_(dy, m); A_(Adx, m); A_(d, m); A_(E, m); A_(Einv, m); A_(pc_t, m);
    A_(at_scale, m); A_(tmp_m, m);
    A_(active, m); A_(active_old, m); A_(mu_changed, m);
    const size_t M2 = 2 * (size_t)m;
    A_(ls_delta, M2); A_(ls_alpha, M2); A_(ls_pa, M2); A_(ls_pb, M2);
    A_(ls_key[0], M2); A_(ls_key[1], M2); A_(ls_idx[0], M2); A_(ls_idx[1], M2);
    d->rs_nblocks = (int)((M2 + RS_TILE - 1) / RS_TILE); if (d->rs_nblocks < 1) d->rs_nblocks = 1;
    A_(rs_hist, (size_t)256 * d->rs_nblocks);
    A_(scan_tsum, (size_t)(n > m ? n : m) / SCN_TILE + 2 + (size_t)256 * d->rs_nblocks / SCN_TILE);      // tiles of the longest scan: n, m or the histograms
    d->ls_nblk = (int)((M2 + LS_TILE - 1) / LS_TILE); if (d->ls_nblk < 1) d->ls_nblk = 1;
    A_(ls_bt, (size_t)2 * d->ls_nblk + 2);
    A_(ctrl, 1); A_(part, (size_t)P_COUNT * PGRID);
    A_(ctrl2, 1); A_(part2, (size_t)7 * PGRID);      // inner CG: 3 sums x 2 parities, then the n-dot partials
    A_(s_x, m); A_(s_r, m); A_(s_z, m); A_(s_p, m); A_(s_Sp, m); A_(s_diag, m); A_(s_v, m); A_(s_s, m); A_(s_acc, m);
#undef A_
    static_assert(sizeof(Ctrl) % 8 == 0 && sizeof(Ctrl) <= 64 * 8 && sizeof(Ctrl) <= CTRL_SEQ_OFF, "k_ctrl_publish copies the control block with one wave");
    if (!rc) { e = hipHostMalloc((void **)&d->hctrl, CTRL_SEQ_OFF + 64, hipHostMallocCoherent); if (e != hipSuccess) rc = set_err(e, "hipHostMalloc", __LINE__); }
    if (!rc) { e = hipHostMalloc((void **)&d->hctrl2, CTRL_SEQ_OFF + 64, hipHostMallocCoherent); if (e != hipSuccess) rc = set_err(e, "hipHostMalloc", __LINE__); }
    if (!rc) {
        d->hseq = (u64 *)((char *)d->hctrl + CTRL_SEQ_OFF); d->hseq2 = (u64 *)((char *)d->hctrl2 + CTRL_SEQ_OFF); *d->hseq = 0; *d->hseq2 = 0;
        const char *cp = getenv("QPDO_CTRL_PUBLISH"); if (cp && *cp) d->ctrl_publish = atoi(cp) != 0;
        { const char *lsm = getenv("QPDO_LS_SMALL"); if (lsm && *lsm) d->ls_small = atoi(lsm) != 0; }
        const char *fo = getenv("QPDO_FUSE_OUTER"); if (fo && *fo) d->fuse_outer = atoi(fo) != 0;
        const char *fr = getenv("QPDO_FUSE_RESID"); if (fr && *fr) d->fuse_resid = atoi(fr) != 0;      // 0: k_axpy5 and k_ctrl_publish as launches of their own
        const char *la = getenv("QPDO_LAUNCH_AHEAD"); if (la && *la) d->launch_ahead = atoi(la) != 0;  // 0: the Newton step is launched after the host has read the pass's norms
    }
    if (!rc) rc = dev_alloc(d, &d->pub_ticket, (size_t)2);
    if (!rc) {
        // (no pinned memory for it: qdev_store_solution keeps its six separate copies)
        const size_t cnt = 3 * (size_t)n + 3 * (size_t)m + 1;
        if (hipHostMalloc((void **)&d->hpack, cnt * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); d->hpack = nullptr; }
        else rc = dev_alloc(d, &d->pack, cnt);
    }
    if (!rc) { e = hipEventCreate(&d->ev0); if (e == hipSuccess) e = hipEventCreate(&d->ev1); if (e != hipSuccess) rc = set_err(e, "hipEventCreate", __LINE__); }
    if (!rc) {
        e = hipMemcpyAsync(d->q, q, (size_t)n * 8, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess && m) e = hipMemcpyAsync(d->l, l, (size_t)m * 8, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess && m) e = hipMemcpyAsync(d->u, u, (size_t)m * 8, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) rc = set_err(e, "upload", __LINE__);
    }
    if (!rc) rc = setup_slabs(d, &d->Ar);
    if (!rc) rc = setup_slabs(d, &d->At);
    if (!rc) rc = setup_slabs(d, &d->Qf);
    if (!rc && d->comm.active && d->Qs.nrows > 0) rc = setup_slabs(d, &d->Qs);
    if (!rc && d->comm.active) {
        const size_t mx = (size_t)(n > m ? n : m) + 8;      // + the scalars that ride on the n-vector payload
        rc = dev_alloc(d, &d->dist_tmp, mx);
        if (!rc) rc = dev_alloc(d, &d->Kp_part, (size_t)n);
        if (!rc) rc = dev_alloc(d, &d->zeros_n, (size_t)n);
        if (!rc && d->comm.mode == 1) { hipError_t e2 = hipHostMalloc((void **)&d->comm.hbuf, mx * 8, hipHostMallocDefault); if (e2 != hipSuccess) rc = set_err(e2, "hipHostMalloc", __LINE__); else d->comm.hcap = mx; }
        if (!rc && d->comm.mode == 2) {
            ncclUniqueId id; memcpy(&id, dist->nccl_id, sizeof(id));
            ncclResult_t r = ncclCommInitRank(&d->comm.nccl, dist->world, id, dist->rank);
            if (r != ncclSuccess) { snprintf(g_err, sizeof(g_err), "ncclCommInitRank: %s", ncclGetErrorString(r)); rc = -1; }
        }
    }
    if (!rc) {   // per-pass compact copies used by PCG
        d->Arc = d->Ar; d->Arc.rp = nullptr; d->Arc.ci = nullptr; d->Arc.val = nullptr; d->Arc.sp = nullptr; d->Arc.ci16 = nullptr;
        d->Atc = d->At; d->Atc.rp = nullptr; d->Atc.ci = nullptr; d->Atc.val = nullptr; d->Atc.sp = nullptr; d->Atc.ci16 = nullptr;
        d->Arc.vsm = nullptr; d->Arc.i16sm = nullptr; d->Arc.cism = nullptr; d->Arc.seg = nullptr; d->Arc.vsm32 = nullptr; d->Arc.vsm16 = nullptr; d->Arc.p16sm = nullptr;
        d->Atc.vsm = nullptr; d->Atc.i16sm = nullptr; d->Atc.cism = nullptr; d->Atc.seg = nullptr; d->Atc.vsm32 = nullptr; d->Atc.vsm16 = nullptr; d->Atc.p16sm = nullptr;
        { const char *f32 = getenv("QPDO_PCG_INNER_F32"); d->inner_f32 = (f32 && atoi(f32) != 0) ? 1 : 0; }
        // the default inner solve: fp32 stream, accepted on the fp64 residual (single GPU; "0": the fp64 inner CG)
        { const char *rf = getenv("QPDO_PCG_INNER_REFINE"); d->inner_refine = !(rf && *rf && atoi(rf) == 0) && !d->comm.active; }
        { const char *ms = getenv("QPDO_INNER_REFINE_MAXSWEEP"); d->refine_maxsweep = (ms && atoi(ms) > 0) ? atoi(ms) : 6; }
        { const char *th = getenv("QPDO_INNER_REFINE_THETA"); d->refine_theta = (th && atof(th) > 0 && atof(th) <= 1.0) ? atof(th) : 0.8; }
        const bool with_f32 = d->inner_f32 != 0 || d->inner_refine != 0;
        { const char *fo = getenv("QPDO_INNER_FOLD"); d->inner_fold = !(fo && *fo && atoi(fo) == 0); }
        { const char *x3 = getenv("QPDO_INNER_X32"); d->inner_x32 = !(x3 && *x3 && atoi(x3) == 0); }
        // coarse sweeps of the refined solve on half-precision images (they are pair-wide products: only with the fp32 operand vectors; never
        // under QPDO_PCG_INNER_F32=1, whose single fp32 solve has no sweeps: no image is allocated or written for it)
        { const char *h = getenv("QPDO_INNER_H16"); d->inner_h16 = !(h && *h && atoi(h) == 0) && d->inner_refine && !d->inner_f32 && d->inner_x32; }
        // 2, not the CPU model's 3: with 3 the complete C4 record's last-pass step length sits 3.57e-7 from the oracle's against the suite's
        // bound of 3e-7, with 2 at 1.3e-8.  That figure is a draw from a spread (1.3e-8 ... 3.6e-7 over eight settings), not a trend: the
        // margin is FRAGILE under any change of the inner solve (docs/LAB_NOTES.md, "16-bit matrix stream", the table)
        { const char *hs = getenv("QPDO_INNER_H16_MAXSWEEP"); d->h16_maxsweep = (hs && *hs && atoi(hs) >= 0) ? atoi(hs) : 2; }
        { const char *he = getenv("QPDO_INNER_H16_ETA"); d->h16_eta = (he && atof(he) > 0 && atof(he) < 1.0) ? atof(he) : 1e-3; }
        const bool with_h16 = d->inner_h16 != 0;
        const bool with_p16 = with_f32 && d->inner_x32;      // the images that will be in pair order (below) carry pair-local index words
        { const char *co = getenv("QPDO_COMPACT_ONE_READ"); d->compact_one_read = !(co && *co && atoi(co) == 0); }
        { const char *ct = getenv("QPDO_COMPACT_T_ONE_READ"); d->compact_t_one_read = !(ct && *ct && atoi(ct) == 0); }
        rc = dev_alloc(d, &d->Arc.rp, (size_t)m + 1);
        if (!rc) rc = dev_alloc(d, &d->Arc.ci, (size_t)d->Ar.nnz);
        if (!rc) rc = dev_alloc(d, &d->Arc.val, (size_t)d->Ar.nnz);
        if (!rc && d->Ar.use_slab) rc = dev_alloc(d, &d->Arc.sp, (size_t)m * (d->Ar.nslabs + 1));
        if (!rc && d->Ar.ci16) rc = dev_alloc(d, &d->Arc.ci16, (size_t)d->Ar.nnz);
        if (!rc && d->Ar.use_slab) rc = slab_major_alloc(d, &d->Arc, (size_t)d->Ar.nnz, (size_t)m * d->Ar.nslabs, with_f32, with_h16, with_p16);
        if (!rc) rc = dev_alloc(d, &d->Atc.rp, (size_t)n + 1);
        if (!rc) rc = dev_alloc(d, &d->Atc.ci, (size_t)d->At.nnz);
        if (!rc) rc = dev_alloc(d, &d->Atc.val, (size_t)d->At.nnz);
        if (!rc && d->At.use_slab) rc = dev_alloc(d, &d->Atc.sp, (size_t)n * (d->At.nslabs + 1));
        if (!rc && d->At.ci16) rc = dev_alloc(d, &d->Atc.ci16, (size_t)d->At.nnz);
        if (!rc && d->At.use_slab) rc = slab_major_alloc(d, &d->Atc, (size_t)d->At.nnz, (size_t)n * d->At.nslabs, with_f32, with_h16, with_p16);
        if (!rc) rc = dev_alloc(d, &d->row_cnt, (size_t)(n > m ? n : m));
        if (!rc) rc = dev_alloc(d, &d->cidx, (size_t)m);
        if (!rc) rc = dev_alloc(d, &d->rowlist, (size_t)m);
        if (!rc) rc = dev_alloc(d, &d->flag_bits, (size_t)(m + 63) / 64 + 1);
        if (!rc) rc = dev_alloc(d, &d->flag_wprefix, (size_t)(m + 63) / 64 + 1);
        if (!rc) rc = dev_alloc(d, &d->kcount, 4);
        if (!rc) rc = dev_alloc(d, &d->dc, (size_t)m);
        if (!rc) rc = dev_alloc(d, &d->tc, (size_t)m);
        if (!rc && with_f32 && d->inner_x32) { rc = dev_alloc(d, &d->s_z32, (size_t)m + 4); if (!rc) rc = dev_alloc(d, &d->tmp_n32, (size_t)n + 4); }
        // pair order only where the pair-wide products will run: the slab-by-slab products are slower on it (docs/LAB_NOTES.md)
        d->Arc.seg_pairs = (d->Arc.p16sm && d->s_z32 && d->tmp_n32) ? 1 : 0; d->Atc.seg_pairs = (d->Atc.p16sm && d->s_z32 && d->tmp_n32) ? 1 : 0;
        d->lds_doubles_At = (int)slab_cap_w((160 * 1024 - 1024) / 8 - d->At.rows_per_wg);
        if (!rc) rc = dev_alloc(d, &d->qdiag, (size_t)n);
        const char *df = getenv("QPDO_DEFLATE");
        d->deflate = !(df && !strcmp(df, "0"));
        int mx = max_row_nnz_A;
        if (mx < 0 && !rc) {                                 // (matrices built on the device: the longest row of A from its row pointers)
            LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_VIOL, 0);
            LAUNCH(k_max_row_len, vgrid(d->Ar.nrows), d->Ar.nrows, (const int *)d->Ar.rp, &d->ctrl->cnt[C_VIOL]);
            rc = read_ctrl(d);
            mx = rc ? 0 : d->hctrl->cnt[C_VIOL];
        }
        if (mx < 0) mx = 0;
        d->max_row_nnz_A = mx;
        if (d->deflate && m > 0) {
            d->Ath = DevCsr(); d->Ath.nrows = n; d->Ath.ncols = m;
            if (!rc) rc = dev_alloc(d, &d->Ath.rp, (size_t)n + 1);
            if (!rc) rc = dev_alloc(d, &d->Ath.ci, (size_t)DEFL_MAX * (mx > 0 ? mx : 1));
            if (!rc) rc = dev_alloc(d, &d->Ath.val, (size_t)DEFL_MAX * (mx > 0 ? mx : 1));
            if (!rc) rc = dev_alloc(d, &d->defl_hist, 32);
            if (!rc) rc = dev_alloc(d, &d->defl_list, DEFL_MAX);
            if (!rc) rc = dev_alloc(d, &d->defl_count, 1);
            if (!rc) rc = dev_alloc(d, &d->defl_flag, (size_t)m);
            if (!rc) rc = dev_alloc(d, &d->defl_t, (size_t)m);
            if (!rc) rc = dev_alloc(d, &d->defl_S, (size_t)DEFL_MAX * DEFL_MAX);
            if (!rc) rc = dev_alloc(d, &d->defl_Sinv, (size_t)DEFL_MAX * DEFL_MAX);
            if (!rc) rc = dev_alloc(d, &d->defl_v, DEFL_MAX);
        }
        if (!rc) rc = h16_refresh_scale(d);      // (the values as uploaded; qdev_scale_data and qdev_update_matrices take it again)
    }
    return rc;
}

void qdev_destroy(QpdoDev *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    h2d_staging_release(d);
    for (void *p : d->allocs) (void)hipFree(p);
    if (d->hctrl) (void)hipHostFree(d->hctrl);
    if (d->hctrl2) (void)hipHostFree(d->hctrl2);
    if (d->grp_hctrl) (void)hipHostFree(d->grp_hctrl);
    if (d->hpack) (void)hipHostFree(d->hpack);
    if (d->comm.hbuf) (void)hipHostFree(d->comm.hbuf);
    if (d->comm.nccl) ncclCommDestroy(d->comm.nccl);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    for (int i = 0; i < 2; i++) { if (d->evF[i]) (void)hipEventDestroy(d->evF[i]); if (d->evB[i]) (void)hipEventDestroy(d->evB[i]); }
    if (d->stream2) (void)hipStreamDestroy(d->stream2);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}
int qdev_sync(QpdoDev *d) { HIPCHK(hipSetDevice(d->device)); HIPCHK(hipStreamSynchronize(d->stream)); return 0; }

// The band solver's variable order (host side of the order: csrc/band_order.c; qpdo_dev.h has the contract).  The two int32 arrays are the
// only resident memory an order costs.
int qdev_set_band_order(QpdoDev *d, const int32_t *newold, int b_natural, int b_ordered) {
    HIPCHK(hipSetDevice(d->device));
    d->bo_seen_nat = b_natural; d->bo_seen_ord = b_ordered;
    if (!newold) return 0;
    const size_t n = (size_t)d->n;
    std::vector<int32_t> oldnew(n ? n : 1);
    for (size_t k = 0; k < n; k++) oldnew[(size_t)newold[k]] = (int32_t)k;
    int rc = dev_alloc(d, &d->bo_newold, n ? n : 1);
    if (!rc) rc = dev_alloc(d, &d->bo_oldnew, n ? n : 1);
    if (rc) { d->bo_newold = nullptr; return rc; }
    if (n) {
        HIPCHK(hipMemcpyAsync(d->bo_newold, newold, n * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(d->bo_oldnew, oldnew.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    d->bo_b = b_ordered;
    return 0;
}
int qdev_band_order_newold(QpdoDev *d, int32_t *newold) {
    HIPCHK(hipSetDevice(d->device));
    if (!d->bo_newold) return set_err(hipErrorInvalidValue, "this workspace has adopted no variable order", __LINE__);
    if (d->n) HIPCHK(hipMemcpyAsync(newold, d->bo_newold, (size_t)d->n * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// The bordered band (host side of the detection: csrc/band_border.c; qpdo_dev.h has the contract).  Nothing is allocated before the first
// factorization (band_alloc).
int qdev_set_band_border(QpdoDev *d, int max_border, int n_core, int border, int b_core, int over) {
    if (border < 0 || border > BC_MAX || (border > 0 && (n_core < 1 || n_core + border != d->n || b_core < 3 || b_core > BAND_MAX_B)))
        return set_err(hipErrorInvalidValue, "band border: not a border of this workspace", __LINE__);
    d->bb_max = max_border; d->bb_c = border; d->bb_ncore = border ? n_core : 0; d->bb_bcore = border ? b_core : 0; d->bb_over = over;
    return 0;
}
int qdev_configure(QpdoDev *d, int linsolve, double pcg_tol, int pcg_maxit) {
    const char *gr = getenv("QPDO_PCG_GRAPH");
    if (gr && !strcmp(gr, "0")) d->pcg_graph = 0;
    const char *mx = getenv("QPDO_DENSE_MAX_N");
    if (mx && *mx) d->dense_max_n = atoi(mx);
    const char *sc = getenv("QPDO_PCG_SCHUR");
    if (sc && *sc) d->schur_mode = atoi(sc) != 0;
    const char *ch = getenv("QPDO_DENSE_SOLVE");
    if (ch && !strcmp(ch, "steps")) d->dense_chain = 0;
    // (a measuring switch: QPDO_AMD_RHS_GROUP=1..8 overrides the group size of qpdo_amd_adjoint / qpdo_amd_tangent, dev/adjoint.inc qdev_rhs_group;
    // 1: the right-hand sides follow one another; tools/workspace_group_latency.py)
    { const char *rg = getenv("QPDO_AMD_RHS_GROUP"); const int g = (rg && *rg) ? atoi(rg) : SPMV_GROUP_MAX; d->rhs_group_cfg = g >= 1 && g <= SPMV_GROUP_MAX ? g : SPMV_GROUP_MAX; }
    { const char *md = getenv("QPDO_DENSE_MID"); if (md && *md) d->dense_mid = atoi(md) != 0; }      // 0: mid-size orders through the multi-launch factorization too
    { const char *la = getenv("QPDO_DENSE_LOOKAHEAD"); if (la && *la) d->dense_lookahead = atoi(la) != 0; }
    // Low-rank update of the kept factor: pays from n ~ 2500 up (tools/lowrank_crossover.py, m = 2n: n = 256: 39 ms with, 11 ms without;
    // 1024: 51 | 43; 2048: 102 | 91; 3072: 106 | 117; 1e4: 0.49 s | 0.63 s) -- below that a fresh MFMA factorization costs less than
    // the update's dozen small launches and its host read-back.  QPDO_DENSE_LOWRANK=0/1 overrides.
    const char *lr = getenv("QPDO_DENSE_LOWRANK");
    if (lr && *lr) d->wb_enable = atoi(lr) != 0;
    // Round 5: the factorization is one launch now and 1.6-2x faster (n = 4096: 1.5 ms), the update's chained solves and read-backs are what
    // they were -- the crossover moved up (same tool, solve ms with | without: 2560: 82 | 46, 4096: 96 | 79, 6000: 140 | 132, 8000: 234 | 230,
    // 10000: 297 | 356, 12000: 578 | 691; profiles/r05_lowrank_crossover.txt)
    else d->wb_enable = d->n >= 9000;
    if (!d->dense_chain) d->wb_enable = 0;                       // the refinement sweeps assume the one-launch solves
    // In-place up/downdate of the kept factor for passes that change few weights (dev/updown.inc): opt-in.  "1": at most UD_DEFAULT_CAP
    // changed rows per pass, "<k>" (k > 1): at most k (<= UD_CAP_MAX); more rows take the path they took without it.  Needs the chained
    // solves (p = L^-1 a is one of them); dense solver on one GPU only (checked below, once the solver is chosen).
    { const char *ud = getenv("QPDO_DENSE_UPDOWN"); const int k = (ud && *ud) ? atoi(ud) : 0; d->ud_cap = k <= 0 ? 0 : k == 1 ? UD_DEFAULT_CAP : k > UD_CAP_MAX ? UD_CAP_MAX : k; }
    if (!d->dense_chain) d->ud_cap = 0;
    // The direct solver is bounded by HBM, not by LDS (the assembly tiles its accumulator): DENSE_LIMIT_N = 40000 keeps the dense
    // matrix (12.8 GB at that order; look-ahead buffers beside it) and every 32-bit tile index in range.
    if (d->dense_max_n > DENSE_LIMIT_N) d->dense_max_n = DENSE_LIMIT_N;
    { const char *at = getenv("QPDO_DENSE_ASM_TILE"); if (at && atoi(at) >= 64 && atoi(at) < d->dense_asm_tile) d->dense_asm_tile = atoi(at); }
    { const char *fb = getenv("QPDO_PCG_DENSE_FALLBACK"); if (fb && *fb) d->pcg_dense_fallback = atoi(fb) != 0; }
#ifdef QPDO_TEST_HOOKS
    { const char *ie = getenv("QPDO_DENSE_CHAIN_INJECT"); d->chain_inject = (ie && *ie) ? atoi(ie) : -1; }
#endif
    { const char *te = getenv("QPDO_SCHUR_TAU"); d->schur_tau0 = (te && atof(te) > 0) ? atof(te) : 3e-6; }
    d->defl_debug = getenv("QPDO_DEFL_DEBUG") != nullptr;
    if (linsolve >= 0 && linsolve != 3) d->linsolve = linsolve;
    else d->linsolve = (d->n <= d->dense_max_n) ? 1 : 0;
    if (d->linsolve == 1 && d->n > DENSE_LIMIT_N) d->linsolve = 0;
    if (d->comm.active) { d->linsolve = 0; d->deflate = 0; }   // the dense factor and the Woodbury rows are not partitioned
    // A banded Newton matrix (chain-structured QPs: half-bandwidth of Q + A'A <= 127) gets the band direct solver -- what CHOLMOD's
    // natural-order factorization gives the reference on such problems -- by default from n = 2048 up (below, the dense MFMA factor of a
    // small matrix is as fast), or when asked for (QPDO_LINSOLVE=band; an explicit pcg / dense keeps those).  Half-bandwidths 128 .. 1023
    // (the tiled solver of dev/band_wide.inc) are taken only when asked for: its crossover against dense and PCG decides the default later.
    // QPDO_BAND_COUPLING=<R>, 1 <= R <= 64 (opt-in): up to R rows of A wider than the band are taken out of it and handled as a low-rank
    // term of the band solver (dev/band.inc, host_band.inc); the selection rule below is the same, on the half-bandwidth of the rest.
    { const char *bc = getenv("QPDO_BAND_COUPLING"); const int R = (bc && *bc) ? atoi(bc) : 0; d->band_coupling = R <= 0 ? 0 : R > BC_MAX ? BC_MAX : R; }
    // QPDO_BAND_BORDER=<C> (opt-in): a border of 1 .. C trailing variables over a core that this rule takes was adopted by the caller
    // (qdev_set_band_border; csrc/band_border.c has the detection and qpdo_api.c the rule on (n_core, b_core)): the band solver, on the core.
    if ((linsolve < 0 || linsolve == 3) && d->bb_c > 0) { d->band_b = d->bb_bcore; d->bc_r = 0; d->bc_over = 0; d->linsolve = 3; }
    else if (linsolve < 0 || linsolve == 3) {
        int rcb = band_detect(d); if (rcb) return rcb;
        const int wide_enough = d->n >= 4 * (d->band_b + 1);
        if (d->band_b > 0 && wide_enough && (linsolve == 3 || (d->band_b <= BAND_MAX_B && d->n >= 2048))) d->linsolve = 3;
        else if (linsolve == 3 && d->bb_over) { snprintf(g_err, sizeof(g_err), "QPDO_LINSOLVE=band: the Newton matrix is not banded: %d trailing border variables reach beyond the band (half-bandwidth > %d), QPDO_BAND_BORDER accepts %d", d->bb_over, BAND_MAX_B, d->bb_max); return -1; }
        else if (linsolve == 3 && d->bc_over) { snprintf(g_err, sizeof(g_err), "QPDO_LINSOLVE=band: %d rows of A are wider than the band (column span > %d), QPDO_BAND_COUPLING accepts %d", d->bc_over, BAND_MAX_B, d->band_coupling); return -1; }
        else if (linsolve == 3 && d->bo_seen_ord >= 0) {
            snprintf(g_err, sizeof(g_err), "QPDO_LINSOLVE=band: the Newton matrix is not banded (half-bandwidth > %d or order too small; half-bandwidth %d in the caller's "
                     "variable order, %d under the configured band order)", BAND_WIDE_MAX_B, d->bo_seen_nat, d->bo_seen_ord);
            return -1;
        }
        else if (linsolve == 3) { snprintf(g_err, sizeof(g_err), "QPDO_LINSOLVE=band: the Newton matrix is not banded (half-bandwidth > %d or order too small)", BAND_WIDE_MAX_B); return -1; }
    }
    if (pcg_tol > 0) d->pcg_tol = pcg_tol;
    if (pcg_maxit > 0) d->pcg_maxit = pcg_maxit;
    {   // hybrid PCG -> dense (see state.inc): only where the dense solver was selected automatically
        // default (round 4): on from n = 8192 -- C2 0.473 -> 0.442 s with the fixture's per-pass integers (profiles/r04_c2_hybrid_probe.txt);
        // QPDO_HYBRID=0 switches it off, =1 forces it from n = 4096, =<budget> also sets the iteration budget
        const char *hy = getenv("QPDO_HYBRID");
        const int want = (hy && *hy) ? atoi(hy) : -1;
        const int nmin = want > 0 ? 4096 : 8192;
        d->hybrid = (want != 0 && linsolve < 0 && d->linsolve == 1 && d->n >= nmin && !d->comm.active) ? 1 : 0;
        if (want > 1) d->hybrid_budget = want;
    }
    if (d->linsolve != 1 || d->comm.active) d->ud_cap = 0;
    d->st.linsolve = d->linsolve;
    d->cfg.linsolve = d->linsolve; d->cfg.dense_chain = d->dense_chain; d->cfg.dense_mid = d->dense_mid; d->cfg.dense_lookahead = d->dense_lookahead;
    d->cfg.wb_enable = d->wb_enable; d->cfg.ud_cap = d->ud_cap; d->cfg.deflate = d->deflate; d->cfg.pcg_maxit = d->pcg_maxit; d->cfg.band_b = d->band_b; d->cfg.bc_r = d->bc_r;
    return 0;
}
// absolute stopping rule of the linear solves follows the caller's eps_abs (QPDO_PCG_ABS: the factor, default 1e-5; 0 disables)
int qdev_set_eps_abs(QpdoDev *d, double eps_abs) {
    const char *e = getenv("QPDO_PCG_ABS");
    if (e && *e) d->pcg_abs_factor = atof(e);
    d->pcg_abs = d->pcg_abs_factor > 0.0 ? d->pcg_abs_factor * eps_abs : -1.0;
    return 0;
}
int qdev_get_stats(QpdoDev *d, QdevStats *out) { *out = d->st; out->coupled_rows = d->bc_r; return 0; }
int qdev_get_ac_sample(QpdoDev *d, double *seconds_sum, double *bytes_sum, long *samples, long *schur_passes) {
    *seconds_sum = d->ev_ac_ms * 1e-3; *bytes_sum = d->ev_ac_bytes; *samples = (long)d->ev_ac_n; *schur_passes = (long)d->schur_passes;
    return 0;
}
int qdev_get_spmv_sample(QpdoDev *d, double *avg_seconds, long *samples) {
    *samples = (long)d->ev_spmv_n;
    *avg_seconds = d->ev_spmv_n ? d->ev_spmv_ms * 1e-3 / (double)d->ev_spmv_n : 0.0;
    return 0;
}
int qdev_reset_stats(QpdoDev *d) { int ls = d->st.linsolve; d->st = QdevStats{}; d->st.linsolve = ls; d->ev_spmv_ms = 0; d->ev_spmv_n = 0; d->ev_ac_ms = 0; d->ev_ac_bytes = 0; d->ev_ac_n = 0; d->schur_passes = 0; return 0; }

// ---- scaling (scaling.c:24-91) ------------------------------------------------------------------
int qdev_scale_data(QpdoDev *d, int iters, int use_Qx, double *D_host, double *E_host, double *c_out) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, m = d->m;
    LAUNCH(k_fill, vgrid(n), n, 1.0, d->D);
    LAUNCH(k_fill, vgrid(m), m, 1.0, d->E);
    const int gAt = spmv_grid(d->At, false), gAr = spmv_grid(d->Ar, false);
    for (int it = 0; it < iters; it++) {
        // column norms of A = row norms of CSR(A'); row norms of A = row norms of CSR(A)
        DISPATCH_TPR(d->At, k_row_absmax, gAt, n, d->At.rp, d->At.val, d->tmp_n);
        if (d->comm.active) {   // max over the row slices; row norms gathered through a sum with zero padding
            int rcx = comm_allreduce(d, d->tmp_n, (size_t)n, 1); if (rcx) return rcx;
            HIPCHK(hipMemsetAsync(d->tmp_m, 0, (size_t)m * 8, d->stream));
        }
        DISPATCH_TPR(d->Ar, k_row_absmax, gAr, d->mloc, d->Ar.rp, d->Ar.val, d->tmp_m + d->m0);
        if (d->comm.active) { int rcx = comm_allreduce(d, d->tmp_m, (size_t)m, 0); if (rcx) return rcx; }
        LAUNCH(k_ruiz_factor, vgrid(n), n, d->tmp_n, d->D);
        LAUNCH(k_ruiz_factor, vgrid(m), m, d->tmp_m, d->E);
        // A <- E A D: (a * E_i) * D_j on both stored copies
        DISPATCH_TPR(d->Ar, k_scale_rows_cols, gAr, d->mloc, d->Ar.rp, d->Ar.ci, d->Ar.val, (const double *)(d->tmp_m + d->m0), (const double *)nullptr,
                     (const double *)nullptr, (const double *)d->tmp_n);
        DISPATCH_TPR(d->At, k_scale_rows_cols, gAt, n, d->At.rp, d->At.ci, d->At.val, (const double *)nullptr, (const double *)(d->tmp_m + d->m0),
                     (const double *)d->tmp_n, (const double *)nullptr);
    }
    const int gQ = spmv_grid(d->Qf, false);
    DISPATCH_TPR(d->Qf, k_scale_sym, gQ, n, d->Qf.rp, d->Qf.ci, d->Qf.val, (const double *)d->D);
    if (d->comm.active && d->Qs.nnz) hipLaunchKernelGGL(k_scale_sym_rows, dim3(vgrid(d->nloc)), dim3(BLK), 0, d->stream, d->nloc, d->n0, d->Qs.rp, d->Qs.ci, d->Qs.val, (const double *)d->D);
    d->qdiag_valid = 0; d->dense_valid = 0; d->dense_factored = 0;
    d->Ar.sm_dirty = d->At.sm_dirty = d->Qf.sm_dirty = d->Qs.sm_dirty = 1;
    LAUNCH(k_mul, vgrid(n), n, d->D, d->q, d->q);                    // q <- D q
    // cost scaling: c = 1 / max(1, ||Qx + q||inf)
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_axpy, vgrid(n), n, (const double *)d->q, use_Qx ? (const double *)d->Qx : (const double *)nullptr, 1.0, d->ctrl, N_A);
    int rc = read_ctrl(d); if (rc) return rc;
    const double nq = nrm_of(d->hctrl, N_A);
    const double c = 1 / (1.0 > nq ? 1.0 : nq);
    // q <- c q (vec_self_mult_scalar), Q <- c Q
    LAUNCH(k_scal, vgrid(n), n, c, d->q);
    if (d->Qf.nnz) hipLaunchKernelGGL(k_scale_vals, dim3(2048), dim3(BLK), 0, d->stream, d->Qf.nnz, d->Qf.val, c);
    if (d->comm.active && d->Qs.nnz) hipLaunchKernelGGL(k_scale_vals, dim3(2048), dim3(BLK), 0, d->stream, d->Qs.nnz, d->Qs.val, c);
    d->Ar.sm_dirty = d->At.sm_dirty = d->Qf.sm_dirty = d->Qs.sm_dirty = 1;      // values changed: the slab-major images are stale
    rc = h16_refresh_scale(d); if (rc) return rc;                               // ... and so is the scale of the half-precision ones
    HIPCHK(hipMemcpyAsync(D_host, d->D, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (m) HIPCHK(hipMemcpyAsync(E_host, d->E, (size_t)m * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *c_out = c;
    return 0;
}
int qdev_set_scaling(QpdoDev *d, int scaled, const double *D, const double *Dinv, const double *E, const double *Einv, double c, double cinv) {
    HIPCHK(hipSetDevice(d->device));
    d->scaled = scaled; d->sc_c = c; d->sc_cinv = cinv;
    if (scaled) {
        HIPCHK(hipMemcpyAsync(d->D, D, (size_t)d->n * 8, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(d->Dinv, Dinv, (size_t)d->n * 8, hipMemcpyHostToDevice, d->stream));
        if (d->m) {
            HIPCHK(hipMemcpyAsync(d->E, E, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream));
            HIPCHK(hipMemcpyAsync(d->Einv, Einv, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream));
        }
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    return 0;
}
int qdev_upload_bounds(QpdoDev *d, const double *l, const double *u) {
    HIPCHK(hipSetDevice(d->device));
    if (d->m) {
        if (l) HIPCHK(hipMemcpyAsync(d->l, l, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream));
        if (u) HIPCHK(hipMemcpyAsync(d->u, u, (size_t)d->m * 8, hipMemcpyHostToDevice, d->stream));
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
int qdev_upload_q(QpdoDev *d, const double *q) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemcpyAsync(d->q, q, (size_t)d->n * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// qpdo_update_q for a scaled problem without pulling Qx and x to the host (qpdo.c:549-586): one upload of the new q, two
// elementwise kernels and the scalars c, norm_q back.  c_new / cinv_new / norm_q follow the reference's arithmetic.
int qdev_update_q_scaled(QpdoDev *d, const double *q_unscaled, int proximal, double sigma_old, double sigma_new, double c_old,
                         double *c_new, double *cinv_new, double *norm_q) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, g = vgrid(n);
    HIPCHK(hipMemcpyAsync(d->tmp_n, q_unscaled, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_update_q1, g, n, (const double *)d->tmp_n, (const double *)d->D, (const double *)d->x, proximal, sigma_old, d->sc_cinv, d->q, d->Qx, d->ctrl);
    int rc = read_ctrl(d); if (rc) return rc;
    const double mx = nrm_of(d->hctrl, N_A);
    const double c = 1.0 / (mx > 1.0 ? mx : 1.0);
    const double f = c / c_old;
    LAUNCH(k_update_q2, g, n, c, f, proximal, sigma_new, (const double *)d->x, (const double *)d->Dinv, d->q, d->Qx, d->ctrl);
    rc = qdev_scale_Q_values(d, f); if (rc) return rc;
    rc = read_ctrl(d); if (rc) return rc;
    *c_new = c; *cinv_new = 1.0 / c; *norm_q = nrm_of(d->hctrl, N_B);
    d->sc_c = c; d->sc_cinv = 1.0 / c;
    return 0;
}
int qdev_download_q(QpdoDev *d, double *q) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemcpyAsync(q, d->q, (size_t)d->n * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
int qdev_scale_Q_values(QpdoDev *d, double factor) {
    HIPCHK(hipSetDevice(d->device));
    d->qdiag_valid = 0; d->dense_valid = 0; d->dense_factored = 0;
    d->Qf.sm_dirty = d->Qs.sm_dirty = 1;
    if (d->comm.active && d->Qs.nnz) hipLaunchKernelGGL(k_scale_vals, dim3(2048), dim3(BLK), 0, d->stream, d->Qs.nnz, d->Qs.val, factor);
    if (d->Qf.nnz) hipLaunchKernelGGL(k_scale_vals, dim3(2048), dim3(BLK), 0, d->stream, d->Qf.nnz, d->Qf.val, factor);
    HIPCHK(hipGetLastError());
    return 0;
}
static double *vec_by_id(QpdoDev *d, int which, size_t *len) {
    switch (which) {
        case 0: *len = d->n; return d->x;
        case 1: *len = d->n; return d->Qx;
        case 2: *len = d->m; return d->y;
        case 3: *len = d->m; return d->mu;
        case 4: *len = d->m; return d->d;
        case 5: *len = d->n; return d->dx;
        case 6: *len = d->m; return d->dy;
        case 7: *len = d->m; return d->Ax;
        case 8: *len = d->n; return d->Aty;
        case 9: *len = d->m; return d->l;
        case 10: *len = d->m; return d->u;
        case 11: *len = d->m; return d->ybar;
        case 12: *len = d->n; return d->xbar;
        case 13: *len = d->m; return d->w;
    }
    *len = 0; return nullptr;
}
int qdev_download_vec(QpdoDev *d, int which, double *dst) {
    HIPCHK(hipSetDevice(d->device));
    size_t len; double *p = vec_by_id(d, which, &len);
    if (!p) return -1;
    if (len) HIPCHK(hipMemcpyAsync(dst, p, len * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
int qdev_upload_vec(QpdoDev *d, int which, const double *src) {
    HIPCHK(hipSetDevice(d->device));
    size_t len; double *p = vec_by_id(d, which, &len);
    if (!p) return -1;
    if (len) HIPCHK(hipMemcpyAsync(p, src, len * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

// ---- warm start (qpdo.c:217-299, iteration.c:98-122) ---------------------------------------------
int qdev_objective(QpdoDev *d, int proximal, double sigma, double c_const, double *objective) {
    HIPCHK(hipSetDevice(d->device));
    const int g = vgrid(d->n);
    LAUNCH(k_objective, g, d->n, proximal, sigma, d->x, d->Qx, d->q, d->part + P_OBJ * PGRID);
    LAUNCH(k_reduce_to_ctrl, 1, d->part + P_OBJ * PGRID, g, d->ctrl, V_OBJ);
    int rc = read_ctrl(d); if (rc) return rc;
    double obj = d->hctrl->val[V_OBJ];
    if (d->scaled) obj *= d->sc_cinv;
    obj += c_const;
    *objective = obj;
    return 0;
}
int qdev_warm_start(QpdoDev *d, const double *x_ws, const double *y_ws, int proximal, double sigma, double mu_min,
                    double c_const, double *objective) {
    HIPCHK(hipSetDevice(d->device));
    const int n = d->n, m = d->m;
    (void)mu_min;
    *objective = 0.0;
    if (!x_ws && !(y_ws && m)) {
        // cold start: every vector of both branches zeroed by one launch instead of six memsets
        LAUNCH(k_cold_start_zero, vgrid(n > m ? n : m), n, m, d->x, d->xbar, d->Qx, d->Aty, d->Ax, d->y, d->ybar);
    } else {
    if (x_ws) {
        HIPCHK(hipMemcpyAsync(d->tmp_n, x_ws, (size_t)n * 8, hipMemcpyHostToDevice, d->stream));
        LAUNCH(k_ws_x, vgrid(n), n, d->scaled, d->tmp_n, d->Dinv, d->x, d->xbar);
        launch_spmv(d, d->Qf, d->x, EpiQpure{d->x, sigma, proximal, d->Qx}, false);
        { int rc2 = spmv_A(d, d->x, EpiStore{d->Ax}, false); if (rc2) return rc2; }
        int rc = qdev_objective(d, proximal, sigma, c_const, objective); if (rc) return rc;
    } else {
        HIPCHK(hipMemsetAsync(d->x, 0, (size_t)n * 8, d->stream));
        HIPCHK(hipMemsetAsync(d->xbar, 0, (size_t)n * 8, d->stream));
        HIPCHK(hipMemsetAsync(d->Qx, 0, (size_t)n * 8, d->stream));
        if (m) HIPCHK(hipMemsetAsync(d->Ax, 0, (size_t)m * 8, d->stream));
    }
    if (y_ws && m) {
        HIPCHK(hipMemcpyAsync(d->tmp_m, y_ws, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
        LAUNCH(k_ws_y, vgrid(m), m, d->scaled, d->sc_c, d->tmp_m, d->Einv, d->y, d->ybar);
        { int rc2 = spmv_At(d, d->y, EpiStore{d->Aty}, false); if (rc2) return rc2; }
    } else {
        if (m) { HIPCHK(hipMemsetAsync(d->y, 0, (size_t)m * 8, d->stream)); HIPCHK(hipMemsetAsync(d->ybar, 0, (size_t)m * 8, d->stream)); }
        HIPCHK(hipMemsetAsync(d->Aty, 0, (size_t)n * 8, d->stream));
    }
    }
    const int g = vgrid(n);
    LAUNCH(k_dots_f, g, n, d->x, d->Qx, d->q, d->part + P_F1 * PGRID, d->part + P_F2 * PGRID);
    LAUNCH(k_init_mu, vgrid(m), m, d->part + P_F1 * PGRID, d->part + P_F2 * PGRID, g, d->Ax, d->l, d->u, d->mu, d->isq);
    if (x_ws || y_ws) HIPCHK(hipStreamSynchronize(d->stream));   // x_ws / y_ws host buffers may be released by the caller
    else HIPCHK(hipGetLastError());
    return 0;
}
int qdev_begin_solve(QpdoDev *d) {
    HIPCHK(hipSetDevice(d->device));
    d->last_jacobi_iters = 0; d->schur_off = 0; d->schur_strikes = 0; d->ctrl_clean = 0; d->step_pending = 0; d->axpy_pending = 0;
    if (d->hybrid) { d->linsolve = 0; d->hybrid_active = 1; }
    if (d->direct_hook_used) {       // a factor kept by the test entry qdev_direct_solve is not this solve's: start as an untouched workspace
        d->dense_valid = 0; d->dense_factored = 0; d->wb_k = 0; d->mid_fwd_valid = 0; d->dense_fact_sigma = 0.0;
        d->dense_last_branch = -1; d->dense_last_sigma = -1.0; d->direct_hook_used = 0; d->bc_factored = 0;
    }
    // the lost-producer latch of the polling kernels is cleared by the redo (step_redo_if_lost) -- and here, so that a solve that was
    // left between the latch and its redo (a HIP error on the way) cannot make k_axpy5 skip every iterate update of the next solve
    LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_CHAIN_ERR, 0);
    if (d->ud_cap) LAUNCH(k_ctrl_set_int, 1, d->ctrl, C_UD_REJECT, 0);      // (likewise the up/downdate's latch)
    if (d->m) HIPCHK(hipMemsetAsync(d->active_old, 0, (size_t)d->m * sizeof(int), d->stream));
    return 0;
}
