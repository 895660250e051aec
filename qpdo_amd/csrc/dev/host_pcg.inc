// host_pcg.inc -- part of qpdo_dev.hip (one translation unit; included in order): host side (extern C): compact index space, deflation, Schur-complement mode, PCG driver
// ---- linear solve -----------------------------------------------------------------------------------
// Build the compact index space of this Newton pass: k weighted rows, A_c (k x n) copied out of CSR(A),
// A_c' (n x k) compacted out of CSR(A') with renumbered columns, d_c; both with their slab tables and slab-major images where they take the
// slab kernel.  Once per Newton pass: one read of the weighted rows of A, two of CSR(A') (count, then compaction).
// Schur-complement mode whenever its inner system is well conditioned (k/n <= 0.8) and worth the set-up (k >= 256); kglob: the number of
// weighted rows over all ranks
static bool schur_allowed(const QpdoDev *d, long long kglob) {
    return !d->schur_off && d->schur_mode != 0 && kglob >= 256 && (double)kglob <= 0.8 * (double)d->n && kglob <= (long long)d->m;
}
static int build_compact(QpdoDev *d) {
    const int n = d->n, m = d->mloc;                 // local rows; dl = their weights
    const double *dl = d->d + d->m0;
    d->kact = 0; d->sdiag_valid = 0;
    if (m == 0) return 0;
    const int fwords = (m + 63) / 64;     // (the words' counts pass through row_cnt, which the row counts below overwrite)
    LAUNCH(k_flag_words, (fwords + 3) / 4, m, dl, d->flag_bits, d->row_cnt);
    dev_scan(d, d->row_cnt, fwords, d->flag_wprefix, d->kcount, d->scan_tsum);
    LAUNCH(k_flag_apply, (fwords + 3) / 4, m, (const u64 *)d->flag_bits, (const int *)d->flag_wprefix, d->cidx, d->rowlist);
    int k = 0;
    HIPCHK(hipMemcpyAsync(&k, d->kcount, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (k <= 0) return 0;
    // A_c: rows
    LAUNCH(k_gather_rowinfo, vgrid(k), k, (const int *)d->rowlist, d->Ar.rp, dl, d->row_cnt, d->dc);
    dev_scan(d, d->row_cnt, k, d->Arc.rp, d->Arc.rp + k, d->scan_tsum);
    DevCsr &R = d->Arc;
    R.nrows = k; R.ncols = n; R.tpr = d->Ar.tpr; R.use_slab = d->Ar.use_slab && k >= 4096; R.slab_ovl = d->Ar.slab_ovl; R.slab_nt = d->Ar.slab_nt;
    int RW16 = 0;
    if (R.use_slab) {
        R.rows_per_wg = (k + 255) / 256; R.slab_grid = (k + R.rows_per_wg - 1) / R.rows_per_wg;
        // own slab width: k/256 rows per workgroup need less accumulator space than m/256, the x slice can be wider
        // (C4 late passes: 5 slabs of 20 k columns instead of 6 of 16.7 k)
        const long long lds_doubles = slab_cap_w((160 * 1024 - 1024) / 8 - R.rows_per_wg);
        int nslabs = (int)((n + lds_doubles - 1) / lds_doubles); if (nslabs < 1) nslabs = 1;
        int W = ((n + nslabs - 1) / nslabs + 63) & ~63;
        if (W > lds_doubles) { nslabs++; W = ((n + nslabs - 1) / nslabs + 63) & ~63; }
        if (nslabs > d->Ar.nslabs || (R.ci16 && W >= 65536)) { nslabs = d->Ar.nslabs; W = d->Ar.W; }     // the sp table holds Ar.nslabs + 1 per row
        R.nslabs = nslabs; R.W = W;
        if (R.ci16) RW16 = W;
    }
    const bool one_read = d->compact_one_read && R.use_slab && R.nslabs <= PASS_SLABS_MAX;
    if (one_read) {
        // sp and seg of the copy first, from the source rows; then one read of those rows writes the CSR copy, the slab image and -- where
        // this pass can take the Schur mode on one GPU and k_schur_diag would run 64 lanes per row -- that mode's inner diagonal
        const bool diag = d->Ar.tpr == 64 && !d->comm.active && schur_allowed(d, k);
        LAUNCH(k_build_slab_ptr_rows, vgrid(k), k, (const int *)d->rowlist, d->Ar.rp, d->Ar.ci, (const int *)R.rp, R.nslabs, R.W, R.sp);
        hipLaunchKernelGGL(k_slab_seg, dim3(R.slab_grid), dim3(1024), 0, d->stream, R.nrows, R.nslabs, R.rows_per_wg, (const int *)R.sp, R.seg, R.seg_pairs);
#define COPY_ROWS_SLAB(DIAG) LAUNCH((k_copy_rows_slab<DIAG>), PASS_GRID, k, (const int *)d->rowlist, d->Ar.rp, d->Ar.ci, (const unsigned short *)d->Ar.ci16, \
            d->Ar.val, (const int *)R.rp, R.ci, R.ci16, R.val, RW16, R.nslabs, R.W, (const int *)R.sp, (const int2 *)R.seg, R.vsm, R.i16sm, R.cism, \
            R.vsm32, h16_dst(d, R), d->h16_scale, (const double *)d->qdiag, d->sigma_f, (const double *)d->dc, d->s_diag, R.p16sm)
        if (diag) { COPY_ROWS_SLAB(true); d->sdiag_valid = 1; d->sdiag_sigma = d->sigma_f; } else COPY_ROWS_SLAB(false);
#undef COPY_ROWS_SLAB
    } else {
        LAUNCH(k_copy_rows, 2048, k, (const int *)d->rowlist, d->Ar.rp, d->Ar.ci, (const unsigned short *)d->Ar.ci16, d->Ar.val,
               (const int *)d->Arc.rp, d->Arc.ci, d->Arc.ci16, d->Arc.val, RW16);
        if (R.use_slab) LAUNCH(k_build_slab_ptr, vgrid(k), k, R.rp, R.ci, R.nslabs, R.W, R.sp, (int *)nullptr);
    }
    // A_c': columns, renumbered
    DevCsr &T = d->Atc;
    const DevCsr &M = d->At;
    T.nrows = n; T.ncols = k; T.tpr = M.tpr; T.use_slab = M.use_slab && k >= 1024; T.slab_ovl = M.slab_ovl; T.slab_nt = M.slab_nt;
    int W16 = 0;
    if (T.use_slab) {
        T.rows_per_wg = M.rows_per_wg; T.slab_grid = M.slab_grid;
        int nslabs = (k + d->lds_doubles_At - 1) / d->lds_doubles_At; if (nslabs < 1) nslabs = 1;
        int W = ((k + nslabs - 1) / nslabs + 63) & ~63;
        if (W > d->lds_doubles_At) { nslabs++; W = ((k + nslabs - 1) / nslabs + 63) & ~63; }
        if (nslabs > M.nslabs) { nslabs = M.nslabs; W = M.W; }           // never more slabs than the sp table holds
        T.nslabs = nslabs; T.W = W;
        if (T.ci16 && W < 65536) W16 = W;
    }
    const int g = rowloop_grid(M);
    const int words = (m + 63) / 64;
    const size_t lds_tab = (size_t)words * (sizeof(u64) + sizeof(int));
    // one read of CSR(A') for the CSR and the image: with the LDS tables, and where the slab-local 16-bit index is the image's own
    const bool t_one_read = d->compact_t_one_read && lds_tab <= 60 * 1024 && (!T.use_slab || (T.nslabs <= PASS_SLABS_MAX && (!T.ci16 || W16 > 0)));
    if (t_one_read) {
        // counts per (row, slab) from the counting pass: the slab pointers follow from the scanned row pointers without a search; then
        // seg, then the compaction writes every kept pair to the CSR and to its slab-major place
        int *spT = T.use_slab ? T.sp : (int *)nullptr;
        hipLaunchKernelGGL(k_count_flagged_slabs, dim3(2048), dim3(BLK), (size_t)words * 8, d->stream, n, M.rp, M.ci, (const u64 *)d->flag_bits, words,
                           (const int *)d->rowlist, k, T.nslabs, T.W, d->row_cnt, spT);
        dev_scan(d, d->row_cnt, n, T.rp, T.rp + n, d->scan_tsum);
        if (spT) {
            LAUNCH(k_sp_add_rp, vgrid(n), n, T.nslabs, (const int *)T.rp, T.sp);
            hipLaunchKernelGGL(k_slab_seg, dim3(T.slab_grid), dim3(1024), 0, d->stream, T.nrows, T.nslabs, T.rows_per_wg, (const int *)T.sp, T.seg, T.seg_pairs);
        }
        hipLaunchKernelGGL(k_compact_rows_bits_slab, dim3(PASS_GRID), dim3(BLK), lds_tab, d->stream, n, M.rp, M.ci, M.val, (const u64 *)d->flag_bits,
                           (const int *)d->flag_wprefix, words, (const int *)T.rp, T.ci, T.val, W16, M.ci16 ? d->Atc.ci16 : (unsigned short *)nullptr,
                           T.nslabs, T.W, (const int *)spT, (const int2 *)T.seg, T.vsm, T.i16sm, T.cism, T.vsm32, h16_dst(d, T), d->h16_scale, T.p16sm);
    } else if (lds_tab <= 60 * 1024) {          // flags and renumbering as LDS tables: the kernels stream the matrix only
        DISPATCH_TPR_LDS(M, k_count_flagged_bits, g, (size_t)words * 8, n, M.rp, M.ci, (const u64 *)d->flag_bits, words, d->row_cnt);
        dev_scan(d, d->row_cnt, n, T.rp, T.rp + n, d->scan_tsum);
        hipLaunchKernelGGL(k_compact_rows_bits, dim3(2048), dim3(BLK), lds_tab, d->stream, n, M.rp, M.ci, M.val, (const u64 *)d->flag_bits,
                           (const int *)d->flag_wprefix, words, (const int *)T.rp, T.ci, T.val, W16, M.ci16 ? d->Atc.ci16 : (unsigned short *)nullptr);
    } else {
        DISPATCH_TPR(M, k_count_flagged, g, n, M.rp, M.ci, dl, d->row_cnt);
        dev_scan(d, d->row_cnt, n, T.rp, T.rp + n, d->scan_tsum);
        LAUNCH(k_compact_rows, 2048, n, M.rp, M.ci, M.val, dl, (const int *)T.rp, T.ci, T.val, (const int *)d->cidx, W16,
               M.ci16 ? d->Atc.ci16 : (unsigned short *)nullptr);
    }
    if (T.use_slab && !t_one_read) LAUNCH(k_build_slab_ptr, vgrid(n), n, T.rp, T.ci, T.nslabs, T.W, T.sp, (int *)nullptr);
    int nn[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&nn[0], d->Arc.rp + k, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(&nn[1], T.rp + n, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    R.nnz = nn[0]; T.nnz = nn[1];
    R.sm_dirty = one_read ? 0 : 1; T.sm_dirty = (t_one_read && T.use_slab) ? 0 : 1;      // stale images are rebuilt by the first product (slab_major_build)
    d->kact = k;
    return 0;
}
// Si = S^-1 of the symmetric positive definite leading r x r block of S (row stride N) by Cholesky on the host; L, Li: zeroed
// workspace of the same shape.  false: S is not positive definite.
static bool spd_inverse(int r, int N, const double *S, double *L, double *Li, double *Si) {
    for (int i = 0; i < r; i++)                     // Cholesky S = L L'
        for (int j = 0; j <= i; j++) {
            double t = S[i * N + j];
            for (int q = 0; q < j; q++) t -= L[i * N + q] * L[j * N + q];
            if (i == j) { if (!(t > 0.0)) return false; L[i * N + i] = sqrt(t); }
            else L[i * N + j] = t / L[j * N + j];
        }
    for (int c = 0; c < r; c++)                     // Li = L^-1 (lower)
        for (int i = 0; i < r; i++) {
            if (i < c) { Li[i * N + c] = 0.0; continue; }
            double t = (i == c) ? 1.0 : 0.0;
            for (int q = c; q < i; q++) t -= L[i * N + q] * Li[q * N + c];
            Li[i * N + c] = t / L[i * N + i];
        }
    for (int i = 0; i < r; i++)                     // S^-1 = Li' Li
        for (int j = 0; j <= i; j++) {
            double t = 0.0;
            for (int q = i; q < r; q++) t += Li[q * N + i] * Li[q * N + j];
            Si[i * N + j] = t; Si[j * N + i] = t;
        }
    return true;
}
// choose the heavy rows of this pass (in the compact space) and build P, A_h', S^-1.  Sets d->defl_r.
static int defl_build(QpdoDev *d) {
    const int n = d->n, k = d->kact;
    d->defl_r = 0;
    if (!d->deflate || k <= 4 * DEFL_MAX) return 0;   // few weighted rows: plain Jacobi-PCG ends within ~n iterations anyway
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    LAUNCH(k_absmax_mul, vgrid(k), k, (const double *)d->dc, (const double *)nullptr, d->ctrl, N_A);
    HIPCHK(hipMemsetAsync(d->defl_hist, 0, 32 * sizeof(int), d->stream));
    LAUNCH(k_defl_hist, vgrid(k), k, (const double *)d->dc, (const Ctrl *)d->ctrl, d->defl_hist);
    int hist[32];
    HIPCHK(hipMemcpyAsync(hist, d->defl_hist, sizeof(hist), hipMemcpyDeviceToHost, d->stream));
    int rc = read_ctrl(d); if (rc) return rc;
    const double dmax = nrm_of(d->hctrl, N_A);
    if (!(dmax > 0.0)) return 0;
    const bool dbg = d->defl_debug != 0;
    if (dbg) { fprintf(stderr, "[defl] k=%d dmax=%.3e sigma_f=%.3e hist:", k, dmax, d->sigma_f); for (int b = 0; b < 32; b++) fprintf(stderr, " %d", hist[b]); fprintf(stderr, "\n"); }
    // largest bucket index kb whose cumulative count still fits; rows in buckets 0..kb are > dmax / 2^(kb+1)
    int cum = 0, kb = -1;
    for (int b = 0; b < 32; b++) { if (cum + hist[b] > DEFL_MAX) break; cum += hist[b]; kb = b; }
    if (kb < 2 || cum == 0) return 0;              // no group of <= 64 rows stands out by a factor of 8: nothing to deflate
    const double thr = dmax * ldexp(1.0, -(kb + 1));
    hipLaunchKernelGGL(k_defl_select, dim3(1), dim3(1024), 0, d->stream, k, (const double *)d->dc, thr, d->defl_flag, d->tmp_m, d->defl_list, d->defl_count);
    int r = 0;
    HIPCHK(hipMemcpyAsync(&r, d->defl_count, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (r <= 0 || r > DEFL_MAX) return 0;
    const DevCsr &T = d->Atc;
    // P: Jacobi diagonal of the remainder (floored), A_h': the heavy columns of A_c'
    const int gAt = rowloop_grid(d->At);
    DISPATCH_TPR(d->At, k_jacobi_diag2, gAt, n, T.rp, T.ci, T.val, (const double *)d->tmp_m, (const double *)d->dc, (const double *)d->qdiag, d->sigma_f, d->pc_diag);
    DISPATCH_TPR(d->At, k_count_flagged, gAt, n, T.rp, T.ci, (const double *)d->defl_flag, d->row_cnt);
    dev_scan(d, d->row_cnt, n, d->Ath.rp, d->Ath.rp + n, d->scan_tsum);
    LAUNCH(k_compact_rows, 2048, n, T.rp, T.ci, T.val, (const double *)d->defl_flag, (const int *)d->Ath.rp, d->Ath.ci, d->Ath.val,
           (const int *)nullptr, 0, (unsigned short *)nullptr);
    d->Ath.nrows = n; d->Ath.ncols = k; d->Ath.tpr = 4; d->Ath.use_slab = 0; d->Ath.nnz = (long long)r * d->max_row_nnz_A;
    HIPCHK(hipMemsetAsync(d->defl_t, 0, (size_t)k * 8, d->stream));
    // S and its inverse (host, r <= 64)
    hipLaunchKernelGGL(k_defl_S, dim3(r, r), dim3(64), 0, d->stream, r, (const int *)d->defl_list, d->Arc.rp, d->Arc.ci, d->Arc.val,
                       (const double *)d->pc_diag, (const double *)d->dc, d->defl_S);
    static thread_local std::vector<double> Sv, Lv, Liv, Siv;
    Sv.assign((size_t)DEFL_MAX * DEFL_MAX, 0.0); Lv.assign((size_t)DEFL_MAX * DEFL_MAX, 0.0); Liv.assign((size_t)DEFL_MAX * DEFL_MAX, 0.0); Siv.assign((size_t)DEFL_MAX * DEFL_MAX, 0.0);
    double *S = Sv.data(), *L = Lv.data(), *Li = Liv.data(), *Si = Siv.data();
    HIPCHK(hipMemcpyAsync(S, d->defl_S, (size_t)DEFL_MAX * DEFL_MAX * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (!spd_inverse(r, DEFL_MAX, S, L, Li, Si)) return 0;
    HIPCHK(hipMemcpyAsync(d->defl_Sinv, Si, (size_t)DEFL_MAX * DEFL_MAX * 8, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    d->defl_r = r;
    d->defl_passes++;
    return 0;
}
// z <- M^-1 r given u = P^-1 r in z; leaves the r.z partials in p_rz.  Returns their count.
static int defl_apply(QpdoDev *d, const int *done, double *p_rz) {
    const int r = d->defl_r;
    hipLaunchKernelGGL(k_defl_v, dim3(r), dim3(64), 0, d->stream, done, r, (const int *)d->defl_list, d->Arc.rp, d->Arc.ci, d->Arc.val,
                       (const double *)d->pc_z, d->defl_v);
    hipLaunchKernelGGL(k_defl_w, dim3(1), dim3(DEFL_MAX), 0, d->stream, done, r, (const double *)d->defl_Sinv, (const double *)d->defl_v,
                       (const int *)d->defl_list, d->defl_t);
    EpiDeflZ e{d->pc_diag, d->pc_r, d->pc_z, p_rz};
    launch_spmv(d, d->Ath, d->defl_t, e, true, done);
    d->st.spmv_calls--; d->st.spmv_bytes -= (int64_t)d->Ath.alg_bytes();     // not one of the big products
    return spmv_pgrid(d->Ath);
}
// ---- Schur-complement mode of the PCG ---------------------------------------------------------------------
// Late in a solve the weights d = 1/mu of the active rows spread over 2^8..2^16 and Jacobi-PCG on
// K = Q~ + A_c' D A_c needs 1000+ iterations per pass (kappa ~ spread x the Marchenko-Pastur ratio of A_c).
// Preconditioner M = Dq + A_c' D A_c with Dq = diag(Q~): it treats the whole penalty term exactly, so M^-1 K =
// I + M^-1 offdiag(Q) and the outer CG converges in ~10 iterations when Q is diagonally dominant in the spectral
// sense.  M^-1 r = u - Dq^-1 A_c' s,  u = Dq^-1 r,  S' s = A_c u,  S' = D^-1 + A_c Dq^-1 A_c'  (k x k, never formed):
// the inner system is solved by Jacobi-PCG; its conditioning is that of A_c Dq^-1 A_c' (Marchenko-Pastur,
// ((1+sqrt(k/n))/(1-sqrt(k/n)))^2 ~ 160 at k/n = 0.73) and does NOT depend on the spread of d; its products are two
// SpMV with the compact matrices and no Q product.  Measured on the C2 system of the last pass (numpy prototype):
// 1862 Jacobi iterations (5586 SpMV) -> 11 outer x 78 inner (1777 SpMV, none of them Q).  The inner solve must be
// tight (1e-6): at 1e-3 the outer iteration degrades to hundreds of steps even with a flexible beta.
// Used when 256 <= k <= 0.8 n (beyond that ratio the inner conditioning explodes); falls back to the deflated
// Jacobi-PCG below when the outer iteration does not converge within SCHUR_OUTER_MAXIT steps (twice: off for the solve).
static int read_ctrl2(QpdoDev *d) {
    { int rc = read_ctrl_block(d, d->ctrl2, d->hctrl2, d->hseq2); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    return 0;
}
static const int SCHUR_INNER_MAXIT = 4000, SCHUR_OUTER_MAXIT = 40;
static const int PCG_NOT_CONVERGED = -7;        // (distinct from a HIP failure: the caller may redo the pass with the dense solver)
static const int PCG_NAN = -8;                  // a NaN residual: a numerical failure too, not a HIP one
// Row-partitioned solve (dist): rank r owns the k_loc = d->kact weighted rows among ITS rows of A; every k-vector of the inner
// solver (x, r, u, w, p, s, the diagonal, the weights) is PARTITIONED -- length k_loc, never exchanged.  The only exchange of
// an application of S' is the sum over the ranks of A_c,loc' u_loc (n doubles); the three local scalar sums of the
// single-reduction CG ride at the end of that payload (see pcg_kernels.inc): ONE collective per inner iteration.
//
// One application  w = S' u = u ./ d + A_c ((A_c' u) ./ Dq):  t in d->tmp_n, the partial sums of (A_c' u).t in Pf (fcnt of them).
// par: parity of the local partial sums (in P3) that accompany this application.
// both compact matrices of this pass take the 16-bit slab kernel and have their fp32 images
static bool schur_f32_ready(const QpdoDev *d) {
    return !d->comm.active && d->Atc.use_slab && d->Arc.use_slab && d->Atc.vsm32 && d->Arc.vsm32 && d->Atc.i16sm && d->Arc.i16sm;
}
// QPDO_PCG_INNER_F32=1: ONE inner CG solve on the fp32 images, accepted on its own recursive residual (opt-in, never the measured configuration)
static bool schur_inner_f32(const QpdoDev *d) { return d->inner_f32 && schur_f32_ready(d); }
// the default: the fp32 images only propose corrections, the solve is accepted on the fp64 residual (schur_inner_solve)
static bool schur_inner_refine(const QpdoDev *d) { return d->inner_refine && !d->inner_f32 && schur_f32_ready(d); }
// The fp32 inner CG stages fp32 copies of its two operand vectors and streams the column slabs in pairs (k_spmv_slab, XT = float;
// QPDO_INNER_X32=0: fp64 operands, slab by slab).  The copies are written where the vectors are: u = s_z -> s_z32 (cgcg_elem, k_cgcg_init,
// k_refine_init), t = tmp_n -> tmp_n32 (EpiDivDotSums, EpiDivDot).  Both schedules of the CG use the same width.
static bool schur_x32(const QpdoDev *d) { return d->inner_x32 && d->s_z32 && d->tmp_n32 && d->Arc.seg_pairs && d->Atc.seg_pairs && schur_f32_ready(d); }
// The coarse sweeps of the refined solve stream the half-precision images: the workspace has them, a scale, and the fp32 operand vectors
// (QPDO_INNER_H16; off with QPDO_INNER_X32=0)
static bool schur_h16_ready(const QpdoDev *d) { return d->inner_h16 && d->h16_set && d->Arc.vsm16 && d->Atc.vsm16 && schur_x32(d); }
// width: both products stream that copy of the values (narrow ones: single GPU); x32: and stage the fp32 copies of their operands, u being s_z
static int schur_S_apply(QpdoDev *d, const double *u, double *w, int par, const int *done2, bool sample, int *fcnt, StreamWidth width, bool x32 = false) {
    const bool dist = d->comm.active;
    const int n = d->n, kl = d->kact;
    double *Pf = d->part2 + 6 * PGRID;
    if (!dist) {
        const bool narrow = width != STREAM_F64;
        const float *u32 = (narrow && x32) ? d->s_z32 : nullptr; float *t32 = (narrow && x32) ? d->tmp_n32 : nullptr;
        launch_spmv_inner(d, d->Atc, u, u32, EpiDivDot{d->pc_diag, d->tmp_n, Pf, 0.0, t32}, true, done2, width);
        // HIP-event sample of the dominant kernel (the A_c product), taken mid-batch by the caller's choice of `sample`
        if (sample) (void)hipEventRecord(d->ev0, d->stream);
        launch_spmv_inner(d, d->Arc, d->tmp_n, t32, EpiSchurW{d->dc, u, w}, false, done2, width);
        if (sample) (void)hipEventRecord(d->ev1, d->stream);
        *fcnt = spmv_pgrid(d->Atc);
        return 0;
    }
    double *payload = d->dist_tmp;                   // [A_c,loc' u_loc (n) | (r,u) | (r,r) | sum u^2/d]
    if (kl > 0) launch_spmv(d, d->Atc, u, EpiStore{payload}, false);
    else HIPCHK(hipMemsetAsync(payload, 0, (size_t)n * 8, d->stream));
    hipLaunchKernelGGL(k_cgcg_pack3, dim3(1), dim3(BLK), 0, d->stream, (const int *)nullptr, (const double *)d->part2, par, vgrid(kl), payload + n);
    int rc = comm_allreduce(d, payload, (size_t)n + 3, 0); if (rc) return rc;
    d->st.inner_collectives++;
    hipLaunchKernelGGL((k_epi_apply<EpiDivDot>), dim3(vgrid(n)), dim3(BLK), 0, d->stream, n, (const double *)payload, EpiDivDot{d->pc_diag, d->tmp_n, Pf});
    if (kl > 0) launch_spmv(d, d->Arc, d->tmp_n, EpiSchurW{d->dc, u, w}, false);
    *fcnt = vgrid(n);
    return 0;
}
// s_x = S'^-1 b by the single-reduction Jacobi-PCG (device latch in ctrl2, batches of iterations between host syncs), to a recursive
// residual of tol ||b||.  width: the copy of the matrix values that the products stream.  init: b = s_v and k_cgcg_init runs; otherwise the
// caller has left the state of step 0 (k_refine_init, k_refine_norm).  first_batch: iterations issued before the first host read.
static int schur_inner_cg(QpdoDev *d, double tol, StreamWidth width, bool init, int first_batch, int *iters) {
    const bool dist = d->comm.active;
    const int kl = d->kact, g = vgrid(kl);
    double *P3 = d->part2;                   // [3 sums][2 parities][PGRID]; Pf behind them
    double *Pf = d->part2 + 6 * PGRID;
    const int *done2 = &d->ctrl2->cnt[C_PCG_DONE];
    const double *glob3 = dist ? d->dist_tmp + d->n : (const double *)nullptr;
    int fcnt = 0;
    // Two-launch schedule (single GPU, either value width, one element per thread of k_cgcg_step's grid): product 2 of application
    // j - 1 performs step j (EpiSchurStep), product 1 of application j forms that step's three partial sums first (EpiDivDotSums).
    // QPDO_INNER_FOLD=0 selects the three-launch schedule; both run the same device functions (pcg_kernels.inc) and give the same bits.
    const bool fold = d->inner_fold && !dist && (long long)g * BLK >= kl;
    // fp32 operands (schur_x32): u32, t32 are the copies that the step and product 1 write and the products stage; null otherwise
    const bool x32 = width != STREAM_F64 && schur_x32(d);
    float *u32 = x32 ? d->s_z32 : nullptr, *t32 = x32 ? d->tmp_n32 : nullptr;
    if (init) LAUNCH(k_cgcg_init, g, kl, (const double *)d->s_v, (const double *)d->s_diag, (const double *)d->dc, d->s_x, d->s_r, d->s_z, d->s_p, d->s_s, P3, d->ctrl2, u32);
    int rc = 0;
    if (fold) {
        launch_spmv_inner(d, d->Atc, d->s_z, u32, EpiDivDotSums{d->pc_diag, d->tmp_n, Pf, kl, 0, d->s_r, d->s_z, d->dc, (double *)nullptr, 0.0, t32}, true, done2, width);
        fcnt = spmv_pgrid(d->Atc);
    } else { rc = schur_S_apply(d, d->s_z, d->s_Sp, 0, dist ? nullptr : done2, false, &fcnt, width, x32); if (rc) return -1; }
    int j = 0;
    int batch = first_batch;
    while (j < SCHUR_INNER_MAXIT) {
        const int it_before = j, sample_b = batch / 2;
        for (int b = 0; b < batch; b++, j++) {           // issue iteration j: step j, then S' applied to the new u
            const bool sample = !dist && b == sample_b;
            if (fold) {
                // (the HIP-event sample of the A_c product includes the step it performs; its byte count is that of the product)
                if (sample) (void)hipEventRecord(d->ev0, d->stream);
                launch_spmv_inner(d, d->Arc, d->tmp_n, t32, EpiSchurStep{j, d->ctrl2, P3, g, Pf, fcnt, d->s_diag, d->dc, d->s_x, d->s_r, d->s_z, d->s_p, d->s_s, tol, nullptr, u32}, false, nullptr, width);
                if (sample) (void)hipEventRecord(d->ev1, d->stream);
                launch_spmv_inner(d, d->Atc, d->s_z, u32, EpiDivDotSums{d->pc_diag, d->tmp_n, Pf, kl, (j + 1) & 1, d->s_r, d->s_z, d->dc, P3, 0.0, t32}, true, done2, width);
            } else {
                LAUNCH(k_cgcg_step, g, kl, j, d->ctrl2, glob3, P3, g, (const double *)Pf, fcnt, (const double *)d->s_Sp, (const double *)d->s_diag,
                       (const double *)d->dc, d->s_x, d->s_r, d->s_z, d->s_p, d->s_s, tol, u32);
                rc = schur_S_apply(d, d->s_z, d->s_Sp, (j + 1) & 1, dist ? nullptr : done2, sample, &fcnt, width, x32); if (rc) return -1;
            }
            d->st.inner_steps++;
            if (x32) d->st.inner_x32_steps++;
            if (width == STREAM_H16) d->st.inner_h16_steps++;
        }
        rc = read_ctrl2(d); if (rc) return rc;
        if (!dist && d->hctrl2->cnt[C_PCG_IT] > it_before + sample_b) {          // the sampled iteration of this batch really ran
            float ms = 0.f;
            // (the bytes of the product that was sampled: the roofline fraction stays a statement about the kernel that ran)
            if (hipEventElapsedTime(&ms, d->ev0, d->ev1) == hipSuccess) { d->ev_ac_ms += ms; d->ev_ac_bytes += width == STREAM_H16 ? d->Arc.alg_bytes16() : width == STREAM_F32 ? d->Arc.alg_bytes32() : d->Arc.alg_bytes(); d->ev_ac_n++; }
        }
        if (d->hctrl2->cnt[C_PCG_DONE]) break;
        batch = 4;
    }
    *iters = d->hctrl2->cnt[C_PCG_IT];
    const double rn = d->hctrl2->val[V_RNORM], bn = d->hctrl2->val[V_BNORM];
    const bool conv = d->hctrl2->cnt[C_PCG_DONE] && (rn <= tol * bn);          // the latch is also set by a NaN residual
    return conv ? 0 : 1;                                                       // 1: not converged
}
// s = S'^-1 s_v to ||s_v - S' s||_2 <= tol ||s_v||_2; leaves d->s_sol pointing at s.  Returns 0, 1 (not converged) or < 0 (failure).
// Default where both compact matrices have their fp32 images (schur_inner_refine): iterative refinement.  s = 0, rho = b; per sweep the
// CG runs on the fp32 images with right-hand side rho to a recursive residual of theta tol ||b|| and gives e; s += e; rho = b - S' s with
// the fp64 images (one EpiDivDot and one EpiSchurW product, k_refine_init); the solve is accepted when ||rho|| <= tol ||b||.  The rounded
// matrices only propose corrections: what is accepted satisfies today's tolerance on the fp64 residual, and every vector, accumulation
// and test is fp64.  Past refine_maxsweep sweeps (or a sweep that does not converge) the solve is redone by the fp64 CG and counted.
// theta is a cost knob (QPDO_INNER_REFINE_THETA): docs/LAB_NOTES.md.
static int schur_inner_solve(QpdoDev *d, double tol, int *iters) {
    // The iteration count of an inner solve is almost the same as that of the previous one in the pass (same operator, same
    // tolerance), so the first batch runs to just short of it and the rest are short: few syncs and few latched (no-op) launches
    // after convergence.  (Row-partitioned: the collectives of a latched iteration still run, on every rank alike.)
    const int first_batch = d->schur_last_inner > 12 ? d->schur_last_inner - 6 : d->pcg_batch;
    d->st.inner_solves++;
    d->s_sol = d->s_x;
    if (!schur_inner_refine(d)) {
        const int st = schur_inner_cg(d, tol, schur_inner_f32(d) ? STREAM_F32 : STREAM_F64, true, first_batch, iters);
        if (st >= 0) d->schur_last_inner = *iters;
        return st;
    }
    const int kl = d->kact, g = vgrid(kl);
    double bn = 0.0, rho = 0.0;
    int total = 0;
    // Coarse sweeps (schur_h16_ready): the first h16_maxsweep sweeps stream the half-precision images and stop at a recursive residual of
    // max(theta tol ||b||, h16_eta ||rho||) -- the 11-bit matrix gains 2.5-2.8 decades of the fp64 residual per sweep whatever the CG is
    // asked for (tools/inner_h16_model.py).  Acceptance is the same test on the same fp64 residual after every sweep, coarse or not.
    const int coarse_sweeps = schur_h16_ready(d) ? d->h16_maxsweep : 0;
    for (int sweep = 0; sweep < d->refine_maxsweep; sweep++) {
        int it = 0;
        const bool coarse = sweep < coarse_sweeps;
        // the sweep's own right-hand side is rho: theta tol ||b|| relative to ||rho|| (not accepted: rho > tol ||b||, so this is < theta)
        double tol_s = sweep == 0 ? d->refine_theta * tol : d->refine_theta * tol * bn / rho;
        if (coarse && tol_s < d->h16_eta) tol_s = d->h16_eta;
        // with coarse sweeps a later sweep's iteration count is remembered like the first one's: batches of pcg_batch, their reads and
        // latched launches, would cost a 40-iteration sweep a tenth of its time
        int *mem = sweep == 0 ? &d->schur_last_inner : sweep < QpdoDev::SWEEP_MEMORY ? &d->sweep_last_inner[sweep] : (int *)nullptr;
        const int fb = sweep == 0 ? first_batch : (coarse_sweeps && mem && *mem > 12) ? *mem - 6 : d->pcg_batch;
        const int st = schur_inner_cg(d, tol_s, coarse ? STREAM_H16 : STREAM_F32, sweep == 0, fb, &it);
        if (st < 0) return st;
        total += it;
        if (sweep == 0) bn = d->hctrl2->val[V_BNORM];
        if (mem) *mem = it;
        if (st) break;                                                         // not converged, or NaN: the fp64 CG decides
        if (coarse) d->st.inner_h16_sweeps++;
        LAUNCH(k_refine_acc, g, kl, sweep == 0 ? 1 : 0, (const double *)d->s_x, d->s_acc);
        int fcnt = 0;
        if (schur_S_apply(d, d->s_acc, d->s_Sp, 0, nullptr, false, &fcnt, STREAM_F64)) return -1;
        LAUNCH(k_refine_init, g, kl, (const double *)d->s_v, (const double *)d->s_Sp, (const double *)d->s_diag, (const double *)d->dc,
               d->s_x, d->s_r, d->s_z, d->s_p, d->s_s, d->part2, schur_x32(d) ? d->s_z32 : (float *)nullptr);
        LAUNCH(k_refine_norm, 1, (const double *)d->part2, g, d->ctrl2);
        { const int rc = read_ctrl2(d); if (rc) return rc; }
        rho = d->hctrl2->val[V_RNORM];
        d->st.inner_refine_sweeps++; d->st.inner_refine_fp64_applies++;
        if (!(rho == rho)) break;
        if (rho <= tol * bn) {
            const double ratio = bn > 0.0 ? rho / (tol * bn) : 0.0;
            if (ratio > d->st.inner_refine_max_res_over_tol) d->st.inner_refine_max_res_over_tol = ratio;
            d->s_sol = d->s_acc;
            *iters = total;
            return 0;
        }
    }
    d->st.inner_refine_fallbacks++;
    int it = 0;
    const int st = schur_inner_cg(d, tol, STREAM_F64, true, first_batch, &it);
    *iters = total + it;
    return st;
}
// z <- M^-1 r given u = Dq^-1 r in pc_z; leaves the r.z partials in p_rz.  Returns their count (or -1 on failure).
static int schur_apply(QpdoDev *d, double tol, double *p_rz, int *inner_iters, int *status) {
    const bool dist = d->comm.active;
    const int kl = d->kact;
    if (!dist || kl > 0) launch_spmv(d, d->Arc, d->pc_z, EpiStore{d->s_v}, false);      // rows of A_c are local: no exchange
    int it = 0;
    *status = schur_inner_solve(d, tol, &it);
    *inner_iters += it;
    if (*status < 0) return -1;
    if (dist) {
        if (kl > 0) launch_spmv(d, d->Atc, d->s_sol, EpiStore{d->dist_tmp}, false);
        else HIPCHK(hipMemsetAsync(d->dist_tmp, 0, (size_t)d->n * 8, d->stream));
        if (comm_allreduce(d, d->dist_tmp, (size_t)d->n, 0)) return -1;
        hipLaunchKernelGGL((k_epi_apply<EpiDeflZ>), dim3(vgrid(d->n)), dim3(BLK), 0, d->stream, d->n, (const double *)d->dist_tmp, EpiDeflZ{d->pc_diag, d->pc_r, d->pc_z, p_rz});
        return vgrid(d->n);
    }
    launch_spmv(d, d->Atc, d->s_sol, EpiDeflZ{d->pc_diag, d->pc_r, d->pc_z, p_rz}, true);
    return spmv_pgrid(d->Atc);
}
// The per-block partial arrays of the outer PCG in d->part, named once per solve.
struct PcgPart { double *rz, *rr, *pKp, *rinf; };
static PcgPart pcg_part(const QpdoDev *d) { double *P = d->part; return {P + P_RZ * PGRID, P + P_RR * PGRID, P + P_PKP * PGRID, P + P_RINF * PGRID}; }
// The device latch is set on convergence and on a NaN residual alike; this is the host's copy of the convergence test, on the
// residual norms the device published with the latch.
static bool pcg_within_tol(const QpdoDev *d) {
    return d->hctrl->val[V_RNORM] <= d->pcg_tol * d->hctrl->val[V_BNORM] || d->hctrl->val[V_RINF] <= d->pcg_abs_now;
}
// Kp = K p for p = pc_p, K = Q + sigma_f I + A_c' D A_c, with the per-block partial sums of p.Kp in p_pKp (*cnt of them); every
// launch leaves at once when the latch `done` is set.  Only launches, events and the collective: capturable into a hipGraph.
// sample: HIP events around the Q product.
static int pcg_K_apply(QpdoDev *d, const int *done, double *p_pKp, bool sample, int *cnt) {
    const int n = d->n, k = d->kact;
    if (d->comm.active) {   // K p = sigma_f p + sum over ranks of ( Q_rows p  [rows n0..]  +  A_c,loc' (d_c .* A_c,loc p) )
        HIPCHK(hipMemsetAsync(d->Kp_part, 0, (size_t)n * 8, d->stream));
        if (k > 0) launch_spmv(d, d->Arc, d->pc_p, EpiPcgA{d->dc, d->tc, nullptr}, false, done);
        if (sample) (void)hipEventRecord(d->ev0, d->stream);
        if (d->nloc > 0) launch_spmv(d, d->Qs, d->pc_p, EpiAddTo{d->Kp_part, d->n0}, false, done);
        if (sample) (void)hipEventRecord(d->ev1, d->stream);
        if (k > 0) launch_spmv(d, d->Atc, d->tc, EpiAddTo{d->Kp_part, 0}, false, done);
        int rc = comm_allreduce(d, d->Kp_part, (size_t)n, 0); if (rc) return rc;
        *cnt = vgrid(n);
        hipLaunchKernelGGL(k_pcg_dist_finish, dim3(*cnt), dim3(BLK), 0, d->stream, n, done, (const double *)d->Kp_part, (const double *)d->pc_p,
                           d->sigma_f, d->pc_Kp, p_pKp);
    } else if (k > 0) {
        launch_spmv(d, d->Arc, d->pc_p, EpiPcgA{d->dc, d->tc, nullptr}, false, done);
        if (sample) (void)hipEventRecord(d->ev0, d->stream);
        launch_spmv(d, d->Qf, d->pc_p, EpiPcgQ{d->pc_p, d->sigma_f, d->pc_Kp}, false, done);
        if (sample) (void)hipEventRecord(d->ev1, d->stream);
        launch_spmv(d, d->Atc, d->tc, EpiPcgAt{d->pc_p, d->pc_Kp, p_pKp}, true, done);
        *cnt = spmv_pgrid(d->Atc);
    } else {                // no weighted rows
        if (sample) (void)hipEventRecord(d->ev0, d->stream);
        launch_spmv(d, d->Qf, d->pc_p, EpiPcgQdot{d->pc_p, d->sigma_f, d->pc_Kp, p_pKp}, true, done);
        if (sample) (void)hipEventRecord(d->ev1, d->stream);
        *cnt = spmv_pgrid(d->Qf);
    }
    return 0;
}
// K dx = rhs with the Schur-preconditioned outer CG.  *fallback = 1: did not converge, the caller reruns Jacobi-PCG.
static int pcg_schur_solve(QpdoDev *d, int *iters_out, int *fallback) {
    const bool dist = d->comm.active;
    const int n = d->n, kl = d->kact, k = dist ? d->kg : d->kact, g = vgrid(n);
    const PcgPart P = pcg_part(d);
    *fallback = 0;
    LAUNCH(k_axpy_const, g, n, (const double *)d->qdiag, d->sigma_f, d->pc_diag);                  // Dq
    // inner diagonal Sd_i = 1/d_i + sum_j A_ij^2 / Dq_j over this rank's compact rows (partitioned: no exchange)
    // (build_compact has left it when it read the weighted rows once, with this sigma_f)
    d->sdiag_from_build = kl > 0 && d->sdiag_valid && d->sdiag_sigma == d->sigma_f;
    if (kl > 0 && !d->sdiag_from_build) {
        DISPATCH_TPR(d->Ar, k_schur_diag, rowloop_grid(d->Ar), kl, d->Arc.rp, d->Arc.ci, d->Arc.val,
                     (const double *)d->pc_diag, (const double *)d->dc, d->s_diag);
    }
    // Inner tolerance.  An inner residual rho leaves M z - r = A_c' D rho: the error that matters is weighted by D, so
    // the tolerance must shrink with the largest weight (a constant tau sufficed on every C4 pass with dmax <= 5e3 and
    // failed at dmax = 7e5).  It is also tightened on the fly whenever an outer step reduces the residual by less than 4x.
    LAUNCH(k_ctrl_clear_aux, 1, d->ctrl);
    if (kl > 0) LAUNCH(k_absmax_mul, vgrid(kl), kl, (const double *)d->dc, (const double *)nullptr, d->ctrl, N_A);
    if (dist) { int rcx = comm_allreduce(d, reinterpret_cast<double *>(&d->ctrl->nrm[N_A]), 1, 1); if (rcx) return rcx; }   // bit pattern of a non-negative double
    LAUNCH(k_pcg_init, g, n, d->rhs, d->pc_diag, d->dx, d->pc_r, d->pc_z, d->pc_p, P.rz, P.rr);
    { int rc0 = read_ctrl(d); if (rc0) return rc0; }
    const double dmax = nrm_of(d->hctrl, N_A);
    d->schur_last_inner = 0;
    for (int &v : d->sweep_last_inner) v = 0;
    // Base value: the inner solve only defines a preconditioner, so this is a cost knob, not an accuracy one.  C4 time-to-eps against
    // it (tools/tol_probe.py, one box): 1e-6 8.01 s, 2e-6 7.83, 3e-6 7.45, 4e-6 7.56, 5e-6 7.67, 7e-6 8.03, 1e-5 8.70 (the on-the-fly
    // tightening starts to fire), 1e-4 20.4; the n = 1.3e4 / 3e4 fixtures have the same shallow basin.  3e-6 = its middle.
    const double tau0 = d->schur_tau0;
    double tau = tau0 * (dmax > 1e4 ? 1e4 / dmax : 1.0);
    if (tau < 1e-13) tau = 1e-13;
    int inner = 0, st = 0;
    int cnt_rz = schur_apply(d, tau, P.rz, &inner, &st);
    if (cnt_rz < 0) return -1;
    if (st) { *fallback = 1; return 0; }
    LAUNCH(k_copy, g, n, (const double *)d->pc_z, d->pc_p);
    LAUNCH(k_pcg_init2, 1, P.rz, cnt_rz, P.rr, g, d->ctrl);
    const int *done = &d->ctrl->cnt[C_PCG_DONE];
    int outer = 0;
    double prev_rn = -1.0;
    { int rc = read_ctrl(d); if (rc) return rc; }          // (the latch after k_pcg_init2: a zero right-hand side is done at once)
    for (;;) {
        if (d->hctrl->cnt[C_PCG_DONE]) break;
        if (outer > 0) {
            const double rn = d->hctrl->val[V_RNORM];
            if (prev_rn > 0.0 && rn > 0.25 * prev_rn && tau > 1e-13) { tau *= 1e-2; if (tau < 1e-13) tau = 1e-13; }
            prev_rn = rn;
        }
        if (d->hybrid_active && outer + inner > d->hybrid_budget) { snprintf(g_err, sizeof(g_err), "hybrid: PCG budget exceeded"); return PCG_NOT_CONVERGED; }
        if (outer >= SCHUR_OUTER_MAXIT) { if (d->defl_debug) fprintf(stderr, "[schur] k=%d outer cap reached (inner=%d)\n", k, inner); *fallback = 1; return 0; }
        int pKp_cnt = 0;
        { int rc = pcg_K_apply(d, done, P.pKp, false, &pKp_cnt); if (rc) return rc; }
        LAUNCH(k_pcg_update, g, n, (const Ctrl *)d->ctrl, P.pKp, pKp_cnt, (const double *)d->pc_p, (const double *)d->pc_Kp,
               (const double *)d->pc_diag, d->dx, d->pc_r, d->pc_z, P.rz, P.rr,
               d->scaled ? (const double *)d->Dinv : (const double *)nullptr, P.rinf);
        // Convergence is decided HERE, from the residual the update just formed (round 3; it used to be decided after the
        // preconditioner had been applied to that residual): a converged iteration no longer pays for an inner solve -- ~60 inner
        // iterations, one in eight of a pass -- whose result nobody uses.  Same test on the same numbers: same iteration counts, same dx.
        LAUNCH(k_pcg_scalar, 1, d->ctrl, P.rz, cnt_rz, P.rr, g, d->pcg_tol, P.rinf, d->scaled ? d->sc_cinv : 1.0, d->pcg_abs_now, 1);
        { int rc = read_ctrl(d); if (rc) return rc; }
        outer++;
        if (d->hctrl->cnt[C_PCG_DONE]) break;
        cnt_rz = schur_apply(d, tau, P.rz, &inner, &st);
        if (cnt_rz < 0) return -1;
        if (st) { if (d->defl_debug) fprintf(stderr, "[schur] k=%d inner solve did not converge (outer=%d inner=%d)\n", k, outer, inner); *fallback = 1; return 0; }
        LAUNCH(k_pcg_scalar, 1, d->ctrl, P.rz, cnt_rz, P.rr, g, d->pcg_tol, P.rinf, d->scaled ? d->sc_cinv : 1.0, d->pcg_abs_now, 2);
        LAUNCH(k_pcg_p, g, n, (const Ctrl *)d->ctrl, (const double *)d->pc_z, d->pc_p);
    }
    if (d->defl_debug) fprintf(stderr, "[schur] dmax=%.2e tau_end=%.1e ", dmax, tau);
    {   // the latch is also set by a NaN residual: that is not convergence -- let the Jacobi path redo the pass
        const double rnv = d->hctrl->val[V_RNORM], bnv = d->hctrl->val[V_BNORM];
        if (outer > 0 && !pcg_within_tol(d)) { *fallback = 1; return 0; }
        if (outer > 0 && bnv > 0.0 && rnv / bnv > d->st.pcg_max_relres) d->st.pcg_max_relres = rnv / bnv;
    }
    *iters_out = outer + inner;
    d->schur_passes++;
    // converged, but slowly: Q is far from its diagonal in the spectral sense and every outer step pays a full inner solve --
    // the deflated Jacobi-PCG is the better solver for such a Q (two slow passes switch the mode off for the solve)
    if (outer > 20 && ++d->schur_strikes >= 2) d->schur_off = 1;
    if (d->defl_debug) fprintf(stderr, "[schur] k=%d outer=%d inner=%d\n", k, outer, inner);
    return 0;
}
// The reference solves the Newton system exactly (CHOLMOD); a PCG solve that ends without meeting its tolerance must not
// hand an arbitrary dx to the linesearch silently.  `done`: the device latch; rnorm / bnorm: the last recursive residual
// and right-hand side 2-norms.  NaN, or a relative residual above PCG_SOFT_TOL, ends the solve with an error (status
// QPDO_ERROR through the driver); a stalled or capped solve below it is accepted and counted in the statistics.
static const double PCG_SOFT_TOL = 1e-8;
static int pcg_verdict(QpdoDev *d, bool converged, double rnorm, double bnorm, const char *which, bool stalled = false) {
    const double rel = bnorm > 0.0 ? rnorm / bnorm : 0.0;
    if (!(rel == rel) || !(rnorm == rnorm)) { snprintf(g_err, sizeof(g_err), "%s: NaN residual in the linear solve", which); return PCG_NAN; }
    if (rel > d->st.pcg_max_relres) d->st.pcg_max_relres = rel;
    if (converged) return 0;
    if (rel <= PCG_SOFT_TOL) { d->st.pcg_soft_accepts++; return 0; }
    snprintf(g_err, sizeof(g_err), "%s did not converge: relative residual %.3e (tolerance %.1e, %s)%s", which, rel, d->pcg_tol,
             stalled ? "stagnated: no 1 % progress in 3000 iterations" : "iteration cap reached",
             d->cur_proximal ? "" : "; settings->proximal = 0: the Newton matrix Q + A'DA has no proximal term and may be singular");
    return PCG_NOT_CONVERGED;
}
static int pcg_solve(QpdoDev *d, int *iters_out) {
    const int n = d->n;
    if (!d->qdiag_valid) {
        LAUNCH(k_extract_diag, vgrid(n), n, d->Qf.rp, d->Qf.ci, d->Qf.val, d->qdiag);
        d->qdiag_valid = 1;
    }
    int rc = build_compact(d); if (rc) return rc;
    const int k = d->kact;
    {   // Schur-complement mode whenever its inner system is well conditioned (k/n <= 0.8) and worth the set-up (k >= 256);
        // it also wins on the early passes (uniform weights): fewer products and almost none of them with Q
        // (C4: 9.2 s when used only after a slow Jacobi pass, 8.8 s when used from the first pass on)
        long long kglob = k;
        if (d->comm.active && !d->schur_off && d->schur_mode != 0) {     // global number of weighted rows (eligibility only)
            const double kd = (double)k;
            HIPCHK(hipMemcpyAsync(d->dist_tmp, &kd, 8, hipMemcpyHostToDevice, d->stream));
            rc = comm_allreduce(d, d->dist_tmp, 1, 0); if (rc) return rc;
            double ks = 0.0;
            HIPCHK(hipMemcpyAsync(&ks, d->dist_tmp, 8, hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
            kglob = (long long)ks;
            d->kg = (int)kglob;
        }
        if (schur_allowed(d, kglob)) {
            int fb = 0;
            rc = pcg_schur_solve(d, iters_out, &fb); if (rc) return rc;
            if (!fb) return 0;
            if (++d->schur_strikes >= 2) d->schur_off = 1;      // did not converge twice: plain path from here on
        }
    }
    rc = defl_build(d); if (rc) return rc;
    const bool defl = d->defl_r > 0;
    const bool dist = d->comm.active;
    // Jacobi diagonal Q_jj + sigma_f + sum_i A_ij^2 d_i; row-partitioned: the sum over the local rows, summed over the ranks, then the rest
    auto jacobi_diag = [&](const double *base, double shift, double *out) {
        DISPATCH_TPR(d->At, k_jacobi_diag, rowloop_grid(d->At), n, d->Atc.rp, d->Atc.ci, d->Atc.val, (const double *)d->dc, base, shift, out);
    };
    if (!defl && dist) {
        if (k > 0) jacobi_diag(d->zeros_n, 0.0, d->dist_tmp);
        else HIPCHK(hipMemsetAsync(d->dist_tmp, 0, (size_t)n * 8, d->stream));
        rc = comm_allreduce(d, d->dist_tmp, (size_t)n, 0); if (rc) return rc;
        LAUNCH(k_add3, vgrid(n), n, (const double *)d->dist_tmp, (const double *)d->qdiag, d->sigma_f, d->pc_diag);
    } else if (!defl) {
        if (k > 0) jacobi_diag(d->qdiag, d->sigma_f, d->pc_diag);
        else LAUNCH(k_axpy_const, vgrid(n), n, (const double *)d->qdiag, d->sigma_f, d->pc_diag);
    }
    const int g = vgrid(n);
    const PcgPart P = pcg_part(d);
    const int *done = &d->ctrl->cnt[C_PCG_DONE];
    LAUNCH(k_pcg_init, g, n, d->rhs, d->pc_diag, d->dx, d->pc_r, d->pc_z, d->pc_p, P.rz, P.rr);
    int cnt_rz = g;
    if (defl) {
        cnt_rz = defl_apply(d, nullptr, P.rz);
        LAUNCH(k_copy, g, n, (const double *)d->pc_z, d->pc_p);
    }
    LAUNCH(k_pcg_init2, 1, P.rz, cnt_rz, P.rr, g, d->ctrl);
    // one PCG iteration as a sequence of launches on the backend stream
    auto issue_iteration = [&](bool sample) -> int {
        int pKp_cnt = 0;
        { int rcx = pcg_K_apply(d, done, P.pKp, sample, &pKp_cnt); if (rcx) return rcx; }
        LAUNCH(k_pcg_update, g, n, d->ctrl, P.pKp, pKp_cnt, d->pc_p, d->pc_Kp, d->pc_diag, d->dx, d->pc_r, d->pc_z,
               P.rz, P.rr, d->scaled ? (const double *)d->Dinv : (const double *)nullptr, P.rinf);
        if (defl) defl_apply(d, done, P.rz);
        LAUNCH(k_pcg_scalar, 1, d->ctrl, P.rz, cnt_rz, P.rr, g, d->pcg_tol, P.rinf, d->scaled ? d->sc_cinv : 1.0, d->pcg_abs_now);
        LAUNCH(k_pcg_p, g, n, d->ctrl, d->pc_z, d->pc_p);
        return 0;
    };
    // Launch-bound regime (cache-resident matrices): replay a captured batch of iterations as a hipGraph.  The
    // kernels leave immediately once the device-side latch is set, so replaying whole batches stays exact.
    hipGraph_t graph = nullptr; hipGraphExec_t gexec = nullptr;
    const bool use_graph = d->pcg_graph && !dist && !d->Qf.use_slab && d->pcg_maxit >= d->pcg_batch;
    if (use_graph) {
        bool ok = hipStreamBeginCapture(d->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            for (int b = 0; b < d->pcg_batch && ok; b++) ok = issue_iteration(false) == 0;
            hipError_t e = hipStreamEndCapture(d->stream, &graph);
            ok = ok && e == hipSuccess && graph;
        }
        if (ok) ok = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (!ok) { if (graph) (void)hipGraphDestroy(graph); graph = nullptr; gexec = nullptr; (void)hipGetLastError(); }
    }
    int it = 0;
    rc = 0;
    double best_rn = -1.0; int best_it = 0; bool stalled = false;
    const int maxit_now = (d->hybrid_active && d->hybrid_budget < d->pcg_maxit) ? d->hybrid_budget : d->pcg_maxit;
    while (it < maxit_now) {
        const int it_before = it;
        int batch = d->pcg_batch; if (it + batch > maxit_now) batch = maxit_now - it;
        if (gexec && batch == d->pcg_batch) {
            hipError_t e = hipGraphLaunch(gexec, d->stream);
            if (e != hipSuccess) { rc = set_err(e, "hipGraphLaunch", __LINE__); break; }
            d->st.spmv_calls += (k > 0 ? 3 : 1) * (batch - 1);      // issue_iteration counted one batch during capture
        } else {
            for (int b = 0; b < batch && !rc; b++) rc = issue_iteration(b == 0 && !gexec);
            if (rc) break;
        }
        it += batch;
        rc = read_ctrl(d); if (rc) break;
        if (!gexec && d->hctrl->cnt[C_PCG_IT] > it_before) {      // the sampled (first) iteration of this batch really ran
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, d->ev0, d->ev1) == hipSuccess) { d->ev_spmv_ms += ms; d->ev_spmv_n++; }
        }
        if (d->hctrl->cnt[C_PCG_DONE]) break;
        // stagnation exit: no 1 % improvement of the residual norm over 3000 iterations (a system with kappa ~ 1e12 can sit at
        // its attainable accuracy forever; without this the cap costs 100000 x 3 SpMV before anyone notices)
        const double rn = d->hctrl->val[V_RNORM];
        if (best_rn < 0.0 || rn < 0.99 * best_rn) { best_rn = rn; best_it = it; }
        else if (it - best_it >= 3000) { stalled = true; break; }
    }
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    *iters_out = d->hctrl->cnt[C_PCG_IT];
    d->last_jacobi_iters = *iters_out;
    {   // DONE is also latched on a NaN residual (k_pcg_scalar): "converged" means DONE with a finite residual within tolerance
        const double rnv = d->hctrl->val[V_RNORM], bnv = d->hctrl->val[V_BNORM];
        const bool conv = d->hctrl->cnt[C_PCG_DONE] && (bnv == 0.0 || *iters_out == 0 || pcg_within_tol(d));
        if (!conv && d->hybrid_active) { snprintf(g_err, sizeof(g_err), "hybrid: PCG budget exceeded"); return PCG_NOT_CONVERGED; }      // (no soft accept: the dense factor takes over)
        rc = pcg_verdict(d, conv, (bnv == 0.0 || *iters_out == 0) ? 0.0 : rnv, bnv, "Jacobi-PCG", stalled); if (rc) return rc;
    }
    if (d->defl_debug) fprintf(stderr, "[pcg] k=%d defl_r=%d iters=%d\n", k, d->defl_r, *iters_out);
    return 0;
}

