// state.inc -- part of qpdo_dev.hip (one translation unit; included in order): control block, matrix and workspace state
// ------------------------------------------------------------------------------------------------
// control block: everything the host reads back per pass
// ------------------------------------------------------------------------------------------------
enum { N_PRIM = 0, N_DUAL, N_PRIM_IN, N_DUAL_IN, N_A, N_B, N_C, N_D, N_COUNT };
enum { C_ACTIVE = 0, C_ENTER, C_LEAVE, C_NL, C_KSTAR, C_MUCH, C_VIOL, C_PCG_DONE, C_PCG_IT, C_CHAIN_ERR, C_DINF,
       C_SPEC_SKIP, C_SPEC_BRANCH,            // launch-ahead of the Newton step (k_resid_mn decides, host_step.inc ahead_enqueue_step): nonzero = the guarded kernels leave at once; the factor branch
       C_UD_REJECT,                           // up/downdate of the kept dense factor (dev/updown.inc): a scan met a pivot that is not a positive finite number
       C_COUNT = 16 };
enum { V_TAU = 0, V_A0, V_B0, V_RZ, V_BNORM, V_OOB, V_QDX, V_OBJ, V_F, V_RR, V_RNORM, V_RINF = 15, V_COUNT = 16 };
struct Ctrl {
    u64 nrm[N_COUNT];      // non-negative doubles as bit patterns: atomicMax is exact and order free
    int cnt[C_COUNT];
    double val[V_COUNT];
};
// one right-hand side's slots of the group control array (dev/adjoint.inc adj_sweeps_group): the four maxima the single call keeps in
// N_A .. N_D of the control block, and the non-finite marker it keeps in C_VIOL
struct AdjGrpCtrl { u64 nrm[4]; int nonfin, pad; };

// partial-sum slots (each PGRID doubles)
enum { P_ETA_M = 0, P_BETA_M, P_A0, P_B0, P_DXQDX, P_DXDF, P_PKP, P_RZ, P_RR, P_OOB, P_QDX, P_OBJ, P_F1, P_F2, P_RINF, P_COUNT };

struct DevCsr {
    int nrows = 0, ncols = 0;
    long long nnz = 0;
    int *rp = nullptr, *ci = nullptr;
    double *val = nullptr;
    int tpr = 64;            // threads cooperating on one row
    // LDS-staged variant: columns are cut into `nslabs` slabs of W columns; sp[r*(nslabs+1)+s] is the
    // position inside row r where slab s starts (rows are column-sorted, so a slab is a sub-range)
    int use_slab = 0, nslabs = 0, W = 0, rows_per_wg = 0, slab_grid = 0;
    int slab_ovl = 1;        // k_spmv_slab issues the next slab's first loads before its barriers (QPDO_SLAB_OVERLAP=0: the old schedule)
    int slab_nt = 0;         // QPDO_SLAB_NT=1: k_spmv_slab reads the values with non-temporal loads (off: faster per launch in the lab, not in the C4 solve)
    int *sp = nullptr;
    unsigned short *ci16 = nullptr;   // column index inside its slab (W < 65536): 10 instead of 12 bytes per nonzero
    // Slab-major image, the arrays the slab kernel actually streams: per workgroup the row segments of slab 0 back to
    // back, then those of slab 1, ... so that a slab phase reads one sequential range instead of 1.3 KB pieces at a
    // row stride (measured on C4: 6.4 -> 7.3 TB/s algorithmic).  seg[r*nslabs+s] = {start, length}; rebuilt lazily
    // (sm_dirty) after the values or the structure of the row-major arrays change.
    double *vsm = nullptr; unsigned short *i16sm = nullptr; int *cism = nullptr; int2 *seg = nullptr; mutable int sm_dirty = 1;
    int seg_pairs = 0;                // the image is in pair order (k_slab_seg): the compact matrices of a workspace whose fp32 CG stages fp32 operands
    float *vsm32 = nullptr;           // optional fp32 copy of vsm (the stream of the Schur mode's inner CG: QPDO_PCG_INNER_REFINE, QPDO_PCG_INNER_F32)
    // optional half-precision copy of vsm in the same image, scaled by the workspace's power of two (QpdoDev::h16_e): the stream of the
    // refined inner solve's coarse sweeps (QPDO_INNER_H16).  Only on an image in pair order (seg_pairs).
    _Float16 *vsm16 = nullptr;
    // pair-local 16-bit indices of an image in pair order (seg_pairs): i16sm's slab-local index, plus W for an entry of the odd slab of a
    // pair -- the index words of the pair-wide products (k_spmv_slab, XT = float), whose LDS holds the 2 W floats of a pair (2 W <= 65536:
    // the kernel's LDS holds fewer than 40 960 floats).  The slab-by-slab products of the same image read i16sm.
    unsigned short *p16sm = nullptr;
    double alg_bytes() const { return 12.0 * (double)nnz + 4.0 * (nrows + 1) + 8.0 * nrows + 8.0 * ncols; }
    double alg_bytes32() const { return alg_bytes() - 4.0 * (double)nnz; }       // the same product on the fp32 copy of the values
    double alg_bytes16() const { return alg_bytes() - 6.0 * (double)nnz; }       // ... and on the half-precision copy
};

// Row partition of one large QP over G ranks (one process per GPU): every vector is replicated, only the
// matrices are split (rows [m0, m0+mloc) of A, the matching columns of A', rows [n0, n0+nloc) of Q for the PCG
// operator).  The single exchange step is a sum all-reduce of an n-vector per A' / K product (plus max / sum
// all-reduces of the Ruiz norms and of A x results): RCCL on the backend stream, or a host callback (tests).
struct Comm {
    int rank = 0, world = 1, mode = 0;          // mode: 0 none, 1 host callback, 2 RCCL
    bool active = false;                         // world > 1, or a forced single-rank communicator (tests of the RCCL branch)
    qdev_allreduce_fn fn = nullptr; void *ctx = nullptr;
    ncclComm_t nccl = nullptr;
    double *hbuf = nullptr; size_t hcap = 0;     // pinned staging for the host-callback mode
};
static const int DENSE_LIMIT_N = 40000;      // largest order the dense direct solver accepts (the dense matrix: 12.8 GB; every tile index in 32 bits)
struct QpdoDev {
    int device = 0, n = 0, m = 0;
    int m0 = 0, mloc = 0, n0 = 0, nloc = 0;      // this rank's slices (whole ranges when world == 1)
    Comm comm;
    double *dist_tmp = nullptr, *Kp_part = nullptr, *zeros_n = nullptr;
    hipStream_t stream = nullptr;
    DevCsr Ar, At, Qf;        // world > 1: Ar = local rows (mloc x n), At = local columns (n x mloc), Qf replicated
    DevCsr Qs;                // world > 1: rows [n0, n0+nloc) of Qf for the PCG operator
    // compact index space of the current Newton pass: the k weighted rows of A, renumbered 0..k-1
    DevCsr Arc, Atc;          // A_c (k x n) and A_c' (n x k)
    int *row_cnt = nullptr, *cidx = nullptr, *rowlist = nullptr, *kcount = nullptr; int kact = 0;
    u64 *flag_bits = nullptr; int *flag_wprefix = nullptr;      // the pass's weighted rows as a bit mask + per-word prefix (LDS tables of the compaction)
    double *dc = nullptr, *tc = nullptr; int lds_doubles_At = 0;
    // per-pass set-up (build_compact), each switch read at setup; 0 selects the former sequence, the same bits:
    int compact_one_read = 1; // QPDO_COMPACT_ONE_READ: A_c's CSR copy, slab image and Schur diagonal from one read of the weighted rows
    int compact_t_one_read = 1; // QPDO_COMPACT_T_ONE_READ: A_c' the same way: slab pointers from the counting pass, CSR and image from one compaction
    int *scan_tsum = nullptr; // tile sums of a pass's scans (dev_scan)
    int sdiag_valid = 0; double sdiag_sigma = 0.0;      // s_diag holds this pass's Schur diagonal, formed with that sigma_f
    int sdiag_from_build = 0;                           // the last pcg_schur_solve took that diagonal instead of running k_schur_diag (probe: info[10])
    double *qdiag = nullptr; int qdiag_valid = 0;
    // heavy-row deflation
    // knobs read from the environment ONCE, at qdev_configure (not per pass: getenv is not safe against a concurrent setenv)
#ifdef QPDO_TEST_HOOKS              // (test builds only: _build.build_lib_testhooks; never in the product library)
    int chain_inject = -1;          // QPDO_DENSE_CHAIN_INJECT=<Newton pass>: pretend that pass's chained solve lost a producer
#endif
    double schur_tau0 = 3e-6;       // QPDO_SCHUR_TAU: base of the inner tolerance of the Schur-complement mode
    int defl_debug = 0;             // QPDO_DEFL_DEBUG: per-pass solver diagnostics on stderr
    int ctrl_clean = 0;                         // the per-pass slots of the control block are zero (the last Newton step cleared them)
    int defer_step = 0, step_pending = 0;       // deferred read-back of the Newton step (see qdev_set_deferred_step)
    int pend_proximal = 0; double pend_sigma = 0.0;
    int pcg_dense_fallback = 1;   // redo a PCG solve that cannot converge with the dense solver (n <= DENSE_LIMIT_N; QPDO_PCG_DENSE_FALLBACK=0: error)
    int cur_proximal = 1;      // settings->proximal of the Newton step in progress (error messages, stopping rule)
    int deflate = 1, defl_r = 0, max_row_nnz_A = 0; DevCsr Ath; int *defl_hist = nullptr, *defl_list = nullptr, *defl_count = nullptr;
    double *defl_flag = nullptr, *defl_t = nullptr, *defl_S = nullptr, *defl_Sinv = nullptr, *defl_v = nullptr; long long defl_passes = 0;
    // dense direct solver
    int dense_ld = 0, dense_nblk = 0, dense_valid = 0;
    int dense_max_n = 12288;  // dense beats deflated PCG at n = 1e4 (0.90 s vs 1.35 s at C2, DESIGN.md 3.4)
    // hybrid of the two solvers for mid-size dense problems (QPDO_HYBRID): every solve starts with PCG, whose early Newton systems (few
    // active rows, moderate weights) cost 13-400 iterations against a 13 ms factorization, and switches to the dense factor for the rest of
    // the solve at the first pass whose iteration count exceeds the budget
    int hybrid = 0, hybrid_active = 0, hybrid_budget = 450;
    int dense_asm_tile = 19000;   // rows of a column the assembly accumulates in LDS at a time (152 KB of the 160 KB)
    // band direct solver (dev/band.inc): half-bandwidth of Q + A'A (-1: not banded within BAND_WIDE_MAX_B), order padded to 4, band storage
    int band_b = -1, band_np = 0; double *Kb = nullptr, *Lt = nullptr, *band_z = nullptr;
    // a variable order of the band solver (qdev_set_band_order; null: the caller's order, and nothing below is read): bo_newold[k] = the
    // caller's index of the variable at position k, bo_oldnew its inverse (device, n each); bo_b: the half-bandwidth under it, from the
    // host (band_order.c; band_detect takes it instead of measuring).  bo_seen_*: the bandwidths of an order that was looked at,
    // adopted or not, for setup's "not banded" message (-1: none was).
    int *bo_newold = nullptr, *bo_oldnew = nullptr; int bo_b = -1, bo_seen_nat = -1, bo_seen_ord = -1;
    // chain QPs with dense coupling rows (QPDO_BAND_COUPLING = band_coupling > 0; dev/band.inc): bc_r of them (0: none, the plain band
    // solver), band_b is then the half-bandwidth of the OTHER rows and of Q.  bc_over: more than band_coupling were counted (setup's
    // message).  The kept factor of B belongs to (bc_dfact, bc_fact_sigma); bc_zvalid: the slots whose column of Z = B^-1 U was solved with
    // it; bc_act / bc_k: the slots with a nonzero weight that S was last built and factored for.
    int band_coupling = 0, bc_r = 0, bc_over = 0, bc_k = 0, bc_factored = 0; double bc_fact_sigma = 0.0; u64 bc_zvalid = 0, bc_act = 0;
    int *bc_rows = nullptr, *bc_info = nullptr; std::vector<int> bc_rows_h;
    double *bc_dcore = nullptr, *bc_dfact = nullptr, *bc_U = nullptr, *bc_T = nullptr, *bc_Z = nullptr, *bc_S = nullptr, *bc_SL = nullptr, *bc_t = nullptr, *bc_z0 = nullptr;
    // chain QPs with a few coupling VARIABLES (QPDO_BAND_BORDER; qdev_set_band_border before qdev_configure; dev/band.inc, the bordered
    // mode): the trailing bb_c variables (0: none, and nothing below is read) border a core of bb_ncore variables whose half-bandwidth
    // bb_bcore becomes band_b; band_np is then bb_ncore rounded up to 4.  bb_over / bb_max: a border of bb_over > bb_max columns was seen and
    // not adopted (setup's message).  C, the forward results and Z = B^-1 C: band_np x bb_c; D, S and its factor: BC_MAX x BC_MAX; t: BC_MAX.
    int bb_c = 0, bb_ncore = 0, bb_bcore = 0, bb_over = 0, bb_max = 0;
    double *bb_C = nullptr, *bb_T = nullptr, *bb_Z = nullptr, *bb_D = nullptr, *bb_S = nullptr, *bb_SL = nullptr, *bb_t = nullptr;
    // half-bandwidths BAND_MAX_B + 1 .. BAND_WIDE_MAX_B (dev/band_wide.inc): order padded to 64, w = (b + 63) / 64; the band as 64 x 64 tiles
    // (w + 1 per block column), the diagonal tiles while they are being updated, D, the diagonal blocks' inverses and their transposes
    int bw_w = 0; double *bw_Wb = nullptr, *bw_Wdiag = nullptr, *bw_Wd = nullptr, *bw_Li = nullptr, *bw_LiT = nullptr;
    double *Kd = nullptr, *Wd = nullptr, *Dg = nullptr, *Linv = nullptr, *LinvT = nullptr, *dz = nullptr, *dxw = nullptr;
    double *ch_y = nullptr, *ch_x = nullptr, *dsol = nullptr; int dense_chain = 1;
    hipStream_t stream2 = nullptr;            // dense factor look-ahead: trailing updates run here
    int dense_lookahead = -1;                 // multi-launch factor: -1 automatic (from n = 7000 up), 0 off, 1 on (QPDO_DENSE_LOOKAHEAD)
    // mid-size orders (dense_nblk <= MID_MAX_NB): the whole factorization and the forward solve in one launch (k_mid_factor, dev/mid_kernels.inc)
    int dense_mid = 1, mid_fwd_valid = 0; unsigned int *mid_flags = nullptr, mid_epoch = 0; double *mid_C = nullptr, *mid_dinv = nullptr;   // k_mid_factor: flags, the published C tiles (one per block row), 1 / D
    // low-rank factor update (Woodbury on the kept factor): see the k_wb_* kernels
    int dense_factored = 0, wb_enable = 1, wb_k = 0; double dense_fact_sigma = 0.0;
    double *d_fact = nullptr, *wb_Z = nullptr, *wb_T = nullptr, *wb_T2 = nullptr, *wb_G = nullptr, *wb_M = nullptr, *wb_v = nullptr, *wb_w = nullptr, *wb_t = nullptr;
    int *wb_slot = nullptr, *wb_rows = nullptr, *wb_cnt = nullptr;
    // in-place up/downdate of the kept factor (QPDO_DENSE_UPDOWN; dev/updown.inc): ud_cap = changed rows a pass may apply (0: off),
    // ud_dirty = the factor carries at least one up/downdate since its last full factorization (its solves are residual-checked)
    int ud_cap = 0, ud_dirty = 0; int *ud_rows = nullptr, *ud_cnt = nullptr;
    double *ud_a = nullptr, *ud_p = nullptr, *ud_q = nullptr, *ud_G = nullptr, *ud_Dn = nullptr, *ud_beta = nullptr;
    hipEvent_t evF[2] = {nullptr, nullptr}, evB[2] = {nullptr, nullptr};
    int dense_last_branch = -1; double dense_last_sigma = -1.0;
    int direct_hook_used = 0;      // qdev_direct_solve ran since the last solve: the next qdev_begin_solve drops its kept factor
    // n-vectors
    double *x, *xbar, *Qx, *Aty, *q, *df, *res_dual, *res_dual_in, *rhs, *dx, *Qdx, *Atdy, *D, *Dinv;
    double *pc_r, *pc_z, *pc_p, *pc_Kp, *pc_diag, *tmp_n;
    // m-vectors
    double *y, *ybar, *Ax, *l, *u, *mu, *isq, *w, *res_prim, *res_prim_old, *res_prim_in, *dy, *Adx, *d, *E,
        *Einv, *pc_t, *at_scale, *tmp_m;
    int *active, *active_old, *mu_changed;
    // 2m linesearch
    double *ls_delta, *ls_alpha, *ls_pa, *ls_pb;
    u64 *ls_key[2];
    u32 *ls_idx[2];
    int *rs_hist; int rs_nblocks = 0;
    double *ls_bt;           // block totals (2 * nblk)
    int ls_nblk = 0;
    // control
    Ctrl *ctrl = nullptr;    // device
    double *pack = nullptr, *hpack = nullptr;      // store_solution as one image: device staging + pinned host copy (3n + 3m + 1 doubles)
    Ctrl *hctrl = nullptr;   // pinned host
    // read-back by publication (k_ctrl_publish): the sequence words live behind the pinned blocks; 0 = hipMemcpyAsync + hipStreamSynchronize
    int ctrl_publish = 1; u64 *hseq = nullptr, *hseq2 = nullptr; u64 pub_seq = 0;
    // folded into the residual launch (k_resid_mn): the read-back's publication (ticket: the last block publishes) and the deferred step's five axpys
    unsigned int *pub_ticket = nullptr; int fuse_resid = 1, axpy_pending = 0;
    int ls_small = 1;        // 2m <= LS_SMALL_MAX: the linesearch as ONE launch (QPDO_LS_SMALL=0: the radix-sort path at every size; the same bits)
    // launch-ahead of the Newton step (qdev_residuals_ahead, host_step.inc ahead_enqueue_step): QPDO_LAUNCH_AHEAD=0 switches it off
    int launch_ahead = 1, ahead_inflight = 0, ahead_branch = -1; double ahead_sigma_f02 = 0.0; int64_t ahead_spmv_calls0 = 0, ahead_spmv_bytes0 = 0;
    int tail_shift = 0, tail_muchg = 0, tail_sigma = 0; double tail_dsig = 0.0;      // parts of an outer update's tail waiting for their one launch (k_outer_tail)
    int fuse_outer = 1;      // the outer-update sequences in 4 + 8 launches instead of 8 + 13 (QPDO_FUSE_OUTER=0: the separate kernels)
    // Schur-complement mode of the PCG (pcg_solve): inner CG on S' = D^-1 + A_c Dq^-1 A_c' with its own control block
    Ctrl *ctrl2 = nullptr, *hctrl2 = nullptr; double *part2 = nullptr;
    double *s_x = nullptr, *s_r = nullptr, *s_z = nullptr, *s_p = nullptr, *s_Sp = nullptr, *s_diag = nullptr, *s_v = nullptr, *s_s = nullptr;
    int kg = 0;                                                           // row-partitioned Schur mode: global number of weighted rows (k-vectors stay partitioned)
    // Schur mode, inner solve (host_pcg.inc schur_inner_solve).  inner_refine (QPDO_PCG_INNER_REFINE, default 1): the CG streams the fp32 copies
    // and the solve is accepted on the residual formed with the fp64 matrices; inner_f32 (QPDO_PCG_INNER_F32=1): ONE fp32 CG solve, unverified
    int inner_refine = 1, refine_maxsweep = 6; double refine_theta = 0.8; double *s_acc = nullptr, *s_sol = nullptr;
    // inner_x32 (QPDO_INNER_X32, default 1): the fp32 CG also stages fp32 copies of its operand vectors (s_z32 of s_z, tmp_n32 of tmp_n) and
    // walks the column slabs in pairs (spmv.inc, XT = float); 0: fp64 operands, slab by slab
    int inner_x32 = 1; float *s_z32 = nullptr, *tmp_n32 = nullptr;
    // inner_h16 (QPDO_INNER_H16, default 1; off with QPDO_INNER_X32=0): the first h16_maxsweep sweeps (QPDO_INNER_H16_MAXSWEEP) of a refined
    // inner solve are COARSE: the CG streams the half-precision images (DevCsr::vsm16) and stops at max(theta tau ||b||, h16_eta ||rho||)
    // (QPDO_INNER_H16_ETA).  h16_set: the images' scale 2^h16_e is valid -- max |a_ij| 2^h16_e lies in [2^14, 2^15), taken over A where its
    // values are set (h16_refresh_scale: setup, qpdo_amd_update_matrices); a maximum of 0, inf or NaN leaves the coarse sweeps off.
    // h16_scale = 2^h16_e (0: the builders write no half-precision values)
    int inner_h16 = 1, h16_maxsweep = 2, h16_set = 0, h16_e = 0; double h16_eta = 1e-3, h16_scale = 0.0;
    static const int SWEEP_MEMORY = 8; int sweep_last_inner[SWEEP_MEMORY] = {0, 0, 0, 0, 0, 0, 0, 0};      // as schur_last_inner, per sweep index from 1 on
    int inner_f32 = 0; int inner_fold = 1 /* the inner CG's vector step inside its two products (QPDO_INNER_FOLD=0: k_cgcg_step) */; int schur_mode = -1 /* -1 auto, 0 off, 1 on */, schur_off = 0, schur_strikes = 0, last_jacobi_iters = 0, schur_last_inner = 0; long long schur_passes = 0;
    double *part = nullptr;  // P_COUNT * PGRID
    // scaling
    int scaled = 0; double sc_c = 1.0, sc_cinv = 1.0;
    // factor state
    double sigma_f = 0.0;
    // config
    int linsolve = 0; double pcg_tol = 1e-12; int pcg_maxit = 100000; int pcg_batch = 16; int pcg_graph = 1;
    double pcg_abs = 1e-11, pcg_abs_now = -1.0, pcg_abs_factor = 1e-5;      // absolute stopping rule of the Newton solves: pcg_abs = pcg_abs_factor * eps_abs (qdev_set_eps_abs)
    // stats
    QdevStats st{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ev_spmv_ms = 0.0; long long ev_spmv_n = 0;
    double ev_ac_ms = 0.0, ev_ac_bytes = 0.0; long long ev_ac_n = 0;      // sampled A_c products of the Schur mode's inner solve
    // pinned staging for large host -> device uploads (h2d_staged): owned by the workspace, released when setup ends
    char *pin[2] = {nullptr, nullptr}; hipEvent_t pin_ev[2] = {nullptr, nullptr}; bool pin_used[2] = {false, false}; bool pin_failed = false;
    std::vector<void *> allocs;
    // qpdo_amd_update_matrices (dev/host_update.inc).  raw*: the caller's unscaled values (a scaled workspace: kept by qdev_keep_raw_values at
    // setup, so that a matrix passed as NULL is scaled again from its own values); map*: built by the first call that needs them
    double *rawA = nullptr, *rawQ = nullptr;      // CSC order of A (= At), the full storage of Q (= Qf)
    u32 *mapA = nullptr, *mapQ = nullptr;         // mapA[k]: CSC position of entry k of CSR(A); mapQ[k]: the caller's position of entry k of Qf
    double *qstage = nullptr;                     // the caller's stored Q values (stype +-1), gathered through mapQ
    std::vector<long long> upd_Ap, upd_Qp;        // column pointers whose pattern passed the device check (later calls compare these)
    // qpdo_amd_adjoint (dev/adjoint.inc): the call's own work vectors (6 n + 7 m doubles and m flags, allocated by the first call), the
    // per-entry outputs (allocated by the first call that asks for them) and its counters
    double *adj_n = nullptr, *adj_m = nullptr, *adj_dA = nullptr, *adj_dQ = nullptr; int *adj_flag = nullptr;
    QdevAdjointStats adj{};
    // qpdo_amd_tangent (dev/adjoint.inc) shares those work vectors; its own: the staging of one right-hand side's tq, tl, tu, tQx, tAx (each
    // allocated by the first call that passes the array) and its counters
    double *tan_q = nullptr, *tan_l = nullptr, *tan_u = nullptr, *tan_Q = nullptr, *tan_A = nullptr;
    QdevTangentStats tan{};
    // the group path of the two calls (dev/adjoint.inc adj_sweeps_group): rhs_group_cfg right-hand sides go through every launch of the sweep
    // loop at once (QPDO_AMD_RHS_GROUP at setup; the rule that makes it 1: qdev_rhs_group).  The group's vectors -- rhs_group_cfg copies of the
    // per-right-hand-side work vectors, the solve's columns, the group control array and its pinned host copy -- are allocated by the first
    // call with nrhs > 1 on a workspace whose group size is above 1 and booked in grp.scratch_bytes alone.
    int rhs_group_cfg = 8;
    double *grp_n = nullptr, *grp_m = nullptr, *grp_sol = nullptr;
    AdjGrpCtrl *grp_ctrl = nullptr, *grp_hctrl = nullptr;
    QdevGroupStats grp{};
    // what qdev_configure decided; a solve may change these (fallbacks, hybrid), qpdo_amd_update_matrices puts them back
    struct { int linsolve, dense_chain, dense_mid, dense_lookahead, wb_enable, ud_cap, deflate, pcg_maxit, band_b, bc_r; } cfg{};
};

