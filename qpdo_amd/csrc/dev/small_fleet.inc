// small_fleet.inc -- a resident FLEET of small QPs (qpdo_amd_fleet_*, include/qpdo_amd_ext.h; part of qpdo_small.hip's translation unit).
// The many-item form of one small workspace: the matrices of all items are converted, uploaded and scaled ONCE (k_small_fleet_setup:
// small_scale of the fused kernel, one workgroup per item); every item keeps a SmallRes record in device memory -- its scaling vectors,
// its cost scaling c, the state vectors qpdo_warm_start leaves behind, x / Qx of the last solve -- and a control step is
//   update      k_small_fleet_update   qpdo_update_bounds then qpdo_update_q of every item that has an entry (qpdo.c:522-586)
//   warm start  k_small_fleet, op 1/2  the shared solve body in mode 1 (qpdo.c:217-299)
//   solve       k_small_fleet, op 0    the shared solve body from the item's state (mode 2), or from zero (mode 0)
//   new Q / A   k_small_fleet_matrices the new values into the item's three CSR images, then the item's setup again (flag MATRIX_UPDATES)
// each ONE launch for the whole fleet, in the oracle's operation order: item i carries the bits of a workspace of its own.  The *_dev calls
// put a gather (k_small_fleet_gather, k_small_fleet_gather_matrices) in front of the same kernels and a scatter behind the solve.

// What qpdo_setup leaves behind for the item's unscaled matrices, q, l, u, everything but tpos (a function of the pattern): the state zeroed,
// Ruiz + cost scaling, the record of a fresh workspace.  ONE copy, for create (k_small_fleet_setup) and for new matrix values
// (k_small_fleet_matrices).  The last solve's outputs and whether they are finite (last_finite) are not part of a workspace and stay.
__device__ void small_fleet_item_setup(SmallQP &Pg, SmallQP &P, SmallRes *R, const QPDOSettings &st, double *sm) {
    const int n = P.n, m = P.m;
    FOR_T(j, n) { R->state_x[j] = 0.0; R->state_Qx[j] = 0.0; R->st_xbar[j] = 0.0; R->st_Aty[j] = 0.0; }
    FOR_T(i, m) { R->st_y[i] = 0.0; R->st_ybar[i] = 0.0; R->st_Ax[i] = 0.0; R->st_mu[i] = 0.0; R->st_isq[i] = 0.0; }
    SYNC;
    double c = 1.0, cinv = 1.0;
    if (st.scaling > 0)
        small_scale(P, (int)st.scaling, const_cast<double *>(R->rD), const_cast<double *>(R->rDinv), const_cast<double *>(R->rE), const_cast<double *>(R->rEinv),
                    P.nv + (size_t)NV_T * n, P.mv + (size_t)MV_T * m, c, cinv, sm);
    if (threadIdx.x == 0) {
        R->r_c = c; R->r_cinv = cinv; R->mode = 0; R->sigma_end = st.sigma_init; R->tau_end = 0.0; R->ws_objective = 0.0;
        R->fleet_status = QPDO_UNSOLVED;
        small_status(Pg.info, QPDO_UNSOLVED);
    }
}
// Ruiz + cost scaling of every item, tpos, the state zeroed: what k_small_solve has after its own scaling phase, left in the item's arrays
__global__ __launch_bounds__(SM_THREADS) void k_small_fleet_setup(SmallQP *probs, int count, QPDOSettings st) {
    __shared__ double sm[32];
    if ((int)blockIdx.x >= count) return;
    SmallQP &Pg = probs[blockIdx.x];
    SmallQP P = Pg;
    SmallRes *R = Pg.res;
    small_build_tpos(P);
    if (R->raw_q) {                                 // MATRIX_UPDATES: the unscaled q, l, u and (scaling rounds: it cannot be undone bit for bit) matrix values
        const int n = P.n, m = P.m;
        FOR_T(j, n) R->raw_q[j] = P.q[j];
        FOR_T(i, m) { R->raw_l[i] = P.l[i]; R->raw_u[i] = P.u[i]; }
        if (st.scaling > 0) {
            const int nnzA = P.Trp[n], nnzQ = P.Qrp[n];
            FOR_T(k, nnzA) R->rawA[k] = P.Tval[k];
            FOR_T(k, nnzQ) R->rawQ[k] = P.Qval[k];
        }
    }
    small_fleet_item_setup(Pg, P, R, st, sm);
}
// New values of Q and / or A in the create-time pattern for item i when tab[2 i] / tab[2 i + 1] name an offset into `stage` (-1: no entry;
// neither: the workgroup leaves).  Q arrives as the caller's stored values, A as its CSC values = the value array of CSR(A').  A matrix that
// is not passed is restored from its unscaled copy (scaling 0: the values in place are the unscaled ones), q, l, u from theirs, and the
// item is set up as at create: afterwards it holds what qpdo_setup leaves for these inputs.
__global__ __launch_bounds__(SM_THREADS) void k_small_fleet_matrices(SmallQP *probs, int count, QPDOSettings st, const int *tab, const double *stage) {
    __shared__ double sm[32];
    if ((int)blockIdx.x >= count) return;
    const int oQ = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.x]), oA = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.x + 1]);
    if (oQ < 0 && oA < 0) return;
    SmallQP &Pg = probs[blockIdx.x];
    SmallQP P = Pg;
    SmallRes *R = Pg.res;
    const int n = P.n, m = P.m, nnzA = P.Trp[n], nnzQ = P.Qrp[n];
    const int scaled = st.scaling > 0;
    if (oA >= 0) { const double *an = stage + oA; double *rawA = R->rawA; FOR_T(k, nnzA) { const double v = an[k]; P.Tval[k] = v; if (scaled) rawA[k] = v; } }
    else if (scaled) { const double *rawA = R->rawA; FOR_T(k, nnzA) P.Tval[k] = rawA[k]; }
    if (oQ >= 0) {
        const double *qn = stage + oQ; const int *mapQ = R->mapQ; double *rawQ = R->rawQ;
        FOR_T(k, nnzQ) { const double v = qn[mapQ ? mapQ[k] : k]; P.Qval[k] = v; if (scaled) rawQ[k] = v; }
    } else if (scaled) { const double *rawQ = R->rawQ; FOR_T(k, nnzQ) P.Qval[k] = rawQ[k]; }
    FOR_T(j, n) P.q[j] = R->raw_q[j];
    FOR_T(i, m) { P.l[i] = R->raw_l[i]; P.u[i] = R->raw_u[i]; }
    SYNC;
    if (oA >= 0 || scaled) { const int *mapA = R->mapA; FOR_T(k, nnzA) P.Aval[k] = P.Tval[mapA[k]]; }
    small_fleet_item_setup(Pg, P, R, st, sm);       // (its first barrier orders the stores above before the scaling reads them)
}
// qpdo_update_bounds (qpdo.c:522-544), then qpdo_update_q (qpdo.c:549-586) of item i when tab[4 i + 1] / [4 i + 2] (l, u) or tab[4 i] (q) name
// an offset into `stage` (-1: no entry).  The two commute: bounds touch l, u and read E only.  The c / c_old rescale of Q's values and of Qx, the
// exact inf-norm and every product in the oracle's order (oracle_update_q).
__global__ __launch_bounds__(SM_THREADS) void k_small_fleet_update(SmallQP *probs, int count, QPDOSettings st, const int *tab, const double *stage) {
    __shared__ double sm[32];
    if ((int)blockIdx.x >= count) return;
    const int oq = __builtin_amdgcn_readfirstlane(tab[4 * blockIdx.x]), ol = __builtin_amdgcn_readfirstlane(tab[4 * blockIdx.x + 1]),
              ou = __builtin_amdgcn_readfirstlane(tab[4 * blockIdx.x + 2]);
    if (oq < 0 && ol < 0 && ou < 0) return;
    SmallQP &Pg = probs[blockIdx.x];
    SmallRes *R = Pg.res;
    const int n = Pg.n, m = Pg.m;
    const int scaled = st.scaling > 0, prox = (int)st.proximal;
    const double *E = R->rE, *D = R->rD;
    if (R->raw_q) {                                 // MATRIX_UPDATES: the unscaled vectors a later k_small_fleet_matrices sets the item up from
        if (oq >= 0) { const double *qn = stage + oq; double *rq = R->raw_q; FOR_T(j, n) rq[j] = qn[j]; }
        if (ol >= 0) { const double *ln = stage + ol; double *rl = R->raw_l; FOR_T(i, m) rl[i] = ln[i]; }
        if (ou >= 0) { const double *un = stage + ou; double *ru = R->raw_u; FOR_T(i, m) ru[i] = un[i]; }
    }
    if (ol >= 0) { const double *ln = stage + ol; double *l = Pg.l; FOR_T(i, m) l[i] = scaled ? E[i] * ln[i] : ln[i]; }
    if (ou >= 0) { const double *un = stage + ou; double *u = Pg.u; FOR_T(i, m) u[i] = scaled ? E[i] * un[i] : un[i]; }
    if (oq < 0) return;
    const double *qn = stage + oq;
    double *q = Pg.q, *x = R->state_x, *Qx = R->state_Qx;
    if (!scaled) { FOR_T(j, n) q[j] = qn[j]; return; }
    const double c_old = R->r_c, cinv_old = R->r_cinv, sigma = R->sigma_end;
    double mx = 0.0;
    FOR_T(j, n) {                                    // (entry j of every vector belongs to this thread throughout)
        const double qj = D[j] * qn[j];
        q[j] = qj;
        double qx = Qx[j];
        if (prox) { qx = qx + (-sigma) * x[j]; Qx[j] = qx; }
        const double t = s_abs(qj + cinv_old * qx);
        mx = t > mx ? t : mx;
    }
    const double nrm = blk_max(mx, sm);              // (its barriers: every thread has read c_old before lane 0 writes the new one)
    const double c = 1 / s_max(1.0, nrm), cinv = 1 / c;
    const double f = c / c_old;
    FOR_T(j, n) {
        q[j] *= c;
        double qx = Qx[j] * f;
        if (prox) qx = qx + st.sigma_init * x[j];
        Qx[j] = qx;
    }
    const int nnzQ = Pg.Qrp[n];
    double *Qval = Pg.Qval;
    FOR_T(k, nnzQ) Qval[k] *= f;
    if (threadIdx.x == 0) { R->r_c = c; R->r_cinv = cinv; if (prox) R->sigma_end = st.sigma_init; }
}

// ---- device-resident inputs and outputs (qpdo_amd_fleet_*_dev): the caller's PACKED arrays -- the n-vectors of all items back to back, item
// i at offs[i], the m-vectors at offs[count + 1 + i]; offs[count] = N and offs[2 count + 1] = M are the totals -- on one side, the staging and
// the call table that the kernels above and k_small_fleet op 1 already read on the other.  One workgroup per item, 8-byte accesses that
// are contiguous over the lanes, the item's offsets in scalar registers.
#define FLEET_IO_THREADS 256
#define FLEET_REC_NONE 2147483647                   // rec[1] while no item was refused
// kind 0, an update: a0 = q (mask bit 0), a1 = l (bit 1), a2 = u (bit 2).  kind 1, a warm start: a0 = x0 (bit 0), a1 = y0 (bit 1), a2 = NULL.
// A vector of the item is TAKEN when its array is passed and its mask bit is set (mask NULL: all set): it is copied to the fixed place
// stage[offs n | N + offs m | N + M + offs m] and the item's table entry names that place; the others get -1, which the consumers read as
// "unchanged" (update) or "from zero" (warm start).  An update item with l and u both taken and l > u somewhere is REFUSED: the table
// entry says -1, -1, -1 -- q included, the item is not touched --, rec[0] counts it and rec[1] keeps the smallest such item.  The test
// completes (a block-wide OR) before the table is written; what a refused item left in the staging is never read.
__global__ __launch_bounds__(FLEET_IO_THREADS) void k_small_fleet_gather(int count, const int *offs, int kind, const double *a0, const double *a1, const double *a2,
                                                                         const int *mask, int *tab, double *stage, int *rec) {
    if ((int)blockIdx.x >= count) return;
    const int b = blockIdx.x;
    const int no = __builtin_amdgcn_readfirstlane(offs[b]), n = __builtin_amdgcn_readfirstlane(offs[b + 1]) - no;
    const int mo = __builtin_amdgcn_readfirstlane(offs[count + 1 + b]), m = __builtin_amdgcn_readfirstlane(offs[count + 2 + b]) - mo;
    const int N = __builtin_amdgcn_readfirstlane(offs[count]), M = __builtin_amdgcn_readfirstlane(offs[2 * count + 1]);
    const int mk = mask ? __builtin_amdgcn_readfirstlane(mask[b]) : 7;
    const int t0 = a0 && (mk & 1), t1 = a1 && (mk & 2), t2 = a2 && (mk & 4);
    const int s0 = no, s1 = N + mo, s2 = N + M + mo;
    if (t0) { const double *src = a0 + no; double *dst = stage + s0; FOR_T(j, n) dst[j] = src[j]; }
    int bad = 0;
    if (t1 && t2) {
        const double *ls = a1 + mo, *us = a2 + mo; double *ld = stage + s1, *ud = stage + s2;
        FOR_T(i, m) { const double lv = ls[i], uv = us[i]; ld[i] = lv; ud[i] = uv; bad |= lv > uv; }
    } else {
        if (t1) { const double *src = a1 + mo; double *dst = stage + s1; FOR_T(i, m) dst[i] = src[i]; }
        if (t2) { const double *src = a2 + mo; double *dst = stage + s2; FOR_T(i, m) dst[i] = src[i]; }
    }
    bad = kind == 0 ? __syncthreads_or(bad) : 0;
    if (threadIdx.x == 0) {
        int *t = tab + 4 * b;
        t[0] = (t0 && !bad) ? s0 : -1; t[1] = (t1 && !bad) ? s1 : -1; t[2] = (t2 && !bad) ? s2 : -1; t[3] = 0;
        if (bad) { atomicAdd(rec, 1); atomicMin(rec + 1, b); }
    }
}
// The matrix counterpart (qpdo_amd_fleet_update_matrices_dev): the caller's PACKED value arrays -- the stored values of all items' Q back to
// back, item i at offs[i], the CSC values of all items' A, item i at offs[count + 1 + i]; offs[count] = NQ and offs[2 count + 1] = NA are the
// totals -- on one side, the matrix staging and the two-int table that k_small_fleet_matrices already reads on the other.  Bit 0 of the mask:
// the item takes Q, bit 1: A (mask NULL: both).  A matrix of the item is TAKEN when its array is passed and its bit is set: it is copied to
// the fixed place stage[offs q | NQ + offs a] and the table entry names that place -- also for a matrix without a stored entry, where the
// place is a valid offset and nothing is copied (the consumer's test is >= 0) --; the other gets -1, "unchanged".
__global__ __launch_bounds__(FLEET_IO_THREADS) void k_small_fleet_gather_matrices(int count, const int *offs, const double *Qx, const double *Ax, const int *mask,
                                                                                  int *tab, double *stage) {
    if ((int)blockIdx.x >= count) return;
    const int b = blockIdx.x;
    const int qo = __builtin_amdgcn_readfirstlane(offs[b]), nq = __builtin_amdgcn_readfirstlane(offs[b + 1]) - qo;
    const int ao = __builtin_amdgcn_readfirstlane(offs[count + 1 + b]), na = __builtin_amdgcn_readfirstlane(offs[count + 2 + b]) - ao;
    const int NQ = __builtin_amdgcn_readfirstlane(offs[count]);
    const int mk = mask ? __builtin_amdgcn_readfirstlane(mask[b]) : 3;
    const int tQ = Qx && (mk & 1), tA = Ax && (mk & 2);
    const int sQ = qo, sA = NQ + ao;
    if (tQ) { const double *src = Qx + qo; double *dst = stage + sQ; FOR_T(k, nq) dst[k] = src[k]; }
    if (tA) { const double *src = Ax + ao; double *dst = stage + sA; FOR_T(k, na) dst[k] = src[k]; }
    if (threadIdx.x == 0) { int *t = tab + 2 * b; t[0] = tQ ? sQ : -1; t[1] = tA ? sA : -1; }
}
// After k_small_fleet op 0: what qpdo_amd_fleet_solve delivers for item i, into the caller's packed arrays (a NULL array is not wanted).  x, y:
// NaN at status -3 / -4; prim_inf_cert (m): the item's dy at -3, dual_inf_cert (n): its dx at -4, NaN otherwise (the rule of the reference's
// mex gateway); status: status_val, iterations, oterations; norms: res_prim, res_dual, res_prim_in, res_dual_in, objective.
__global__ __launch_bounds__(FLEET_IO_THREADS) void k_small_fleet_scatter(const SmallQP *probs, int count, const int *offs, double *x, double *y, long *status,
                                                                          double *norms, double *prim_inf_cert, double *dual_inf_cert) {
    if ((int)blockIdx.x >= count) return;
    const int b = blockIdx.x;
    const SmallQP &Pg = probs[b];
    const int no = __builtin_amdgcn_readfirstlane(offs[b]), n = __builtin_amdgcn_readfirstlane(offs[b + 1]) - no;
    const int mo = __builtin_amdgcn_readfirstlane(offs[count + 1 + b]), m = __builtin_amdgcn_readfirstlane(offs[count + 2 + b]) - mo;
    const int stv = __builtin_amdgcn_readfirstlane((int)Pg.info.status_val);
    const int pinf = stv == QPDO_PRIMAL_INFEASIBLE, dinf = stv == QPDO_DUAL_INFEASIBLE, infeasible = pinf || dinf;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);      // the bits of the host's NAN
    if (x) { const double *src = uni_ptr(Pg.sol_x); double *dst = x + no; FOR_T(j, n) dst[j] = infeasible ? nan : src[j]; }
    if (y) { const double *src = uni_ptr(Pg.sol_y); double *dst = y + mo; FOR_T(i, m) dst[i] = infeasible ? nan : src[i]; }
    if (prim_inf_cert) { const double *src = uni_ptr(Pg.cert_dy); double *dst = prim_inf_cert + mo; FOR_T(i, m) dst[i] = pinf ? src[i] : nan; }
    if (dual_inf_cert) { const double *src = uni_ptr(Pg.cert_dx); double *dst = dual_inf_cert + no; FOR_T(j, n) dst[j] = dinf ? src[j] : nan; }
    if (threadIdx.x == 0) {
        if (status) { long *s = status + 3 * (size_t)b; s[0] = Pg.info.status_val; s[1] = Pg.info.iterations; s[2] = Pg.info.oterations; }
        if (norms) {
            double *v = norms + 5 * (size_t)b;
            v[0] = Pg.info.res_prim_norm; v[1] = Pg.info.res_dual_norm; v[2] = Pg.info.res_prim_in_norm; v[3] = Pg.info.res_dual_in_norm; v[4] = Pg.info.objective;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct FleetItem { int n, m; size_t o_q, o_l, o_u, o_solx, o_soly, o_dx, o_dy, out_off; };
// MATRIX_UPDATES: the create-time CSC pattern of an item's A and stored Q (host copies: every update_matrices call is compared against them in full)
struct FleetPattern { size_t Anrow = 0, Ancol = 0, Qnrow = 0, Qncol = 0; int Qstype = 0; std::vector<int> Ap, Ai, Qp, Qi; };
static const int FLEET_RHS_GROUP = 8;                 // one right-hand side per wave of the workgroup
struct SmallFleet {
    int device = 0; long count = 0; QPDOSettings st;
    hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    char *arena = nullptr;                          // [matrices + q, l, u of all items][outputs of all items][records' vectors][scratch]
    SmallQP *dprobs = nullptr; SmallRes *dres = nullptr;
    double *dstage = nullptr; int *dtab = nullptr;  // a call's vectors and its per-item table (QPDO_AMD_FLEET_TABLE_BYTES each)
    char *hstage = nullptr; size_t stage_doubles = 0;       // pinned: [vectors][table]
    char *hout = nullptr; size_t out_off = 0, out_bytes = 0;  // pinned image of the outputs
    SmallQP *hp = nullptr;                          // pinned image of the descriptors (info comes back in them)
    std::vector<FleetItem> it;
    size_t lds = 0; int kflags = 0, layout = 0;
    long matrix_bytes = 0, vector_bytes_last = 0, solve_launches = 0, solves = 0; double kernel_s = 0.0;
    bool solved = false;
    // QPDO_AMD_FLEET_MATRIX_UPDATES (all empty / zero without the flag)
    long flags = 0;
    std::vector<FleetPattern> pat;
    char *dmstage = nullptr, *hmstage = nullptr;    // a matrix call's [table: 2 ints per item][values], device and pinned
    size_t mstage_doubles = 0;
    long m_calls = 0, m_items_last = 0, m_bytes_last = 0, m_extra_bytes = 0; double m_kernel_s = 0.0;
    int *dmoffs = nullptr;                          // the packed value layout [qoff: count + 1][aoff: count + 1] of update_matrices_dev
    std::vector<long> qoff, aoff;
    // device-resident inputs and outputs (the *_dev calls; DESIGN.md 3.6)
    hipEvent_t ev_chain = nullptr;                  // recorded at the end of every fleet call on the stream it used; the next call's stream waits for it
    int *doffs = nullptr, *drec = nullptr;          // the packed layout [noff: count + 1][moff: count + 1], then the refusal record {items, smallest item}
    int *hrec = nullptr;                            // pinned: the record as qdev_small_fleet_sync reads it
    std::vector<long> noff, moff;
    long d_updates = 0, d_warm_starts = 0, d_solves = 0;
    bool timing_pending = false;                    // ev0 / ev1 bracket a device solve whose duration has not been read yet
    // QPDO_AMD_FLEET_ADJOINT: the most recent state-changing call was a solve (the resident q, l, u and matrices belong to the x, y it returned)
    bool last_was_solve = false;
    long adjoint_calls = 0;
    int rhs_group = 1; double *sens_scratch = nullptr; long sens_scratch_bytes = 0;     // k_small_fleet_sens: G, and its slots (allocated at the first call that needs them)
    long sens_calls = 0, sens_rhs = 0;              // adjoint_multi_dev + tangent_dev calls that launched, and their right-hand sides
};
// Ordering between the streams the fleet is driven on, its own included: ONE event.  Every call makes its stream wait for what the previous
// call recorded and records again behind its last operation, so host and device calls mix freely and the caller may change streams.
static hipError_t fleet_enter(SmallFleet *F, hipStream_t s) { return hipStreamWaitEvent(s, F->ev_chain, 0); }
static hipError_t fleet_leave(SmallFleet *F, hipStream_t s) { return hipEventRecord(F->ev_chain, s); }
static void fleet_free(SmallFleet *F) {
    if (!F) return;
    (void)hipSetDevice(F->device);
    if (F->stream) (void)hipStreamSynchronize(F->stream);
    if (F->arena) (void)hipFree(F->arena);
    if (F->dprobs) (void)hipFree(F->dprobs);
    if (F->dres) (void)hipFree(F->dres);
    if (F->dstage) (void)hipFree(F->dstage);
    if (F->doffs) (void)hipFree(F->doffs);
    if (F->hrec) (void)hipHostFree(F->hrec);
    if (F->ev_chain) (void)hipEventDestroy(F->ev_chain);
    if (F->dmstage) (void)hipFree(F->dmstage);
    if (F->dmoffs) (void)hipFree(F->dmoffs);
    if (F->sens_scratch) (void)hipFree(F->sens_scratch);
    if (F->hmstage) (void)hipHostFree(F->hmstage);
    if (F->hstage) (void)hipHostFree(F->hstage);
    if (F->hout) (void)hipHostFree(F->hout);
    if (F->hp) (void)hipHostFree(F->hp);
    if (F->ev0) (void)hipEventDestroy(F->ev0);
    if (F->ev1) (void)hipEventDestroy(F->ev1);
    if (F->stream) (void)hipStreamDestroy(F->stream);
    delete F;
}

extern "C" {

void qdev_small_fleet_destroy(void *h) { fleet_free((SmallFleet *)h); }

// data: `count` QPDOData pointers, every item already checked (qdev_small_eligible, validate_data).  Converts, uploads and scales; NULL on
// failure with qdev_small_last_error() set and nothing left allocated.
void *qdev_small_fleet_create(int device, long count, const void *const *data_, const void *settings_, long flags) {
    int rc = 0;
    std::atomic<int> conv_failed{0};
    const bool mu = (flags & QPDO_AMD_FLEET_MATRIX_UPDATES) != 0;
    struct MatLay { size_t mapA = 0, mapQ = 0, rq = 0, rl = 0, ru = 0, rawA = 0, rawQ = 0; bool has_mapQ = false; };
    std::vector<MatLay> ml(mu ? (size_t)count : 0);
    size_t extra = 0, mstage = 0;
    const QPDOData *const *data = (const QPDOData *const *)data_;
    SmallFleet *F = new SmallFleet();
    F->device = device; F->count = count; F->st = *(const QPDOSettings *)settings_; F->flags = flags;
    F->it.resize((size_t)count);
    std::vector<Lay> lay((size_t)count);
    std::vector<SmallQP> hp((size_t)count);
    std::vector<SmallRes> hr((size_t)count);
    std::vector<size_t> o_rec((size_t)count);
    std::vector<int> hoffs(2 * ((size_t)count + 1) + 2);        // the packed layout and the empty refusal record, as uploaded
    std::vector<int> hmoffs(mu ? 2 * ((size_t)count + 1) : 0);  // MATRIX_UPDATES: the packed value layout, as uploaded
    char *h = nullptr;
    size_t total = 0, nmax = 1, mmax = 0, stage = 0;
    auto reserve = [&](size_t bytes) { size_t o = total; total += (bytes + 255) & ~(size_t)255; return o; };
    auto reserve_extra = [&](size_t bytes) { const size_t o = reserve(bytes); extra += total - o; return o; };
    parallel_items(count, [&](long i) { const QPDOData *d = data[i]; Lay &L = lay[(size_t)i]; L.nnzA = (size_t)idx_at(d->A->p, d->A->itype, (long long)d->A->ncol); L.nnzQ = (size_t)sym_full_nnz(d->Q); });
    for (long i = 0; i < count; i++) {
        const QPDOData *d = data[i]; Lay &L = lay[(size_t)i];
        const size_t n = d->n, m = d->m;
        lay_inputs(L, n, m, reserve);
        if (n > nmax) nmax = n;
        if (m > mmax) mmax = m;
        stage += n + 2 * m;                          // the largest call: q, l and u of every item
        F->noff.push_back(F->noff.empty() ? 0 : F->noff.back() + (long)data[i - 1]->n);
        F->moff.push_back(F->moff.empty() ? 0 : F->moff.back() + (long)data[i - 1]->m);
        if (mu) {                                    // the maps ride in create's upload
            MatLay &X = ml[(size_t)i];
            X.mapA = reserve_extra(L.nnzA * 4 + 4);
            X.has_mapQ = d->Q->stype != 0;
            if (X.has_mapQ) X.mapQ = reserve_extra(L.nnzQ * 4 + 4);
            const size_t storedQ = (size_t)idx_at(d->Q->p, d->Q->itype, (long long)d->Q->ncol);
            mstage += L.nnzA + storedQ;              // the largest call: every stored entry of every Q and A
            if (i == 0) { F->qoff.push_back(0); F->aoff.push_back(0); }
            F->qoff.push_back(F->qoff.back() + (long)storedQ); F->aoff.push_back(F->aoff.back() + (long)L.nnzA);
        }
    }
    if (mstage >= 2147483647ULL) { snprintf(s_err, sizeof(s_err), "fleet: %zu matrix entries per call exceed the 2^31 the call table can address; split the fleet", mstage); delete F; return nullptr; }
    // (a call's table holds 32-bit offsets, in doubles, into the staging of the whole fleet)
    if (stage >= 2147483647ULL) { snprintf(s_err, sizeof(s_err), "fleet: %zu vector elements per call exceed the 2^31 the call table can address; split the fleet", stage); delete F; return nullptr; }
    F->noff.push_back(F->noff.back() + (long)data[count - 1]->n); F->moff.push_back(F->moff.back() + (long)data[count - 1]->m);
    for (long i = 0; i <= count; i++) { hoffs[(size_t)i] = (int)F->noff[(size_t)i]; hoffs[(size_t)(count + 1 + i)] = (int)F->moff[(size_t)i]; }    // (N + 2 M = stage < 2^31)
    hoffs[2 * ((size_t)count + 1)] = 0; hoffs[2 * ((size_t)count + 1) + 1] = FLEET_REC_NONE;
    if (mu) for (long i = 0; i <= count; i++) { hmoffs[(size_t)i] = (int)F->qoff[(size_t)i]; hmoffs[(size_t)(count + 1 + i)] = (int)F->aoff[(size_t)i]; }  // (NQ + NA = mstage < 2^31)
    const size_t upload_bytes = total;
    for (long i = 0; i < count; i++) {
        const QPDOData *d = data[i]; Lay &L = lay[(size_t)i];
        lay_outputs(L, d->n, d->m, reserve);
    }
    const size_t out_bytes = total - upload_bytes;
    for (long i = 0; i < count; i++) {
        const QPDOData *d = data[i]; Lay &L = lay[(size_t)i];
        const size_t n = d->n, m = d->m;
        o_rec[(size_t)i] = reserve((6 * n + 7 * m) * 8 + 8);          // D, Dinv, x, Qx, xbar, A'y | E, Einv, y, ybar, Ax, mu, 1/sqrt(mu)
        lay_scratch(L, n, m, reserve);
        if (mu) {
            MatLay &X = ml[(size_t)i];
            X.rq = reserve_extra(n * 8); X.rl = reserve_extra(m * 8 + 8); X.ru = reserve_extra(m * 8 + 8);
            if (F->st.scaling > 0) { X.rawA = reserve_extra(L.nnzA * 8 + 8); X.rawQ = reserve_extra(L.nnzQ * 8 + 8); }
        }
    }
    SHIP(hipSetDevice(device));
    SHIP(hipStreamCreateWithFlags(&F->stream, hipStreamNonBlocking));
    SHIP(hipEventCreate(&F->ev0)); SHIP(hipEventCreate(&F->ev1));
    SHIP(hipEventCreateWithFlags(&F->ev_chain, hipEventDisableTiming));
    SHIP(hipMalloc((void **)&F->doffs, hoffs.size() * sizeof(int)));
    F->drec = F->doffs + 2 * ((size_t)count + 1);
    SHIP(hipHostMalloc((void **)&F->hrec, 2 * sizeof(int), hipHostMallocDefault));
    SHIP(hipMalloc((void **)&F->arena, total));
    SHIP(hipMalloc((void **)&F->dprobs, (size_t)count * sizeof(SmallQP)));
    SHIP(hipMalloc((void **)&F->dres, (size_t)count * sizeof(SmallRes)));
    F->stage_doubles = stage;
    SHIP(hipMalloc((void **)&F->dstage, stage * 8 + (size_t)count * QPDO_AMD_FLEET_TABLE_BYTES + 16));
    F->dtab = (int *)(F->dstage + stage);
    SHIP(hipHostMalloc((void **)&F->hstage, stage * 8 + (size_t)count * QPDO_AMD_FLEET_TABLE_BYTES + 16, hipHostMallocDefault));
    if (mu) {
        const size_t mbytes = (size_t)count * QPDO_AMD_FLEET_MATRIX_TABLE_BYTES + mstage * 8 + 16;
        F->mstage_doubles = mstage;
        SHIP(hipMalloc((void **)&F->dmstage, mbytes));
        SHIP(hipHostMalloc((void **)&F->hmstage, mbytes, hipHostMallocDefault));
        SHIP(hipMalloc((void **)&F->dmoffs, hmoffs.size() * sizeof(int)));
        F->m_extra_bytes = (long)(extra + mbytes + hmoffs.size() * sizeof(int));
        F->pat.resize((size_t)count);
    }
    SHIP(hipHostMalloc((void **)&F->hout, out_bytes ? out_bytes : 1, hipHostMallocDefault));
    SHIP(hipHostMalloc((void **)&F->hp, (size_t)count * sizeof(SmallQP), hipHostMallocDefault));
    F->out_off = upload_bytes; F->out_bytes = out_bytes;
    h = (char *)calloc(upload_bytes ? upload_bytes : 1, 1);
    if (!h) { snprintf(s_err, sizeof(s_err), "fleet: host staging allocation failed"); rc = -1; goto done; }
    parallel_items(count, [&](long i) {              // the conversions of slot_submit, straight into the staging image
        static thread_local ItemScratch W;
        if (!mu) { if (lay_convert(data[i], lay[(size_t)i], h, W)) conv_failed = 1; return; }
        const QPDOData *d = data[i]; const MatLay &X = ml[(size_t)i]; FleetPattern &Pt = F->pat[(size_t)i];
        if (lay_convert(d, lay[(size_t)i], h, W, (int *)(h + X.mapA), X.has_mapQ ? (int *)(h + X.mapQ) : nullptr)) { conv_failed = 1; return; }
        auto keep = [](const cholmod_sparse *M, std::vector<int> &p, std::vector<int> &ix) {
            const long long nc = (long long)M->ncol, nnz = idx_at(M->p, M->itype, nc);
            p.resize((size_t)nc + 1); ix.resize((size_t)nnz);
            for (long long j = 0; j <= nc; j++) p[(size_t)j] = (int)idx_at(M->p, M->itype, j);
            for (long long k = 0; k < nnz; k++) ix[(size_t)k] = (int)idx_at(M->i, M->itype, k);
        };
        Pt.Anrow = d->A->nrow; Pt.Ancol = d->A->ncol; Pt.Qnrow = d->Q->nrow; Pt.Qncol = d->Q->ncol; Pt.Qstype = d->Q->stype;
        keep(d->A, Pt.Ap, Pt.Ai); keep(d->Q, Pt.Qp, Pt.Qi);
    });
    if (conv_failed) { snprintf(s_err, sizeof(s_err), "fleet: host memory for the matrix conversions"); rc = -1; goto done; }
    SHIP(hipMemcpyAsync(F->arena, h, upload_bytes, hipMemcpyHostToDevice, F->stream));     // the only matrix upload the fleet ever makes
    F->matrix_bytes = (long)upload_bytes;
    {
        // where K lives: the rule of every launch (small_plan); the pattern, hence every item's half-bandwidth, is fixed for the fleet's life
        std::vector<int> bws;
        const SmallPlan plan = small_plan(2, nmax, mmax, [&]() { return small_band_bytes(count, [&](long i) { return data[i]; }, bws); });
        F->lds = plan.lds; F->layout = plan.layout;
        F->kflags = small_kflags(plan);
        // the work vectors beside the factor in LDS when both fit (as a batch through the latency kernel has them)
        size_t lds_vec = 0;
        const size_t voff = small_vec_lds(F->lds, nmax, mmax, &lds_vec);
        const unsigned vec_off = plan.layout != K_GLOBAL ? (unsigned)voff : 0u;
        if (vec_off) F->lds = lds_vec;
        char *dbase = F->arena;
        for (long i = 0; i < count; i++) {
            const QPDOData *d = data[i]; Lay &L = lay[(size_t)i]; SmallQP &p = hp[(size_t)i]; SmallRes &r = hr[(size_t)i]; FleetItem &I = F->it[(size_t)i];
            const size_t n = d->n, m = d->m;
            lay_describe(p, d, L, dbase); memset(&r, 0, sizeof(r));
            p.res = F->dres + i;
            if (plan.layout == K_BAND) p.bw = bws[(size_t)i];
            double *v = (double *)(dbase + o_rec[(size_t)i]);
            double *D = v, *Dinv = D + n, *sx = Dinv + n, *sQx = sx + n, *sxb = sQx + n, *sAty = sxb + n;
            double *E = sAty + n, *Einv = E + m, *sy = Einv + m, *syb = sy + m, *sAx = syb + m, *smu = sAx + m, *sisq = smu + m;
            r.rD = D; r.rDinv = Dinv; r.rE = E; r.rEinv = Einv; r.r_c = 1.0; r.r_cinv = 1.0;
            r.state_x = sx; r.state_Qx = sQx; r.st_xbar = sxb; r.st_Aty = sAty; r.st_y = sy; r.st_ybar = syb; r.st_Ax = sAx; r.st_mu = smu; r.st_isq = sisq;
            r.lds_vec_off = vec_off; r.fleet_status = QPDO_UNSOLVED;
            if (mu) {
                const MatLay &X = ml[(size_t)i];
                r.mapA = (const int *)(dbase + X.mapA); r.mapQ = X.has_mapQ ? (const int *)(dbase + X.mapQ) : nullptr;
                r.raw_q = (double *)(dbase + X.rq); r.raw_l = (double *)(dbase + X.rl); r.raw_u = (double *)(dbase + X.ru);
                if (F->st.scaling > 0) { r.rawA = (double *)(dbase + X.rawA); r.rawQ = (double *)(dbase + X.rawQ); }
            }
            I.n = (int)n; I.m = (int)m; I.o_solx = L.solx - upload_bytes; I.o_soly = L.soly - upload_bytes; I.o_dx = L.dx - upload_bytes; I.o_dy = L.dy - upload_bytes;
        }
    }
    SHIP(hipMemcpyAsync(F->dprobs, hp.data(), (size_t)count * sizeof(SmallQP), hipMemcpyHostToDevice, F->stream));
    SHIP(hipMemcpyAsync(F->dres, hr.data(), (size_t)count * sizeof(SmallRes), hipMemcpyHostToDevice, F->stream));
    SHIP(hipMemcpyAsync(F->doffs, hoffs.data(), hoffs.size() * sizeof(int), hipMemcpyHostToDevice, F->stream));
    if (mu) SHIP(hipMemcpyAsync(F->dmoffs, hmoffs.data(), hmoffs.size() * sizeof(int), hipMemcpyHostToDevice, F->stream));
    SHIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_small_fleet), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMALL_LDS_BUDGET));
    if (flags & QPDO_AMD_FLEET_ADJOINT)                // (the adjoint launch takes the solve's plan: nothing of its own is resident)
        SHIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_small_fleet_adjoint), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMALL_LDS_BUDGET));
    if ((flags & QPDO_AMD_FLEET_ADJOINT) && F->layout == K_PACKED) {
        // (a measuring switch: QPDO_AMD_FLEET_RHS_GROUP=1..8 at create overrides the group size, tools/fleet_sensitivity_latency.py)
        const char *e = getenv("QPDO_AMD_FLEET_RHS_GROUP");
        const int g = e ? atoi(e) : FLEET_RHS_GROUP;
        F->rhs_group = g < 1 ? 1 : (g > 8 ? 8 : g);
    }
    if (flags & QPDO_AMD_FLEET_ADJOINT)                // (adjoint_multi_dev, tangent_dev: the same plan)
        SHIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_small_fleet_sens), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMALL_LDS_BUDGET));
    hipLaunchKernelGGL(k_small_fleet_setup, dim3((unsigned)count), dim3(SM_THREADS), 0, F->stream, F->dprobs, (int)count, F->st);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));           // (the pageable staging images above are read until here)
done:
    free(h);
    if (rc) { fleet_free(F); return nullptr; }
    return F;
}

// q, l, u: arrays of `count` pointers or NULL; entries may be NULL.  Checked by the caller (qpdo_api.c): l <= u where both are passed.
int qdev_small_fleet_update(void *h_, const double *const *q, const double *const *l, const double *const *u) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    double *hs = (double *)F->hstage; int *ht = (int *)(hs + F->stage_doubles);
    size_t off = 0;
    for (long i = 0; i < F->count; i++) {
        const size_t n = (size_t)F->it[(size_t)i].n, m = (size_t)F->it[(size_t)i].m;
        int *t = ht + 4 * i;
        t[0] = t[1] = t[2] = -1; t[3] = 0;
        if (q && q[i]) { t[0] = (int)off; memcpy(hs + off, q[i], n * 8); off += n; }
        if (l && l[i]) { t[1] = (int)off; if (m) memcpy(hs + off, l[i], m * 8); off += m; }
        if (u && u[i]) { t[2] = (int)off; if (m) memcpy(hs + off, u[i], m * 8); off += m; }
    }
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    if (off) SHIP(hipMemcpyAsync(F->dstage, hs, off * 8, hipMemcpyHostToDevice, F->stream));
    SHIP(hipMemcpyAsync(F->dtab, ht, (size_t)F->count * QPDO_AMD_FLEET_TABLE_BYTES, hipMemcpyHostToDevice, F->stream));
    hipLaunchKernelGGL(k_small_fleet_update, dim3((unsigned)F->count), dim3(SM_THREADS), 0, F->stream, F->dprobs, (int)F->count, F->st, (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));           // (the pinned staging is free for the next call)
    F->vector_bytes_last = (long)(off * 8 + (size_t)F->count * QPDO_AMD_FLEET_TABLE_BYTES);
done:
    F->last_was_solve = false;
    return rc;
}
// Q, A: arrays of `count` cholmod_sparse pointers or NULL; entries may be NULL.  Every passed matrix is compared with the create-time pattern
// in full before anything is written; then one upload [table][values], one launch (k_small_fleet_matrices), one stream sync.
static int fleet_pattern_differs(const cholmod_sparse *M, size_t nrow, size_t ncol, int stype, bool check_stype, const std::vector<int> &p, const std::vector<int> &ix,
                                 const char *name, long item) {
    auto refuse = [&](const char *why) { snprintf(s_err, sizeof(s_err), "item %ld: %s %s", item, name, why); return 1; };
    if (M->nrow != nrow) return refuse("has a different number of rows than at create");
    if (M->ncol != ncol) return refuse("has a different number of columns than at create");
    if (check_stype && M->stype != stype) return refuse("has a different stype than at create");
    if (M->itype != 0 && M->itype != 2) return refuse("has an unknown itype");
    if (!M->p || (!M->i && !ix.empty())) return refuse("has a NULL pattern array");
    if (idx_at(M->p, M->itype, (long long)ncol) != (long long)ix.size()) return refuse("has a different number of entries than at create");
    for (size_t j = 0; j <= ncol; j++) if (idx_at(M->p, M->itype, (long long)j) != (long long)p[j]) return refuse("has a column pointer that differs from the pattern at create");
    for (size_t k = 0; k < ix.size(); k++) if (idx_at(M->i, M->itype, (long long)k) != (long long)ix[k]) return refuse("has a row index that differs from the pattern at create");
    if (!M->x && !ix.empty()) return refuse("has a NULL value array x");
    return 0;
}
int qdev_small_fleet_update_matrices(void *h_, const void *const *Q_, const void *const *A_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    const cholmod_sparse *const *Q = (const cholmod_sparse *const *)Q_, *const *A = (const cholmod_sparse *const *)A_;
    if (!(F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES)) {
        snprintf(s_err, sizeof(s_err), "the fleet was created without QPDO_AMD_FLEET_MATRIX_UPDATES (qpdo_amd_fleet_create_ex)");
        return -1;
    }
    for (long i = 0; i < F->count; i++) {
        const FleetPattern &Pt = F->pat[(size_t)i];
        if (Q && Q[i] && fleet_pattern_differs(Q[i], Pt.Qnrow, Pt.Qncol, Pt.Qstype, true, Pt.Qp, Pt.Qi, "Q", i)) return -1;
        if (A && A[i] && fleet_pattern_differs(A[i], Pt.Anrow, Pt.Ancol, 0, false, Pt.Ap, Pt.Ai, "A", i)) return -1;
    }
    if (!Q && !A) return 0;
    const size_t tab_bytes = (size_t)F->count * QPDO_AMD_FLEET_MATRIX_TABLE_BYTES;
    int *ht = (int *)F->hmstage; double *hs = (double *)(F->hmstage + tab_bytes);
    size_t off = 0; long items = 0;
    for (long i = 0; i < F->count; i++) {
        const FleetPattern &Pt = F->pat[(size_t)i];
        int *t = ht + 2 * i;
        t[0] = t[1] = -1;
        if (Q && Q[i]) { t[0] = (int)off; if (!Pt.Qi.empty()) memcpy(hs + off, Q[i]->x, Pt.Qi.size() * 8); off += Pt.Qi.size(); }
        if (A && A[i]) { t[1] = (int)off; if (!Pt.Ai.empty()) memcpy(hs + off, A[i]->x, Pt.Ai.size() * 8); off += Pt.Ai.size(); }
        items += (t[0] >= 0 || t[1] >= 0);
    }
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    SHIP(hipMemcpyAsync(F->dmstage, F->hmstage, tab_bytes + off * 8, hipMemcpyHostToDevice, F->stream));
    SHIP(hipEventRecord(F->ev0, F->stream));
    hipLaunchKernelGGL(k_small_fleet_matrices, dim3((unsigned)F->count), dim3(SM_THREADS), 0, F->stream, F->dprobs, (int)F->count, F->st,
                       (const int *)F->dmstage, (const double *)(F->dmstage + tab_bytes));
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(F->ev1, F->stream));
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));           // (the pinned staging is free for the next call)
    { float ms = 0.f; if (hipEventElapsedTime(&ms, F->ev0, F->ev1) == hipSuccess) F->m_kernel_s = (double)ms * 1e-3; }
    F->timing_pending = false;                       // (ev0 / ev1 no longer bracket a solve)
    F->m_calls++; F->m_items_last = items; F->m_bytes_last = (long)(tab_bytes + off * 8);
done:
    F->last_was_solve = false;
    return rc;
}
void qdev_small_fleet_matrix_stats(const void *h_, long *out4, double *kernel_s) {
    const SmallFleet *F = (const SmallFleet *)h_;
    out4[0] = F->m_calls; out4[1] = F->m_items_last; out4[2] = F->m_bytes_last; out4[3] = F->m_extra_bytes;
    *kernel_s = F->m_kernel_s;
}
// last = 1: every item from the x, y its last solve returned (device copies; zero where that solve left no finite solution)
int qdev_small_fleet_warm_start(void *h_, const double *const *x0, const double *const *y0, int last) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    double *hs = (double *)F->hstage; int *ht = (int *)(hs + F->stage_doubles);
    size_t off = 0;
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    if (!last) {
        for (long i = 0; i < F->count; i++) {
            const size_t n = (size_t)F->it[(size_t)i].n, m = (size_t)F->it[(size_t)i].m;
            int *t = ht + 4 * i;
            t[0] = t[1] = t[2] = -1; t[3] = 0;
            if (x0 && x0[i]) { t[0] = (int)off; memcpy(hs + off, x0[i], n * 8); off += n; }
            if (y0 && y0[i]) { t[1] = (int)off; if (m) memcpy(hs + off, y0[i], m * 8); off += m; }
        }
        if (off) SHIP(hipMemcpyAsync(F->dstage, hs, off * 8, hipMemcpyHostToDevice, F->stream));
        SHIP(hipMemcpyAsync(F->dtab, ht, (size_t)F->count * QPDO_AMD_FLEET_TABLE_BYTES, hipMemcpyHostToDevice, F->stream));
    }
    hipLaunchKernelGGL(k_small_fleet, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, F->stream, F->dprobs, (int)F->count, F->st, F->kflags, last ? 2 : 1,
                       (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));
    F->vector_bytes_last = last ? 0 : (long)(off * 8 + (size_t)F->count * QPDO_AMD_FLEET_TABLE_BYTES);
done:
    F->last_was_solve = false;
    return rc;
}
// The last solve's descriptors and outputs to the host on the fleet's stream (the caller has made it wait for the chain event), then what a
// solve delivers: info[i], x and y with NaN for the infeasible statuses.  The end of a host solve, and the whole of fetch_last.
static int fleet_fetch(SmallFleet *F, double *const *x, double *const *y, QPDOInfo *info) {
    int rc = 0;
    SHIP(hipMemcpyAsync(F->hp, F->dprobs, (size_t)F->count * sizeof(SmallQP), hipMemcpyDeviceToHost, F->stream));
    if (F->out_bytes) SHIP(hipMemcpyAsync(F->hout, F->arena + F->out_off, F->out_bytes, hipMemcpyDeviceToHost, F->stream));
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));
    if (F->timing_pending) { float ms = 0.f; if (hipEventElapsedTime(&ms, F->ev0, F->ev1) == hipSuccess) F->kernel_s = (double)ms * 1e-3; }
    F->timing_pending = false; F->solved = true;
    parallel_items(F->count, [&](long i) {
        const FleetItem &I = F->it[(size_t)i];
        if (info) info[i] = F->hp[(size_t)i].info;
        const long stv = F->hp[(size_t)i].info.status_val;
        const bool infeasible = (stv == QPDO_PRIMAL_INFEASIBLE) || (stv == QPDO_DUAL_INFEASIBLE);
        const double *sx = (const double *)(F->hout + I.o_solx), *sy = (const double *)(F->hout + I.o_soly);
        if (x && x[i]) for (int k = 0; k < I.n; k++) x[i][k] = infeasible ? NAN : sx[k];
        if (y && y[i]) for (int k = 0; k < I.m; k++) y[i][k] = infeasible ? NAN : sy[k];
    });
done:
    return rc;
}
// ONE launch for the whole fleet; x, y: arrays of `count` pointers or NULL (entries may be NULL), info: `count` QPDOInfo
int qdev_small_fleet_solve(void *h_, double *const *x, double *const *y, void *info_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    SHIP(hipEventRecord(F->ev0, F->stream));
    hipLaunchKernelGGL(k_small_fleet, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, F->stream, F->dprobs, (int)F->count, F->st, F->kflags, 0,
                       (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(F->ev1, F->stream));
    F->solve_launches++; F->solves++; F->timing_pending = true; F->last_was_solve = true;
    rc = fleet_fetch(F, x, y, (QPDOInfo *)info_);
done:
    return rc;
}

// ---- the calls on device arrays and the caller's stream (include/qpdo_amd_ext.h): checks on the host, then launches, no wait ---------------
static int fleet_dev_lens(const SmallFleet *F, long n_len, long m_len) {
    const long N = F->noff.back(), M = F->moff.back();
    if (n_len != N) { snprintf(s_err, sizeof(s_err), "n_len is %ld, the fleet's packed n-vectors have %ld elements", n_len, N); return -1; }
    if (m_len != M) { snprintf(s_err, sizeof(s_err), "m_len is %ld, the fleet's packed m-vectors have %ld elements", m_len, M); return -1; }
    return 0;
}
// a passed array must be device (or managed) memory of the fleet's device by the runtime's own record: no kernel sees any other pointer
static int fleet_dev_ptr(const SmallFleet *F, const void *p, const char *name) {
    if (!p) return 0;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) (void)hipGetLastError();    // (a pointer the runtime does not know: the error is the answer, not a fault of this call)
    if (e == hipSuccess && (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) && a.device == F->device) return 0;
    snprintf(s_err, sizeof(s_err), "%s is not device memory on the fleet's device %d", name, F->device);
    return -1;
}
static void fleet_gather(SmallFleet *F, hipStream_t s, int kind, const double *a0, const double *a1, const double *a2, const int *mask) {
    hipLaunchKernelGGL(k_small_fleet_gather, dim3((unsigned)F->count), dim3(FLEET_IO_THREADS), 0, s, (int)F->count, (const int *)F->doffs, kind, a0, a1, a2, mask,
                       F->dtab, F->dstage, F->drec);
}
int qdev_small_fleet_update_dev(void *h_, const double *q, const double *l, const double *u, const int *item_mask, long n_len, long m_len, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    hipStream_t s = (hipStream_t)stream_;
    SHIP(hipSetDevice(F->device));
    if (fleet_dev_lens(F, n_len, m_len) || fleet_dev_ptr(F, q, "q") || fleet_dev_ptr(F, l, "l") || fleet_dev_ptr(F, u, "u") || fleet_dev_ptr(F, item_mask, "item_mask")) return -1;
    if (!q && !l && !u) return 0;
    SHIP(fleet_enter(F, s));
    fleet_gather(F, s, 0, q, l, u, item_mask);
    SHIP(hipGetLastError());
    hipLaunchKernelGGL(k_small_fleet_update, dim3((unsigned)F->count), dim3(SM_THREADS), 0, s, F->dprobs, (int)F->count, F->st, (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, s));
    F->vector_bytes_last = 0; F->d_updates++; F->last_was_solve = false;
done:
    return rc;
}
// last = 1: warm_start_last on the caller's stream (nothing to gather)
int qdev_small_fleet_warm_start_dev(void *h_, const double *x0, const double *y0, const int *item_mask, long n_len, long m_len, int last, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    hipStream_t s = (hipStream_t)stream_;
    SHIP(hipSetDevice(F->device));
    if (!last && (fleet_dev_lens(F, n_len, m_len) || fleet_dev_ptr(F, x0, "x0") || fleet_dev_ptr(F, y0, "y0") || fleet_dev_ptr(F, item_mask, "item_mask"))) return -1;
    SHIP(fleet_enter(F, s));
    if (!last) { fleet_gather(F, s, 1, x0, y0, nullptr, item_mask); SHIP(hipGetLastError()); }
    hipLaunchKernelGGL(k_small_fleet, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, s, F->dprobs, (int)F->count, F->st, F->kflags, last ? 2 : 1,
                       (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, s));
    F->vector_bytes_last = 0; F->d_warm_starts++; F->last_was_solve = false;
done:
    return rc;
}
// New Q / A values from the caller's packed device arrays (layout: qdev_small_fleet_packed_matrix_layout).  The pattern is fixed at create
// and the arrays carry values only, so there is nothing to compare: the gather fills the staging and the table, k_small_fleet_matrices
// runs behind it as in the host call.  No event timing: m_kernel_s keeps the last host call's figure.
static const char *const FLEET_NO_MATRIX_FLAG = "the fleet was created without QPDO_AMD_FLEET_MATRIX_UPDATES (qpdo_amd_fleet_create_ex)";   // (the host call's message)
int qdev_small_fleet_update_matrices_dev(void *h_, const double *Qx, const double *Ax, const int *item_mask, long q_len, long a_len, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    hipStream_t s = (hipStream_t)stream_;
    if (!(F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES)) { snprintf(s_err, sizeof(s_err), "%s", FLEET_NO_MATRIX_FLAG); return -1; }
    const long NQ = F->qoff.back(), NA = F->aoff.back();
    if (q_len != NQ) { snprintf(s_err, sizeof(s_err), "q_len is %ld, the fleet's packed Q values have %ld elements", q_len, NQ); return -1; }
    if (a_len != NA) { snprintf(s_err, sizeof(s_err), "a_len is %ld, the fleet's packed A values have %ld elements", a_len, NA); return -1; }
    SHIP(hipSetDevice(F->device));
    if (fleet_dev_ptr(F, Qx, "Qx") || fleet_dev_ptr(F, Ax, "Ax") || fleet_dev_ptr(F, item_mask, "item_mask")) return -1;
    if (!Qx && !Ax) return 0;
    {
        const size_t tab_bytes = (size_t)F->count * QPDO_AMD_FLEET_MATRIX_TABLE_BYTES;
        SHIP(fleet_enter(F, s));
        // dmstage is shared with the host matrix call.  No new hazard: both calls wait for the chain event before they write it, this one
        // records the event behind the consumer kernel, and the host call ends in its own stream sync -- so whichever call comes next
        // starts writing only after the previous call's k_small_fleet_matrices has read the table and the values.
        hipLaunchKernelGGL(k_small_fleet_gather_matrices, dim3((unsigned)F->count), dim3(FLEET_IO_THREADS), 0, s, (int)F->count, (const int *)F->dmoffs, Qx, Ax, item_mask,
                           (int *)F->dmstage, (double *)(F->dmstage + tab_bytes));
        SHIP(hipGetLastError());
        hipLaunchKernelGGL(k_small_fleet_matrices, dim3((unsigned)F->count), dim3(SM_THREADS), 0, s, F->dprobs, (int)F->count, F->st,
                           (const int *)F->dmstage, (const double *)(F->dmstage + tab_bytes));
        SHIP(hipGetLastError());
        SHIP(fleet_leave(F, s));
        F->m_calls++; F->m_items_last = -1; F->m_bytes_last = 0;      // (which items took a matrix is known on the device only)
        F->last_was_solve = false;
    }
done:
    return rc;
}
int qdev_small_fleet_packed_matrix_layout(const void *h_, long *qoff, long *aoff) {
    const SmallFleet *F = (const SmallFleet *)h_;
    if (!(F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES)) { snprintf(s_err, sizeof(s_err), "%s", FLEET_NO_MATRIX_FLAG); return -1; }
    memcpy(qoff, F->qoff.data(), F->qoff.size() * sizeof(long)); memcpy(aoff, F->aoff.data(), F->aoff.size() * sizeof(long));
    return 0;
}
int qdev_small_fleet_solve_dev(void *h_, double *x, double *y, long *status, double *norms, double *prim_inf_cert, double *dual_inf_cert, long n_len, long m_len, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    hipStream_t s = (hipStream_t)stream_;
    SHIP(hipSetDevice(F->device));
    if (fleet_dev_lens(F, n_len, m_len) || fleet_dev_ptr(F, x, "x") || fleet_dev_ptr(F, y, "y") || fleet_dev_ptr(F, status, "status") || fleet_dev_ptr(F, norms, "norms") ||
        fleet_dev_ptr(F, prim_inf_cert, "prim_inf_cert") || fleet_dev_ptr(F, dual_inf_cert, "dual_inf_cert")) return -1;
    SHIP(fleet_enter(F, s));
    SHIP(hipEventRecord(F->ev0, s));
    hipLaunchKernelGGL(k_small_fleet, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, s, F->dprobs, (int)F->count, F->st, F->kflags, 0,
                       (const int *)F->dtab, (const double *)F->dstage);
    SHIP(hipGetLastError());
    SHIP(hipEventRecord(F->ev1, s));
    F->solve_launches++; F->solves++; F->d_solves++; F->last_was_solve = true;
    F->timing_pending = true; F->solved = false;     // (the host image is the previous solve's until fetch_last)
    if (x || y || status || norms || prim_inf_cert || dual_inf_cert) {
        hipLaunchKernelGGL(k_small_fleet_scatter, dim3((unsigned)F->count), dim3(FLEET_IO_THREADS), 0, s, (const SmallQP *)F->dprobs, (int)F->count, (const int *)F->doffs,
                           x, y, status, norms, prim_inf_cert, dual_inf_cert);
        SHIP(hipGetLastError());
    }
    SHIP(fleet_leave(F, s));
done:
    return rc;
}
long qdev_small_fleet_adjoint_calls(const void *h_) { return ((const SmallFleet *)h_)->adjoint_calls; }
// The adjoint of the last solve and many right-hand sides per factorization (include/qpdo_amd_ext.h): ONE set of checks on the host, then
// ONE launch in the solve's launch shape, no wait.  No call changes the fleet's state or moves a counter other than its own.
// The kernel addresses right-hand side r at r * (per-RHS length) in 64 bits; what it counts in 32 bits is the right-hand sides.
static const long FLEET_SENS_MAX_NRHS = 2147483647L;
static int fleet_sens_checks(const SmallFleet *F, long nrhs, bool matrices, const char *mname, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len,
                             bool need_q, bool need_a) {
    if (!(F->flags & QPDO_AMD_FLEET_ADJOINT)) { snprintf(s_err, sizeof(s_err), "the fleet was created without QPDO_AMD_FLEET_ADJOINT (qpdo_amd_fleet_create_ex)"); return -1; }
    if (nrhs < 1) { snprintf(s_err, sizeof(s_err), "nrhs is %ld, it must be at least 1", nrhs); return -1; }
    if (nrhs > FLEET_SENS_MAX_NRHS) { snprintf(s_err, sizeof(s_err), "nrhs is %ld, the kernel counts at most %ld right-hand sides", nrhs, FLEET_SENS_MAX_NRHS); return -1; }
    if (fleet_dev_lens(F, n_len, m_len)) return -1;
    if (matrices) {
        if (!(F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES)) { snprintf(s_err, sizeof(s_err), "%s was passed, but %s", mname, FLEET_NO_MATRIX_FLAG); return -1; }
        const long NQ = F->qoff.back(), NA = F->aoff.back();
        if (need_q && q_len != NQ) { snprintf(s_err, sizeof(s_err), "q_len is %ld, the fleet's packed Q values have %ld elements", q_len, NQ); return -1; }
        if (need_a && a_len != NA) { snprintf(s_err, sizeof(s_err), "a_len is %ld, the fleet's packed A values have %ld elements", a_len, NA); return -1; }
    }
    if (!(tol > 0.0) || !(tol <= 1.7976931348623157e308)) { snprintf(s_err, sizeof(s_err), "tol is %g, it must be a positive finite number", tol); return -1; }
    if (max_sweeps < 1) { snprintf(s_err, sizeof(s_err), "max_sweeps is %ld, it must be at least 1", max_sweeps); return -1; }
    return 0;
}
static int fleet_sens_launch(SmallFleet *F, hipStream_t s, SensArgs &a, long nrhs) {
    int rc = 0;
    a.nrhs = (int)nrhs; a.N = F->noff.back(); a.M = F->moff.back();
    a.NQ = (F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES) ? F->qoff.back() : 0; a.NA = (F->flags & QPDO_AMD_FLEET_MATRIX_UPDATES) ? F->aoff.back() : 0;
    a.group = nrhs > 1 ? F->rhs_group : 1; a.scratch = nullptr;
    if (a.group > 1) {
        // the slots of the right-hand sides carried at once: a host allocation, once (the first call with nrhs > 1 may block)
        if (!F->sens_scratch) {
            const size_t bytes = (size_t)F->rhs_group * (7 * (size_t)a.N + 5 * (size_t)a.M) * sizeof(double);
            SHIP(hipMalloc((void **)&F->sens_scratch, bytes));
            F->sens_scratch_bytes = (long)bytes;
        }
        a.scratch = F->sens_scratch;
    }
    SHIP(fleet_enter(F, s));
    hipLaunchKernelGGL(k_small_fleet_sens, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, s, F->dprobs, (int)F->count, F->st, F->kflags, (const int *)F->doffs,
                       (const int *)F->dmoffs, a);
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, s));
    F->sens_calls++; F->sens_rhs += nrhs;
done:
    return rc;
}
static const char *const FLEET_NOT_A_SOLVE = "the most recent state-changing fleet call was not a solve: the resident q, l, u and matrices must be those of the x, y returned";
// every check of adjoint_dev (nrhs = 1) and adjoint_multi_dev, in ONE order; sname, rname: what the call names its status and residual arrays
static int fleet_adjoint_checks(SmallFleet *F, long nrhs, const double *gx, const double *gy, double *dq, double *dl, double *du, double *dQx, double *dAx, int *active,
                                long *status, const char *sname, double *res, const char *rname, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len) {
    int rc = 0;
    if (fleet_sens_checks(F, nrhs, dQx || dAx, dQx ? "dQx" : "dAx", tol, max_sweeps, n_len, m_len, q_len, a_len, dQx != nullptr, dAx != nullptr)) return -1;
    if (!gx) { snprintf(s_err, sizeof(s_err), "gx is NULL"); return -1; }
    if (!dq) { snprintf(s_err, sizeof(s_err), "dq is NULL"); return -1; }
    if (!dl) { snprintf(s_err, sizeof(s_err), "dl is NULL"); return -1; }
    if (!du) { snprintf(s_err, sizeof(s_err), "du is NULL"); return -1; }
    if (!F->last_was_solve) { snprintf(s_err, sizeof(s_err), "%s", FLEET_NOT_A_SOLVE); return -1; }
    SHIP(hipSetDevice(F->device));
    if (fleet_dev_ptr(F, gx, "gx") || fleet_dev_ptr(F, gy, "gy") || fleet_dev_ptr(F, dq, "dq") || fleet_dev_ptr(F, dl, "dl") || fleet_dev_ptr(F, du, "du") ||
        fleet_dev_ptr(F, dQx, "dQx") || fleet_dev_ptr(F, dAx, "dAx") || fleet_dev_ptr(F, active, "active") || fleet_dev_ptr(F, status, sname) ||
        fleet_dev_ptr(F, res, rname)) return -1;
done:
    return rc;
}
// The adjoint of the last solve on the caller's stream (include/qpdo_amd_ext.h): the checks, then ONE launch of its own kernel in the solve's
// launch shape (layout word, dynamic LDS), no wait.  Moves adjoint_calls and no other counter.  (k_small_fleet_sens with one right-hand side
// delivers the same bits, but 0.02 ms later on 4096 C3 items: profiles/fleet_one_sens_kernel_latency.txt.)
int qdev_small_fleet_adjoint_dev(void *h_, const double *gx, const double *gy, double *dq, double *dl, double *du, double *dQx, double *dAx, int *active, long *adj_status,
                                 double *adj_res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    hipStream_t s = (hipStream_t)stream_;
    if (fleet_adjoint_checks(F, 1, gx, gy, dq, dl, du, dQx, dAx, active, adj_status, "adj_status", adj_res, "adj_res", tol, max_sweeps, n_len, m_len, q_len, a_len)) return -1;
    SHIP(fleet_enter(F, s));
    hipLaunchKernelGGL(k_small_fleet_adjoint, dim3((unsigned)F->count), dim3(SM_THREADS), F->lds, s, F->dprobs, (int)F->count, F->st, F->kflags, (const int *)F->doffs,
                       (const int *)F->dmoffs, gx, gy, dq, dl, du, dQx, dAx, active, adj_status, adj_res, tol, (int)(max_sweeps > 1000000 ? 1000000 : max_sweeps));
    SHIP(hipGetLastError());
    SHIP(fleet_leave(F, s));
    F->adjoint_calls++;
done:
    return rc;
}
int qdev_small_fleet_adjoint_multi_dev(void *h_, long nrhs, const double *gx, const double *gy, double *dq, double *dl, double *du, double *dQx, double *dAx, int *active,
                                       long *status, double *res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len, void *stream_) {
    SmallFleet *F = (SmallFleet *)h_;
    if (fleet_adjoint_checks(F, nrhs, gx, gy, dq, dl, du, dQx, dAx, active, status, "status", res, "res", tol, max_sweeps, n_len, m_len, q_len, a_len)) return -1;
    SensArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = 0; a.in_n = gx; a.in_l = gy; a.out_n = dq; a.out_m1 = dl; a.out_m2 = du; a.out_q = dQx; a.out_a = dAx;
    a.active = active; a.status = status; a.res = res; a.tol = tol; a.max_sweeps = (int)(max_sweeps > 1000000 ? 1000000 : max_sweeps);
    return fleet_sens_launch(F, (hipStream_t)stream_, a, nrhs);
}
int qdev_small_fleet_tangent_dev(void *h_, long nrhs, const double *tq, const double *tl, const double *tu, const double *tQx, const double *tAx, double *dx, double *dy,
                                 int *active, long *status, double *res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len, void *stream_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    if (fleet_sens_checks(F, nrhs, tQx || tAx, tQx ? "tQx" : "tAx", tol, max_sweeps, n_len, m_len, q_len, a_len, tQx != nullptr, tAx != nullptr)) return -1;
    if (!tq && !tl && !tu && !tQx && !tAx) { snprintf(s_err, sizeof(s_err), "no tangent passed: tq, tl, tu, tQx and tAx are all NULL"); return -1; }
    if (!dx) { snprintf(s_err, sizeof(s_err), "dx is NULL"); return -1; }
    if (!dy) { snprintf(s_err, sizeof(s_err), "dy is NULL"); return -1; }
    if (!F->last_was_solve) { snprintf(s_err, sizeof(s_err), "%s", FLEET_NOT_A_SOLVE); return -1; }
    SHIP(hipSetDevice(F->device));
    if (fleet_dev_ptr(F, tq, "tq") || fleet_dev_ptr(F, tl, "tl") || fleet_dev_ptr(F, tu, "tu") || fleet_dev_ptr(F, tQx, "tQx") || fleet_dev_ptr(F, tAx, "tAx") ||
        fleet_dev_ptr(F, dx, "dx") || fleet_dev_ptr(F, dy, "dy") || fleet_dev_ptr(F, active, "active") || fleet_dev_ptr(F, status, "status") ||
        fleet_dev_ptr(F, res, "res")) return -1;
    {
        SensArgs a;
        memset(&a, 0, sizeof(a));
        a.mode = 1; a.in_n = tq; a.in_l = tl; a.in_u = tu; a.in_q = tQx; a.in_a = tAx; a.out_n = dx; a.out_m1 = dy;
        a.active = active; a.status = status; a.res = res; a.tol = tol; a.max_sweeps = (int)(max_sweeps > 1000000 ? 1000000 : max_sweeps);
        rc = fleet_sens_launch(F, (hipStream_t)stream_, a, nrhs);
    }
done:
    return rc;
}
// right-hand sides one workgroup carries at once: FLEET_RHS_GROUP in the PACKED layout, 1 (one after another) in the others
int qdev_small_fleet_rhs_group(const void *h_) { return ((const SmallFleet *)h_)->rhs_group; }
void qdev_small_fleet_sens_stats(const void *h_, long *out3) {
    const SmallFleet *F = (const SmallFleet *)h_;
    out3[0] = F->sens_calls; out3[1] = F->sens_rhs; out3[2] = F->sens_scratch_bytes;
}
int qdev_small_fleet_fetch_last(void *h_, double *const *x, double *const *y, void *info_) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    if (!F->solves) { snprintf(s_err, sizeof(s_err), "no solve yet"); return -1; }
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    rc = fleet_fetch(F, x, y, (QPDOInfo *)info_);
done:
    return rc;
}
// waits for everything the fleet was asked to do; out5: device updates, warm starts, solves since create, then the refusal record since the last sync
int qdev_small_fleet_sync(void *h_, long *out5) {
    int rc = 0;
    SmallFleet *F = (SmallFleet *)h_;
    SHIP(hipSetDevice(F->device));
    SHIP(fleet_enter(F, F->stream));
    SHIP(hipMemcpyAsync(F->hrec, F->drec, 2 * sizeof(int), hipMemcpyDeviceToHost, F->stream));
    SHIP(hipMemsetD32Async((hipDeviceptr_t)F->drec, 0, 1, F->stream));
    SHIP(hipMemsetD32Async((hipDeviceptr_t)(F->drec + 1), FLEET_REC_NONE, 1, F->stream));
    SHIP(fleet_leave(F, F->stream));
    SHIP(hipStreamSynchronize(F->stream));
    if (F->timing_pending) { float ms = 0.f; if (hipEventElapsedTime(&ms, F->ev0, F->ev1) == hipSuccess) F->kernel_s = (double)ms * 1e-3; F->timing_pending = false; }
    out5[0] = F->d_updates; out5[1] = F->d_warm_starts; out5[2] = F->d_solves;
    out5[3] = F->hrec[0]; out5[4] = F->hrec[0] ? F->hrec[1] : -1;
done:
    return rc;
}
void qdev_small_fleet_packed_layout(const void *h_, long *noff, long *moff) {
    const SmallFleet *F = (const SmallFleet *)h_;
    memcpy(noff, F->noff.data(), F->noff.size() * sizeof(long)); memcpy(moff, F->moff.data(), F->moff.size() * sizeof(long));
}
// the certificates of the last solve as the kernel left them (host image): dy (m) of a primal infeasible item, dx (n) of a dual infeasible one
int qdev_small_fleet_certificates(const void *h_, long item, double *prim_inf_cert, double *dual_inf_cert) {
    const SmallFleet *F = (const SmallFleet *)h_;
    if (!F->solved) { snprintf(s_err, sizeof(s_err), "fleet: no solve yet"); return -1; }
    const FleetItem &I = F->it[(size_t)item];
    if (prim_inf_cert && I.m) memcpy(prim_inf_cert, F->hout + I.o_dy, (size_t)I.m * 8);
    if (dual_inf_cert) memcpy(dual_inf_cert, F->hout + I.o_dx, (size_t)I.n * 8);
    return 0;
}
void qdev_small_fleet_stats(const void *h_, long *out5, double *kernel_s) {
    const SmallFleet *F = (const SmallFleet *)h_;
    out5[0] = F->count; out5[1] = F->matrix_bytes; out5[2] = F->vector_bytes_last; out5[3] = F->solve_launches; out5[4] = F->solves;
    *kernel_s = F->kernel_s;
}
int qdev_small_fleet_layout(const void *h_) { return ((const SmallFleet *)h_)->layout; }
int qdev_small_fleet_device(const void *h_) { return ((const SmallFleet *)h_)->device; }
void qdev_small_fleet_dims(const void *h_, long item, int *n, int *m) {
    const SmallFleet *F = (const SmallFleet *)h_;
    *n = F->it[(size_t)item].n; *m = F->it[(size_t)item].m;
}

}  // extern "C"
