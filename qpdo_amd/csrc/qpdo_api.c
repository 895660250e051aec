/*
 * qpdo_api.c -- C host driver behind the qpdo.h C-ABI (the drop-in boundary).
 *
 * Mirrors the reference's public functions (src/qpdo.c) in name, argument
 * meaning, ownership and error behaviour.  The driver keeps only scalars and
 * the small host mirrors documented in include/qpdo.h; every vector and matrix
 * operation is a HIP kernel reached through the thin C-ABI of qpdo_dev.h.
 * There is no CPU fallback: if the device backend cannot be created,
 * qpdo_setup returns NULL.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <pthread.h>

#include "qpdo.h"
#include "qpdo_amd_ext.h"
#include "qpdo_dev.h"
#include "csc_convert.h"
#include "band_order.h"
#include "pass_decision.h"

struct QPDO_TIMER { struct timespec tic, toc; };   /* reference include/util.h:98-104 */

struct QPDOBackend {
    QpdoDev *dev;
    int reset_newton;             /* reference chol->reset_newton (types.h:132) */
    int fix_status_reset;
    QPDOAmdTraceRec *trace; long ntrace, captrace;
    long newton_passes;
    /* small problems (the packed Newton matrix fits one workgroup's LDS, n <= QPDO_SMALL_FUSED_MAX_N): qpdo_solve runs as ONE launch of
     * the fused kernel on the workspace's own device arrays (qdev_small_resident_*), in the oracle's operation order */
    void *small;                  /* resident fused-solve handle, or NULL: generic multi-kernel path */
    int ws_state;                 /* the workspace's device vectors hold the warm-started state of the pending solve (0: qpdo_solve's automatic
                                   * cold start of a fused-path workspace, which is part of the solve's launch) */
    int auto_ws;                  /* qpdo_warm_start is being called by qpdo_solve itself (qpdo.c:312-314) */
    long fused_solves, fused_factor_count; double fused_kernel_s; int last_fused;
    /* qpdo_amd_update_matrices: the caller's latest UNSCALED q, l, u (the scaled mirrors in work->data cannot give them back bit for
     * bit) and the shape of the matrices given to qpdo_setup */
    c_float *q_raw, *l_raw, *u_raw;
    int q_stype; int64_t q_nnz, a_nnz;
    QPDOAmdBandOrderInfo band_order;      /* what qpdo_setup decided about the band solver's variable order (band_order_setup) */
    QPDOAmdBandBorderInfo band_border;    /* ... and about a border of coupling variables (band_border_setup); border_solves is read from the device */
    int solved_last;              /* the most recent state-changing call was qpdo_solve (set there; cleared by qpdo_warm_start, qpdo_update_q,
                                   * qpdo_update_bounds, qpdo_amd_update_matrices): what qpdo_amd_adjoint asks before it reads the solution */
};

#define c_max(a, b) (((a) > (b)) ? (a) : (b))
#define c_min(a, b) (((a) < (b)) ? (a) : (b))
#define c_absval(x) (((x) < 0) ? -(x) : (x))

#define QPDO_PRINT(...) do { printf(__VA_ARGS__); fflush(stdout); } while (0)
#define QPDO_EPRINT(...) do { printf("ERROR in %s: ", __func__); printf(__VA_ARGS__); printf("\n"); fflush(stdout); } while (0)

/* ---- timing (reference src/util.c:245-264) ---------------------------------- */
static void tic(QPDOTimer *t) { clock_gettime(CLOCK_MONOTONIC, &t->tic); }
static c_float toc(QPDOTimer *t) {
    clock_gettime(CLOCK_MONOTONIC, &t->toc);
    return (c_float)(t->toc.tv_sec - t->tic.tv_sec) + 1e-9 * (c_float)(t->toc.tv_nsec - t->tic.tv_nsec);
}

/* ---- status strings (reference src/util.c:50-91) ------------------------------ */
static void update_status(QPDOInfo *info, c_int status_val) {
    const char *s;
    info->status_val = status_val;
    switch (status_val) {
        case QPDO_SOLVED: s = "solved"; break;
        case QPDO_DUAL_TERMINATED: s = "dual terminated"; break;
        case QPDO_PRIMAL_INFEASIBLE: s = "primal infeasible"; break;
        case QPDO_DUAL_INFEASIBLE: s = "dual infeasible"; break;
        case QPDO_PRIMAL_DUAL_INFEASIBLE: s = "primal-dual infeasible"; break;
        case QPDO_MAX_TIME_REACHED: s = "max time exceeded"; break;
        case QPDO_MAX_ITER_REACHED: s = "maximum iterations reached"; break;
        case QPDO_UNSOLVED: s = "unsolved"; break;
        case QPDO_ERROR: s = "error"; break;
        default: s = "unrecognised status value"; break;
    }
    strncpy(info->status, s, sizeof(info->status) - 1);
    info->status[sizeof(info->status) - 1] = '\0';
}

/* ---- validation (reference src/validate.c:9-170) ------------------------------- */
static int validate_data(const QPDOData *data) {
    if (!data) { QPDO_EPRINT("Missing data"); return 0; }
    for (size_t j = 0; j < data->m; j++)
        if (data->l[j] > data->u[j]) {
            QPDO_EPRINT("Lower bound at index %d is greater than upper bound: %.4e > %.4e", (int)j, data->l[j], data->u[j]);
            return 0;
        }
    return 1;
}
static int validate_settings(const QPDOSettings *s) {
    if (!s) { QPDO_EPRINT("Missing settings!"); return 0; }
    if (s->max_iter <= 0) { QPDO_EPRINT("max_iter must be positive"); return 0; }
    if (s->inner_max_iter <= 0) { QPDO_EPRINT("inner_max_iter must be positive"); return 0; }
    if (s->eps_abs <= 0) { QPDO_EPRINT("eps_abs must be positive"); return 0; }
    if (s->eps_abs_in <= 0) { QPDO_EPRINT("eps_abs_in must be positive"); return 0; }
    if (s->eps_prim_inf < 0) { QPDO_EPRINT("eps_prim_inf must be nonnegative"); return 0; }
    if (s->eps_dual_inf < 0) { QPDO_EPRINT("eps_dual_inf must be nonnegative"); return 0; }
    if (s->rho <= 0 || s->rho >= 1) { QPDO_EPRINT("rho must be positive and smaller than 1"); return 0; }
    if (s->theta <= 0 || s->theta > 1) { QPDO_EPRINT("theta must be positive and smaller than or equal to 1"); return 0; }
    if (s->delta <= 0 || s->delta >= 1) { QPDO_EPRINT("delta must be positive and smaller than 1"); return 0; }
    if (s->mu_min <= 0) { QPDO_EPRINT("mu_min must be positive"); return 0; }
    if ((s->proximal != 0) && (s->proximal != 1)) { QPDO_EPRINT("proximal must be either 0 or 1"); return 0; }
    if (s->sigma_init <= 0) { QPDO_EPRINT("sigma_init must be positive"); return 0; }
    if (s->sigma_upd <= 0 || s->sigma_upd > 1) { QPDO_EPRINT("sigma_upd must be positive and smaller than or equal to 1"); return 0; }
    if (s->sigma_min > s->sigma_init) { QPDO_EPRINT("sigma_min must be smaller than or equal to sigma_init"); return 0; }
    if (s->scaling < 0) { QPDO_EPRINT("scaling must be nonnegative"); return 0; }
    if (s->verbose < 0) { QPDO_EPRINT("verbose must be nonnegative"); return 0; }
    if (s->print_interval < 0) { QPDO_EPRINT("print_interval must be nonnegative"); return 0; }
    if (s->reset_newton_iter < 0) { QPDO_EPRINT("reset_newton_iter must be nonnegative"); return 0; }
    return 1;
}

/* reference src/qpdo.c:24-44 with include/constants.h:44-69 */
void qpdo_set_default_settings(QPDOSettings *s) {
    s->max_time = QPDO_INFTY;
    s->max_iter = 10000;
    s->inner_max_iter = 1000;
    s->eps_abs = 1e-6;
    s->eps_abs_in = 1e0;
    s->eps_prim_inf = 1e-6;
    s->eps_dual_inf = 1e-6;
    s->rho = 0.1;
    s->theta = 0.25;
    s->delta = 1e-2;
    s->mu_min = 1e-9;
    s->proximal = 1;
    s->sigma_init = 1e-3;
    s->sigma_upd = 1e-1;
    s->sigma_min = 1e-7;
    s->scaling = 10;
    s->verbose = 1;
    s->print_interval = 1;
    s->reset_newton_iter = 1000;
}
static QPDOSettings *copy_settings(const QPDOSettings *s) {   /* src/util.c:21-45 */
    QPDOSettings *n = malloc(sizeof(QPDOSettings));
    if (n) *n = *s;
    return n;
}

/* The batch stream (qpdo_amd_batch_stream_*) keeps up to `depth` fused-kernel launches in flight on separate HIP streams.  The
 * runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams that share a queue serialise: measured
 * on MI355X, 16 batches of 4096 C3 QPs at depth 12: 7.0 k QP/s on 4 queues, 10.1 k on 16.  The variable is read when the HIP
 * runtime initialises (the first HIP call of the process).  This library does NOT touch its host's environment: the caller sets
 * GPU_MAX_HW_QUEUES before its first HIP call (the Python front end does so before it loads the library), and
 * qpdo_amd_batch_stream_create says so once when a deep stream is created without it. */
static void warn_hw_queues_once(int depth) {
    static int warned = 0;
    const char *v = getenv("GPU_MAX_HW_QUEUES");
    const int have = (v && *v) ? atoi(v) : 4;
    if (depth > have && !__sync_lock_test_and_set(&warned, 1))
        fprintf(stderr, "qpdo_amd: batch stream of depth %d on %d HIP hardware queues (GPU_MAX_HW_QUEUES%s): streams that share a queue "
                        "serialise; export GPU_MAX_HW_QUEUES=%d before the process's first HIP call\n", depth, have, (v && *v) ? "" : " unset", depth > 16 ? depth : 16);
}

static int env_int_early(const char *name, int dflt) { const char *v = getenv(name); return (v && *v) ? atoi(v) : dflt; }
static double wall_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
/* ---- matrix intake: CSC (int32 or int64 indices) -> int32 CSR triples (csc_convert.h) ------------- */
static int sparse_ok(const cholmod_sparse *M) {
    if (!M || !M->p) return 0;
    if (M->itype != 0 && M->itype != 2) return 0;      /* CHOLMOD_INT / CHOLMOD_LONG */
    if (M->xtype != 1 || M->dtype != 0) return 0;      /* real, double */
    if (!M->packed && M->nz) return 0;                 /* unpacked storage not supported */
    if (M->nrow >= (size_t)INT32_MAX || M->ncol >= (size_t)INT32_MAX) return 0;
    if (idx_at(M->p, M->itype, (int64_t)M->ncol) >= (int64_t)INT32_MAX) return 0;
    return 1;
}
/* release the staging copies on a detached thread (falls back to freeing in place) */
typedef struct { HostCsr h[3]; } FreeJob;
static void *free_job(void *arg) { FreeJob *j = (FreeJob *)arg; for (int i = 0; i < 3; i++) host_csr_free(&j->h[i]); free(j); return NULL; }
static void host_csr_free_async(HostCsr *a, HostCsr *b, HostCsr *c) {
    FreeJob *j = malloc(sizeof(FreeJob));
    pthread_t th; pthread_attr_t at;
    if (j) {
        j->h[0] = *a; j->h[1] = *b; j->h[2] = *c;
        pthread_attr_init(&at); pthread_attr_setdetachstate(&at, PTHREAD_CREATE_DETACHED);
        if (pthread_create(&th, &at, free_job, j) == 0) { pthread_attr_destroy(&at); memset(a, 0, sizeof(*a)); memset(b, 0, sizeof(*b)); memset(c, 0, sizeof(*c)); return; }
        pthread_attr_destroy(&at); free(j);
    }
    host_csr_free(a); host_csr_free(b); host_csr_free(c);
}
/* One image of M into arrays of its own: CSR(M), CSR(M') or the full symmetric CSR (M = Q).  The conversions run on
 * QPDO_SETUP_THREADS OpenMP threads (default min(16, cores)).  Returns 1, or 0 (no memory; a full Q of INT32_MAX entries or more). */
enum { IMG_CSR, IMG_CSR_T, IMG_SYM_FULL };
static int host_csr_from(const cholmod_sparse *M, int which, HostCsr *out) {
    const int64_t nnz = idx_at(M->p, M->itype, (int64_t)M->ncol);
    /* a triangle mirrors into 2 nnz - (its diagonal entries): room for 2 nnz, at most n untouched entries too many, spares the full Q
     * a serial count pass over the stored entries (sym_full_nnz) before the threaded conversion */
    const int64_t cap = (which == IMG_SYM_FULL && M->stype) ? 2 * nnz : nnz;
    const int threads = env_int_early("QPDO_SETUP_THREADS", 0);
    ConvScratch W;
    int rc = 0;
    memset(out, 0, sizeof(*out));
    out->nrows = (int32_t)(which == IMG_CSR ? M->nrow : M->ncol); out->ncols = (int32_t)(which == IMG_CSR ? M->ncol : M->nrow);
    out->rp = malloc(((size_t)out->nrows + 1) * sizeof(int32_t));
    out->ci = malloc((size_t)(cap ? cap : 1) * sizeof(int32_t));
    out->val = malloc((size_t)(cap ? cap : 1) * sizeof(double));
    if (!out->rp || !out->ci || !out->val) { host_csr_free(out); return 0; }
    conv_scratch_init(&W);
    if (which == IMG_CSR) rc = csc_to_csr(M, out->rp, out->ci, out->val, NULL, threads, &W);
    else if (which == IMG_CSR_T) csc_as_csr_of_transpose(M, out->rp, out->ci, out->val, threads);
    else rc = sym_to_full_csr(M, out->rp, out->ci, out->val, NULL, threads, &W);
    conv_scratch_free(&W);
    if (rc) { host_csr_free(out); return 0; }
    out->nnz = out->rp[out->nrows];
    return 1;
}

/* ---- small host vector helpers (operation order of reference src/lin_alg.c) --------- */
static c_float vec_norm_inf(const c_float *a, size_t n) {
    c_float mx = 0.0;
    for (size_t i = 0; i < n; i++) { c_float s = c_absval(a[i]); mx = s > mx ? s : mx; }
    return mx;
}
static c_float *vec_dup(const c_float *a, size_t n) {
    c_float *b = malloc((n ? n : 1) * sizeof(c_float));
    if (b && n) memcpy(b, a, n * sizeof(c_float));
    return b;
}

/* Distributed configuration for the workspaces created next in this process (read once, under the lock, by each
 * qpdo_setup).  An RCCL unique id creates exactly ONE communicator: the qpdo_setup that consumes it clears it, and a
 * further distributed setup without a fresh qpdo_amd_dist_config fails with a message instead of hanging in
 * ncclCommInitRank on a spent id.  The host-callback mode has no such limit. */
static QdevDist g_dist = {0, 1, 0, 0, 0, 0, NULL, NULL, {0}, 0};
static int g_dist_has_id = 0, g_dist_id_spent = 0;
static pthread_mutex_t g_dist_mu = PTHREAD_MUTEX_INITIALIZER;
int qpdo_amd_dist_config(int rank, int world, const void *rccl_unique_id, qpdo_amd_allreduce_fn fn, void *ctx) {
    if (world < 1 || rank < 0 || rank >= world) return -1;
    if (world > 1 && !fn && !rccl_unique_id) return -1;
    pthread_mutex_lock(&g_dist_mu);
    memset(&g_dist, 0, sizeof(g_dist));
    g_dist.rank = rank; g_dist.world = world; g_dist.fn = (qdev_allreduce_fn)fn; g_dist.ctx = ctx;
    g_dist_has_id = 0; g_dist_id_spent = 0;
    if (rccl_unique_id && !fn) { memcpy(g_dist.nccl_id, rccl_unique_id, 128); g_dist_has_id = 1; }
    /* world == 1 with a communicator: a forced single-rank partition -- every collective call site runs (on one GPU) */
    g_dist.force = (world == 1 && (fn || rccl_unique_id)) ? 1 : 0;
    pthread_mutex_unlock(&g_dist_mu);
    return 0;
}
/* snapshot for one qpdo_setup; returns 0, or -1 when the RCCL id of the configuration has already been used */
static int dist_take(QdevDist *out) {
    int rc = 0;
    pthread_mutex_lock(&g_dist_mu);
    *out = g_dist;
    if ((g_dist.world > 1 || g_dist.force) && !g_dist.fn) {
        if (!g_dist_has_id || g_dist_id_spent) rc = -1;
        else g_dist_id_spent = 1;
    }
    pthread_mutex_unlock(&g_dist_mu);
    return rc;
}
int qpdo_amd_dist_unique_id(void *out128) { return qdev_rccl_unique_id(out128); }

static int env_int(const char *name, int dflt) { const char *v = getenv(name); return (v && *v) ? atoi(v) : dflt; }
static double env_double(const char *name, double dflt) { const char *v = getenv(name); return (v && *v) ? atof(v) : dflt; }

static QPDOAmdTraceRec *trace_push(struct QPDOBackend *b) {
    if (b->ntrace == b->captrace) {
        long cap = b->captrace ? 2 * b->captrace : 256;
        QPDOAmdTraceRec *t = realloc(b->trace, (size_t)cap * sizeof(*t));
        if (!t) return NULL;
        b->trace = t; b->captrace = cap;
    }
    QPDOAmdTraceRec *r = &b->trace[b->ntrace++];
    memset(r, 0, sizeof(*r));
    r->factor_branch = -1;
    return r;
}

/* apply this call's Ruiz/cost scaling to the host-side q,l,u mirrors and install the totals */
static int install_scaling(QPDOWorkspace *work) {
    size_t n = work->data->n, m = work->data->m;
    QPDOScaling *sc = work->scaling;
    for (size_t i = 0; i < n; i++) sc->Dinv[i] = (c_float)1.0 / sc->D[i];
    for (size_t i = 0; i < m; i++) sc->Einv[i] = (c_float)1.0 / sc->E[i];
    sc->cinv = (c_float)1.0 / sc->c;
    return qdev_set_scaling(work->chol->dev, 1, sc->D, sc->Dinv, sc->E, sc->Einv, sc->c, sc->cinv);
}

/* small problems: the fused one-launch solve (QPDO_SMALL_FUSED=0 keeps the generic path; an explicit QPDO_LINSOLVE asks for one of the
 * generic path's solvers; a row-partitioned workspace is never small) */
static int small_route_wanted(size_t n, size_t m) {
    const char *ls = getenv("QPDO_LINSOLVE");
    const int want = env_int("QPDO_SMALL_FUSED", 1) && !(ls && *ls && strcmp(ls, "auto"));
    return want && (long)n <= env_int("QPDO_SMALL_FUSED_MAX_N", 160) && qdev_small_resident_fits((int32_t)n, (int32_t)m);
}
static void small_resident_setup(QPDOWorkspace *work, const QPDOSettings *settings) {
    const size_t n = work->data->n, m = work->data->m;
    if (small_route_wanted(n, m)) {
        QdevSmallView v;
        if (qdev_small_view(work->chol->dev, &v) == 0) {
            long cap = (long)settings->max_iter < 16384 ? (long)settings->max_iter : 16384;
            work->chol->small = qdev_small_resident_create(&v, cap);      /* NULL: not fatal, the generic path serves the workspace */
        }
    }
}

/* QPDO_LINSOLVE as the backend's mode: -1 automatic, 0 pcg, 1 dense, 3 band */
static int linsolve_mode_env(void) {
    const char *ls = getenv("QPDO_LINSOLVE");
    if (ls && !strcmp(ls, "pcg")) return 0;
    if (ls && !strcmp(ls, "dense")) return 1;
    if (ls && !strcmp(ls, "band")) return 3;
    return -1;
}
/* the device of this process: QPDO_DEVICE, else LOCAL_RANK, modulo the visible devices.  Returns 0 when there is none: the caller refuses */
#define NO_DEVICE_MSG "no HIP device available (this library has no CPU path)"
static int pick_device(int *device) {
    const int ndev = qdev_device_count();
    if (ndev <= 0) return 0;
    *device = env_int("QPDO_DEVICE", env_int("LOCAL_RANK", 0)) % ndev;
    return 1;
}

/* QPDO_BAND_BORDER=<C> (contract: qpdo_amd_ext.h): a border of trailing coupling variables over a band core, between the creation of the
 * device backend and band_order_setup / qdev_configure.  The detection is band_border.c's; the rule that adopts a border -- 1 <= c <= C and
 * a core that the band solver's selection rule takes on (n_core, b_core) -- is applied here, and qdev_configure finds the decision made.
 * Variable unset or 0: nothing is computed.  Returns 0, or -1 with the message printed. */
static int band_border_setup(QPDOWorkspace *work, const cholmod_sparse *Q, const cholmod_sparse *A, const QdevDist *dd) {
    QPDOAmdBandBorderInfo *bb = &work->chol->band_border;
    memset(bb, 0, sizeof(*bb));
    const int C = env_int("QPDO_BAND_BORDER", 0);
    if (C <= 0) return 0;
    bb->max_border = C > 64 ? 64 : C;
    const int ls = linsolve_mode_env();
    if (dd->world > 1 || dd->force) bb->reason = BAND_BORDER_REASON_PARTITIONED;
    else if (env_int("QPDO_BAND_COUPLING", 0) > 0) bb->reason = BAND_BORDER_REASON_COUPLING;
    else if (small_route_wanted(work->data->n, work->data->m)) bb->reason = BAND_BORDER_REASON_FUSED;
    else if (ls == 0 || ls == 1) bb->reason = BAND_BORDER_REASON_LINSOLVE;
    if (bb->reason) return 0;
    long info[4];
    if (qpdo_amd_band_border(Q, A, bb->max_border, info)) { QPDO_EPRINT("band border: the detection failed (out of memory)"); return -1; }
    bb->n_core = info[0]; bb->b_core = info[2];
    const long c = info[1];
    if (c == 0) return 0;                                                   /* a plain band, or no band at all: as without the variable */
    const int worth = ls == 3 ? bb->n_core >= 4 * (bb->b_core + 1) : (bb->b_core <= 127 && bb->n_core >= 2048);
    if (c > bb->max_border) { bb->over = c; bb->reason = BAND_BORDER_REASON_OVER; }
    else if (!worth) { bb->over = c; bb->reason = BAND_BORDER_REASON_CORE; }
    else bb->border = c;
    if (qdev_set_band_border(work->chol->dev, (int)bb->max_border, (int)bb->n_core, (int)bb->border, (int)bb->b_core, c > bb->max_border ? (int)c : 0)) {
        QPDO_EPRINT("device backend: %s", qdev_last_error()); return -1;
    }
    return 0;
}

/* The band solver's variable order for this workspace (band_order.h; contract: qpdo_amd_ext.h), between the creation of the device
 * backend and qdev_configure, whose band detection and selection rule then run on the adopted order.  Nothing configured: nothing is
 * computed, allocated or launched.  Returns 0, or -1 with the message printed. */
static int band_order_setup(QPDOWorkspace *work, const cholmod_sparse *Q, const cholmod_sparse *A, const QdevDist *dd) {
    QPDOAmdBandOrderInfo *bo = &work->chol->band_order;
    const long n = (long)work->data->n;
    char msg[256] = "";
    int mode = QPDO_AMD_BAND_ORDER_NATURAL, rc = 0;
    int32_t *given = NULL;
    memset(bo, 0, sizeof(*bo));
    bo->b_natural = bo->b_ordered = -1;
    if (band_order_snapshot(n, &mode, &given, msg, sizeof(msg))) { qdev_set_error(msg); QPDO_EPRINT("%s", msg); return -1; }
    bo->mode = mode;
    if (mode == QPDO_AMD_BAND_ORDER_NATURAL) return 0;
    const int ls = linsolve_mode_env();
    if (work->chol->band_border.border > 0) bo->reason = BAND_ORDER_REASON_BORDER;
    else if (dd->world > 1 || dd->force) bo->reason = BAND_ORDER_REASON_PARTITIONED;
    else if (env_int("QPDO_BAND_COUPLING", 0) > 0) bo->reason = BAND_ORDER_REASON_COUPLING;
    else if (small_route_wanted((size_t)n, work->data->m)) bo->reason = BAND_ORDER_REASON_FUSED;
    else if (ls == 0 || ls == 1) bo->reason = BAND_ORDER_REASON_LINSOLVE;
    if (bo->reason) { free(given); return 0; }
    const double t0 = wall_now();
    long *newold = malloc(((size_t)n + 1) * sizeof(long));
    int32_t *no32 = given ? given : malloc(((size_t)n + 1) * sizeof(int32_t)), *oldnew = NULL;
    if (!newold || !no32) { QPDO_EPRINT("band order: out of memory"); free(newold); free(no32); return -1; }
    if (mode == QPDO_AMD_BAND_ORDER_RCM) {
        long info[4];
        if (qpdo_amd_band_order(Q, A, newold, info)) { QPDO_EPRINT("band order: the ordering failed (out of memory)"); rc = -1; }
        for (long k = 0; !rc && k < n; k++) no32[k] = (int32_t)newold[k];
        bo->b_natural = info[0]; bo->b_ordered = info[1];
        bo->adopted = !rc && info[1] < info[0];
        if (!rc && !bo->adopted) bo->reason = BAND_ORDER_REASON_NO_GAIN;
    } else {
        oldnew = malloc(((size_t)n + 1) * sizeof(int32_t));
        if (!oldnew) { QPDO_EPRINT("band order: out of memory"); rc = -1; }
        for (long k = 0; !rc && k < n; k++) oldnew[no32[k]] = (int32_t)k;
        if (!rc) { bo->b_natural = band_order_bandwidth(Q, A, NULL); bo->b_ordered = band_order_bandwidth(Q, A, oldnew); }
        if (!rc && (bo->b_natural < 0 || bo->b_ordered < 0)) { QPDO_EPRINT("band order: out of memory"); rc = -1; }
        bo->adopted = !rc;
    }
    bo->order_seconds = wall_now() - t0;
    if (!rc && qdev_set_band_order(work->chol->dev, bo->adopted ? no32 : NULL, (int)bo->b_natural, (int)bo->b_ordered)) { QPDO_EPRINT("device backend: %s", qdev_last_error()); rc = -1; }
    free(newold); free(no32); free(oldnew);
    return rc;
}

/* The device backend from the three host images: whole on one GPU, or -- a row partition -- this rank's rows [m0, m0+mloc) of A, the
 * same columns of A' and rows [n0, n0+nloc) of Q (cut_row_partition, csc_convert.h; the ranges go into dd). */
static QdevCsr csr_view(const HostCsr *h) { QdevCsr v = {h->nrows, h->ncols, h->nnz, h->rp, h->ci, h->val}; return v; }
static int create_from_host(QPDOWorkspace *work, int device, const HostCsr *Ar, const HostCsr *At, const HostCsr *Qf, QdevDist *dd) {
    const int32_t n = (int32_t)work->data->n, m = (int32_t)work->data->m;
    const QdevCsr a = csr_view(Ar), t = csr_view(At), qf = csr_view(Qf);
    if (dd->world <= 1 && !dd->force)
        return qdev_create(&work->chol->dev, device, n, m, &a, &t, &qf, work->data->q, work->data->l, work->data->u);
    RowPartition P;
    if (cut_row_partition(Ar, At, Qf, dd->rank, dd->world, &P)) return -1;
    dd->m0 = P.m0; dd->mloc = P.mloc; dd->n0 = P.n0; dd->nloc = P.nloc;
    const QdevCsr al = csr_view(&P.Al), tl = csr_view(&P.Tl), ql = csr_view(&P.Ql);
    const int rc = qdev_create_dist(&work->chol->dev, device, n, m, &al, &tl, &qf, &ql, work->data->q, work->data->l, work->data->u, dd);
    row_partition_free(&P);
    return rc;
}

/* scale_data (scaling.c:24-91) for the matrices, q, l, u now on the device: A, Q, q there, l and u through the host mirrors; the
 * totals installed; || Dinv q || (qpdo.c:163-165).  allocate: qpdo_setup -- the scaling arrays are made first, and the unscaled
 * values stay on the device for qpdo_amd_update_matrices (a matrix it is not given is scaled again from them).  An unscaled
 * workspace installs the identity.  Returns 0, -1 with the reason in qdev_last_error(), or 1 when the scaling arrays cannot be allocated. */
static int apply_scaling(QPDOWorkspace *work, int allocate, int prof) {
    const size_t n = work->data->n, m = work->data->m;
    QpdoDev *dev = work->chol->dev;
    if (allocate && work->settings->scaling) {
        QPDOScaling *sc = work->scaling = calloc(1, sizeof(QPDOScaling));
        if (sc) { sc->D = calloc(n ? n : 1, sizeof(c_float)); sc->Dinv = calloc(n ? n : 1, sizeof(c_float)); sc->E = calloc(m ? m : 1, sizeof(c_float)); sc->Einv = calloc(m ? m : 1, sizeof(c_float)); }
        if (!sc || !sc->D || !sc->Dinv || !sc->E || !sc->Einv) return 1;
        if (qdev_keep_raw_values(dev)) return -1;
    }
    QPDOScaling *sc = work->scaling;
    if (!sc) {
        if (qdev_set_scaling(dev, 0, NULL, NULL, NULL, NULL, 1.0, 1.0)) return -1;
        work->norm_q = vec_norm_inf(work->data->q, n);
        return 0;
    }
    const double ts0 = wall_now();
    if (qdev_scale_data(dev, (int)work->settings->scaling, 0, sc->D, sc->E, &sc->c)) return -1;
    if (prof) fprintf(stderr, "[setup] device scaling    %.3f s\n", wall_now() - ts0);
    if (install_scaling(work) || qdev_download_q(dev, work->data->q)) return -1;
    for (size_t i = 0; i < m; i++) { work->data->l[i] = sc->E[i] * work->data->l[i]; work->data->u[i] = sc->E[i] * work->data->u[i]; }
    if (qdev_upload_bounds(dev, work->data->l, work->data->u)) return -1;
    c_float mx = 0.0;
    for (size_t i = 0; i < n; i++) { c_float s = c_absval(sc->Dinv[i] * work->data->q[i]); mx = s > mx ? s : mx; }
    work->norm_q = mx;
    return 0;
}

/* ---- qpdo_setup (reference src/qpdo.c:49-212) ----------------------------------------- */
QPDOWorkspace *qpdo_setup(const QPDOData *data, const QPDOSettings *settings) {
    if (!validate_data(data)) { QPDO_EPRINT("Data validation returned failure"); return QPDO_NULL; }
    if (!validate_settings(settings)) { QPDO_EPRINT("Settings validation returned failure"); return QPDO_NULL; }
    if (!sparse_ok(data->Q) || !sparse_ok(data->A)) { QPDO_EPRINT("unsupported sparse matrix storage"); return QPDO_NULL; }
    if (data->Q->nrow != data->n || data->Q->ncol != data->n || data->A->nrow != data->m || data->A->ncol != data->n) {
        QPDO_EPRINT("matrix dimensions do not match n, m"); return QPDO_NULL;
    }
    QPDOWorkspace *work = calloc(1, sizeof(QPDOWorkspace));
    if (!work) { QPDO_EPRINT("allocating work failure"); return QPDO_NULL; }
    work->timer = malloc(sizeof(QPDOTimer));
    if (!work->timer) { free(work); return QPDO_NULL; }
    tic(work->timer);

    const size_t n = data->n, m = data->m;
    work->settings = copy_settings(settings);
    work->chol = calloc(1, sizeof(struct QPDOBackend));
    work->data = calloc(1, sizeof(QPDOData));
    work->solution = calloc(1, sizeof(QPDOSolution));
    work->info = calloc(1, sizeof(QPDOInfo));
    if (!work->settings || !work->chol || !work->data || !work->solution || !work->info) goto fail;
    work->sqrt_delta = sqrt(work->settings->delta);
    work->sigma = work->settings->sigma_init;
    work->data->n = n; work->data->m = m; work->data->c = data->c;
    work->data->q = vec_dup(data->q, n);
    work->data->l = vec_dup(data->l, m);
    work->data->u = vec_dup(data->u, m);
    work->x = calloc(n ? n : 1, sizeof(c_float));
    work->y = calloc(m ? m : 1, sizeof(c_float));
    work->dx = calloc(n ? n : 1, sizeof(c_float));
    work->dy = calloc(m ? m : 1, sizeof(c_float));
    work->solution->x = calloc(n ? n : 1, sizeof(c_float));
    work->solution->y = calloc(m ? m : 1, sizeof(c_float));
    if (!work->data->q || !work->data->l || !work->data->u || !work->x || !work->y || !work->dx || !work->dy ||
        !work->solution->x || !work->solution->y) goto fail;
    work->initialized = 0;
    work->n_mu_changed = 0;
    work->chol->reset_newton = 1;
    work->chol->fix_status_reset = env_int("QPDO_FIX_STATUS_RESET", 0);
    work->chol->q_raw = vec_dup(data->q, n); work->chol->l_raw = vec_dup(data->l, m); work->chol->u_raw = vec_dup(data->u, m);
    if (!work->chol->q_raw || !work->chol->l_raw || !work->chol->u_raw) goto fail;
    const cholmod_sparse *A = data->A, *Q = data->Q;
    work->chol->q_stype = Q->stype;
    work->chol->q_nnz = idx_at(Q->p, Q->itype, (int64_t)Q->ncol); work->chol->a_nnz = idx_at(A->p, A->itype, (int64_t)A->ncol);

    /* matrices to the device.  One GPU (the default): the caller's CSC arrays are uploaded as they are -- they ARE CSR(A') -- and
     * CSR(A) and the full symmetric CSR(Q) are built on the device (qdev_create_csc: the same arrays, bit for bit, that the host
     * conversions of csc_convert.c produce; QPDO_SETUP_HOST=1 keeps those).  A row-partitioned workspace cuts its slices on the host. */
    const int prof = env_int("QPDO_SETUP_PROF", 0);
    int device;
    QdevDist dd;
    pthread_mutex_lock(&g_dist_mu); dd = g_dist; pthread_mutex_unlock(&g_dist_mu);
    double t0 = wall_now();
    if (dd.world <= 1 && !dd.force && !env_int("QPDO_SETUP_HOST", 0)) {
        if (!pick_device(&device)) { QPDO_EPRINT(NO_DEVICE_MSG); goto fail; }
        QdevCsc a = {(int32_t)A->nrow, (int32_t)A->ncol, work->chol->a_nnz, A->itype, A->p, A->i, (const double *)A->x, 0};
        QdevCsc qq = {(int32_t)Q->nrow, (int32_t)Q->ncol, work->chol->q_nnz, Q->itype, Q->p, Q->i, (const double *)Q->x, Q->stype};
        if (qdev_create_csc(&work->chol->dev, device, (int32_t)n, (int32_t)m, &a, &qq, work->data->q, work->data->l, work->data->u)) goto fail_dev;
        if (prof) fprintf(stderr, "[setup] device create     %.3f s (upload of the CSC arrays, transpositions and slab tables on the device)\n", wall_now() - t0);
    } else {   /* host conversions (row-partitioned workspaces; QPDO_SETUP_HOST=1) */
        HostCsr Ar = {0}, At = {0}, Qf = {0};
        int ok = host_csr_from(A, IMG_CSR, &Ar);
        if (prof) { fprintf(stderr, "[setup] CSR(A)            %.3f s\n", wall_now() - t0); t0 = wall_now(); }
        ok = ok && host_csr_from(A, IMG_CSR_T, &At);
        if (prof) { fprintf(stderr, "[setup] CSR(A') narrowing %.3f s\n", wall_now() - t0); t0 = wall_now(); }
        ok = ok && host_csr_from(Q, IMG_SYM_FULL, &Qf);
        if (prof) { fprintf(stderr, "[setup] full CSR(Q)       %.3f s\n", wall_now() - t0); t0 = wall_now(); }
        if (!ok) { host_csr_free(&Ar); host_csr_free(&At); host_csr_free(&Qf); QPDO_EPRINT("matrix conversion failed"); goto fail; }
        if (!pick_device(&device)) { host_csr_free(&Ar); host_csr_free(&At); host_csr_free(&Qf); QPDO_EPRINT(NO_DEVICE_MSG); goto fail; }
        if (dist_take(&dd)) {
            host_csr_free(&Ar); host_csr_free(&At); host_csr_free(&Qf);
            QPDO_EPRINT("the RCCL unique id of qpdo_amd_dist_config has already created a communicator: call qpdo_amd_dist_config "
                        "with a fresh id before setting up another row-partitioned workspace"); goto fail;
        }
        const int rc = create_from_host(work, device, &Ar, &At, &Qf, &dd);
        if (prof) { fprintf(stderr, "[setup] device create     %.3f s (upload, slab tables)\n", wall_now() - t0); t0 = wall_now(); }
        host_csr_free_async(&Ar, &At, &Qf);       /* unmapping several GB takes ~0.5 s: off the caller's path */
        if (prof) { fprintf(stderr, "[setup] host free         %.3f s\n", wall_now() - t0); }
        if (rc) goto fail_dev;
    }
    if (band_border_setup(work, Q, A, &dd)) goto fail;
    if (band_order_setup(work, Q, A, &dd)) goto fail;
    if (qdev_configure(work->chol->dev, linsolve_mode_env(), env_double("QPDO_PCG_TOL", 0.0), env_int("QPDO_PCG_MAXIT", 0))) goto fail_dev;
    const int scaled = apply_scaling(work, 1, prof);
    if (scaled < 0) goto fail_dev;
    if (scaled) goto fail;
    small_resident_setup(work, settings);
    update_status(work->info, QPDO_UNSOLVED);
    work->info->solve_time = 0.0;
    work->info->run_time = 0.0;
    work->info->setup_time = toc(work->timer);
    return work;

fail_dev:
    QPDO_EPRINT("device backend: %s", qdev_last_error());
fail:
    qpdo_cleanup(work);
    return QPDO_NULL;
}

/* ---- qpdo_warm_start (reference src/qpdo.c:217-299) --------------------------------------- */
void qpdo_warm_start(QPDOWorkspace *work, c_float *x_warm_start, c_float *y_warm_start) {
    work->chol->solved_last = 0;
    work->sigma = work->settings->sigma_init;
    if (work->info->status_val != QPDO_UNSOLVED) work->info->setup_time = 0;
    tic(work->timer);
    c_float obj = 0.0;
    if (work->chol->small && work->chol->auto_ws && !work->settings->verbose) {
        /* qpdo_solve's automatic warm start (qpdo.c:312-314, x = y = 0) of a fused-path workspace: nothing can come between it and the
         * solve, so it is part of the solve's one launch -- nothing to do on the device here */
        work->chol->ws_state = 0;
        work->info->objective = 0.0;
        work->sqrt_mu_min = 1 / sqrt(work->settings->mu_min);
        work->initialized = 1;
        work->info->setup_time += toc(work->timer);
        return;
    }
    if (work->chol->small) {
        /* an explicit warm start of a fused-path workspace: x, x_bar, Qx, Ax, y, y_bar, A'y, mu in the ORACLE's operation order (one
         * workgroup, qpdo_small.hip mode 1) into the workspace's device vectors; qpdo_update_q / _bounds may then act on them as in the
         * reference before the solve reads them back (mode 2) */
        QdevSmallView v;
        if (qdev_small_view(work->chol->dev, &v) ||
            qdev_small_resident_warm_start(work->chol->small, &v, work->settings, x_warm_start, y_warm_start, work->data->c, &obj)) {
            QPDO_EPRINT("fused small-problem warm start: %s / %s", qdev_small_last_error(), qdev_last_error()); update_status(work->info, QPDO_ERROR); return;
        }
        work->chol->ws_state = 1;
        work->info->objective = x_warm_start ? obj : 0.0;
        work->sqrt_mu_min = 1 / sqrt(work->settings->mu_min);
        work->initialized = 1;
        work->info->setup_time += toc(work->timer);
        return;
    }
    int rc = qdev_warm_start(work->chol->dev, x_warm_start, y_warm_start, (int)work->settings->proximal, work->sigma,
                             work->settings->mu_min, work->data->c, &obj);
    if (rc) { QPDO_EPRINT("device backend: %s", qdev_last_error()); update_status(work->info, QPDO_ERROR); return; }
    work->chol->ws_state = 1;
    work->info->objective = x_warm_start ? obj : 0.0;
    work->sqrt_mu_min = 1 / sqrt(work->settings->mu_min);      /* iteration.c:121 */
    work->initialized = 1;
    work->info->setup_time += toc(work->timer);
}

/* reference src/util.c:101-117 */
static void print_header(void) {
    QPDO_PRINT("============================================================================\n");
    QPDO_PRINT("===                    QPDO  v0.1  (MI355X-native backend)               ===\n");
    QPDO_PRINT("============================================================================\n");
    QPDO_PRINT("  iter |  objective     r.prim     r.dual |  r.p. in    r.d. in   stepsize | \n");
    QPDO_PRINT("============================================================================\n");
}
static void print_iteration(c_int iter, QPDOWorkspace *work) {
    QPDO_PRINT("%6ld | %+-.3e   %.2e   %.2e | %.2e   %.2e   %.2e | \n", (long)iter, work->info->objective, work->info->res_prim_norm,
               work->info->res_dual_norm, work->info->res_prim_in_norm, work->info->res_dual_in_norm, work->tau);
}
static void print_final_message(QPDOWorkspace *work) {   /* src/util.c:122-173 */
    const char *msg;
    switch (work->info->status_val) {
        case QPDO_SOLVED: msg = "QPDO finished successfully."; break;
        case QPDO_PRIMAL_INFEASIBLE: msg = "QPDO detected a primal infeasible problem."; break;
        case QPDO_DUAL_INFEASIBLE: msg = "QPDO detected a dual infeasible problem."; break;
        case QPDO_PRIMAL_DUAL_INFEASIBLE: msg = "QPDO detected a primal-dual infeasible problem."; break;
        case QPDO_MAX_ITER_REACHED: msg = "QPDO hit the maximum number of iterations."; break;
        case QPDO_MAX_TIME_REACHED: msg = "QPDO exceeded the specified time limit."; break;
        default: msg = "QPDO ended with an unrecognised status."; break;
    }
    QPDO_PRINT("============================================================================\n");
    QPDO_PRINT("| %-72s |\n", msg);
    QPDO_PRINT("| primal residual: %5.4e,                primal tolerance: %5.4e |\n", work->info->res_prim_norm, work->settings->eps_abs);
    QPDO_PRINT("| dual residual  : %5.4e,                dual tolerance  : %5.4e |\n", work->info->res_dual_norm, work->settings->eps_abs);
    QPDO_PRINT("| objective value: %+-5.4e                                             |\n", work->info->objective);
    if (work->info->run_time > 1.0) QPDO_PRINT("| runtime:         %4.2f seconds\n", work->info->run_time);
    else QPDO_PRINT("| runtime:         %4.2f milliseconds\n", work->info->run_time * 1000);
    QPDO_PRINT("============================================================================\n\n");
}

/* ---- qpdo_solve of a small workspace: ONE launch of the fused kernel (qpdo_small.hip) on the workspace's device arrays --------------
 * Same loop (src/qpdo.c:343-449) in the oracle's operation order, so status, counts and iterates carry the oracle's bits.  Called by
 * qpdo_solve after its prologue (header, automatic warm start, eps_in / sigma / reset_newton, status quirk Q1, tic, trace reset). */
static void fused_solve(QPDOWorkspace *work) {
    struct QPDOBackend *be = work->chol;
    QPDOSettings st = *work->settings;
    QdevSmallView v;
    QdevSmallResult res;
    QPDOInfo kinfo;
    memset(&res, 0, sizeof(res)); memset(&kinfo, 0, sizeof(kinfo));
    res.info = &kinfo;
    /* max_time (qpdo.c:441-447) counts from the start of setup: run_time = setup_time + time in the solve; the kernel's clock starts now */
    if (st.max_time < 1e19) st.max_time -= work->info->setup_time;
    const c_int status_before = work->info->status_val;
    if (qdev_small_view(be->dev, &v) ||
        qdev_small_resident_solve(be->small, &v, &st, be->ws_state, work->data->c, &res)) {
        QPDO_EPRINT("fused small-problem solve: %s / %s", qdev_small_last_error(), qdev_last_error());
        update_status(work->info, QPDO_ERROR);
        work->initialized = 0;
        work->info->solve_time = toc(work->timer);
        work->info->run_time = work->info->setup_time + work->info->solve_time;
        return;
    }
    const size_t n = work->data->n, m = work->data->m;
    work->info->iterations = kinfo.iterations; work->info->oterations = kinfo.oterations;
    work->info->res_prim_norm = kinfo.res_prim_norm; work->info->res_dual_norm = kinfo.res_dual_norm;
    work->info->res_prim_in_norm = kinfo.res_prim_in_norm; work->info->res_dual_in_norm = kinfo.res_dual_in_norm;
    work->info->objective = kinfo.objective;
    /* quirk Q1 (qpdo.c:451-453): only an UNSOLVED status is overwritten when the loop runs out of passes */
    if (kinfo.status_val == QPDO_MAX_ITER_REACHED) { if (status_before == QPDO_UNSOLVED || be->fix_status_reset) update_status(work->info, QPDO_MAX_ITER_REACHED); }
    else update_status(work->info, kinfo.status_val);
    work->sigma = res.sigma_end; work->tau = res.tau_end;
    memcpy(work->solution->x, res.sol_x, n * sizeof(c_float)); memcpy(work->x, res.x, n * sizeof(c_float)); memcpy(work->dx, res.dx, n * sizeof(c_float));
    if (m) { memcpy(work->solution->y, res.sol_y, m * sizeof(c_float)); memcpy(work->y, res.y, m * sizeof(c_float)); memcpy(work->dy, res.dy, m * sizeof(c_float)); }
    be->newton_passes = res.newton_passes; be->last_fused = 1; be->fused_solves++; be->fused_factor_count = res.factor_count; be->fused_kernel_s = res.kernel_seconds;
    /* the per-pass trace (pinned records written by the kernel) into the workspace's trace array */
    if (res.ntrace > be->captrace) {
        QPDOAmdTraceRec *t = realloc(be->trace, (size_t)res.ntrace * sizeof(*t));
        if (t) { be->trace = t; be->captrace = res.ntrace; }
    }
    be->ntrace = res.ntrace <= be->captrace ? res.ntrace : be->captrace;
    if (be->ntrace > 0) memcpy(be->trace, res.trace, (size_t)be->ntrace * sizeof(QPDOAmdTraceRec));
    work->initialized = 0;
    work->info->solve_time = toc(work->timer);
    work->info->run_time = work->info->setup_time + work->info->solve_time;
}

#define DEVCALL(call) do { if ((call)) { QPDO_EPRINT("device backend: %s", qdev_last_error()); update_status(work->info, QPDO_ERROR); goto done; } } while (0)

/* ---- qpdo_solve (reference src/qpdo.c:304-476) ---------------------------------------------- */
void qpdo_solve(QPDOWorkspace *work) {
    struct QPDOBackend *be = work->chol;
    QpdoDev *dev = be->dev;
    const QPDOSettings *s;
    if (work->settings->verbose) print_header();
    if (!work->initialized) { be->auto_ws = 1; qpdo_warm_start(work, NULL, NULL); be->auto_ws = 0; }
    be->solved_last = 1;
    s = work->settings;
    const int prox = (int)s->proximal;
    work->eps_in = s->eps_abs_in;
    work->sigma = s->sigma_init;
    be->reset_newton = 1;
    if (be->fix_status_reset) update_status(work->info, QPDO_UNSOLVED);
    tic(work->timer);
    be->ntrace = 0; be->newton_passes = 0; be->last_fused = 0;
    qdev_reset_stats(dev);
    c_int iter = 0, oter = 0, iter_old = 0;
    long tr_pending = -1;           /* index of the trace record whose tau is still in flight (deferred step read-back) */
    c_int last_nchange = -1;        /* n_enter + n_leave of the last Newton pass (-1: none yet / an outer update came after it) */
    if (!work->initialized) goto done;      /* warm start failed on the device */
    if (be->small && !s->verbose) { fused_solve(work); return; }
    if (!be->ws_state) {                    /* (cannot happen: the automatic cold start is skipped only when this solve takes the fused path) */
        c_float obj0 = 0.0;
        DEVCALL(qdev_warm_start(dev, NULL, NULL, prox, work->sigma, s->mu_min, work->data->c, &obj0));
        be->ws_state = 1;
    }
    DEVCALL(qdev_begin_solve(dev));
    DEVCALL(qdev_set_eps_abs(dev, s->eps_abs));
    /* One host synchronisation per loop pass instead of two (dense solver; QPDO_DEFER_STEP=0 switches it off): the Newton step is
     * launched without waiting for it; its step length -- needed only by the trace, the iteration line and is_dual_infeasible -- comes
     * back with the next pass's residual norms.  Printing wants tau on the pass's own line, so verbose solves keep two. */
    DEVCALL(qdev_set_deferred_step(dev, !s->verbose && env_int("QPDO_DEFER_STEP", 1)));

    for (iter = 0; iter < s->max_iter; iter++) {
        QdevResid r;
        /* launch-ahead (qpdo_dev.h qdev_residuals_ahead): on the mid-size dense route this pass's Newton step is enqueued behind the
         * residual launch, which forms the decisions below on the device from what the host knows now; the host still makes them itself
         * from the norms it reads back, and any disagreement ends the solve with QPDO_ERROR */
        QdevAhead ah;
        ah.allow_outer = iter > iter_old + 1; ah.force_outer = (iter == iter_old + s->inner_max_iter);
        ah.reset_newton = be->reset_newton || (s->reset_newton_iter > 0 && (iter % s->reset_newton_iter == 0));
        ah.max_rank = QPDO_MAX_RANK_UPDATE; ah.eps_abs = s->eps_abs; ah.eps_in = work->eps_in; ah.infty = QPDO_INFTY;
        /* (not when the last Newton pass saw no row enter or leave and nothing forces a new factorization: the active set tends to
         * stand still then, the host-first path keeps its factor on such a pass and the launched-ahead step would refactor) */
        const int ahead_ok = !s->verbose && (ah.reset_newton || last_nchange != 0);
        DEVCALL(qdev_residuals_ahead(dev, prox, work->sigma, ahead_ok ? &ah : NULL, &r));
        if (r.prev_step_done) {
            work->tau = r.prev_tau;
            if (tr_pending >= 0 && tr_pending < be->ntrace) be->trace[tr_pending].tau = r.prev_tau;
            tr_pending = -1;
        }
        work->info->res_prim_norm = r.res_prim; work->info->res_dual_norm = r.res_dual;
        work->info->res_prim_in_norm = r.res_prim_in; work->info->res_dual_in_norm = r.res_dual_in;
        QPDOAmdTraceRec *tr = trace_push(be);
        if (tr) {
            tr->kind = 2; tr->res_prim = r.res_prim; tr->res_dual = r.res_dual; tr->res_prim_in = r.res_prim_in;
            tr->res_dual_in = r.res_dual_in; tr->sigma = work->sigma; tr->eps_in = work->eps_in;
        }
        if (s->verbose && (s->print_interval > 0) && (iter % s->print_interval == 0)) {
            DEVCALL(qdev_objective(dev, prox, work->sigma, work->data->c, &work->info->objective));
            print_iteration(iter, work);
        }
        /* check_outer_optimality (termination.c:11-23) */
        /* (pass_decision.h: termination.c:11-30, qpdo.c:361-363, newton.c:21-33 -- the function the residual launch itself evaluates on the
         * launch-ahead route, on the same numbers) */
        const QpdoPassDecision pd = qpdo_pass_decision(r.res_prim, r.res_dual, r.res_prim_in, r.res_dual_in, s->eps_abs, work->eps_in, QPDO_INFTY,
                                                       ah.allow_outer, ah.force_outer, ah.reset_newton, (int)r.n_active, (int)(r.n_enter + r.n_leave),
                                                       QPDO_MAX_RANK_UPDATE);
        const int ends_nc = pd.ends_nc, ends_ok = pd.ends_ok, outer_pass = pd.outer;
        if (r.ahead_went && (ends_nc || ends_ok || outer_pass)) {
            QPDO_EPRINT("launch-ahead: the device started a Newton step in pass %ld, which the host ends or makes an outer update", (long)iter);
            update_status(work->info, QPDO_ERROR); break;
        }
        if (ends_nc) { update_status(work->info, QPDO_NON_CVX); break; }
        if (ends_ok) { update_status(work->info, QPDO_SOLVED); break; }

        if (outer_pass) {
            if (tr) tr->kind = 1;
            if (iter < iter_old + s->inner_max_iter) {
                if (s->eps_prim_inf > 0) {
                    int inf = 0;
                    DEVCALL(qdev_primal_infeasibility(dev, s->eps_prim_inf, &inf));
                    if (inf) { update_status(work->info, QPDO_PRIMAL_INFEASIBLE); break; }
                }
            }
            /* is_dual_infeasible and update_mu (iteration.c:127-168) share one read-back: update_mu is enqueued behind the test and does
             * nothing if the test says "infeasible" (update_mu does not look at x_bar / y_bar, so running it before the estimates are
             * shifted changes nothing) */
            const int do_dinf = (iter < iter_old + s->inner_max_iter) && (s->eps_dual_inf > 0);
            const int do_mu = (oter > 0) && (r.res_prim > s->eps_abs);
            int dinf = 0, nch = 0;
            DEVCALL(qdev_dual_infeasibility_and_mu(dev, do_dinf, prox, work->sigma, work->tau, s->eps_dual_inf, do_mu, s->eps_abs, s->theta,
                                                   s->delta, s->mu_min, work->sqrt_mu_min, &dinf, &nch));
            if (dinf) { update_status(work->info, QPDO_DUAL_INFEASIBLE); break; }
            DEVCALL(qdev_shift_estimates(dev));
            if (do_mu) {
                work->n_mu_changed = nch;
                if ((prox && work->sigma > s->sigma_min) || (nch > 0.25 * QPDO_MAX_RANK_UPDATE)) be->reset_newton = 1;
                else if (nch == 0) { /* nothing */ }
                else DEVCALL(qdev_mu_changed_update(dev));
            }
            if (prox && (oter > 0) && (r.res_dual > s->eps_abs)) {
                /* update_sigma (iteration.c:173-180) */
                if (work->sigma > s->sigma_min) {
                    c_float sigma_old = work->sigma;
                    work->sigma = c_max(work->sigma * s->sigma_upd, s->sigma_min);
                    be->reset_newton = 1;
                    DEVCALL(qdev_update_sigma(dev, work->sigma, sigma_old));
                }
            }
            if (iter < iter_old + s->inner_max_iter) {
                work->eps_in = c_max(s->rho * work->eps_in, 0.1 * s->eps_abs);
                if (s->verbose && (s->print_interval > 0) && (iter % s->print_interval == 0))
                    QPDO_PRINT("%6ld |-------------------------------------------------------------------|\n", (long)iter);
            } else if (s->verbose && (s->print_interval > 0) && (iter % s->print_interval == 0)) {
                QPDO_PRINT("%6ld |--  --  --  --  --  --  --  --  --  --  --  --  --  --  --  --  -- |\n", (long)iter);
            }
            DEVCALL(qdev_save_res_prim(dev));
            oter++;
            iter_old = iter;
            last_nchange = -1;
        } else {
            if (tr) tr->kind = 0;
            /* the reference computes iter % reset_newton_iter, a division by zero for the (valid) setting 0;
             * here 0 means "no periodic refactorization" */
            if (s->reset_newton_iter > 0 && (iter % s->reset_newton_iter == 0)) be->reset_newton = 1;
            /* factorization decision (newton.c:21-33) */
            const int branch = pd.branch;          /* (ah.reset_newton is be->reset_newton after the line above) */
            if (branch == 0) be->reset_newton = 0;
            int lin = 0;
            DEVCALL(qdev_newton_step(dev, branch, r.n_enter + r.n_leave, prox, work->sigma, &work->tau, &lin));
            be->newton_passes++;
            last_nchange = r.n_enter + r.n_leave;
            if (tr && work->tau != work->tau) tr_pending = be->ntrace - 1;        /* NaN: the step's read-back is deferred */
            if (tr) { tr->tau = work->tau; tr->n_active = r.n_active; tr->n_enter = r.n_enter; tr->n_leave = r.n_leave; tr->factor_branch = branch; tr->lin_iters = lin; }
        }
        work->info->run_time = work->info->setup_time + toc(work->timer);
        if (work->info->run_time > s->max_time) { update_status(work->info, QPDO_MAX_TIME_REACHED); break; }
    }
    if (work->info->status_val == QPDO_UNSOLVED) update_status(work->info, QPDO_MAX_ITER_REACHED);

done:
    {   /* a Newton step still in flight (loop left by max_iter / max_time right after it): complete it before the solution is stored */
        int had = 0; c_float tau_last = 0.0;
        if (qdev_finish_step(dev, &had, &tau_last)) { QPDO_EPRINT("device backend: %s", qdev_last_error()); update_status(work->info, QPDO_ERROR); }
        else if (had) { work->tau = tau_last; if (tr_pending >= 0 && tr_pending < be->ntrace) be->trace[tr_pending].tau = tau_last; }
    }
    work->info->iterations = iter;
    work->info->oterations = oter;
    /* store_solution (termination.c:82-92) + host mirrors */
    if (qdev_store_solution_obj(dev, prox, work->sigma, work->data->c, work->solution->x, work->solution->y, work->x, work->y, work->dx, work->dy,
                                &work->info->objective)) {
        QPDO_EPRINT("device backend: %s", qdev_last_error());
        update_status(work->info, QPDO_ERROR);
    }
    work->initialized = 0;
    work->info->solve_time = toc(work->timer);
    work->info->run_time = work->info->setup_time + work->info->solve_time;
    if (work->settings->verbose) {
        if (work->settings->print_interval > 0 && (iter % work->settings->print_interval != 0)) print_iteration(iter, work);
        print_final_message(work);
    }
}

/* ---- qpdo_update_settings (reference src/qpdo.c:481-517) --------------------------------------- */
void qpdo_update_settings(QPDOWorkspace *work, const QPDOSettings *settings) {
    if (!validate_settings(settings)) {
        QPDO_EPRINT("Settings validation returned failure");
        update_status(work->info, QPDO_ERROR);
        return;
    }
    if (work->settings->scaling > settings->scaling) {
        QPDO_EPRINT("Decreasing the number of scaling iterations is not allowed");
        update_status(work->info, QPDO_ERROR);
        return;
    } else if (work->settings->scaling < settings->scaling) {
        if (!work->scaling) {   /* the reference dereferences NULL here (qpdo.c:496-499) */
            QPDO_EPRINT("scaling cannot be enabled after setup");
            update_status(work->info, QPDO_ERROR);
            return;
        }
        size_t n = work->data->n, m = work->data->m;
        c_float *Dsave = vec_dup(work->scaling->D, n), *Esave = vec_dup(work->scaling->E, m);
        c_float c_temp = work->scaling->c, c_new = 1.0;
        if (!Dsave || !Esave || qdev_scale_data(work->chol->dev, (int)(settings->scaling - work->settings->scaling), 1,
                                                 work->scaling->D, work->scaling->E, &c_new)) {
            free(Dsave); free(Esave);
            update_status(work->info, QPDO_ERROR);
            return;
        }
        /* bounds: l,u <- E_new .* l,u on the host mirrors (scaling.c:86-87) */
        for (size_t i = 0; i < m; i++) { work->data->l[i] = work->scaling->E[i] * work->data->l[i]; work->data->u[i] = work->scaling->E[i] * work->data->u[i]; }
        for (size_t i = 0; i < n; i++) work->scaling->D[i] = work->scaling->D[i] * Dsave[i];
        for (size_t i = 0; i < m; i++) work->scaling->E[i] = work->scaling->E[i] * Esave[i];
        work->scaling->c = c_new * c_temp;
        free(Dsave); free(Esave);
        if (install_scaling(work) || qdev_download_q(work->chol->dev, work->data->q) ||
            qdev_upload_bounds(work->chol->dev, work->data->l, work->data->u)) {
            update_status(work->info, QPDO_ERROR);
            return;
        }
    }
    free(work->settings);
    work->settings = copy_settings(settings);
    work->sqrt_delta = sqrt(work->settings->delta);
}

/* ---- qpdo_update_bounds (reference src/qpdo.c:522-544) ------------------------------------------ */
void qpdo_update_bounds(QPDOWorkspace *work, const c_float *l, const c_float *u) {
    size_t m = work->data->m;
    work->chol->solved_last = 0;
    if (l != NULL && u != NULL) {
        for (size_t j = 0; j < m; j++) {
            if (l[j] > u[j]) {
                QPDO_EPRINT("Lower bound at index %d is greater than upper bound: %.4e > %.4e", (int)j, l[j], u[j]);
                update_status(work->info, QPDO_ERROR);
                return;
            }
        }
    }
    if (l != NULL) { memcpy(work->data->l, l, m * sizeof(c_float)); memcpy(work->chol->l_raw, l, m * sizeof(c_float)); }
    if (u != NULL) { memcpy(work->data->u, u, m * sizeof(c_float)); memcpy(work->chol->u_raw, u, m * sizeof(c_float)); }
    if (work->settings->scaling) {
        if (l != NULL) for (size_t i = 0; i < m; i++) work->data->l[i] = work->scaling->E[i] * work->data->l[i];
        if (u != NULL) for (size_t i = 0; i < m; i++) work->data->u[i] = work->scaling->E[i] * work->data->u[i];
    }
    if (qdev_upload_bounds(work->chol->dev, l ? work->data->l : NULL, u ? work->data->u : NULL)) update_status(work->info, QPDO_ERROR);
}

/* ---- qpdo_update_q (reference src/qpdo.c:549-586) ------------------------------------------------- */
void qpdo_update_q(QPDOWorkspace *work, const c_float *q) {
    size_t n = work->data->n;
    QpdoDev *dev = work->chol->dev;
    work->chol->solved_last = 0;
    memcpy(work->data->q, q, n * sizeof(c_float));
    memcpy(work->chol->q_raw, q, n * sizeof(c_float));
    if (work->settings->scaling) {
        /* device side (round 3): Qx and x stay in HBM; the host receives the new cost scaling c and norm_q only and keeps its copy
         * of the scaled q (work->data->q) in step by reading it back -- n doubles, instead of 2n down + 5n up before */
        c_float c_new = 1.0, cinv_new = 1.0, nq = 0.0;
        const c_float sigma_new = work->settings->proximal ? work->settings->sigma_init : work->sigma;
        if (qdev_update_q_scaled(dev, q, (int)work->settings->proximal, work->sigma, sigma_new, work->scaling->c, &c_new, &cinv_new, &nq) ||
            qdev_download_q(dev, work->data->q)) { update_status(work->info, QPDO_ERROR); return; }
        work->scaling->c = c_new; work->scaling->cinv = cinv_new;
        if (work->settings->proximal) work->sigma = work->settings->sigma_init;
        work->norm_q = nq;
    } else {
        if (qdev_upload_q(dev, work->data->q)) update_status(work->info, QPDO_ERROR);
        work->norm_q = vec_norm_inf(work->data->q, n);
    }
}

/* ---- qpdo_amd_update_matrices (include/qpdo_amd_ext.h) ----------------------------------------------------------
 * New values of Q and / or A in the setup's pattern.  Afterwards the workspace is the one qpdo_setup would return for the new matrices,
 * the latest unscaled q, l, u, the constant c and the current settings: the scaling is computed again from scratch (the raw values of a
 * matrix passed as NULL are kept on the device), every iterate and factor state goes back to its post-setup value. */
static int update_refuse(const char *msg) { qdev_set_error(msg); return -1; }
int qpdo_amd_update_matrices(QPDOWorkspace *work, const cholmod_sparse *Q, const cholmod_sparse *A) {
    if (!work || !work->chol || !work->chol->dev || !work->data) return update_refuse("qpdo_amd_update_matrices: NULL workspace");
    struct QPDOBackend *be = work->chol;
    const size_t n = work->data->n, m = work->data->m;
    if (Q && !sparse_ok(Q)) return update_refuse("qpdo_amd_update_matrices: unsupported sparse storage of Q");
    if (A && !sparse_ok(A)) return update_refuse("qpdo_amd_update_matrices: unsupported sparse storage of A");
    if (Q && (Q->nrow != n || Q->ncol != n)) return update_refuse("qpdo_amd_update_matrices: Q is not n x n");
    if (A && (A->nrow != m || A->ncol != n)) return update_refuse("qpdo_amd_update_matrices: A is not m x n");
    if (Q && Q->stype != be->q_stype) return update_refuse("qpdo_amd_update_matrices: Q has another stype than at setup");
    if (Q && idx_at(Q->p, Q->itype, (int64_t)n) != be->q_nnz) return update_refuse("qpdo_amd_update_matrices: Q has another number of entries than at setup");
    if (A && idx_at(A->p, A->itype, (int64_t)n) != be->a_nnz) return update_refuse("qpdo_amd_update_matrices: A has another number of entries than at setup");
    QPDOTimer t; tic(&t);
    QdevCsc a, qq;
    if (A) { QdevCsc v = {(int32_t)A->nrow, (int32_t)A->ncol, be->a_nnz, A->itype, A->p, A->i, (const double *)A->x, 0}; a = v; }
    if (Q) { QdevCsc v = {(int32_t)Q->nrow, (int32_t)Q->ncol, be->q_nnz, Q->itype, Q->p, Q->i, (const double *)Q->x, Q->stype}; qq = v; }
    /* the device checks the pattern (and refuses a row-partitioned workspace) before it writes anything */
    const int rc = qdev_update_matrices(be->dev, A ? &a : NULL, Q ? &qq : NULL, be->q_raw, be->l_raw, be->u_raw);
    if (rc) return rc;
    be->solved_last = 0;
    /* from here on, as qpdo_setup: the host mirrors, the scaling, the fused resident, the post-setup scalars */
    memcpy(work->data->q, be->q_raw, n * sizeof(c_float));
    if (m) { memcpy(work->data->l, be->l_raw, m * sizeof(c_float)); memcpy(work->data->u, be->u_raw, m * sizeof(c_float)); }
    const int fail = apply_scaling(work, 0, 0);
    if (n) { memset(work->x, 0, n * sizeof(c_float)); memset(work->dx, 0, n * sizeof(c_float)); memset(work->solution->x, 0, n * sizeof(c_float)); }
    if (m) { memset(work->y, 0, m * sizeof(c_float)); memset(work->dy, 0, m * sizeof(c_float)); memset(work->solution->y, 0, m * sizeof(c_float)); }
    work->initialized = 0; work->n_mu_changed = 0; work->sigma = work->settings->sigma_init; work->tau = 0.0;
    work->eps_in = 0.0; work->sqrt_mu_min = 0.0;
    be->reset_newton = 1; be->ws_state = 0; be->auto_ws = 0; be->ntrace = 0; be->newton_passes = 0;
    be->fused_solves = 0; be->fused_factor_count = 0; be->fused_kernel_s = 0.0; be->last_fused = 0;
    /* the fused resident is rebuilt rather than proven clean (its arena holds the last solve's factor and iterates) */
    qdev_small_resident_destroy(be->small); be->small = NULL;
    if (!fail) small_resident_setup(work, work->settings);
    memset(work->info, 0, sizeof(*work->info));
    update_status(work->info, fail ? QPDO_ERROR : QPDO_UNSOLVED);
    work->info->setup_time = toc(&t);
    if (fail) { QPDO_EPRINT("device backend: %s", qdev_last_error()); return -1; }
    return 0;
}

/* ---- qpdo_cleanup (reference src/qpdo.c:591-689) ---------------------------------------------------- */
void qpdo_cleanup(QPDOWorkspace *work) {
    if (!work) return;
    if (work->data) { free(work->data->q); free(work->data->l); free(work->data->u); free(work->data); }
    if (work->scaling) { free(work->scaling->D); free(work->scaling->Dinv); free(work->scaling->E); free(work->scaling->Einv); free(work->scaling); }
    free(work->x); free(work->y); free(work->dx); free(work->dy);
    free(work->settings);
    if (work->chol) {
        qdev_small_resident_destroy(work->chol->small); qdev_destroy(work->chol->dev); free(work->chol->trace);
        free(work->chol->q_raw); free(work->chol->l_raw); free(work->chol->u_raw); free(work->chol);
    }
    if (work->solution) { free(work->solution->x); free(work->solution->y); free(work->solution); }
    free(work->timer);
    free(work->info);
    free(work);
}

/* ---- extensions (include/qpdo_amd_ext.h) --------------------------------------------------------------- */
int qpdo_amd_device_count(void) { return qdev_device_count(); }
int qpdo_amd_pass_decision(double res_prim, double res_dual, double res_prim_in, double res_dual_in, double eps_abs, double eps_in, int allow_outer,
                           int force_outer, int reset_newton, int n_active, int n_change, int *ends_nc, int *ends_ok, int *outer, int *branch) {
    const QpdoPassDecision pd = qpdo_pass_decision(res_prim, res_dual, res_prim_in, res_dual_in, eps_abs, eps_in, QPDO_INFTY, allow_outer, force_outer,
                                                   reset_newton, n_active, n_change, QPDO_MAX_RANK_UPDATE);
    *ends_nc = pd.ends_nc; *ends_ok = pd.ends_ok; *outer = pd.outer; *branch = pd.branch;
    return 0;
}
const char *qpdo_amd_last_error(void) { return qdev_last_error(); }
int qpdo_amd_sync(QPDOWorkspace *work) { return qdev_sync(work->chol->dev); }
int qpdo_amd_get_trace(const QPDOWorkspace *work, const QPDOAmdTraceRec **recs, long *count) {
    *recs = work->chol->trace; *count = work->chol->ntrace; return 0;
}
int qpdo_amd_bench_spmv(QPDOWorkspace *work, int which, int reps, double *avg_seconds, double *alg_bytes) {
    return qdev_bench_spmv(work->chol->dev, which, reps, avg_seconds, alg_bytes);
}
int qpdo_amd_bench_dense_factor(QPDOWorkspace *work, int reps, double *avg_seconds, double *check) {
    return qdev_bench_dense_factor(work->chol->dev, reps, avg_seconds, check);
}
int qpdo_amd_spmv(QPDOWorkspace *work, int which, const double *v, double *y) { return qdev_spmv(work->chol->dev, which, v, y); }
int qpdo_amd_linesearch(QPDOWorkspace *work, double eta, double beta, const double *delta, const double *alpha, double *tau) {
    return qdev_linesearch(work->chol->dev, eta, beta, delta, alpha, tau);
}
int qpdo_amd_direct_solve(QPDOWorkspace *work, const double *dw, double sigma, const double *rhs, double *x, int flags) {
    const int rc = qdev_direct_solve(work->chol->dev, dw, sigma, rhs, x, flags);
    return rc == QDEV_DIRECT_LOST ? QPDO_AMD_DIRECT_LOST : rc ? -1 : 0;
}
int qpdo_amd_get_band_order(const QPDOWorkspace *work, QPDOAmdBandOrderInfo *out, long *newold) {
    if (!work || !work->chol || !out) return -1;
    *out = work->chol->band_order;
    if (newold && out->adopted) {
        const size_t n = work->data->n;
        int32_t *no = malloc((n + 1) * sizeof(int32_t));
        if (!no || qdev_band_order_newold(work->chol->dev, no)) { free(no); return -1; }
        for (size_t k = 0; k < n; k++) newold[k] = no[k];
        free(no);
    }
    return 0;
}
int qpdo_amd_get_band_border(const QPDOWorkspace *work, QPDOAmdBandBorderInfo *out) {
    if (!work || !work->chol || !work->chol->dev || !out) return -1;
    QdevStats st;
    qdev_get_stats(work->chol->dev, &st);
    *out = work->chol->band_border;
    out->border_solves = (long)st.border_solves;
    return 0;
}
int qpdo_amd_download_factor(QPDOWorkspace *work, int which, double *dst, long count) {
    return qdev_download_factor(work->chol->dev, which, dst, count) ? -1 : 0;
}
/* ---- qpdo_amd_adjoint (include/qpdo_amd_ext.h): the argument checks, in the header's order, before the backend is touched
 * (tests/adjoint_args_driver.c); then the state checks; the solver kind and the pattern of Q are the backend's (dev/adjoint.inc) */
static int adjoint_refuse(const char *msg) {
    char buf[240];
    snprintf(buf, sizeof(buf), "qpdo_amd_adjoint: %s", msg);
    qdev_set_error(buf);
    return -1;
}
int qpdo_amd_adjoint(QPDOWorkspace *work, long nrhs, const double *gx, const double *gy, double *dq, double *dl, double *du, const cholmod_sparse *Q,
                     double *dQx, double *dAx, int *active, long *status, double *res, double tol, long max_sweeps) {
    if (nrhs < 1) return adjoint_refuse("nrhs must be at least 1");
    if (!(tol > 0.0) || !(tol <= 1.7976931348623157e308)) return adjoint_refuse("tol is not a positive finite number");
    if (max_sweeps < 1) return adjoint_refuse("max_sweeps must be at least 1");
    if (!gx) return adjoint_refuse("gx is NULL");
    if (!dq) return adjoint_refuse("dq is NULL");
    if (!dl) return adjoint_refuse("dl is NULL");
    if (!du) return adjoint_refuse("du is NULL");
    if (dQx && !Q) return adjoint_refuse("dQx needs Q (the matrix in the pattern given to qpdo_setup)");
    if (!work || !work->chol || !work->chol->dev || !work->data || !work->info || !work->solution) return adjoint_refuse("NULL workspace");
    struct QPDOBackend *be = work->chol;
    const size_t n = work->data->n;
    if (work->info->status_val != QPDO_SOLVED) return adjoint_refuse("the workspace's status is not QPDO_SOLVED (never solved, infeasible, out of passes or an error): there is no solution to differentiate");
    if (!be->solved_last)
        return adjoint_refuse("the most recent state-changing call was not a solve (qpdo_warm_start, qpdo_update_q, qpdo_update_bounds or qpdo_amd_update_matrices since the last qpdo_solve): call qpdo_solve first");
    if (qdev_adjoint_check_kind(be->dev, "qpdo_amd_adjoint")) return -1;
    QdevCsc qq;
    if (dQx) {
        if (!sparse_ok(Q)) return adjoint_refuse("unsupported sparse storage of Q");
        if (Q->nrow != n || Q->ncol != n) return adjoint_refuse("Q is not n x n");
        if (Q->stype != be->q_stype) return adjoint_refuse("the pattern of Q differs from the one given to qpdo_setup (another stype)");
        if (idx_at(Q->p, Q->itype, (int64_t)n) != be->q_nnz) return adjoint_refuse("the pattern of Q differs from the one given to qpdo_setup (another number of entries)");
        QdevCsc v = {(int32_t)Q->nrow, (int32_t)Q->ncol, be->q_nnz, Q->itype, Q->p, Q->i, (const double *)Q->x, Q->stype};
        qq = v;
    }
    return qdev_adjoint(be->dev, work->solution->x, work->solution->y, nrhs, gx, gy, dq, dl, du, dQx ? &qq : NULL, dQx, dAx, active, status, res, tol, max_sweeps) ? -1 : 0;
}
int qpdo_amd_get_adjoint_stats(const QPDOWorkspace *work, QPDOAmdAdjointStats *out) {
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("qpdo_amd_get_adjoint_stats: NULL workspace"); return -1; }
    if (!out) { qdev_set_error("qpdo_amd_get_adjoint_stats: NULL out"); return -1; }
    QdevAdjointStats st;
    qdev_get_adjoint_stats(work->chol->dev, &st);
    out->calls = (long)st.calls; out->rhs_total = (long)st.rhs_total; out->factorizations = (long)st.factorizations;
    out->sweeps_total = (long)st.sweeps_total; out->scratch_bytes = (long)st.scratch_bytes; out->last_seconds = st.last_seconds;
    return 0;
}
/* ---- qpdo_amd_tangent (include/qpdo_amd_ext.h): the argument checks, in the header's order, before the backend is touched
 * (tests/tangent_args_driver.c); then the adjoint's state checks; the solver kind and the pattern of Q are the backend's (dev/adjoint.inc) */
static int tangent_refuse(const char *msg) {
    char buf[240];
    snprintf(buf, sizeof(buf), "qpdo_amd_tangent: %s", msg);
    qdev_set_error(buf);
    return -1;
}
int qpdo_amd_tangent(QPDOWorkspace *work, long nrhs, const double *tq, const double *tl, const double *tu, const cholmod_sparse *Q, const double *tQx,
                     const double *tAx, double *dx, double *dy, int *active, long *status, double *res, double tol, long max_sweeps) {
    if (nrhs < 1) return tangent_refuse("nrhs must be at least 1");
    if (!(tol > 0.0) || !(tol <= 1.7976931348623157e308)) return tangent_refuse("tol is not a positive finite number");
    if (max_sweeps < 1) return tangent_refuse("max_sweeps must be at least 1");
    if (!dx) return tangent_refuse("dx is NULL");
    if (!dy) return tangent_refuse("dy is NULL");
    if (!tq && !tl && !tu && !tQx && !tAx) return tangent_refuse("no tangent passed (tq, tl, tu, tQx and tAx are all NULL)");
    if (tQx && !Q) return tangent_refuse("tQx needs Q (the matrix in the pattern given to qpdo_setup)");
    if (!work || !work->chol || !work->chol->dev || !work->data || !work->info || !work->solution) return tangent_refuse("NULL workspace");
    struct QPDOBackend *be = work->chol;
    const size_t n = work->data->n;
    if (work->info->status_val != QPDO_SOLVED) return tangent_refuse("the workspace's status is not QPDO_SOLVED (never solved, infeasible, out of passes or an error): there is no solution to differentiate");
    if (!be->solved_last)
        return tangent_refuse("the most recent state-changing call was not a solve (qpdo_warm_start, qpdo_update_q, qpdo_update_bounds or qpdo_amd_update_matrices since the last qpdo_solve): call qpdo_solve first");
    if (qdev_adjoint_check_kind(be->dev, "qpdo_amd_tangent")) return -1;
    QdevCsc qq;
    if (tQx) {
        if (!sparse_ok(Q)) return tangent_refuse("unsupported sparse storage of Q");
        if (Q->nrow != n || Q->ncol != n) return tangent_refuse("Q is not n x n");
        if (Q->stype != be->q_stype) return tangent_refuse("the pattern of Q differs from the one given to qpdo_setup (another stype)");
        if (idx_at(Q->p, Q->itype, (int64_t)n) != be->q_nnz) return tangent_refuse("the pattern of Q differs from the one given to qpdo_setup (another number of entries)");
        QdevCsc v = {(int32_t)Q->nrow, (int32_t)Q->ncol, be->q_nnz, Q->itype, Q->p, Q->i, (const double *)Q->x, Q->stype};
        qq = v;
    }
    return qdev_tangent(be->dev, work->solution->x, work->solution->y, nrhs, tq, tl, tu, tQx ? &qq : NULL, tQx, tAx, dx, dy, active, status, res, tol, max_sweeps) ? -1 : 0;
}
int qpdo_amd_get_tangent_stats(const QPDOWorkspace *work, QPDOAmdTangentStats *out) {
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("qpdo_amd_get_tangent_stats: NULL workspace"); return -1; }
    if (!out) { qdev_set_error("qpdo_amd_get_tangent_stats: NULL out"); return -1; }
    QdevTangentStats st;
    qdev_get_tangent_stats(work->chol->dev, &st);
    out->calls = (long)st.calls; out->rhs_total = (long)st.rhs_total; out->factorizations = (long)st.factorizations;
    out->sweeps_total = (long)st.sweeps_total; out->scratch_bytes = (long)st.scratch_bytes; out->last_seconds = st.last_seconds;
    return 0;
}
/* ---- groups of right-hand sides in the two calls (include/qpdo_amd_ext.h; dev/adjoint.inc adj_sweeps_group) ---- */
int qpdo_amd_rhs_group(const QPDOWorkspace *work) {
    if (!work || !work->chol || !work->chol->dev) return -1;
    return qdev_rhs_group(work->chol->dev);
}
int qpdo_amd_get_group_stats(const QPDOWorkspace *work, QPDOAmdGroupStats *out) {
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("qpdo_amd_get_group_stats: NULL workspace"); return -1; }
    if (!out) { qdev_set_error("qpdo_amd_get_group_stats: NULL out"); return -1; }
    QdevGroupStats st;
    qdev_get_group_stats(work->chol->dev, &st);
    out->group = (long)st.group; out->groups_run = (long)st.groups_run; out->rounds_total = (long)st.rounds_total; out->scratch_bytes = (long)st.scratch_bytes;
    return 0;
}
/* the range and pointer checks are made here, before the backend is touched (tests/group_args_driver.c) */
int qpdo_amd_spmv_group(QPDOWorkspace *work, int which, int nvec, unsigned live_mask, const double *v, double *y) {
    if (nvec < 1 || nvec > 8) { qdev_set_error("qpdo_amd_spmv_group: nvec must be 1 .. 8"); return -1; }
    if (live_mask >> nvec) { qdev_set_error("qpdo_amd_spmv_group: live_mask names a vector >= nvec"); return -1; }
    if (which < 0 || which > 2) { qdev_set_error("qpdo_amd_spmv_group: which is 0 (A), 1 (A') or 2 (Q)"); return -1; }
    if (!v) { qdev_set_error("qpdo_amd_spmv_group: v is NULL"); return -1; }
    if (!y) { qdev_set_error("qpdo_amd_spmv_group: y is NULL"); return -1; }
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("qpdo_amd_spmv_group: NULL workspace"); return -1; }
    return qdev_spmv_group(work->chol->dev, which, nvec, live_mask, v, y) ? -1 : 0;
}
/* the pointer checks of the two PCG test entries are made here, before the backend is touched (tests/pcg_probe_args_driver.c) */
int qpdo_amd_pcg_probe(QPDOWorkspace *work, const double *dw, double sigma, const double *v, double *out, int mode, double *info) {
    if (mode != 0 && mode != 1 && (mode < 32 || mode > 37)) { qdev_set_error("pcg probe: mode is 0 (one K product), 1 (one solve), 32 or 33 (one fp32-stream product), 34 or 35 (one pair-wide fp32 product), 36 or 37 (one pair-wide half-precision product)"); return -1; }
    if (!dw || !v || !out || !info) { qdev_set_error("pcg probe: NULL vector (dw, v, out and info are required, also at m = 0)"); return -1; }
    if (!(sigma == sigma)) { qdev_set_error("pcg probe: sigma is NaN"); return -1; }
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("pcg probe: NULL workspace"); return -1; }
    const int rc = qdev_pcg_probe(work->chol->dev, dw, sigma, v, out, mode, info);
    return rc == QDEV_PCG_NOT_CONVERGED ? QPDO_AMD_PCG_NOT_CONVERGED : rc == QDEV_PCG_NAN ? QPDO_AMD_PCG_NAN : rc ? -1 : 0;
}
int qpdo_amd_download_compact(QPDOWorkspace *work, int which, void *dst, long count) {
    if (which < 0 || which > 96 || (which > 57 && which < 64 && which != 59 && which != 60) || (which < 48 && which % 16 > 5) || (which >= 64 && which < 96 && which % 16 > 4)) {
        qdev_set_error("download compact: unknown array"); return -1;
    }
    if (count < 0) { qdev_set_error("download compact: negative count"); return -1; }
    if (count > 0 && !dst) { qdev_set_error("download compact: NULL destination"); return -1; }
    if (!work || !work->chol || !work->chol->dev) { qdev_set_error("download compact: NULL workspace"); return -1; }
    return qdev_download_compact(work->chol->dev, which, dst, count) ? -1 : 0;
}
int qpdo_amd_slab_trip_shape(int value_bytes, int operand_bytes, int *shape) {
    if (!shape) { qdev_set_error("slab trip shape: NULL shape"); return -1; }
    if (qdev_slab_trip_shape(value_bytes, operand_bytes, shape)) { qdev_set_error("slab trip shape: no instance streams that value and operand width (bytes: 8/8, 4/8, 4/4, 2/4)"); return -1; }
    return 0;
}
int qpdo_amd_download(QPDOWorkspace *work, int which, double *dst) { return qdev_download_vec(work->chol->dev, which, dst); }
int qpdo_amd_get_stats(const QPDOWorkspace *work, QPDOAmdStats *out) {
    QdevStats st;
    double avg = 0.0; long ns = 0;
    qdev_get_stats(work->chol->dev, &st);
    qdev_get_spmv_sample(work->chol->dev, &avg, &ns);
    out->newton_passes = work->chol->newton_passes;
    out->lin_iters = (long)st.lin_iters;
    out->spmv_calls = (long)st.spmv_calls;
    out->spmv_alg_bytes = (double)st.spmv_bytes;
    out->factor_count = (long)st.factor_count;
    out->linsolve = st.linsolve;
    out->spmv_Q_avg_s = avg;
    out->spmv_Q_samples = ns;
    { double ts = 0, bs = 0; long n2 = 0, sp = 0; qdev_get_ac_sample(work->chol->dev, &ts, &bs, &n2, &sp);
      out->spmv_Ac_time_s = ts; out->spmv_Ac_bytes = bs; out->spmv_Ac_samples = n2; out->schur_passes = sp; }
    out->lowrank_solves = (long)st.lowrank_solves;
    out->lowrank_cols = (long)st.lowrank_cols;
    out->lowrank_sweeps = (long)st.lowrank_sweeps;
    out->lowrank_rejects = (long)st.lowrank_rejects;
    out->pcg_soft_accepts = (long)st.pcg_soft_accepts;
    out->chain_fallbacks = (long)st.chain_fallbacks;
    out->collectives = (long)st.collectives; out->inner_solves = (long)st.inner_solves;
    out->inner_steps = (long)st.inner_steps; out->inner_collectives = (long)st.inner_collectives;
    out->pcg_max_relres = st.pcg_max_relres;
    out->pcg_dense_fallbacks = (long)st.pcg_dense_fallbacks;
    out->pcg_rescues = (long)st.pcg_rescues; out->pcg_rescue_kinds = (long)st.pcg_rescue_kinds;
    out->hybrid_pcg_passes = (long)st.hybrid_pcg_passes; out->band_fallbacks = (long)st.band_fallbacks;
    out->onelaunch_factors = (long)st.onelaunch_factors;
    out->ahead_steps = (long)st.ahead_steps; out->ahead_skips = (long)st.ahead_skips;
    out->updown_solves = (long)st.updown_solves; out->updown_rows = (long)st.updown_rows; out->updown_rejects = (long)st.updown_rejects;
    out->coupled_rows = (long)st.coupled_rows; out->coupled_solves = (long)st.coupled_solves; out->coupled_sweeps = (long)st.coupled_sweeps;
    out->coupled_rejects = (long)st.coupled_rejects;
    out->inner_refine_sweeps = (long)st.inner_refine_sweeps; out->inner_refine_fp64_applies = (long)st.inner_refine_fp64_applies;
    out->inner_refine_fallbacks = (long)st.inner_refine_fallbacks; out->inner_refine_max_res_over_tol = st.inner_refine_max_res_over_tol;
    out->inner_x32_steps = (long)st.inner_x32_steps;
    out->inner_h16_steps = (long)st.inner_h16_steps; out->inner_h16_sweeps = (long)st.inner_h16_sweeps;
    out->fused_solves = work->chol->fused_solves;
    out->fused_kernel_s = work->chol->last_fused ? work->chol->fused_kernel_s : 0.0;
    if (work->chol->last_fused) { out->factor_count = work->chol->fused_factor_count; out->linsolve = 2; }
    return 0;
}

/* ---- batch of independent QPs ------------------------------------------------------------------------------ */
typedef struct { long count; QPDOAmdBatchItem *items; const QPDOSettings *settings; long next; long failed; pthread_mutex_t mu; } BatchCtx;
static void *batch_worker(void *arg) {
    BatchCtx *b = (BatchCtx *)arg;
    for (;;) {
        pthread_mutex_lock(&b->mu);
        long i = b->next++;
        pthread_mutex_unlock(&b->mu);
        if (i >= b->count) break;
        QPDOAmdBatchItem *it = &b->items[i];
        const size_t n = it->data->n, m = it->data->m;
        QPDOWorkspace *w = qpdo_setup(it->data, b->settings);
        if (!w) {
            memset(&it->info, 0, sizeof(it->info));
            update_status(&it->info, QPDO_ERROR);
            pthread_mutex_lock(&b->mu); b->failed++; pthread_mutex_unlock(&b->mu);
            continue;
        }
        if (it->x0 || it->y0) qpdo_warm_start(w, (c_float *)it->x0, (c_float *)it->y0);
        qpdo_solve(w);
        it->info = *w->info;
        const int infeasible = (w->info->status_val == QPDO_PRIMAL_INFEASIBLE) || (w->info->status_val == QPDO_DUAL_INFEASIBLE);
        if (it->x) for (size_t k = 0; k < n; k++) it->x[k] = infeasible ? NAN : w->solution->x[k];
        if (it->y) for (size_t k = 0; k < m; k++) it->y[k] = infeasible ? NAN : w->solution->y[k];
        qpdo_cleanup(w);
    }
    return NULL;
}
double qpdo_amd_batch_kernel_seconds(void) { return qdev_small_last_kernel_seconds(); }
/* where the fused kernel keeps the Newton matrix: see include/qpdo_amd_ext.h.  The query and the launches share one rule (small_plan, qpdo_small.hip) */
int qpdo_amd_batch_factor_layout(void) { return qdev_small_last_batch_layout(); }
int qpdo_amd_small_factor_layout(long count, const QPDOData *const *data, const QPDOSettings *settings, int kind, long *half_bandwidth) {
    (void)settings;                                  /* (no setting enters the rule) */
    const int lay = qdev_small_factor_layout(count, (const void *const *)data, kind, half_bandwidth);
    if (lay < 0) qdev_set_error(qdev_small_last_error());
    return lay;
}
int qpdo_amd_fleet_factor_layout(const QPDOAmdFleet *f) {
    if (!f) { qdev_set_error("qpdo_amd_fleet_factor_layout: NULL fleet"); return -1; }
    return qdev_small_fleet_layout(f);
}
long qpdo_amd_solve_batch(long count, QPDOAmdBatchItem *items, const QPDOSettings *settings, int nthreads) {
    if (count <= 0) return 0;
    /* small problems: the fused one-workgroup-per-QP kernel solves the whole batch in one launch
     * (QPDO_BATCH=threads forces the generic multi-kernel path on a host thread pool) */
    const char *mode = getenv("QPDO_BATCH");
    if (!(mode && !strcmp(mode, "threads")) && validate_settings(settings) && qdev_small_eligible(count, items)) {
        long bad = 0;
        for (long i = 0; i < count; i++) if (!validate_data(items[i].data)) bad++;
        if (!bad) {
            int device;
            if (pick_device(&device)) {
                const double tb0 = wall_now();
                const int rcb = qdev_small_batch(device, count, items, settings);
                if (env_int("QPDO_SMALL_PROF", 0) == 2) fprintf(stderr, "[qpdo_small host] qdev_small_batch total   %.3f s\n", wall_now() - tb0);
                if (rcb == 0) return 0;
                QPDO_EPRINT("fused batch kernel failed (%s); using the generic path", qdev_small_last_error());
            }
        }
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if (nthreads > count) nthreads = (int)count;
    BatchCtx b = {count, items, settings, 0, 0, PTHREAD_MUTEX_INITIALIZER};
    pthread_t th[64];
    int started = 0;
    for (int t = 0; t < nthreads; t++) if (pthread_create(&th[started], NULL, batch_worker, &b) == 0) started++;
    if (started == 0) batch_worker(&b);
    for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    return b.failed;
}

/* streamed batches: see include/qpdo_amd_ext.h */
QPDOAmdBatchStream *qpdo_amd_batch_stream_create(int depth) {
    int device;
    if (!pick_device(&device)) { QPDO_EPRINT(NO_DEVICE_MSG); return NULL; }
    warn_hw_queues_once(depth);
    return (QPDOAmdBatchStream *)qdev_small_stream_create(device, depth);
}
long qpdo_amd_batch_stream_submit(QPDOAmdBatchStream *stream, long count, QPDOAmdBatchItem *items, const QPDOSettings *settings) {
    if (!stream || count <= 0 || !items || !settings) return -1;
    if (!validate_settings(settings)) return -1;
    if (!qdev_small_eligible(count, items)) { QPDO_EPRINT("batch stream: an item does not fit the fused kernel (n, m <= 1024); use qpdo_amd_solve_batch"); return -1; }
    for (long i = 0; i < count; i++) if (!validate_data(items[i].data)) return -1;
    const long t = qdev_small_stream_submit(stream, count, items, settings);
    if (t < 0) QPDO_EPRINT("batch stream: %s", qdev_small_last_error());
    return t;
}
int qpdo_amd_batch_stream_wait(QPDOAmdBatchStream *stream, long ticket, double *kernel_seconds) {
    if (!stream) return -1;
    const int rc = qdev_small_stream_wait(stream, ticket, kernel_seconds);
    if (rc) QPDO_EPRINT("batch stream: %s", qdev_small_last_error());
    return rc;
}
void qpdo_amd_batch_stream_destroy(QPDOAmdBatchStream *stream) { qdev_small_stream_destroy(stream); }

/* ---- a resident fleet of small QPs: see include/qpdo_amd_ext.h.  Argument checks here (they precede every write and need no device),
 * the work in qdev_small_fleet_* (qpdo_small.hip) ------------------------------------------------------------------------------- */
static int fleet_refuse(const char *msg) { qdev_set_error(msg); return -1; }
QPDOAmdFleet *qpdo_amd_fleet_create(long count, const QPDOData *const *data, const QPDOSettings *settings) {
    return qpdo_amd_fleet_create_ex(count, data, settings, 0L);
}
QPDOAmdFleet *qpdo_amd_fleet_create_ex(long count, const QPDOData *const *data, const QPDOSettings *settings, long flags) {
    if (flags & ~(QPDO_AMD_FLEET_MATRIX_UPDATES | QPDO_AMD_FLEET_ADJOINT)) {
        fleet_refuse("qpdo_amd_fleet_create_ex: unknown flag bits (known: QPDO_AMD_FLEET_MATRIX_UPDATES, QPDO_AMD_FLEET_ADJOINT)"); return NULL;
    }
    if (count <= 0) { fleet_refuse("qpdo_amd_fleet_create: count must be positive"); return NULL; }
    if (!data) { fleet_refuse("qpdo_amd_fleet_create: NULL data array"); return NULL; }
    if (!settings) { fleet_refuse("qpdo_amd_fleet_create: NULL settings"); return NULL; }
    if (!validate_settings(settings)) { fleet_refuse("qpdo_amd_fleet_create: invalid settings"); return NULL; }
    for (long i = 0; i < count; i++) {
        char msg[160];
        QPDOAmdBatchItem it;
        memset(&it, 0, sizeof(it));
        it.data = data[i];
        if (!data[i] || !qdev_small_eligible(1, &it)) {
            snprintf(msg, sizeof(msg), "qpdo_amd_fleet_create: item %ld does not fit the fused kernel (n, m <= 1024, the matrix checks of qpdo_setup)", i);
            fleet_refuse(msg); return NULL;
        }
        for (size_t j = 0; j < data[i]->m; j++)          /* (validate.c:20-28; the pointers were checked by qdev_small_eligible) */
            if (data[i]->l[j] > data[i]->u[j]) {
                snprintf(msg, sizeof(msg), "qpdo_amd_fleet_create: item %ld has a lower bound above its upper bound (index %ld)", i, (long)j);
                fleet_refuse(msg); return NULL;
            }
    }
    int device;
    if (!pick_device(&device)) { fleet_refuse("qpdo_amd_fleet_create: " NO_DEVICE_MSG); return NULL; }
    void *f = qdev_small_fleet_create(device, count, (const void *const *)data, settings, flags);
    if (!f) { char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_create: %s", qdev_small_last_error()); fleet_refuse(msg); }
    return (QPDOAmdFleet *)f;
}
int qpdo_amd_fleet_update(QPDOAmdFleet *f, const c_float *const *q, const c_float *const *l, const c_float *const *u) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_update: NULL fleet");
    long st[5]; double ks;
    qdev_small_fleet_stats(f, st, &ks);
    if (l && u)
        for (long i = 0; i < st[0]; i++) {
            if (!l[i] || !u[i]) continue;
            int n, m;
            qdev_small_fleet_dims(f, i, &n, &m);
            for (int j = 0; j < m; j++)
                if (l[i][j] > u[i][j]) {
                    char msg[160];
                    snprintf(msg, sizeof(msg), "qpdo_amd_fleet_update: item %ld: lower bound at index %d is greater than upper bound", i, j);
                    return fleet_refuse(msg);
                }
        }
    if (qdev_small_fleet_update(f, q, l, u)) { char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_update: %s", qdev_small_last_error()); return fleet_refuse(msg); }
    return 0;
}
int qpdo_amd_fleet_warm_start(QPDOAmdFleet *f, const c_float *const *x0, const c_float *const *y0) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_warm_start: NULL fleet");
    if (qdev_small_fleet_warm_start(f, x0, y0, 0)) { char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_warm_start: %s", qdev_small_last_error()); return fleet_refuse(msg); }
    return 0;
}
int qpdo_amd_fleet_warm_start_last(QPDOAmdFleet *f) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_warm_start_last: NULL fleet");
    if (qdev_small_fleet_warm_start(f, NULL, NULL, 1)) { char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_warm_start_last: %s", qdev_small_last_error()); return fleet_refuse(msg); }
    return 0;
}
int qpdo_amd_fleet_solve(QPDOAmdFleet *f, c_float *const *x, c_float *const *y, QPDOInfo *info) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_solve: NULL fleet");
    if (!info) return fleet_refuse("qpdo_amd_fleet_solve: NULL info array");
    if (qdev_small_fleet_solve(f, x, y, info)) { char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_solve: %s", qdev_small_last_error()); return fleet_refuse(msg); }
    return 0;
}
int qpdo_amd_fleet_get_stats(const QPDOAmdFleet *f, QPDOAmdFleetStats *out) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_stats: NULL fleet");
    if (!out) return fleet_refuse("qpdo_amd_fleet_get_stats: NULL output");
    long st[5]; double ks;
    qdev_small_fleet_stats(f, st, &ks);
    out->count = st[0]; out->matrix_bytes_uploaded = st[1]; out->vector_bytes_uploaded_last_call = st[2];
    out->solve_launches = st[3]; out->solves = st[4]; out->last_kernel_seconds = ks;
    return 0;
}
int qpdo_amd_fleet_update_matrices(QPDOAmdFleet *f, const cholmod_sparse *const *Q, const cholmod_sparse *const *A) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_update_matrices: NULL fleet");
    if (qdev_small_fleet_update_matrices(f, (const void *const *)Q, (const void *const *)A)) {
        char msg[320]; snprintf(msg, sizeof(msg), "qpdo_amd_fleet_update_matrices: %s", qdev_small_last_error()); return fleet_refuse(msg);
    }
    return 0;
}
int qpdo_amd_fleet_get_matrix_stats(const QPDOAmdFleet *f, QPDOAmdFleetMatrixStats *out) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_matrix_stats: NULL fleet");
    if (!out) return fleet_refuse("qpdo_amd_fleet_get_matrix_stats: NULL output");
    long st[4]; double ks;
    qdev_small_fleet_matrix_stats(f, st, &ks);
    out->calls = st[0]; out->items_last_call = st[1]; out->value_bytes_uploaded_last_call = st[2]; out->resident_extra_bytes = st[3];
    out->last_kernel_seconds = ks;
    return 0;
}
int qpdo_amd_fleet_get_certificates(const QPDOAmdFleet *f, long item, c_float *prim_inf_cert, c_float *dual_inf_cert) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_certificates: NULL fleet");
    long st[5]; double ks;
    qdev_small_fleet_stats(f, st, &ks);
    if (item < 0 || item >= st[0]) return fleet_refuse("qpdo_amd_fleet_get_certificates: item out of range");
    if (qdev_small_fleet_certificates(f, item, prim_inf_cert, dual_inf_cert)) return fleet_refuse("qpdo_amd_fleet_get_certificates: no solve yet");
    return 0;
}
int qpdo_amd_fleet_device(const QPDOAmdFleet *f) {
    if (!f) { fleet_refuse("qpdo_amd_fleet_device: NULL fleet"); return -1; }
    return qdev_small_fleet_device(f);
}
/* the packed layout of the device calls: pure host arithmetic, no device needed */
int qpdo_amd_fleet_packed_layout(long count, const QPDOData *const *data, long *noff, long *moff) {
    if (count <= 0) return fleet_refuse("qpdo_amd_fleet_packed_layout: count must be positive");
    if (!data) return fleet_refuse("qpdo_amd_fleet_packed_layout: NULL data array");
    if (!noff || !moff) return fleet_refuse("qpdo_amd_fleet_packed_layout: NULL output");
    for (long i = 0; i < count; i++) if (!data[i]) return fleet_refuse("qpdo_amd_fleet_packed_layout: NULL item");
    noff[0] = moff[0] = 0;
    for (long i = 0; i < count; i++) { noff[i + 1] = noff[i] + (long)data[i]->n; moff[i + 1] = moff[i] + (long)data[i]->m; }
    return 0;
}
int qpdo_amd_fleet_get_packed_layout(const QPDOAmdFleet *f, long *noff, long *moff) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_packed_layout: NULL fleet");
    if (!noff || !moff) return fleet_refuse("qpdo_amd_fleet_get_packed_layout: NULL output");
    qdev_small_fleet_packed_layout(f, noff, moff);
    return 0;
}
/* device arrays on the caller's stream: the checks that need the runtime (is this pointer device memory?) are in qdev_small_fleet_*_dev */
static int fleet_dev_failed(const char *name) { char msg[320]; snprintf(msg, sizeof(msg), "%s: %s", name, qdev_small_last_error()); return fleet_refuse(msg); }
int qpdo_amd_fleet_update_dev(QPDOAmdFleet *f, const double *q, const double *l, const double *u, const int *item_mask, long n_len, long m_len, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_update_dev: NULL fleet");
    if (qdev_small_fleet_update_dev(f, q, l, u, item_mask, n_len, m_len, stream)) return fleet_dev_failed("qpdo_amd_fleet_update_dev");
    return 0;
}
int qpdo_amd_fleet_warm_start_dev(QPDOAmdFleet *f, const double *x0, const double *y0, const int *item_mask, long n_len, long m_len, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_warm_start_dev: NULL fleet");
    if (qdev_small_fleet_warm_start_dev(f, x0, y0, item_mask, n_len, m_len, 0, stream)) return fleet_dev_failed("qpdo_amd_fleet_warm_start_dev");
    return 0;
}
int qpdo_amd_fleet_warm_start_last_dev(QPDOAmdFleet *f, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_warm_start_last_dev: NULL fleet");
    if (qdev_small_fleet_warm_start_dev(f, NULL, NULL, NULL, 0, 0, 1, stream)) return fleet_dev_failed("qpdo_amd_fleet_warm_start_last_dev");
    return 0;
}
int qpdo_amd_fleet_solve_dev(QPDOAmdFleet *f, double *x, double *y, long *status, double *norms, double *prim_inf_cert, double *dual_inf_cert, long n_len, long m_len,
                             void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_solve_dev: NULL fleet");
    if (qdev_small_fleet_solve_dev(f, x, y, status, norms, prim_inf_cert, dual_inf_cert, n_len, m_len, stream)) return fleet_dev_failed("qpdo_amd_fleet_solve_dev");
    return 0;
}
/* the packed VALUE layout of update_matrices_dev: the stored entries of every Q and of every A, pure host arithmetic (either itype) */
static long fleet_stored_entries(const cholmod_sparse *M) { return (M && M->p) ? (long)idx_at(M->p, M->itype, (int64_t)M->ncol) : 0L; }
int qpdo_amd_fleet_packed_matrix_layout(long count, const QPDOData *const *data, long *qoff, long *aoff) {
    if (count <= 0) return fleet_refuse("qpdo_amd_fleet_packed_matrix_layout: count must be positive");
    if (!data) return fleet_refuse("qpdo_amd_fleet_packed_matrix_layout: NULL data array");
    if (!qoff || !aoff) return fleet_refuse("qpdo_amd_fleet_packed_matrix_layout: NULL output");
    for (long i = 0; i < count; i++) if (!data[i]) return fleet_refuse("qpdo_amd_fleet_packed_matrix_layout: NULL item");
    qoff[0] = aoff[0] = 0;
    for (long i = 0; i < count; i++) { qoff[i + 1] = qoff[i] + fleet_stored_entries(data[i]->Q); aoff[i + 1] = aoff[i] + fleet_stored_entries(data[i]->A); }
    return 0;
}
int qpdo_amd_fleet_get_packed_matrix_layout(const QPDOAmdFleet *f, long *qoff, long *aoff) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_packed_matrix_layout: NULL fleet");
    if (!qoff || !aoff) return fleet_refuse("qpdo_amd_fleet_get_packed_matrix_layout: NULL output");
    if (qdev_small_fleet_packed_matrix_layout(f, qoff, aoff)) return fleet_dev_failed("qpdo_amd_fleet_get_packed_matrix_layout");
    return 0;
}
int qpdo_amd_fleet_update_matrices_dev(QPDOAmdFleet *f, const double *Qx, const double *Ax, const int *item_mask, long q_len, long a_len, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_update_matrices_dev: NULL fleet");
    if (qdev_small_fleet_update_matrices_dev(f, Qx, Ax, item_mask, q_len, a_len, stream)) return fleet_dev_failed("qpdo_amd_fleet_update_matrices_dev");
    return 0;
}
int qpdo_amd_fleet_fetch_last(QPDOAmdFleet *f, c_float *const *x, c_float *const *y, QPDOInfo *info) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_fetch_last: NULL fleet");
    if (!info) return fleet_refuse("qpdo_amd_fleet_fetch_last: NULL info array");
    if (qdev_small_fleet_fetch_last(f, x, y, info)) return fleet_dev_failed("qpdo_amd_fleet_fetch_last");
    return 0;
}
int qpdo_amd_fleet_sync(QPDOAmdFleet *f, QPDOAmdFleetDevStats *out) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_sync: NULL fleet");
    long st[5] = {0, 0, 0, 0, -1};
    if (qdev_small_fleet_sync(f, st)) return fleet_dev_failed("qpdo_amd_fleet_sync");
    if (out) { out->update_calls = st[0]; out->warm_start_calls = st[1]; out->solve_calls = st[2]; out->refused_items = st[3]; out->first_refused_item = st[4]; }
    return 0;
}
int qpdo_amd_fleet_adjoint_dev(QPDOAmdFleet *f, const double *gx, const double *gy, double *dq, double *dl, double *du, double *dQx, double *dAx, int *active,
                               long *adj_status, double *adj_res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_adjoint_dev: NULL fleet");
    if (qdev_small_fleet_adjoint_dev(f, gx, gy, dq, dl, du, dQx, dAx, active, adj_status, adj_res, tol, max_sweeps, n_len, m_len, q_len, a_len, stream))
        return fleet_dev_failed("qpdo_amd_fleet_adjoint_dev");
    return 0;
}
int qpdo_amd_fleet_get_adjoint_stats(const QPDOAmdFleet *f, QPDOAmdFleetAdjointStats *out) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_adjoint_stats: NULL fleet");
    if (!out) return fleet_refuse("qpdo_amd_fleet_get_adjoint_stats: NULL output");
    out->adjoint_calls = qdev_small_fleet_adjoint_calls(f); out->resident_extra_bytes = 0;
    return 0;
}
int qpdo_amd_fleet_adjoint_multi_dev(QPDOAmdFleet *f, long nrhs, const double *gx, const double *gy, double *dq, double *dl, double *du, double *dQx, double *dAx,
                                     int *active, long *status, double *res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len, void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_adjoint_multi_dev: NULL fleet");
    if (qdev_small_fleet_adjoint_multi_dev(f, nrhs, gx, gy, dq, dl, du, dQx, dAx, active, status, res, tol, max_sweeps, n_len, m_len, q_len, a_len, stream))
        return fleet_dev_failed("qpdo_amd_fleet_adjoint_multi_dev");
    return 0;
}
int qpdo_amd_fleet_tangent_dev(QPDOAmdFleet *f, long nrhs, const double *tq, const double *tl, const double *tu, const double *tQx, const double *tAx, double *dx,
                               double *dy, int *active, long *status, double *res, double tol, long max_sweeps, long n_len, long m_len, long q_len, long a_len,
                               void *stream) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_tangent_dev: NULL fleet");
    if (qdev_small_fleet_tangent_dev(f, nrhs, tq, tl, tu, tQx, tAx, dx, dy, active, status, res, tol, max_sweeps, n_len, m_len, q_len, a_len, stream))
        return fleet_dev_failed("qpdo_amd_fleet_tangent_dev");
    return 0;
}
int qpdo_amd_fleet_rhs_group(const QPDOAmdFleet *f) { return f ? qdev_small_fleet_rhs_group(f) : -1; }
int qpdo_amd_fleet_get_sensitivity_stats(const QPDOAmdFleet *f, QPDOAmdFleetSensitivityStats *out) {
    if (!f) return fleet_refuse("qpdo_amd_fleet_get_sensitivity_stats: NULL fleet");
    if (!out) return fleet_refuse("qpdo_amd_fleet_get_sensitivity_stats: NULL output");
    long s[3] = {0, 0, 0};
    qdev_small_fleet_sens_stats(f, s);
    out->calls = s[0]; out->rhs_total = s[1]; out->scratch_bytes = s[2];
    return 0;
}
void qpdo_amd_fleet_destroy(QPDOAmdFleet *f) { if (f) qdev_small_fleet_destroy(f); }
