/*
 * qpdo_amd_ext.h -- extensions of libqpdo_amd.so beyond the reference API.
 *
 * Nothing here is needed to use the library as a drop-in for the reference;
 * these entry points exist for measurement (bench.py), for the parity tests of
 * single kernels, and for device selection.  All are plain C-ABI.
 *
 * Environment variables read once per qpdo_setup:
 *   QPDO_DEVICE      HIP device ordinal (default: LOCAL_RANK if set, else 0)
 *   QPDO_LINSOLVE    "pcg" | "dense" | "band" | "auto" (default auto: the BAND direct solver when the Newton matrix is banded -- half-bandwidth
 *                    of Q + A'A <= 127, chain-structured QPs -- and n >= 2048; otherwise dense LDL' for n <= QPDO_DENSE_MAX_N = 12288, PCG
 *                    above; "band" takes the band solver for every half-bandwidth <= 1023 with n >= 4 (b + 1) -- 128 .. 1023 through the
 *                    tiled fp64-MFMA factorization of dev/band_wide.inc, which is never chosen automatically (its crossover against
 *                    dense and PCG is not measured yet) except as the rescue of a PCG solve that cannot converge above n = 40000 --
 *                    and on a matrix that is not banded (half-bandwidth > 1023 or order too small) makes qpdo_setup fail with a
 *                    message; the dense solver accepts
 *                    n <= 40000 -- its assembly tiles the LDS accumulator, QPDO_DENSE_ASM_TILE rows at a time -- and is also the rescue of
 *                    a PCG solve that cannot converge up to that order)
 *   QPDO_BAND_COUPLING  unset or "0": off (default).  "<R>", 1 <= R <= 64: a COUPLING ROW is a row of A whose column span (last - first column)
 *                    exceeds 127 -- a budget over the whole horizon, a terminal average, a conservation equality on a chain-structured QP.
 *                    With 1 .. R of them, Q's bandwidth <= 127 and the other rows' spans <= 127, the band solver's half-bandwidth is that of
 *                    the rest (b_core, at least 3) and the selection rule above runs on it (automatic from n = 2048, on request from n =
 *                    4 (b_core + 1)); the Newton matrix is then solved as band plus low rank, K = B + U W U': the band LDL' of B = Q + sigma I
 *                    + the other rows' term, one multi-right-hand-side band solve for Z = B^-1 U (a column per coupling row with a nonzero
 *                    weight), the k x k system S = W^-1 + U'Z factored in LDS, and every solve checked against the true K (three SpMV;
 *                    refinement sweeps and acceptance rule of the dense low-rank path).  While the other rows' weights and sigma stay, B's
 *                    factor and Z are kept and only S is rebuilt (factor_count does not move).  A solve that misses the check, or a pivot
 *                    of B or S that is not a positive finite number, hands the pass to the dense solver / PCG (band_fallbacks;
 *                    QPDOAmdStats.coupled_*).  No such row: the plain band solver, bit for bit.  More than R: the matrix counts as not
 *                    banded ("band" makes qpdo_setup fail with a message that names both numbers).  Q or the other rows wider than 127:
 *                    the half-bandwidth over all rows, as without the variable.  Read at qpdo_setup; one GPU
 *   QPDO_BAND_BORDER unset or "0": off (default).  "<C>", 1 <= C <= 64: BORDER VARIABLES are a few variables that appear everywhere on a
 *                    chain-structured QP -- a global slack, a free final time, a shared parameter, the first stage of a multi-scenario
 *                    problem -- and give K a dense row and column each.  They MUST BE NUMBERED LAST (problems.permute_variables, or the
 *                    caller's own numbering).  qpdo_setup runs qpdo_amd_band_border (below) on the pattern: K = [B C; C' D] with B the
 *                    n_core x n_core core of half-bandwidth b_core <= 127 and c = n - n_core trailing border variables.  With 1 <= c <= C
 *                    and a core that the selection rule above takes on (n_core, b_core) -- automatic for n_core >= 2048, on request from
 *                    n_core = 4 (b_core + 1) -- the band solver runs by block elimination: the band LDL' of B (the bits of the plain band
 *                    workspace on the problem without the border columns), the c columns of [C; D], one multi-right-hand-side band solve
 *                    for Z = B^-1 C, S = D - C'Z factored in LDS; a solve is z0 = B^-1 rhs_1, t = S^-1 (rhs_2 - C'z0), x = [z0 - Z t; t]:
 *                    three launches, an exact LDL' of K in that order, no refinement.  A pivot of B or S that is not a positive finite
 *                    number hands the pass to the dense solver / PCG (band_fallbacks).  c = 0: the plain band workspace, bit for bit.
 *                    c > C, or a core the rule does not take: as if the variable were unset (QPDOAmdBandBorderInfo keeps c in `over`;
 *                    for c > C "band" makes qpdo_setup fail with a message that names both numbers).  IGNORED, with the reason recorded:
 *                    row-partitioned workspaces, the fused small-problem route, QPDO_LINSOLVE = dense or pcg, QPDO_BAND_COUPLING > 0
 *                    (the coupling-row mode keeps precedence).  A configured band order is ignored on a workspace that adopts a border
 *                    (reason 6 of qpdo_amd_get_band_order).  qpdo_amd_adjoint / _tangent take such a workspace with the right-hand
 *                    sides one after the other (qpdo_amd_rhs_group = 1).  Read at qpdo_setup; one GPU
 *   QPDO_BAND_ORDER  unset, "" or "0": the band solver works in the caller's variable order (default).  "rcm": qpdo_setup computes a reverse
 *                    Cuthill-McKee order of the pattern of Q + A'A on the host and, where that narrows the half-bandwidth, the band
 *                    detection, the selection rule above and the band solver run on the reordered matrix (qpdo_amd_band_order_config
 *                    below, which overrides the variable, has the contract and the kinds of workspace that ignore it).  Any other value
 *                    makes qpdo_setup fail with a message
 *   QPDO_HYBRID      where the dense solver is selected automatically and n >= 8192, every solve starts with PCG and switches to the dense
 *                    factor at the first Newton pass that needs more than 450 PCG iterations (default since round 4; same per-pass integers;
 *                    QPDOAmdStats.hybrid_pcg_passes counts the PCG passes; every numerical PCG failure hands the pass to the dense factor).  "0": off; "1": on from n = 4096; "<budget>" > 1: on from n = 4096 with that budget
 *   QPDO_DENSE_MID   "0": the dense factorization as the multi-launch blocked pipeline of rounds 1-4 instead of ONE launch of tile-owning
 *                    workgroups (k_mid_factor, the default at every order since round 5: n = 1e4 8.4 ms against 13.3 ms).  The
 *                    look-ahead below acts on the multi-launch path only
 *   QPDO_CTRL_PUBLISH "0": the per-pass read-back of the control block as hipMemcpyAsync + hipStreamSynchronize instead of a kernel that
 *                    writes the block and a sequence word into coherent pinned memory while the host spins (bounded; default since round 5:
 *                    15.7 -> 9.9 us per read-back).  Only the transport differs: the same bits
 *   QPDO_FUSE_RESID  "0": the deferred Newton step's five axpys and the read-back's publication as launches of their own instead of
 *                    inside the residual launch (dense / band routes; the same bits)
 *   QPDO_LS_SMALL    "0": the linesearch through the radix-sort kernels (28 launches) at every size instead of ONE launch for 2m <= 8192
 *                    (read at qpdo_setup; the same tau bits: tests/test_gpu_parity.py)
 *   QPDO_FUSE_OUTER  "0": the outer-update sequences (infeasibility tests, mu update, shifting the estimates) as their separate kernels and
 *                    device copies (27 launches) instead of 10 (the same bits); also: Q dx and A dx of a Newton step as two launches
 *   QPDO_LAUNCH_AHEAD "0": the Newton step of a pass is launched after the host has read the pass's norms and decided, instead of behind
 *                    the residual launch with the decision formed on the device (mid-size dense route, n < 9000, 2m <= 8192; DESIGN.md
 *                    section 5; read at qpdo_setup; QPDOAmdStats.ahead_steps / ahead_skips).  The same kernels in the same order: the same bits,
 *                    except on a pass whose factor the host-first path would keep (it is refactored: the same matrix)
 *   QPDO_DENSE_LOWRANK  "0": refactor on every weight change, "1": low-rank update of the kept dense factor (default: from n = 9000 up)
 *   QPDO_DENSE_UPDOWN   unset or "0": off (default).  "1" or "<k>" (k > 1): a Newton pass that keeps sigma and changes the weight of at most k rows of
 *                    A (k = 1 for "1"; at most 64) changes the kept dense factor IN PLACE, one row at a time (K' = K + delta a a': a chained
 *                    forward solve, a prefix scan for D' and the multipliers, one streaming pass over the tiles of L that also rewrites the
 *                    transposed copies and the diagonal blocks' inverses) instead of factoring again; more rows take the
 *                    path they took without it (QPDO_DENSE_LOWRANK if on, else a factorization).  While the factor carries such a change every
 *                    solve is checked against the true K (three SpMV; refinement sweeps as on the low-rank path) and a failed check, or a
 *                    downdate whose scan meets a non-positive pivot, refactors (QPDOAmdStats.updown_*).  Dense solver with the chained
 *                    solves on one GPU only; switches the launch-ahead route off (it refactors every pass by construction).  Read at qpdo_setup
 *   QPDO_DENSE_LOOKAHEAD "0": factor on one stream, "1": overlap the next panel with the trailing update (default: from n = 7000 up;
 *                    read at qpdo_setup)
 *   QPDO_DENSE_SOLVE "steps": per-block-step triangular solve kernels instead of the one-launch chained solves
 *   QPDO_AMD_RHS_GROUP  "1".."8": the right-hand sides qpdo_amd_adjoint / qpdo_amd_tangent carry through every launch of their sweep loop at
 *                    once (default 8 where the workspace qualifies: "GROUPS of right-hand sides" below; "1": one after the other).  A
 *                    measuring switch; the same bits at every value.  Read at qpdo_setup
 *   QPDO_SETUP_THREADS  host threads of the CSC -> CSR conversions in qpdo_setup (default min(16, cores)); QPDO_SETUP_PROF=1 prints phase times
 *   QPDO_SPMV        "slab" | "plain" (default: LDS-staged slab kernel for matrices >= 192 MB)
 *   QPDO_DEFLATE     "0" disables the heavy-row deflation of the PCG preconditioner
 *   QPDO_IDX16       "0" disables the 16-bit slab-local column indices
 *   QPDO_PCG_SCHUR   "0" disables / "1" forces the Schur-complement mode of the PCG (default: automatic)
 *   QPDO_PCG_INNER_REFINE  how the Schur mode solves its inner (preconditioner) system S' s = b.  Default (unset or "1", one GPU, both compact
 *                    matrices under the slab kernel with 16-bit indices): the inner CG streams fp32 copies of the compact matrix values (6
 *                    instead of 10 bytes per nonzero; +4 bytes per nonzero of A and A' of device memory) and only PROPOSES corrections; after
 *                    each CG sweep the residual b - S' s is formed with the fp64 matrices and the solve is accepted on ||b - S' s||_2 <= tau
 *                    ||b||_2, today's tolerance: THE ACCEPTANCE IS IN FP64, as are all vectors, accumulations and tests.  A solve that is not
 *                    accepted after QPDO_INNER_REFINE_MAXSWEEP sweeps (default 6) is redone by the fp64 inner CG (QPDOAmdStats.inner_refine_*).
 *                    QPDO_INNER_REFINE_THETA (default 0.8): a sweep's CG runs to a recursive residual of theta tau ||b|| (cost knob).
 *                    "0": the fp64 inner CG.  Row-partitioned solves always take the fp64 inner CG
 *   QPDO_INNER_H16   "0": no coarse sweeps.  Default (with the refined inner solve and QPDO_INNER_X32 on): the first QPDO_INNER_H16_MAXSWEEP
 *                    sweeps (default 2) of a refined inner solve stream HALF-PRECISION copies of the compact matrix values, scaled by one power
 *                    of two per workspace (4 bytes per nonzero; +2 bytes per nonzero of A and A' of device memory), and stop at a recursive
 *                    residual of max(theta tau ||b||, QPDO_INNER_H16_ETA ||rho||) (default 1e-3); the sweeps behind them are the fp32 sweeps.
 *                    Acceptance is unchanged: after every sweep, on the residual of the fp64 matrices (QPDOAmdStats.inner_h16_*)
 *   QPDO_PCG_INNER_F32  "1": ONE inner CG solve on the fp32 copies, accepted on its own recursive residual -- nothing checks what the rounded
 *                    matrices did to it (opt-in, default off, never the measured configuration; overrides QPDO_PCG_INNER_REFINE); vectors,
 *                    accumulation and the outer CG on the exact K stay fp64
 *   QPDO_PCG_TOL     relative residual tolerance of the Jacobi-PCG solve (default 1e-12)
 *   QPDO_PCG_ABS     factor f of the absolute stopping rule of the PCG solve: stop when the residual, in the unscaled inf-norm of
 *                    the reference's inner dual residual, is <= f * eps_abs (default 1e-5; 0: relative rule only; proximal only)
 *   QPDO_PCG_MAXIT   PCG iteration cap per Newton step (default 100000)
 *   QPDO_SMALL_FUSED "0": never route qpdo_solve through the fused one-launch kernel (default: workspaces with n <= QPDO_SMALL_FUSED_MAX_N
 *                    = 160, m <= 1024 whose packed Newton matrix fits one workgroup's LDS, verbose = 0, no explicit QPDO_LINSOLVE)
 *   QPDO_SMALL_BATCH_KERNEL  "wide" | "lat": launch shape of a fused batch (qpdo_amd_solve_batch / batch_stream).  Default: a batch solved one at a
 *                    time takes the latency kernel (one workgroup per CU, work vectors in LDS) when it has <= 256 items or max_iter >= 1000 -- it is
 *                    as slow as its slowest item --, batches of a stream the wide one (two workgroups per CU: the throughput).  Same bits either way
 *   QPDO_FIX_STATUS_RESET  "1": reset info->status_val at the start of qpdo_solve
 *                    (the reference does not: src/qpdo.c:451-453 vs :200)
 */
#ifndef QPDO_AMD_EXT_H
#define QPDO_AMD_EXT_H

#include "qpdo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one record per loop pass of qpdo_solve (reference src/qpdo.c:343-449) */
typedef struct {
    long   kind;            /* 0 Newton step, 1 outer update, 2 terminated in this pass */
    long   n_active, n_enter, n_leave;
    long   factor_branch;   /* 0 full, 1 rank update, 2 Q only, -1 n/a (src/newton.c:21-33) */
    long   lin_iters;       /* PCG iterations of this pass (0 for the dense solver)       */
    double tau;
    double res_prim, res_dual, res_prim_in, res_dual_in;
    double sigma, eps_in;
} QPDOAmdTraceRec;

typedef struct {
    long   newton_passes;   /* passes that ran update_iterate (iterations - oterations - final) */
    long   lin_iters;       /* PCG iterations, all passes                                  */
    long   spmv_calls;      /* SpMV launches in the last solve                             */
    double spmv_alg_bytes;  /* sum over those launches of 12 nnz + 4(rows+1) + 8 rows + 8 cols */
    long   factor_count;    /* dense LDL' factorizations                                   */
    long   linsolve;        /* 0 pcg, 1 dense, 2 fused small-problem kernel, 3 band direct  */
    double spmv_Q_avg_s;    /* HIP-event average duration of the sampled Q SpMV inside PCG */
    long   spmv_Q_samples;
    double spmv_Ac_time_s;  /* Schur-mode inner solves: summed HIP-event time of the sampled A_c products ...          */
    double spmv_Ac_bytes;   /* ... and their summed algorithmic bytes (compact matrix, size changes per pass)          */
    long   spmv_Ac_samples;
    long   schur_passes;    /* Newton passes solved by the Schur-complement mode of the PCG                            */
    long   lowrank_solves;  /* dense solves through the low-rank update of the kept factor (cholmod_interface.c:57-93) */
    long   lowrank_cols;    /* rows that entered the low-rank set (one multi-RHS solve column each)                 */
    long   lowrank_sweeps;  /* refinement sweeps of the low-rank solves (one kept-factor solve + 3 SpMV each)        */
    long   lowrank_rejects; /* low-rank solves abandoned for a refactorization (ill-conditioned downdate)          */
    long   pcg_soft_accepts;/* PCG solves that stopped at the iteration cap or stagnated and were accepted because their relative
                             * residual was <= 1e-8; a worse or NaN residual ends qpdo_solve with status QPDO_ERROR instead      */
    long   collectives;     /* all-reduces issued by a row-partitioned solve (0 on one GPU)                                        */
    long   inner_solves, inner_steps, inner_collectives;   /* Schur mode: inner (preconditioner) solves, the iterations launched for them,
                             * and the all-reduces they issued: exactly one per launched iteration plus one per solve              */
    long   chain_fallbacks; /* dense triangular solves redone with the stepwise kernels (dense LDL')                  */
    double pcg_max_relres;  /* largest ||r||/||rhs|| a PCG solve of the last qpdo_solve ended with (tolerance QPDO_PCG_TOL)      */
    long   pcg_dense_fallbacks; /* PCG solves that could not converge (relative residual > 1e-8: e.g. settings->proximal = 0 on a singular
                             * Q + A'DA) and were redone by the dense LDL' solver, which the rest of that qpdo_solve then keeps (n <= 40000) */
    long   fused_solves;    /* qpdo_solve calls of this workspace that ran as ONE launch of the fused small-problem kernel (then linsolve = 2:
                             * in-LDS natural-order LDL' in the oracle's operation order, factor_count = its factorizations)                  */
    double fused_kernel_s;  /* HIP-event duration of that launch in the last qpdo_solve (0 if it took the generic path)                     */
    /* round 5 (appended: the members above keep their offsets) */
    long   pcg_rescues;     /* PCG solves that could not converge where no dense factor is possible (n > 40000 or a row partition) and were rescued */
    long   pcg_rescue_kinds;/* bit 0: the band direct solver took over (banded Newton matrix); bit 1: the pass was redone by plain Jacobi-PCG
                             * (Schur mode and deflation off, four times the iteration cap)                                                */
    long   hybrid_pcg_passes;/* hybrid PCG -> dense (default from n = 8192): Newton passes solved by PCG before the dense factor took over --
                             * `linsolve` reads 1 for such a workspace although its first passes ran PCG                                    */
    long   band_fallbacks;  /* band factorizations that met a non-positive or non-finite pivot and were redone by the dense solver / PCG   */
    long   onelaunch_factors;/* dense factorizations that ran as ONE launch of the tile-dataflow kernel (k_mid_factor, the default)          */
    long   ahead_steps;     /* Newton steps launched ahead of the host's decision (mid-size dense route, QPDO_LAUNCH_AHEAD) that ran ...   */
    long   ahead_skips;     /* ... and passes whose launched-ahead step left at once because the pass was an outer update or the last one  */
    /* in-place up/downdate of the kept dense factor (QPDO_DENSE_UPDOWN; appended: the members above keep their offsets) */
    long   updown_solves;   /* dense solves with a kept factor that carries up/downdates, accepted by their residual check (no factorization) */
    long   updown_rows;     /* changed rows of A SENT through the up/downdate (three launches each; a row its scan refuses, and the rows behind it in that
                             * pass, are counted but never touch the factor: updown_rejects); factor_count does not move on such a pass */
    long   updown_rejects;  /* up/downdated factors given up for a refactorization: a scan met a pivot that is not a positive finite number
                             * (the factor was not touched by that row), or a solve missed its residual check after the refinement sweeps */
    /* band solver with coupling rows (QPDO_BAND_COUPLING; appended: the members above keep their offsets) */
    long   coupled_rows;    /* coupling rows of the workspace (r; 0: none, or the variable is off)                                        */
    long   coupled_solves;  /* band solves with at least one weighted coupling row that were accepted by their residual check             */
    long   coupled_sweeps;  /* sweeps of those solves: one band solve, the k x k correction and 3 SpMV each (1 = accepted at once)         */
    long   coupled_rejects; /* such solves that missed the residual check after the sweeps: the pass went to the band fallback (band_fallbacks) */
    /* refined inner solves of the Schur mode (QPDO_PCG_INNER_REFINE, the default; appended: the members above keep their offsets) */
    long   inner_refine_sweeps;       /* fp32 CG sweeps that converged and were followed by a residual formed with the fp64 matrices (>= inner_solves
                                       * when no inner solve needed the fallback at its first sweep)                                           */
    long   inner_refine_fp64_applies; /* applications of S' with the fp64 matrices that formed those residuals (two products each)              */
    long   inner_refine_fallbacks;    /* inner solves redone by the fp64 inner CG: QPDO_INNER_REFINE_MAXSWEEP sweeps (default 6) did not reach the
                                       * tolerance, or a sweep did not converge                                                                */
    double inner_refine_max_res_over_tol; /* largest ||b - S' s||_2 / (tau ||b||_2) an inner solve was accepted with, fp64 residual: <= 1        */
    long   inner_x32_steps;           /* inner CG steps (inner_steps) whose two products staged fp32 copies of their operand vectors and streamed the
                                       * column slabs in pairs (the default of the narrow sweeps, coarse ones included; QPDO_INNER_X32=0: none) */
    long   inner_h16_steps;           /* inner CG steps of COARSE sweeps: both products streamed the half-precision copies of the compact matrix
                                       * values (4 bytes per nonzero; QPDO_INNER_H16=0 or QPDO_INNER_X32=0: none)                              */
    long   inner_h16_sweeps;          /* coarse sweeps among inner_refine_sweeps: the first QPDO_INNER_H16_MAXSWEEP (default 2) sweeps of a refined
                                       * inner solve, each stopped at max(theta tau ||b||, QPDO_INNER_H16_ETA ||rho||) (default 1e-3)          */
} QPDOAmdStats;

int  qpdo_amd_device_count(void);
/* What a loop pass of qpdo_solve is, from its residual norms and active-set counts (reference src/termination.c:11-30, src/qpdo.c:361-363,
 * src/newton.c:21-33): the one function behind both the host loop and the residual launch's decision on the launch-ahead route
 * (qpdo_amd/csrc/pass_decision.h).  Pure host arithmetic (no device needed): exported for the CPU tests.  res_dual / res_dual_in: already
 * multiplied by cinv.  allow_outer: iter > iter_old + 1; force_outer: iter == iter_old + inner_max_iter; n_change: n_enter + n_leave.
 * Out: the solve ends with QPDO_NON_CVX / QPDO_SOLVED, the pass is an outer update, else a Newton step with factorization branch 0 | 1 | 2. */
int  qpdo_amd_pass_decision(double res_prim, double res_dual, double res_prim_in, double res_dual_in, double eps_abs, double eps_in, int allow_outer,
                            int force_outer, int reset_newton, int n_active, int n_change, int *ends_nc, int *ends_ok, int *outer, int *branch);
const char *qpdo_amd_last_error(void);
int  qpdo_amd_get_stats(const QPDOWorkspace *work, QPDOAmdStats *out);
/* trace of the last qpdo_solve; pointer stays valid until the next solve / cleanup */
int  qpdo_amd_get_trace(const QPDOWorkspace *work, const QPDOAmdTraceRec **recs, long *count);
int  qpdo_amd_sync(QPDOWorkspace *work);

/* New values of Q and / or A in the sparsity pattern given to qpdo_setup.  Q, A: the same dimensions, stype (Q), itype-independent
 * pattern (p, i) and number of entries as at setup; only x differs.  NULL: that matrix is unchanged.  Returns 0, or nonzero with
 * qpdo_amd_last_error() set -- and then the workspace is exactly as before the call (checks precede every write).
 * After a successful call the workspace is bit for bit the one qpdo_setup returns for the new matrices, the latest UNSCALED q, l, u
 * (from setup, qpdo_update_q, qpdo_update_bounds), the constant c and the workspace's current settings: scaling computed again from
 * scratch, x = y = 0, status QPDO_UNSOLVED; info->setup_time = the call's duration.  A warm start is the caller's (qpdo_warm_start).
 * The pattern: the first call that passes a matrix compares its (p, i) with the setup's on the device; later calls compare the
 * dimensions, stype, entry counts and column pointers only -- changing row indices without changing their count is UNDEFINED.
 * Costs: the first call allocates 4 B per entry of A and of the full storage of Q (the maps; + 8 B per stored entry of Q when stype is
 * +-1); a scaled workspace keeps the unscaled values on the device from setup on (8 B per entry of A and of the full Q).
 * Not for row-partitioned workspaces (qpdo_amd_dist_config): refused. */
int  qpdo_amd_update_matrices(QPDOWorkspace *work, const cholmod_sparse *Q, const cholmod_sparse *A);

/* HIP-event timing of the SpMV kernel on the workspace's own (scaled) matrices.
 * which: 0 = A (CSR m x n), 1 = A' (CSR n x m), 2 = Q (full symmetric CSR). */
int  qpdo_amd_bench_spmv(QPDOWorkspace *work, int which, int reps, double *avg_seconds, double *alg_bytes);
/* HIP-event timing of the dense LDL' factorization (n <= QPDO_DENSE_MAX_N) with the workspace's current weights; *check
 * (optional) receives the relative residual of one solve with the fresh factor */
int  qpdo_amd_bench_dense_factor(QPDOWorkspace *work, int reps, double *avg_seconds, double *check);
/* y = M v on the device, host in/out (parity tests) */
int  qpdo_amd_spmv(QPDOWorkspace *work, int which, const double *v, double *y);
/* root of eta t + beta + delta'[delta t - alpha]_+ over 2m breakpoints (reference
 * src/linesearch.c:74-158) on the device, host in/out (parity tests) */
int  qpdo_amd_linesearch(QPDOWorkspace *work, double eta, double beta, const double *delta,
                         const double *alpha, double *tau);
/* ---- the direct solvers as single linear solves (tests of the factorizations; tests/test_gpu_direct_solvers.py) ----------------------
 * qpdo_amd_direct_solve: x (n) = K^-1 rhs (n) with K = Q + sigma I + A' diag(dw) A (dw: m weights), Q and A the workspace's stored, i.e.
 * scaled, matrices (the caller's own with settings->scaling = 0), through the workspace's direct solver exactly as a Newton pass drives
 * it: the dense LDL' (QPDO_LINSOLVE=dense, with its QPDO_DENSE_* routes) or the band LDL' (QPDO_LINSOLVE=band; with coupling rows,
 * QPDO_BAND_COUPLING, every call brings B's factor, Z and S up to date with dw: B is factored again only where a weight of another row or
 * sigma moved, or bit 0 asks for it; a solve that misses its residual check returns QPDO_AMD_DIRECT_LOST like a bad pivot).
 *   flags bit 0  refactor.  Clear: the factor kept from the previous call is reused -- with QPDO_DENSE_LOWRANK on, every row whose weight
 *                differs from the factored one gets a low-rank slot (more than 256 such rows refactor); otherwise it is reused as it is,
 *                i.e. the caller passes the factored weights.  No factor yet, or (dense) another sigma: refactor.  With QPDO_DENSE_UPDOWN on,
 *                rows whose weight differs go through the in-place up/downdate of the kept factor if they are at most its cap (and no
 *                low-rank slot is held); more rows take the low-rank path if that is on and refactor otherwise.
 *   flags bit 1  the factorization launch carries the forward solve along (one-launch route of the dense factor).
 * Returns 0; QPDO_AMD_DIRECT_LOST when a polling kernel lost its producer or the band factorization met a pivot that is not a positive
 * finite number (the latch is cleared, the result is not redone, qpdo_amd_last_error says which); -1 on any other failure, including a
 * PCG workspace and a row-partitioned one (refused).  The workspace's weights, sigma and direction are untouched; the next qpdo_solve
 * drops the kept factor and runs as on a workspace that never saw this call.
 * qpdo_amd_download_factor: copies a factor array of the last factorization to the host; count must be the array's length.
 *   which 6: the geometry, 4 entries: ld = n rounded up to 64, nb = ld / 64 (dense), np = n rounded up to 4 (to 64 for b > 127), b = the
 *            half-bandwidth (band); 0 where that solver never factored.
 *   dense, column-major, element (i, j) at [i + j ld]:
 *     0  Kd     ld x ld.  Below the diagonal: L (unit diagonal implied).  The upper triangle of every off-diagonal 64 x 64 tile holds the
 *               transposed copy that the backward solve reads: Kd(j, i) = L(i, j) for i, j in different tiles.  The diagonal and the upper
 *               triangle of a diagonal tile keep assembled values; rows / columns n .. ld-1 are identity padding.
 *     1  Dg     ld: D.
 *     2  Linv   nb x 64 x 64: the inverse of the unit-lower diagonal block k of L, column-major: Linv[k 4096 + c 64 + r] = (L_kk^-1)(r, c).
 *     3  LinvT  the same blocks transposed: LinvT[k 4096 + c 64 + r] = (L_kk^-1)(c, r).
 *   band, lower band storage, np x (b + 1):
 *     4  Kb     Kb[j (b+1) + t] = L(j + t, j) for t >= 1, D_j at t = 0 (zero beyond the matrix; columns n .. np-1 identity padding).
 *     5  Lt     Lt[i (b+1) + t] = L(i, i - t), the row-band copy the backward solve reads (t >= 1).
 *   band with b > 127, 64 x 64 tiles, w = (b + 63) / 64 (arrays 4 and 5 return -1 with a message on such a workspace):
 *     7  Wb     (np / 64) x (w + 1) x 64 x 64: Wb[(J (w+1) + s) 4096 + c 64 + r] = element (r, c) of tile (J + s, J) of the unit-lower L
 *               (diagonal tiles: 1 on the diagonal, 0 above it; rows / columns n .. np-1 identity padding; tiles whose block row is
 *               >= np / 64 are zero).  An element outside the band, i - j > b, is an exact zero.
 *     8  Wd     np: D (ones behind n).
 *   band with coupling rows (QPDO_BAND_COUPLING; arrays 4 and 5 hold the factor of B, which 6 its geometry):
 *     9  the coupled geometry, 4 entries: r = the coupling rows of the workspace, k = those with a nonzero weight at the last factorization,
 *            b_core, np (k and np 0 before the first factorization).
 *    10  the r coupling row numbers, ascending, as doubles.
 *    11  Z      np x k, leading dimension np: column j = B^-1 (the j-th weighted coupling row, ascending, as a dense column).
 *   band under a variable order (qpdo_amd_band_order_config below):
 *    12  newold n entries as doubles: newold[k] = the caller's index of the variable at position k of the solver's order (-1 with a
 *               message on a workspace that adopted none).  On such a workspace arrays 4, 5, 7 and 8 are in the SOLVER's order: they
 *               hold the factor of P K P', P K P'(k, l) = K(newold[k], newold[l]).
 *   band with border variables (QPDO_BAND_BORDER; arrays 4 and 5 hold the factor of the core B, which 6 its geometry):
 *    13  the border geometry, 4 entries: n_core, c, b_core, np = n_core rounded up to 4 (0 before the first factorization).
 *    14  C      np x c, leading dimension np: column j = K(0 .. n_core-1, n_core + j) (rows n_core .. np-1 zero).
 *    15  Z      np x c, leading dimension np: column j = B^-1 C(:, j) (-1 with a message on a workspace without a border).  */
#define QPDO_AMD_DIRECT_LOST (-2)
int  qpdo_amd_direct_solve(QPDOWorkspace *work, const double *dw, double sigma, const double *rhs, double *x, int flags);
int  qpdo_amd_download_factor(QPDOWorkspace *work, int which, double *dst, long count);
/* ---- a variable order for the band solver (qpdo_amd/csrc/band_order.c) ------------------------------------------------------
 * The band solver factors K in the order of its variables; band_detect measures the half-bandwidth in the caller's order.  A chain QP
 * whose variables are not numbered along the chain (all states, then all inputs; one block per signal) is banded only after a
 * relabelling.  Opt-in: with nothing configured every workspace, launch and bit is what it is without this section.
 *
 * qpdo_amd_band_order: reverse Cuthill-McKee on the pattern of Q + A'A (never formed: the search walks the rows of A), O(nnz), pure
 *   host code, deterministic.  Q's stype is honoured as qpdo_setup honours it, explicit zeros count, both itypes; A may be NULL or
 *   have no rows.  newold[k] = the caller's index of the variable that takes position k (n entries); info4 (may be NULL) =
 *   {b_natural, b_ordered, connected components, early_out}: the exact half-bandwidths (the largest |i - j| over the stored entries
 *   of Q, the largest column span over the rows of A) in the caller's order and under newold -- the solver itself never goes below 3.
 *   A row of A with more than 1024 entries forces a half-bandwidth above 1023 under every order: the identity comes back at once,
 *   early_out = 1.  Degrees are exact (distinct neighbours; sum of squared row lengths of work, at most 1024 nnz(A)); the searches
 *   are O(nnz).  Returns 0, or -1 (bad arguments, no memory).
 * qpdo_amd_band_order_config: applies to the workspaces set up afterwards in this process (read once per qpdo_setup, as
 *   qpdo_amd_dist_config).  ENV (the default): QPDO_BAND_ORDER decides.  RCM: qpdo_setup runs qpdo_amd_band_order and adopts the
 *   order only if b_ordered < b_natural; otherwise the workspace is the natural-order one, bit for bit, nothing allocated.  GIVEN:
 *   newold (n entries, copied) is adopted always, the identity included; -1 with a message if it is not a permutation of 0 .. n-1,
 *   and a qpdo_setup whose n differs fails with a message.  The selection rule of QPDO_LINSOLVE then runs on the adopted
 *   half-bandwidth (automatic: b <= 127 and n >= 2048; "band": b <= 1023 and n >= 4 (b + 1)), the PCG rescue included.
 *   An adopted order costs two int32 arrays of n on the device.  The assembly kernels write the band of P K P' (the same bits the
 *   natural-order band of K holds for the same entries); every solve takes its right-hand side and delivers its solution in the
 *   CALLER's order -- the gather and the scatter are folded into the solve kernels' first load and last store: one launch per solve,
 *   as without an order -- so qpdo_amd_direct_solve, qpdo_amd_adjoint / _tangent (groups of 8 included), the band fallback ladder,
 *   qpdo_amd_update_matrices (fixed pattern: the order stays) and qpdo_update_q see no difference.
 *   IGNORED (the natural order is kept, `reason` says why): 2 row-partitioned workspaces; 3 QPDO_BAND_COUPLING > 0 (a coupling row is
 *   wide under every order); 4 workspaces on the fused small-problem route; 5 QPDO_LINSOLVE = dense or pcg; 6 a workspace that adopted
 *   a border of coupling variables (QPDO_BAND_BORDER: an arrowhead is wide under every order).  reason 1: RCM found no narrower order.
 *   0: adopted, or nothing configured.
 * qpdo_amd_get_band_order: what the workspace's setup decided; newold (n entries, or NULL) is written only when adopted = 1. */
#define QPDO_AMD_BAND_ORDER_ENV     0   /* default: QPDO_BAND_ORDER in the environment decides ("rcm"; unset, "" or "0": natural) */
#define QPDO_AMD_BAND_ORDER_NATURAL 1
#define QPDO_AMD_BAND_ORDER_RCM     2
#define QPDO_AMD_BAND_ORDER_GIVEN   3   /* newold (n entries, copied; must be a permutation of 0..n-1, else -1 with a message) */
typedef struct { long mode, adopted, b_natural, b_ordered, reason; double order_seconds; } QPDOAmdBandOrderInfo;
int  qpdo_amd_band_order(const cholmod_sparse *Q, const cholmod_sparse *A, long *newold, long *info4);
int  qpdo_amd_band_order_config(int mode, const long *newold, long n);
int  qpdo_amd_get_band_order(const QPDOWorkspace *work, QPDOAmdBandOrderInfo *out, long *newold /* n entries or NULL */);
/* ---- a border of coupling variables over a band core (QPDO_BAND_BORDER above; qpdo_amd/csrc/band_border.c) ---------------
 * qpdo_amd_band_border: the detection, O(nnz), pure host code, deterministic.  With T = 127, n_core starts at n; a stored entry (i, j) of Q
 *   with |i - j| > T sets n_core <= max(i, j); a row of A with ascending columns c1 < c2 < ... sets n_core <= the first column that
 *   exceeds c1 + T (every column of the row below that one is then within T of every other).  info4 = {n_core, c = n - n_core, b_core,
 *   reason}: b_core = the half-bandwidth of the pattern restricted to the columns < n_core, at least 3; reason = 1 when c > max_border,
 *   else 0.  The border variables are the TRAILING ones: number shared variables last.  Q's stype is honoured as qpdo_setup honours it,
 *   explicit zeros count, both itypes, row indices in any order within a column; A may be NULL or have no rows.  Returns 0, or -1 (bad
 *   arguments, no memory).
 * qpdo_amd_get_band_border: what the workspace's setup decided.  max_border: C as read (0: unset); border: the adopted c (0: none);
 *   n_core, b_core: the detection's (0 where it did not run); over: a c that was seen and not adopted; reason: 0 adopted, no border or
 *   unset; 1 c > C; 2 row-partitioned; 3 QPDO_BAND_COUPLING > 0; 4 the fused small-problem route; 5 QPDO_LINSOLVE = dense or pcg; 6 the
 *   core is too short for the selection rule.  border_solves: the solves by block elimination since the counters were last reset (with
 *   QPDOAmdStats). */
typedef struct { long max_border, border, n_core, b_core, over, reason; long border_solves; } QPDOAmdBandBorderInfo;
int  qpdo_amd_band_border(const cholmod_sparse *Q, const cholmod_sparse *A, long max_border, long *info4);
int  qpdo_amd_get_band_border(const QPDOWorkspace *work, QPDOAmdBandBorderInfo *out);
/* ---- the PCG linear-solve path as single steps (tests of its pieces; tests/test_gpu_pcg_pieces.py) ------------------------------------
 * K = Q + sigma I + A' diag(dw) A with the workspace's stored matrices (the caller's own with settings->scaling = 0), dw: m weights; a row
 * is "weighted" when dw_i != 0.0 (so -0.0 is not, a subnormal is).  Only for PCG workspaces (QPDO_LINSOLVE=pcg) on one GPU: a dense, band
 * or row-partitioned workspace is refused (-1).  dw, v, out and info must not be NULL, also where m = 0.
 * qpdo_amd_pcg_probe, info: QPDO_AMD_PCG_INFO_LEN doubles.
 *   mode 0  the per-pass compact matrices are built from dw and ONE K product runs on p = v (n): out (n) = K v.  info[0] = k, the number of
 *           weighted rows; info[1] = cnt; info[16 .. 16 + cnt) = the per-workgroup partial sums of p.Kp as the device left them.
 *   mode 1  ONE solve of K x = v exactly as a Newton pass runs it (Schur-complement mode, heavy-row deflation, graph replay as the workspace
 *           is configured), with the relative stopping rule ||r||_2 <= pcg_tol ||v||_2 alone: out (n) = x.  info[0] = k, [1] = iterations
 *           (Schur mode: outer + inner steps), [2] = deflated rows, [3] = 1 when the Schur mode delivered x, [4], [5] = the recursive residual
 *           and right-hand side 2-norms of the last iteration, [6], [7] = inner solves and inner steps launched, [8] = class: 0 ok,
 *           1 not converged, 2 NaN residual, [9] = iterations of the outer CG alone (= [1] outside the Schur mode), [10] = 1 when the Schur
 *           mode took its inner diagonal from the pass's one read of the weighted rows (QPDO_COMPACT_ONE_READ), 0 when k_schur_diag ran.
 *   mode 32, 33  the compact matrices are built from dw and ONE product runs through the slab kernel's fp32-stream instance (the stream of the
 *           refined inner solve): mode 32 out[0 .. k) = A_c32 v, mode 33 out (n) = A_c32' v[0 .. k), A_c32 = the compact values rounded to float,
 *           products and sums in double.  info[0] = k.  Refused (-1) where the pass has no fp32 images: a compact matrix on the plain kernel
 *           or without 16-bit indices, QPDO_PCG_INNER_REFINE=0 without QPDO_PCG_INNER_F32=1, or k > n.
 *   mode 34, 35  the same two products through the pair-wide instance that the fp32 inner CG runs by default: v is rounded to float as well
 *           and the column slabs are streamed in pairs; products and sums in double (a float times a float is exact there).  Refused
 *           (-1) as modes 32, 33 and under QPDO_INNER_X32=0.
 *   mode 36, 37  the same two products through the pair-wide HALF-PRECISION instance that the coarse sweeps of the refined inner solve run:
 *           the values are those of the half-precision image -- (half)(float)(a 2^e), one power of two per workspace with max |a_ij| 2^e in
 *           [2^14, 2^15) -- v is rounded to float, products and sums in double, the row sums times 2^-e.  info[0] = k, info[1] = e.  Refused
 *           (-1) as modes 34, 35, under QPDO_INNER_H16=0 and where max |a_ij| is 0 or not finite.
 * Returns 0; QPDO_AMD_PCG_NOT_CONVERGED / QPDO_AMD_PCG_NAN for a solve of class 1 / 2 (out is not written, qpdo_amd_last_error carries the
 * solver's message); -1 on any other failure.  The workspace's weights, sigma, direction, right-hand side, stopping rule, Schur-mode
 * state and counters are put back: the next qpdo_solve runs as on a workspace that never saw the call.
 * qpdo_amd_download_compact: what the last probe (or Newton pass) left; count = the number of ELEMENTS and must be the array's length.
 *   which = 16 mat + part, mat 0 A_c (k x n: the weighted rows of A), 1 A_c' (n x k: CSR(A') restricted to them, columns renumbered),
 *   2 A_h' (n x k: the deflated columns of A_c', after a deflated solve only); refused while the last pass built no such matrix (k = 0):
 *     part 0  geometry, 7 x int64: nrows, ncols, nnz, use_slab, nslabs, W, ci16 present
 *          1  rp   int32  nrows + 1         2  ci  int32  nnz         3  val  double  nnz
 *          4  ci16 uint16 nnz: ci mod W (slab kernel with 16-bit indices; count 0 where absent)
 *          5  sp   int32  nrows x (nslabs + 1): sp[r (nslabs + 1) + s] = first position of row r whose column is >= s W, sp[.. + nslabs] =
 *                  the row's end (slab kernel; count 0 where absent)
 *   48 index space, 5 x int64: n, m, k, words = (m + 63) / 64, deflated rows
 *   49 rowlist int32 k: the weighted rows, ascending      50 cidx int32 m: weighted rows before row i      51 dc double k: their weights
 *   52 flag_bits uint64 words: bit b of word w = row 64 w + b is weighted      53 flag_wprefix int32 words: cidx[64 w]
 *   54 pc_diag double n: the diagonal preconditioner of the last solve (Jacobi route: Q_jj + sigma + sum_i A_ij^2 dw_i; Schur mode: Q_jj +
 *      sigma; deflated: the remainder without the heavy rows, floored)      55 s_diag double k: Schur mode, 1 / dw_i + sum_j A_ij^2 / pc_diag_j
 *   56 defl_list int32 (deflated rows): their compact row numbers      57 defl_Sinv double 256 x 256, row stride 256: the inverse of
 *      S = D_h^-1 + A_h P^-1 A_h' in its leading block
 *   59 int64 2: [1 where the images of A_c and A_c' carry half-precision values (mode 36, 37 available), else 0; the exponent e of their scale]
 *   60 ls_idx uint32 2 m: the breakpoint indices in the order the last linesearch's radix sort left them (2 m > 8192, or QPDO_LS_SMALL=0;
 *      candidates first, by ratio, ties by index)
 *   which = 64 + 16 mat + part, mat 0 A_c, 1 A_c': the slab-major image that the slab kernel streams (count 0 where the matrix does not
 *   take the slab kernel):
 *     part 0  seg  int32 pairs, 2 nrows nslabs: seg[r nslabs + s] = {first position in the image, length} of row r's entries in slab s
 *          1  vsm  double nnz: the values, per workgroup the segments of slab 0 back to back, then those of slab 1, ...; where the pair-wide
 *                  products run on the matrix (mode 34, 35 available) in pair order instead: per workgroup the slab pairs (0, 1), (2, 3), ..., in a pair the
 *                  rows, per row its segment of the even slab and then that of the odd one (adjacent), an odd last slab by rows
 *          2  the slab-local column indices in the same order: uint16 where ci16 is present, else int32 (ci - s W)
 *          3  vsm16  IEEE half nnz: (half)(float)(vsm 2^e) in the same order, the stream of the coarse sweeps (count 0 where which 59 says 0)
 *          4  p16sm  uint16 nnz: the pair-local column indices of an image in pair order, part 2's index plus W for an entry of the odd
 *                  slab of a pair -- what the pair-wide products gather with (count 0 where the image is not in pair order)
 *   96 (count 0, dst unused): marks both images stale and runs one product with each compact matrix that takes the slab kernel, so
 *      that the image is rebuilt from the CSR, sp and seg as after any change of the row-major arrays */
#define QPDO_AMD_PCG_NOT_CONVERGED (-3)
#define QPDO_AMD_PCG_NAN (-4)
#define QPDO_AMD_PCG_INFO_LEN 1040
int  qpdo_amd_pcg_probe(QPDOWorkspace *work, const double *dw, double sigma, const double *v, double *out, int mode, double *info);
int  qpdo_amd_download_compact(QPDOWorkspace *work, int which, void *dst, long count);
/* The trip shape of the slab kernel's instance that streams values of value_bytes (8 double, 4 float, 2 half) against a staged operand
 * of operand_bytes (8 double, 4 float): shape = {EPL, UNR, NSA, TPR}.  A lane group of TPR lanes walks a row segment in trips of EPL UNR TPR
 * entries from the segment's start rounded down to EPL entries; lane l's load u of a trip holds the EPL entries from EPL (TPR u + l) on;
 * entry EPL u + e of a lane's trip is added to the lane's partial sum (EPL u + e) mod NSA; the NSA sums are folded in pairs, in order, and
 * the lanes' sums by a shuffle tree (offsets TPR / 2 down to 1); a row's segments are added in slab (operand_bytes 4: slab-pair) order.
 * For tests that reproduce the kernel's summation order.  Needs no workspace and no GPU.  Returns 0, or -1 for a combination that no
 * instance streams (8/8, 4/8, 4/4 and 2/4 exist) or a NULL shape. */
int  qpdo_amd_slab_trip_shape(int value_bytes, int operand_bytes, int *shape);
/* copy a device-resident vector to the host: 0 x, 1 Qx, 2 y, 3 mu, 4 d (factor weights),
 * 5 dx, 6 dy, 7 Ax, 8 Aty, 9 l, 10 u, 11 ybar, 12 xbar, 13 w (of the last loop pass that ran) */
int  qpdo_amd_download(QPDOWorkspace *work, int which, double *dst);
/* ---- the ADJOINT of a workspace's last solve: gradients of the solution w.r.t. q, l, u, Q, A at every size the direct solvers take ----------
 * The contract of qpdo_amd_fleet_adjoint_dev / _adjoint_multi_dev (below), applied to ONE workspace on its own direct solver.  All pointers
 * are HOST pointers, as for every other single-workspace entry point.  Arrays are right-hand-side major: right-hand side r of an array whose
 * per-RHS length is L (n, m, nnz(Q as stored), nnz(A)) starts at r * L.  All quantities are the caller's UNSCALED ones; x, y are the ones
 * qpdo_solve delivered in work->solution: the call uploads them and forms the scaled x itself, it reads nothing of the iterate state on the
 * device, and so it also works after a solve that ran as the fused one-launch kernel.
 * ACTIVE SET  t = Ax + y.  Row i is upper-active (flag +1) if t_i >= u_i, else lower-active (-1) if t_i <= l_i, else inactive (0).  A bound of
 *          magnitude >= 1e20 is never reached.  The rule is evaluated in the workspace's scaled space (E_i t_i against the stored scaled
 *          bounds), so a row within rounding of a bound may fall either way: the call DELIVERS its flags (`active`, m int32, ONE array: the
 *          flags depend on the solve, not on the right-hand side), and everything else is defined by them.  S: the flagged rows, k = |S|.
 * SYSTEM   Given gx = dL/dx (nrhs x n) and gy = dL/dy (nrhs x m, or NULL = zero; entries of inactive rows are ignored and may hold anything,
 *          NaN included):
 *              [ Q    A_S' ] [vx]   [ gx   ]
 *              [ A_S  0    ] [vy] = [ gy_S ]
 *          dq = -vx;  du_i = vy_i on +1 rows, dl_i = vy_i on -1 rows, every other entry of dl, du an exact +0.0;  for a stored entry (i, j) of
 *          A: -(y_i vx_j + vy_i x_j) on a flagged row, else +0.0;  for a stored entry (a, b) of Q: -vx_a x_b (stype 0), -(vx_a x_b + vx_b x_a)
 *          (off-diagonal, stype +-1), -vx_a x_a (diagonal); a stored entry in the triangle that stype +-1 ignores gets +0.0.  dAx follows the
 *          order of data->A->x at setup, dQx the order of Q->x as stored at setup; both are evaluated from the very dq, dl, du delivered.
 *          Q is needed only with dQx: the first such call compares its pattern with the setup's on the device (and, for stype +-1, builds the
 *          map that qpdo_amd_update_matrices builds on its first call with a Q; whichever call comes first builds it); later calls compare
 *          the column pointers.  A workspace with m = 0 solves Q vx = gx.
 * METHOD   The fleet's, on the scaled matrices Qs, As: sigma = 1e-10 s, W_i = 1e10 s / ||row i of As||^2 on flagged rows and 0 elsewhere, s the
 *          largest |diagonal entry| of Qs (1 when there is none).  K = Qs + sigma I + As' W As is factored ONCE per call by the workspace's
 *          direct solver -- always a full factorization, whatever QPDO_DENSE_LOWRANK / QPDO_DENSE_UPDOWN say --, and per right-hand side
 *          K dvx = rx + As_S' W ry,  dvy = W (As_S dvx - ry)  is repeated on the residual (rx, ry) of the TRUE system (no sigma, no W^-1);
 *          the right-hand sides follow one another on the one factor, each with the single call's operations in its order: slab r of an
 *          nrhs = R call carries the bits of the nrhs = 1 call with that gx / gy, and the same call twice returns the same bits.
 * ACCEPTANCE  max(||Q vx + A_S' vy - gx||_inf, ||A_S vx - gy_S||_inf) <= tol * max(||gx||_inf, ||gy_S||_inf), on the true residual in unscaled
 *          terms, looked at before every sweep; at most max_sweeps sweeps.  A residual that is not finite is never accepted.
 * status   nrhs x 3: (code, sweeps, k).  code 0: accepted.  1: not accepted within max_sweeps (an inconsistent, singular or very
 *          ill-conditioned system; this right-hand side's own).  3: a pivot of K that is not a positive finite number, or a polling kernel of
 *          the triangular solves that lost its producer; the latch is cleared as qpdo_amd_direct_solve clears it, nothing is redone, code 3
 *          repeats for every r and `active` is all 0.  A right-hand side with code != 0 gets NaN in all its slices of dq, dl, du, dQx, dAx and
 *          NaN in res[r]; res[r] of an accepted one is its relative residual.  (There is no code 2: a workspace that is not solved is refused.)
 * Accepted workspaces: one GPU; the workspace's solver is the dense LDL' or the band LDL' of every kind -- half-bandwidth <= 127, the
 *          tiled wide band (128 .. 1023), either in the natural order or under an adopted variable order (QPDO_BAND_ORDER), and
 *          half-bandwidth <= 127 with coupling rows (QPDO_BAND_COUPLING).  With coupling rows K = B + U W_c U' (B: the band part, U: the
 *          flagged coupling rows, W_c: their weights) is not factored as one matrix: B and S = W_c^-1 + U' B^-1 U are, once per call, and
 *          the solve of every sweep is ONE Woodbury application dvx = z0 - Z S^-1 U' z0, z0 = B^-1 rhs, Z = B^-1 U, without the residual
 *          check and the refinement a Newton pass wraps around it: the sweeps already refine on the true system.  Such a workspace TAKES
 *          MORE SWEEPS than a plain band one (3 .. 8 against 2 on the test instances), and an inner solve that is too inexact ends as
 *          code 1, never as code 3; code 3 there is a pivot of B or of S that is not a positive finite number.  When no coupling row is
 *          flagged, the plain band solve on B is the whole solve.
 *          Refused with a message that names what to do instead: PCG workspaces, hybrid workspaces (the automatically chosen dense solver
 *          from n = 8192, whose solves start with PCG: set QPDO_LINSOLVE=dense), row-partitioned workspaces.
 * Checks   all before anything is launched or written; a refused call returns nonzero with qpdo_amd_last_error() set and leaves every
 *          output array untouched.  The first fault in this order is reported: nrhs < 1; tol not a positive finite number; max_sweeps < 1;
 *          NULL gx, dq, dl or du; dQx without Q; NULL workspace; info->status_val != QPDO_SOLVED; THE MOST RECENT STATE-CHANGING CALL WAS NOT A
 *          SOLVE -- qpdo_warm_start, qpdo_update_q, qpdo_update_bounds or qpdo_amd_update_matrices since the last qpdo_solve mean that the
 *          resident q, l, u or matrices are no longer those of the x, y in work->solution (the adjoint and the getters do not count: several
 *          adjoint calls may follow one solve) --; the solver kind; the shape, stype, entry count and pattern of Q.
 * No trace The call writes none of the workspace's state, solution, matrices, q, l, u, info, trace or QPDOAmdStats: what it overwrites on
 *          the way (the factor weights, sigma, the direction and right-hand side vectors, the counters) is put back, and the factor it leaves
 *          is dropped by the next qpdo_solve, as after qpdo_amd_direct_solve.  Every later qpdo_solve carries the bits it would have had.
 * Stats    QPDOAmdAdjointStats: calls that launched, their right-hand sides, factorizations (one per call), sweeps of all right-hand sides,
 *          the device memory the calls hold -- 6 n + 7 m doubles and m flags of work vectors, allocated by the FIRST call (a host
 *          allocation: THAT CALL MAY BLOCK until earlier device work has finished), plus one array per entry of A / of the stored Q from the
 *          first call that asks for dAx / dQx; freed by qpdo_cleanup --, and the wall time of the last call. */
typedef struct {
    long   calls, rhs_total, factorizations, sweeps_total, scratch_bytes;
    double last_seconds;
} QPDOAmdAdjointStats;
int  qpdo_amd_adjoint(QPDOWorkspace *work, long nrhs,
                      const double *gx /* nrhs x n */, const double *gy /* nrhs x m or NULL */,
                      double *dq /* nrhs x n */, double *dl /* nrhs x m */, double *du /* nrhs x m */,
                      const cholmod_sparse *Q /* the setup's Q pattern; needed only with dQx */,
                      double *dQx /* nrhs x nnz(Q as stored) or NULL */, double *dAx /* nrhs x nnz(A) or NULL */,
                      int *active /* m int32 or NULL */, long *status /* nrhs x 3 or NULL */, double *res /* nrhs or NULL */,
                      double tol, long max_sweeps);
int  qpdo_amd_get_adjoint_stats(const QPDOWorkspace *work, QPDOAmdAdjointStats *out);
/* ---- the TANGENT of a workspace's last solve: the first-order change (dx, dy) of the solution for a change of q, l, u, Q, A -----------------
 * The contract of qpdo_amd_fleet_tangent_dev (below), applied to ONE workspace on its own direct solver, at every size qpdo_amd_adjoint
 * takes: the advanced-step update x + dx of an MPC controller from one factorization and a few triangular solves instead of a re-solve, or
 * a few columns of dx / dtheta without the n right-hand sides the adjoint would need.  All pointers are HOST pointers.  Arrays are
 * right-hand-side major: right-hand side r of an array whose per-RHS length is L (n, m, nnz(Q as stored), nnz(A)) starts at r * L.  All
 * quantities are the caller's UNSCALED ones; x, y are those in work->solution (uploaded by the call, as the adjoint does).
 * ACTIVE SET  the rule, the flags and k are exactly those qpdo_amd_adjoint delivers after the same solve (one classification code for both
 *          calls); `active` is ONE array of m int32.  S: the flagged rows; b = u on +1 rows and l on -1 rows.
 * SYSTEM   Given a perturbation (tq, tl, tu, tQ, tA) of the data:
 *              [ Q    A_S' ] [dx  ]   [ -(tq + tQ x + tA_S' y_S) ]
 *              [ A_S  0    ] [dy_S] = [  tb_S - tA_S x           ]
 *          dy_i is an exact +0.0 off S.  A NULL array is a zero perturbation; all five NULL is refused ("no tangent passed").  tQx follows
 *          the order of Q->x as stored at setup, tAx the order of data->A->x at setup.  tQ acts as the symmetric matrix its stored entries
 *          stand for: under stype +-1 an off-diagonal stored entry (a, b) contributes to rows a and b and an entry in the ignored triangle
 *          contributes nothing; under stype 0 the caller passes a SYMMETRIC perturbation (as the solver reads a stype-0 Q as symmetric) and
 *          row a is evaluated from the stored entries of COLUMN a.  Q is needed only with tQx and is looked at as qpdo_amd_adjoint looks at
 *          it with dQx (the first such call of either kind, or of qpdo_amd_update_matrices, compares the pattern on the device and builds
 *          the map).  A workspace with m = 0 solves Q dx = -(tq + tQ x).
 * IGNORED  tl on a row that is not -1, tu on a row that is not +1 and tAx on an unflagged row are ignored and may hold anything, NaN
 *          included: the kernels branch past them (they are not multiplied by zero).
 * RIGHT-HAND SIDE  formed in fp64 on the device from the unscaled x, y, by 16 lanes per row with a FIXED split and fold.  Component rx_j:
 *          lane L (0 .. 15) adds, into one partial sum that starts at 0, the products of the entries L, L + 16, ... of row j of tQ in
 *          stored order (stype 0: the stored entries of column j; stype +-1: row j of the symmetric image, ascending columns) and then
 *          those of the entries L, L + 16, ... of column j of tA in the caller's CSC order (flagged rows only); the 16 partial sums are
 *          folded pairwise at distances 8, 4, 2, 1 (lane L += lane L + distance); rx_j = -(tq_j + fold).  Component ry_i of a flagged row:
 *          the same split and fold over the entries of row i of tA in column order; ry_i = tb_i - fold.  Nothing else enters: the
 *          right-hand side depends on the inputs of ITS slab alone.
 * METHOD   qpdo_amd_adjoint's, by the same code: ONE full factorization of K per call with the adjoint's sigma and W, then per right-hand
 *          side the adjoint's sweeps on the true residual (the KKT matrix of the active set is symmetric: the adjoint's driver is fed (rx, ry)
 *          where the adjoint feeds it (gx, gy)).  The right-hand sides follow one another on the one factor: slab r of an nrhs = R call
 *          carries the bits of the nrhs = 1 call with slab r of the inputs, and the same call twice returns the same bits.
 * ACCEPTANCE  the true unscaled residual's inf-norm <= tol * max(||rx||_inf, ||ry_S||_inf), looked at before every sweep; at most max_sweeps
 *          sweeps.  A non-finite entry among those used is never accepted (code 1).  A zero right-hand side is accepted at sweep 0 with zeros.
 * status   nrhs x 3: (code, sweeps, k); codes 0, 1 and 3 with the adjoint's meaning.  A right-hand side with code != 0 gets NaN in its slices
 *          of dx and dy and NaN in res[r]; code 1 is that right-hand side's own and touches no other.  After code 3 `active` is all 0.
 * Accepted workspaces and refusals: those of qpdo_amd_adjoint, by the same function -- the wide band, a variable order and coupling rows
 *          included, with the adjoint's one Woodbury application per sweep and its larger sweep counts on a workspace with coupling rows;
 *          PCG, hybrid and row-partitioned workspaces are refused; the messages begin with "qpdo_amd_tangent:".
 * Checks   all before anything is launched or written; a refused call returns nonzero with qpdo_amd_last_error() set and leaves every
 *          output array untouched.  The first fault in this order is reported: nrhs < 1; tol not a positive finite number; max_sweeps < 1;
 *          NULL dx or dy; no tangent passed; tQx without Q; NULL workspace; info->status_val != QPDO_SOLVED; the most recent state-changing
 *          call was not a solve (the adjoint's flag; the call itself is not state-changing: any mix of adjoint and tangent calls may
 *          follow one solve); the solver kind; the shape, stype, entry count and pattern of Q.
 * No trace The call writes none of the workspace's state, solution, matrices, q, l, u, info, trace, QPDOAmdStats or QPDOAmdAdjointStats (nor
 *          does qpdo_amd_adjoint move QPDOAmdTangentStats); every later qpdo_solve carries the bits it would have had.
 * Stats    QPDOAmdTangentStats, the adjoint's members for the tangent calls.  The 6 n + 7 m doubles and m flags of work vectors are SHARED
 *          with qpdo_amd_adjoint and booked in scratch_bytes of whichever kind of call allocated them; the staging of one right-hand
 *          side's tq, tl, tu, tQx, tAx is the tangent's own, each array allocated by the first call that passes it (with tAx, on a workspace
 *          that never saw qpdo_amd_update_matrices, also the map from CSR(A) to the caller's order); freed by qpdo_cleanup.  These are host
 *          allocations: THE FIRST CALL (and the first that passes a further array) MAY BLOCK until earlier device work has finished. */
typedef struct {
    long   calls, rhs_total, factorizations, sweeps_total, scratch_bytes;
    double last_seconds;
} QPDOAmdTangentStats;
int  qpdo_amd_tangent(QPDOWorkspace *work, long nrhs,
                      const double *tq /* nrhs x n or NULL */, const double *tl /* nrhs x m or NULL */, const double *tu /* nrhs x m or NULL */,
                      const cholmod_sparse *Q /* the setup's Q pattern; needed only with tQx */,
                      const double *tQx /* nrhs x nnz(Q as stored) or NULL */, const double *tAx /* nrhs x nnz(A) or NULL */,
                      double *dx /* nrhs x n */, double *dy /* nrhs x m */,
                      int *active /* m int32 or NULL */, long *status /* nrhs x 3 or NULL */, double *res /* nrhs or NULL */,
                      double tol, long max_sweeps);
int  qpdo_amd_get_tangent_stats(const QPDOWorkspace *work, QPDOAmdTangentStats *out);
/* ---- GROUPS of right-hand sides in qpdo_amd_adjoint / qpdo_amd_tangent ----------------------------------------------------------------------
 * Both calls keep their contracts above, every sentence of them.  What a group size G > 1 changes is WHEN the work is launched: a call with
 * nrhs = R > 1 takes its right-hand sides in ceil(R / G) groups of up to G (the last may be partial), and inside a group every launch of
 * the sweep loop -- the five products (a multi-vector CSR product: one read of the matrix, a gather per right-hand side), the four vector
 * kernels, the two triangular solves (one column per right-hand side) -- is made ONCE for the group, with ONE read-back per sweep.  Every
 * right-hand side still receives the single call's operations in the single call's order: slab r carries the bits of the nrhs = 1 call
 * with slab r of the inputs.  A right-hand side leaves the sweeps at its own sweep count (accepted, or code 1 at max_sweeps); from then on
 * no launch reads or writes its vectors.  The non-finite marker is per right-hand side (a code 1 touches no other); the code-3 latch is the
 * call's: it hits the right-hand sides of the group in flight and all behind it.  A call with nrhs = 1 runs the G = 1 code path.
 * G        8 where the workspace is one the two calls accept, Q, A and A' all take the plain CSR kernel, and the solver is the band LDL'
 *          (every kind the calls accept: b <= 127, the wide band 128 .. 1023, a variable order, coupling rows) or the dense LDL' with the
 *          chained one-launch solves.  The band solves of a group run the single solve's kernel body once per live right-hand side, one
 *          workgroup each (k_band_solve_group, k_bw_solve_group and their _perm instances); with coupling rows the Woodbury application's
 *          three launches are made once per group (k_band_solve_group, k_bc_t_group, k_bc_apply_group), and a group's right-hand sides
 *          may leave at different sweep counts.  G = 1 (the right-hand sides follow one another): a matrix on
 *          the slab kernel (>= 192 MB, QPDO_SPMV) -- a multi-vector slab product does not exist --, and the stepwise dense solves
 *          (QPDO_DENSE_SOLVE=steps, or after a lost producer).  QPDO_AMD_RHS_GROUP=1..8 in the environment at qpdo_setup overrides G (a
 *          measuring switch, as QPDO_AMD_FLEET_RHS_GROUP is for the fleet; tools/workspace_group_latency.py); 1 runs the launch sequence
 *          of a build without groups.
 * Scratch  G copies of the per-right-hand-side work vectors (5 n + 5 m doubles each; x, y, the row norms and the flags are shared with the
 *          single path), the solves' columns (G x (n + 5 ld) doubles, ld = n rounded up to 64; the band routes' columns -- with coupling
 *          rows z0 and t too -- lie inside them) and the group control array, allocated
 *          ONCE by the first call of either kind with nrhs > 1 on a workspace with G > 1 -- host allocations: THAT CALL MAY BLOCK until
 *          earlier device work has finished --, booked in QPDOAmdGroupStats.scratch_bytes ALONE (not in the two calls' scratch_bytes), freed
 *          by qpdo_cleanup.  No trace: as before, with these buffers included.
 * qpdo_amd_rhs_group  G >= 1 as the workspace stands; 0: a workspace the two calls refuse; -1: NULL.
 * qpdo_amd_spmv_group  test hook beside qpdo_amd_spmv: slab g of y (nvec x nrows) = M (slab g of v, nvec x ncols) for every g in
 *          live_mask, bit for bit what qpdo_amd_spmv returns for that slab; slabs outside the mask are not written.  nvec 1..8.  Refused
 *          (-1, message), before any device call: nvec out of range, a mask bit >= nvec, which not 0 (A), 1 (A') or 2 (Q), NULL pointers; then a row-partitioned workspace
 *          and a matrix on the slab kernel. */
typedef struct {
    long group;         /* = qpdo_amd_rhs_group */
    long groups_run;    /* groups carried through the sweep driver by adjoint + tangent calls since setup (nrhs = 1 or G = 1: one per
                           right-hand side) */
    long rounds_total;  /* looks at the residual = read-backs of the sweep loop: per group 1 + the largest sweep count among its right-hand
                           sides (code 3: unspecified) */
    long scratch_bytes; /* device memory of the group's vectors; 0 until a call with nrhs > 1 on a G > 1 workspace */
} QPDOAmdGroupStats;
int  qpdo_amd_rhs_group(const QPDOWorkspace *work);
int  qpdo_amd_get_group_stats(const QPDOWorkspace *work, QPDOAmdGroupStats *out);
int  qpdo_amd_spmv_group(QPDOWorkspace *work, int which, int nvec, unsigned live_mask, const double *v, double *y);

/* ---- one large QP row-partitioned over G GPUs (BASELINE.json configs[3]) --------------------------------
 * One process per GPU.  Every rank calls the normal API with the SAME full problem; the library keeps rows
 * [rank*ceil(m/G), ...) of A (and the matching slices of A' and, for the PCG operator, of Q) on its GPU and
 * replicates the vectors.  The exchange step is one sum all-reduce of an n-vector per A' / K product: RCCL on
 * the solver's stream (rccl_unique_id: 128 bytes created by rank 0 with qpdo_amd_dist_unique_id and sent to
 * the others by the caller), or - for tests on a single GPU - a host callback `fn` (e.g. gloo).
 * Applies to workspaces set up afterwards in this process; world = 1 switches it off.  All ranks obtain the
 * same status, counts and solution. */
typedef void (*qpdo_amd_allreduce_fn)(void *ctx, double *buf, long count, int op /* 0 sum, 1 max */);
int  qpdo_amd_dist_config(int rank, int world, const void *rccl_unique_id, qpdo_amd_allreduce_fn fn, void *ctx);
int  qpdo_amd_dist_unique_id(void *out128);

/* ---- batch of independent QPs (BASELINE.json configs[2]: MPC-sized problems, no collective) --------------
 * Default path (every item has n, m <= 1024 and passes the checks of qpdo_setup): ONE launch of the fused kernel
 * k_small_solve, one workgroup per item running the item's qpdo_setup (Ruiz scaling), qpdo_warm_start and the whole
 * qpdo_solve loop, including settings->max_time (QPDO_MAX_TIME_REACHED, checked at the end of every pass as in the
 * reference, src/qpdo.c:441-447) and the three PROFILING times of QPDOInfo (per item, from the device wall clock).
 * Otherwise, or with QPDO_BATCH=threads: every item goes through the entry points above on `nthreads` host threads, each
 * with its own workspace and HIP stream on the device of this process (QPDO_DEVICE).  Across GPUs the caller shards
 * the item list over processes (item b -> GPU b mod G; qpdo_amd/solver.py shard_indices).  x (n) and y (m) receive the
 * solution (NaN for infeasible statuses, as the reference's mex gateway does), info the final QPDOInfo. */
typedef struct {
    const QPDOData *data;       /* problem (caller-owned, read only)                     */
    const c_float  *x0, *y0;    /* optional warm start (NULL: cold)                      */
    c_float        *x, *y;      /* out: solution, caller-allocated, length n / m         */
    QPDOInfo        info;       /* out                                                    */
} QPDOAmdBatchItem;
/* returns the number of items whose setup failed (their info.status_val is QPDO_ERROR) */
long qpdo_amd_solve_batch(long count, QPDOAmdBatchItem *items, const QPDOSettings *settings, int nthreads);
/* HIP-event duration of the fused kernel launch of the last qpdo_amd_solve_batch on this process (0 if it took the threaded path) */
double qpdo_amd_batch_kernel_seconds(void);

/* ---- where the fused kernel keeps the Newton matrix K = Q + sigma I + A'DA (batches, batch streams, fleets) ------------------------------
 * One layout per LAUNCH, decided from all its items:
 *   PACKED  the packed lower triangle of the largest item, n (n+1) / 2 doubles, fits the workgroup's LDS beside the rest (n up to about
 *           170-200, depending on m): K lives there.  This decision comes first and is what it was before the band layout existed.
 *   BAND    otherwise, when for EVERY item the lower band of K, n_i (b_i + 1) doubles (element (i, j), j <= i <= j + b, at
 *           j (b+1) + (i - j)), fits the same region beside the fixed part sized for the largest n and m of the launch: every item's K
 *           lives in LDS in band storage, and the factorization and both triangular solves touch the band alone.  b_i, the item's
 *           half-bandwidth, is the largest |i - j| over the stored entries of Q and the largest column span (last - first column) over
 *           the rows of A: a function of the pattern, so scaling, qpdo_update_q and qpdo_amd_fleet_update_matrices never change it.  A
 *           dense item in such a launch is b = n - 1; an item with m = 0 takes Q's bandwidth.  b_i <= 128: an item with a wider band sends the
 *           launch to GLOBAL (the widest band measured, b = 70, wins; nothing wider was measured).  The work vectors of a fleet,
 *           and of a batch that takes the latency kernel, go to LDS as well where they fit behind the band image; the band
 *           factorization has no look-ahead, so such a launch keeps one set of column buffers.
 *   GLOBAL  otherwise: K is a full n x n square in global memory (everything up to n = m = 1024).
 * QPDO_SMALL_BAND=0 in the environment keeps K out of the band layout (PACKED or GLOBAL as before); it is read at every launch and query.
 * CONTRACT: an item solved in the band layout returns what it returns through the global-memory layout, and what the CPU oracle returns --
 * status, iteration counts, x, y, objective, residual norms, certificates, the per-pass trace -- bit for bit, with one exception: natural-
 * order LDL' of a band matrix creates no fill outside the band, and the operations the band code leaves out are subtractions of an exact
 * zero product; such a subtraction can turn a -0.0 into +0.0 (a right-hand-side component that is exactly -0.0: -0.0 - (-0.0) = +0.0), so a
 * zero may come back with the other sign.  No nonzero value can differ.
 * qpdo_amd_small_factor_layout: the layout a launch over these items takes -- the launches go through the same function -- as pure host
 * arithmetic, no device needed.  kind 0: qpdo_amd_solve_batch, 1: a batch of a stream, 2: a fleet.  half_bandwidth: optional out, `count`
 * entries.  settings may be NULL (no setting enters the rule).  -1: an item does not fit the fused kernel (or count < 1, an unknown kind). */
#define QPDO_AMD_SMALL_K_GLOBAL 0
#define QPDO_AMD_SMALL_K_PACKED 1
#define QPDO_AMD_SMALL_K_BAND   2
int qpdo_amd_small_factor_layout(long count, const QPDOData *const *data, const QPDOSettings *settings, int kind, long *half_bandwidth);
/* the last qpdo_amd_solve_batch of this process, as qpdo_amd_batch_kernel_seconds (-1: none yet through the fused kernel) */
int qpdo_amd_batch_factor_layout(void);

/* ---- STREAMED batches (BASELINE.json configs[2]: "batch of 4096 MPC-sized QPs ... streamed") ----------------------------
 * A fused-kernel launch is as slow as its slowest item: an instance that never reaches eps_abs (in the reference either)
 * holds one workgroup for max_iter passes while the other CUs idle.  A batch stream keeps up to `depth` batches in flight,
 * each on its own HIP stream with its own device arena and pinned staging: submit packs, uploads and launches batch i+1 and
 * returns; its workgroups fill the CUs that the stragglers of batch i do not occupy.  Per item the arithmetic is that of
 * qpdo_amd_solve_batch (same kernel): results do not depend on what else is in flight.
 * submit: ticket >= 0, or -1 (invalid settings / data, an item that does not fit the fused kernel -- use
 * qpdo_amd_solve_batch for those --, no free slot: wait for the oldest ticket first).  The items and everything they point
 * to must stay valid and untouched until wait(ticket) has returned; wait fills x, y and info of every item and returns 0
 * (-1: device error or unknown ticket), optionally the HIP-event duration of that batch's kernel. */
typedef struct QPDOAmdBatchStream_ QPDOAmdBatchStream;
QPDOAmdBatchStream *qpdo_amd_batch_stream_create(int depth);
long qpdo_amd_batch_stream_submit(QPDOAmdBatchStream *stream, long count, QPDOAmdBatchItem *items, const QPDOSettings *settings);
int  qpdo_amd_batch_stream_wait(QPDOAmdBatchStream *stream, long ticket, double *kernel_seconds);
void qpdo_amd_batch_stream_destroy(QPDOAmdBatchStream *stream);

/* ---- a resident FLEET of small QPs (closed-loop MPC: every control step changes q and the bounds; with the flag below also Q / A values) ----
 * A fleet is `count` small QPs set up ONCE and kept on the device.  Item i behaves bit for bit as a workspace of its own that
 * received qpdo_setup(data[i], settings), then -- in the order the fleet calls were made -- qpdo_update_bounds for every fleet
 * update that passed an l or u entry for it, qpdo_update_q for every fleet update that passed a q entry, qpdo_warm_start for every
 * fleet warm start and qpdo_solve for every fleet solve, the reference's quirks included: a solve clears `initialized`, so a solve
 * that no warm start precedes starts from zero (src/qpdo.c:312-314); qpdo_update_q recomputes the cost scaling c from the current x
 * and Qx -- whatever the last solve or warm start left -- and rescales Q and Qx by c / c_old (src/qpdo.c:552-580); a solve that
 * runs out of passes overwrites an UNSOLVED status only (src/qpdo.c:451-453).
 * create   copies everything it needs (the caller's data may be freed afterwards), makes the only matrix upload the fleet ever
 *          makes and scales every item on the device in one launch.  Every item must fit the fused kernel (n, m <= 1024 and the
 *          matrix checks of qpdo_setup) and have l <= u; otherwise NULL with qpdo_amd_last_error() set and nothing left allocated.
 *          The settings are FIXED at create: there is no qpdo_update_settings for a fleet.  Matrix VALUES can change in a fleet
 *          created with QPDO_AMD_FLEET_MATRIX_UPDATES only (below).
 * update   q, l, u: arrays of `count` pointers (q[i]: n_i values, l[i] / u[i]: m_i).  A NULL array leaves that kind of data unchanged
 *          for all items, a NULL entry for that item.  Within one call the bounds are applied first, then q (the two commute in the
 *          reference: bounds touch l, u and the row scaling E only).  An item whose l[i] and u[i] are both passed with l > u somewhere
 *          makes the call fail before anything is written (the reference sets QPDO_ERROR on that workspace instead).
 * warm_start       x0, y0 as for update; an item with a NULL entry (or array) starts that vector from zero, as qpdo_warm_start(work, NULL, ..).
 * warm_start_last  in bits warm_start with the unscaled x and y the last solve returned for each item, taken from the device copy (no
 *          host traffic); an item whose status after the last solve is -3, -4, -10 (never solved) or -99 is warm-started from zero.
 * solve    ONE kernel launch for the whole fleet; uploads nothing.  Fills info[i] and, where x / y and their entries are non-NULL, the
 *          solution (NaN for infeasible statuses, as the batch call does); returns when the results are on the host.
 * Every call returns 0, or nonzero with qpdo_amd_last_error() set and the fleet as it was (checks precede every write).
 * One thread at a time per fleet; different fleets are independent.  Not for row-partitioned setups; one fleet lives on one GPU
 * (QPDO_DEVICE) -- the caller shards items over processes as for batches.
 * Stats: vector_bytes_uploaded_last_call of an update or warm start = 8 bytes per vector element passed + a fixed table of
 * QPDO_AMD_FLEET_TABLE_BYTES per item (the offsets of the item's vectors in the upload); 0 after warm_start_last. */
#define QPDO_AMD_FLEET_TABLE_BYTES 16
/* ---- new Q / A VALUES for fleet items (real-time-iteration NMPC, LTV models: the pattern stays, the values move) ---------------------
 * qpdo_amd_fleet_create equals qpdo_amd_fleet_create_ex(.., 0): the arena, uploads, launches and bits of a fleet that cannot change its
 * matrices.  flags = QPDO_AMD_FLEET_MATRIX_UPDATES additionally keeps, per item: two int32 maps (one per entry of A, one per entry of the
 * full Q unless stype is 0) that ride in create's upload (matrix_bytes_uploaded includes them); device copies of the unscaled q, l, u
 * (fleet updates keep them current); with scaling > 0 device copies of the unscaled values of A and of the full Q (scaling rounds, and
 * qpdo_update_q rescales Q: neither can be undone bit for bit); host copies of the two CSC patterns; pinned and device staging for every
 * stored entry of every Q and A.  resident_extra_bytes is the device total.  Unknown flag bits are refused before any device call.
 * update_matrices  Q, A: arrays of `count` pointers to matrices in the item's create-time pattern (Q in its create-time stype storage).  A
 *          NULL array leaves that matrix unchanged for all items, a NULL entry for that item; both arrays NULL: returns 0, nothing is
 *          launched.  An item with neither entry is not touched: its state, status and a pending warm start are kept.  An item with an
 *          entry is afterwards, bit for bit, what qpdo_setup leaves for the new matrix or matrices, the latest values of the one not
 *          passed, the latest UNSCALED q, l, u (create and every fleet update since), c and the fleet's settings: scaling from scratch,
 *          state zero, sigma = sigma_init, status QPDO_UNSOLVED (so "out of passes overwrites UNSOLVED only" starts afresh), no pending
 *          warm start.  The outputs of its last solve stay readable, and warm_start_last is then qpdo_warm_start with the x, y that
 *          solve returned if it returned finite ones (the status it left none of -3, -4, -10, -99), from zero otherwise: the
 *          real-time-iteration step  update_matrices -> update(q, l, u) -> warm_start_last -> solve  without host traffic for x, y.
 *          Checks (all on the host, before any write or upload; the call is all-or-nothing): the fleet has the flag; per passed matrix
 *          nrow, ncol, stype (Q), the entry count, EVERY column pointer and row index equal the create-time pattern (either itype), x is
 *          not NULL.  The message names the item and the reason.
 *          Cost: 8 bytes per passed entry + QPDO_AMD_FLEET_MATRIX_TABLE_BYTES per item in ONE upload, ONE launch (one workgroup per
 *          item: a gather per CSR image, then the item's setup -- the Ruiz iterations dominate), one stream sync.
 * solve_launches and solves of QPDOAmdFleetStats are not moved by matrix calls; matrix_bytes_uploaded stays what create uploaded. */
#define QPDO_AMD_FLEET_MATRIX_UPDATES 1L
#define QPDO_AMD_FLEET_MATRIX_TABLE_BYTES 8
typedef struct QPDOAmdFleet_ QPDOAmdFleet;
typedef struct {
    long count;
    long matrix_bytes_uploaded;             /* by create; never grows afterwards */
    long vector_bytes_uploaded_last_call;   /* by the last update / warm_start / warm_start_last */
    long solve_launches;                    /* kernel launches made by solve calls ... */
    long solves;                            /* ... and the solve calls themselves */
    double last_kernel_seconds;             /* HIP-event duration of the last solve's launch */
} QPDOAmdFleetStats;
typedef struct {
    long calls;                             /* update_matrices calls that launched */
    long items_last_call;                   /* items that had a Q or an A entry in the last such call */
    long value_bytes_uploaded_last_call;    /* 8 per entry passed + QPDO_AMD_FLEET_MATRIX_TABLE_BYTES per item of the fleet */
    long resident_extra_bytes;              /* device memory the flag costs (maps, unscaled copies, staging); 0 without it */
    double last_kernel_seconds;             /* HIP-event duration of the last update_matrices launch */
} QPDOAmdFleetMatrixStats;
QPDOAmdFleet *qpdo_amd_fleet_create(long count, const QPDOData *const *data, const QPDOSettings *settings);
QPDOAmdFleet *qpdo_amd_fleet_create_ex(long count, const QPDOData *const *data, const QPDOSettings *settings, long flags);
int  qpdo_amd_fleet_update_matrices(QPDOAmdFleet *f, const cholmod_sparse *const *Q, const cholmod_sparse *const *A);
int  qpdo_amd_fleet_get_matrix_stats(const QPDOAmdFleet *f, QPDOAmdFleetMatrixStats *out);
int  qpdo_amd_fleet_update(QPDOAmdFleet *f, const c_float *const *q, const c_float *const *l, const c_float *const *u);
int  qpdo_amd_fleet_warm_start(QPDOAmdFleet *f, const c_float *const *x0, const c_float *const *y0);
int  qpdo_amd_fleet_warm_start_last(QPDOAmdFleet *f);
int  qpdo_amd_fleet_solve(QPDOAmdFleet *f, c_float *const *x, c_float *const *y, QPDOInfo *info);
int  qpdo_amd_fleet_get_stats(const QPDOAmdFleet *f, QPDOAmdFleetStats *out);
/* what this fleet's launches use (QPDO_AMD_SMALL_K_*; fixed at create: new matrix values keep the pattern, hence the band); -1: NULL fleet.
 * update, update_matrices, warm_start and warm_start_last behave on a band fleet as on any other */
int  qpdo_amd_fleet_factor_layout(const QPDOAmdFleet *f);
/* the infeasibility certificates of `item` from the last solve: prim_inf_cert (m values, meaningful at status -3), dual_inf_cert (n, at -4);
 * either may be NULL */
int  qpdo_amd_fleet_get_certificates(const QPDOAmdFleet *f, long item, c_float *prim_inf_cert, c_float *dual_inf_cert);
/* ---- DEVICE-RESIDENT inputs and outputs on the CALLER'S STREAM (batched simulators, learned-model MPC, sampling planners: q, l, u are
 * computed on the GPU and x is consumed there) ------------------------------------------------------------------------------------------
 * The calls above take host pointers and return when the device is done.  The *_dev calls below take DEVICE arrays, enqueue on the stream
 * the caller names (`void *stream`: a hipStream_t; NULL is the null stream) and return at once: no stream synchronisation, no copy to or
 * from the host, no spinning on pinned memory.  Per item they are the host calls bit for bit: an item updated, warm-started or solved from
 * device memory is the item the host call with the same values leaves.  The kernels that do the work are the host calls' own; two small
 * ones (one workgroup per item) move the vectors between the caller's arrays and the fleet's staging / outputs.
 * PACKED LAYOUT  The n-vectors of all items live back to back in ONE array of N = sum n_i doubles, item i at noff[i]; the m-vectors in
 *          one array of M = sum m_i doubles, item i at moff[i] (a uniform fleet: (count, n) and (count, m) row-major tensors).
 *          qpdo_amd_fleet_packed_layout fills count + 1 entries each, the last one the total, as pure host arithmetic (no device needed);
 *          qpdo_amd_fleet_get_packed_layout does the same for an existing fleet.  n_len / m_len of every call must equal N / M.
 * Arrays   every array is a device (or managed) pointer on the fleet's device.  NULL: not passed (update, warm start) / not wanted (solve).
 * item_mask  optional, `count` int32 on the device.  update: bit 0 / 1 / 2 = the item takes q / l / u from the arrays passed, a clear bit
 *          leaves that vector unchanged.  warm start: bit 0 / 1 = x0 / y0 are taken, a clear bit starts that vector from zero (a NULL
 *          entry of the host call).  NULL mask: every item takes every array passed.
 * update_dev       no q, l and u at all: returns 0 and launches nothing.  l <= u CANNOT be checked on the host here -- the data is on the
 *          device -- and so, UNLIKE THE ALL-OR-NOTHING HOST CALL, the check is made on the device PER ITEM: an item that takes both l
 *          and u with l > u somewhere is not touched at all by that call, its q included; it is counted, and the smallest such item
 *          index since the last qpdo_amd_fleet_sync is kept; all other items proceed.
 * warm_start_dev   neither x0 nor y0: every item starts from zero, as qpdo_amd_fleet_warm_start(f, NULL, NULL).
 * warm_start_last_dev  qpdo_amd_fleet_warm_start_last on the caller's stream.
 * solve_dev        ONE solve launch, then the results into the arrays wanted: x (N), y (M) -- NaN for items whose status is -3 or -4, as
 *          qpdo_amd_fleet_solve returns them --; status, count x 3 int64: status_val, iterations, oterations; norms, count x 5 doubles:
 *          res_prim_norm, res_dual_norm, res_prim_in_norm, res_dual_in_norm, objective; prim_inf_cert (M) / dual_inf_cert (N): NaN except
 *          the item's certificate at status -3 / -4.  With no array wanted the solve still runs (fetch_last delivers it).
 * Checks   all on the host, before any launch; a refused call returns nonzero with qpdo_amd_last_error() set and has launched nothing:
 *          NULL fleet; n_len != N or m_len != M; a passed pointer that hipPointerGetAttributes does not report as device or managed
 *          memory of the fleet's device (the message names the argument).  The extent of an array cannot be checked: it is the caller's.
 * ORDER    One event orders all streams a fleet is driven on, its own included: EVERY fleet call, host or device, first makes its stream
 *          wait for the event the previous fleet call recorded and records it again behind its last operation.  Host and device calls
 *          may therefore be mixed freely, and the caller may change streams between calls.  What the caller must order itself is its own
 *          arrays: they are read / written on the stream passed, so produce inputs and consume outputs on that stream (or behind an event
 *          of it), and keep them alive and unchanged until the call's work is done.  Still one thread at a time per fleet.  hipGraph
 *          capture of these calls is not supported.
 * fetch_last  (HOST pointers, as qpdo_amd_fleet_solve) waits for the event, downloads the descriptors and outputs of the last solve,
 *          whichever kind of call launched it, and delivers exactly what qpdo_amd_fleet_solve would have delivered, launching nothing.
 *          After a solve_dev, qpdo_amd_fleet_get_certificates is refused ("no solve yet") until a fetch_last has made the host image current.
 * sync     waits for that event, i.e. for everything the fleet was asked to do; fills the counters (out may be NULL), refreshes
 *          last_kernel_seconds of QPDOAmdFleetStats from the last solve_dev, and resets the refusal record.
 * Stats    solve_launches and solves grow by 1 per solve_dev; vector_bytes_uploaded_last_call is 0 after update_dev / warm_start_dev.
 * ---- new Q / A VALUES from device arrays (a fleet created with QPDO_AMD_FLEET_MATRIX_UPDATES): the first call of the real-time-iteration
 * step  update_matrices_dev -> update_dev(q, l, u) -> warm_start_last_dev -> solve_dev, which then runs on the caller's stream from end to
 * end without a host wait.  The pattern is fixed at create, so the call carries VALUES ONLY and compares no pattern.
 * CONTRACT  After the call every item that took a matrix is, bit for bit, what qpdo_amd_fleet_update_matrices leaves when given the same
 *          values for the same items: what qpdo_setup leaves for the new matrix or matrices, the latest values of the one not taken, the
 *          latest unscaled q, l, u, c and the fleet's settings; status QPDO_UNSOLVED, no pending warm start, and warm_start_last(_dev) still
 *          starts from the x, y of the previous solve.  An item that takes neither matrix is not touched (state, status, pending warm start).
 * PACKED VALUE LAYOUT  The stored values of all items' Q live back to back in ONE array of NQ = sum nnzQ_i doubles, item i at qoff[i], in
 *          the order of data[i]->Q->x at create (the caller's stored triangle for stype +-1, the full matrix for stype 0); the CSC values of
 *          all items' A in one array of NA = sum nnzA_i doubles, item i at aoff[i], in the order of data[i]->A->x.  An item with m = 0, or with
 *          a Q that stores no entry, occupies nothing.  qpdo_amd_fleet_packed_matrix_layout fills count + 1 entries each, the last one the
 *          total, as pure host arithmetic (either itype, no device needed); qpdo_amd_fleet_get_packed_matrix_layout does the same for an
 *          existing fleet and is refused for one created without the flag.  q_len / a_len must equal NQ / NA.
 * update_matrices_dev  Qx (NQ) / Ax (NA): device (or managed) arrays on the fleet's device; NULL: that matrix is unchanged for all items; both
 *          NULL: returns 0 and launches nothing.  item_mask: optional, `count` int32 on the device, bit 0 = the item takes Q from Qx, bit 1 = A
 *          from Ax; a clear bit (or a NULL array) leaves that matrix unchanged for the item; NULL mask: every item takes every array passed.
 *          Checks, all on the host before any launch (a refused call has launched nothing): NULL fleet; a fleet without the flag; q_len != NQ
 *          or a_len != NA (the message names both numbers); a passed pointer that is not device or managed memory of the fleet's device (the
 *          message names Qx, Ax or item_mask).  The values themselves are not examined, as in the host call.
 *          Cost: no upload, no host copy, no stream synchronisation, no event timing.  TWO launches on `stream`: one workgroup per item
 *          copies the values taken into the fleet's matrix staging (8 bytes read and written per entry taken) and writes the item's table
 *          entry, then the host call's own kernel runs unchanged.  A table of 2 (count + 1) int32 offsets is uploaded once, at create.
 *          ORDER is that of the other device calls (above); hipGraph capture stays unsupported.
 * Stats    QPDOAmdFleetMatrixStats after a device call that launched: calls + 1; value_bytes_uploaded_last_call 0; items_last_call -1 (which
 *          items took a matrix is known on the device only); last_kernel_seconds keeps the last HOST call's figure.  resident_extra_bytes
 *          includes the offset table.  solve_launches and solves of QPDOAmdFleetStats do not move. */
typedef struct {
    long update_calls, warm_start_calls, solve_calls;   /* device calls that launched, since create (warm_start_last_dev counts as a warm start) */
    long refused_items;                     /* items refused by update_dev calls (l > u) since the last sync ... */
    long first_refused_item;                /* ... and the smallest such item index; -1: none */
} QPDOAmdFleetDevStats;
/* the HIP device ordinal the fleet lives on (every array of a device call must be memory of this device); -1: NULL fleet */
int  qpdo_amd_fleet_device(const QPDOAmdFleet *f);
int  qpdo_amd_fleet_packed_layout(long count, const QPDOData *const *data, long *noff, long *moff);
int  qpdo_amd_fleet_get_packed_layout(const QPDOAmdFleet *f, long *noff, long *moff);
int  qpdo_amd_fleet_update_dev(QPDOAmdFleet *f, const double *q, const double *l, const double *u, const int *item_mask, long n_len, long m_len, void *stream);
int  qpdo_amd_fleet_warm_start_dev(QPDOAmdFleet *f, const double *x0, const double *y0, const int *item_mask, long n_len, long m_len, void *stream);
int  qpdo_amd_fleet_warm_start_last_dev(QPDOAmdFleet *f, void *stream);
int  qpdo_amd_fleet_solve_dev(QPDOAmdFleet *f, double *x, double *y, long *status, double *norms, double *prim_inf_cert, double *dual_inf_cert, long n_len, long m_len,
                              void *stream);
int  qpdo_amd_fleet_packed_matrix_layout(long count, const QPDOData *const *data, long *qoff, long *aoff);
int  qpdo_amd_fleet_get_packed_matrix_layout(const QPDOAmdFleet *f, long *qoff, long *aoff);
int  qpdo_amd_fleet_update_matrices_dev(QPDOAmdFleet *f, const double *Qx, const double *Ax, const int *item_mask, long q_len, long a_len, void *stream);
int  qpdo_amd_fleet_fetch_last(QPDOAmdFleet *f, c_float *const *x, c_float *const *y, QPDOInfo *info);
int  qpdo_amd_fleet_sync(QPDOAmdFleet *f, QPDOAmdFleetDevStats *out);
/* ---- the ADJOINT of the last solve (learned-model MPC: a loss gradient goes back through the QP to whatever produced q, l, u, Q, A) --------
 * Item: min 1/2 x'Qx + q'x s.t. l <= Ax <= u, solved to the x, y solve(_dev) delivered.  All quantities below are the caller's UNSCALED ones.
 * ACTIVE SET  t = Ax + y.  Row i is upper-active (flag +1) if t_i >= u_i, else lower-active (-1) if t_i <= l_i, else inactive (0): the
 *          projection of the outer residual (termination.c).  A row with l_i = u_i is always active; a bound of magnitude >= 1e20 is never
 *          reached.  The rule is evaluated in the item's scaled space, so a row within rounding of a bound may fall either way: the call
 *          DELIVERS its flags (`active`), and everything else is defined by them.  S: the flagged rows, k = |S|.
 * SYSTEM   Given gx = dL/dx (N) and gy = dL/dy (M, or NULL = zero; entries of inactive rows are ignored and may hold anything, NaN included):
 *              [ Q    A_S' ] [vx]   [ gx   ]
 *              [ A_S  0    ] [vy] = [ gy_S ]
 *          dq = -vx;  du_i = vy_i on +1 rows, dl_i = vy_i on -1 rows, every other entry of dl, du an exact +0.0;  for a stored entry (i, j) of
 *          A: -(y_i vx_j + vy_i x_j) on a flagged row, else +0.0;  for a stored entry (a, b) of Q: -vx_a x_b (stype 0), -(vx_a x_b + vx_b x_a)
 *          (off-diagonal, stype +-1), -vx_a x_a (diagonal); a stored entry in the triangle that stype +-1 ignores gets +0.0.  dQx (NQ) /
 *          dAx (NA) are in the packed value layout of
 *          qpdo_amd_fleet_get_packed_matrix_layout and are evaluated from the very dq, dl, du delivered and the x, y of the solve.
 * METHOD   One launch (k_small_fleet_adjoint), one workgroup per item, in the solve's own launch shape.  In the item's scaled space, block
 *          elimination on the regularised matrix: K = Qs + sigma I + As_S' W As_S is assembled and factored by the solve loop's own device
 *          functions (all three layouts of K), and  K dvx = rx + As_S' W ry,  dvy = W (As_S dvx - ry)  is repeated on the residual of the
 *          TRUE system (no sigma, no W^-1): the proximal method of multipliers on an equality QP, which converges for PSD Q and a consistent
 *          system.  sigma = 1e-10 s, W_i = 1e10 s / ||row i of As||^2 with s the largest |diagonal entry| of Qs (1 when there is none).
 * ACCEPTANCE  max(||Q vx + A_S' vy - gx||_inf, ||A_S vx - gy_S||_inf) <= tol * max(||gx||_inf, ||gy_S||_inf), on the true residual in unscaled terms,
 *          looked at before every sweep; at most max_sweeps sweeps.  A residual that is not finite is never accepted.
 * adj_status  count x 3 int64: code, sweeps, k.  code 0: accepted.  1: the residual did not reach tol in max_sweeps sweeps -- the system is
 *          inconsistent (dependent active rows with gy_S outside their range), singular, or so ill-conditioned that the sweeps contract
 *          too slowly; the code says that no gradient is delivered, not which of these it was (more sweeps settle the last case).  2: the item's status is not QPDO_SOLVED --
 *          never solved, infeasible, out of passes, or matrices replaced since its last solve.  3: a pivot of K that is not a positive
 *          finite number.  An item with code != 0 gets NaN in all its slices of dq, dl, du, dQx, dAx and 0 flags; adj_res (count): the
 *          accepted relative residual, NaN otherwise.  An item with m = 0 solves Q vx = gx.
 * FLAG     create_ex with QPDO_AMD_FLEET_ADJOINT (combinable with QPDO_AMD_FLEET_MATRIX_UPDATES); a fleet without it is what it was and is
 *          refused here.  The launch works in the solve's work-vector area and K buffer and reads the packed layouts the *_dev calls already
 *          keep, so the flag reserves no memory of its own: QPDOAmdFleetAdjointStats.resident_extra_bytes reports 0.  The call writes none
 *          of the item's state, of the last solve's outputs, of the matrices, q, l, u: every later solve carries the bits it would have had.
 * Checks   all on the host before the launch; a refused call returns nonzero with qpdo_amd_last_error() set and has launched nothing: NULL
 *          fleet; a fleet without the flag; n_len != N or m_len != M; dQx or dAx on a fleet without QPDO_AMD_FLEET_MATRIX_UPDATES, q_len != NQ
 *          with dQx or a_len != NA with dAx (both numbers named); NULL gx, dq, dl or du; a passed pointer that is not device or managed
 *          memory of the fleet's device (named); tol not a positive finite number; max_sweeps < 1; THE MOST RECENT STATE-CHANGING FLEET CALL
 *          WAS NOT A SOLVE -- an update, warm start or matrix update since the last solve(_dev) means the resident q, l, u or matrices are no
 *          longer those of the x, y returned.  adjoint_dev, fetch_last, sync and the getters do not count: several adjoint calls may follow
 *          one solve (the rows of a Jacobian).  Where several faults coincide the first in this order is reported, for adjoint_dev and
 *          adjoint_multi_dev alike: the flag, (nrhs,) the lengths, the matrix flag and q_len / a_len, tol, max_sweeps, the NULL pointers,
 *          "was not a solve", the pointers that are not device memory.
 * ORDER    that of the other device calls: enqueues on `stream`, returns at once, joins the fleet's one-event chain.  No hipGraph capture.
 * Stats    adjoint_calls of QPDOAmdFleetAdjointStats counts the calls that launched (QPDOAmdFleetDevStats keeps its five members: its size
 *          is part of the ABI); solve_launches, solves and the device-call counters do not move. */
#define QPDO_AMD_FLEET_ADJOINT 8L
typedef struct {
    long adjoint_calls;                     /* adjoint_dev calls that launched, since create */
    long resident_extra_bytes;              /* device memory the flag holds beyond a fleet without it: 0 */
} QPDOAmdFleetAdjointStats;
int  qpdo_amd_fleet_adjoint_dev(QPDOAmdFleet *f, const double *gx /* N */, const double *gy /* M or NULL */, double *dq /* N */, double *dl /* M */, double *du /* M */,
                                double *dQx /* NQ or NULL */, double *dAx /* NA or NULL */, int *active /* M int32 or NULL */,
                                long *adj_status /* count x 3: code, sweeps, k; or NULL */, double *adj_res /* count; or NULL */, double tol, long max_sweeps,
                                long n_len, long m_len, long q_len, long a_len, void *stream);
int  qpdo_amd_fleet_get_adjoint_stats(const QPDOAmdFleet *f, QPDOAmdFleetAdjointStats *out);
/* ---- MANY RIGHT-HAND SIDES PER FACTORIZATION: the rows of a Jacobian (adjoint_multi_dev) and the TANGENT of the last solve (tangent_dev) ----
 * Both solve the adjoint's system -- the KKT matrix of the active set is symmetric -- on a fleet created with QPDO_AMD_FLEET_ADJOINT (the
 * matrix arrays dQx, dAx, tQx, tAx also need QPDO_AMD_FLEET_MATRIX_UPDATES); there is no flag of their own.  One launch (k_small_fleet_sens),
 * one workgroup per item, in the solve's own launch shape.  Per item, ONCE: the status gate, the classification of the rows, W and sigma,
 * the assembly of K, its factorization (all three layouts of K) and the pivot check, exactly as in adjoint_dev.  Then the nrhs right-hand
 * sides follow, each by the adjoint call's sweeps, sigma, W and acceptance rule, every right-hand side's operations in the single call's order.
 * LAYOUT   right-hand-side major: right-hand side r of an array whose per-RHS length is L (N, M, NQ or NA) starts at r * L, and every such
 *          slab is one of the packed arrays the other device calls take.  n_len, m_len, q_len, a_len stay N, M, NQ, NA.  `active` (M) is ONE
 *          array: the flags depend on the solve, not on the right-hand side; an item with code 2 or 3 gets 0 flags, every other item its
 *          flags whatever the codes of its right-hand sides.  status[r][item] (nrhs x count x 3 int64) is the triple (code, sweeps, k) of
 *          the single call with the same codes 0 .. 3; codes 2 and 3 are the item's and repeat for every r, code 1 is one right-hand
 *          side's own and touches no other right-hand side of the item.  res[r][item] (nrhs x count) as adj_res.
 * ADJOINT  qpdo_amd_fleet_adjoint_multi_dev: slab r of dq, dl, du, dQx, dAx, status and res carries THE BITS qpdo_amd_fleet_adjoint_dev delivers
 *          for slab r of gx / gy after the same solve (NaN slices included), in all three layouts of K, with and without scaling.
 * TANGENT  qpdo_amd_fleet_tangent_dev: the first-order change (dx, dy) of the solution for a change (tq, tl, tu, tQ, tA) of the item's data at
 *          a fixed active set -- the advanced-step / sensitivity update of an MPC controller: x + dx for the measured state from one
 *          factorization and a few triangular solves instead of a re-solve.  All quantities are the caller's UNSCALED ones; S and the flags as
 *          for the adjoint; b = u on +1 rows and l on -1 rows:
 *              [ Q    A_S' ] [dx  ]   [ -(tq + tQ x + tA_S' y_S) ]
 *              [ A_S  0    ] [dy_S] = [  tb_S - tA_S x           ]
 *          dy_i is an exact +0.0 off S.  A NULL array is a zero perturbation (all five NULL: refused).  Entries of tl, tu, tAx on rows that do
 *          not use them (tl on a row that is not -1, tu on a row that is not +1, tAx on an unflagged row) are ignored and may hold NaN.  tQ
 *          acts as the symmetric matrix its stored entries stand for: under stype +-1 an off-diagonal stored entry (a, b) contributes to
 *          rows a and b and an entry in the ignored triangle contributes nothing; under stype 0 the caller passes a SYMMETRIC perturbation
 *          (as the solver reads a stype-0 Q as symmetric) and row a is evaluated from the stored entries of COLUMN a.  The right-hand side
 *          is formed in fp64 on the device from the x, y the solve returned, one thread per row in ascending stored order
 *          (rx_j: tq_j, then the entries of row j of tQ, then those of column j of tA in the caller's CSC order; ry_i: the entries of
 *          row i of tA in column order, subtracted from tb_i), taken into the item's scaled space as the adjoint takes gx, gy, and solved
 *          by the same sweeps.  ACCEPTANCE on the true unscaled residual against tol * max(||rx||_inf, ||ry_S||_inf); a non-finite entry
 *          among those used is never accepted (code 1); a zero right-hand side is accepted at sweep 0 with zeros.
 * DUALITY  with (vx, vy) = (-dq, dl + du) of the adjoint for (gx, gy) and (dx, dy) of the tangent, in exact arithmetic
 *              <gx, dx> + <gy_S, dy_S> = <dq, tq> + <dl, tl> + <du, tu> + <dQx, tQx> + <dAx, tAx>.
 * Checks   the adjoint call's, on the host before the launch (a refused call has launched nothing), and: nrhs < 1; nrhs > 2147483647 (the
 *          kernel counts right-hand sides in 32 bits; the offsets r * N, r * M, r * NQ, r * NA are formed in 64 bits and have no limit of
 *          their own); NULL dx or dy; "no tangent passed".  THE MOST RECENT STATE-CHANGING FLEET CALL WAS NOT A SOLVE applies unchanged;
 *          neither call is state-changing: any mix of adjoint_dev, adjoint_multi_dev and tangent_dev calls may follow one solve.
 * ORDER    that of the other device calls: enqueues on `stream`, returns at once, joins the fleet's one-event chain.  No hipGraph capture.
 * GROUPS   qpdo_amd_fleet_rhs_group: the right-hand sides one workgroup carries AT ONCE on this fleet; -1: NULL fleet.  G = 8 where K is
 *          PACKED in LDS (one right-hand side per wave of the workgroup: wave w runs the triangular solves of right-hand side w, the
 *          products and element loops run over (right-hand side, row) pairs, a right-hand side leaves the sweeps at its own sweep count);
 *          a last, partial group and nrhs < G work; a call with nrhs = 1 runs as G = 1.  G = 1 in the BAND and GLOBAL layouts: the
 *          right-hand sides follow one another in the solve's work-vector area.  Either way every right-hand side receives the single
 *          call's operations in its order.  QPDO_AMD_FLEET_RHS_GROUP=1..8 in the environment at create overrides G (a measuring switch).
 * MEMORY   G = 1 needs none.  G > 1 keeps the carried right-hand sides' vectors in a device scratch of G x (7 N + 5 M) doubles, allocated
 *          ONCE by the first call with nrhs > 1 -- a host allocation: THAT CALL MAY BLOCK until earlier device work has finished, as
 *          qpdo_amd_update_matrices says of its maps --, reported in scratch_bytes and freed by qpdo_amd_fleet_destroy.
 *          QPDOAmdFleetAdjointStats.resident_extra_bytes stays 0.
 * Stats    QPDOAmdFleetSensitivityStats counts the two calls that launched and their right-hand sides; adjoint_calls, solve_launches, solves and
 *          the device-call counters do not move. */
typedef struct {
    long calls;                             /* adjoint_multi_dev + tangent_dev calls that launched, since create */
    long rhs_total;                         /* right-hand sides of those calls */
    long scratch_bytes;                     /* device scratch allocated for carrying G > 1 right-hand sides at once; 0 until a call needs it */
} QPDOAmdFleetSensitivityStats;
int  qpdo_amd_fleet_adjoint_multi_dev(QPDOAmdFleet *f, long nrhs, const double *gx /* nrhs x N */, const double *gy /* nrhs x M or NULL */,
                                      double *dq /* nrhs x N */, double *dl /* nrhs x M */, double *du /* nrhs x M */,
                                      double *dQx /* nrhs x NQ or NULL */, double *dAx /* nrhs x NA or NULL */, int *active /* M int32 or NULL */,
                                      long *status /* nrhs x count x 3 or NULL */, double *res /* nrhs x count or NULL */, double tol, long max_sweeps,
                                      long n_len, long m_len, long q_len, long a_len, void *stream);
int  qpdo_amd_fleet_tangent_dev(QPDOAmdFleet *f, long nrhs, const double *tq /* nrhs x N or NULL */, const double *tl /* nrhs x M or NULL */,
                                const double *tu /* nrhs x M or NULL */, const double *tQx /* nrhs x NQ or NULL */, const double *tAx /* nrhs x NA or NULL */,
                                double *dx /* nrhs x N */, double *dy /* nrhs x M */, int *active /* M int32 or NULL */,
                                long *status /* nrhs x count x 3 or NULL */, double *res /* nrhs x count or NULL */, double tol, long max_sweeps,
                                long n_len, long m_len, long q_len, long a_len, void *stream);
int  qpdo_amd_fleet_rhs_group(const QPDOAmdFleet *f);
int  qpdo_amd_fleet_get_sensitivity_stats(const QPDOAmdFleet *f, QPDOAmdFleetSensitivityStats *out);
void qpdo_amd_fleet_destroy(QPDOAmdFleet *f);

#ifdef __cplusplus
}
#endif
#endif
