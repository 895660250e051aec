"""Python front end over the C-ABI of libqpdo_amd.so.

Plays the role of the reference's MATLAB handle class (interfaces/mex/qpdo.m) and mex gateway
(interfaces/mex/qpdo_mex.c): dimension checks, +-Inf -> +-1e20 clipping (qpdo.m:138-139,215-216),
settings merge with unknown-field rejection (qpdo.m:238-273), and the result marshalling rule of
qpdo_mex.c:247-279 (NaN solution for infeasible statuses, NaN certificates otherwise).

Every numerical call goes through the C entry points declared in include/qpdo.h; there is no
Python or CPU implementation behind this class.
"""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _build

QPDO_INFTY = 1e20
c_int = C.c_long
c_float = C.c_double
dp = C.POINTER(C.c_double)


class CholmodSparse(C.Structure):
    """Layout of cholmod_sparse (include/qpdo.h)."""
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t), ("p", C.c_void_p),
                ("i", C.c_void_p), ("nz", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p),
                ("stype", C.c_int), ("itype", C.c_int), ("xtype", C.c_int), ("dtype", C.c_int),
                ("sorted", C.c_int), ("packed", C.c_int)]


class QPDOSettings(C.Structure):
    _fields_ = [("max_time", c_float), ("max_iter", c_int), ("inner_max_iter", c_int), ("eps_abs", c_float),
                ("eps_abs_in", c_float), ("eps_prim_inf", c_float), ("eps_dual_inf", c_float), ("rho", c_float),
                ("theta", c_float), ("delta", c_float), ("mu_min", c_float), ("proximal", c_int),
                ("sigma_init", c_float), ("sigma_upd", c_float), ("sigma_min", c_float), ("scaling", c_int),
                ("verbose", c_int), ("print_interval", c_int), ("reset_newton_iter", c_int)]


class QPDOData(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("Q", C.POINTER(CholmodSparse)), ("A", C.POINTER(CholmodSparse)),
                ("q", dp), ("c", c_float), ("l", dp), ("u", dp)]


class QPDOInfo(C.Structure):
    _fields_ = [("iterations", c_int), ("oterations", c_int), ("status", C.c_char * 32), ("status_val", c_int),
                ("res_prim_norm", c_float), ("res_dual_norm", c_float), ("res_prim_in_norm", c_float),
                ("res_dual_in_norm", c_float), ("objective", c_float), ("setup_time", c_float),
                ("solve_time", c_float), ("run_time", c_float)]


class QPDOSolution(C.Structure):
    _fields_ = [("x", dp), ("y", dp)]


class QPDOScaling(C.Structure):
    _fields_ = [("D", dp), ("Dinv", dp), ("E", dp), ("Einv", dp), ("c", c_float), ("cinv", c_float)]


class QPDOWorkspace(C.Structure):
    """Member order of QPDOWorkspace in include/qpdo.h (= reference include/types.h:147-224)."""
    _fields_ = [
        ("data", C.POINTER(QPDOData)),
        ("x", dp), ("y", dp), ("Ax", dp), ("Qx", dp), ("Aty", dp), ("initialized", c_int),
        ("temp_m", dp), ("temp_n", dp), ("temp_2m", dp),
        ("mu", dp), ("sqrt_mu", dp), ("sqrt_mu_min", c_float), ("sqrt_delta", c_float), ("n_mu_changed", c_int),
        ("sigma", c_float), ("sigma_mined", c_int), ("norm_q", c_float),
        ("xbar", dp), ("ybar", dp), ("dx", dp), ("dy", dp), ("tau", c_float), ("Qdx", dp), ("Adx", dp), ("Atdy", dp),
        ("w", dp), ("z", dp), ("df", dp), ("res_prim", dp), ("res_dual", dp), ("res_prim_old", dp),
        ("res_prim_in", dp), ("res_dual_in", dp), ("linsys_rhs", dp),
        ("res_prim_norm_old", c_float), ("res_dual_norm_old", c_float),
        ("ls_eta", c_float), ("ls_beta", c_float), ("ls_delta", dp), ("ls_alpha", dp), ("ls_taus", C.c_void_p),
        ("ls_idx_L", C.c_void_p), ("ls_idx_P", C.c_void_p), ("ls_idx_J", C.c_void_p),
        ("eps_prim", c_float), ("eps_dual", c_float), ("eps_prim_in", c_float), ("eps_dual_in", c_float), ("eps_in", c_float),
        ("D_temp", dp), ("E_temp", dp),
        ("chol", C.c_void_p), ("settings", C.POINTER(QPDOSettings)), ("scaling", C.POINTER(QPDOScaling)),
        ("solution", C.POINTER(QPDOSolution)), ("info", C.POINTER(QPDOInfo)), ("timer", C.c_void_p),
    ]


class TraceRec(C.Structure):
    _fields_ = [("kind", C.c_long), ("n_active", C.c_long), ("n_enter", C.c_long), ("n_leave", C.c_long),
                ("factor_branch", C.c_long), ("lin_iters", C.c_long), ("tau", C.c_double), ("res_prim", C.c_double),
                ("res_dual", C.c_double), ("res_prim_in", C.c_double), ("res_dual_in", C.c_double),
                ("sigma", C.c_double), ("eps_in", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("newton_passes", C.c_long), ("lin_iters", C.c_long), ("spmv_calls", C.c_long),
                ("spmv_alg_bytes", C.c_double), ("factor_count", C.c_long), ("linsolve", C.c_long),
                ("spmv_Q_avg_s", C.c_double), ("spmv_Q_samples", C.c_long),
                ("spmv_Ac_time_s", C.c_double), ("spmv_Ac_bytes", C.c_double), ("spmv_Ac_samples", C.c_long),
                ("schur_passes", C.c_long), ("lowrank_solves", C.c_long), ("lowrank_cols", C.c_long), ("lowrank_sweeps", C.c_long),
                ("lowrank_rejects", C.c_long), ("pcg_soft_accepts", C.c_long), ("collectives", C.c_long), ("inner_solves", C.c_long),
                ("inner_steps", C.c_long), ("inner_collectives", C.c_long), ("chain_fallbacks", C.c_long),
                ("pcg_max_relres", C.c_double), ("pcg_dense_fallbacks", C.c_long), ("fused_solves", C.c_long), ("fused_kernel_s", C.c_double),
                ("pcg_rescues", C.c_long), ("pcg_rescue_kinds", C.c_long), ("hybrid_pcg_passes", C.c_long), ("band_fallbacks", C.c_long),
                ("onelaunch_factors", C.c_long), ("ahead_steps", C.c_long), ("ahead_skips", C.c_long),
                ("updown_solves", C.c_long), ("updown_rows", C.c_long), ("updown_rejects", C.c_long),
                ("coupled_rows", C.c_long), ("coupled_solves", C.c_long), ("coupled_sweeps", C.c_long), ("coupled_rejects", C.c_long),
                ("inner_refine_sweeps", C.c_long), ("inner_refine_fp64_applies", C.c_long), ("inner_refine_fallbacks", C.c_long),
                ("inner_refine_max_res_over_tol", C.c_double), ("inner_x32_steps", C.c_long),
                ("inner_h16_steps", C.c_long), ("inner_h16_sweeps", C.c_long)]


API_SYMBOLS = ["qpdo_set_default_settings", "qpdo_setup", "qpdo_warm_start", "qpdo_solve", "qpdo_update_settings",
               "qpdo_update_bounds", "qpdo_update_q", "qpdo_cleanup"]
class BatchItem(C.Structure):
    _fields_ = [("data", C.POINTER(QPDOData)), ("x0", dp), ("y0", dp), ("x", dp), ("y", dp), ("info", QPDOInfo)]


EXT_SYMBOLS = ["qpdo_amd_dist_config", "qpdo_amd_dist_unique_id", "qpdo_amd_solve_batch", "qpdo_amd_batch_kernel_seconds", "qpdo_amd_batch_stream_create",
               "qpdo_amd_batch_stream_submit", "qpdo_amd_batch_stream_wait", "qpdo_amd_batch_stream_destroy", "qpdo_amd_device_count", "qpdo_amd_last_error", "qpdo_amd_get_stats", "qpdo_amd_get_trace",
               "qpdo_amd_sync", "qpdo_amd_pass_decision", "qpdo_amd_bench_spmv", "qpdo_amd_bench_dense_factor", "qpdo_amd_spmv", "qpdo_amd_linesearch", "qpdo_amd_download",
               "qpdo_amd_update_matrices", "qpdo_amd_direct_solve", "qpdo_amd_download_factor", "qpdo_amd_pcg_probe", "qpdo_amd_download_compact",
               "qpdo_amd_fleet_create", "qpdo_amd_fleet_update", "qpdo_amd_fleet_warm_start", "qpdo_amd_fleet_warm_start_last",
               "qpdo_amd_fleet_solve", "qpdo_amd_fleet_get_stats", "qpdo_amd_fleet_get_certificates", "qpdo_amd_fleet_destroy",
               "qpdo_amd_fleet_create_ex", "qpdo_amd_fleet_update_matrices", "qpdo_amd_fleet_get_matrix_stats",
               "qpdo_amd_small_factor_layout", "qpdo_amd_fleet_factor_layout", "qpdo_amd_batch_factor_layout",
               "qpdo_amd_fleet_device", "qpdo_amd_fleet_packed_layout", "qpdo_amd_fleet_get_packed_layout", "qpdo_amd_fleet_update_dev",
               "qpdo_amd_fleet_warm_start_dev", "qpdo_amd_fleet_warm_start_last_dev", "qpdo_amd_fleet_solve_dev", "qpdo_amd_fleet_fetch_last",
               "qpdo_amd_fleet_sync", "qpdo_amd_slab_trip_shape",
               "qpdo_amd_fleet_packed_matrix_layout", "qpdo_amd_fleet_get_packed_matrix_layout", "qpdo_amd_fleet_update_matrices_dev",
               "qpdo_amd_fleet_adjoint_dev", "qpdo_amd_fleet_get_adjoint_stats",
               "qpdo_amd_fleet_adjoint_multi_dev", "qpdo_amd_fleet_tangent_dev", "qpdo_amd_fleet_rhs_group", "qpdo_amd_fleet_get_sensitivity_stats",
               "qpdo_amd_adjoint", "qpdo_amd_get_adjoint_stats", "qpdo_amd_tangent", "qpdo_amd_get_tangent_stats",
               "qpdo_amd_rhs_group", "qpdo_amd_get_group_stats", "qpdo_amd_spmv_group",
               "qpdo_amd_band_order", "qpdo_amd_band_order_config", "qpdo_amd_get_band_order",
               "qpdo_amd_band_border", "qpdo_amd_get_band_border"]


class BandOrderInfo(C.Structure):
    """QPDOAmdBandOrderInfo (include/qpdo_amd_ext.h)"""
    _fields_ = [("mode", C.c_long), ("adopted", C.c_long), ("b_natural", C.c_long), ("b_ordered", C.c_long), ("reason", C.c_long),
                ("order_seconds", C.c_double)]


BAND_ORDER_ENV, BAND_ORDER_NATURAL, BAND_ORDER_RCM, BAND_ORDER_GIVEN = 0, 1, 2, 3      # QPDO_AMD_BAND_ORDER_*
BAND_ORDER_REASONS = {0: "", 1: "reverse Cuthill-McKee found no narrower order", 2: "row-partitioned workspace", 3: "QPDO_BAND_COUPLING is set",
                      4: "fused small-problem route", 5: "QPDO_LINSOLVE is dense or pcg", 6: "the workspace adopted a border of coupling variables"}


class BandBorderInfo(C.Structure):
    """QPDOAmdBandBorderInfo (include/qpdo_amd_ext.h)"""
    _fields_ = [("max_border", C.c_long), ("border", C.c_long), ("n_core", C.c_long), ("b_core", C.c_long), ("over", C.c_long), ("reason", C.c_long),
                ("border_solves", C.c_long)]


BAND_BORDER_REASONS = {0: "", 1: "more border variables than QPDO_BAND_BORDER accepts", 2: "row-partitioned workspace", 3: "QPDO_BAND_COUPLING is set",
                       4: "fused small-problem route", 5: "QPDO_LINSOLVE is dense or pcg", 6: "the core is too short for the band solver"}


class AdjointStats(C.Structure):
    """QPDOAmdAdjointStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("calls", C.c_long), ("rhs_total", C.c_long), ("factorizations", C.c_long), ("sweeps_total", C.c_long),
                ("scratch_bytes", C.c_long), ("last_seconds", C.c_double)]


class TangentStats(C.Structure):
    """QPDOAmdTangentStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("calls", C.c_long), ("rhs_total", C.c_long), ("factorizations", C.c_long), ("sweeps_total", C.c_long),
                ("scratch_bytes", C.c_long), ("last_seconds", C.c_double)]


class GroupStats(C.Structure):
    """QPDOAmdGroupStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("group", C.c_long), ("groups_run", C.c_long), ("rounds_total", C.c_long), ("scratch_bytes", C.c_long)]


class FleetStats(C.Structure):
    """QPDOAmdFleetStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("count", C.c_long), ("matrix_bytes_uploaded", C.c_long), ("vector_bytes_uploaded_last_call", C.c_long),
                ("solve_launches", C.c_long), ("solves", C.c_long), ("last_kernel_seconds", C.c_double)]


class FleetMatrixStats(C.Structure):
    """QPDOAmdFleetMatrixStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("calls", C.c_long), ("items_last_call", C.c_long), ("value_bytes_uploaded_last_call", C.c_long),
                ("resident_extra_bytes", C.c_long), ("last_kernel_seconds", C.c_double)]


class FleetDevStats(C.Structure):
    """QPDOAmdFleetDevStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("update_calls", C.c_long), ("warm_start_calls", C.c_long), ("solve_calls", C.c_long), ("refused_items", C.c_long),
                ("first_refused_item", C.c_long)]


class FleetAdjointStats(C.Structure):
    """QPDOAmdFleetAdjointStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("adjoint_calls", C.c_long), ("resident_extra_bytes", C.c_long)]


class FleetSensitivityStats(C.Structure):
    """QPDOAmdFleetSensitivityStats (include/qpdo_amd_ext.h)"""
    _fields_ = [("calls", C.c_long), ("rhs_total", C.c_long), ("scratch_bytes", C.c_long)]


FLEET_TABLE_BYTES = 16     # QPDO_AMD_FLEET_TABLE_BYTES
FLEET_ADJOINT = 8          # QPDO_AMD_FLEET_ADJOINT
ADJ_ACCEPTED, ADJ_NOT_ACCEPTED, ADJ_NOT_SOLVED, ADJ_BAD_PIVOT = 0, 1, 2, 3     # the codes of adj_status
FLEET_MATRIX_UPDATES = 1   # QPDO_AMD_FLEET_MATRIX_UPDATES
FLEET_MATRIX_TABLE_BYTES = 8     # QPDO_AMD_FLEET_MATRIX_TABLE_BYTES
K_GLOBAL, K_PACKED, K_BAND = 0, 1, 2     # QPDO_AMD_SMALL_K_*: where the fused kernel keeps the Newton matrix
KIND_BATCH, KIND_STREAM, KIND_FLEET = 0, 1, 2

_lib = None


def lib():
    """Loads libqpdo_amd.so (building it in-tree if needed).  Raises if it is unavailable."""
    global _lib
    if _lib is None:
        # batch streams keep up to `depth` launches in flight on separate HIP streams; two streams that share one of the runtime's
        # GPU_MAX_HW_QUEUES (default 4) hardware queues serialise (7.0 k vs 10.1 k QP/s at depth 12).  The variable is read at the
        # process's first HIP call, so it is the CALLER's to set: this front end does it here, before the library is loaded -- the
        # library itself never changes its host's environment.  No effect if HIP was initialised earlier.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        L = C.CDLL(_build.ensure_lib())
        W = C.POINTER(QPDOWorkspace)
        L.qpdo_set_default_settings.argtypes = [C.POINTER(QPDOSettings)]
        L.qpdo_setup.restype = W
        L.qpdo_setup.argtypes = [C.POINTER(QPDOData), C.POINTER(QPDOSettings)]
        L.qpdo_warm_start.argtypes = [W, dp, dp]
        L.qpdo_solve.argtypes = [W]
        L.qpdo_update_settings.argtypes = [W, C.POINTER(QPDOSettings)]
        L.qpdo_update_bounds.argtypes = [W, dp, dp]
        L.qpdo_update_q.argtypes = [W, dp]
        L.qpdo_cleanup.argtypes = [W]
        L.qpdo_amd_device_count.restype = C.c_int
        L.qpdo_amd_last_error.restype = C.c_char_p
        L.qpdo_amd_get_stats.argtypes = [W, C.POINTER(Stats)]
        L.qpdo_amd_get_trace.argtypes = [W, C.POINTER(C.POINTER(TraceRec)), C.POINTER(C.c_long)]
        L.qpdo_amd_sync.argtypes = [W]
        L.qpdo_amd_bench_spmv.argtypes = [W, C.c_int, C.c_int, dp, dp]
        L.qpdo_amd_spmv.argtypes = [W, C.c_int, dp, dp]
        L.qpdo_amd_bench_dense_factor.argtypes = [W, C.c_int, dp, dp]
        L.qpdo_amd_linesearch.argtypes = [W, C.c_double, C.c_double, dp, dp, dp]
        L.qpdo_amd_download.argtypes = [W, C.c_int, dp]
        L.qpdo_amd_direct_solve.argtypes = [W, dp, C.c_double, dp, dp, C.c_int]
        L.qpdo_amd_direct_solve.restype = C.c_int
        L.qpdo_amd_download_factor.argtypes = [W, C.c_int, dp, C.c_long]
        L.qpdo_amd_download_factor.restype = C.c_int
        L.qpdo_amd_pcg_probe.argtypes = [W, dp, C.c_double, dp, dp, C.c_int, dp]
        L.qpdo_amd_pcg_probe.restype = C.c_int
        L.qpdo_amd_download_compact.argtypes = [W, C.c_int, C.c_void_p, C.c_long]
        L.qpdo_amd_download_compact.restype = C.c_int
        L.qpdo_amd_update_matrices.argtypes = [W, C.POINTER(CholmodSparse), C.POINTER(CholmodSparse)]
        L.qpdo_amd_update_matrices.restype = C.c_int
        if hasattr(L, "qpdo_amd_adjoint"):                  # (absent from an older build named by QPDO_AMD_LIB: calling it there raises)
            L.qpdo_amd_adjoint.argtypes = [W, C.c_long, dp, dp, dp, dp, dp, C.POINTER(CholmodSparse), dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_long), dp,
                                           C.c_double, C.c_long]
            L.qpdo_amd_adjoint.restype = C.c_int
            L.qpdo_amd_get_adjoint_stats.argtypes = [W, C.POINTER(AdjointStats)]
            L.qpdo_amd_get_adjoint_stats.restype = C.c_int
        if hasattr(L, "qpdo_amd_tangent"):
            L.qpdo_amd_tangent.argtypes = [W, C.c_long, dp, dp, dp, C.POINTER(CholmodSparse), dp, dp, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_long), dp,
                                           C.c_double, C.c_long]
            L.qpdo_amd_tangent.restype = C.c_int
            L.qpdo_amd_get_tangent_stats.argtypes = [W, C.POINTER(TangentStats)]
            L.qpdo_amd_get_tangent_stats.restype = C.c_int
        if hasattr(L, "qpdo_amd_band_order"):
            lp_ = C.POINTER(C.c_long)
            L.qpdo_amd_band_order.argtypes = [C.POINTER(CholmodSparse), C.POINTER(CholmodSparse), lp_, lp_]
            L.qpdo_amd_band_order.restype = C.c_int
            L.qpdo_amd_band_order_config.argtypes = [C.c_int, lp_, C.c_long]
            L.qpdo_amd_band_order_config.restype = C.c_int
            L.qpdo_amd_get_band_order.argtypes = [W, C.POINTER(BandOrderInfo), lp_]
            L.qpdo_amd_get_band_order.restype = C.c_int
        if hasattr(L, "qpdo_amd_band_border"):
            L.qpdo_amd_band_border.argtypes = [C.POINTER(CholmodSparse), C.POINTER(CholmodSparse), C.c_long, C.POINTER(C.c_long)]
            L.qpdo_amd_band_border.restype = C.c_int
            L.qpdo_amd_get_band_border.argtypes = [W, C.POINTER(BandBorderInfo)]
            L.qpdo_amd_get_band_border.restype = C.c_int
        if hasattr(L, "qpdo_amd_rhs_group"):
            L.qpdo_amd_rhs_group.argtypes = [W]
            L.qpdo_amd_rhs_group.restype = C.c_int
            L.qpdo_amd_get_group_stats.argtypes = [W, C.POINTER(GroupStats)]
            L.qpdo_amd_get_group_stats.restype = C.c_int
            L.qpdo_amd_spmv_group.argtypes = [W, C.c_int, C.c_int, C.c_uint, dp, dp]
            L.qpdo_amd_spmv_group.restype = C.c_int
        L.qpdo_amd_dist_config.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qpdo_amd_dist_unique_id.argtypes = [C.c_void_p]
        L.qpdo_amd_solve_batch.restype = C.c_long
        L.qpdo_amd_batch_kernel_seconds.restype = C.c_double
        L.qpdo_amd_solve_batch.argtypes = [C.c_long, C.POINTER(BatchItem), C.POINTER(QPDOSettings), C.c_int]
        L.qpdo_amd_batch_stream_create.restype = C.c_void_p
        L.qpdo_amd_batch_stream_create.argtypes = [C.c_int]
        L.qpdo_amd_batch_stream_submit.restype = C.c_long
        L.qpdo_amd_batch_stream_submit.argtypes = [C.c_void_p, C.c_long, C.POINTER(BatchItem), C.POINTER(QPDOSettings)]
        L.qpdo_amd_batch_stream_wait.restype = C.c_int
        L.qpdo_amd_batch_stream_wait.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_double)]
        L.qpdo_amd_batch_stream_destroy.argtypes = [C.c_void_p]
        pp = C.POINTER(dp)
        L.qpdo_amd_fleet_create.restype = C.c_void_p
        L.qpdo_amd_fleet_create.argtypes = [C.c_long, C.POINTER(C.POINTER(QPDOData)), C.POINTER(QPDOSettings)]
        L.qpdo_amd_fleet_create_ex.restype = C.c_void_p
        L.qpdo_amd_fleet_create_ex.argtypes = [C.c_long, C.POINTER(C.POINTER(QPDOData)), C.POINTER(QPDOSettings), C.c_long]
        sparse_pp = C.POINTER(C.POINTER(CholmodSparse))
        L.qpdo_amd_fleet_update_matrices.argtypes = [C.c_void_p, sparse_pp, sparse_pp]
        L.qpdo_amd_fleet_get_matrix_stats.argtypes = [C.c_void_p, C.POINTER(FleetMatrixStats)]
        L.qpdo_amd_fleet_update.argtypes = [C.c_void_p, pp, pp, pp]
        L.qpdo_amd_fleet_warm_start.argtypes = [C.c_void_p, pp, pp]
        L.qpdo_amd_fleet_warm_start_last.argtypes = [C.c_void_p]
        L.qpdo_amd_fleet_solve.argtypes = [C.c_void_p, pp, pp, C.POINTER(QPDOInfo)]
        L.qpdo_amd_fleet_get_stats.argtypes = [C.c_void_p, C.POINTER(FleetStats)]
        L.qpdo_amd_fleet_get_certificates.argtypes = [C.c_void_p, C.c_long, dp, dp]
        L.qpdo_amd_fleet_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "qpdo_amd_fleet_solve_dev"):          # (device arrays on the caller's stream; absent from an older build, as below)
            lp, vp = C.POINTER(C.c_long), C.c_void_p        # (device pointers travel as plain addresses)
            L.qpdo_amd_fleet_device.argtypes = [C.c_void_p]
            L.qpdo_amd_fleet_packed_layout.argtypes = [C.c_long, C.POINTER(C.POINTER(QPDOData)), lp, lp]
            L.qpdo_amd_fleet_get_packed_layout.argtypes = [C.c_void_p, lp, lp]
            L.qpdo_amd_fleet_update_dev.argtypes = [C.c_void_p, vp, vp, vp, vp, C.c_long, C.c_long, vp]
            L.qpdo_amd_fleet_warm_start_dev.argtypes = [C.c_void_p, vp, vp, vp, C.c_long, C.c_long, vp]
            L.qpdo_amd_fleet_warm_start_last_dev.argtypes = [C.c_void_p, vp]
            L.qpdo_amd_fleet_solve_dev.argtypes = [C.c_void_p, vp, vp, vp, vp, vp, vp, C.c_long, C.c_long, vp]
            L.qpdo_amd_fleet_fetch_last.argtypes = [C.c_void_p, pp, pp, C.POINTER(QPDOInfo)]
            L.qpdo_amd_fleet_sync.argtypes = [C.c_void_p, C.POINTER(FleetDevStats)]
            if hasattr(L, "qpdo_amd_fleet_update_matrices_dev"):    # (new matrix values from device arrays; absent from an older build)
                L.qpdo_amd_fleet_packed_matrix_layout.argtypes = [C.c_long, C.POINTER(C.POINTER(QPDOData)), lp, lp]
                L.qpdo_amd_fleet_get_packed_matrix_layout.argtypes = [C.c_void_p, lp, lp]
                L.qpdo_amd_fleet_update_matrices_dev.argtypes = [C.c_void_p, vp, vp, vp, C.c_long, C.c_long, vp]
            if hasattr(L, "qpdo_amd_fleet_adjoint_dev"):            # (the adjoint of the last solve; absent from an older build)
                L.qpdo_amd_fleet_adjoint_dev.argtypes = [C.c_void_p] + [vp] * 10 + [C.c_double, C.c_long] + [C.c_long] * 4 + [vp]
                L.qpdo_amd_fleet_get_adjoint_stats.argtypes = [C.c_void_p, C.POINTER(FleetAdjointStats)]
            if hasattr(L, "qpdo_amd_fleet_tangent_dev"):            # (many right-hand sides per factorization; absent from an older build)
                L.qpdo_amd_fleet_adjoint_multi_dev.argtypes = [C.c_void_p, C.c_long] + [vp] * 10 + [C.c_double, C.c_long] + [C.c_long] * 4 + [vp]
                L.qpdo_amd_fleet_tangent_dev.argtypes = [C.c_void_p, C.c_long] + [vp] * 10 + [C.c_double, C.c_long] + [C.c_long] * 4 + [vp]
                L.qpdo_amd_fleet_rhs_group.argtypes = [C.c_void_p]
                L.qpdo_amd_fleet_rhs_group.restype = C.c_int
                L.qpdo_amd_fleet_get_sensitivity_stats.argtypes = [C.c_void_p, C.POINTER(FleetSensitivityStats)]
        if hasattr(L, "qpdo_amd_slab_trip_shape"):          # (absent from an older build, as below)
            L.qpdo_amd_slab_trip_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
            L.qpdo_amd_slab_trip_shape.restype = C.c_int
        if hasattr(L, "qpdo_amd_small_factor_layout"):      # (absent from an older build named by QPDO_AMD_LIB for A/B timing: calling it there raises)
            L.qpdo_amd_small_factor_layout.argtypes = [C.c_long, C.POINTER(C.POINTER(QPDOData)), C.POINTER(QPDOSettings), C.c_int, C.POINTER(C.c_long)]
            L.qpdo_amd_small_factor_layout.restype = C.c_int
            L.qpdo_amd_fleet_factor_layout.argtypes = [C.c_void_p]
            L.qpdo_amd_fleet_factor_layout.restype = C.c_int
            L.qpdo_amd_batch_factor_layout.restype = C.c_int
        _lib = L
    return _lib


DIRECT_LOST = -2       # QPDO_AMD_DIRECT_LOST (include/qpdo_amd_ext.h)


PCG_NOT_CONVERGED, PCG_NAN, PCG_INFO_LEN, PCG_INFO_HEAD = -3, -4, 1040, 16      # QPDO_AMD_PCG_* (include/qpdo_amd_ext.h)


class PcgNotConverged(RuntimeError):
    """qpdo_amd_pcg_probe: the solve ended without meeting its tolerance (iteration cap, stagnation)"""


class PcgNaN(RuntimeError):
    """qpdo_amd_pcg_probe: the solve met a NaN residual"""


class LostProducer(RuntimeError):
    """qpdo_amd_direct_solve: a polling kernel lost its producer, or the band factorization met a bad pivot"""


def slab_trip_shape(value_bytes, operand_bytes):
    """(EPL, UNR, NSA, TPR) of the slab kernel's instance that streams values of value_bytes against a staged operand of operand_bytes
    (qpdo_amd_slab_trip_shape: 8/8, 4/8, 4/4, 2/4); what a reproduction of the kernel's summation order needs.  No GPU is touched."""
    shape = (C.c_int * 4)()
    if lib().qpdo_amd_slab_trip_shape(int(value_bytes), int(operand_bytes), shape):
        raise ValueError("slab_trip_shape: %s" % (lib().qpdo_amd_last_error() or b"").decode())
    return tuple(shape)


def device_count():
    return int(lib().qpdo_amd_device_count())


def default_settings(**over):
    s = QPDOSettings()
    lib().qpdo_set_default_settings(C.byref(s))
    names = {f for f, _ in QPDOSettings._fields_}
    for k, v in over.items():
        if k not in names:                      # qpdo.m:262-266 rejects unknown fields
            raise KeyError("unrecognized solver setting '%s'" % k)
        setattr(s, k, v)
    return s


def _as_dp(a):
    return None if a is None else a.ctypes.data_as(dp)


def _sparse_view(M, stype, keep, index_dtype=None):
    """cholmod_sparse header over the CSC arrays of M.  index_dtype None: the index type scipy holds (int32 below 2^31 entries), which the
    host driver reads as CHOLMOD_INT -- no 64-bit copy of the index arrays (0.4 s of setup at 2e8 nonzeros); np.int64: CHOLMOD_LONG, the
    reference's DLONG layout."""
    M = sp.csc_matrix(M)
    M.sort_indices()
    if index_dtype is None:
        index_dtype = np.int32 if M.indices.dtype == np.int32 and M.indptr.dtype == np.int32 else np.int64
    p = np.ascontiguousarray(M.indptr, index_dtype)
    i = np.ascontiguousarray(M.indices, index_dtype)
    x = np.ascontiguousarray(M.data, np.float64)
    keep.extend([p, i, x])
    s = CholmodSparse()
    s.nrow, s.ncol, s.nzmax = M.shape[0], M.shape[1], max(1, len(x))
    s.p, s.i, s.x = p.ctypes.data, i.ctypes.data, x.ctypes.data
    s.nz, s.z = None, None
    s.stype, s.itype, s.xtype, s.dtype, s.sorted, s.packed = stype, (2 if index_dtype == np.int64 else 0), 1, 0, 1, 1
    return s


def project_to_pattern(M, indptr, indices):
    """The values of the sparse matrix M laid out in the CSC pattern (indptr, indices) -- sorted row indices, as setup hands them over.
    M's own pattern must be a subset of it: an entry of the pattern that M lacks becomes an explicit 0.0; an entry of M outside the
    pattern raises ValueError.  Duplicates of M are summed first.  Pure host arithmetic (qpdo_amd_update_matrices takes the setup's
    pattern only)."""
    if sp.isspmatrix_csc(M) and M.has_canonical_format and len(M.indices) == len(indices) and np.array_equal(M.indptr, indptr) \
            and np.array_equal(M.indices, indices):
        return np.array(M.data, np.float64)            # the pattern itself (the common case): no search
    M = sp.csc_matrix(M, copy=True)
    M.sum_duplicates()
    ncol = len(indptr) - 1
    if M.shape[1] != ncol:
        raise ValueError("matrix has %d columns, the pattern %d" % (M.shape[1], ncol))
    nrow = M.shape[0]
    pcol = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(np.asarray(indptr, np.int64)))
    pkey = pcol * nrow + np.asarray(indices, np.int64)
    mcol = np.repeat(np.arange(ncol, dtype=np.int64), np.diff(M.indptr.astype(np.int64)))
    mkey = mcol * nrow + M.indices.astype(np.int64)
    pos = np.searchsorted(pkey, mkey)
    ok = pos < len(pkey)
    ok[ok] = pkey[pos[ok]] == mkey[ok]
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError("entry (%d, %d) is outside the sparsity pattern given to setup" % (int(M.indices[k]), int(mcol[k])))
    x = np.zeros(len(pkey))
    x[pos] = M.data
    return x


class QPDO:
    """solver = QPDO(); solver.setup(Q, q, A, l, u, **settings); res = solver.solve()"""

    def __init__(self):
        self._w = None
        self.n = self.m = 0

    # qpdo.m:50-160
    def setup(self, Q, q, A, l, u, settings=None, Qstype=None, c=0.0, index_dtype=None, **kw):
        if self._w:
            raise RuntimeError("Solver is already initialized with problem data.")   # qpdo_mex.c:122-124
        A = sp.csc_matrix(A)
        Q = sp.csc_matrix(Q)
        m, n = A.shape
        if Q.shape != (n, n):
            raise ValueError("Q must be n x n with n = number of columns of A")
        q = np.zeros(n) if q is None else np.ascontiguousarray(q, np.float64).ravel()
        l = np.full(m, -QPDO_INFTY) if l is None else np.ascontiguousarray(l, np.float64).ravel()
        u = np.full(m, QPDO_INFTY) if u is None else np.ascontiguousarray(u, np.float64).ravel()
        if len(q) != n or len(l) != m or len(u) != m:
            raise ValueError("incompatible vector dimensions")
        l = np.clip(l, -QPDO_INFTY, QPDO_INFTY)      # qpdo.m:138-139
        u = np.clip(u, -QPDO_INFTY, QPDO_INFTY)
        self._Qtril = Qstype is None
        if Qstype is None:
            Q = sp.tril(Q).tocsc()                     # the mex reads the lower triangle (qpdo_mex.c:150)
            Qstype = -1
        if settings is None:
            settings = default_settings(**kw)
        elif kw:
            for k, v in kw.items():
                if not hasattr(settings, k):
                    raise KeyError("unrecognized solver setting '%s'" % k)
                setattr(settings, k, v)
        keep = [q, l, u]
        Qs, As = _sparse_view(Q, Qstype, keep, index_dtype), _sparse_view(A, 0, keep, index_dtype)
        data = QPDOData()
        data.n, data.m, data.Q, data.A = n, m, C.pointer(Qs), C.pointer(As)
        data.q, data.c, data.l, data.u = _as_dp(q), float(c), _as_dp(l), _as_dp(u)
        w = lib().qpdo_setup(C.byref(data), C.byref(settings))
        if not w:
            raise RuntimeError("Invalid problem setup: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        self._w, self.n, self.m = w, n, m
        # the pattern as handed over (sorted CSC; keep[] holds Q's p, i, x then A's): update_matrices projects onto it
        self._Qstype, self._Qpat, self._Apat = Qstype, (keep[3], keep[4]), (keep[6], keep[7])
        self._Qview, self._Qview_keep = Qs, keep[3:6]      # (the header over Q's arrays as handed over: adjoint passes it with dQx)
        return self

    def update_matrices(self, Q=None, A=None):
        """New values of Q and / or A (None: unchanged) in the pattern given to setup; a matrix whose pattern is a subset of the setup's is
        projected onto it (dropped entries become explicit zeros).  Afterwards the workspace is the one setup would return for the new
        matrices and the latest q, l, u (qpdo_amd_update_matrices); warm-start explicitly if wanted."""
        keep, views = [], []
        for is_Q, M, pat, stype, shape in ((True, Q, self._Qpat, self._Qstype, (self.n, self.n)), (False, A, self._Apat, 0, (self.m, self.n))):
            if M is None:
                views.append(None)
                continue
            M = sp.csc_matrix(M)
            if M.shape != shape:
                raise ValueError("matrix is %d x %d, expected %d x %d" % (M.shape + shape))
            if is_Q and self._Qtril and not (M.has_canonical_format and np.array_equal(M.indptr, pat[0]) and np.array_equal(M.indices, pat[1])):
                M = sp.tril(M).tocsc()                 # as setup normalised it (a matrix in the stored pattern already is lower)
            x = project_to_pattern(M, pat[0], pat[1])
            keep.append(x)
            s = CholmodSparse()
            s.nrow, s.ncol, s.nzmax = shape[0], shape[1], max(1, len(x))
            s.p, s.i, s.x = pat[0].ctypes.data, pat[1].ctypes.data, x.ctypes.data
            s.nz, s.z = None, None
            s.stype, s.itype, s.xtype, s.dtype, s.sorted, s.packed = stype, (2 if pat[0].dtype == np.int64 else 0), 1, 0, 1, 1
            views.append(s)
        rc = lib().qpdo_amd_update_matrices(self._w, C.byref(views[0]) if views[0] is not None else None,
                                            C.byref(views[1]) if views[1] is not None else None)
        if rc:
            raise RuntimeError("update_matrices: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        return self

    @property
    def work(self):
        return self._w.contents

    def warm_start(self, x=None, y=None):
        x = None if x is None else np.ascontiguousarray(x, np.float64)
        y = None if y is None else np.ascontiguousarray(y, np.float64)
        lib().qpdo_warm_start(self._w, _as_dp(x), _as_dp(y))

    def update_bounds(self, l=None, u=None):
        l = None if l is None else np.clip(np.ascontiguousarray(l, np.float64), -QPDO_INFTY, QPDO_INFTY)   # qpdo.m:215-216
        u = None if u is None else np.clip(np.ascontiguousarray(u, np.float64), -QPDO_INFTY, QPDO_INFTY)
        lib().qpdo_update_bounds(self._w, _as_dp(l), _as_dp(u))

    def update_q(self, q):
        q = np.ascontiguousarray(q, np.float64)
        if len(q) != self.n:
            raise ValueError("q has wrong length")
        lib().qpdo_update_q(self._w, _as_dp(q))

    def update_settings(self, settings=None, **kw):
        s = QPDOSettings()
        C.memmove(C.byref(s), self.work.settings, C.sizeof(QPDOSettings))
        if settings is not None:
            s = settings
        for k, v in kw.items():
            if not hasattr(s, k):
                raise KeyError("unrecognized solver setting '%s'" % k)
            setattr(s, k, v)
        lib().qpdo_update_settings(self._w, C.byref(s))

    def info(self):
        i = self.work.info.contents
        d = {f: getattr(i, f) for f, _ in QPDOInfo._fields_}
        d["status"] = d["status"].decode()
        return d

    def _vec(self, ptr, n):
        return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0)

    # qpdo_mex.c:227-281
    def solve(self):
        lib().qpdo_solve(self._w)
        info = self.info()
        st = info["status_val"]
        w = self.work
        nan_n, nan_m = np.full(self.n, np.nan), np.full(self.m, np.nan)
        res = dict(info=info, x=nan_n, y=nan_m, prim_inf_cert=nan_m.copy(), dual_inf_cert=nan_n.copy())
        if st not in (-3, -4):
            res["x"] = self._vec(w.solution.contents.x, self.n)
            res["y"] = self._vec(w.solution.contents.y, self.m)
        elif st == -3:
            res["prim_inf_cert"] = self._vec(w.dy, self.m)
        else:
            res["dual_inf_cert"] = self._vec(w.dx, self.n)
        return res

    # extensions
    def stats(self):
        s = Stats()
        lib().qpdo_amd_get_stats(self._w, C.byref(s))
        return {f: getattr(s, f) for f, _ in Stats._fields_}

    def trace(self):
        p, n = C.POINTER(TraceRec)(), C.c_long(0)
        lib().qpdo_amd_get_trace(self._w, C.byref(p), C.byref(n))
        return [{f: getattr(p[i], f) for f, _ in TraceRec._fields_} for i in range(n.value)]

    def bench_spmv(self, which, reps=20):
        t, b = C.c_double(0), C.c_double(0)
        rc = lib().qpdo_amd_bench_spmv(self._w, which, reps, C.byref(t), C.byref(b))
        if rc:
            raise RuntimeError(lib().qpdo_amd_last_error().decode())
        return t.value, b.value

    def bench_dense_factor(self, reps=5, check=True):
        t, c = C.c_double(0), C.c_double(0)
        rc = lib().qpdo_amd_bench_dense_factor(self._w, reps, C.byref(t), C.byref(c) if check else None)
        if rc:
            raise RuntimeError(lib().qpdo_amd_last_error().decode())
        return t.value, c.value

    def spmv(self, which, v):
        v = np.ascontiguousarray(v, np.float64)
        rows = {0: self.m, 1: self.n, 2: self.n}[which]
        y = np.zeros(rows)
        rc = lib().qpdo_amd_spmv(self._w, which, _as_dp(v), _as_dp(y))
        if rc:
            raise RuntimeError(lib().qpdo_amd_last_error().decode())
        return y

    def linesearch(self, eta, beta, delta, alpha):
        delta = np.ascontiguousarray(delta, np.float64)
        alpha = np.ascontiguousarray(alpha, np.float64)
        assert len(delta) == 2 * self.m == len(alpha)
        t = C.c_double(0)
        rc = lib().qpdo_amd_linesearch(self._w, float(eta), float(beta), _as_dp(delta), _as_dp(alpha), C.byref(t))
        if rc:
            raise RuntimeError(lib().qpdo_amd_last_error().decode())
        return t.value

    def direct_solve(self, dw, sigma, rhs, refactor=True, carry_forward=False):
        """x = K^-1 rhs, K = Q + sigma I + A' diag(dw) A, through the workspace's direct solver (qpdo_amd_direct_solve).  A lost producer
        (or a bad band pivot) raises LostProducer, any other failure RuntimeError."""
        dw = np.ascontiguousarray(dw, np.float64)
        rhs = np.ascontiguousarray(rhs, np.float64)
        if len(dw) != self.m or len(rhs) != self.n:
            raise ValueError("dw needs m entries and rhs n")
        x = np.zeros(self.n)
        rc = lib().qpdo_amd_direct_solve(self._w, _as_dp(dw), float(sigma), _as_dp(rhs), _as_dp(x), (1 if refactor else 0) | (2 if carry_forward else 0))
        if rc:
            msg = (lib().qpdo_amd_last_error() or b"").decode()
            raise (LostProducer if rc == DIRECT_LOST else RuntimeError)("direct_solve: %s" % msg)
        return x

    def adjoint(self, gx, gy=None, matrices=False, tol=1e-9, max_sweeps=20):
        """The gradients of a loss L(x, y) of the last solve's solution w.r.t. q, l, u (and, matrices=True, the stored values of Q and A)
        from gx = dL/dx and gy = dL/dy (None: zero), through the workspace's direct solver (qpdo_amd_adjoint, include/qpdo_amd_ext.h).
        gx: (n,) or (R, n), gy: (m,) / (R, m): R right-hand sides on ONE factorization; the outputs carry the same leading R.  Returns
        dict(dq, dl, du, dQ_values, dA_values (None without matrices), active (m,) int32, status (3,) / (R, 3) int64: code, sweeps,
        active rows, residual).  A right-hand side whose code is not 0 holds NaN.  A refused call raises RuntimeError with the reason.
        Taken: the dense LDL' and every band workspace (QPDO_LINSOLVE=band: half-bandwidth <= 127, the wide band 128 .. 1023, a variable
        order, coupling rows -- the last takes more sweeps, one Woodbury application each); refused: PCG, hybrid, row-partitioned."""
        def arr(name, a, length):
            if not isinstance(a, np.ndarray):
                raise ValueError("%s: expected a numpy array, got %s" % (name, type(a).__name__))
            if a.dtype != np.float64:
                raise ValueError("%s: expected dtype float64, got %s" % (name, a.dtype))
            if a.ndim not in (1, 2) or a.shape[-1] != length:
                raise ValueError("%s: expected shape (%d,) or (R, %d), got %s" % (name, length, length, a.shape))
            return np.ascontiguousarray(a)
        gx = arr("gx", gx, self.n)
        single = gx.ndim == 1
        R = 1 if single else gx.shape[0]
        if R < 1:
            raise ValueError("gx: expected at least one right-hand side")
        if gy is not None:
            gy = arr("gy", gy, self.m)
            if gy.shape != gx.shape[:-1] + (self.m,):
                raise ValueError("gy: expected shape %s to go with gx, got %s" % (gx.shape[:-1] + (self.m,), gy.shape))
        if not self._w:
            raise RuntimeError("adjoint: no workspace (call setup first)")
        nq, na = len(self._Qview_keep[2]), len(self._Apat[1])
        dq, dl, du = np.empty((R, self.n)), np.empty((R, self.m)), np.empty((R, self.m))
        dQ, dA = (np.empty((R, nq)), np.empty((R, na))) if matrices else (None, None)
        active, status, res = np.zeros(self.m, np.int32), np.zeros((R, 3), np.int64), np.empty(R)
        rc = lib().qpdo_amd_adjoint(self._w, R, _as_dp(gx), _as_dp(gy), _as_dp(dq), _as_dp(dl), _as_dp(du), C.byref(self._Qview) if matrices else None,
                                    _as_dp(dQ), _as_dp(dA), active.ctypes.data_as(C.POINTER(C.c_int)), status.ctypes.data_as(C.POINTER(C.c_long)),
                                    _as_dp(res), float(tol), int(max_sweeps))
        if rc:
            raise RuntimeError("adjoint: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        out = dict(dq=dq, dl=dl, du=du, dQ_values=dQ, dA_values=dA, status=status, residual=res)
        if single:
            out = {k: (None if v is None else v[0]) for k, v in out.items()}
        out["active"] = active
        return out

    def adjoint_stats(self):
        s = AdjointStats()
        if lib().qpdo_amd_get_adjoint_stats(self._w, C.byref(s)):
            raise RuntimeError("adjoint_stats: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        return {f: getattr(s, f) for f, _ in AdjointStats._fields_}

    def tangent(self, tq=None, tl=None, tu=None, tQ_values=None, tA_values=None, tol=1e-9, max_sweeps=20):
        """The first-order change (dx, dy) of the last solve's solution for a change (tq, tl, tu, tQ_values, tA_values) of q, l, u and the
        stored values of Q and A (None: no change), at the fixed active set, through the workspace's direct solver (qpdo_amd_tangent,
        include/qpdo_amd_ext.h).  Every array is (L,) or (R, L) with L = n, m, m, the stored entries of Q, the entries of A: R right-hand
        sides on ONE factorization; all arrays passed agree on R and the outputs carry the same leading R.  Returns dict(dx, dy, active
        (m,) int32, status (3,) / (R, 3) int64: code, sweeps, active rows, residual).  A right-hand side whose code is not 0 holds NaN.  A
        refused call raises RuntimeError with the reason."""
        if not hasattr(self, "_Qview_keep"):
            nq, na = None, None
        else:
            nq, na = len(self._Qview_keep[2]), len(self._Apat[1])
        given = [(k, a, length) for k, a, length in (("tq", tq, self.n), ("tl", tl, self.m), ("tu", tu, self.m), ("tQ_values", tQ_values, nq),
                                                      ("tA_values", tA_values, na)) if a is not None]
        if not given:
            raise ValueError("no tangent passed: at least one of tq, tl, tu, tQ_values, tA_values is needed")
        arrs, lead = {}, None
        for name, a, length in given:
            if not isinstance(a, np.ndarray):
                raise ValueError("%s: expected a numpy array, got %s" % (name, type(a).__name__))
            if a.dtype != np.float64:
                raise ValueError("%s: expected dtype float64, got %s" % (name, a.dtype))
            if length is None:
                raise RuntimeError("tangent: no workspace (call setup first)")
            if a.ndim not in (1, 2) or a.shape[-1] != length:
                raise ValueError("%s: expected shape (%d,) or (R, %d), got %s" % (name, length, length, a.shape))
            if lead is None:
                lead, first = a.shape[:-1], name
            elif a.shape[:-1] != lead:
                raise ValueError("%s and %s do not agree on R: leading shapes %s and %s" % (first, name, lead, a.shape[:-1]))
            arrs[name] = np.ascontiguousarray(a)
        single = lead == ()
        R = 1 if single else lead[0]
        if R < 1:
            raise ValueError("%s: expected at least one right-hand side" % first)
        if not self._w:
            raise RuntimeError("tangent: no workspace (call setup first)")
        dx, dy = np.empty((R, self.n)), np.empty((R, self.m))
        active, status, res = np.zeros(self.m, np.int32), np.zeros((R, 3), np.int64), np.empty(R)
        g = arrs.get
        rc = lib().qpdo_amd_tangent(self._w, R, _as_dp(g("tq")), _as_dp(g("tl")), _as_dp(g("tu")), C.byref(self._Qview) if "tQ_values" in arrs else None,
                                    _as_dp(g("tQ_values")), _as_dp(g("tA_values")), _as_dp(dx), _as_dp(dy), active.ctypes.data_as(C.POINTER(C.c_int)),
                                    status.ctypes.data_as(C.POINTER(C.c_long)), _as_dp(res), float(tol), int(max_sweeps))
        if rc:
            raise RuntimeError("tangent: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        out = dict(dx=dx, dy=dy, status=status, residual=res)
        if single:
            out = {k: v[0] for k, v in out.items()}
        out["active"] = active
        return out

    def tangent_stats(self):
        s = TangentStats()
        if lib().qpdo_amd_get_tangent_stats(self._w, C.byref(s)):
            raise RuntimeError("tangent_stats: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        return {f: getattr(s, f) for f, _ in TangentStats._fields_}

    def rhs_group(self):
        """The right-hand sides adjoint / tangent carry through every launch of their sweep loop at once on this workspace
        (qpdo_amd_rhs_group): 8 where it qualifies (the dense LDL' with chained solves and every band workspace, the wide band and coupling
        rows included), 1: one after the other, 0: a workspace the two calls refuse."""
        g = lib().qpdo_amd_rhs_group(self._w)
        if g < 0:
            raise RuntimeError("rhs_group: no workspace (call setup first)")
        return g

    def group_stats(self):
        s = GroupStats()
        if lib().qpdo_amd_get_group_stats(self._w, C.byref(s)):
            raise RuntimeError("group_stats: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        return {f: getattr(s, f) for f, _ in GroupStats._fields_}

    def spmv_group(self, which, v, live_mask, fill=0.0):
        """Test hook (qpdo_amd_spmv_group): y[g] = M v[g] for the slabs g of live_mask; v: (nvec, ncols).  The other slabs of the
        returned (nvec, nrows) array keep `fill`."""
        v = np.ascontiguousarray(v, np.float64)
        rows = {0: self.m, 1: self.n, 2: self.n}[which]
        y = np.full((v.shape[0], rows), fill)
        rc = lib().qpdo_amd_spmv_group(self._w, which, v.shape[0], int(live_mask), _as_dp(v), _as_dp(y))
        if rc:
            raise RuntimeError(lib().qpdo_amd_last_error().decode())
        return y

    def jacobian(self, wrt=("q", "l", "u"), outputs=("x",), mode="auto", tol=1e-9, max_sweeps=20):
        """Dense Jacobians of the last solve's solution at the fixed active set: dx_dq (n x n), dx_dl, dx_du (n x m) for the names in wrt
        and, with "y" in outputs, dy_dq (m x n), dy_dl, dy_du (m x m), from ONE call with many right-hand sides -- which the workspace
        carries through its sweeps in groups (rhs_group()).
          mode="tangent": R = the sum of the sizes of wrt; column j of d._dq is tangent(tq = e_j), of d._dl tangent(tl = e_j), ...
          mode="adjoint": R = the sum of the sizes of outputs; row i of dx_d. is adjoint(gx = e_i), row i of dy_d. adjoint(gx = 0, gy = e_i)
          mode="auto": the mode with fewer right-hand sides, adjoint on a tie.
        Returns a dict with the requested blocks, active (m,) int32, status (R, 3) int64 and the mode taken.  A right-hand side whose
        code is not 0 leaves NaN in its column (tangent) or row (adjoint) of every block.  Host memory: the call's arrays hold R x (n + m)
        doubles each (the unit right-hand sides and the results); the blocks returned are copies of those.  Names are checked before
        any library call; a refused call raises RuntimeError with the reason."""
        def names(arg, what, allowed):
            if isinstance(arg, str) or not isinstance(arg, (tuple, list)):
                raise ValueError("%s: expected a tuple of names from %s, got %r" % (what, allowed, arg))
            for a in arg:
                if a not in allowed:
                    raise ValueError("%s: unknown name %r (expected names from %s)" % (what, a, allowed))
            if len(set(arg)) != len(arg):
                raise ValueError("%s: a name is given twice: %r" % (what, tuple(arg)))
            if not arg:
                raise ValueError("%s: expected at least one name from %s" % (what, allowed))
            return tuple(arg)
        wrt = names(wrt, "wrt", ("q", "l", "u"))
        outputs = names(outputs, "outputs", ("x", "y"))
        if mode not in ("auto", "tangent", "adjoint"):
            raise ValueError("mode: expected 'auto', 'tangent' or 'adjoint', got %r" % (mode,))
        if not self._w:
            raise RuntimeError("jacobian: no workspace (call setup first)")
        n, m = self.n, self.m
        size = {"q": n, "l": m, "u": m, "x": n, "y": m}
        r_tan, r_adj = sum(size[k] for k in wrt), sum(size[k] for k in outputs)
        if mode == "auto":
            mode = "tangent" if r_tan < r_adj else "adjoint"
        out = {"mode": mode}
        if mode == "tangent":
            if r_tan < 1:
                raise ValueError("wrt: the names given have no entries on this workspace (m = 0)")
            arrs, off = {}, 0
            for k in wrt:
                a = np.zeros((r_tan, size[k]))
                a[off + np.arange(size[k]), np.arange(size[k])] = 1.0
                arrs["t" + k] = a
                off += size[k]
            t = self.tangent(tol=tol, max_sweeps=max_sweeps, **arrs)
            off = 0
            for k in wrt:
                for o in outputs:
                    out["d%s_d%s" % (o, k)] = np.ascontiguousarray(t["d" + o][off:off + size[k]].T)
                off += size[k]
            out["active"], out["status"] = t["active"], t["status"]
            return out
        if r_adj < 1:
            raise ValueError("outputs: the names given have no entries on this workspace (m = 0)")
        gx, gy = np.zeros((r_adj, n)), (np.zeros((r_adj, m)) if "y" in outputs else None)
        off = 0
        for o in outputs:
            (gx if o == "x" else gy)[off + np.arange(size[o]), np.arange(size[o])] = 1.0
            off += size[o]
        a = self.adjoint(gx, gy, tol=tol, max_sweeps=max_sweeps)
        off = 0
        for o in outputs:
            for k in wrt:
                out["d%s_d%s" % (o, k)] = a["d" + k][off:off + size[o]].copy()
            off += size[o]
        out["active"], out["status"] = a["active"], a["status"]
        return out

    def _pcg_probe(self, dw, sigma, v, mode):
        dw = np.ascontiguousarray(dw, np.float64)
        v = np.ascontiguousarray(v, np.float64)
        if len(dw) != self.m or len(v) != self.n:
            raise ValueError("dw needs m entries and v n")
        dwb = np.zeros(max(self.m, 1)); dwb[:self.m] = dw            # (the C side refuses NULL, which an empty array may be)
        vb = np.zeros(max(self.n, 1)); vb[:self.n] = v
        out, info = np.zeros(max(self.n, 1)), np.zeros(PCG_INFO_LEN)
        rc = lib().qpdo_amd_pcg_probe(self._w, _as_dp(dwb), float(sigma), _as_dp(vb), _as_dp(out), mode, _as_dp(info))
        if rc:
            msg = (lib().qpdo_amd_last_error() or b"").decode()
            raise {PCG_NOT_CONVERGED: PcgNotConverged, PCG_NAN: PcgNaN}.get(rc, RuntimeError)("pcg_probe: %s" % msg)
        return out[:self.n].copy(), info

    def pcg_K_product(self, dw, sigma, p):
        """one K product of the PCG path after a fresh build of the compact matrices (qpdo_amd_pcg_probe, mode 0): K p, and a dict with
        kact and the per-workgroup partial sums of p.Kp as the device left them"""
        out, info = self._pcg_probe(dw, sigma, p, 0)
        cnt = int(info[1])
        return out, dict(kact=int(info[0]), cnt=cnt, partials=info[PCG_INFO_HEAD:PCG_INFO_HEAD + cnt].copy())

    def pcg_solve(self, dw, sigma, rhs):
        """one linear solve K x = rhs as a Newton pass of a PCG workspace runs it (qpdo_amd_pcg_probe, mode 1): x and a dict of what ran.
        A capped or stagnated solve raises PcgNotConverged, a NaN residual PcgNaN."""
        out, info = self._pcg_probe(dw, sigma, rhs, 1)
        return out, dict(kact=int(info[0]), iters=int(info[1]), defl_r=int(info[2]), schur=bool(info[3]), rnorm=float(info[4]),
                         bnorm=float(info[5]), inner_solves=int(info[6]), inner_steps=int(info[7]), outer=int(info[9]),
                         diag_from_build=bool(info[10]))

    def pcg_f32_product(self, dw, which, v, x32=False):
        """one product of the slab kernel's fp32-stream instance after a fresh build of the compact matrices (qpdo_amd_pcg_probe, mode 32 / 33):
        which = "Arc": A_c32 v (k values), "Atc": A_c32' v[:k] (n values); v has n entries.  x32: the pair-wide instance with v rounded
        to float32 as well (mode 34 / 35).  Returns the product and k."""
        out, info = self._pcg_probe(dw, 0.0, v, {"Arc": 32, "Atc": 33}[which] + (2 if x32 else 0))
        k = int(info[0])
        return (out[:k].copy() if which == "Arc" else out), k

    def pcg_h16_product(self, dw, which, v):
        """one product of the slab kernel's pair-wide half-precision instance after a fresh build of the compact matrices (qpdo_amd_pcg_probe,
        mode 36 / 37): the values as the half-precision image holds them, v rounded to float32.  Returns the product, k and the exponent e
        of the image's scale 2^e."""
        out, info = self._pcg_probe(dw, 0.0, v, {"Arc": 36, "Atc": 37}[which])
        k = int(info[0])
        return (out[:k].copy() if which == "Arc" else out), k, int(info[1])

    _COMPACT_VECS = {"rowlist": (49, np.int32, "k"), "cidx": (50, np.int32, "m"), "dc": (51, np.float64, "k"),
                     "flag_bits": (52, np.uint64, "words"), "flag_wprefix": (53, np.int32, "words"), "pc_diag": (54, np.float64, "n"),
                     "s_diag": (55, np.float64, "k"), "defl_list": (56, np.int32, "defl_r"), "defl_Sinv": (57, np.float64, None)}

    def _compact_get(self, which, dtype, count):
        out = np.zeros(max(count, 1), dtype)
        if lib().qpdo_amd_download_compact(self._w, which, out.ctypes.data_as(C.c_void_p), count):
            raise RuntimeError("download_compact: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        return out[:count]

    def compact_geometry(self):
        g = self._compact_get(48, np.int64, 5)
        return dict(n=int(g[0]), m=int(g[1]), k=int(g[2]), words=int(g[3]), defl_r=int(g[4]))

    def download_compact_vector(self, name):
        """a vector of the compact index space of the last PCG probe or Newton pass (qpdo_amd_download_compact; defl_Sinv: 256 x 256)"""
        which, dtype, key = self._COMPACT_VECS[name]
        if key is None:
            return self._compact_get(which, dtype, 256 * 256).reshape(256, 256)
        return self._compact_get(which, dtype, self.compact_geometry()[key])

    def download_compact_matrix(self, name):
        """a compact matrix of the last PCG probe or Newton pass -- "Arc" (k x n), "Atc" (n x k), "Ath" (n x k, deflated solves) -- as a
        dict: the geometry, rp, ci, val, and ci16 / sp (None where the matrix has none)"""
        base = 16 * {"Arc": 0, "Atc": 1, "Ath": 2}[name]
        g = self._compact_get(base, np.int64, 7)
        r = dict(nrows=int(g[0]), ncols=int(g[1]), nnz=int(g[2]), use_slab=int(g[3]), nslabs=int(g[4]), W=int(g[5]), has_ci16=int(g[6]))
        r["rp"] = self._compact_get(base + 1, np.int32, r["nrows"] + 1)
        r["ci"] = self._compact_get(base + 2, np.int32, r["nnz"])
        r["val"] = self._compact_get(base + 3, np.float64, r["nnz"])
        r["ci16"] = self._compact_get(base + 4, np.uint16, r["nnz"]) if r["has_ci16"] else None
        r["sp"] = self._compact_get(base + 5, np.int32, r["nrows"] * (r["nslabs"] + 1)).reshape(r["nrows"], r["nslabs"] + 1) if r["use_slab"] else None
        return r

    def download_compact_image(self, name):
        """the slab-major image of "Arc" or "Atc" as the slab kernel streams it (qpdo_amd_download_compact, which >= 64): seg as an
        nrows x nslabs x 2 array of (start, length), vsm, the slab-local indices and vsm16, the half-precision values as float16 (None where
        the image has none); None where the matrix takes the plain kernel.  download_compact_pair_index has the pair-local indices."""
        mat = {"Arc": 0, "Atc": 1}[name]
        g = self._compact_get(16 * mat, np.int64, 7)
        nrows, nnz, use_slab, nslabs, has_ci16 = int(g[0]), int(g[2]), int(g[3]), int(g[4]), int(g[6])
        if not use_slab:
            return None
        base = 64 + 16 * mat
        h16 = self._compact_get(59, np.int64, 2)               # [the images carry half-precision values, the exponent of their scale]
        return dict(vsm16=self._compact_get(base + 3, np.float16, nnz) if h16[0] else None, h16_e=int(h16[1]) if h16[0] else None, seg=self._compact_get(base, np.int32, 2 * nrows * nslabs).reshape(nrows, nslabs, 2),
                    vsm=self._compact_get(base + 1, np.float64, nnz),
                    idx=self._compact_get(base + 2, np.uint16 if has_ci16 else np.int32, nnz))

    def download_compact_pair_index(self, name):
        """the pair-local 16-bit indices of the image of "Arc" or "Atc" (qpdo_amd_download_compact, which 68 / 84): what the pair-wide
        products gather with -- the slab-local index, plus W in the odd slab of a pair; None where the image is not in pair order"""
        mat = {"Arc": 0, "Atc": 1}[name]
        g = self._compact_get(16 * mat, np.int64, 7)
        if not int(g[3]):
            return None
        which, probe = 64 + 16 * mat + 4, np.zeros(1, np.uint16)
        if lib().qpdo_amd_download_compact(self._w, which, probe.ctypes.data_as(C.c_void_p), 0) == 0:
            return None                                       # (the array's length is 0: a count of 0 is accepted only then)
        return self._compact_get(which, np.uint16, int(g[2]))

    def download_linesearch_order(self):
        """the breakpoint indices as the last linesearch's radix sort left them (qpdo_amd_download_compact, which 60)"""
        return self._compact_get(60, np.uint32, 2 * self.m)

    def rebuild_compact_images(self):
        """marks the images of the compact matrices stale and runs one product with each, which rebuilds them from the CSR arrays"""
        self._compact_get(96, np.int32, 0)

    def factor_geometry(self):
        g = np.zeros(4)
        if lib().qpdo_amd_download_factor(self._w, 6, _as_dp(g), 4):
            raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
        return dict(ld=int(g[0]), nb=int(g[1]), np=int(g[2]), b=int(g[3]))

    def download_factor(self, name):
        """a factor array of the last factorization (layouts: include/qpdo_amd_ext.h).  Kd comes back as the ld x ld matrix (element
        (i, j) = Kd[i, j]), Kb / Lt as np x (b + 1) arrays (row j = column / row j of the band), Dg flat, Linv / LinvT as their raw nb x 4096
        arrays.  A band wider than 127 has Wb and Wd instead of Kb and Lt: Wb as (np / 64) x (w + 1) x 64 x 64, w = (b + 63) // 64, where
        Wb[J, s, c, r] is element (r, c) of tile (J + s, J) of the unit-lower L; Wd = D flat."""
        if name in ("coupled_geometry", "coupled_rows", "Z"):
            # band solver with coupling rows (QPDO_BAND_COUPLING): dict(r, k, b_core, np); the r row numbers; Z = B^-1 U as np x k
            g = np.zeros(4)
            if lib().qpdo_amd_download_factor(self._w, 9, _as_dp(g), 4):
                raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
            geo = dict(r=int(g[0]), k=int(g[1]), b_core=int(g[2]), np=int(g[3]))
            if name == "coupled_geometry":
                return geo
            which, count = (10, geo["r"]) if name == "coupled_rows" else (11, geo["np"] * geo["k"])
            out = np.zeros(max(count, 1))
            if lib().qpdo_amd_download_factor(self._w, which, _as_dp(out), count):
                raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
            return out[:count].astype(np.int64) if name == "coupled_rows" else out[:count].reshape(geo["k"], geo["np"]).T
        if name in ("border_geometry", "border_C", "border_Z"):
            # band solver with border variables (QPDO_BAND_BORDER): dict(n_core, c, b_core, np); C = K[:n_core, n_core:] and Z = B^-1 C as np x c
            g = np.zeros(4)
            if lib().qpdo_amd_download_factor(self._w, 13, _as_dp(g), 4):
                raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
            geo = dict(n_core=int(g[0]), c=int(g[1]), b_core=int(g[2]), np=int(g[3]))
            if name == "border_geometry":
                return geo
            count = geo["np"] * geo["c"]
            out = np.zeros(max(count, 1))
            if lib().qpdo_amd_download_factor(self._w, 14 if name == "border_C" else 15, _as_dp(out), count):
                raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
            return out[:count].reshape(geo["c"], geo["np"]).T
        if name == "perm":
            # the band solver's variable order (band_order_config): newold, n integers; Kb / Lt / Wb / Wd are then in that order
            out = np.zeros(max(self.n, 1))
            if lib().qpdo_amd_download_factor(self._w, 12, _as_dp(out), self.n):
                raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
            return out[:self.n].astype(np.int64)
        g = self.factor_geometry()
        ld, nb, npad, b = g["ld"], g["nb"], g["np"], g["b"]
        which, count = {"Kd": (0, ld * ld), "Dg": (1, ld), "Linv": (2, nb * 4096), "LinvT": (3, nb * 4096),
                        "Kb": (4, npad * (b + 1)), "Lt": (5, npad * (b + 1)),
                        "Wb": (7, npad // 64 * ((b + 63) // 64 + 1) * 4096), "Wd": (8, npad)}[name]
        out = np.zeros(count)
        if lib().qpdo_amd_download_factor(self._w, which, _as_dp(out), count):
            raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
        if name == "Kd":
            return out.reshape(ld, ld).T
        if name in ("Kb", "Lt"):
            return out.reshape(npad, b + 1)
        if name == "Wb":
            return out.reshape(npad // 64, (b + 63) // 64 + 1, 64, 64)
        if name in ("Linv", "LinvT"):
            return out.reshape(nb, 4096)
        return out

    def band_order_info(self):
        """what setup decided about the band solver's variable order (QPDOAmdBandOrderInfo): mode, adopted, b_natural / b_ordered (-1 where
        no order was looked at), reason (+ reason_text) where a configured order was not adopted, order_seconds; newold where adopted"""
        info = BandOrderInfo()
        newold = np.zeros(max(self.n, 1), dtype=np.int64 if C.sizeof(C.c_long) == 8 else np.int32)
        if lib().qpdo_amd_get_band_order(self._w, C.byref(info), newold.ctypes.data_as(C.POINTER(C.c_long))):
            raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
        out = {f: getattr(info, f) for f, _ in BandOrderInfo._fields_}
        out["reason_text"] = BAND_ORDER_REASONS.get(int(info.reason), "")
        out["newold"] = newold[:self.n].astype(np.int64) if info.adopted else None
        return out

    def band_border(self):
        """what setup decided about a border of coupling variables (QPDOAmdBandBorderInfo, QPDO_BAND_BORDER): max_border, border (the adopted
        c), n_core, b_core, over (a c that was seen and not adopted), reason (+ reason_text), border_solves"""
        info = BandBorderInfo()
        if lib().qpdo_amd_get_band_border(self._w, C.byref(info)):
            raise RuntimeError((lib().qpdo_amd_last_error() or b"").decode())
        out = {f: int(getattr(info, f)) for f, _ in BandBorderInfo._fields_}
        out["reason_text"] = BAND_BORDER_REASONS.get(out["reason"], "")
        return out

    def download(self, name):
        which, n = {"x": (0, self.n), "Qx": (1, self.n), "y": (2, self.m), "mu": (3, self.m), "d": (4, self.m),
                    "dx": (5, self.n), "dy": (6, self.m), "Ax": (7, self.m), "Aty": (8, self.n),
                    "l": (9, self.m), "u": (10, self.m), "ybar": (11, self.m), "xbar": (12, self.n), "w": (13, self.m)}[name]
        out = np.zeros(n)
        lib().qpdo_amd_download(self._w, which, _as_dp(out))
        return out

    def scaling(self):
        w = self.work
        if not w.scaling:
            return None
        s = w.scaling.contents
        return dict(D=self._vec(s.D, self.n), E=self._vec(s.E, self.m), c=s.c, cinv=s.cinv)

    def delete(self):
        if self._w:
            lib().qpdo_cleanup(self._w)
            self._w = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


def solve_problem(prob, settings=None, **kw):
    """Convenience: prob dict from qpdo_amd.problems -> result dict (+ stats, trace)."""
    s = QPDO().setup(prob["Q"], prob["q"], prob["A"], prob["l"], prob["u"], settings=settings,
                     Qstype=prob.get("Qstype", -1), c=prob.get("c", 0.0), **kw)
    res = s.solve()
    res["stats"], res["trace"] = s.stats(), s.trace()
    s.delete()
    return res


class Batch:
    """Host-side image of a batch of independent QPs for qpdo_amd_solve_batch (ctypes structs + the arrays they point
    to).  Building it is Python/scipy work; `run()` is the C call alone and may be repeated."""

    def __init__(self, probs, indices=None):
        self.keep, self.items, self.outs = [], (BatchItem * len(probs))(), []
        self.probs = probs
        self.indices = list(range(len(probs))) if indices is None else list(indices)   # global item numbers of this shard
        for i, p in enumerate(probs):
            A, Q = sp.csc_matrix(p["A"]), sp.csc_matrix(p["Q"])
            m, n = A.shape
            q = np.ascontiguousarray(p["q"], np.float64)
            l = np.clip(np.ascontiguousarray(p["l"], np.float64), -QPDO_INFTY, QPDO_INFTY)
            u = np.clip(np.ascontiguousarray(p["u"], np.float64), -QPDO_INFTY, QPDO_INFTY)
            Qs, As = _sparse_view(Q, p.get("Qstype", -1), self.keep), _sparse_view(A, 0, self.keep)
            data = QPDOData()
            data.n, data.m, data.Q, data.A = n, m, C.pointer(Qs), C.pointer(As)
            data.q, data.c, data.l, data.u = _as_dp(q), float(p.get("c", 0.0)), _as_dp(l), _as_dp(u)
            x, y = np.zeros(n), np.zeros(m)
            self.keep.extend([q, l, u, Qs, As, data, x, y])
            self.items[i].data = C.pointer(data)
            self.items[i].x0, self.items[i].y0 = None, None
            self.items[i].x, self.items[i].y = _as_dp(x), _as_dp(y)
            self.outs.append((x, y))

    def twin(self):
        """A second host image of the same batch that shares the (read-only) problem data and has its own output buffers: several
        twins of one Batch can be in flight on a BatchStream at once (building an image from scratch is Python / scipy work)."""
        t = Batch.__new__(Batch)
        t.probs, t.indices = self.probs, list(self.indices)
        t.keep, t.items, t.outs = [self], (BatchItem * len(self.outs))(), []
        for i in range(len(self.outs)):
            n, m = len(self.outs[i][0]), len(self.outs[i][1])
            x, y = np.zeros(n), np.zeros(m)
            t.items[i].data = self.items[i].data
            t.items[i].x0, t.items[i].y0 = self.items[i].x0, self.items[i].y0
            t.items[i].x, t.items[i].y = _as_dp(x), _as_dp(y)
            t.outs.append((x, y))
        return t

    def run(self, settings=None, nthreads=16, results=True, **kw):
        """results=False: skip building the per-item dicts (25 ms for 4096 items); the outputs are in info_view() and outs"""
        if settings is None:
            settings = default_settings(**kw)
        failed = lib().qpdo_amd_solve_batch(len(self.outs), self.items, C.byref(settings), int(nthreads))
        self.kernel_seconds = float(lib().qpdo_amd_batch_kernel_seconds())
        return (self.results() if results else None), int(failed)

    def info_view(self):
        """The items' QPDOInfo fields as ONE numpy structured array over the item array itself (no copy, no per-item Python work):
        info_view()["iterations"], ["oterations"], ["status_val"], ["res_prim_norm"] ... -- what a caller that streams batches
        looks at per batch; x and y of item i are self.outs[i] either way.  results() builds the per-item dicts from the same memory."""
        base = BatchItem.info.offset
        names, formats, offsets = [], [], []
        for f, t in QPDOInfo._fields_:
            if f == "status":
                continue
            names.append(f); formats.append(np.dtype(t)); offsets.append(base + getattr(QPDOInfo, f).offset)
        dt = np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(BatchItem)))
        return np.frombuffer(self.items, dtype=dt, count=len(self.outs))

    def results(self):
        """list of dicts (info, x, y) from the items' output fields (after run(), or after BatchStream.wait)"""
        names = [f for f, _ in QPDOInfo._fields_]
        res = []
        for i, (x, y) in enumerate(self.outs):
            inf = self.items[i].info
            info = {f: getattr(inf, f) for f in names}
            info["status"] = info["status"].decode()
            res.append(dict(info=info, x=x.copy(), y=y.copy()))
        return res


class BatchStream:
    """Up to `depth` fused-kernel batches in flight on this process's GPU (qpdo_amd_batch_stream_*): submit() packs, uploads
    and launches a Batch and returns a ticket without waiting for the GPU; wait(ticket) blocks until that batch is complete
    and returns (results, kernel_seconds).  A Batch object may be in flight only once at a time (its items hold the output
    buffers)."""

    def __init__(self, depth=8):
        self._h = lib().qpdo_amd_batch_stream_create(int(depth))
        if not self._h:
            raise RuntimeError("qpdo_amd_batch_stream_create failed")
        self._inflight = {}

    def submit(self, batch, settings=None, **kw):
        if settings is None:
            settings = default_settings(**kw)
        if any(b is batch for b, _ in self._inflight.values()):
            raise ValueError("this Batch is already in flight")
        t = int(lib().qpdo_amd_batch_stream_submit(self._h, len(batch.outs), batch.items, C.byref(settings)))
        if t < 0:
            raise RuntimeError("qpdo_amd_batch_stream_submit failed: " + lib().qpdo_amd_last_error().decode())
        self._inflight[t] = (batch, settings)
        return t

    def wait(self, ticket, results=True):
        """results=False: skip building the per-item dicts (the outputs are in the Batch: info_view(), outs)"""
        batch, _ = self._inflight.pop(ticket)
        ks = C.c_double(0.0)
        if lib().qpdo_amd_batch_stream_wait(self._h, int(ticket), C.byref(ks)) != 0:
            raise RuntimeError("qpdo_amd_batch_stream_wait failed: " + lib().qpdo_amd_last_error().decode())
        batch.kernel_seconds = float(ks.value)
        return (batch.results() if results else None), float(ks.value)

    def close(self):
        if self._h:
            lib().qpdo_amd_batch_stream_destroy(self._h)
            self._h = None
            self._inflight.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_one_hip_runtime = False


def require_one_hip_runtime():
    """A torch wheel bundles its own HIP runtime, and the loader shares it with libqpdo_amd.so only if torch was imported BEFORE the
    library was loaded; the other way round the process holds two runtimes, and a device pointer or stream of one means nothing to the
    other.  The device calls refuse to run in such a process (checked once, from the process's own memory map)."""
    global _one_hip_runtime
    if _one_hip_runtime:
        return
    try:
        with open("/proc/self/maps") as f:
            paths = {os.path.realpath(ln.split()[-1]) for ln in f if "libamdhip64" in ln}
    except OSError:
        paths = set()
    if len(paths) > 1:
        raise RuntimeError("two HIP runtimes are loaded in this process (%s): import torch before the first qpdo_amd call, so that "
                           "libqpdo_amd.so binds to the runtime torch ships (INTEGRATION.md)" % ", ".join(sorted(paths)))
    _one_hip_runtime = True


def check_device_tensor(name, t, device_index, dtype, count):
    """The one check of every tensor a Fleet device call hands to the library, made BEFORE any library call: a GPU tensor on the fleet's
    device, of the dtype named ("float64", "int32", "int64"), contiguous, with `count` elements.  ValueError names the argument.  Returns
    the tensor's address, None for None.  (Reads attributes only: torch itself is imported by the callers.)"""
    if t is None:
        return None
    if not all(hasattr(t, a) for a in ("device", "dtype", "is_contiguous", "numel", "data_ptr")):
        raise ValueError("%s: expected a torch tensor on the GPU, got %s" % (name, type(t).__name__))
    if str(t.dtype) != "torch." + dtype:
        raise ValueError("%s: expected dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: the tensor is not contiguous" % name)
    if t.numel() != count:
        raise ValueError("%s: expected %d elements (the fleet's packed layout), got %d" % (name, count, t.numel()))
    if t.device.type != "cuda":
        raise ValueError("%s: expected a tensor on the GPU, got one on device '%s'" % (name, t.device))
    if t.device.index != device_index:
        raise ValueError("%s: the tensor is on GPU %s, the fleet on GPU %d" % (name, t.device.index, device_index))
    return t.data_ptr()


def _fleet_mat_views(dims, qstype, mats, which):
    """list of `count` scipy matrices (None entries allowed) -> (array of cholmod_sparse pointers or None, what they point into, the views
    by item: header and value array); converted as Batch converts at create.  which: "Q" (n x n, in the item's create-time Qstype storage) or "A" (m x n).
    dims: the items' (n, m); qstype: their create-time Qstype.  Host arithmetic: no fleet, no device."""
    if mats is None:
        return None, [], {}
    count = len(dims)
    if len(mats) != count:
        raise ValueError("%s: expected a list of %d matrices, got %d" % (which, count, len(mats)))
    keep, views, arr = [], {}, (C.POINTER(CholmodSparse) * count)()
    for i, M in enumerate(mats):
        if M is None:
            continue
        n, m = dims[i]
        shape = (n, n) if which == "Q" else (m, n)
        M = sp.csc_matrix(M)
        if M.shape != shape:
            raise ValueError("%s[%d]: expected shape %r, got %r" % (which, i, shape, M.shape))
        view = _sparse_view(M, qstype[i] if which == "Q" else 0, keep)
        views[i] = (view, keep[-1])                          # (the header and the value array its x points to)
        keep.append(view)
        arr[i] = C.pointer(view)
    return arr, keep, views


def pack_matrix_values(dims, qstype, qoff, aoff, Q=None, A=None):
    """Lists of `count` scipy matrices (None entries and None lists allowed, as Fleet.update_matrices takes them) -> (Q_values, A_values,
    mask): the float64 arrays of the packed value layout (qoff / aoff: count + 1 offsets each, the last one the total; None for a None
    list) and the int32 mask those lists imply, bit 0 = the item has a Q entry, bit 1 = an A entry.  Every matrix goes through the
    conversion the host call hands to the library (_fleet_mat_views), and the values are read from THAT header: their order is the
    create-time one by construction.  Items without an entry keep zeros.  A function of the problems' host images: no fleet, no device."""
    count = len(dims)
    mask = np.zeros(count, np.int32)
    out = []
    for which, mats, off, bit in (("Q", Q, qoff, 1), ("A", A, aoff, 2)):
        _, _, views = _fleet_mat_views(dims, qstype, mats, which)
        if mats is None:
            out.append(None)
            continue
        vals = np.zeros(int(off[count]), np.float64)
        for i, (_, x) in views.items():
            nnz = int(off[i + 1] - off[i])
            if len(x) != nnz:
                raise ValueError("%s[%d]: %d stored entries, the pattern at create has %d" % (which, i, len(x), nnz))
            vals[int(off[i]):int(off[i + 1])] = x
            mask[i] |= bit
        out.append(vals)
    return out[0], out[1], mask


class Fleet:
    """A resident fleet of small QPs (qpdo_amd_fleet_*): set up once, then per control step update() / warm_start_last() / solve(), one
    launch each for all items.  Item i carries the bits of a QPDO workspace of its own driven through the same calls.  The settings are
    fixed at construction.  matrix_updates=True (QPDO_AMD_FLEET_MATRIX_UPDATES) also allows update_matrices(): new Q / A values per item;
    adjoint=True (QPDO_AMD_FLEET_ADJOINT) allows adjoint_device(): gradients of the last solve (qpdo_amd/torch_layer.py builds on it)."""

    def __init__(self, probs, settings=None, matrix_updates=False, adjoint=False, **kw):
        self._h = None
        if settings is None:
            settings = default_settings(**kw)
        elif kw:
            for k, v in kw.items():
                if not hasattr(settings, k):
                    raise KeyError("unrecognized solver setting '%s'" % k)
                setattr(settings, k, v)
        img = Batch(probs)                                   # the host image of the data; the library copies what it needs
        self.count = len(probs)
        self.dims = [(len(x), len(y)) for x, y in img.outs]
        arr = (C.POINTER(QPDOData) * max(1, self.count))(*[img.items[i].data for i in range(self.count)])
        self._qstype = [int(p.get("Qstype", -1)) for p in probs]
        if matrix_updates or adjoint:
            flags = (FLEET_MATRIX_UPDATES if matrix_updates else 0) | (FLEET_ADJOINT if adjoint else 0)
            h = lib().qpdo_amd_fleet_create_ex(self.count, arr, C.byref(settings), flags)
        else:
            h = lib().qpdo_amd_fleet_create(self.count, arr, C.byref(settings))
        if not h:
            raise RuntimeError("Fleet: %s" % (lib().qpdo_amd_last_error() or b"").decode())
        self._h = h
        self._outs = [(np.zeros(n), np.zeros(m)) for n, m in self.dims]
        self._xp = (dp * self.count)(*[_as_dp(x) for x, _ in self._outs])
        self._yp = (dp * self.count)(*[_as_dp(y) for _, y in self._outs])
        self._info = (QPDOInfo * self.count)()
        self.kernel_seconds = 0.0
        self._layout, self._device, self._dev_out = None, None, None     # (the device calls: filled on first use)
        self._mlayout = None
        self._adj_out = None
        self.solve_serial = 0                                # solve()/solve_device() calls so far (FleetQP: is a backward still current?)

    def _ptrs(self, vecs, which, clip=False):
        """list of `count` vectors (None entries allowed) -> (array of pointers or None, the arrays kept alive)"""
        if vecs is None:
            return None, []
        if len(vecs) != self.count:
            raise ValueError("%s: expected a list of %d vectors, got %d" % (which[0], self.count, len(vecs)))
        keep, arr = [], (dp * self.count)()
        for i, v in enumerate(vecs):
            if v is None:
                continue
            v = np.ascontiguousarray(v, np.float64)
            if v.shape != (self.dims[i][which[1]],):
                raise ValueError("%s[%d]: expected shape (%d,), got %r" % (which[0], i, self.dims[i][which[1]], v.shape))
            if clip:
                v = np.clip(v, -QPDO_INFTY, QPDO_INFTY)     # qpdo.m:215-216
            keep.append(v)
            arr[i] = _as_dp(v)
        return arr, keep

    def _call(self, rc, what):
        if rc:
            raise RuntimeError("Fleet.%s: %s" % (what, (lib().qpdo_amd_last_error() or b"").decode()))

    def update(self, q=None, l=None, u=None):
        """new q / l / u per item (lists of length count; None entries and None lists: unchanged).  Bounds first, then q."""
        qa, k1 = self._ptrs(q, ("q", 0))
        la, k2 = self._ptrs(l, ("l", 1), clip=True)
        ua, k3 = self._ptrs(u, ("u", 1), clip=True)
        self._call(lib().qpdo_amd_fleet_update(self._h, qa, la, ua), "update")

    def _mat_ptrs(self, mats, which):
        """list of `count` scipy matrices (None entries allowed) -> (array of cholmod_sparse pointers or None, what they point into); converted
        as Batch converts at create.  which: "Q" (n x n, in the item's create-time Qstype storage) or "A" (m x n)"""
        arr, keep, _ = _fleet_mat_views(self.dims, self._qstype, mats, which)
        return arr, keep

    def update_matrices(self, Q=None, A=None):
        """new VALUES of Q / A per item in the create-time pattern (lists of length count of scipy matrices; None entries and None lists:
        unchanged).  An item with an entry becomes the workspace qpdo_setup leaves for its new matrices and its latest q, l, u; the others
        are not touched.  Needs matrix_updates=True at construction."""
        Qa, k1 = self._mat_ptrs(Q, "Q")
        Aa, k2 = self._mat_ptrs(A, "A")
        self._call(lib().qpdo_amd_fleet_update_matrices(self._h, Qa, Aa), "update_matrices")

    def matrix_stats(self):
        s = FleetMatrixStats()
        self._call(lib().qpdo_amd_fleet_get_matrix_stats(self._h, C.byref(s)), "matrix_stats")
        return {f: getattr(s, f) for f, _ in FleetMatrixStats._fields_}

    def warm_start(self, x=None, y=None):
        xa, k1 = self._ptrs(x, ("x", 0))
        ya, k2 = self._ptrs(y, ("y", 1))
        self._call(lib().qpdo_amd_fleet_warm_start(self._h, xa, ya), "warm_start")

    def warm_start_last(self):
        self._call(lib().qpdo_amd_fleet_warm_start_last(self._h), "warm_start_last")

    def solve(self, results=True):
        """results=False: skip building the per-item dicts; the outputs are in info_view() and outs"""
        self._call(lib().qpdo_amd_fleet_solve(self._h, self._xp, self._yp, self._info), "solve")
        self.solve_serial = getattr(self, "solve_serial", 0) + 1
        self.kernel_seconds = self.stats()["last_kernel_seconds"]
        return self.results() if results else None

    @property
    def outs(self):
        return self._outs

    def info_view(self):
        names, formats, offsets = [], [], []
        for f, t in QPDOInfo._fields_:
            if f == "status":
                continue
            names.append(f); formats.append(np.dtype(t)); offsets.append(getattr(QPDOInfo, f).offset)
        dt = np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(QPDOInfo)))
        return np.frombuffer(self._info, dtype=dt, count=self.count)

    def results(self):
        """the per-item dicts of Batch.results() (info, x, y) plus the certificates QPDO.solve() returns (NaN unless the status is -3 / -4)"""
        names = [f for f, _ in QPDOInfo._fields_]
        res = []
        for i, (x, y) in enumerate(self._outs):
            info = {f: getattr(self._info[i], f) for f in names}
            info["status"] = info["status"].decode()
            n, m = self.dims[i]
            r = dict(info=info, x=x.copy(), y=y.copy(), prim_inf_cert=np.full(m, np.nan), dual_inf_cert=np.full(n, np.nan))
            if info["status_val"] in (-3, -4):
                pc, dc = np.zeros(m), np.zeros(n)
                self._call(lib().qpdo_amd_fleet_get_certificates(self._h, i, _as_dp(pc), _as_dp(dc)), "results")
                if info["status_val"] == -3:
                    r["prim_inf_cert"] = pc
                else:
                    r["dual_inf_cert"] = dc
            res.append(r)
        return res

    # ---- device arrays on the caller's stream (qpdo_amd_fleet_*_dev): torch tensors in, torch tensors out, no host wait ----------------
    def packed_layout(self):
        """(noff, moff), count + 1 entries each: item i's n-vector is [noff[i], noff[i + 1]) of a packed n-array, its m-vector
        [moff[i], moff[i + 1]) of a packed m-array; the last entries are the totals N and M"""
        if getattr(self, "_layout", None) is None:
            no, mo = (C.c_long * (self.count + 1))(), (C.c_long * (self.count + 1))()
            self._call(lib().qpdo_amd_fleet_get_packed_layout(self._h, no, mo), "packed_layout")
            self._layout = (np.array(no[:], np.int64), np.array(mo[:], np.int64))
            self._device = int(lib().qpdo_amd_fleet_device(self._h))
        return self._layout

    def _dev_args(self, pairs, mask):
        """[(name, tensor, dtype, count)] (+ the optional int32 mask) -> addresses, after every tensor has passed check_device_tensor"""
        self.packed_layout()
        ptrs = [check_device_tensor(nm, t, self._device, dt, cnt) for nm, t, dt, cnt in pairs]
        return ptrs, check_device_tensor("mask", mask, self._device, "int32", self.count)

    def _stream(self):
        import torch
        require_one_hip_runtime()
        return torch.cuda.current_stream(self._device).cuda_stream

    def update_device(self, q=None, l=None, u=None, mask=None):
        """update() from packed GPU tensors on torch's current stream; returns without waiting.  q: N float64, l / u: M float64 (clamped to
        +-1e20 as update() clips), mask: count int32, bit 0 / 1 / 2 = the item takes q / l / u.  An item that takes l and u with l > u
        somewhere is left untouched and counted (sync()); the others proceed."""
        import torch
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        (qp, _, _), mp = self._dev_args([("q", q, "float64", N), ("l", l, "float64", M), ("u", u, "float64", M)], mask)
        # qpdo.m:215-216.  The clamped copies are made on the current stream and read by launches on it: torch's allocator reuses their
        # memory only for work that the same stream runs afterwards
        l = None if l is None else torch.clamp(l, -QPDO_INFTY, QPDO_INFTY)
        u = None if u is None else torch.clamp(u, -QPDO_INFTY, QPDO_INFTY)
        lp, up = (None if l is None else l.data_ptr()), (None if u is None else u.data_ptr())
        self._call(lib().qpdo_amd_fleet_update_dev(self._h, qp, lp, up, mp, N, M, self._stream()), "update_device")

    def packed_matrix_layout(self):
        """(qoff, aoff), count + 1 entries each: item i's stored Q values are [qoff[i], qoff[i + 1]) of a packed Q-value array, its CSC A
        values [aoff[i], aoff[i + 1]) of a packed A-value array; the last entries are the totals NQ and NA.  Needs matrix_updates=True."""
        if getattr(self, "_mlayout", None) is None:
            qo, ao = (C.c_long * (self.count + 1))(), (C.c_long * (self.count + 1))()
            self._call(lib().qpdo_amd_fleet_get_packed_matrix_layout(self._h, qo, ao), "packed_matrix_layout")
            self._mlayout = (np.array(qo[:], np.int64), np.array(ao[:], np.int64))
        return self._mlayout

    def pack_matrix_values(self, Q=None, A=None):
        """lists of scipy matrices as update_matrices() takes them -> (Q_values, A_values, mask): two float64 numpy arrays in the packed
        value layout (None for a None list; zeros where an item has no entry) and the int32 mask the lists imply.  Move them to the GPU
        for update_matrices_device(); packing matrices whose values are their own indices (0, 1, 2, ...) gives the index map from a
        caller's ordering to the packed one."""
        qoff, aoff = self.packed_matrix_layout()
        return pack_matrix_values(self.dims, self._qstype, qoff, aoff, Q, A)

    def update_matrices_device(self, Q_values=None, A_values=None, mask=None):
        """update_matrices() from packed GPU tensors on torch's current stream; returns without waiting.  Q_values: NQ float64, A_values: NA
        float64 (packed_matrix_layout(); values only, the pattern is the create-time one), mask: count int32, bit 0 / 1 = the item takes
        Q / A.  None: that matrix is unchanged for every item.  Needs matrix_updates=True."""
        qoff, aoff = self.packed_matrix_layout()
        NQ, NA = int(qoff[-1]), int(aoff[-1])
        (qp, ap), mp = self._dev_args([("Q_values", Q_values, "float64", NQ), ("A_values", A_values, "float64", NA)], mask)
        self._call(lib().qpdo_amd_fleet_update_matrices_dev(self._h, qp, ap, mp, NQ, NA, self._stream()), "update_matrices_device")

    def warm_start_device(self, x=None, y=None, mask=None):
        """warm_start() from packed GPU tensors (x: N, y: M float64; mask bit 0 / 1 = the item takes x / y, else starts it from zero)"""
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        (xp, yp), mp = self._dev_args([("x", x, "float64", N), ("y", y, "float64", M)], mask)
        self._call(lib().qpdo_amd_fleet_warm_start_dev(self._h, xp, yp, mp, N, M, self._stream()), "warm_start_device")

    def warm_start_last_device(self):
        self.packed_layout()
        self._call(lib().qpdo_amd_fleet_warm_start_last_dev(self._h, self._stream()), "warm_start_last_device")

    def solve_device(self, out=None):
        """solve() on torch's current stream into GPU tensors; returns them without waiting: x (N), y (M), status (count, 3) int64 =
        status_val, iterations, oterations, norms (count, 5) = the four residual norms and the objective, prim_inf_cert (M),
        dual_inf_cert (N); NaN rules of results().  The tensors are allocated once and reused by later calls unless `out` (a dict with
        any of these keys) supplies them."""
        import torch
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        spec = [("x", "float64", (N,)), ("y", "float64", (M,)), ("status", "int64", (self.count, 3)), ("norms", "float64", (self.count, 5)),
                ("prim_inf_cert", "float64", (M,)), ("dual_inf_cert", "float64", (N,))]
        if out is None:
            if getattr(self, "_dev_out", None) is None:
                dev = torch.device("cuda", self._device)
                self._dev_out = {k: torch.empty(shape, dtype=getattr(torch, dt), device=dev) for k, dt, shape in spec}
            out = self._dev_out
        unknown = set(out) - {k for k, _, _ in spec}
        if unknown:
            raise ValueError("out: unknown keys %r" % sorted(unknown))
        ptrs, _ = self._dev_args([(k, out.get(k), dt, int(np.prod(shape))) for k, dt, shape in spec], None)
        self._call(lib().qpdo_amd_fleet_solve_dev(self._h, *ptrs, N, M, self._stream()), "solve_device")
        self.solve_serial = getattr(self, "solve_serial", 0) + 1
        return out

    def adjoint_device(self, gx, gy=None, matrices=False, out=None, tol=1e-9, max_sweeps=20):
        """The adjoint of the last solve (qpdo_amd_fleet_adjoint_dev) on torch's current stream; returns without waiting.  gx: N float64 =
        dL/dx, gy: M float64 = dL/dy or None (zero; entries of inactive rows are ignored).  Returns a dict of GPU tensors: dq (N), dl, du
        (M), dQ_values (NQ) / dA_values (NA) in the packed value layout (None unless matrices=True, which needs matrix_updates=True),
        active (M int32: +1 upper-active, -1 lower-active, 0), status (count, 3) int64 = code, sweeps, active rows (code 0 accepted,
        1 not accepted, 2 the item is not solved, 3 bad pivot), residual (count) = the accepted relative residual.  An item with code != 0
        has NaN in all its slices.  The tensors are allocated once and reused unless `out` (a dict with any of these keys) supplies
        them.  Needs adjoint=True, and the most recent update / warm start / solve call of the fleet must be a solve."""
        import torch
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        NQ = NA = 0
        if matrices:
            qoff, aoff = self.packed_matrix_layout()
            NQ, NA = int(qoff[-1]), int(aoff[-1])
        spec = [("dq", "float64", (N,)), ("dl", "float64", (M,)), ("du", "float64", (M,)), ("dQ_values", "float64", (NQ,)), ("dA_values", "float64", (NA,)),
                ("active", "int32", (M,)), ("status", "int64", (self.count, 3)), ("residual", "float64", (self.count,))]
        (gxp, gyp), _ = self._dev_args([("gx", gx, "float64", N), ("gy", gy, "float64", M)], None)
        if gx is None:
            raise ValueError("gx: expected a tensor, got None")
        if out is None:
            if getattr(self, "_adj_out", None) is None or (matrices and self._adj_out["dQ_values"] is None):
                dev = torch.device("cuda", self._device)
                self._adj_out = {k: (None if k in ("dQ_values", "dA_values") and not matrices else torch.empty(shape, dtype=getattr(torch, dt), device=dev))
                                 for k, dt, shape in spec}
            out = dict(self._adj_out)
            if not matrices:
                out["dQ_values"] = out["dA_values"] = None
        else:
            unknown = set(out) - {k for k, _, _ in spec}
            if unknown:
                raise ValueError("out: unknown keys %r" % sorted(unknown))
            out = {k: out.get(k) for k, _, _ in spec}
            if not matrices:
                out["dQ_values"] = out["dA_values"] = None
        for k in ("dq", "dl", "du") + (("dQ_values", "dA_values") if matrices else ()):
            if out[k] is None:
                raise ValueError("out: '%s' is needed" % k)
        ptrs, _ = self._dev_args([(k, out[k], dt, int(np.prod(shape))) for k, dt, shape in spec], None)
        self._call(lib().qpdo_amd_fleet_adjoint_dev(self._h, gxp, gyp, *ptrs, float(tol), int(max_sweeps), N, M, NQ, NA, self._stream()), "adjoint_device")
        return out

    def adjoint_stats(self):
        """adjoint_calls: adjoint_device calls that launched, since create; resident_extra_bytes: what adjoint=True holds on the device (0)"""
        s = FleetAdjointStats()
        self._call(lib().qpdo_amd_fleet_get_adjoint_stats(self._h, C.byref(s)), "adjoint_stats")
        return {f: getattr(s, f) for f, _ in FleetAdjointStats._fields_}

    # ---- many right-hand sides per factorization (qpdo_amd_fleet_adjoint_multi_dev, qpdo_amd_fleet_tangent_dev) --------------------------
    def _sens_out(self, spec, out, needed, cache):
        """the output tensors of a sensitivity call: `out` (a dict with any of spec's keys), or ONE set per call kind (`cache`), kept for the
        most recent shapes only and reused while they stay the same -- a caller who changes R gets new tensors and the old set is dropped"""
        import torch
        if out is None:
            store = getattr(self, "_sens_cache", None)
            if store is None:
                store = self._sens_cache = {}
            key = tuple((k, shape) for k, _, shape in spec)
            if store.get(cache, (None, None))[0] != key:
                dev = torch.device("cuda", self._device)
                store[cache] = (key, {k: (None if shape is None else torch.empty(shape, dtype=getattr(torch, dt), device=dev)) for k, dt, shape in spec})
            return dict(store[cache][1])
        unknown = set(out) - {k for k, _, _ in spec}
        if unknown:
            raise ValueError("out: unknown keys %r" % sorted(unknown))
        out = {k: (None if shape is None else out.get(k)) for k, _, shape in spec}
        for k in needed:
            if out[k] is None:
                raise ValueError("out: '%s' is needed" % k)
        return out

    def adjoint_many_device(self, gx, gy=None, matrices=False, out=None, tol=1e-9, max_sweeps=20):
        """R adjoints of the last solve from ONE classification, assembly and factorization per item (qpdo_amd_fleet_adjoint_multi_dev) on
        torch's current stream; returns without waiting.  gx: (R, N) float64, gy: (R, M) float64 or None.  Returns what adjoint_device
        returns with a leading R on dq, dl, du, dQ_values, dA_values, status (R, count, 3) and residual (R, count); active (M) is one array,
        the flags being the solve's.  Slab r carries the bits of adjoint_device(gx[r], gy[r]).  Needs adjoint=True (matrices=True also
        matrix_updates=True), and the most recent update / warm start / solve call of the fleet must be a solve."""
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        if gx is None:
            raise ValueError("gx: expected a tensor, got None")
        if not hasattr(gx, "dim") or gx.dim() != 2:
            raise ValueError("gx: expected a tensor of shape (R, %d)" % N)
        R = int(gx.shape[0])
        if R < 1:
            raise ValueError("gx: expected at least one right-hand side, got shape %r" % (tuple(gx.shape),))
        NQ = NA = 0
        if matrices:
            qoff, aoff = self.packed_matrix_layout()
            NQ, NA = int(qoff[-1]), int(aoff[-1])
        spec = [("dq", "float64", (R, N)), ("dl", "float64", (R, M)), ("du", "float64", (R, M)), ("dQ_values", "float64", (R, NQ) if matrices else None),
                ("dA_values", "float64", (R, NA) if matrices else None), ("active", "int32", (M,)), ("status", "int64", (R, self.count, 3)),
                ("residual", "float64", (R, self.count))]
        (gxp, gyp), _ = self._dev_args([("gx", gx, "float64", R * N), ("gy", gy, "float64", R * M)], None)
        out = self._sens_out(spec, out, ("dq", "dl", "du") + (("dQ_values", "dA_values") if matrices else ()), "adjoint_many")
        ptrs, _ = self._dev_args([(k, out[k], dt, 0 if shape is None else int(np.prod(shape))) for k, dt, shape in spec], None)
        self._call(lib().qpdo_amd_fleet_adjoint_multi_dev(self._h, R, gxp, gyp, *ptrs, float(tol), int(max_sweeps), N, M, NQ, NA, self._stream()), "adjoint_many_device")
        return out

    def tangent_device(self, tq=None, tl=None, tu=None, tQ_values=None, tA_values=None, out=None, tol=1e-9, max_sweeps=20):
        """The tangent of the last solve (qpdo_amd_fleet_tangent_dev) on torch's current stream; returns without waiting: the first-order
        change (dx, dy) of the solution for a change tq (N), tl, tu (M), tQ_values (NQ), tA_values (NA) of the fleet's data at the solve's
        active set.  Every passed array is (L,) or (R, L) float64 and all must agree on R; None is a zero perturbation (not all five).
        Entries of tl, tu, tA_values on rows that do not use them are ignored.  A stype-0 Q takes a symmetric tQ.  Returns a dict of GPU
        tensors with the leading R where the inputs had one: dx (N), dy (M; +0.0 off the active rows), active (M int32), status (count, 3)
        int64 = code, sweeps, active rows, residual (count).  A right-hand side with code != 0 has NaN in its slices of dx, dy.  Needs
        adjoint=True (tQ_values / tA_values also matrix_updates=True), and the most recent state-changing call must be a solve."""
        (no, mo) = self.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        NQ = NA = 0
        if tQ_values is not None or tA_values is not None:
            qoff, aoff = self.packed_matrix_layout()
            NQ, NA = int(qoff[-1]), int(aoff[-1])
        ins = [("tq", tq, N), ("tl", tl, M), ("tu", tu, M), ("tQ_values", tQ_values, NQ), ("tA_values", tA_values, NA)]
        passed = [(nm, t) for nm, t, _ in ins if t is not None]
        if not passed:
            raise ValueError("no tangent passed: tq, tl, tu, tQ_values and tA_values are all None")
        for nm, t in passed:
            if not hasattr(t, "dim") or t.dim() not in (1, 2):
                raise ValueError("%s: expected a tensor of shape (L,) or (R, L)" % nm)
        dims = {t.dim() for _, t in passed}
        Rs = {int(t.shape[0]) if t.dim() == 2 else 1 for _, t in passed}
        if len(dims) != 1 or len(Rs) != 1:
            raise ValueError("the passed tangents do not agree on R: %s" % ", ".join("%s %r" % (nm, tuple(t.shape)) for nm, t in passed))
        lead, R = dims == {2}, Rs.pop()
        if R < 1:
            raise ValueError("%s: expected at least one right-hand side" % passed[0][0])
        sh = (lambda *s: (R,) + s) if lead else (lambda *s: s)
        spec = [("dx", "float64", sh(N)), ("dy", "float64", sh(M)), ("active", "int32", (M,)), ("status", "int64", sh(self.count, 3)),
                ("residual", "float64", sh(self.count))]
        inp, _ = self._dev_args([(nm, t, "float64", R * L) for nm, t, L in ins], None)
        out = self._sens_out(spec, out, ("dx", "dy"), "tangent")
        ptrs, _ = self._dev_args([(k, out[k], dt, int(np.prod(shape))) for k, dt, shape in spec], None)
        self._call(lib().qpdo_amd_fleet_tangent_dev(self._h, R, *inp, *ptrs, float(tol), int(max_sweeps), N, M, NQ, NA, self._stream()), "tangent_device")
        return out

    def rhs_group(self):
        """right-hand sides one workgroup carries at once in adjoint_many_device / tangent_device (1: one after another)"""
        return int(lib().qpdo_amd_fleet_rhs_group(self._h))

    def sensitivity_stats(self):
        """calls: adjoint_many_device + tangent_device calls that launched, since create; rhs_total: their right-hand sides; scratch_bytes"""
        s = FleetSensitivityStats()
        self._call(lib().qpdo_amd_fleet_get_sensitivity_stats(self._h, C.byref(s)), "sensitivity_stats")
        return {f: getattr(s, f) for f, _ in FleetSensitivityStats._fields_}

    def fetch_last(self):
        """what results() returns, for the last solve whichever call launched it (waits for it; launches nothing)"""
        self._call(lib().qpdo_amd_fleet_fetch_last(self._h, self._xp, self._yp, self._info), "fetch_last")
        self.kernel_seconds = self.stats()["last_kernel_seconds"]
        return self.results()

    def sync(self):
        """waits for everything this fleet was asked to do; the device-call counters and the refusal record since the last sync()"""
        s = FleetDevStats()
        self._call(lib().qpdo_amd_fleet_sync(self._h, C.byref(s)), "sync")
        return {f: getattr(s, f) for f, _ in FleetDevStats._fields_}

    def factor_layout(self):
        """where this fleet's launches keep the Newton matrix: K_GLOBAL, K_PACKED or K_BAND (qpdo_amd_fleet_factor_layout)"""
        return int(lib().qpdo_amd_fleet_factor_layout(self._h))

    def stats(self):
        s = FleetStats()
        self._call(lib().qpdo_amd_fleet_get_stats(self._h, C.byref(s)), "stats")
        return {f: getattr(s, f) for f, _ in FleetStats._fields_}

    def close(self):
        if self._h:
            lib().qpdo_amd_fleet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_indices(count, rank, world):
    """Items of a batch of `count` independent QPs owned by `rank` of `world` processes (one per GPU): item b goes to
    GPU b mod world.  Disjoint, complete and order-stable; no data-path collective."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("rank %r not in [0, %r)" % (rank, world))
    return list(range(rank, count, world))


def shard_batch(count, rank, world, make_problem):
    """Batch of this rank's items only: make_problem(i) is called for the owned global indices."""
    idx = shard_indices(count, rank, world)
    return Batch([make_problem(i) for i in idx], indices=idx)


def merge_shards(count, shards):
    """shards: iterable of (indices, results) as returned per rank -> list of `count` results in global order."""
    out = [None] * count
    for idx, res in shards:
        for i, r in zip(idx, res):
            if out[i] is not None:
                raise ValueError("item %d solved twice" % i)
            out[i] = r
    missing = [i for i, r in enumerate(out) if r is None]
    if missing:
        raise ValueError("items not solved: %r" % missing[:8])
    return out


def solve_batch(probs, settings=None, nthreads=16, **kw):
    """Solve independent QPs (dicts from qpdo_amd.problems) concurrently on this process's GPU.
    Returns a list of dicts (info, x, y) and the number of failed items."""
    return Batch(probs).run(settings, nthreads, **kw)


def small_factor_layout(probs, kind, settings=None, **kw):
    """(layout, [half-bandwidth of every item]) of a fused-kernel launch over `probs`: K_GLOBAL, K_PACKED or K_BAND, or -1 when an item
    does not fit the fused kernel.  kind: KIND_BATCH (solve_batch), KIND_STREAM (a batch of a BatchStream), KIND_FLEET.  Host arithmetic
    by the function the launches go through (qpdo_amd_small_factor_layout); needs no device."""
    if settings is None:
        settings = default_settings(**kw)
    img = Batch(probs)
    n = len(probs)
    arr = (C.POINTER(QPDOData) * max(1, n))(*[img.items[i].data for i in range(n)])
    bw = (C.c_long * max(1, n))()
    lay = int(lib().qpdo_amd_small_factor_layout(n, arr, C.byref(settings), int(kind), bw))
    return lay, [int(bw[i]) for i in range(n)]


def batch_factor_layout():
    """the layout the last solve_batch of this process took (qpdo_amd_batch_factor_layout); -1: none yet through the fused kernel"""
    return int(lib().qpdo_amd_batch_factor_layout())


# ---- one large QP row-partitioned over the ranks of a torch.distributed job ---------------------------------
ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_long, C.c_int)
_dist_keep = []


def band_order_config(mode, newold=None):
    """The band solver's variable order for the workspaces set up next in this process (qpdo_amd_band_order_config): mode "env" (the default:
    QPDO_BAND_ORDER decides), "natural", "rcm", or "given" with newold -- newold[k] = the caller's index of the variable at position k."""
    code = {"env": BAND_ORDER_ENV, "natural": BAND_ORDER_NATURAL, "rcm": BAND_ORDER_RCM, "given": BAND_ORDER_GIVEN}.get(mode, mode)
    if code not in (BAND_ORDER_ENV, BAND_ORDER_NATURAL, BAND_ORDER_RCM, BAND_ORDER_GIVEN):
        raise ValueError("unknown band order mode %r" % (mode,))
    arr, n = None, 0
    if code == BAND_ORDER_GIVEN:
        if newold is None:
            raise ValueError("mode 'given' needs newold")
        arr = np.ascontiguousarray(newold, dtype=np.int64 if C.sizeof(C.c_long) == 8 else np.int32)
        n = len(arr)
        if not np.array_equal(np.sort(arr), np.arange(n)):
            raise ValueError("newold is not a permutation of 0 .. n-1")
    if lib().qpdo_amd_band_order_config(code, None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_long)), n):
        raise ValueError("qpdo_amd_band_order_config refused the order")


def band_order(Q, A, Qstype=-1):
    """Reverse Cuthill-McKee on the pattern of Q + A'A (qpdo_amd_band_order; host only, no device): (newold, info) with newold[k] = the
    index of the variable that takes position k and info = dict(b_natural, b_ordered, components, early_out).  Q as setup takes it: a
    stored triangle with Qstype -1 / +1, or both triangles with 0.  problems.permute_variables(prob, newold) is the reordered QP."""
    keep = []
    Q = sp.csc_matrix(Q)
    n = Q.shape[0]
    A = sp.csc_matrix((0, n)) if A is None else sp.csc_matrix(A)
    qv, av = _sparse_view(Q, int(Qstype), keep), _sparse_view(A, 0, keep)
    ltype = np.int64 if C.sizeof(C.c_long) == 8 else np.int32
    newold, info = np.zeros(max(n, 1), dtype=ltype), np.zeros(4, dtype=ltype)
    lp_ = C.POINTER(C.c_long)
    if lib().qpdo_amd_band_order(C.byref(qv), C.byref(av), newold.ctypes.data_as(lp_), info.ctypes.data_as(lp_)):
        raise RuntimeError("qpdo_amd_band_order failed")
    return newold[:n].astype(np.int64), dict(b_natural=int(info[0]), b_ordered=int(info[1]), components=int(info[2]), early_out=int(info[3]))


def band_border(Q, A, max_border=64, Qstype=-1):
    """The detection of a border of coupling variables over a band core (qpdo_amd_band_border; host only, no device): dict(n_core, c,
    b_core, reason) -- the trailing c = n - n_core variables reach beyond half-bandwidth 127, the rest has half-bandwidth b_core; reason 1
    when c > max_border.  Q as setup takes it (band_order above).  The border variables are the trailing ones: number shared variables
    last (problems.permute_variables)."""
    keep = []
    Q = sp.csc_matrix(Q)
    n = Q.shape[0]
    A = sp.csc_matrix((0, n)) if A is None else sp.csc_matrix(A)
    qv, av = _sparse_view(Q, int(Qstype), keep), _sparse_view(A, 0, keep)
    info = np.zeros(4, dtype=np.int64 if C.sizeof(C.c_long) == 8 else np.int32)
    if lib().qpdo_amd_band_border(C.byref(qv), C.byref(av), int(max_border), info.ctypes.data_as(C.POINTER(C.c_long))):
        raise RuntimeError("qpdo_amd_band_border failed")
    return dict(n_core=int(info[0]), c=int(info[1]), b_core=int(info[2]), reason=int(info[3]))


def dist_config(rank, world, mode="rccl", group=None, force=False):
    """Partition the rows of A over `world` ranks for the workspaces created next in this process.
    mode 'rccl': all-reduce with RCCL on the solver stream (one GPU per rank); the unique id is created by rank 0
    and broadcast over torch.distributed.  mode 'host': all-reduce through torch.distributed on host buffers
    (gloo) - slow, for tests of the partition logic on a single GPU."""
    L = lib()
    if world <= 1 and force and mode == "rccl":
        # a single-rank RCCL communicator: the partition is the whole problem, but every collective call site of the
        # row-partitioned solver runs through ncclAllReduce on the solver's stream (tests of the RCCL branch on one GPU)
        uid = C.create_string_buffer(128)
        if L.qpdo_amd_dist_unique_id(uid) != 0:
            raise RuntimeError("ncclGetUniqueId failed")
        _dist_keep.append(uid)
        return L.qpdo_amd_dist_config(0, 1, C.cast(uid, C.c_void_p), None, None)
    if world <= 1:
        return L.qpdo_amd_dist_config(0, 1, None, None, None)
    import torch
    import torch.distributed as dist
    if mode == "host":
        def _cb(ctx, buf, count, op):
            a = np.ctypeslib.as_array(buf, shape=(count,))
            t = torch.from_numpy(a)
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)
        fn = ALLREDUCE_FN(_cb)
        _dist_keep.append(fn)
        return L.qpdo_amd_dist_config(rank, world, None, C.cast(fn, C.c_void_p), None)
    uid = C.create_string_buffer(128)
    if rank == 0:
        if L.qpdo_amd_dist_unique_id(uid) != 0:
            raise RuntimeError("ncclGetUniqueId failed")
    box = [bytes(uid.raw)]
    dist.broadcast_object_list(box, src=0, group=group)
    uid = C.create_string_buffer(box[0], 128)
    _dist_keep.append(uid)
    return L.qpdo_amd_dist_config(rank, world, C.cast(uid, C.c_void_p), None, None)
