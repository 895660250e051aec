"""The workspace tangent (qpdo_amd_tangent, include/qpdo_amd_ext.h) where no device is needed: every argument check that comes before the
backend is touched, by message and in the header's order, from a compiled C program (tests/tangent_args_driver.c), plain and with the
host driver under AddressSanitizer + UBSan; the symbols and the layout of the stats; solver.QPDO.tangent validates shapes and dtypes before
any library call; and the sign convention the GPU test's "one sweep driver" check leans on, in the longdouble references, on the n = 40
problem of tests/test_gpu_workspace_tangent.py at the CPU oracle's solution."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fleet_adjoint_ref as ref
import fleet_sensitivity_ref as sref
from oracle import binding as ob
from qpdo_amd import _build, problems, solver

LD = ref.LD
EPS_LD = float(np.finfo(LD).eps)


# ---- the C-side checks from a C caller -----------------------------------------------------------------------------------------------------
def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="tangent_args_driver.c")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    if sanitize:
        supp = tmp_path / "lsan.supp"
        supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\nleak:librccl\n")
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                   LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    return out.returncode, out.stdout + out.stderr


def test_argument_checks_from_a_c_caller(tmp_path):
    rc, txt = run_driver(tmp_path, False)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """the host driver (qpdo_api.c) and the C caller with -fsanitize=address,undefined, as a stand-alone program on the CPU"""
    rc, txt = run_driver(tmp_path, True)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]


def test_the_symbols_and_the_stats_layout():
    L = solver.lib()
    for name in ("qpdo_amd_tangent", "qpdo_amd_get_tangent_stats"):
        assert name in solver.EXT_SYMBOLS and hasattr(L, name)
    assert C.sizeof(solver.TangentStats) == 48 and C.sizeof(solver.AdjointStats) == 48
    assert [f for f, _ in solver.TangentStats._fields_] == ["calls", "rhs_total", "factorizations", "sweeps_total", "scratch_bytes", "last_seconds"]
    s = solver.TangentStats()
    assert L.qpdo_amd_get_tangent_stats(None, C.byref(s)) != 0
    assert (L.qpdo_amd_last_error() or b"").decode() == "qpdo_amd_get_tangent_stats: NULL workspace"


# ---- the Python wrapper's validation ---------------------------------------------------------------------------------------------------------
def test_tangent_validates_before_any_library_call():
    """no workspace here (the handle is NULL and never reached): every refusal comes from the shape and dtype checks"""
    qp = solver.QPDO()
    qp.n, qp.m = 5, 3
    qp._Qview_keep, qp._Apat = (None, None, np.zeros(7)), (None, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"^no tangent passed"):
        qp.tangent()
    with pytest.raises(ValueError, match=r"^tq: expected a numpy array, got list"):
        qp.tangent(tq=[0.0] * 5)
    with pytest.raises(ValueError, match=r"^tl: expected dtype float64, got float32"):
        qp.tangent(tl=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match=r"^tq: expected shape \(5,\) or \(R, 5\), got \(4,\)"):
        qp.tangent(tq=np.zeros(4))
    with pytest.raises(ValueError, match=r"^tu: expected shape \(3,\) or \(R, 3\), got \(2, 2, 3\)"):
        qp.tangent(tu=np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match=r"^tQ_values: expected shape \(7,\) or \(R, 7\), got \(5,\)"):
        qp.tangent(tq=np.zeros(5), tQ_values=np.zeros(5))
    with pytest.raises(ValueError, match=r"^tA_values: expected shape \(4,\) or \(R, 4\), got \(2, 5\)"):
        qp.tangent(tA_values=np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"^tq and tl do not agree on R"):
        qp.tangent(tq=np.zeros((2, 5)), tl=np.zeros(3))
    with pytest.raises(ValueError, match=r"^tq and tA_values do not agree on R"):
        qp.tangent(tq=np.zeros((2, 5)), tu=np.zeros((2, 3)), tA_values=np.zeros((3, 4)))
    with pytest.raises(ValueError, match=r"^tq: expected at least one right-hand side"):
        qp.tangent(tq=np.zeros((0, 5)))
    with pytest.raises(RuntimeError, match=r"^tangent: no workspace"):
        qp.tangent(tq=np.zeros(5), tl=np.zeros(3))


def test_workspace_qp_sensitivities_are_refused_before_a_forward():
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    lay = WorkspaceQP(None)
    assert lay.tangent_status is None and lay.vjp_status is None
    with pytest.raises(RuntimeError, match=r"^WorkspaceQP.tangent: no forward yet"):
        lay.tangent(tq=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"^WorkspaceQP.vjp_many: no forward yet"):
        lay.vjp_many(torch.zeros((2, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"^no tangent passed"):
        lay.tangent()


# ---- the sign convention -----------------------------------------------------------------------------------------------------------------------
def test_the_reference_tangent_of_tq_is_the_reference_adjoint_of_gx_equal_tq():
    """For tq alone the tangent's right-hand side is (-tq, 0) and the adjoint's for gx = tq, gy = None is (tq, 0), on ONE symmetric matrix:
    (dx, dy_S) = -(vx, vy_S).  With the adjoint's outputs dq = -vx and dl + du = vy that is
        dx = dq   and   dy = -(dl + du)
    -- the multiplier's sign turns: in the 1 x 1 problem Q = A = 1 with the row active, M^-1 = [0 1; 1 -1], the adjoint of gx = t gives
    vx = 0, vy = du = t and the tangent of tq = t gives dx = 0, dy = -t.  Checked here in longdouble up to the references' own rounding
    (both solve M by the same solve_ref: the bound is their two residuals through 2 ||M^-1||_inf), on random_qp(4, 40, 60, 0.3, n_eq=4) at
    the CPU oracle's solution."""
    p = problems.random_qp(4, 40, 60, 0.3, n_eq=4)
    o = ob.OracleSolver(p, ob.default_settings(max_iter=1000))
    r = o.solve()
    o.close()
    assert r["info"]["status_val"] == 1
    x, y = r["x"], r["y"]
    l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
    flags = ref.classify(x, y, ref.dense(p["A"]), l, u)
    assert 0 < (flags != 0).sum() < p["m"]
    stype = p["Qstype"]
    tq = np.random.default_rng(12).standard_normal(p["n"])
    Qd, Ad = ref.full_Q(p["Q"], stype), ref.dense(p["A"])
    vx, vy, M, S = ref.adjoint(Qd, Ad, flags, tq.astype(LD), None)
    g = ref.gradients(p["Q"], stype, p["A"], flags, x, y, vx, vy)
    rh = sref.tangent_rhs(p["Q"], stype, p["A"], flags, x, y, tq=tq)
    assert np.array_equal(rh["rx"], -tq.astype(LD)) and not rh["ry"].any()
    dx, dy, M2, _ = sref.tangent(Qd, Ad, flags, rh["rx"], rh["ry"])
    assert np.array_equal(M, M2)
    v, d = np.concatenate([vx, vy[S]]), np.concatenate([dx, dy[S]])
    gg = np.concatenate([tq.astype(LD), np.zeros(len(S), LD)])
    minv = float(np.abs(np.linalg.inv(M.astype(np.float64))).sum(axis=1).max())
    bound = 2.0 * minv * (float(np.abs(M @ v - gg).max()) + float(np.abs(M @ d + gg).max())) + 4 * EPS_LD * float(np.abs(v).max())
    ex, ey = float(np.abs(dx - g["dq"]).max()), float(np.abs(dy + (g["dl"] + g["du"])).max())
    print("dx against dq: %.3e, dy against -(dl + du): %.3e, bound %.3e, |dy|max %.3e" % (ex, ey, bound, float(np.abs(dy).max())))
    assert ex <= bound and ey <= bound, (ex, ey, bound)
    assert bound <= 1e-6 * float(np.abs(dy).max()), "the check would not tell the two signs apart"
    assert not bits_any(dy[flags == 0]), "dy off S"


def bits_any(a):
    return np.asarray(a, np.float64).view(np.uint64).any()
