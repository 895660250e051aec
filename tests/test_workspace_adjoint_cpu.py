"""The workspace adjoint (qpdo_amd_adjoint, include/qpdo_amd_ext.h) where no device is needed: every argument check that comes before the
backend is touched, by message and in the header's order, from a compiled C program (tests/adjoint_args_driver.c), plain and with the
host driver under AddressSanitizer + UBSan; solver.QPDO.adjoint validates shapes and dtypes before any library call; and the reference
the GPU tests lean on (tests/fleet_adjoint_ref.py) satisfies the duality identity with the tangent system on the n = 40 problem of
tests/test_gpu_workspace_adjoint.py, at the CPU oracle's solution."""
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
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="adjoint_args_driver.c")
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
    for name in ("qpdo_amd_adjoint", "qpdo_amd_get_adjoint_stats"):
        assert name in solver.EXT_SYMBOLS and hasattr(L, name)
    assert C.sizeof(solver.AdjointStats) == 48
    assert [f for f, _ in solver.AdjointStats._fields_] == ["calls", "rhs_total", "factorizations", "sweeps_total", "scratch_bytes", "last_seconds"]
    s = solver.AdjointStats()
    assert L.qpdo_amd_get_adjoint_stats(None, C.byref(s)) != 0
    assert (L.qpdo_amd_last_error() or b"").decode() == "qpdo_amd_get_adjoint_stats: NULL workspace"


# ---- the Python wrapper's validation ---------------------------------------------------------------------------------------------------------
def test_adjoint_validates_before_any_library_call():
    """no workspace here (the handle is NULL and never reached): every refusal comes from the shape and dtype checks"""
    qp = solver.QPDO()
    qp.n, qp.m = 5, 3
    with pytest.raises(ValueError, match=r"^gx: expected a numpy array, got list"):
        qp.adjoint([0.0] * 5)
    with pytest.raises(ValueError, match=r"^gx: expected dtype float64, got float32"):
        qp.adjoint(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match=r"^gx: expected shape \(5,\) or \(R, 5\), got \(4,\)"):
        qp.adjoint(np.zeros(4))
    with pytest.raises(ValueError, match=r"^gx: expected shape \(5,\) or \(R, 5\), got \(2, 2, 5\)"):
        qp.adjoint(np.zeros((2, 2, 5)))
    with pytest.raises(ValueError, match=r"^gx: expected at least one right-hand side"):
        qp.adjoint(np.zeros((0, 5)))
    with pytest.raises(ValueError, match=r"^gy: expected shape \(3,\) or \(R, 3\), got \(5,\)"):
        qp.adjoint(np.zeros(5), np.zeros(5))
    with pytest.raises(ValueError, match=r"^gy: expected dtype float64"):
        qp.adjoint(np.zeros(5), np.zeros(3, np.int64))
    with pytest.raises(ValueError, match=r"^gy: expected shape \(2, 3\) to go with gx, got \(3,\)"):
        qp.adjoint(np.zeros((2, 5)), np.zeros(3))
    with pytest.raises(RuntimeError, match=r"^adjoint: no workspace"):
        qp.adjoint(np.zeros(5), np.zeros(3))


def test_workspace_qp_rejects_an_unknown_on_failure():
    from qpdo_amd.torch_layer import WorkspaceQP
    with pytest.raises(ValueError, match="^on_failure: expected one of"):
        WorkspaceQP(None, on_failure="ignore")
    lay = WorkspaceQP(None, on_failure="zero")
    assert lay.on_failure == "zero" and lay.warm_start_last is True and lay.serial == 0


# ---- the reference the GPU test leans on --------------------------------------------------------------------------------------------------------
def test_the_reference_satisfies_the_duality_identity_on_the_n40_problem():
    """<gx, dx> + <gy_S, dy_S> = <dq, tq> + <dl, tl> + <du, tu> + <dQx, tQx> + <dAx, tAx> (include/qpdo_amd_ext.h, DUALITY) with the adjoint
    of tests/fleet_adjoint_ref.py and the tangent of tests/fleet_sensitivity_ref.py, both longdouble, at the CPU oracle's solution of
    random_qp(4, 40, 60, 0.3, n_eq=4) and the flags classify() gives there.  The bound is the one of tests/test_fleet_sensitivity_cpu.py:
    the two systems' longdouble residuals times the other solution's 1-norm, plus the rounding of the dot products."""
    p = problems.random_qp(4, 40, 60, 0.3, n_eq=4)
    o = ob.OracleSolver(p, ob.default_settings(max_iter=1000))
    r = o.solve()
    o.close()
    assert r["info"]["status_val"] == 1
    x, y = r["x"], r["y"]
    l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
    flags = ref.classify(x, y, ref.dense(p["A"]), l, u)
    assert ref.margins(x, y, p["A"], l, u).min() >= 1e-9 and 0 < (flags != 0).sum() < p["m"]
    stype = p["Qstype"]
    rng = np.random.default_rng(11)
    gx, gy = rng.standard_normal(p["n"]).astype(LD), rng.standard_normal(p["m"]).astype(LD)
    Qd, Ad = ref.full_Q(p["Q"], stype), ref.dense(p["A"])
    vx, vy, M, S = ref.adjoint(Qd, Ad, flags, gx, gy)
    g = ref.gradients(p["Q"], stype, p["A"], flags, x, y, vx, vy)
    import scipy.sparse as sp
    t = dict(tq=rng.standard_normal(p["n"]), tl=rng.standard_normal(p["m"]), tu=rng.standard_normal(p["m"]),
             tQ_values=rng.standard_normal(sp.csc_matrix(p["Q"]).nnz), tA_values=rng.standard_normal(sp.csc_matrix(p["A"]).nnz))
    if stype == 0:                       # (a full-storage perturbation is passed symmetric)
        T = sp.csc_matrix(p["Q"]).copy(); T.sort_indices(); T.data = t["tQ_values"].copy()
        T = ((T + T.T) / 2).tocsc(); T.sort_indices()
        t["tQ_values"] = np.asarray(T.data)
    rh = sref.tangent_rhs(p["Q"], stype, p["A"], flags, x, y, **t)
    dx, dy, M2, _ = sref.tangent(Qd, Ad, flags, rh["rx"], rh["ry"])
    assert np.array_equal(M, M2)
    lhs = gx @ dx + gy[S] @ dy[S]
    rhs = sum(g[k] @ t[tk].astype(LD) for k, tk in (("dq", "tq"), ("dl", "tl"), ("du", "tu"), ("dQ_values", "tQ_values"), ("dA_values", "tA_values")))
    v, d = np.concatenate([vx, vy[S]]), np.concatenate([dx, dy[S]])
    gg, rr = np.concatenate([gx, gy[S]]), np.concatenate([rh["rx"], rh["ry"]])
    e_a, e_t = np.abs(M @ v - gg).max(), np.abs(M @ d - rr).max()
    _, _, mag = sref.duality_sides(gg, d, v, rr)
    terms = sum(np.abs(g[k]) @ np.abs(t[tk]) for k, tk in (("dq", "tq"), ("dl", "tl"), ("du", "tu"), ("dQ_values", "tQ_values"), ("dA_values", "tA_values")))
    size = len(v) + sp.csc_matrix(p["Q"]).nnz + sp.csc_matrix(p["A"]).nnz + 2
    bound = np.abs(v).sum() * e_t + np.abs(d).sum() * e_a + size * EPS_LD * (mag + terms + np.abs(v) @ rh["T"])
    print("duality: |lhs - rhs| = %.3e, bound %.3e, magnitude %.3e" % (float(abs(lhs - rhs)), float(bound), float(mag)))
    assert abs(lhs - rhs) <= bound, (float(abs(lhs - rhs)), float(bound))
