"""The fleet's many-right-hand-side calls (qpdo_amd_fleet_adjoint_multi_dev, qpdo_amd_fleet_tangent_dev, include/qpdo_amd_ext.h) where no
device is needed: the reference the GPU tests lean on (tests/fleet_sensitivity_ref.py) satisfies the duality identity with the adjoint
reference to longdouble rounding and equals central differences of the longdouble KKT solution, the new calls on a NULL fleet are refused
under their own names, Fleet.adjoint_many_device / tangent_device validate their tensors before any library call, and the C-side checks run
again from a compiled C program with the host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import fleet_adjoint_ref as ref
import fleet_sensitivity_ref as sref
from qpdo_amd import _build, solver
from test_fleet_adjoint_cpu import kkt_solution, tiny_qp

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


def random_tangent(p, rng, stype):
    n, m = p["n"], p["m"]
    B = rng.standard_normal((n, n))
    rows, cols = p["Q"].indices, np.repeat(np.arange(n), np.diff(p["Q"].indptr))
    return dict(tq=rng.standard_normal(n), tl=rng.standard_normal(m), tu=rng.standard_normal(m), tQ_values=(B + B.T)[rows, cols],
                tA_values=rng.standard_normal(p["A"].nnz))


@pytest.mark.parametrize("stype", [-1, 1, 0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tangent_and_adjoint_references_are_dual(stype, seed):
    """<gx, dx> + <gy_S, dy_S> = <dq, tq> + <dl, tl> + <du, tu> + <dQ, tQ> + <dA, tA> for random small KKT matrices, both sides in longdouble:
    the gap is bounded by the two solves' longdouble residuals times the other solution's 1-norm plus the rounding of the dot products"""
    p, flags = tiny_qp(60 + 7 * seed + stype, stype)
    rng = np.random.default_rng(seed)
    x, y, Qd, Ad = kkt_solution(p, flags)
    if stype == 0:
        Qd = (Qd + Qd.T) / 2
    gx, gy = rng.standard_normal(p["n"]).astype(LD), rng.standard_normal(p["m"]).astype(LD)
    t = random_tangent(p, rng, stype)
    vx, vy, M, S = ref.adjoint(Qd, Ad, flags, gx, gy)
    g = ref.gradients(p["Q"], stype, p["A"], flags, x, y, vx, vy)
    rh = sref.tangent_rhs(p["Q"], stype, p["A"], flags, x, y, **t)
    dx, dy, M2, _ = sref.tangent(Qd, Ad, flags, rh["rx"], rh["ry"])
    assert np.array_equal(M, M2) and not dy[flags == 0].any() and rh["L"] >= 2
    lhs = gx @ dx + gy[S] @ dy[S]
    rhs = g["dq"] @ t["tq"].astype(LD) + g["dl"] @ t["tl"].astype(LD) + g["du"] @ t["tu"].astype(LD) + g["dQ_values"] @ t["tQ_values"].astype(LD) + \
        g["dA_values"] @ t["tA_values"].astype(LD)
    v, d = np.concatenate([vx, vy[S]]), np.concatenate([dx, dy[S]])
    gg, rr = np.concatenate([gx, gy[S]]), np.concatenate([rh["rx"], rh["ry"]])
    e_a, e_t = np.abs(M @ v - gg).max(), np.abs(M @ d - rr).max()
    a, b, mag = sref.duality_sides(gg, d, v, rr)
    assert abs(a - lhs) <= len(v) * EPS_LD * mag
    terms = np.abs(g["dq"]) @ np.abs(t["tq"]) + np.abs(g["dl"]) @ np.abs(t["tl"]) + np.abs(g["du"]) @ np.abs(t["tu"]) + np.abs(g["dQ_values"]) @ np.abs(t["tQ_values"]) + \
        np.abs(g["dA_values"]) @ np.abs(t["tA_values"])
    size = len(v) + p["Q"].nnz + p["A"].nnz + 2
    bound = np.abs(v).sum() * e_t + np.abs(d).sum() * e_a + size * EPS_LD * (mag + terms + np.abs(v) @ rh["T"])
    assert abs(lhs - rhs) <= bound, (float(abs(lhs - rhs)), float(bound))
    assert abs(lhs - rhs) <= 1e-15 * float(mag), "longdouble rounding, not a float64 quantity"


@pytest.mark.parametrize("stype", [-1, 1, 0])
def test_the_tangent_equals_central_differences(stype):
    """tangent() against central differences of the longdouble KKT solution along the perturbation (h = 1e-5, relative 1e-7: the solution map
    is linear in q, l, u and the truncation term of Q, A is O(h^2))"""
    p, flags = tiny_qp(80 + stype, stype)
    rng = np.random.default_rng(11)
    t = random_tangent(p, rng, stype)
    x, y, Qd, Ad = kkt_solution(p, flags)
    if stype == 0:
        Qd = (Qd + Qd.T) / 2
    rh = sref.tangent_rhs(p["Q"], stype, p["A"], flags, x, y, **t)
    dx, dy, _, S = sref.tangent(Qd, Ad, flags, rh["rx"], rh["ry"])
    h = LD(1e-5)

    def at(s):
        return kkt_solution(p, flags, Qdata=p["Q"].data.astype(LD) + s * t["tQ_values"], Adata=p["A"].data.astype(LD) + s * t["tA_values"],
                            q=p["q"].astype(LD) + s * t["tq"], l=p["l"].astype(LD) + s * t["tl"], u=p["u"].astype(LD) + s * t["tu"])[:2]

    (xp, yp), (xm, ym) = at(h), at(-h)
    scale = max(float(np.abs(dx).max()), float(np.abs(dy).max()))
    assert float(np.abs((xp - xm) / (2 * h) - dx).max()) <= 1e-7 * scale
    assert float(np.abs((yp - ym) / (2 * h) - dy)[S].max()) <= 1e-7 * scale


def test_null_perturbations_and_unused_rows():
    p, flags = tiny_qp(33, -1)
    x, y, _, _ = kkt_solution(p, flags)
    rng = np.random.default_rng(4)
    t = random_tangent(p, rng, -1)
    z = sref.tangent_rhs(p["Q"], -1, p["A"], flags, x, y)
    assert not z["rx"].any() and not z["ry"].any() and z["L"] == 1 and not z["T"].any()
    base = sref.tangent_rhs(p["Q"], -1, p["A"], flags, x, y, **t)
    tn = {k: v.copy() for k, v in t.items()}
    tn["tl"][flags != -1] = np.nan
    tn["tu"][flags != 1] = np.nan
    tn["tA_values"][flags[p["A"].indices] == 0] = np.nan
    other = sref.tangent_rhs(p["Q"], -1, p["A"], flags, x, y, **tn)
    assert np.array_equal(base["rx"], other["rx"]) and np.array_equal(base["ry"], other["ry"])
    # an entry of the triangle that stype -1 ignores contributes nothing
    full = p["Q"].toarray()
    Qu = sp.csc_matrix(full + np.triu(np.ones_like(full), 1) * 0.5)
    Qu.sort_indices()
    tv = rng.standard_normal(Qu.nnz)
    rows, cols = Qu.indices, np.repeat(np.arange(p["n"]), np.diff(Qu.indptr))
    tw = tv.copy(); tw[rows < cols] = 1e6
    a = sref.tangent_rhs(Qu, -1, p["A"], flags, x, y, tQ_values=tv)
    b = sref.tangent_rhs(Qu, -1, p["A"], flags, x, y, tQ_values=tw)
    assert np.array_equal(a["rx"], b["rx"])


# ---- host arithmetic and refusals without a device -----------------------------------------------------------------------------------------
def test_the_new_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    s = solver.FleetSensitivityStats()
    calls = dict(
        qpdo_amd_fleet_adjoint_multi_dev=lambda: L.qpdo_amd_fleet_adjoint_multi_dev(None, 3, *([None] * 10), 1e-9, 20, 0, 0, 0, 0, None),
        qpdo_amd_fleet_tangent_dev=lambda: L.qpdo_amd_fleet_tangent_dev(None, 0, *([None] * 10), 1e-9, 20, 0, 0, 0, 0, None),
        qpdo_amd_fleet_get_sensitivity_stats=lambda: L.qpdo_amd_fleet_get_sensitivity_stats(None, C.byref(s)))
    for name, call in calls.items():
        assert call() != 0 and last_error() == name + ": NULL fleet", (name, last_error())
        assert name in solver.EXT_SYMBOLS and hasattr(L, name)
    assert L.qpdo_amd_fleet_rhs_group(None) == -1 and "qpdo_amd_fleet_rhs_group" in solver.EXT_SYMBOLS
    assert C.sizeof(solver.FleetSensitivityStats) == 24 and [f for f, _ in solver.FleetSensitivityStats._fields_] == ["calls", "rhs_total", "scratch_bytes"]
    assert C.sizeof(solver.FleetAdjointStats) == 16 and C.sizeof(solver.FleetDevStats) == 40


def fake_fleet():
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims = None, 2, [(4, 3), (2, 0)]
    F._layout, F._device, F._dev_out, F._adj_out = (np.array([0, 4, 6]), np.array([0, 3, 3])), 0, None, None
    F._mlayout = (np.array([0, 7, 9]), np.array([0, 5, 5]))
    return F


def test_the_device_calls_validate_before_any_library_call():
    """no GPU here: shapes, dtype and element counts are checked before the device, so each refusal is reachable with CPU tensors; the (NULL)
    handle is never reached"""
    import torch
    F = fake_fleet()
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError, match="^gx: expected a tensor, got None"):
        F.adjoint_many_device(None)
    with pytest.raises(ValueError, match=r"^gx: expected a tensor of shape \(R, 6\)"):
        F.adjoint_many_device(z(6))
    with pytest.raises(ValueError, match="^gx: expected at least one right-hand side"):
        F.adjoint_many_device(z(0, 6))
    with pytest.raises(ValueError, match="^gx: expected 12 elements"):
        F.adjoint_many_device(z(2, 5))
    with pytest.raises(ValueError, match="^gx: expected dtype float64, got torch.float32"):
        F.adjoint_many_device(z(2, 6, dt=torch.float32))
    with pytest.raises(ValueError, match="^gx: expected a tensor on the GPU"):
        F.adjoint_many_device(z(2, 6))
    with pytest.raises(ValueError, match="^no tangent passed"):
        F.tangent_device()
    with pytest.raises(ValueError, match="do not agree on R"):
        F.tangent_device(tq=z(2, 6), tl=z(3, 3))
    with pytest.raises(ValueError, match="do not agree on R"):
        F.tangent_device(tq=z(6), tl=z(1, 3))
    with pytest.raises(ValueError, match=r"^tq: expected a tensor of shape \(L,\) or \(R, L\)"):
        F.tangent_device(tq=z(1, 2, 3))
    with pytest.raises(ValueError, match="^tA_values: expected 10 elements"):
        F.tangent_device(tA_values=z(2, 4))
    with pytest.raises(ValueError, match="^tq: expected a tensor on the GPU"):
        F.tangent_device(tq=z(6))


def test_fleet_qp_sensitivities_need_a_forward():
    from qpdo_amd.torch_layer import FleetQP
    layer = FleetQP(fake_fleet())
    with pytest.raises(RuntimeError, match="FleetQP.tangent: no forward yet"):
        layer.tangent()
    with pytest.raises(RuntimeError, match="FleetQP.vjp_many: no forward yet"):
        layer.vjp_many(None)


# ---- the C-side checks from a C caller ------------------------------------------------------------------------------------------------------
def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_sensitivity_args_driver.c")
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
