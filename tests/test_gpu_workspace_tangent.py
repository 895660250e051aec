"""The workspace tangent (qpdo_amd_tangent, solver.QPDO.tangent, qpdo_amd.torch_layer.WorkspaceQP.tangent / vjp_many; include/qpdo_amd_ext.h,
DESIGN.md 3.7) on the MI355X, in this process, on the problems and workspaces of tests/test_gpu_workspace_adjoint.py (imported from there:
one 64-tile, ld = 192 with a ragged tile, two band workspaces, the fused-route workspace, m = 0; Q stored as a triangle and in full).

The acceptance rule is that of tests/_fleet_sensitivity_worker.py check_tangent, for one QP: with d = (dx, dy_S) read back, r the longdouble
right-hand side of tests/fleet_sensitivity_ref.py for the DEVICE's flags, the longdouble residual of the unscaled system is at most
    tol max(||rx||, ||ry_S||) + (n + k + 2) eps || |M| |d| ||_inf + (L + 2) eps ||T||_inf
(second term: the device's fp64 residual evaluation; third: its fp64 right-hand side, L the longest row of the formation, T the sum of the
absolute values of its terms per component), and where cond(M) < 1 / eps the error against solve_ref is at most 2 ||M^-1||_inf times that.
Every output array is pre-filled with a sentinel."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fleet_adjoint_ref as ref
import fleet_sensitivity_ref as sref
from qpdo_amd import problems, solver
from test_gpu_workspace_adjoint import SENTINEL, TOL, W, bits, problem, raw_adjoint, same_bits, snapshot, with_storage, workspace  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(ref.LD).eps)
T_KEYS = ("tq", "tl", "tu", "tQ_values", "tA_values")
O_KEYS = ("dx", "dy", "residual")


def raw_tangent(qp, t, tol=TOL, max_sweeps=20, Qview=None):
    """qpdo_amd_tangent with every output pre-filled with a sentinel; t: dict of the arrays passed; returns (rc, message, outputs)"""
    a = {k: (None if t.get(k) is None else np.ascontiguousarray(t[k], np.float64)) for k in T_KEYS}
    first = next(v for v in a.values() if v is not None)
    R = 1 if first.ndim == 1 else first.shape[0]
    o = dict(dx=np.full((R, qp.n), SENTINEL), dy=np.full((R, qp.m), SENTINEL), active=np.full(qp.m, 77, np.int32), status=np.full((R, 3), -77, np.int64),
             residual=np.full(R, SENTINEL))
    dp = solver._as_dp
    Qv = Qview if Qview is not None else qp._Qview
    rc = solver.lib().qpdo_amd_tangent(qp._w, R, dp(a["tq"]), dp(a["tl"]), dp(a["tu"]), C.byref(Qv) if a["tQ_values"] is not None else None, dp(a["tQ_values"]),
                                       dp(a["tA_values"]), dp(o["dx"]), dp(o["dy"]), o["active"].ctypes.data_as(C.POINTER(C.c_int)),
                                       o["status"].ctypes.data_as(C.POINTER(C.c_long)), dp(o["residual"]), float(tol), int(max_sweeps))
    return rc, (solver.lib().qpdo_amd_last_error() or b"").decode(), o


def untouched(o):
    return all((v == (77 if k == "active" else -77 if k == "status" else SENTINEL)).all() for k, v in o.items())


def perturbation(p, rng, R):
    """tq, tl, tu, tQ, tA of R right-hand sides; tQ symmetric as a matrix (needed where Q is stored in full)"""
    Q = sp.csc_matrix(p["Q"]); Q.sort_indices()
    rows, cols = Q.indices, np.repeat(np.arange(p["n"]), np.diff(Q.indptr))
    tQ = np.zeros((R, Q.nnz))
    for r in range(R):
        B = rng.standard_normal((p["n"], p["n"]))
        tQ[r] = (B + B.T)[rows, cols]
    return dict(tq=rng.standard_normal((R, p["n"])), tl=rng.standard_normal((R, p["m"])), tu=rng.standard_normal((R, p["m"])), tQ_values=tQ,
                tA_values=rng.standard_normal((R, sp.csc_matrix(p["A"]).nnz)))


def pick(t, r):
    return {k: (None if t.get(k) is None else (t[k] if t[k].ndim == 1 else t[k][r])) for k in T_KEYS}


def check_rhs(p, sol, o, r, t, what, accept=(0,)):
    """every check of right-hand side r of one call against the reference; returns (code, 1 where the error-bound branch ran)"""
    n, m = p["n"], p["m"]
    code, sweeps, k = o["status"][r].tolist()
    dx, dy, flags = o["dx"][r], o["dy"][r], o["active"]
    assert code in accept, (what, code, sweeps)
    assert set(np.unique(flags)) <= {-1, 0, 1} and k == int((flags != 0).sum()), (what, "flags", k)
    if code != 0:
        assert np.isnan(dx).all() and np.isnan(dy).all() and np.isnan(o["residual"][r]), (what, "NaN slices")
        return code, 0
    assert np.isfinite(dx).all() and np.isfinite(dy).all() and (dx != SENTINEL).all() and (dy != SENTINEL).all(), (what, "NaN or an unwritten entry")
    assert o["residual"][r] <= TOL and 0 <= sweeps <= 20, (what, o["residual"][r], sweeps)
    assert not bits(dy)[flags == 0].any(), (what, "dy off S is a bitwise +0.0")
    Qf, A = ref.full_Q(p["Q"], p["Qstype"]), (ref.dense(p["A"]) if m else np.zeros((0, n)))
    rh = sref.tangent_rhs(p["Q"], p["Qstype"], p["A"], flags, sol["x"], sol["y"], **pick(t, r))
    M, S = ref.kkt(Qf, A, flags)
    d = np.concatenate([dx.astype(ref.LD), dy.astype(ref.LD)[S]])
    rhs = np.concatenate([rh["rx"], rh["ry"]])
    gn = float(np.abs(rhs).max()) if len(rhs) else 0.0
    res = float(np.abs(M @ d - rhs).max())
    bound = TOL * gn + (n + k + 2) * EPS * float((np.abs(M) @ np.abs(d)).max()) + (rh["L"] + 2) * EPS * float(rh["T"].max())
    assert res <= bound, (what, "residual", res, bound)
    ran = 0
    M64 = M.astype(np.float64)
    cond = np.linalg.cond(M64)
    if np.isfinite(cond) and cond < 1.0 / EPS:
        minv = float(np.abs(np.linalg.inv(M64)).sum(axis=1).max())
        dref, _ = ref.solve_ref(M, rhs)
        err = float(np.abs(d - dref).max())
        assert err <= 2.0 * minv * bound, (what, "error", err, 2.0 * minv * bound)
        ran = 1
    print("%s: code 0, %d sweeps, k = %d, residual %.2e, longdouble residual %.2e <= %.2e" % (what, sweeps, k, o["residual"][r], res, bound))
    return code, ran


def solve_and_check(monkeypatch, p, linsolve, scaling, what, expect_linsolve):
    """tq alone; tq + tQ; all five with R = 3 -- each against the reference; the flags are the adjoint's; the wrapper delivers the raw bits"""
    qp = workspace(monkeypatch, p, linsolve, scaling)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1 and qp.stats()["linsolve"] == expect_linsolve, (what, sol["info"], qp.stats()["linsolve"])
        rng = np.random.default_rng(300 + scaling)
        t = perturbation(p, rng, 3)
        rc, msg, a = raw_adjoint(qp, t["tq"][0])
        assert rc == 0 and a["status"][0, 0] == 0, msg
        ran = 0
        t1 = dict(tq=t["tq"][0])
        rc, msg, o1 = raw_tangent(qp, t1)
        assert rc == 0, msg
        ran += check_rhs(p, sol, o1, 0, t1, what + " tq")[1]
        assert np.array_equal(o1["active"], a["active"]) and o1["status"][0, 2] == a["status"][0, 2], (what, "the flags are the adjoint's")
        t2 = dict(tq=t["tq"][:2], tQ_values=t["tQ_values"][:2])
        rc, msg, o2 = raw_tangent(qp, t2)
        assert rc == 0, msg
        for r in range(2):
            ran += check_rhs(p, sol, o2, r, t2, what + " tq, tQ rhs %d" % r)[1]
        rc, msg, o3 = raw_tangent(qp, t)
        assert rc == 0, msg
        for r in range(3):
            ran += check_rhs(p, sol, o3, r, t, what + " all rhs %d" % r)[1]
        assert np.array_equal(o2["active"], a["active"]) and np.array_equal(o3["active"], a["active"])
        assert ran >= 1, "the error-bound branch ran for no right-hand side of %s" % what
        st = qp.tangent_stats()
        assert (st["calls"], st["rhs_total"], st["factorizations"]) == (3, 6, 3) and st["scratch_bytes"] > 0 and st["last_seconds"] > 0, st
        w = qp.tangent(**t)
        for k in O_KEYS:
            assert same_bits(w[k], o3[k]), (what, k)
        assert np.array_equal(w["active"], o3["active"]) and np.array_equal(w["status"], o3["status"])
        w1 = qp.tangent(tq=t["tq"][0])
        assert w1["dx"].shape == (p["n"],) and w1["status"].shape == (3,) and same_bits(w1["dx"], o1["dx"][0]) and same_bits(w1["dy"], o1["dy"][0])
    finally:
        qp.delete()


# ---- 1. against the longdouble reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", ["n40", "n130"])
def test_dense(monkeypatch, name, scaling):
    solve_and_check(monkeypatch, problem(name), "dense", scaling, "dense %s[%d]" % (name, scaling), 1)


@pytest.mark.parametrize("scaling", [10, 0])
def test_fused_route_workspace(monkeypatch, scaling):
    """no QPDO_LINSOLVE: qpdo_solve ran as ONE launch of the fused kernel (stats: linsolve 2); the tangent reads nothing of the iterate state"""
    solve_and_check(monkeypatch, problem("n40"), None, scaling, "fused n40[%d]" % scaling, 2)


@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", ["band72", "band96"])
def test_band(monkeypatch, name, scaling):
    solve_and_check(monkeypatch, problem(name), "band", scaling, "band %s[%d]" % (name, scaling), 3)


@pytest.mark.parametrize("stype", [1, 0])
@pytest.mark.parametrize("name", ["n40", "n130"])
def test_dense_Q_stored_upper_and_full(monkeypatch, name, stype):
    """(the lower triangle is what test_dense runs); stype 0: tQ is read straight, row a from the stored entries of column a"""
    solve_and_check(monkeypatch, with_storage(problem(name), stype), "dense", 10, "dense %s stype %d" % (name, stype), 1)


def test_no_rows(monkeypatch):
    """m = 0: Q dx = -(tq + tQ x) with a strictly convex Q of n = 40"""
    rng = np.random.default_rng(2)
    n = 40
    B = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.2)
    Q = sp.csc_matrix(np.tril(B @ B.T + n * np.eye(n))); Q.sort_indices()
    p = dict(n=n, m=0, Q=Q, Qstype=-1, A=sp.csc_matrix((0, n)), q=rng.standard_normal(n), l=np.zeros(0), u=np.zeros(0), c=0.0)
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        t = perturbation(p, rng, 3)
        for tt, what in ((dict(tq=t["tq"][0]), "m = 0 tq"), (dict(tq=t["tq"][:2], tQ_values=t["tQ_values"][:2]), "m = 0 tq, tQ"), (t, "m = 0 all")):
            rc, msg, o = raw_tangent(qp, tt)
            assert rc == 0, msg
            for r in range(o["dx"].shape[0]):
                assert check_rhs(p, sol, o, r, tt, "%s rhs %d" % (what, r)) == (0, 1) and o["status"][r, 2] == 0
    finally:
        qp.delete()


# ---- 2. ignored entries -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_ignored_entries_may_hold_nan(monkeypatch, name, linsolve):
    p = problem(name)
    qp = workspace(monkeypatch, p, linsolve, 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        t = perturbation(p, np.random.default_rng(41), 2)
        rc, msg, clean = raw_tangent(qp, t)
        assert rc == 0 and clean["status"][:, 0].tolist() == [0, 0], (msg, clean["status"].tolist())
        flags = clean["active"]
        A = sp.csc_matrix(p["A"]); A.sort_indices()
        unused = flags[A.indices] == 0
        assert (flags == 1).any() and (flags == -1).any() and (flags == 0).any() and unused.any()

        def planted(value):
            tn = {k: v.copy() for k, v in t.items()}
            tn["tl"][:, flags != -1] = value
            tn["tu"][:, flags != 1] = value
            tn["tA_values"][:, unused] = value
            return tn
        rc, msg, zeros = raw_tangent(qp, planted(0.0))
        assert rc == 0, msg
        rc, msg, nans = raw_tangent(qp, planted(np.nan))
        assert rc == 0, msg
        for k in O_KEYS:
            assert same_bits(nans[k], zeros[k]) and same_bits(nans[k], clean[k]), (name, k, "NaN on entries that are not used")
        assert np.array_equal(nans["status"], zeros["status"]) and np.array_equal(nans["active"], flags)
        # a NaN in a USED entry: code 1 and NaN slices for that right-hand side; the one behind it carries its single call's bits
        tb = planted(np.nan)
        tb["tu"][0, np.flatnonzero(flags == 1)[0]] = np.nan
        rc, msg, bad = raw_tangent(qp, tb)
        assert rc == 0 and bad["status"][:, 0].tolist() == [1, 0], (msg, bad["status"].tolist())
        check_rhs(p, sol, bad, 0, tb, name + " NaN in a used tu", accept=(1,))
        rc, msg, one = raw_tangent(qp, pick(t, 1))
        assert rc == 0, msg
        for k in O_KEYS:
            assert same_bits(bad[k][1], one[k][0]), (name, k, "behind a NaN right-hand side")
        for key, arr in (("tq", None), ("tQ_values", None), ("tA_values", np.flatnonzero(~unused))):
            tb = {k: v.copy() for k, v in t.items()}
            tb[key][1, 0 if arr is None else arr[0]] = np.nan
            rc, msg, bad = raw_tangent(qp, tb)
            assert rc == 0 and bad["status"][:, 0].tolist() == [0, 1] and np.isnan(bad["dx"][1]).all() and np.isnan(bad["dy"][1]).all(), (key, msg, bad["status"].tolist())
            assert same_bits(bad["dx"][0], clean["dx"][0]) and same_bits(bad["dy"][0], clean["dy"][0]), key
    finally:
        qp.delete()


# ---- 3. slabs and repeatability ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_many_right_hand_sides(monkeypatch, name, linsolve):
    """R = 3 on one factorization: every slab carries the bits of the single call with that slab of the inputs; the same call twice, the
    same bits; a zero right-hand side is accepted at sweep 0 with zeros"""
    p = problem(name)
    qp = workspace(monkeypatch, p, linsolve, 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        t = perturbation(p, np.random.default_rng(17), 3)
        t["tq"][1] = 0.0
        f0 = qp.tangent_stats()["factorizations"]
        rc, msg, many = raw_tangent(qp, t)
        assert rc == 0, msg
        assert qp.tangent_stats()["factorizations"] == f0 + 1 and qp.tangent_stats()["rhs_total"] == 3
        rc, msg, again = raw_tangent(qp, t)
        assert rc == 0, msg
        assert qp.tangent_stats()["factorizations"] == f0 + 2
        for k, v in many.items():
            assert np.array_equal(bits(v), bits(again[k])) if v.dtype == np.float64 else np.array_equal(v, again[k]), (k, "the same call twice")
        for r in range(3):
            rc, msg, one = raw_tangent(qp, pick(t, r))
            assert rc == 0, msg
            for k in O_KEYS:
                assert same_bits(many[k][r], one[k][0]), (name, r, k)
            assert many["status"][r].tolist() == one["status"][0].tolist() and np.array_equal(many["active"], one["active"])
            assert check_rhs(p, sol, many, r, t, "%s R=3 slab %d" % (name, r)) == (0, 1)
        rc, msg, z = raw_tangent(qp, dict(tq=np.zeros(p["n"]), tl=np.zeros(p["m"])))
        assert rc == 0 and z["status"][0, :2].tolist() == [0, 0] and not z["dx"].any() and not z["dy"].any(), (msg, z["status"].tolist())
    finally:
        qp.delete()


# ---- 4. one sweep driver -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_the_tangent_of_tq_is_the_adjoint_of_gx_equal_tq(monkeypatch, name, linsolve):
    """For tq alone the tangent's right-hand side is (-tq, 0), the adjoint's for gx = tq, gy = None is (tq, 0): they differ in sign only and
    every operation between them and the outputs is sign-symmetric (round to nearest; the norms are of absolute values), so ONE driver gives
    (dx, dy) = -(vx, vy) exactly.  In the adjoint's outputs dq = -vx and dl + du = vy, that is dx == dq and dy == -(dl + du): the
    multiplier's sign turns (tests/test_workspace_tangent_cpu.py pins this convention in the references).  Value equality: zero signs may
    differ.  The status triples and res are equal."""
    p = problem(name)
    qp = workspace(monkeypatch, p, linsolve, 10)
    try:
        assert qp.solve()["info"]["status_val"] == 1
        tq = np.random.default_rng(23).standard_normal((2, p["n"]))
        rc, msg, a = raw_adjoint(qp, tq, None)
        assert rc == 0 and (a["status"][:, 0] == 0).all(), (msg, a["status"].tolist())
        rc, msg, o = raw_tangent(qp, dict(tq=tq))
        assert rc == 0, msg
        assert np.array_equal(o["dx"], a["dq"]) and np.array_equal(o["dy"], -(a["dl"] + a["du"])), name
        assert np.array_equal(o["status"], a["status"]) and same_bits(o["residual"], a["residual"]) and np.array_equal(o["active"], a["active"])
        assert (a["status"][:, 1] >= 1).all() and np.abs(o["dy"]).max() > 0
    finally:
        qp.delete()


# ---- 5. duality ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_duality(monkeypatch, name, linsolve):
    """<gx, dx> + <gy_S, dy_S> = <dq, tq> + <dl, tl> + <du, tu> + <dQx, tQx> + <dAx, tAx>, all from the device.  With v = (-dq, (dl + du)_S),
    d = (dx, dy_S), g and r the two right-hand sides (r the reference's, longdouble): |<g, d> - <v, r>| is within the bound of
    tests/_fleet_sensitivity_worker.py duality -- the two systems' longdouble residuals times the other solution's 1-norm, plus
    (n + k + 2) eps (|g|.|d| + |v|.|r|).  The right side of the identity is <v, r> expanded term by term with the DELIVERED dQx, dAx, each of
    which is within 4 eps of its term sum (what test_gpu_workspace_adjoint.py asserts of them): that adds at most 4 eps |v|.T, T the sums of
    the absolute values of the formation's terms; the longdouble evaluation of the sums adds (entries) eps_ld of their magnitude."""
    p = problem(name)
    n, m = p["n"], p["m"]
    qp = workspace(monkeypatch, p, linsolve, 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        rng = np.random.default_rng(900)
        R = 3
        t = perturbation(p, rng, R)
        gx, gy = rng.standard_normal((R, n)), rng.standard_normal((R, m))
        rc, msg, a = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        rc, msg, d = raw_tangent(qp, t)
        assert rc == 0, msg
        flags = a["active"]
        assert np.array_equal(flags, d["active"]) and (a["status"][:, 0] == 0).all() and (d["status"][:, 0] == 0).all()
        Mk, S = ref.kkt(ref.full_Q(p["Q"], p["Qstype"]), ref.dense(p["A"]), flags)
        k = len(S)
        LD = ref.LD
        for r in range(R):
            v = np.concatenate([-a["dq"][r].astype(LD), (a["dl"][r] + a["du"][r]).astype(LD)[S]])
            dd = np.concatenate([d["dx"][r].astype(LD), d["dy"][r].astype(LD)[S]])
            g = np.concatenate([gx[r].astype(LD), gy[r].astype(LD)[S]])
            rh = sref.tangent_rhs(p["Q"], p["Qstype"], p["A"], flags, sol["x"], sol["y"], **pick(t, r))
            rr = np.concatenate([rh["rx"], rh["ry"]])
            e_a, e_t = np.abs(Mk @ v - g).max(), np.abs(Mk @ dd - rr).max()
            lhs, vr, mag = sref.duality_sides(g, dd, v, rr)
            bound = np.abs(v).sum() * e_t + np.abs(dd).sum() * e_a + (n + k + 2) * EPS * mag
            assert abs(lhs - vr) <= bound, ("duality", name, r, float(abs(lhs - vr)), float(bound))
            pairs = (("dq", "tq"), ("dl", "tl"), ("du", "tu"), ("dQ_values", "tQ_values"), ("dA_values", "tA_values"))
            tl_used, tu_used = np.where(flags == -1, t["tl"][r], 0.0), np.where(flags == 1, t["tu"][r], 0.0)     # (dl, du are +0.0 elsewhere)
            tt = dict(pick(t, r), tl=tl_used, tu=tu_used)
            rhs = sum(a[gk][r].astype(LD) @ tt[tk].astype(LD) for gk, tk in pairs)
            terms = sum(np.abs(a[gk][r]).astype(LD) @ np.abs(tt[tk]).astype(LD) for gk, tk in pairs)
            size = n + 2 * m + a["dQ_values"].shape[1] + a["dA_values"].shape[1]
            bound2 = bound + 4 * EPS * float(np.abs(v) @ rh["T"]) + size * EPS_LD * float(mag + terms)
            print("duality %s rhs %d: |<g,d> - <v,r>| %.3e <= %.3e; |lhs - rhs| %.3e <= %.3e; magnitude %.3e"
                  % (name, r, float(abs(lhs - vr)), float(bound), float(abs(lhs - rhs)), float(bound2), float(mag)))
            assert abs(lhs - rhs) <= bound2, ("duality, expanded", name, r, float(abs(lhs - rhs)), float(bound2))
            assert bound2 <= 1e-6 * mag, ("the check would be vacuous", float(bound2), float(mag))
    finally:
        qp.delete()


# ---- 6. code 1 -----------------------------------------------------------------------------------------------------------------------------------
def test_not_accepted(W, monkeypatch):
    """two identical active rows: consistent for tq alone, not for a tl / tu that differs on them (code 1 after 20 sweeps, NaN slices, the
    flags delivered); the neighbouring right-hand sides of the same call are untouched"""
    p = W.dup_item()
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        tq = np.random.default_rng(3).standard_normal(p["n"])
        tb = np.zeros(p["m"])
        tb[0], tb[1] = 1.0, -1.0
        tbad = dict(tq=tq, tl=tb, tu=tb)
        rc, msg, bad = raw_tangent(qp, tbad)
        assert rc == 0, msg
        assert bad["status"][0, :2].tolist() == [1, 20] and bad["active"][0] != 0 and bad["active"][1] != 0, bad["status"].tolist()
        check_rhs(p, sol, bad, 0, tbad, "inconsistent tb", accept=(1,))
        tq3 = np.stack([tq, tq, 2.0 * tq])
        tb3 = np.stack([np.zeros(p["m"]), tb, np.zeros(p["m"])])
        t3 = dict(tq=tq3, tl=tb3, tu=tb3)
        rc, msg, mix = raw_tangent(qp, t3)
        assert rc == 0 and mix["status"][:, 0].tolist() == [0, 1, 0] and mix["status"][1, 1] == 20, (msg, mix["status"].tolist())
        assert np.array_equal(mix["active"], bad["active"])
        for r in range(3):
            check_rhs(p, sol, mix, r, t3, "mixed call, right-hand side %d" % r, accept=((1,) if r == 1 else (0,)))
        for r in (0, 2):
            rc, msg, one = raw_tangent(qp, pick(t3, r))
            assert rc == 0, msg
            for k in O_KEYS:
                assert same_bits(mix[k][r], one[k][0]), (k, r, "a right-hand side beside a code 1 carries the single call's bits")
    finally:
        qp.delete()


# ---- 7. no bit moves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_no_bit_moves(monkeypatch, name, linsolve):
    """two workspaces on one problem, tangent calls (all five arrays) on X only: every later solve of X carries Y's bits -- x, y, every info
    field but the wall times, every trace record, every QPDOAmdStats member but the event timings.  Adjoint and tangent calls do not move
    each other's stats."""
    p = problem(name)
    X, Y = workspace(monkeypatch, p, linsolve, 10), workspace(monkeypatch, p, linsolve, 10)
    try:
        t = perturbation(p, np.random.default_rng(5), 2)
        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b)
        adj0 = X.adjoint_stats()
        rc, msg, o = raw_tangent(X, t)
        assert rc == 0 and (o["status"][:, 0] != 3).all(), (msg, o["status"].tolist())
        assert snapshot(X, a)["stats"] == snapshot(Y, b)["stats"], "QPDOAmdStats after the tangent call"
        assert X.adjoint_stats() == adj0 and adj0["calls"] == 0 and adj0["scratch_bytes"] == 0, "adjoint_stats after a tangent call"
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "the solve after the tangent call"
        rc, msg, o = raw_tangent(X, pick(t, 0))
        assert rc == 0, msg
        tan0 = X.tangent_stats()
        rc, msg, adj = raw_adjoint(X, t["tq"], t["tl"], matrices=True)
        assert rc == 0, msg
        assert X.tangent_stats() == tan0, "tangent_stats after an adjoint call"
        assert X.adjoint_stats()["calls"] == 1
        rc, msg, o2 = raw_tangent(X, pick(t, 0))                      # any mix of the two calls may follow one solve
        assert rc == 0 and all(same_bits(o[k], o2[k]) for k in O_KEYS), msg
        for S in (X, Y):
            S.update_q(1.5 * p["q"] + 0.1)
            S.warm_start(a["x"], a["y"])
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "update_q, warm_start, solve"
        assert X.tangent_stats()["calls"] == 3 and Y.tangent_stats()["calls"] == 0 and Y.adjoint_stats()["calls"] == 0
        # X's tangent calls built mapA (tAx) and mapQ (tQx); Y's first qpdo_amd_update_matrices builds its own: the same values arrive
        Q2, A2 = sp.csc_matrix(p["Q"]) * 1.25, sp.csc_matrix(p["A"]) * 0.75
        for S in (X, Y):
            S.update_matrices(Q=Q2, A=A2)
        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b), "update_matrices after the tangent built the maps"
        rc, msg, o = raw_tangent(X, t)
        assert rc == 0 and (o["status"][:, 0] == 0).all(), (msg, o["status"].tolist())
    finally:
        X.delete(); Y.delete()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    """each: nonzero return, a message that begins with the call's name and names the reason, the sentinel outputs untouched, `calls` unmoved"""
    p = problem("n40")
    tq = np.ones(p["n"])

    def refused(qp, msg_part, t=None, **kw):
        before = qp.tangent_stats()
        rc, msg, o = raw_tangent(qp, dict(tq=tq) if t is None else t, **kw)
        assert rc != 0 and msg.startswith("qpdo_amd_tangent: ") and msg_part in msg, (msg_part, rc, msg)
        assert untouched(o), msg_part
        assert qp.tangent_stats() == before, msg_part

    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        refused(qp, "status is not QPDO_SOLVED")                               # before any solve
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        rc, msg, o = raw_tangent(qp, dict(tq=tq))
        assert rc == 0 and o["status"][0, 0] == 0 and qp.tangent_stats()["calls"] == 1, msg
        qp.update_q(p["q"] * 1.25)
        refused(qp, "was not a solve")                                         # after update_q
        qp.solve()
        qp.warm_start(sol["x"], sol["y"])
        refused(qp, "was not a solve")                                         # after warm_start
        qp.solve()
        qp.update_bounds(p["l"] - 0.5, p["u"] + 0.5)
        refused(qp, "was not a solve")                                         # after update_bounds
        qp.solve()
        # "no tangent passed": the raw call with five NULL arrays
        o = dict(dx=np.full((1, qp.n), SENTINEL), dy=np.full((1, qp.m), SENTINEL))
        before = qp.tangent_stats()
        rc = solver.lib().qpdo_amd_tangent(qp._w, 1, None, None, None, None, None, None, solver._as_dp(o["dx"]), solver._as_dp(o["dy"]), None, None, None, TOL, 20)
        msg = (solver.lib().qpdo_amd_last_error() or b"").decode()
        assert rc != 0 and msg.startswith("qpdo_amd_tangent: no tangent passed") and untouched(o) and qp.tangent_stats() == before, msg
        # tQx with a Q of another pattern (the same stype, shape, entry count and column pointers: the device comparison finds it)
        Q2 = sp.csc_matrix(p["Q"]).copy(); Q2.sort_indices()
        ind = Q2.indices.copy()
        j = next(j for j in range(p["n"]) if Q2.indptr[j + 1] > Q2.indptr[j] and ind[Q2.indptr[j + 1] - 1] < p["n"] - 1)
        ind[Q2.indptr[j + 1] - 1] += 1
        keep = []
        view = solver._sparse_view(sp.csc_matrix((Q2.data, ind, Q2.indptr), shape=Q2.shape), p["Qstype"], keep)
        tQ = dict(tq=tq, tQ_values=np.ones(Q2.nnz))
        refused(qp, "pattern of Q differs", t=tQ, Qview=view)
        rc, msg, o = raw_tangent(qp, tQ)                                       # ... and the setup's own pattern passes
        assert rc == 0 and o["status"][0, 0] == 0, msg
    finally:
        qp.delete()
    k = problems.infeasibility_kat("primal_infeasible")
    qp = workspace(monkeypatch, k, "dense", 10, max_iter=k["max_iter"])
    try:
        assert qp.solve()["info"]["status_val"] == -3
        refused(qp, "status is not QPDO_SOLVED", t=dict(tq=np.ones(k["n"])))
    finally:
        qp.delete()
    qp = workspace(monkeypatch, p, "pcg", 10)
    try:
        assert qp.solve()["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 0
        refused(qp, "the workspace's solver is PCG")
        refused(qp, "QPDO_LINSOLVE=dense")
    finally:
        qp.delete()


# ---- 9. WorkspaceQP.tangent and WorkspaceQP.vjp_many -------------------------------------------------------------------------------------------
def test_workspace_qp_layer(monkeypatch):
    """bits equal the direct calls; refused before a forward; "zero" and "nan" per right-hand side; one first-order check of w'dx against a
    central difference of two extra solves"""
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    p = problem("n40")
    n, m = p["n"], p["m"]
    qp = workspace(monkeypatch, p, "dense", 0, eps_abs=1e-9, max_iter=10000)
    try:
        rng = np.random.default_rng(21)
        w = rng.standard_normal(n)
        rng = np.random.default_rng(31)
        t = dict(tq=rng.standard_normal(n), tl=rng.standard_normal(m), tu=rng.standard_normal(m))
        eq = p["l"] == p["u"]
        t["tu"][eq] = t["tl"][eq]                                   # (an equality row stays one along the direction)
        tt = {k: torch.from_numpy(v) for k, v in t.items()}
        layer = WorkspaceQP(qp)
        with pytest.raises(RuntimeError, match="no forward yet"):
            layer.tangent(**tt)
        with pytest.raises(RuntimeError, match="no forward yet"):
            layer.vjp_many(torch.from_numpy(w))
        x, y = layer(torch.from_numpy(p["q"].copy()))
        assert layer.status == 1
        sol = dict(x=x.numpy().copy(), y=y.numpy().copy())
        # the bits of the direct calls, single and R = 2
        full = perturbation(p, np.random.default_rng(33), 2)
        for tdict in (t, full):
            out = layer.tangent(**{k: torch.from_numpy(v) for k, v in tdict.items()})
            direct = qp.tangent(**tdict)
            for k in O_KEYS:
                assert same_bits(out[k].numpy(), direct[k]), k
            assert np.array_equal(out["status"].numpy(), direct["status"]) and np.array_equal(layer.tangent_status.numpy(), direct["status"])
            assert np.array_equal(out["active"].numpy(), direct["active"]) and (direct["status"][..., 0] == 0).all()
        gx, gy = rng.standard_normal((2, n)), rng.standard_normal((2, m))
        out = layer.vjp_many(torch.from_numpy(gx), torch.from_numpy(gy), matrices=True)
        direct = qp.adjoint(gx, gy, matrices=True)
        for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
            assert same_bits(out[k].numpy(), direct[k]), k
        assert np.array_equal(layer.vjp_status.numpy(), direct["status"]) and (direct["status"][:, 0] == 0).all()
        out = layer.vjp_many(torch.from_numpy(gx[0]))
        assert out["dQ_values"] is None and out["dA_values"] is None and same_bits(out["dq"].numpy(), qp.adjoint(gx[0])["dq"])
        # "zero" / "nan" per right-hand side: slab 1 carries a NaN in a used entry (code 1), slab 0 is delivered
        flags = direct["active"]
        bad = {k: v.copy() for k, v in full.items()}
        bad["tq"][1, 0] = np.nan
        badg = gx.copy()
        badg[1, 0] = np.nan
        for mode in ("zero", "nan"):
            lay = WorkspaceQP(qp, on_failure=mode)
            lay(torch.from_numpy(p["q"].copy()))
            good = qp.tangent(**full)
            out = lay.tangent(**{k: torch.from_numpy(v) for k, v in bad.items()})
            assert lay.tangent_status[:, 0].tolist() == [0, 1]
            assert same_bits(out["dx"][0].numpy(), good["dx"][0]) and same_bits(out["dy"][0].numpy(), good["dy"][0]), mode
            for k in ("dx", "dy"):
                assert (not bits(out[k][1].numpy()).any()) if mode == "zero" else np.isnan(out[k][1].numpy()).all(), (mode, k)
            out = lay.vjp_many(torch.from_numpy(badg), matrices=True)
            assert lay.vjp_status[:, 0].tolist() == [0, 1]
            for k in ("dq", "dl", "du", "dQ_values", "dA_values"):
                assert (not bits(out[k][1].numpy()).any()) if mode == "zero" else np.isnan(out[k][1].numpy()).all(), (mode, k)
                assert np.isfinite(out[k][0].numpy()).all(), (mode, k)
        # a workspace that moved on since the forward's solve: the library refuses, the layer passes the reason on
        qp.update_q(p["q"].copy())
        with pytest.raises(RuntimeError, match="was not a solve"):
            layer.tangent(**tt)
        # ---- first order: L = w'x along the direction (tq, tl, tu).  With the active set fixed the solution map is LINEAR in (q, l, u), so a
        # central difference has no truncation term, and what is left is the two solves' error over 2 h.  As in the adjoint test: a solve
        # that ends with the unscaled residuals (rp, rd) of its info (scaling 0) has |dL| <= ||vx||_1 (rd + ||A'||_inf rp) + ||vy_S||_1 rp with
        # (vx, vy) the REFERENCE's adjoint solution for gx = w and the device's flags.  To that the tangent's own error is added:
        # |w'(dx - dx_ref)| <= ||w||_1 2 ||M^-1||_inf (the residual bound that check_rhs asserts).  h was chosen on the CPU oracle with the
        # reference tangent (eps_abs 1e-9): h = 1e-3 moves the active set, h = 1e-5 has a bound of 1.8e-3; at h = 1e-4 the difference is
        # 3.8e-7, the bound 1.8e-4, |w'dx| 5.70.  Measured on the MI355X: difference 3.8e-7, bound 1.9e-4.
        h = 1e-4
        x, y = layer(torch.from_numpy(p["q"].copy()))
        sol = dict(x=x.numpy().copy(), y=y.numpy().copy())
        rc, msg, o = raw_tangent(qp, t)
        assert rc == 0, msg
        assert check_rhs(p, sol, o, 0, t, "first-order check") == (0, 1)
        flags = o["active"]
        Ad = ref.dense(p["A"])
        Qd = ref.full_Q(p["Q"], p["Qstype"])
        rvx, rvy, M, S = ref.adjoint(Qd, Ad, flags, w.astype(ref.LD), None)
        rh = sref.tangent_rhs(p["Q"], p["Qstype"], p["A"], flags, sol["x"], sol["y"], **t)
        d = np.concatenate([o["dx"][0].astype(ref.LD), o["dy"][0].astype(ref.LD)[S]])
        rbound = TOL * float(np.abs(np.concatenate([rh["rx"], rh["ry"]])).max()) + (n + len(S) + 2) * EPS * float((np.abs(M) @ np.abs(d)).max()) \
            + (rh["L"] + 2) * EPS * float(rh["T"].max())
        minv = float(np.abs(np.linalg.inv(M.astype(np.float64))).sum(axis=1).max())
        anorm = float(np.abs(Ad.astype(np.float64)).sum(axis=0).max())
        v1x, v1y = float(np.abs(rvx).sum()), float(np.abs(rvy).sum())
        L, dL = [], 0.0
        for sgn in (1.0, -1.0):
            lj, uj = p["l"] + sgn * h * t["tl"], p["u"] + sgn * h * t["tu"]
            plain = WorkspaceQP(qp)
            xs, ys = plain(torch.from_numpy(p["q"] + sgn * h * t["tq"]), torch.from_numpy(lj), torch.from_numpy(uj))
            assert plain.status == 1
            assert np.array_equal(ref.classify(xs.numpy(), ys.numpy(), Ad, lj, uj), flags), "the step h moved the active set"
            info = qp.info()
            dL += v1x * (info["res_dual_norm"] + anorm * info["res_prim_norm"]) + v1y * info["res_prim_norm"]
            L.append(float(w @ xs.numpy()))
        fd = (L[0] - L[1]) / (2 * h)
        wdx = float(w @ o["dx"][0])
        bound = dL / (2 * h) + np.abs(w).sum() * 2.0 * minv * rbound
        diff = abs(fd - wdx)
        print("first order: w'dx %.12e, central difference %.12e, |difference| %.3e, bound %.3e, |difference| / bound = %.3e" % (wdx, fd, diff, bound, diff / bound))
        assert bound <= 1e-2 * abs(float(w.astype(ref.LD) @ sref.tangent(Qd, Ad, flags, rh["rx"], rh["ry"])[0])), ("the check would be vacuous", bound)
        assert diff <= bound, (fd, wdx, bound)
    finally:
        qp.delete()


def test_workspace_qp_layer_when_the_solve_is_not_solved(monkeypatch):
    """a forward that runs out of passes (max_iter = 2): tangent and vjp_many make no library call and give NaN, or zeros under "zero" (code 2)"""
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    p = problem("n40")
    qp = workspace(monkeypatch, p, "dense", 10, max_iter=2)
    try:
        for mode in ("nan", "zero"):
            layer = WorkspaceQP(qp, on_failure=mode)
            layer(torch.from_numpy(p["q"].copy()))
            assert layer.status == -5
            out = layer.tangent(tq=torch.ones((2, p["n"]), dtype=torch.float64))
            assert layer.tangent_status.tolist() == [[2, 0, 0]] * 2 and out["dx"].shape == (2, p["n"]) and out["dy"].shape == (2, p["m"])
            vj = layer.vjp_many(torch.ones(p["n"], dtype=torch.float64))
            assert layer.vjp_status.tolist() == [2, 0, 0] and vj["dq"].shape == (p["n"],)
            assert qp.tangent_stats()["calls"] == 0 and qp.adjoint_stats()["calls"] == 0
            for g in (out["dx"].numpy(), out["dy"].numpy(), vj["dq"].numpy(), vj["du"].numpy()):
                assert np.isnan(g).all() if mode == "nan" else not bits(g).any(), mode
    finally:
        qp.delete()
