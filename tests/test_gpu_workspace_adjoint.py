"""The workspace adjoint (qpdo_amd_adjoint, solver.QPDO.adjoint, qpdo_amd.torch_layer.WorkspaceQP; include/qpdo_amd_ext.h)
on the MI355X, in this process: dense LDL' workspaces (one 64-tile; ld = 192 with a ragged last tile), a workspace whose qpdo_solve ran as
the fused one-launch kernel, band LDL' workspaces, m = 0; with and without scaling; Q stored as the lower triangle, the upper triangle
and in full.

The acceptance rules are those of the fleet's adjoint test, IMPORTED from tests/_fleet_adjoint_worker.py (check_item, check_matrices) and
tests/fleet_adjoint_ref.py: everything is checked against the DEVICE's flags -- the longdouble residual of the unscaled system is at most
tol max(||gx||, ||gy_S||) + (n + k + 2) eps || |M| |v| ||_inf; where cond(M) < 1 / eps the error against solve_ref is at most 2 ||M^-1||_inf
times that; the flags equal classify() on every row whose margin is >= 1e-9 (at most 1 % of the rows may be below it); dQ / dA are within 4 eps
of the per-entry term sums; entries off the set are a bitwise +0.0.  Every output array is pre-filled with a sentinel, so an entry the call
never wrote is seen.  0 <= sweeps <= 20 is asserted as the fleet test asserts it."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fleet_adjoint_ref as ref
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QPDO_LINSOLVE", "QPDO_DENSE_MID", "QPDO_DENSE_LOOKAHEAD", "QPDO_DENSE_SOLVE", "QPDO_DENSE_LOWRANK", "QPDO_DENSE_UPDOWN", "QPDO_HYBRID",
            "QPDO_DENSE_MAX_N", "QPDO_SMALL_FUSED", "QPDO_BAND_COUPLING")
TOL = 1e-9
SENTINEL = 12345.678
TIMING = ("setup_time", "solve_time", "run_time", "spmv_Q_avg_s", "spmv_Ac_time_s", "fused_kernel_s")


@pytest.fixture(scope="module")
def W():
    """tests/_fleet_adjoint_worker.py (check_item, check_matrices, dup_item): imported when the first test runs, the library loaded before it"""
    solver.lib()
    import _fleet_adjoint_worker as w
    return w


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


PROBLEMS = {
    "n40": lambda: problems.random_qp(4, 40, 60, 0.3, n_eq=4),
    "n130": lambda: problems.random_qp(3, 130, 200, 0.15, n_eq=10),
    "band72": lambda: problems.banded_random_qp(5, 72, 5),
    "band96": lambda: problems.banded_qp(6, 96),
}
_cache = {}


def problem(name):
    if name not in _cache:
        _cache[name] = PROBLEMS[name]()
    return _cache[name]


def with_storage(p, stype):
    """the same QP with Q stored as the lower triangle (-1), the upper triangle (+1) or in full (0)"""
    Qf = problems.full_Q(p)
    Q = sp.tril(Qf) if stype < 0 else sp.triu(Qf) if stype > 0 else Qf
    Q = sp.csc_matrix(Q); Q.sort_indices()
    return dict(p, Q=Q, Qstype=stype)


def workspace(monkeypatch, p, linsolve, scaling, **kw):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if linsolve:
        monkeypatch.setenv("QPDO_LINSOLVE", linsolve)
    return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), scaling=scaling, verbose=0,
                               max_iter=kw.pop("max_iter", 1000), **kw)


def raw_adjoint(qp, gx, gy=None, matrices=False, tol=TOL, max_sweeps=20, Qview=None):
    """qpdo_amd_adjoint with every output pre-filled with a sentinel; returns (rc, message, outputs)"""
    gx = np.ascontiguousarray(gx, np.float64)
    R = 1 if gx.ndim == 1 else gx.shape[0]
    gy = None if gy is None else np.ascontiguousarray(gy, np.float64)
    nq, na = len(qp._Qview_keep[2]), len(qp._Apat[1])
    o = dict(dq=np.full((R, qp.n), SENTINEL), dl=np.full((R, qp.m), SENTINEL), du=np.full((R, qp.m), SENTINEL),
             dQ_values=np.full((R, nq), SENTINEL) if matrices else None, dA_values=np.full((R, na), SENTINEL) if matrices else None,
             active=np.full(qp.m, 77, np.int32), status=np.full((R, 3), -77, np.int64), residual=np.full(R, SENTINEL))
    dp = solver._as_dp
    Qv = Qview if Qview is not None else qp._Qview
    rc = solver.lib().qpdo_amd_adjoint(qp._w, R, dp(gx), dp(gy), dp(o["dq"]), dp(o["dl"]), dp(o["du"]), C.byref(Qv) if matrices else None, dp(o["dQ_values"]),
                                       dp(o["dA_values"]), o["active"].ctypes.data_as(C.POINTER(C.c_int)), o["status"].ctypes.data_as(C.POINTER(C.c_long)),
                                       dp(o["residual"]), float(tol), int(max_sweeps))
    return rc, (solver.lib().qpdo_amd_last_error() or b"").decode(), o


def untouched(o):
    return all((v == (77 if k == "active" else -77 if k == "status" else SENTINEL)).all() for k, v in o.items() if v is not None)


def check_rhs(W, p, sol, o, r, gx, gy, matrices, what, accept=(0,)):
    """every check of right-hand side r of one call; returns its code"""
    code, sweeps, k = o["status"][r].tolist()
    sl = [o["dq"][r], o["dl"][r], o["du"][r]] + ([o["dQ_values"][r], o["dA_values"][r]] if matrices else [])
    flags = o["active"]
    assert code in accept, (what, code, sweeps)
    assert set(np.unique(flags)) <= {-1, 0, 1} and k == int((flags != 0).sum()), (what, "flags", k)
    if code != 0:
        assert all(np.isnan(s).all() for s in sl) and np.isnan(o["residual"][r]), (what, "NaN slices")
        return code
    assert not any(np.isnan(s).any() for s in sl) and all((s != SENTINEL).all() for s in sl), (what, "NaN or an unwritten entry")
    assert o["residual"][r] <= TOL and 0 <= sweeps <= 20, (what, o["residual"][r], sweeps)
    x, y = sol["x"], sol["y"]
    l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
    if p["m"]:
        mg = ref.margins(x, y, p["A"], l, u)
        sure = mg >= 1e-9
        assert (flags[sure] == ref.classify(x, y, ref.dense(p["A"]), l, u)[sure]).all(), (what, "flags against classify")
        assert int((~sure).sum()) <= 0.01 * p["m"], (what, "rows below the margin", int((~sure).sum()))
    vx, vy = W.check_item(p, x, y, flags, sl[0], sl[1], sl[2], gx, gy, TOL, what)
    if matrices:
        W.check_matrices(p, x, y, flags, vx, vy, sl[3], sl[4], what)
    print("%s: code 0, %d sweeps, k = %d, residual %.2e" % (what, sweeps, k, o["residual"][r]))
    return code


def solve_and_check(W, monkeypatch, p, linsolve, scaling, what, expect_linsolve):
    qp = workspace(monkeypatch, p, linsolve, scaling)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1 and qp.stats()["linsolve"] == expect_linsolve, (what, sol["info"], qp.stats()["linsolve"])
        rng = np.random.default_rng(100 + scaling)
        gx = rng.standard_normal(p["n"])
        rc, msg, o = raw_adjoint(qp, gx, None, matrices=True)
        assert rc == 0, msg
        check_rhs(W, p, sol, o, 0, gx, None, True, what + " gy=None")
        flags = o["active"].copy()
        # a random gy with NaN on every inactive row: NaN must not reach the result (none of these problems has dependent active rows: code 0)
        gy = rng.standard_normal(p["m"])
        gy[flags == 0] = np.nan
        rc, msg, o2 = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        assert np.array_equal(o2["active"], flags)
        check_rhs(W, p, sol, o2, 0, gx, gy, True, what + " gy")
        st = qp.adjoint_stats()
        assert (st["calls"], st["rhs_total"], st["factorizations"]) == (2, 2, 2) and st["scratch_bytes"] > 0 and st["last_seconds"] > 0
        # the wrapper delivers the raw call's bits
        w = qp.adjoint(gx, None, matrices=True, tol=TOL)
        for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
            assert same_bits(w[k], o[k][0]), (what, k)
        assert np.array_equal(w["active"], flags) and w["status"].tolist() == o["status"][0].tolist()
    finally:
        qp.delete()


@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", ["n40", "n130"])
def test_dense(W, monkeypatch, name, scaling):
    solve_and_check(W, monkeypatch, problem(name), "dense", scaling, "dense %s[%d]" % (name, scaling), 1)


@pytest.mark.parametrize("scaling", [10, 0])
def test_fused_route_workspace(W, monkeypatch, scaling):
    """no QPDO_LINSOLVE: qpdo_solve ran as ONE launch of the fused kernel (stats: linsolve 2); the adjoint reads nothing of the iterate state"""
    solve_and_check(W, monkeypatch, problem("n40"), None, scaling, "fused n40[%d]" % scaling, 2)


@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", ["band72", "band96"])
def test_band(W, monkeypatch, name, scaling):
    solve_and_check(W, monkeypatch, problem(name), "band", scaling, "band %s[%d]" % (name, scaling), 3)


@pytest.mark.parametrize("stype", [1, 0])
@pytest.mark.parametrize("name", ["n40", "n130"])
def test_dense_Q_stored_upper_and_full(W, monkeypatch, name, stype):
    """(the lower triangle is what test_dense runs)"""
    solve_and_check(W, monkeypatch, with_storage(problem(name), stype), "dense", 10, "dense %s stype %d" % (name, stype), 1)


def test_no_rows(W, monkeypatch):
    """m = 0: Q vx = gx with a strictly convex Q of n = 40"""
    rng = np.random.default_rng(2)
    n = 40
    B = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.2)
    Q = sp.csc_matrix(np.tril(B @ B.T + n * np.eye(n))); Q.sort_indices()
    p = dict(n=n, m=0, Q=Q, Qstype=-1, A=sp.csc_matrix((0, n)), q=rng.standard_normal(n), l=np.zeros(0), u=np.zeros(0), c=0.0)
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        gx = rng.standard_normal(n)
        rc, msg, o = raw_adjoint(qp, gx, None, matrices=True)
        assert rc == 0, msg
        assert check_rhs(W, p, sol, o, 0, gx, None, True, "m = 0") == 0 and o["status"][0, 2] == 0
    finally:
        qp.delete()


@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_many_right_hand_sides(W, monkeypatch, name, linsolve):
    """R = 3 on one factorization: every slab carries the bits of the single call with that gx / gy; the same call twice, the same bits"""
    p = problem(name)
    qp = workspace(monkeypatch, p, linsolve, 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        rng = np.random.default_rng(17)
        gx = rng.standard_normal((3, p["n"]))
        rc, msg, o0 = raw_adjoint(qp, gx[0])
        assert rc == 0, msg
        gy = rng.standard_normal((3, p["m"]))
        gy[:, o0["active"] == 0] = np.nan
        gy[1, o0["active"] != 0] = 0.0
        f0 = qp.adjoint_stats()["factorizations"]
        rc, msg, many = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        assert qp.adjoint_stats()["factorizations"] == f0 + 1 and qp.adjoint_stats()["rhs_total"] == 4
        rc, msg, again = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        for k, v in many.items():
            assert np.array_equal(bits(v), bits(again[k])) if v.dtype == np.float64 else np.array_equal(v, again[k]), (k, "the same call twice")
        codes = []
        for r in range(3):
            rc, msg, one = raw_adjoint(qp, gx[r], gy[r], matrices=True)
            assert rc == 0, msg
            for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
                assert same_bits(many[k][r], one[k][0]), (name, r, k)
            assert many["status"][r].tolist() == one["status"][0].tolist() and np.array_equal(many["active"], one["active"])
            codes.append(check_rhs(W, p, sol, many, r, gx[r], gy[r], True, "%s R=3 slab %d" % (name, r)))
        assert codes == [0, 0, 0], codes
    finally:
        qp.delete()


def test_not_accepted(W, monkeypatch):
    """two identical active rows: consistent for gy = None, not for a gy that differs on them (code 1, NaN slices, the flags delivered)"""
    p = W.dup_item()
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        gx = np.random.default_rng(3).standard_normal(p["n"])
        gy = np.zeros(p["m"])
        gy[0], gy[1] = 1.0, -1.0
        rc, msg, bad = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        assert bad["status"][0, :2].tolist() == [1, 20] and bad["active"][0] != 0 and bad["active"][1] != 0, bad["status"].tolist()
        check_rhs(W, p, sol, bad, 0, gx, gy, True, "inconsistent gy", accept=(1,))
        rc, msg, ok = raw_adjoint(qp, gx, None, matrices=True)
        assert rc == 0, msg
        check_rhs(W, p, sol, ok, 0, gx, None, True, "gy=None")
        assert np.array_equal(ok["active"], bad["active"])
        # ONE call with three right-hand sides: code 0, code 1, code 0 -- a right-hand side that is not accepted touches no other one
        gx3 = np.stack([gx, gx, 2.0 * gx])
        gy3 = np.stack([np.zeros(p["m"]), gy, np.zeros(p["m"])])
        rc, msg, mix = raw_adjoint(qp, gx3, gy3, matrices=True)
        assert rc == 0 and mix["status"][:, 0].tolist() == [0, 1, 0] and mix["status"][1, 1] == 20, (msg, mix["status"].tolist())
        for r in range(3):
            check_rhs(W, p, sol, mix, r, gx3[r], gy3[r], True, "mixed call, right-hand side %d" % r, accept=((1,) if r == 1 else (0,)))
        for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
            assert same_bits(mix[k][1], bad[k][0]) or np.isnan(mix[k][1]).all(), k
        rc, msg, last = raw_adjoint(qp, gx3[2], gy3[2], matrices=True)
        assert rc == 0, msg
        for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
            assert same_bits(mix[k][2], last[k][0]), (k, "the right-hand side behind a code 1 carries the single call's bits")
    finally:
        qp.delete()


def snapshot(qp, res):
    info = {k: v for k, v in res["info"].items() if k not in TIMING}
    stats = {k: v for k, v in qp.stats().items() if k not in TIMING}
    trace = [tuple(bits(np.array([float(v)]))[0] for v in t.values()) for t in qp.trace()]
    return dict(x=bits(res["x"]).tolist(), y=bits(res["y"]).tolist(), info={k: (bits(np.array([v]))[0] if isinstance(v, float) else v) for k, v in info.items()},
                stats={k: (bits(np.array([v]))[0] if isinstance(v, float) else v) for k, v in stats.items()}, trace=trace)


@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_no_bit_moves(monkeypatch, name, linsolve):
    """two workspaces on one problem, adjoint calls on X only: every later solve of X carries Y's bits -- x, y, every info field but the
    wall times, every trace record, every QPDOAmdStats member but the event timings"""
    p = problem(name)
    X, Y = workspace(monkeypatch, p, linsolve, 10), workspace(monkeypatch, p, linsolve, 10)
    try:
        rng = np.random.default_rng(5)
        gx, gy = rng.standard_normal((2, p["n"])), rng.standard_normal((2, p["m"]))
        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b)
        rc, msg, o = raw_adjoint(X, gx, gy, matrices=True)
        assert rc == 0 and (o["status"][:, 0] != 3).all(), (msg, o["status"].tolist())
        assert snapshot(X, a)["stats"] == snapshot(Y, b)["stats"], "QPDOAmdStats after the adjoint call"
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "the solve after the adjoint call"
        rc, msg, o = raw_adjoint(X, gx[0])
        assert rc == 0, msg
        for S in (X, Y):
            S.update_q(1.5 * p["q"] + 0.1)
            S.warm_start(a["x"], a["y"])
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "update_q, warm_start, solve"
        assert X.adjoint_stats()["calls"] == 2 and Y.adjoint_stats()["calls"] == 0
    finally:
        X.delete(); Y.delete()


def test_refusals(monkeypatch):
    """each: nonzero return, a message that names the reason, the sentinel outputs untouched, `calls` unmoved"""
    p = problem("n40")
    gx = np.ones(p["n"])

    def refused(qp, msg_part, **kw):
        before = qp.adjoint_stats()
        rc, msg, o = raw_adjoint(qp, kw.pop("gx", gx), **kw)
        assert rc != 0 and msg_part in msg, (msg_part, rc, msg)
        assert untouched(o), msg_part
        assert qp.adjoint_stats() == before, msg_part

    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        refused(qp, "status is not QPDO_SOLVED")                               # before any solve
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        rc, msg, o = raw_adjoint(qp, gx)
        assert rc == 0 and o["status"][0, 0] == 0 and qp.adjoint_stats()["calls"] == 1, msg
        qp.update_q(p["q"] * 1.25)
        refused(qp, "was not a solve")                                         # after update_q
        qp.solve()
        qp.warm_start(sol["x"], sol["y"])
        refused(qp, "was not a solve")                                         # after warm_start
        qp.solve()
        qp.update_bounds(p["l"] - 0.5, p["u"] + 0.5)
        refused(qp, "was not a solve")                                         # after update_bounds
        qp.solve()
        # dQx with a Q of another pattern (the same stype, shape, entry count and column pointers: the device comparison finds it)
        Q2 = sp.csc_matrix(p["Q"]).copy(); Q2.sort_indices()
        ind = Q2.indices.copy()
        j = next(j for j in range(p["n"]) if Q2.indptr[j + 1] > Q2.indptr[j] and ind[Q2.indptr[j + 1] - 1] < p["n"] - 1)
        ind[Q2.indptr[j + 1] - 1] += 1
        keep = []
        view = solver._sparse_view(sp.csc_matrix((Q2.data, ind, Q2.indptr), shape=Q2.shape), p["Qstype"], keep)
        refused(qp, "pattern of Q differs", matrices=True, Qview=view)
        rc, msg, o = raw_adjoint(qp, gx, matrices=True)                         # ... and the setup's own pattern passes
        assert rc == 0 and o["status"][0, 0] == 0, msg
    finally:
        qp.delete()
    k = problems.infeasibility_kat("primal_infeasible")
    qp = workspace(monkeypatch, k, "dense", 10, max_iter=k["max_iter"])
    try:
        assert qp.solve()["info"]["status_val"] == -3
        refused(qp, "status is not QPDO_SOLVED", gx=np.ones(k["n"]))
    finally:
        qp.delete()
    qp = workspace(monkeypatch, p, "pcg", 10)
    try:
        assert qp.solve()["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 0
        refused(qp, "the workspace's solver is PCG")
        refused(qp, "QPDO_LINSOLVE=dense")
    finally:
        qp.delete()


def test_workspace_qp_layer(W, monkeypatch):
    """WorkspaceQP: backward equals the direct call bit for bit; which inputs get gradients; "zero"; the stale backward; one
    finite-difference spot check of dL/dq against two extra solves"""
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    p = problem("n40")
    qp = workspace(monkeypatch, p, "dense", 0, eps_abs=1e-9, max_iter=10000)
    try:
        Qp = sp.csc_matrix(p["Q"]); Qp.sort_indices()
        Ap = sp.csc_matrix(p["A"]); Ap.sort_indices()
        rng = np.random.default_rng(21)
        w, z = rng.standard_normal(p["n"]), rng.standard_normal(p["m"])
        wt, zt = torch.from_numpy(w), torch.from_numpy(z)

        def leaves(req, q=None):
            vals = [p["q"] if q is None else q, p["l"], p["u"], Qp.data, Ap.data]
            return [torch.from_numpy(np.array(v, np.float64)).requires_grad_(r) for v, r in zip(vals, req)]

        def loss_of(x, y):
            return (wt * x).sum() + (zt * torch.nan_to_num(y)).sum()

        layer = WorkspaceQP(qp)
        t = leaves([True] * 5)
        x, y = layer(*t)
        assert layer.status == 1
        loss_of(x, y).backward()
        direct = qp.adjoint(w, z, matrices=True)
        assert direct["status"][0] == 0 and layer.adjoint_status.tolist() == direct["status"].tolist()
        for v, k in zip(t, ("dq", "dl", "du", "dQ_values", "dA_values")):
            assert same_bits(v.grad.numpy(), direct[k]), k
        sol = dict(x=x.detach().numpy(), y=y.detach().numpy())
        o = {k: (None if v is None else v[None]) for k, v in direct.items() if k != "active"}
        o["active"] = direct["active"]
        check_rhs(W, p, sol, o, 0, w, z, True, "WorkspaceQP backward")
        # inputs that do not require a gradient get none
        t2 = leaves([True, False, False, False, True])
        x, y = layer(*t2)
        loss_of(x, y).backward()
        assert t2[0].grad is not None and t2[4].grad is not None and all(v.grad is None for v in t2[1:4])
        # "zero": an adjoint that is not delivered (max_sweeps = 1 at a tolerance no single sweep reaches) gives zeros, not NaN
        lz = WorkspaceQP(qp, on_failure="zero", tol=1e-300, max_sweeps=1)
        t3 = leaves([True] * 5)
        x, y = lz(*t3)
        loss_of(x, y).backward()
        assert lz.adjoint_status[0] == 1 and all(not bits(v.grad.numpy()).any() for v in t3)
        ln = WorkspaceQP(qp, on_failure="nan", tol=1e-300, max_sweeps=1)
        t3 = leaves([True] * 5)
        x, y = ln(*t3)
        loss_of(x, y).backward()
        assert ln.adjoint_status[0] == 1 and all(np.isnan(v.grad.numpy()).all() for v in t3)
        # a backward that belongs to an earlier forward
        t4 = leaves([True] * 5)
        x1, y1 = layer(*t4)
        x2, y2 = layer(*t4)
        with pytest.raises(RuntimeError, match="solved again since this forward"):
            loss_of(x1, y1).backward()
        loss_of(x2, y2).backward()
        dqw = qp.adjoint(w, None)                  # (of L = w'x alone, at the solution of the last forward)
        assert dqw["status"][0] == 0 and np.array_equal(dqw["active"], direct["active"])
        # ---- finite differences of L = w'x in q_j.  With the active set fixed the solution map is LINEAR in q, so a central difference has
        # no truncation term, and what is left is the two solves' error over 2 h.  A solve that ends with the unscaled residuals (rp, rd)
        # of its info (scaling 0) satisfies the KKT system of its active set with a residual vector r: |r| <= rd + ||A'||_inf rp in the
        # stationarity rows (the multipliers of inactive rows are bounded by rp each) and <= rp in the active rows.  Its error in L is
        # w' dx = <M^-1 (w; 0), r> = <(vx, vy_S), r>, so |dL| <= ||vx||_1 (rd + ||A'||_inf rp) + ||vy_S||_1 rp, with (vx, vy) the REFERENCE's
        # adjoint solution (longdouble, tests/fleet_adjoint_ref.py) for the device's flags -- not the output under test.  To that the
        # adjoint's own error bound 2 ||M^-1||_inf tol ||w||_inf is added, which check_item asserted above.  Measured on the CPU oracle
        # (eps_abs 1e-9, h = 1e-4, j = 3): difference 1.3e-7, bound 1.8e-4, |dq_j| 0.39.
        h, j = 1e-4, 3
        flags = direct["active"]
        Ad = ref.dense(p["A"])
        rvx, rvy, M, S = ref.adjoint(ref.full_Q(p["Q"], p["Qstype"]), Ad, flags, w.astype(ref.LD), None)
        minv = float(np.abs(np.linalg.inv(M.astype(np.float64))).sum(axis=1).max())
        anorm = float(np.abs(Ad.astype(np.float64)).sum(axis=0).max())
        v1x, v1y = float(np.abs(rvx).sum()), float(np.abs(rvy).sum())
        L, dL = [], 0.0
        for sgn in (1.0, -1.0):
            qj = p["q"].copy(); qj[j] += sgn * h
            plain = WorkspaceQP(qp)
            xs, ys = plain(torch.from_numpy(qj))
            assert plain.status == 1
            assert np.array_equal(ref.classify(xs.numpy(), ys.numpy(), Ad, p["l"], p["u"]), flags), "the step h moved the active set"
            info = qp.info()
            dL += v1x * (info["res_dual_norm"] + anorm * info["res_prim_norm"]) + v1y * info["res_prim_norm"]
            L.append(float(w @ xs.numpy()))
        fd = (L[0] - L[1]) / (2 * h)
        bound = dL / (2 * h) + 2.0 * minv * TOL * np.abs(w).max()
        diff = abs(fd - dqw["dq"][j])
        print("finite differences of dL/dq[%d]: adjoint %.12e, central difference %.12e, |difference| %.3e, bound %.3e, |difference| / bound = %.3e"
              % (j, dqw["dq"][j], fd, diff, bound, diff / bound))
        assert bound <= 1e-2 * abs(float(rvx[j])), ("the check would be vacuous", bound, float(rvx[j]))
        assert diff <= bound, (fd, dqw["dq"][j], bound)
    finally:
        qp.delete()


def test_workspace_qp_layer_when_the_solve_is_not_solved(monkeypatch):
    """a forward that runs out of passes (max_iter = 2): backward makes no adjoint call and gives NaN, or zeros under "zero" (FleetQP's code 2)"""
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    p = problem("n40")
    qp = workspace(monkeypatch, p, "dense", 10, max_iter=2)
    try:
        for mode in ("nan", "zero"):
            layer = WorkspaceQP(qp, on_failure=mode)
            q = torch.from_numpy(p["q"].copy()).requires_grad_(True)
            u = torch.from_numpy(p["u"].copy()).requires_grad_(True)
            x, y = layer(q, None, u)
            assert layer.status == -5
            (torch.nan_to_num(x).sum() + torch.nan_to_num(y).sum()).backward()
            assert layer.adjoint_status.tolist() == [2, 0, 0] and qp.adjoint_stats()["calls"] == 0
            for g in (q.grad.numpy(), u.grad.numpy()):
                assert np.isnan(g).all() if mode == "nan" else not bits(g).any(), mode
    finally:
        qp.delete()
