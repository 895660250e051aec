"""The fleet's adjoint call (qpdo_amd_fleet_adjoint_dev, include/qpdo_amd_ext.h) where no device is needed: the reference the GPU tests lean
on (tests/fleet_adjoint_ref.py) is pinned against central differences -- of the longdouble-solved KKT system for the formulas, of two CPU
oracle solves for the active-set rule --, the new calls on a NULL fleet are refused under their own names, Fleet.adjoint_device validates its
tensors before any library call, FleetQP rejects an unknown on_failure, and the C-side checks run again from a compiled C program with the
host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import fleet_adjoint_ref as ref
from oracle import binding as ob
from qpdo_amd import _build, problems, solver

LD = np.longdouble


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------
def tiny_qp(seed, stype):
    """strictly convex Q (n = 5) in the storage of `stype`, m = 4 rows of which row 0 is upper-active and row 2 lower-active, by decree"""
    rng = np.random.default_rng(seed)
    n, m = 5, 4
    B = rng.standard_normal((n, n))
    Qf = B @ B.T + n * np.eye(n)
    Q = sp.csc_matrix(Qf if stype == 0 else (np.tril(Qf) if stype < 0 else np.triu(Qf)))
    Q.sort_indices()
    A = sp.csc_matrix(rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.8))
    A.sort_indices()
    flags = np.array([1, 0, -1, 0], np.int32)
    return dict(n=n, m=m, Q=Q, Qstype=stype, A=A, q=rng.standard_normal(n), l=rng.standard_normal(m) - 1.0, u=rng.standard_normal(m) + 1.0), flags


def kkt_solution(p, flags, Qdata=None, Adata=None, q=None, l=None, u=None):
    """x, y (all m rows, 0 off S) of  Qx + q + A_S' y_S = 0,  A_S x = b_S  (b: u on +1 rows, l on -1 rows), solved in longdouble"""
    Q, A = p["Q"], p["A"]
    Qd = np.zeros(Q.shape, LD); Ad = np.zeros(A.shape, LD)
    qa, qb = Q.indices, np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    Qd[qa, qb] = p["Q"].data.astype(LD) if Qdata is None else Qdata
    if p["Qstype"] != 0:
        Qd = Qd + Qd.T - np.diag(np.diag(Qd))
    ai, aj = A.indices, np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    Ad[ai, aj] = p["A"].data.astype(LD) if Adata is None else Adata
    q = p["q"].astype(LD) if q is None else q
    l = p["l"].astype(LD) if l is None else l
    u = p["u"].astype(LD) if u is None else u
    M, S = ref.kkt(Qd, Ad, flags)
    b = np.where(flags[S] > 0, u[S], l[S])
    v, _ = ref.solve_ref(M, np.concatenate([-q, b]))
    y = np.zeros(p["m"], LD); y[S] = v[p["n"]:]
    return v[:p["n"]], y, Qd, Ad


@pytest.mark.parametrize("stype", [-1, 1, 0])
def test_the_formulas_equal_central_differences(stype):
    """gradients() against central differences of the longdouble KKT solution with respect to every q_j, l_i, u_i, stored Q entry and stored
    A entry.  The solution map is linear in q, l, u (exact up to rounding); for Q, A the truncation term is O(h^2): h = 1e-5, relative 1e-7.
    (A stored off-diagonal entry of a full-storage Q is perturbed on its own: the formula of stype 0 is the derivative with respect to that
    one stored value, the matrix the solver sees being whatever is stored.)"""
    p, flags = tiny_qp(40 + stype, stype)
    rng = np.random.default_rng(7)
    gx, gy = rng.standard_normal(p["n"]).astype(LD), rng.standard_normal(p["m"]).astype(LD)
    x, y, Qd, Ad = kkt_solution(p, flags)
    if stype == 0:
        Qd = (Qd + Qd.T) / 2
    vx, vy, _, _ = ref.adjoint(Qd, Ad, flags, gx, gy)
    g = ref.gradients(p["Q"], stype, p["A"], flags, x, y, vx, vy)
    S = flags != 0

    def loss(**kw):
        xs, ys, _, _ = kkt_solution(p, flags, **kw)
        return gx @ xs + gy[S] @ ys[S]

    h = LD(1e-5)

    def cd(name, base, k):
        e = np.zeros(len(base), LD); e[k] = h
        return (loss(**{name: base + e}) - loss(**{name: base - e})) / (2 * h)

    scale = max(float(np.abs(v).max()) for v in g.values() if len(v))
    for name, key, base in (("q", "dq", p["q"].astype(LD)), ("l", "dl", p["l"].astype(LD)), ("u", "du", p["u"].astype(LD)),
                            ("Qdata", "dQ_values", p["Q"].data.astype(LD)), ("Adata", "dA_values", p["A"].data.astype(LD))):
        num = np.array([cd(name, base, k) for k in range(len(base))], LD)
        assert len(num) == len(g[key])
        assert float(np.abs(num - g[key]).max()) <= 1e-7 * scale, (name, float(np.abs(num - g[key]).max()), scale)
    assert np.array_equal(g["dl"] != 0, flags < 0) and np.array_equal(g["du"] != 0, flags > 0)


def test_classify_and_margins():
    A = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, -1.0]])
    x, y = np.array([1.0, 2.0]), np.array([0.5, -0.5, 0.0, 0.0])
    l, u = np.array([-1e20, 1.5, 3.0, -1.0]), np.array([1.5, 1e20, 3.0, 1e20])
    #   t =  1.5 (>= u)   1.5 (<= l)   3 (l = u: active)   -1 (<= l)
    assert ref.classify(x, y, A, l, u).tolist() == [1, -1, 1, -1]
    assert ref.classify(x, np.zeros(4), A, l, u).tolist() == [0, 0, 1, -1]
    assert ref.classify(x, np.array([1e30, -1e30, 0, 0]), A, np.full(4, -1e20), np.full(4, 1e20)).tolist() == [0, 0, 0, 0]      # never reached
    assert np.allclose(ref.margins(x, np.zeros(4), A, l, u), [0.5 / 2.5, 0.5 / 2.5, 0.0, 0.0]) and np.isinf(ref.margins(x, y, A, np.full(4, -1e20), np.full(4, 1e20))).all()


# ---- the active-set rule against two oracle solves ----------------------------------------------------------------------------------------
def oracle_solution(p, eps):
    o = ob.OracleSolver(p, ob.default_settings(eps_abs=eps, max_iter=10000))
    r = o.solve()
    o.close()
    return r["info"]["status_val"], r["x"], r["y"]


def directional_discrepancy(p, h, seed=0):
    """|predicted - central difference| / |predicted| of d/dt L(x(t), y(t)) at t = 0 along a random (dq, dl, du), L = w'x + z'y, the QPs solved by
    the CPU oracle at the tightest eps_abs (a power of ten) at which all solves involved reach status 1"""
    rng = np.random.default_rng(seed)
    n, m = p["n"], p["m"]
    w, z = rng.standard_normal(n), rng.standard_normal(m)
    dq, dl, du = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    eq = p["l"] == p["u"]
    du[eq] = dl[eq]                                          # an equality row stays one
    fin_l, fin_u = np.abs(p["l"]) < 1e20, np.abs(p["u"]) < 1e20
    moved = lambda t: dict(p, q=p["q"] + t * dq, l=np.where(fin_l, p["l"] + t * dl, p["l"]), u=np.where(fin_u, p["u"] + t * du, p["u"]))
    for eps in (1e-13, 1e-12, 1e-11, 1e-10, 1e-9):
        sols = [oracle_solution(moved(t), eps) for t in (0.0, h, -h)]
        if all(s[0] == 1 for s in sols):
            break
    else:
        raise AssertionError("the oracle does not reach status 1")
    (_, x, y), (_, xp, yp), (_, xm, ym) = sols
    flags = ref.classify(x, y, ref.dense(p["A"]), p["l"], p["u"])
    assert ref.margins(x, y, p["A"], p["l"], p["u"]).min() >= 1e-6      # no row sits on the fence
    vx, vy, _, _ = ref.adjoint(ref.full_Q(p["Q"], p["Qstype"]), p["A"], flags, w, z)
    g = ref.gradients(p["Q"], p["Qstype"], p["A"], flags, x, y, vx, vy)
    pred = float(g["dq"] @ dq + g["dl"] @ dl + g["du"] @ du)
    S = flags != 0
    num = float((w @ (xp - xm) + z[S] @ (yp - ym)[S]) / (2 * h))
    return abs(pred - num) / abs(pred), eps


@pytest.mark.parametrize("which", ["random_qp", "C3"])
def test_the_active_set_rule_predicts_the_oracles_directional_derivative(which):
    """Measured (relative discrepancy at h = 1e-5 and at h / 2; DISCREPANCY below, docs/LAB_NOTES.md):
        random_qp(23, 40, 60, 0.2, 10)   4.404e-11   4.568e-10   (oracle at eps_abs 1e-13)
        C3 item 5                        4.230e-05   8.295e-05   (oracle at eps_abs 1e-10, the tightest it reaches in 10000 passes)
    Both grow as h shrinks: what is left is the solves' own error over h (eps_abs / h), not a truncation or a modelling term.  Asserted with a
    margin of ten times the larger of the two."""
    p = problems.random_qp(23, 40, 60, 0.2, 10) if which == "random_qp" else problems.config_qp("C3", 5)
    d1, eps1 = directional_discrepancy(p, 1e-5)
    d2, eps2 = directional_discrepancy(p, 0.5e-5)
    print("directional discrepancy %s: %.3e (h = 1e-5, eps_abs %g), %.3e (h / 2, eps_abs %g)" % (which, d1, eps1, d2, eps2))
    assert max(d1, d2) <= 10 * max(DISCREPANCY[which]), (d1, d2)


# measured with the CPU oracle: relative discrepancy at h = 1e-5 and at h / 2
DISCREPANCY = {"random_qp": (4.404e-11, 4.568e-10), "C3": (4.230e-05, 8.295e-05)}


# ---- host arithmetic and refusals without a device -----------------------------------------------------------------------------------------
def test_the_new_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    s = solver.FleetAdjointStats()
    calls = dict(
        qpdo_amd_fleet_adjoint_dev=lambda: L.qpdo_amd_fleet_adjoint_dev(None, *([None] * 10), 1e-9, 20, 0, 0, 0, 0, None),
        qpdo_amd_fleet_get_adjoint_stats=lambda: L.qpdo_amd_fleet_get_adjoint_stats(None, C.byref(s)))
    for name, call in calls.items():
        assert call() != 0 and last_error() == name + ": NULL fleet", (name, last_error())
        assert name in solver.EXT_SYMBOLS and hasattr(L, name)
    assert C.sizeof(solver.FleetAdjointStats) == 16 and [f for f, _ in solver.FleetAdjointStats._fields_] == ["adjoint_calls", "resident_extra_bytes"]
    hdr = open(os.path.join(os.path.dirname(_build.INCLUDE), "include", "qpdo_amd_ext.h")).read()
    assert "#define QPDO_AMD_FLEET_ADJOINT %dL" % solver.FLEET_ADJOINT in hdr
    assert solver.FLEET_ADJOINT & solver.FLEET_MATRIX_UPDATES == 0


def test_adjoint_device_validates_before_any_library_call():
    """no GPU here: dtype and element count are checked before the device, so each refusal is reachable with CPU tensors; the (NULL)
    handle is never reached"""
    import torch
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims = None, 2, [(4, 3), (2, 0)]
    F._layout, F._device, F._dev_out, F._adj_out = (np.array([0, 4, 6]), np.array([0, 3, 3])), 0, None, None
    F._mlayout = (np.array([0, 7, 9]), np.array([0, 5, 5]))
    with pytest.raises(ValueError, match="^gx: expected 6 elements"):
        F.adjoint_device(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="^gx: expected dtype float64, got torch.float32"):
        F.adjoint_device(torch.zeros(6, dtype=torch.float32))
    with pytest.raises(ValueError, match="^gy: expected 3 elements"):
        F.adjoint_device(None, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="^gx: expected a tensor on the GPU"):
        F.adjoint_device(torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="^gx: expected a torch tensor"):
        F.adjoint_device(np.zeros(6))
    with pytest.raises(ValueError, match="^gx: expected a tensor, got None"):
        F.adjoint_device(None)


def test_fleet_qp_rejects_an_unknown_on_failure():
    from qpdo_amd.torch_layer import FleetQP
    with pytest.raises(ValueError, match="^on_failure: expected one of"):
        FleetQP(None, on_failure="ignore")
    assert FleetQP(None, on_failure="zero").on_failure == "zero" and FleetQP(None).warm_start_last is True


# ---- the C-side checks from a C caller ------------------------------------------------------------------------------------------------------
def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_adjoint_args_driver.c")
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
