"""The workspace adjoint / tangent on a band workspace WITH COUPLING ROWS (dev/adjoint.inc adj_sweeps), where no device is
needed: a float64 numpy emulation of the METHOD of include/qpdo_amd_ext.h -- flags from t = Ax + y, sigma = 1e-10 s, W_i = 1e10 s / ||a_i||^2,
block elimination on K = Q + sigma I + A_S' W A_S, repeated on the residual of the TRUE system, accepted on its inf-norm -- in which the
solve with K is ONE Woodbury application per sweep, K = B + U W_c U' with B the band part (tests/band_coupled_ref.py):
    z0 = B^-1 rhs,  t = S^-1 U' z0,  dvx = z0 - Z t,   Z = B^-1 U,  S = W_c^-1 + U' Z,
with no inner refinement and no inner check.  emulate_sweeps() is what tests/test_gpu_workspace_band_sens.py points to: it pins the choice
of the coupled instances there -- each is accepted within 20 sweeps at tol 1e-9, the duplicated coupling row behaves as two identical
active rows do on the dense route (consistent: accepted; inconsistent: not accepted at 20 sweeps, never a bad pivot), and every pivot of S
is positive -- independently of the device.  Unscaled (scaling 0), at the CPU oracle's solution."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import band_coupled_ref as bref
import fleet_adjoint_ref as ref
from oracle import binding as ob
from qpdo_amd import problems

SEED = 11
COUPLED_KEYS = [(600, 5, 1), (600, 5, 3), (520, 12, 8)]
TOL = 1e-9
MAX_SWEEPS = 20


def coupled_instance(key):
    return bref.coupled_banded_qp(SEED, *key)


def free_rows_instance():
    """banded_random_qp(11, 600, 5) with two coupling rows that have no finite bound: they are never flagged (k = 0 in every call)"""
    return bref.append_rows(problems.banded_random_qp(SEED, 600, 5), bref.coupling_rows(SEED, 600, 2), np.full(2, -1e20), np.full(2, 1e20))


def dup_instance():
    """coupled_banded_qp(11, 600, 5, 3) with its last row -- the equality coupling row -- stored once more: two identical active coupling rows"""
    p = coupled_instance((600, 5, 3))
    last = sp.csr_matrix(p["A"])[p["m"] - 1].toarray()
    assert p["l"][-1] == p["u"][-1] == 0.0
    return bref.append_rows(p, last, p["l"][-1:], p["u"][-1:])


@functools.lru_cache(maxsize=None)
def oracle_solution(name):
    """(problem, x, y) at the CPU oracle's solution; name: a key of COUPLED_KEYS, "free" or "dup" """
    p = free_rows_instance() if name == "free" else dup_instance() if name == "dup" else coupled_instance(name)
    o = ob.OracleSolver(p, ob.default_settings(max_iter=1000))
    r = o.solve()
    o.close()
    assert r["info"]["status_val"] == 1, (name, r["info"])
    return p, r["x"], r["y"]


def emulate_sweeps(p, x, y, gx, gy=None, tol=TOL, max_sweeps=MAX_SWEEPS, exact=False):
    """The sweep loop of adj_sweeps in float64 for one right-hand side (gx, gy; gy None = zeros).  exact: solve with the true K (a dense
    Cholesky) instead of the Woodbury application.  Returns dict(code, sweeps, rel, flags, k_coupled, s_pivots, vx, vy): code 0 accepted,
    1 not accepted at max_sweeps; s_pivots: the pivots of the unpivoted LDL' of S in slot order (what k_bc_factor_S latches on)."""
    n, m = p["n"], p["m"]
    Qf = ref.full_Q(p["Q"], p["Qstype"])
    A = ref.dense(p["A"])
    l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
    flags = ref.classify(x, y, A, l, u)
    S = flags != 0
    s = float(np.abs(np.diag(Qf)).max()) or 1.0
    sigma = 1e-10 * s
    a2 = (A * A).sum(axis=1)
    W = np.where(S & (a2 > 0), 1e10 * s / np.where(a2 > 0, a2, 1.0), 0.0)
    rows_c, _ = bref.classify(problems.full_Q(p), p["A"])
    core = W.copy()
    core[rows_c] = 0.0
    act = rows_c[W[rows_c] != 0.0]
    B = Qf + sigma * np.eye(n) + A.T @ (core[:, None] * A)
    K = Qf + sigma * np.eye(n) + A.T @ (W[:, None] * A)
    piv = np.zeros(0)
    if exact:
        cK = sla.cho_factor(K, lower=True)

        def inner(v):
            return sla.cho_solve(cK, v)
    else:
        cB = sla.cho_factor(B, lower=True)
        k = len(act)
        if k:
            U = A[act].T
            Z = sla.cho_solve(cB, U)
            Sm = np.diag(1.0 / W[act]) + U.T @ Z
            Lm, piv = Sm.copy(), np.zeros(k)
            for j in range(k):                                   # unpivoted LDL', k_bc_factor_S's elimination order
                piv[j] = Lm[j, j]
                Lm[j + 1:, j] /= piv[j]
                Lm[j + 1:, j + 1:] -= np.outer(Lm[j + 1:, j], Lm[j + 1:, j]) * piv[j]
            Ls = np.tril(Lm, -1) + np.eye(k)

        def inner(v):
            z0 = sla.cho_solve(cB, v)
            if not k:
                return z0
            t = sla.solve_triangular(Ls, U.T @ z0, lower=True, unit_diagonal=True) / piv
            t = sla.solve_triangular(Ls.T, t, lower=False, unit_diagonal=True)
            return z0 - Z @ t
    gys = np.where(S, np.zeros(m) if gy is None else np.where(S, gy, 0.0), 0.0)
    gnorm = max(float(np.abs(gx).max()), float(np.abs(gys).max()) if m else 0.0)
    vx, vy = np.zeros(n), np.zeros(m)
    code, sweep, rel = 1, 0, np.nan
    while True:
        rx = (gx - Qf @ vx) - A.T @ vy
        ry = np.where(S, gys - A @ vx, 0.0)
        rn = max(float(np.abs(rx).max()), float(np.abs(ry).max()) if m else 0.0)
        if np.isfinite(rn) and rn <= tol * gnorm:
            code, rel = 0, (rn / gnorm if gnorm > 0 else rn)
            break
        if sweep >= max_sweeps:
            break
        dvx = inner(rx + A.T @ (W * ry))
        vy = vy + W * (A @ dvx - ry)
        vx = vx + dvx
        sweep += 1
    return dict(code=code, sweeps=sweep, rel=rel, flags=flags, k_coupled=len(act), s_pivots=piv, vx=vx, vy=vy)


def right_hand_sides(p, flags, seed):
    rng = np.random.default_rng(seed)
    gx = rng.standard_normal(p["n"])
    gy = np.where(flags != 0, rng.standard_normal(p["m"]), 0.0)
    return gx, gy


@pytest.mark.parametrize("key", COUPLED_KEYS)
def test_the_coupled_instances_are_accepted_with_one_woodbury_application_per_sweep(key):
    p, x, y = oracle_solution(key)
    l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
    assert int((ref.margins(x, y, p["A"], l, u) < 1e-9).sum()) == 0, "rows below the margin at the oracle's solution"
    r = key[2]
    flags = ref.classify(x, y, ref.dense(p["A"]), l, u)
    assert (flags[p["m"] - r:] != 0).any(), "no coupling row is active: the instance would not run the Woodbury application"
    gx, gy = right_hand_sides(p, flags, 100)
    for what, g in (("gy=None", None), ("random gy", gy)):
        e = emulate_sweeps(p, x, y, gx, g)
        ex = emulate_sweeps(p, x, y, gx, g, exact=True)
        print("%s %s: Woodbury %d sweeps (rel %.2e), exact K %d sweeps, k = %d, smallest pivot of S %.3e"
              % (key, what, e["sweeps"], e["rel"], ex["sweeps"], e["k_coupled"], e["s_pivots"].min()))
        assert e["code"] == 0 and 1 <= e["sweeps"] <= MAX_SWEEPS and e["rel"] <= TOL, (key, what, e["code"], e["sweeps"])
        assert ex["code"] == 0 and ex["sweeps"] <= e["sweeps"], (key, what, ex["sweeps"], e["sweeps"])
        assert e["k_coupled"] == int((flags[p["m"] - r:] != 0).sum()) and (e["s_pivots"] > 0).all(), (key, what, e["s_pivots"])
        # the emulation's solution solves the adjoint system of these flags
        M, S = ref.kkt(ref.full_Q(p["Q"], p["Qstype"]), ref.dense(p["A"]), flags)
        v = np.concatenate([e["vx"], e["vy"][S]]).astype(ref.LD)
        rhs = np.concatenate([gx, (np.zeros(p["m"]) if g is None else g)[S]]).astype(ref.LD)
        assert float(np.abs(M @ v - rhs).max()) <= 2 * TOL * float(np.abs(rhs).max()), (key, what)


def test_coupling_rows_without_a_finite_bound_leave_the_plain_band_solve():
    p, x, y = oracle_solution("free")
    gx, gy = right_hand_sides(p, ref.classify(x, y, ref.dense(p["A"]), np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)), 101)
    e = emulate_sweeps(p, x, y, gx, gy)
    assert e["code"] == 0 and e["k_coupled"] == 0 and not e["flags"][-2:].any() and e["sweeps"] <= 3, (e["code"], e["sweeps"], e["k_coupled"])


def test_a_duplicated_active_coupling_row():
    """consistent right-hand sides are accepted; gy = (+1, -1) on the two copies is not accepted at 20 sweeps; S keeps positive pivots (the
    device reports code 1 for it, never code 3)"""
    p, x, y = oracle_solution("dup")
    m = p["m"]
    gx = np.random.default_rng(3).standard_normal(p["n"])
    ok = emulate_sweeps(p, x, y, gx, None)
    assert ok["flags"][m - 1] != 0 and ok["flags"][m - 2] != 0 and ok["k_coupled"] >= 2
    print("duplicated row, gy=None: %d sweeps; pivots of S %s" % (ok["sweeps"], ok["s_pivots"]))
    assert ok["code"] == 0 and ok["sweeps"] <= MAX_SWEEPS and (ok["s_pivots"] > 0).all() and np.isfinite(ok["s_pivots"]).all()
    gy = np.zeros(m)
    gy[m - 2], gy[m - 1] = 1.0, -1.0
    bad = emulate_sweeps(p, x, y, gx, gy)
    assert (bad["code"], bad["sweeps"]) == (1, MAX_SWEEPS), (bad["code"], bad["sweeps"])
    assert (bad["s_pivots"] > 0).all()
