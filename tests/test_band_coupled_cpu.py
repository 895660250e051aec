"""The band-plus-low-rank solve of QPDO_BAND_COUPLING on the CPU (tests/band_coupled_ref.py): the generator reproduces the recorded oracle
runs, the float64 reference is a backward-stable solver at the weights the linear-solver tests on the device use, and on every Newton
pass of the oracle's runs it is accepted by the residual rule of the device (WB_RES_TOL) after at most one refinement sweep -- the
condition tests/test_gpu_band_coupled.py leans on when it asserts coupled_rejects == 0."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_coupled_ref as ref
from helpers import U64, backward_error, newton_matrix
from oracle import binding as ob
from qpdo_amd import problems


@pytest.mark.parametrize("key", list(ref.ORACLE_RESULTS))
def test_generator_reproduces_the_recorded_oracle_runs(key):
    p = ref.coupled_banded_qp(ref.ORACLE_SEED, *key)
    n, bw, r = key
    rows, b_core = ref.classify(problems.full_Q(p), p["A"])
    assert list(rows) == list(range(p["m"] - r, p["m"])) and b_core == max(3, bw)
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    o.close()
    assert (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"]) == ref.ORACLE_RESULTS[key]
    ax = sp.csr_matrix(p["A"])[rows] @ ro["x"]
    tol = 1e-6 * np.maximum(1.0, np.abs(ax))
    assert np.any((ax <= p["l"][rows] + tol) | (ax >= p["u"][rows] - tol))      # coupling rows are active at the solution


def test_reference_is_backward_stable_at_moderate_weights():
    n, bw, r = 520, 12, 8
    p = ref.coupled_banded_qp(ref.ORACLE_SEED, n, bw, r)
    Qf, A = sp.csr_matrix(problems.full_Q(p)), sp.csr_matrix(p["A"])
    rows, _ = ref.classify(Qf, A)
    rng = np.random.default_rng(1)
    dw = 0.1 + 9.9 * rng.random(p["m"])
    dw[rows[[1, 4]]] = 0.0
    dcore = dw.copy()
    dcore[rows] = 0.0
    K = newton_matrix(Qf, A, 1.0, dw)
    B = newton_matrix(Qf, A, 1.0, dcore).astype(np.float64)
    act = rows[dw[rows] != 0.0]
    U = A[act].toarray().T
    Kmul = lambda x: Qf @ x + 1.0 * x + A.T @ (dw * (A @ x))
    xt = rng.standard_normal(n)
    for rhs in (rng.standard_normal(n), np.eye(n)[0], Kmul(xt)):
        x, sweeps, ok, rel = ref.woodbury_refine_solve(B, U, dw[act], Kmul, rhs)
        assert ok and sweeps <= 2, (sweeps, rel)
        eta = backward_error(Qf, A, 1.0, dw, x, rhs, K=K) / (n * U64)
        assert eta <= 4.0, eta


@pytest.mark.parametrize("key", [(600, 5, 3), (520, 12, 8)])
def test_emulation_is_accepted_on_every_newton_pass_of_the_oracle(key):
    p = ref.coupled_banded_qp(ref.ORACLE_SEED, *key)
    passes, coupled, worst_w = 0, 0, 0.0
    for s in ref.oracle_newton_systems(p):
        K, B, U, w, rhs = s["K"], s["B"], s["U"], s["w"], s["rhs"]
        # the pieces are the oracle's: K dx = rhs for its own direction, and K - B is the weighted coupling rows' term
        scale = np.abs(K).sum(axis=1).max() * np.abs(s["dx"]).max() + np.abs(rhs).max()
        assert np.abs(K @ s["dx"] - rhs).max() <= 1e-9 * scale, s["pass_no"]
        assert np.abs(K - B - (U * w) @ U.T).max() <= 64 * U64 * np.abs(K).max(), s["pass_no"]
        x, sweeps, ok, rel = ref.woodbury_refine_solve(B, U, w, lambda v: K @ v, rhs)
        assert ok and sweeps <= 2, (s["pass_no"], sweeps, rel)          # (sweeps counts the first solve: at most one refinement)
        passes += 1
        coupled += len(w) > 0
        worst_w = max(worst_w, float(w.max()) if len(w) else 0.0)
    print("%s: %d Newton passes, %d with weighted coupling rows, largest coupling weight %.3g" % (key, passes, coupled, worst_w))
    assert passes > 0 and coupled > 0
