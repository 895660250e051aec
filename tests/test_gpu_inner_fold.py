"""The Schur mode's inner CG with its vector step folded into the two products (the default: two launches per iteration) against
the three-launch schedule with k_cgcg_step (QPDO_INNER_FOLD=0), and the slab kernel's non-temporal matrix loads (QPDO_SLAB_NT)
against the default cache policy: bit for bit.  The fold moves no operation and no order of additions; the loads only change
their cache policy."""
import numpy as np
import pytest

from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

INFO_KEYS = ("status_val", "iterations", "oterations", "objective", "res_prim_norm", "res_dual_norm")
FIRST_BATCH = 16        # launched inner iterations of the first batch of a pass's first inner solve (pcg_batch)


def _solve(p, monkeypatch, fold, nt="0"):
    monkeypatch.setenv("QPDO_INNER_FOLD", fold)
    monkeypatch.setenv("QPDO_SLAB_NT", nt)
    return solver.solve_problem(p, verbose=0)


def _assert_same(r0, r1):
    for r in (r0, r1):
        assert r["stats"]["schur_passes"] > 0 and r["stats"]["inner_steps"] > 0      # the mode ran: the test cannot pass with it off
    for k in INFO_KEYS:
        assert r0["info"][k] == r1["info"][k], k
    assert r0["stats"]["lin_iters"] == r1["stats"]["lin_iters"]
    assert r0["stats"]["inner_steps"] == r1["stats"]["inner_steps"] and r0["stats"]["inner_solves"] == r1["stats"]["inner_solves"]
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["y"], r1["y"])


def _active(r):
    return [t["n_active"] for t in r["trace"] if t["kind"] == 0]


@pytest.fixture(scope="module")
def slab_problem():
    return problems.random_qp(8200, 3000, 16000, 0.004, 0)


def _slab_env(monkeypatch):
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    monkeypatch.setenv("QPDO_SPMV", "slab")


def test_slab_path_whole_solve_bitwise(slab_problem, gpu_required, monkeypatch):
    """the setting of test_schur_mode_compact_products_match_old_schedule_bitwise under the four combinations of the two switches.
    (n = 3000 keeps k <= 0.8 n < 4096: A_c' takes the slab kernel, A_c the plain one; test_slab_step_product_bitwise has both on the
    slab kernel.)  Batches: a solve launches FIRST_BATCH iterations, or the previous solve's count less 6, and then 4 at a time.  More
    than FIRST_BATCH launched per solve on average therefore proves a second batch -- the solve's own or, through that rule, an
    earlier one's -- and every solve that ends before the last launch of a batch sends the remaining launches through the latch."""
    _slab_env(monkeypatch)
    res = [_solve(slab_problem, monkeypatch, fold, nt) for fold in ("0", "1") for nt in ("0", "1")]
    for r in res[1:]:
        _assert_same(res[0], r)
    st = res[3]["stats"]
    assert st["inner_steps"] > FIRST_BATCH * st["inner_solves"]
    assert any(k % 256 for k in _active(res[3]))             # ragged last block of the partial sums


def test_slab_path_twice_same_bits(slab_problem, gpu_required, monkeypatch):
    _slab_env(monkeypatch)
    a, b = _solve(slab_problem, monkeypatch, "1"), _solve(slab_problem, monkeypatch, "1")
    assert a["stats"]["schur_passes"] > 0 and a["stats"]["inner_steps"] > 0
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])


def test_plain_kernel_path_bitwise(gpu_required, monkeypatch):
    """random_qp(0, 400, 1600, 0.03): A_c and A_c' stay on k_spmv (no QPDO_SPMV; 256 <= k < 4096 active rows)"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    monkeypatch.delenv("QPDO_SPMV", raising=False)
    p = problems.random_qp(0, 400, 1600, 0.03, 0)
    r0, r1 = _solve(p, monkeypatch, "0"), _solve(p, monkeypatch, "1")
    _assert_same(r0, r1)
    ks = [k for k in _active(r1) if k >= 256]
    assert ks and max(ks) < 4096 and any(k % 256 for k in ks)


def test_slab_step_product_bitwise(gpu_required, monkeypatch):
    """random_qp(0, 6400, 20000, 0.003) with the slab kernels forced: passes with 4096 <= k <= 0.8 n active rows run the step inside
    the SLAB kernel of A_c (the 3000-column problem above keeps A_c on k_spmv: the Schur mode needs k <= 0.8 n).  256 workgroups of
    ceil(k / 256) = 17 .. 20 rows: every 256-block of the partial sums straddles workgroups' row ranges, and k is no multiple of 256."""
    _slab_env(monkeypatch)
    p = problems.random_qp(0, 6400, 20000, 0.003, 0)
    r0, r1 = _solve(p, monkeypatch, "0", "0"), _solve(p, monkeypatch, "1", "1")
    _assert_same(r0, r1)
    ks = [k for k in _active(r1) if 4096 <= k <= 0.8 * 6400]
    assert ks and any(k % 256 for k in ks) and any(((k + 255) // 256) % 256 for k in ks)
