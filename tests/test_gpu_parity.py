"""Parity of the HIP path (through the qpdo.h C-ABI) against the CPU oracle and the committed golden
vectors.  Bar (BASELINE.json north_star): termination status, iteration count and outer-iteration count
identical; iterates within ITERATE_RTOL; KKT residuals within KKT_ATOL."""
import json
import os

import numpy as np
import pytest

from helpers import (ITERATE_RTOL, ITERATE_RTOL_PCG, KKT_ATOL, TAU_RTOL_PCG_C4_FULL, assert_same_trace, close_vec, golden_problem,
                     load_golden, trace_from_npz)
from oracle import binding as ob
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu
GOLD = load_golden()


@pytest.fixture(params=["dense", "pcg"])
def linsolve(request, monkeypatch):
    """both device linear solvers: dense MFMA LDL' (default for n <= 12288) and Jacobi-PCG"""
    monkeypatch.setenv("QPDO_LINSOLVE", request.param)
    return request.param


def rtol_of(linsolve):
    return ITERATE_RTOL if linsolve == "dense" else ITERATE_RTOL_PCG


def assert_same_outcome(res, ref_info, ref_x, ref_y, prob=None, rtol=ITERATE_RTOL):
    i = res["info"]
    assert i["status_val"] == ref_info["status_val"]
    assert i["iterations"] == ref_info["iterations"]
    assert i["oterations"] == ref_info["oterations"]
    assert close_vec(res["x"], ref_x, rtol), np.abs(np.asarray(res["x"]) - np.asarray(ref_x)).max()
    assert close_vec(res["y"], ref_y, rtol), np.abs(np.asarray(res["y"]) - np.asarray(ref_y)).max()
    if prob is not None and i["status_val"] == 1:
        rp, rd = problems.kkt_residuals(prob, res["x"], res["y"])
        rp0, rd0 = problems.kkt_residuals(prob, np.asarray(ref_x), np.asarray(ref_y))
        assert abs(rp - rp0) <= KKT_ATOL and abs(rd - rd0) <= KKT_ATOL
        assert abs(rp - i["res_prim_norm"]) <= 1e-9 and abs(rd - i["res_dual_norm"]) <= 1e-9


@pytest.mark.parametrize("name", sorted(GOLD))
def test_against_golden_vectors(name, linsolve, gpu_required):
    g = GOLD[name]
    p = golden_problem(g["spec"])
    r = solver.solve_problem(p, verbose=0, **g["settings"])
    assert r["stats"]["linsolve"] == (1 if linsolve == "dense" else 0)
    assert_same_outcome(r, g, g["x"], g["y"], p, rtol_of(linsolve))
    assert [t["kind"] for t in r["trace"]] == g["kinds"]
    assert [t["n_active"] for t in r["trace"]] == g["n_active"]
    gt = g["trace"]
    assert_same_trace(r["trace"], [{f: gt[f][k] for f in gt} for k in range(len(gt["kind"]))], pcg=(linsolve == "pcg"))
    assert close_vec(r["prim_inf_cert"], g["prim_inf_cert"], 1e-6)
    assert close_vec(r["dual_inf_cert"], g["dual_inf_cert"], 1e-6)


@pytest.mark.parametrize("case", ["degenerate", "primal_infeasible", "dual_infeasible"])
def test_reference_known_answers_on_device(case, gpu_required):
    """reference examples/infeasibility_tests.m:30,48,75"""
    p = problems.infeasibility_kat(case)
    r = solver.solve_problem(p, verbose=0, max_iter=p["max_iter"])
    assert r["info"]["status_val"] == p["expected_status"]
    assert r["info"]["status"] == {1: "solved", -3: "primal infeasible", -4: "dual infeasible"}[p["expected_status"]]


@pytest.mark.parametrize("seed,n,m,dens,neq,st", [
    (21, 40, 60, 0.2, 0, {}),
    (22, 150, 300, 0.05, 0, {}),
    (23, 150, 300, 0.05, 50, {}),                 # equality rows: tie hazard in the linesearch sort
    (24, 300, 200, 0.03, 0, dict(scaling=0)),
    (25, 300, 200, 0.03, 0, dict(proximal=0)),
    (26, 64, 1, 0.2, 0, {}),                      # single constraint
    (27, 1, 5, 1.0, 0, {}),                       # single variable
    (28, 500, 1000, 0.02, 0, dict(eps_abs=1e-8)),
    (29, 200, 400, 0.05, 0, dict(reset_newton_iter=3, inner_max_iter=6)),
])
def test_random_instances_match_live_oracle(seed, n, m, dens, neq, st, linsolve, gpu_required):
    p = problems.random_qp(seed, n, m, dens, neq)
    o = ob.OracleSolver(p, ob.default_settings(**st))
    ro = o.solve()
    r = solver.solve_problem(p, verbose=0, **st)
    assert_same_outcome(r, ro["info"], ro["x"], ro["y"], p, rtol_of(linsolve))
    assert_same_trace(r["trace"], o.trace(), pcg=(linsolve == "pcg"))
    o.close()


@pytest.mark.parametrize("seed,n,m,dens,neq", [
    (61, 2400, 4800, 0.01, 0),        # dense: every weight change refactors (one launch per factorization, 38 x 39 / 2 tile workgroups)
    (62, 3000, 6000, 0.01, 300),      # the same with equality rows
    (63, 7300, 12000, 0.005, 0),      # 115 block columns: 6 670 workgroups, far more than are resident at once
])
def test_default_dense_regimes_match_live_oracle(seed, n, m, dens, neq, gpu_required, monkeypatch):
    """the DEFAULT solver selection below the low-rank threshold (updates of the kept factor from n = 9000: the C2 fixture covers that side,
    the PCG sizes are covered by the committed fixtures too) against the oracle run here: counts, per-pass trace, iterates"""
    for k in list(os.environ):
        if k.startswith("QPDO_"):
            monkeypatch.delenv(k)
    p = problems.random_qp(seed, n, m, dens, neq)
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    r = solver.solve_problem(p, verbose=0)
    assert r["stats"]["linsolve"] == 1 and r["stats"]["lin_iters"] == 0
    assert r["stats"]["lowrank_solves"] == 0 and r["stats"]["onelaunch_factors"] == r["stats"]["factor_count"] > 0
    assert_same_outcome(r, ro["info"], ro["x"], ro["y"], p)
    assert_same_trace(r["trace"], o.trace())
    o.close()


def test_scaling_is_bit_exact(gpu_required):
    """Ruiz + cost scaling (reference src/scaling.c:24-91) is elementwise: identical bits expected"""
    p = problems.config_qp("C1")
    o = ob.OracleSolver(p, ob.default_settings())
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    sc = s.scaling()
    assert np.array_equal(sc["D"], o.vec("D")) and np.array_equal(sc["E"], o.vec("E"))
    assert sc["c"] == o.info()["scaling_c"]
    assert np.array_equal(s.download("l"), o.vec("l")) and np.array_equal(s.download("u"), o.vec("u"))
    s.delete(); o.close()


@pytest.mark.parametrize("kernel", ["auto", "slab-i16", "slab-i32"])
@pytest.mark.parametrize("shape", [(200, 100, 0.1), (50, 1000, 0.3), (3000, 4000, 0.01), (700, 300, 0.37)])
def test_spmv_matches_oracle(shape, kernel, gpu_required, monkeypatch):
    """plain gather kernel (auto at these sizes) and the LDS-staged slab kernel over the slab-major image with
    16-bit slab-local or 32-bit column indices"""
    if kernel != "auto":
        monkeypatch.setenv("QPDO_SPMV", "slab")
        monkeypatch.setenv("QPDO_IDX16", "1" if kernel == "slab-i16" else "0")
    n, m, dens = shape
    p = problems.random_qp(31, n, m, dens)
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
    rng = np.random.default_rng(1)
    xn, ym = rng.standard_normal(n), rng.standard_normal(m)
    absA, absQ = abs(p["A"]), abs(problems.full_Q(p))
    for which, v, ref, bound in [
        (0, xn, ob.csc_mv(p["A"], xn), absA @ np.abs(xn)),
        (1, ym, ob.csc_mv(p["A"], ym, trans=True), absA.T @ np.abs(ym)),
        (2, xn, ob.csc_mv(p["Q"], xn, stype=-1), absQ @ np.abs(xn)),
    ]:
        got = s.spmv(which, v)
        assert np.all(np.abs(got - ref) <= 1e-13 * (bound + 1e-300)), which
    # linearity (size-independent property)
    a = s.spmv(0, xn); b = s.spmv(0, 2.0 * xn)
    assert np.array_equal(b, 2.0 * a)
    s.delete()


@pytest.mark.parametrize("m", [1, 5, 300, 512, 900, 1500, 2048, 3000, 4096, 5000, 70000])
def test_linesearch_matches_oracle(m, gpu_required):
    rng = np.random.default_rng(m)
    delta = rng.standard_normal(2 * m); delta[m:] = -delta[:m]
    alpha = np.abs(rng.standard_normal(2 * m)) * rng.choice([1.0, -0.3], 2 * m)
    if m >= 5:
        alpha[m:m + 2] = -alpha[:2]                # exact ties
        delta[3] = 0.0; delta[m + 3] = 0.0         # +-inf / nan ratios
        alpha[4] = 1e20                            # "infinite" bound
    eta = 0.7 + rng.random()
    with np.errstate(divide="ignore", invalid="ignore"):
        act0 = ((alpha / delta) > 0) != (delta > 0)
    beta = -abs(float((delta[act0] * alpha[act0]).sum())) - 0.5 - rng.random()
    ref = ob.pwa_linesearch(eta, beta, delta, alpha)
    p = problems.random_qp(1, 4, m, 0.5)
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
    tau = s.linesearch(eta, beta, delta, alpha)
    assert abs(tau - ref) <= 1e-10 * max(1.0, abs(ref))
    psi = eta * tau + beta + delta @ np.maximum(delta * tau - alpha, 0.0)
    scale = abs(beta) + eta * abs(tau) + np.abs(delta) @ np.abs(delta * tau - alpha)
    assert abs(psi) <= 1e-11 * scale
    s.delete()


@pytest.mark.parametrize("m", [100, 600, 1100, 2048, 3000, 4096])
def test_one_launch_linesearch_is_the_radix_path_bit_for_bit(m, gpu_required, monkeypatch):
    """k_ls_small (2m <= 8192: compaction, register bitonic network or side-by-side chunks + rank merge, the scans of the multi-launch
    kernels in their order) against the radix-sort path (QPDO_LS_SMALL=0) on candidates full of EXACT ties -- ratios from a handful of
    values, so that equal keys straddle every chunk boundary and only the index tie-break orders them -- and on generic ones: the same tau
    bits, and the oracle's value."""
    p = problems.random_qp(1, 4, m, 0.5)
    for variant in ("ties", "generic", "all_positive"):
        rng = np.random.default_rng(7 * m + len(variant))
        if variant == "ties":
            delta = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 2 * m)
            alpha = delta * rng.choice([0.25, 0.5, 1.0, 3.0, -1.0], 2 * m)       # t = alpha / delta takes five values
        elif variant == "generic":
            delta = rng.standard_normal(2 * m); alpha = rng.standard_normal(2 * m)
        else:
            delta = np.abs(rng.standard_normal(2 * m)) + 0.1; alpha = delta * (0.01 + rng.random(2 * m))   # every candidate is a breakpoint
        eta = 0.9 + rng.random()
        with np.errstate(divide="ignore", invalid="ignore"):
            act0 = ((alpha / delta) > 0) != (delta > 0)
        beta = -abs(float((delta[act0] * alpha[act0]).sum())) - 0.5 - rng.random()
        ref = ob.pwa_linesearch(eta, beta, delta, alpha)
        taus = []
        for small in ("1", "0"):
            monkeypatch.setenv("QPDO_LS_SMALL", small)
            s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
            taus.append(s.linesearch(eta, beta, delta, alpha))
            s.delete()
        monkeypatch.delenv("QPDO_LS_SMALL")
        assert taus[0] == taus[1], (m, variant, taus)
        assert abs(taus[0] - ref) <= 1e-10 * max(1.0, abs(ref)), (m, variant)


@pytest.mark.parametrize("size", ["C1", "mid"])
def test_warm_start_and_update_sequence_matches_oracle(size, linsolve, gpu_required, monkeypatch):
    """qpdo_warm_start / qpdo_update_bounds / qpdo_update_q / qpdo_update_settings followed by re-solves on one
    workspace (reference src/qpdo.c:217-299,481-586).  "mid" is large enough for the Schur-complement mode of the PCG
    and for the low-rank update of the dense factor to take part in the re-solves."""
    if size == "mid":
        monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    p = problems.config_qp("C1") if size == "C1" else problems.random_qp(71, 600, 1100, 0.03, 40)
    o = ob.OracleSolver(p, ob.default_settings())
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    rt = rtol_of(linsolve)
    ro, rg = o.solve(), s.solve()
    assert_same_outcome(rg, ro["info"], ro["x"], ro["y"], p, rt)
    rng = np.random.default_rng(0)
    xw, yw = ro["x"] + 1e-3 * rng.standard_normal(p["n"]), ro["y"] + 1e-3 * rng.standard_normal(p["m"])
    o.warm_start(xw, yw); s.warm_start(xw, yw)
    ro, rg = o.solve(), s.solve()
    assert_same_outcome(rg, ro["info"], ro["x"], ro["y"], p, rt)
    l2, u2 = p["l"] - 0.1, p["u"] + 0.05
    o.update_bounds(l2, u2); s.update_bounds(l2, u2)
    ro, rg = o.solve(), s.solve()
    p2 = dict(p); p2["l"], p2["u"] = l2, u2
    assert_same_outcome(rg, ro["info"], ro["x"], ro["y"], p2, rt)
    q2 = 1.5 * p["q"] + 0.1
    o.update_q(q2); s.update_q(q2)
    ro, rg = o.solve(), s.solve()
    p3 = dict(p2); p3["q"] = q2
    assert_same_outcome(rg, ro["info"], ro["x"], ro["y"], p3, rt)
    so = ob.default_settings(eps_abs=1e-8, scaling=15)
    o.update_settings(so); s.update_settings(eps_abs=1e-8, scaling=15)
    ro, rg = o.solve(), s.solve()
    assert_same_outcome(rg, ro["info"], ro["x"], ro["y"], p3, rt)
    # error contract: decreasing scaling, inconsistent bounds -> QPDO_ERROR (reference src/qpdo.c:487-494,533)
    s.update_settings(scaling=3)
    assert s.info()["status_val"] == -99
    s.delete(); o.close()


def test_solve_is_reproducible_run_to_run(gpu_required):
    p = problems.random_qp(41, 400, 800, 0.03)
    a = solver.solve_problem(p, verbose=0)
    b = solver.solve_problem(p, verbose=0)
    assert a["info"]["iterations"] == b["info"]["iterations"]
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])


def test_deferred_step_read_back_changes_no_bit(gpu_required, monkeypatch):
    """One host synchronisation per loop pass (the Newton step's read-back rides on the next residual read; round 3) against two
    (QPDO_DEFER_STEP=0): the same kernels in the same order, so the same bits -- solution, counts, and every field of the trace,
    including the step length that arrives one read later; also when the solve is cut off right after a Newton step (max_iter)."""
    for prob, st in ((problems.random_qp(41, 400, 800, 0.03), {}), (problems.config_qp("C1"), dict(max_iter=200)),
                     (problems.config_qp("C3"), dict(max_iter=7)), (problems.infeasibility_kat("dual_infeasible"), dict(max_iter=100))):
        monkeypatch.setenv("QPDO_DEFER_STEP", "0")
        a = solver.solve_problem(prob, verbose=0, **st)
        monkeypatch.setenv("QPDO_DEFER_STEP", "1")
        b = solver.solve_problem(prob, verbose=0, **st)
        assert (a["info"]["status_val"], a["info"]["iterations"], a["info"]["oterations"]) == (b["info"]["status_val"], b["info"]["iterations"], b["info"]["oterations"])
        assert np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["y"], b["y"], equal_nan=True)
        assert np.array_equal(a["dual_inf_cert"], b["dual_inf_cert"], equal_nan=True)
        assert len(a["trace"]) == len(b["trace"])
        for ta, tb in zip(a["trace"], b["trace"]):
            assert all(ta[k] == tb[k] for k in ta), (ta, tb)


def test_max_iter_and_max_time_statuses(gpu_required):
    p = problems.config_qp("C1")
    r = solver.solve_problem(p, verbose=0, max_iter=3)
    assert r["info"]["status_val"] == -5 and r["info"]["iterations"] == 3
    r = solver.solve_problem(p, verbose=0, max_time=1e-9)
    assert r["info"]["status_val"] == -6


def test_dense_factor_is_reused_when_weights_do_not_change(gpu_required, monkeypatch):
    """consecutive passes with an unchanged active set must not refactor (reference: no update at all,
    src/newton.c:25-30)"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    p = problems.config_qp("C1")
    r = solver.solve_problem(p, verbose=0)
    newton = [t for t in r["trace"] if t["kind"] == 0]
    unchanged = sum(1 for t in newton if t["factor_branch"] == 1 and t["n_enter"] + t["n_leave"] == 0)
    assert r["stats"]["factor_count"] <= len(newton) - unchanged
    assert r["stats"]["factor_count"] >= 1 and r["stats"]["lin_iters"] == 0


def test_dense_factor_schedules_leave_the_same_bits(gpu_required, monkeypatch):
    """the multi-launch factorization on one stream and with the look-ahead on a second stream: the look-ahead only reschedules the
    factorization, every element of K receives the same updates in the same order, so the solve is bit-identical"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "0")
    monkeypatch.setenv("QPDO_DENSE_MID", "0")          # the multi-launch factorization (since round 5 the fallback of the one-launch kernel)
    p = problems.random_qp(77, 1500, 2600, 0.01, 100)
    base = None
    for lookahead in ("0", "1"):
        monkeypatch.setenv("QPDO_DENSE_LOOKAHEAD", lookahead)
        r = solver.solve_problem(p, verbose=0)
        assert r["info"]["status_val"] == 1 and r["stats"]["chain_fallbacks"] == 0, lookahead
        if base is None:
            base = r
        else:
            assert r["info"]["iterations"] == base["info"]["iterations"], lookahead
            assert np.array_equal(r["x"], base["x"]) and np.array_equal(r["y"], base["y"]), lookahead


def test_one_launch_factorization_matches_the_multi_launch_one_and_the_oracle(gpu_required, monkeypatch):
    """k_mid_factor (one resident workgroup per 64 x 64 tile, flag hand-offs, forward solve riding along; the default) against the
    multi-launch blocked factorization it replaces (QPDO_DENSE_MID=0) and against the oracle: orders with one block, with a padded last
    block (n mod 64 = 8 and = 40), with more tiles than CUs (n = 1500: 300 workgroups); twice in a row: the same bits"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "0")
    for seed, n, m, dens in ((5, 200, 100, 0.1), (6, 64, 150, 0.2), (7, 360, 500, 0.05), (77, 1500, 2600, 0.01)):
        p = problems.random_qp(seed, n, m, dens, min(50, m // 4))
        monkeypatch.setenv("QPDO_DENSE_MID", "0")
        r0 = solver.solve_problem(p, verbose=0)
        monkeypatch.delenv("QPDO_DENSE_MID")
        r1 = solver.solve_problem(p, verbose=0)
        r2 = solver.solve_problem(p, verbose=0)
        assert r1["stats"]["chain_fallbacks"] == 0 and r1["stats"]["factor_count"] == r0["stats"]["factor_count"] > 0, (n, m)
        assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p)
        assert [(t["kind"], t["n_active"], t["n_enter"], t["n_leave"], t["factor_branch"]) for t in r1["trace"]] == \
               [(t["kind"], t["n_active"], t["n_enter"], t["n_leave"], t["factor_branch"]) for t in r0["trace"]], (n, m)
        assert np.array_equal(r1["x"], r2["x"]) and np.array_equal(r1["y"], r2["y"]), (n, m)
        o = ob.OracleSolver(p, ob.default_settings())
        ro = o.solve()
        assert_same_outcome(r1, ro["info"], ro["x"], ro["y"], p)
        # tau: 5e-8 here instead of the suite's 1e-8 -- instance (7, 360, 500) has an ill-conditioned stretch (passes 33-36) on which the
        # multi-launch factorization deviates from the oracle by 6.4e-9 and the one-launch one by 1.5e-8 (tools/mid_dev_probe.py,
        # profiles/r05_mid_dev_probe.txt: on the other nine instances both stay below 2.5e-9, neither is systematically closer)
        assert_same_trace(r1["trace"], o.trace(), tau_rtol=5e-8)
        o.close()


def test_control_block_read_back_by_publication_is_the_copy_path_bit_for_bit(gpu_required, monkeypatch):
    """The per-pass read-back (dev/host_core.inc read_ctrl_block): a one-wave kernel writes the control block and a sequence word into
    coherent pinned memory while the host spins (default) against hipMemcpyAsync + hipStreamSynchronize (QPDO_CTRL_PUBLISH=0).  Only the
    transport differs, so every route gives the same bits: dense one-launch (C1), PCG with its inner control block (Schur mode), and a
    mid-size dense instance whose factorizations outlast the bounded spin (the hand-over to hipStreamSynchronize)."""
    cases = [("dense", problems.config_qp("C1")), ("pcg", problems.random_qp(11, 900, 1500, 0.02, 60)), ("dense", problems.random_qp(12, 2400, 3000, 0.01, 50))]
    for lin, p in cases:
        monkeypatch.setenv("QPDO_LINSOLVE", lin)
        monkeypatch.setenv("QPDO_CTRL_PUBLISH", "0")
        r0 = solver.solve_problem(p, verbose=0)
        monkeypatch.delenv("QPDO_CTRL_PUBLISH")
        r1 = solver.solve_problem(p, verbose=0)
        # ... and the launches folded into others this round -- the step's axpys and the publication in the residual launch
        # (QPDO_FUSE_RESID), the outer-update sequences in 4 + 8 launches instead of 8 + 13 (QPDO_FUSE_OUTER) -- against their separate kernels
        monkeypatch.setenv("QPDO_FUSE_RESID", "0")
        monkeypatch.setenv("QPDO_FUSE_OUTER", "0")
        r2 = solver.solve_problem(p, verbose=0)
        monkeypatch.delenv("QPDO_FUSE_RESID")
        monkeypatch.delenv("QPDO_FUSE_OUTER")
        for r in (r1, r2):
            assert r0["info"]["status_val"] == r["info"]["status_val"] and r0["info"]["iterations"] == r["info"]["iterations"], lin
            assert np.array_equal(r0["x"], r["x"]) and np.array_equal(r0["y"], r["y"]), lin
            assert [(t["kind"], t["n_active"], t["tau"] if t["tau"] == t["tau"] else None) for t in r0["trace"]] == \
                   [(t["kind"], t["n_active"], t["tau"] if t["tau"] == t["tau"] else None) for t in r["trace"]], lin


def test_newton_step_launched_ahead_of_the_host_decision_changes_no_bit(gpu_required, monkeypatch):
    """Mid-size dense route: the Newton step of a pass is enqueued behind the residual launch, which forms the host's decision (end of the
    solve / outer update / factorization branch: qpdo.c:343-449, newton.c:21-33) on the device; the step's kernels leave at once when the
    answer is no (dev/host_step.inc ahead_enqueue_step, QPDO_LAUNCH_AHEAD=0: the host decides first).  Both routes go through the same
    launch sites (dev/host_dense.inc launch_dense_assemble / launch_mid_factor / launch_ldl_chain, dev/host_step.inc launch_adx_qdx_pair /
    launch_ls_small); the kernels and their order are the same, so every count, every per-pass record and every bit of the iterates must be: cold solves with and without Ruiz scaling, without
    the proximal term, with inner_max_iter forcing outer updates, a primal-infeasible instance (the solve ends in an outer update), and a
    warm start / update sequence on one workspace.  The statistics must show that the steps did go ahead."""
    def rec(t):
        return (t["kind"], t["n_active"], t["n_enter"], t["n_leave"], t["factor_branch"], t["tau"] if t["tau"] == t["tau"] else None,
                t["res_prim"], t["res_dual"], t["res_prim_in"], t["res_dual_in"], t["sigma"], t["eps_in"])
    def same(a, b, what):
        assert (a["info"]["status_val"], a["info"]["iterations"], a["info"]["oterations"]) == \
               (b["info"]["status_val"], b["info"]["iterations"], b["info"]["oterations"]), what
        for k in ("x", "y", "prim_inf_cert"):          # (NaN where the status does not define them)
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
        assert [rec(t) for t in a["trace"]] == [rec(t) for t in b["trace"]], what
    pinf = problems.random_qp(62, 300, 420, 0.05)
    A = pinf["A"].tolil(); A[1, :] = A[0, :]; pinf["A"] = A.tocsc()
    pinf["l"][0], pinf["u"][0], pinf["l"][1], pinf["u"][1] = 1.0, 2.0, -2.0, -1.0
    cases = [("C1", problems.config_qp("C1"), {}), ("n300", problems.random_qp(31, 300, 600, 0.1), {}),
             ("unscaled", problems.random_qp(8, 260, 300, 0.05, 20), dict(scaling=0)), ("no proximal term", problems.random_qp(9, 220, 500, 0.05), dict(proximal=0)),
             ("inner_max_iter 3", problems.random_qp(10, 400, 700, 0.03), dict(inner_max_iter=3, max_iter=400)),
             ("reset_newton_iter 4", problems.random_qp(13, 330, 500, 0.04), dict(reset_newton_iter=4)),
             ("primal infeasible", pinf, dict(max_iter=500))]
    went = n_kept = 0
    for what, p, kw in cases:
        monkeypatch.setenv("QPDO_LAUNCH_AHEAD", "0")
        r0 = solver.solve_problem(p, verbose=0, **kw)
        monkeypatch.delenv("QPDO_LAUNCH_AHEAD")
        r1 = solver.solve_problem(p, verbose=0, **kw)
        assert r0["stats"]["ahead_steps"] == 0 and r0["stats"]["ahead_skips"] == 0 and r0["stats"]["linsolve"] == 1, what
        # A pass whose factor the host-first path keeps (branch 1 with nothing entered or left, or two Q-only passes in a row) is
        # refactored by the launched-ahead step: the same matrix, but the forward solve then rides on the factorization launch instead of
        # the chained kernel -- on instances with such a pass the last bits may differ, so they are compared like two solvers.
        kept = r0["stats"]["factor_count"] < r0["stats"]["newton_passes"]
        assert r0["stats"]["factor_count"] <= r1["stats"]["factor_count"] <= r1["stats"]["newton_passes"], what
        if not kept:
            same(r1, r0, what)
        else:
            n_kept += 1
            assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p)
            assert [rec(t)[:5] for t in r1["trace"]] == [rec(t)[:5] for t in r0["trace"]], what
        st = r1["stats"]
        # every Newton step after the first (which allocates the dense factor) goes ahead, except the steps that follow a Newton pass in
        # which no row entered or left (the host-first path may keep its factor there, so the host decides first: qpdo_api.c ahead_ok);
        # every other pass that tried was an outer update or the last one
        tr = r1["trace"]
        quiet = sum(1 for i in range(1, len(tr)) if tr[i - 1]["kind"] == 0 and tr[i - 1]["n_enter"] + tr[i - 1]["n_leave"] == 0)
        assert st["newton_passes"] - 1 - quiet <= st["ahead_steps"] <= st["newton_passes"] - 1 and st["chain_fallbacks"] == 0, (what, st, quiet)
        tried = r1["info"]["iterations"] - 1 + (1 if r1["info"]["status_val"] in (1, -3, -4) else 0)
        assert tried - quiet <= st["ahead_steps"] + st["ahead_skips"] <= tried, (what, st, quiet)
        went += st["ahead_steps"]
    assert went > 100 and n_kept <= 2
    # one workspace, several solves: the dense factor exists from the second solve's first pass on
    p = problems.random_qp(71, 500, 900, 0.03, 40)
    outs = []
    for ahead in ("0", "1"):
        monkeypatch.setenv("QPDO_LAUNCH_AHEAD", ahead)
        s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
        rs = [s.solve()]
        rng = np.random.default_rng(0)
        s.warm_start(rs[0]["x"] + 1e-3 * rng.standard_normal(p["n"]), rs[0]["y"] + 1e-3 * rng.standard_normal(p["m"]))
        rs.append(s.solve())
        s.update_bounds(p["l"] - 0.1, p["u"] + 0.05)
        rs.append(s.solve())
        s.update_q(1.5 * p["q"] + 0.1)
        rs.append(s.solve())
        s.update_settings(eps_abs=1e-8)
        rs.append(s.solve())
        for r in rs:
            r["trace"] = None
        outs.append((rs, s.stats()))
        s.delete()
    monkeypatch.delenv("QPDO_LAUNCH_AHEAD")
    for a, b in zip(outs[0][0], outs[1][0]):
        assert (a["info"]["status_val"], a["info"]["iterations"], a["info"]["oterations"]) == (b["info"]["status_val"], b["info"]["iterations"], b["info"]["oterations"])
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])
    assert outs[0][1]["ahead_steps"] == 0 and 0 < outs[1][1]["ahead_steps"] <= outs[1][1]["newton_passes"]


def test_dense_lowrank_update_matches_refactoring(gpu_required, monkeypatch):
    """few rows entering/leaving: the kept factor is updated instead of rebuilt (reference
    src/cholmod_interface.c:57-93, src/newton.c:21-30); the solve must be indistinguishable from refactoring"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    p = problems.random_qp(41, 600, 1200, 0.02, 0)
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "0")
    r0 = solver.solve_problem(p, verbose=0)
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "1")
    r1 = solver.solve_problem(p, verbose=0)
    assert r0["stats"]["lowrank_solves"] == 0
    assert r1["stats"]["lowrank_solves"] > 0 and r1["stats"]["factor_count"] < r0["stats"]["factor_count"]
    assert r1["stats"]["lowrank_sweeps"] >= r1["stats"]["lowrank_solves"]
    assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p)
    assert [t["n_active"] for t in r1["trace"]] == [t["n_active"] for t in r0["trace"]]
    assert [t["factor_branch"] for t in r1["trace"]] == [t["factor_branch"] for t in r0["trace"]]
    # ... and from the oracle, which restates the reference's rank-update rules as the weight vector d
    # (oracle/qpdo_oracle.c newton_direction / update_mu): the run that really took the low-rank path (checked above)
    # must reproduce the oracle's outcome and its whole per-pass trace
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    assert_same_outcome(r1, ro["info"], ro["x"], ro["y"], p)
    assert_same_trace(r1["trace"], o.trace())
    assert any(t["factor_branch"] == 1 and t["n_enter"] + t["n_leave"] > 0 for t in r1["trace"])
    o.close()


def test_dense_chained_solve_matches_stepwise(gpu_required, monkeypatch):
    """the one-launch-per-direction triangular solves against the per-block-step kernels (n not a multiple of 64)"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    p = problems.random_qp(43, 1000, 700, 0.03, 50)
    monkeypatch.setenv("QPDO_DENSE_SOLVE", "steps")
    r0 = solver.solve_problem(p, verbose=0)
    monkeypatch.setenv("QPDO_DENSE_SOLVE", "chain")
    r1 = solver.solve_problem(p, verbose=0)
    assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p)
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    assert_same_outcome(r1, ro["info"], ro["x"], ro["y"], p)
    o.close()


def test_pcg_schur_mode_matches_jacobi_and_oracle(gpu_required, monkeypatch):
    """the Schur-complement mode of the PCG (outer CG preconditioned by Dq + A_c' D A_c, inner CG on the k x k
    system) solves the same Newton systems as the deflated Jacobi-PCG: same pass counts, same iterates"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    p = problems.random_qp(61, 700, 1400, 0.03, 0)
    monkeypatch.setenv("QPDO_PCG_SCHUR", "0")
    r0 = solver.solve_problem(p, verbose=0)
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    r1 = solver.solve_problem(p, verbose=0)
    assert r0["stats"]["schur_passes"] == 0 and r1["stats"]["schur_passes"] > 0
    assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p, ITERATE_RTOL_PCG)
    assert [t["n_active"] for t in r1["trace"]] == [t["n_active"] for t in r0["trace"]]
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    assert_same_outcome(r1, ro["info"], ro["x"], ro["y"], p, ITERATE_RTOL_PCG)
    o.close()


def test_pcg_schur_fp32_inner_preconditioner_is_only_a_preconditioner(gpu_required, monkeypatch):
    """opt-in QPDO_PCG_INNER_F32: the inner solve of the Schur mode streams an fp32 copy of the compact matrix values
    (slab kernels forced so that the fp32 path is taken at this size); the outer CG runs on the exact fp64 operator
    to the same tolerance, so counts and iterates must not move beyond the PCG tolerance"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_SPMV", "slab")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    p = problems.random_qp(62, 800, 1500, 0.03, 0)
    monkeypatch.setenv("QPDO_PCG_INNER_F32", "0")
    r0 = solver.solve_problem(p, verbose=0)
    monkeypatch.setenv("QPDO_PCG_INNER_F32", "1")
    r1 = solver.solve_problem(p, verbose=0)
    assert r0["stats"]["schur_passes"] > 0 and r1["stats"]["schur_passes"] > 0
    assert_same_outcome(r1, r0["info"], r0["x"], r0["y"], p, ITERATE_RTOL_PCG)
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    assert_same_outcome(r1, ro["info"], ro["x"], ro["y"], p, ITERATE_RTOL_PCG)
    o.close()


BIG = sorted(f[4:-4] for f in os.listdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
             if f.startswith("big_") and f.endswith(".npz"))


@pytest.mark.parametrize("name", BIG)
def test_production_size_matches_oracle_fixture(name, gpu_required, monkeypatch):
    """Production sizes against committed oracle fixtures (tests/golden/big_<name>.npz, written by
    tests/golden/make_golden_big.py with the oracle's direct LDL' = the reference's algorithm, src/qpdo.c:343-449,
    src/newton.c:21-33).  The device runs its DEFAULT solver selection -- no QPDO_* override: dense MFMA LDL' with
    look-ahead and low-rank updates at C2 (BASELINE.json configs[1], full size; its first passes through PCG), PCG in Schur-complement mode over
    the auto-selected LDS-staged slab kernels above QPDO_DENSE_MAX_N.  Bar: status, iterations, oterations and the
    per-pass kind / n_active / n_enter / n_leave / factor branch IDENTICAL; tau and the four residual norms per pass
    and the final iterates within the stated tolerances; plus the size-independent properties."""
    for k in [k for k in os.environ if k.startswith("QPDO_") and k not in ("QPDO_DEVICE",)]:
        monkeypatch.delenv(k)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    p = golden_problem(meta["spec"])
    assert (p["n"], p["m"]) == (meta["n"], meta["m"])
    r = solver.solve_problem(p, verbose=0, **meta["settings"])
    band = r["stats"]["linsolve"] == 3                      # chain-structured instances: the band direct solver (exact, like the dense one)
    assert band == ("banded" in meta["spec"])
    dense = r["stats"]["linsolve"] == 1 or band
    assert band or (r["stats"]["linsolve"] == 1) == (p["n"] <= 12288)      # the default selection, not an override
    gi, oi = r["info"], meta["info"]
    assert (gi["status_val"], gi["iterations"], gi["oterations"]) == (oi["status_val"], oi["iterations"], oi["oterations"])
    assert_same_trace(r["trace"], trace_from_npz(z), pcg=not dense, tau_rtol=TAU_RTOL_PCG_C4_FULL if name == "C4_full" else None)
    rt = ITERATE_RTOL if dense else ITERATE_RTOL_PCG
    assert close_vec(r["x"], z["x"], rt), np.abs(r["x"] - z["x"]).max()
    assert close_vec(r["y"], z["y"], rt), np.abs(r["y"] - z["y"]).max()
    assert abs(gi["objective"] - oi["objective"]) <= 1e-9 * max(1.0, abs(oi["objective"]))
    if band:
        assert r["stats"]["factor_count"] > 0 and r["stats"]["lin_iters"] == 0
    elif dense:
        assert r["stats"]["lowrank_solves"] > 0              # the kept-factor update path took part
        if p["n"] >= 8192:                                   # default from n = 8192: the first passes through PCG, then the dense factor (QPDO_HYBRID)
            assert r["stats"]["lin_iters"] > 0 and r["stats"]["factor_count"] > 0
    else:
        assert r["stats"]["schur_passes"] > 0
    # size-independent properties: independently recomputed KKT residuals, agreement with the reported norms, complementarity
    rp, rd = problems.kkt_residuals(p, r["x"], r["y"])
    if gi["status_val"] == 1:        # (a record cut off by max_iter -- the first passes of C4 -- is an iterate in flight, not a solution,
        #                               and its reported norms belong to the start of the last pass, not to the final iterate)
        assert abs(rp - gi["res_prim_norm"]) <= 1e-9 and abs(rd - gi["res_dual_norm"]) <= 1e-9
        assert rp <= 1e-6 and rd <= 1e-6
        # north star: "final KKT residual within 1e-10" of the reference's (here: the oracle's record of the same solve)
        assert abs(gi["res_prim_norm"] - oi["res_prim_norm"]) <= KKT_ATOL and abs(gi["res_dual_norm"] - oi["res_dual_norm"]) <= KKT_ATOL
        Ax = p["A"] @ r["x"]
        inside = (Ax > p["l"] + 1e-5) & (Ax < p["u"] - 1e-5)
        assert np.abs(r["y"][inside]).max() <= 1e-5


def _fixture(name):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    return z, meta, golden_problem(meta["spec"])


@pytest.mark.parametrize("name", [n for n in ("banded_20k", "banded_20k_noprox") if n in BIG])
@pytest.mark.parametrize("how", ["forced-dense", "pcg-rescued"])
def test_direct_solver_above_the_former_lds_limit(name, how, gpu_required, monkeypatch):
    """The reference factors whatever Newton matrix it is given (CHOLMOD, cholmod_interface.c:8-52).  Until round 4 the dense direct
    solver here stopped at n = 18000 (its assembly kept an n-double accumulator in LDS) and a PCG solve that could not converge above
    that order ended qpdo_solve with QPDO_ERROR.  The assembly now tiles its accumulator, so the direct solver is bounded by HBM
    (n <= 40000) and is the rescue of a failed PCG solve up to that order.  n = 20000, chain-structured (banded) QP, against the
    oracle's record: (a) the dense solver selected outright; (b) PCG, cut off after 40 iterations per solve so that its first real
    solve fails, redone by the dense solver, which the workspace keeps -- same status, counts, per-pass integers, iterates."""
    for k in [k for k in os.environ if k.startswith("QPDO_") and k not in ("QPDO_DEVICE",)]:
        monkeypatch.delenv(k)
    if how == "forced-dense":
        monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    else:
        monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
        monkeypatch.setenv("QPDO_PCG_MAXIT", "40")
    z, meta, p = _fixture(name)
    assert p["n"] > 18000
    r = solver.solve_problem(p, verbose=0, **meta["settings"])
    st = r["stats"]
    if how == "forced-dense":
        assert st["linsolve"] == 1 and st["factor_count"] > 0 and st["pcg_dense_fallbacks"] == 0
    else:
        assert st["pcg_dense_fallbacks"] == 1 and st["factor_count"] > 0
    gi, oi = r["info"], meta["info"]
    assert (gi["status_val"], gi["iterations"], gi["oterations"]) == (oi["status_val"], oi["iterations"], oi["oterations"])
    assert_same_trace(r["trace"], trace_from_npz(z), pcg=(how != "forced-dense"))
    rt = ITERATE_RTOL if how == "forced-dense" else ITERATE_RTOL_PCG
    assert close_vec(r["x"], z["x"], rt), np.abs(r["x"] - z["x"]).max()
    assert close_vec(r["y"], z["y"], rt), np.abs(r["y"] - z["y"]).max()
    assert abs(gi["res_prim_norm"] - oi["res_prim_norm"]) <= KKT_ATOL and abs(gi["res_dual_norm"] - oi["res_dual_norm"]) <= KKT_ATOL


def test_tiled_dense_assembly_leaves_the_same_bits(gpu_required, monkeypatch):
    """the assembly's LDS accumulator in tiles of 512 rows (as any order above ~19000 needs) against one tile: every element receives its
    contributions in the same ascending row order, so the factor, the trace and the solution carry the same bits"""
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    p = problems.random_qp(5, 3000, 5000, 0.02, 100)
    a = solver.solve_problem(p, verbose=0)
    monkeypatch.setenv("QPDO_DENSE_ASM_TILE", "512")
    b = solver.solve_problem(p, verbose=0)
    assert a["stats"]["factor_count"] == b["stats"]["factor_count"] > 0
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])
    assert len(a["trace"]) == len(b["trace"]) and all(ta[k] == tb[k] for ta, tb in zip(a["trace"], b["trace"]) for k in ta)


def test_fp32_inner_preconditioner_keeps_the_c4_fixture_integers(gpu_required, monkeypatch):
    """QPDO_PCG_INNER_F32=1 (opt-in, never the measured configuration): the Schur mode's inner solve streams an fp32 copy of the compact
    matrix values; it only defines a preconditioner, the outer CG runs on the exact K in fp64.  Claimed: the same pass counts and
    per-pass integers as the complete oracle record of the metric's configuration, iterates within the PCG tolerance -- tested here,
    not just benchmarked."""
    for k in [k for k in os.environ if k.startswith("QPDO_") and k not in ("QPDO_DEVICE",)]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("QPDO_PCG_INNER_F32", "1")
    z, meta, p = _fixture("C4_full")
    r = solver.solve_problem(p, verbose=0, **meta["settings"])
    gi, oi = r["info"], meta["info"]
    assert r["stats"]["schur_passes"] >= 50
    assert (gi["status_val"], gi["iterations"], gi["oterations"]) == (oi["status_val"], oi["iterations"], oi["oterations"])
    assert_same_trace(r["trace"], trace_from_npz(z), pcg=True, tau_rtol=TAU_RTOL_PCG_C4_FULL)
    assert close_vec(r["x"], z["x"], ITERATE_RTOL_PCG) and close_vec(r["y"], z["y"], ITERATE_RTOL_PCG)
    assert abs(gi["res_prim_norm"] - oi["res_prim_norm"]) <= KKT_ATOL and abs(gi["res_dual_norm"] - oi["res_dual_norm"]) <= KKT_ATOL


def test_config4_full_size_properties(gpu_required):
    """BASELINE.json metric configuration: n=1e5, m=2e5, 1 % fill (2e8 + 1e8 nonzeros, LDS-staged slab kernels over
    the slab-major image, deflated Jacobi-PCG).  No oracle reaches this size; checked through size-independent
    properties: the three products against scipy's CSC products on the same arrays, then a full cold-start solve:
    status, independently recomputed KKT residuals, agreement with the reported norms, complementarity."""
    p = problems.config_qp("C4")
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
    assert s.stats()["linsolve"] == 0
    rng = np.random.default_rng(4)
    xn, ym = rng.standard_normal(p["n"]), rng.standard_normal(p["m"])
    Qf = problems.full_Q(p)
    for which, M, v in ((0, p["A"], xn), (1, p["A"].T.tocsr(), ym), (2, Qf, xn)):
        ref = M @ v
        bound = abs(M) @ np.abs(v)
        got = s.spmv(which, v)
        assert np.all(np.abs(got - ref) <= 1e-13 * bound + 1e-300), which
    s.delete()
    r = solver.solve_problem(p, verbose=0)
    assert r["info"]["status_val"] == 1
    rp, rd = problems.kkt_residuals(p, r["x"], r["y"])
    assert rp <= 1e-6 and rd <= 1e-6
    assert abs(rp - r["info"]["res_prim_norm"]) <= 1e-9 and abs(rd - r["info"]["res_dual_norm"]) <= 1e-9
    Ax = p["A"] @ r["x"]
    inside = (Ax > p["l"] + 1e-5) & (Ax < p["u"] - 1e-5)
    assert np.abs(r["y"][inside]).max() <= 1e-5


@pytest.mark.parametrize("mode", ["fused", "threads"])
def test_batch_of_mpc_sized_qps_matches_oracle(mode, gpu_required, monkeypatch):
    """BASELINE.json configs[2] (n=120, m=360 with equality rows), a slice of the batch, plus other small
    shapes and the three reference known-answer QPs in the same batch.  Every item must match the oracle in
    status / iterations / oterations; the fused one-workgroup-per-QP kernel follows the oracle's operation
    order exactly, so its iterates are required to be BIT-IDENTICAL."""
    if mode == "threads":
        monkeypatch.setenv("QPDO_BATCH", "threads")
    probs = [problems.config_qp("C3", i) for i in range(20)]
    probs += [problems.config_qp("C1b", 0), problems.random_qp(26, 64, 1, 0.2), problems.random_qp(27, 1, 5, 1.0),
              problems.random_qp(23, 150, 300, 0.05, 50)]
    res, failed = solver.solve_batch(probs, nthreads=8, verbose=0)
    assert failed == 0
    for p, r in zip(probs, res):
        o = ob.OracleSolver(p, ob.default_settings())
        ro = o.solve()
        assert (r["info"]["status_val"], r["info"]["iterations"], r["info"]["oterations"]) == \
               (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"])
        if mode == "fused":
            assert np.array_equal(r["x"], ro["x"]) and np.array_equal(r["y"], ro["y"])
            assert r["info"]["objective"] == ro["info"]["objective"]
            assert r["info"]["res_prim_norm"] == ro["info"]["res_prim_norm"]
        else:
            assert close_vec(r["x"], ro["x"]) and close_vec(r["y"], ro["y"])
        o.close()


def test_fused_batch_known_answers(gpu_required):
    """reference examples/infeasibility_tests.m through the fused batch kernel"""
    probs = [problems.infeasibility_kat(c) for c in ("degenerate", "primal_infeasible", "dual_infeasible")]
    res, failed = solver.solve_batch(probs, verbose=0, max_iter=100)
    assert failed == 0
    assert [r["info"]["status_val"] for r in res] == [1, -3, -4]
    for p, r in zip(probs, res):
        o = ob.OracleSolver(p, ob.default_settings(max_iter=100)); ro = o.solve()
        assert (r["info"]["iterations"], r["info"]["oterations"]) == (ro["info"]["iterations"], ro["info"]["oterations"])
        o.close()


def test_matrix_storage_variants_give_identical_results(gpu_required):
    """the ABI accepts Q as lower (stype -1, what the reference's mex passes), upper (+1) or full (0) storage
    and int32 or int64 indices (reference DINT / DLONG builds): same instance, same bits out"""
    import scipy.sparse as sp
    p = problems.random_qp(51, 120, 200, 0.06)
    Qf = problems.full_Q(p)
    base = None
    for Qm, st, idt in [(p["Q"], -1, np.int64), (sp.triu(Qf).tocsc(), 1, np.int64), (Qf, 0, np.int64), (p["Q"], -1, np.int32)]:
        s = solver.QPDO().setup(Qm, p["q"], p["A"], p["l"], p["u"], Qstype=st, index_dtype=idt, verbose=0)
        r = s.solve()
        s.delete()
        if base is None:
            base = r
        else:
            assert r["info"]["iterations"] == base["info"]["iterations"]
            assert np.array_equal(r["x"], base["x"]) and np.array_equal(r["y"], base["y"])


@pytest.mark.parametrize("shape", [(120, 200, 0.06, 0), (700, 300, 0.2, 40), (3000, 70000, 0.002, 100), (2048, 4096, 0.01, 0), (1, 5, 1.0, 0),
                                   (40, 0, 0.1, 0)])
def test_device_setup_matches_host_setup(shape, gpu_required, monkeypatch):
    """qpdo_setup's matrix conversions (CSC -> CSR(A), stored triangle -> full symmetric CSR(Q)) run on the device by default (a stable
    radix transposition, dev/transpose.inc); QPDO_SETUP_HOST=1 keeps the OpenMP loops of the host.  Integer work: the arrays must be
    the same, so the three products and the whole solve carry the same bits -- for lower / upper / full storage of Q, 32- and 64-bit
    indices, wide (more than one radix pass over the row index), empty (m = 0) and one-column shapes.  The conversions' row pointers come
    from the device-wide scan in 2048-entry tiles: 35, 7 and 2 tiles with ragged ends at (3000, 70000), exactly one and exactly two at
    (2048, 4096).  (Also forced onto the generic path: small shapes would otherwise run through the fused kernel, which reads the same arrays.)"""
    import scipy.sparse as sp
    n, m, dens, neq = shape
    monkeypatch.setenv("QPDO_SMALL_FUSED", "0")
    if m > 0:
        p = problems.random_qp(77, n, m, dens, neq)
    else:
        p = problems.random_qp(77, n, 4, dens, 0)
        p["A"], p["l"], p["u"], p["m"] = sp.csc_matrix((0, n)), np.zeros(0), np.zeros(0), 0
    Qf = problems.full_Q(p)
    rng = np.random.default_rng(1)
    vn, vm = rng.standard_normal(p["n"]), rng.standard_normal(p["m"])
    for Qm, st, idt in [(p["Q"], -1, np.int32), (sp.triu(Qf).tocsc(), 1, np.int64), (Qf, 0, np.int32)]:
        outs = []
        for host in ("1", "0"):
            monkeypatch.setenv("QPDO_SETUP_HOST", host)
            s = solver.QPDO().setup(Qm, p["q"], p["A"], p["l"], p["u"], Qstype=st, index_dtype=idt, verbose=0, max_iter=60)
            prods = (s.spmv(0, vn) if p["m"] else np.zeros(0), s.spmv(1, vm) if p["m"] else np.zeros(p["n"]), s.spmv(2, vn))
            r = s.solve()
            outs.append((prods, r, s.trace()))
            s.delete()
        (pa, ra, ta), (pb, rb, tb) = outs
        for a, b in zip(pa, pb):
            assert np.array_equal(a, b)
        assert (ra["info"]["status_val"], ra["info"]["iterations"]) == (rb["info"]["status_val"], rb["info"]["iterations"])
        assert np.array_equal(ra["x"], rb["x"], equal_nan=True) and np.array_equal(ra["y"], rb["y"], equal_nan=True)
        assert all(x[k] == y[k] for x, y in zip(ta, tb) for k in x)


def test_threaded_setup_conversions_give_identical_results(gpu_required, monkeypatch):
    """qpdo_setup converts CSC -> CSR with several host threads (column ranges, per-thread row counts); the arrays
    must be the ones the single-threaded counting pass produces: same bits out of the solve"""
    import scipy.sparse as sp
    p = problems.random_qp(52, 300, 500, 0.05, 20)
    Qf = problems.full_Q(p)
    base = None
    monkeypatch.setenv("QPDO_SETUP_HOST", "1")               # (the host conversions: the row-partitioned workspaces still use them)
    for threads in ("1", "7", "16"):
        monkeypatch.setenv("QPDO_SETUP_THREADS", threads)
        for Qm, st in [(p["Q"], -1), (sp.triu(Qf).tocsc(), 1)]:
            s = solver.QPDO().setup(Qm, p["q"], p["A"], p["l"], p["u"], Qstype=st, verbose=0)
            y = s.spmv(0, np.arange(p["n"], dtype=float)); z = s.spmv(2, np.arange(p["n"], dtype=float))
            r = s.solve()
            s.delete()
            if base is None:
                base = (r, y, z)
            else:
                assert np.array_equal(y, base[1]) and np.array_equal(z, base[2])
                assert r["info"]["iterations"] == base[0]["info"]["iterations"]
                assert np.array_equal(r["x"], base[0]["x"]) and np.array_equal(r["y"], base[0]["y"])


def test_problem_without_constraints(gpu_required, linsolve):
    """m = 0: the solve degenerates to (Q + sigma I) steps; every kernel must cope with empty m-vectors"""
    import scipy.sparse as sp
    p = problems.random_qp(52, 80, 1, 0.1)
    p["A"] = sp.csc_matrix((0, 80)); p["l"] = np.zeros(0); p["u"] = np.zeros(0); p["m"] = 0
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    r = solver.solve_problem(p, verbose=0)
    assert (r["info"]["status_val"], r["info"]["iterations"], r["info"]["oterations"]) == \
           (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"])
    assert close_vec(r["x"], ro["x"], 1e-8)
    Q = problems.full_Q(p)
    assert np.abs(Q @ r["x"] + p["q"]).max() <= 1e-6
    o.close()


def test_verbose_iteration_lines(gpu_required, capfd):
    """settings.verbose prints the reference's per-pass line (src/util.c:112-117) and the outer-update separators"""
    p = problems.config_qp("C1b")
    r = solver.solve_problem(p, verbose=1, print_interval=1)
    out = capfd.readouterr().out
    assert "iter |  objective     r.prim     r.dual |  r.p. in    r.d. in   stepsize |" in out
    lines = [l for l in out.splitlines() if l.strip() and l.lstrip()[0].isdigit() and "|" in l]
    assert len([l for l in lines if "---" not in l and "--  --" not in l]) >= r["info"]["iterations"]
    assert len([l for l in lines if "|----" in l]) == r["info"]["oterations"]
    assert "QPDO finished successfully." in out


def test_status_is_not_reset_between_solves_like_the_reference(gpu_required, monkeypatch):
    """reference src/qpdo.c:451-453 vs :200: a second solve that runs out of iterations keeps the
    SOLVED status of the first; QPDO_FIX_STATUS_RESET=1 switches the quirk off.  Oracle and HIP path agree."""
    p = problems.config_qp("C1b")
    o = ob.OracleSolver(p, ob.default_settings())
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    assert o.solve()["info"]["status_val"] == 1 and s.solve()["info"]["status_val"] == 1
    o.update_settings(ob.default_settings(max_iter=2)); s.update_settings(max_iter=2)
    ro, rg = o.solve(), s.solve()
    assert ro["info"]["iterations"] == rg["info"]["iterations"] == 2
    assert ro["info"]["status_val"] == rg["info"]["status_val"] == 1          # stale status, as in the reference
    s.delete(); o.close()
    monkeypatch.setenv("QPDO_FIX_STATUS_RESET", "1")
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    s.solve(); s.update_settings(max_iter=2)
    assert s.solve()["info"]["status_val"] == -5
    s.delete()


def test_update_bounds_rejects_crossed_bounds(gpu_required):
    """reference src/qpdo.c:526-536: l > u => QPDO_ERROR and the stored bounds stay untouched"""
    p = problems.config_qp("C1b")
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    before = s.download("l")
    s.update_bounds(p["u"] + 1.0, p["u"])
    assert s.info()["status_val"] == -99 and np.array_equal(s.download("l"), before)
    s.delete()


def _lp_like(seed, n, m, qdiag):
    import scipy.sparse as sp
    p = problems.random_qp(seed, n, m, 0.1)
    p["Q"] = sp.diags(np.full(n, qdiag)).tocsc() if qdiag > 0 else sp.csc_matrix((n, n))
    return p


@pytest.mark.parametrize("qdiag", [0.0, 1e-3])
def test_lp_and_diagonal_q(qdiag, linsolve, gpu_required):
    """Q = 0 (an LP: the proximal term alone makes the Newton system definite) and a weak diagonal Q"""
    p = _lp_like(61, 40, 120, qdiag)
    o = ob.OracleSolver(p, ob.default_settings(max_iter=400))
    ro = o.solve()
    r = solver.solve_problem(p, verbose=0, max_iter=400)
    assert (r["info"]["status_val"], r["info"]["iterations"], r["info"]["oterations"]) == \
           (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"])
    if ro["info"]["status_val"] == 1:
        assert close_vec(r["x"], ro["x"], 1e-7) and close_vec(r["y"], ro["y"], 1e-7)
    o.close()


def test_constructed_primal_infeasible_instance(linsolve, gpu_required):
    """two identical rows with disjoint bounds: no x satisfies both; the certificate path (reference
    src/termination.c:97-151) must fire with the same pass counts as the oracle"""
    import scipy.sparse as sp
    p = problems.random_qp(62, 30, 60, 0.15)
    A = p["A"].tolil()
    A[1, :] = A[0, :]
    p["A"] = A.tocsc()
    p["l"][0], p["u"][0] = 1.0, 2.0
    p["l"][1], p["u"][1] = -2.0, -1.0
    o = ob.OracleSolver(p, ob.default_settings(max_iter=500))
    ro = o.solve()
    r = solver.solve_problem(p, verbose=0, max_iter=500)
    assert ro["info"]["status_val"] == -3
    assert (r["info"]["status_val"], r["info"]["iterations"], r["info"]["oterations"]) == \
           (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"])
    dy = r["prim_inf_cert"]
    assert np.abs(p["A"].T @ dy).max() <= 1e-5 * np.abs(dy).max()
    o.close()


def test_fused_batch_honours_max_time_and_fills_times(gpu_required):
    """round-1 advisor finding: the fused one-workgroup-per-QP path ignored settings->max_time and left the PROFILING times
    of QPDOInfo at zero.  Reference: src/qpdo.c:441-447 (checked at the end of every pass), :461-464."""
    probs = [problems.config_qp("C3", i) for i in range(8)]
    res, failed = solver.solve_batch(probs, verbose=0)
    assert failed == 0
    for r in res:
        i = r["info"]
        assert i["status_val"] == 1 and i["solve_time"] > 0 and i["setup_time"] > 0
        assert abs(i["run_time"] - (i["setup_time"] + i["solve_time"])) <= 1e-12
    res, failed = solver.solve_batch(probs, verbose=0, max_time=1e-7)
    assert failed == 0
    for r in res:
        assert r["info"]["status_val"] == -6 and r["info"]["status"] == "max time exceeded"
        assert r["info"]["iterations"] == 0                    # stopped at the end of pass 0, iter not advanced (qpdo.c:441-447)


def test_batch_with_inconsistent_dimensions_is_rejected_not_indexed(gpu_required, capfd):
    """round-1 advisor finding: qdev_small_eligible skipped the checks of qpdo_setup.  An item whose Q is not n x n must take
    the generic path, which refuses it (QPDO_ERROR for that item) -- the other items are still solved"""
    import scipy.sparse as sp
    probs = [problems.config_qp("C3", i) for i in range(3)]
    bad = dict(probs[1]); bad["Q"] = sp.csc_matrix(sp.eye(50)); probs[1] = bad      # 50 x 50 against n = 120
    res, failed = solver.solve_batch(probs, verbose=0)
    assert failed == 1
    assert res[1]["info"]["status_val"] == -99
    assert res[0]["info"]["status_val"] == 1 and res[2]["info"]["status_val"] == 1
    assert "dimensions do not match" in capfd.readouterr().out


def test_pcg_that_cannot_converge_is_an_error_not_a_silent_step(gpu_required, monkeypatch):
    """round-1 advisor finding: pcg_solve returned 0 whether or not CG converged.  With an iteration cap far below what the
    Newton systems need, the solve must end with QPDO_ERROR and a message, never continue on an arbitrary dx"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "0")
    monkeypatch.setenv("QPDO_PCG_MAXIT", "3")
    monkeypatch.setenv("QPDO_PCG_DENSE_FALLBACK", "0")
    p = problems.random_qp(22, 150, 300, 0.05, 0)
    r = solver.solve_problem(p, verbose=0)
    assert r["info"]["status_val"] == -99
    assert "did not converge" in solver.lib().qpdo_amd_last_error().decode()
    # default: the pass whose PCG solve cannot converge is redone by the dense LDL' solver (the reference factorizes, it never fails
    # for lack of iterations), which the workspace then keeps: the outcome is the oracle's
    monkeypatch.delenv("QPDO_PCG_DENSE_FALLBACK")
    r = solver.solve_problem(p, verbose=0)
    o = ob.OracleSolver(p, ob.default_settings()); ro = o.solve(); to = o.trace(); o.close()
    assert r["stats"]["pcg_dense_fallbacks"] == 1 and r["stats"]["factor_count"] >= 1
    assert_same_outcome(r, ro["info"], ro["x"], ro["y"], p)
    assert_same_trace(r["trace"], to)
    monkeypatch.delenv("QPDO_PCG_MAXIT")
    r = solver.solve_problem(p, verbose=0)
    assert r["info"]["status_val"] == 1 and r["stats"]["pcg_soft_accepts"] == 0
    # (every solve ended by its stopping rule: relative 1e-12, or 1e-5 eps_abs in the unscaled inf-norm -- the latter may leave a
    # relative residual far above 1e-12 when the right-hand side of a late pass is itself of the order of 1e-6)


def test_lost_producer_of_a_chained_solve_is_redone_stepwise_not_an_error(gpu_required, tmp_path):
    """round-1 advisor finding: a chained triangular solve that loses a producer ended the whole qpdo_solve with QPDO_ERROR.  Now the
    iterate update of that pass is skipped on the device and the step is redone with the stepwise solves on a fresh factor; injected
    at Newton pass 3, the solve must still reproduce the oracle -- counts, trace, iterates.  The injection hook is compiled only into a
    TEST build of the library (-DQPDO_TEST_HOOKS, _build.build_lib_testhooks), loaded by a child process through QPDO_AMD_LIB: the
    product library does not contain it."""
    import json, subprocess, sys
    from qpdo_amd import _build
    so = _build.build_lib_testhooks(str(tmp_path))
    code = r"""
import json, os, sys
sys.path.insert(0, %r)
from qpdo_amd import problems, solver
p = problems.random_qp(43, 1000, 700, 0.03, 50)
r = solver.solve_problem(p, verbose=0)
print(json.dumps(dict(info=r["info"], x=r["x"].tolist(), y=r["y"].tolist(), stats=r["stats"], trace=r["trace"])))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, QPDO_LINSOLVE="dense", QPDO_DENSE_CHAIN_INJECT="3")
    outs = {}
    for label, libpath in (("hooks", so), ("product", None)):
        e = dict(env)
        if libpath:
            e["QPDO_AMD_LIB"] = libpath
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=e)
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
        outs[label] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert outs["hooks"]["stats"]["chain_fallbacks"] == 1
    assert outs["product"]["stats"]["chain_fallbacks"] == 0           # the product library ignores the variable: no hook in it
    p = problems.random_qp(43, 1000, 700, 0.03, 50)
    o = ob.OracleSolver(p, ob.default_settings())
    ro = o.solve()
    for r in outs.values():
        r = dict(r, x=np.array(r["x"]), y=np.array(r["y"]))
        assert_same_outcome(r, ro["info"], ro["x"], ro["y"], p)
        assert_same_trace(r["trace"], o.trace())
    o.close()
