"""The PCG linear-solve path tested piece by piece (qpdo_amd_pcg_probe, qpdo_amd_download_compact; scaling = 0, so the device's matrices
are the caller's) against tests/pcg_ref.py: (a) the per-pass compact index space and matrices, bit for bit; (b) one K product under the
componentwise bound (r_Q + r_A + r_A' + 4) u (|Q| + sigma I + |A|' D |A|) |p| and its p.Kp partial sums; (c) the Jacobi, Dq and Schur
diagonals at (row length + 3) u, the deflation set and S^-1; (d) whole linear solves: the true residual in extended precision under
PCG_TOL ||b|| + c u ||K|| ||x||, iteration counts against a textbook fp64 CG, the route that ran, bit-identical repeats.
tests/test_pcg_checks_cpu.py shows on the CPU that every one of these checks fails on a subtly wrong input.

Largest measured ratios on the MI355X (test_zz_report prints them; every bound is <= 1 unless stated):
  K p, 152 probes at m = 1 .. 1089 (LDS-table compaction) ... componentwise 0.18, p.Kp partial sums 0.0067
  K p with k = 0 or m = 0 (12 probes) ...................... componentwise 0.19, p.Kp 0.053
  K p, slab kernels (10 probes) ............................ componentwise 0.088, p.Kp 1.7e-5
  K p, m = 330000 (the compaction without LDS tables) ..... componentwise 0.0020, p.Kp 1.1e-4; the compact matrices equal the reference's
  diagonals ................................................ Jacobi 0.47, Dq 0.33, Schur inner 0.60, deflated remainder 0.48
  Jacobi route, 12 solves .................................. iteration count within 2 of the reference CG's; c needed: none (every true
                                                             residual is below PCG_TOL ||b|| by itself)
  Schur route, 12 solves ................................... 8 or 9 outer steps against 77 .. 99 Jacobi iterations; c needed: none
  deflated solve ........................................... defl_r = 40, |Sinv S - I| = 1.5e-21 kappa(S) (S is diagonal here), c needed 0.026
Residual bound: c = 4.  The fp64 reference CG (tests/pcg_ref.py, measured in tests/test_pcg_checks_cpu.py) needs c = 0.17 at most on these
systems (the deflation system; on every other one its true residual meets PCG_TOL ||b|| outright, the ratio is negative); twice that is
below the floor of 4.  The device needs 0.026 at most.
The whole file runs in about 6 s on the MI355X.
"""
import json
import os

import numpy as np
import pytest

import pcg_ref as R
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QPDO_LINSOLVE", "QPDO_SPMV", "QPDO_IDX16", "QPDO_PCG_SCHUR", "QPDO_INNER_FOLD", "QPDO_PCG_GRAPH", "QPDO_DEFLATE", "QPDO_PCG_MAXIT",
            "QPDO_PCG_TOL", "QPDO_PCG_INNER_F32", "QPDO_HYBRID", "QPDO_SMALL_FUSED", "QPDO_PCG_DENSE_FALLBACK")
REPORT = {}


def _note(group, **vals):
    g = REPORT.setdefault(group, {"cases": 0})
    for k, v in vals.items():
        g[k] = max(g.get(k, -np.inf), float(v))
    g["cases"] += 1


def _workspace(monkeypatch, Qf, A, env=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    n, m = Qf.shape[0], A.shape[0]
    ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    assert ws.stats()["linsolve"] == 0
    return ws


def _download(ws):
    g = ws.compact_geometry()
    got = dict(k=g["k"], Arc=None, Atc=None)
    for name in ("rowlist", "cidx", "dc", "flag_bits", "flag_wprefix"):
        got[name] = ws.download_compact_vector(name)
    if g["k"]:
        got["Arc"], got["Atc"] = ws.download_compact_matrix("Arc"), ws.download_compact_matrix("Atc")
    else:
        with pytest.raises(RuntimeError):
            ws.download_compact_matrix("Arc")
    return got


def check_probe(ws, Qf, A, sigma, dw, p, group, tag):
    """one mode-0 probe: the compact structures exactly, K p and the p.Kp partial sums under their bounds, the same bits twice"""
    Kp, info = ws.pcg_K_product(dw, sigma, p)
    got = _download(ws)
    ix, arc, atc = R.compact_matrices(A, dw)
    assert info["kact"] == ix["k"], tag
    bad = R.compaction_mismatch(got, ix, arc, atc)
    assert bad is None, (tag, bad)
    ref, absvec, r = R.K_product(Qf, A, sigma, dw, p)
    ratio = R.K_product_ratio(Kp, ref, absvec, r, R.underflow_term(A, r))
    pr = R.pKp_ratio(info["partials"], p, ref, absvec, r)
    print("%s %s: k = %d, K p ratio %.3g, p.Kp ratio %.3g (%d partials)" % (group, tag, ix["k"], ratio, pr, info["cnt"]))
    _note(group, Kp=ratio, pKp=pr)
    assert 1 <= info["cnt"] <= 1024
    assert ratio <= 1.0, (tag, ratio)
    assert pr <= 1.0, (tag, pr)
    Kp2, info2 = ws.pcg_K_product(dw, sigma, p)
    assert np.array_equal(Kp2.view(np.uint64), Kp.view(np.uint64)) and np.array_equal(info2["partials"].view(np.uint64), info["partials"].view(np.uint64)), tag
    return got


# ---- (a) + (b): compaction, exact, and the K product on the same workspaces --------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 1024, 1025, 1089])
def test_compaction_and_K_product_every_pattern(m, gpu_required, monkeypatch):
    """row counts around the edges of the 64-row flag words (k_flag_words, their scan, k_flag_apply: a ragged last word, a full one, one
    row into the next, 1025 rows: 17 words)"""
    n = 200 + 37 * (m % 9)
    Qf, A = R.system(n, m, 1, empty_row=m // 2)
    ws = _workspace(monkeypatch, Qf, A)
    try:
        vecs = R.probe_vectors(n)
        for name, dw in R.weight_patterns(m).items():
            sigma = 1e-7 if name == "late_pass" else 1.0
            for vname in (("random", "e1", "spread") if name in ("all", "random30", "late_pass", "none") else ("random",)):
                got = check_probe(ws, Qf, A, sigma, dw, vecs[vname], "plain", "m=%d %s %s" % (m, name, vname))
            if name == "empty_row_weighted" and m > 2:
                j = int(got["cidx"][m // 2])
                assert got["rowlist"][j] == m // 2 and got["Arc"]["rp"][j] == got["Arc"]["rp"][j + 1]       # counted in k, an empty row of A_c
            if name == "none":
                assert got["k"] == 0
    finally:
        ws.delete()


def test_compaction_flag_words_cross_a_scan_tile(gpu_required, monkeypatch):
    """m = 131141: 2050 flag words, so their scan (2048-entry tiles) has a second tile, which holds two words; about half the rows
    weighted, some of them in those two words"""
    n, m = 300, 131141
    assert (m + 63) // 64 == 2050
    Qf, A = R.system(n, m, 5, per_row=3)
    dw = R.k_weights(m, m // 2, 17)
    assert np.count_nonzero(dw[2048 * 64:]) > 0 and np.count_nonzero(dw[2049 * 64:]) > 0
    ws = _workspace(monkeypatch, Qf, A)
    try:
        check_probe(ws, Qf, A, 1.0, dw, R.probe_vectors(n)["random"], "flag words in two scan tiles", "m=%d k=%d" % (m, m // 2))
    finally:
        ws.delete()


@pytest.mark.parametrize("n,m", [(1, 0), (1, 3), (300, 0)])
def test_K_product_without_weighted_rows_or_constraints(n, m, gpu_required, monkeypatch):
    """k = 0 and m = 0 take the Q product that carries the dot (EpiPcgQdot); n = 1"""
    Qf, A = R.system(n, m, 2)
    ws = _workspace(monkeypatch, Qf, A)
    try:
        for vname, p in R.probe_vectors(n).items():
            check_probe(ws, Qf, A, 0.5, np.zeros(m), p, "no rows", "n=%d m=%d zero weights %s" % (n, m, vname))
            if m:
                check_probe(ws, Qf, A, 0.5, R.weight_patterns(m)["all"], p, "no rows", "n=%d m=%d all %s" % (n, m, vname))
    finally:
        ws.delete()


@pytest.mark.parametrize("idx16", ["1", "0"])
def test_compaction_slab_thresholds(idx16, gpu_required, monkeypatch):
    """QPDO_SPMV=slab: A_c' takes the slab kernel and its own slab width from k = 1024, A_c from k = 4096"""
    n, m = 3000, 6000
    Qf, A = R.system(n, m, 3)
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_SPMV": "slab", "QPDO_IDX16": idx16})
    try:
        p = R.probe_vectors(n)["random"]
        for k in (1023, 1024, 4095, 4096):
            got = check_probe(ws, Qf, A, 1.0, R.k_weights(m, k, k), p, "slab", "idx16=%s k=%d" % (idx16, k))
            assert got["Atc"]["use_slab"] == int(k >= 1024) and got["Arc"]["use_slab"] == int(k >= 4096), k
            for M in (got["Arc"], got["Atc"]):
                assert M["has_ci16"] == (int(idx16) if M["use_slab"] else 0)
                if M["use_slab"] and idx16 == "1":
                    assert np.array_equal(M["ci16"], M["ci"] % M["W"])
    finally:
        ws.delete()


def test_compaction_two_slabs_of_the_parent(gpu_required, monkeypatch):
    """n = 30000: A has two column slabs; the compact copy chooses its own geometry or falls back to the parent's"""
    n, m = 30000, 6000
    Qf, A = R.system(n, m, 4)
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_SPMV": "slab"})
    try:
        p = R.probe_vectors(n)["random"]
        for k in (4096, 6000):
            got = check_probe(ws, Qf, A, 1.0, R.k_weights(m, k, k), p, "slab", "n=30000 k=%d" % k)
            assert got["Arc"]["use_slab"] == 1 and got["Arc"]["nslabs"] == 2 and got["Atc"]["use_slab"] == 1, got["Arc"]["nslabs"]
    finally:
        ws.delete()


# ---- (c) + (d): preconditioner pieces and solves -----------------------------------------------------------------------------------------
_KNORM = {}


def _knorm(key, Qf, A, sigma, dw):
    if key not in _KNORM:
        _KNORM[key] = R.norm2(R.K_sparse(Qf, A, sigma, dw))
    return _KNORM[key]


def check_solve(ws, Qf, A, sigma, dw, b, knorm, group, tag):
    x, info = ws.pcg_solve(dw, sigma, b)
    ratio = R.residual_ratio(Qf, A, sigma, dw, x, b, knorm)
    print("%s %s: iters %d (outer %d), residual needs c = %.3g" % (group, tag, info["iters"], info["outer"], ratio))
    _note(group, c_needed=ratio)
    assert ratio <= R.C_RESID, (tag, ratio)
    return x, info


@pytest.mark.parametrize("name", list(R.SOLVE_CASES))
def test_solves_and_preconditioner_pieces(name, gpu_required, monkeypatch):
    Qf, A, sigma, dw, env, route = R.solve_case(name)
    n = Qf.shape[0]
    knorm = _knorm(name, Qf, A, sigma, dw)
    ws = _workspace(monkeypatch, Qf, A, env)
    try:
        for rname, b in R.solve_rhs(Qf, A, sigma, dw).items():
            x, info = check_solve(ws, Qf, A, sigma, dw, b, knorm, route, "%s %s" % (name, rname))
            assert info["kact"] == SOLVE_K[name] and info["schur"] == (route == "schur") and info["defl_r"] == 0, info
            _, it_ref = R.jacobi_pcg(Qf, A, sigma, dw, b)
            if rname == "zero":
                assert info["iters"] == 0 and not x.any() and not np.signbit(x).any()
                continue
            if route == "jacobi":
                assert info["outer"] == info["iters"] and info["inner_solves"] == 0
                assert R.iterations_close(info["iters"], it_ref), (rname, info["iters"], it_ref)
                _note("jacobi", iteration_gap=abs(info["iters"] - it_ref))
            else:
                assert info["inner_solves"] == info["outer"] and info["iters"] > info["outer"] > 0, info
                assert info["outer"] <= it_ref, (rname, info["outer"], it_ref)
                _note("schur", outer_over_jacobi=info["outer"] / it_ref)
            x2, info2 = ws.pcg_solve(dw, sigma, b)
            assert np.array_equal(x2.view(np.uint64), x.view(np.uint64)) and info2["iters"] == info["iters"]
        # (c) the diagonals the last solve left
        pc = ws.download_compact_vector("pc_diag")
        if route == "jacobi":
            ref, cnt = R.jacobi_diagonal(Qf, A, sigma, dw)
            _note("diagonals", jacobi=R.diagonal_ratio(pc, ref, cnt))
            assert R.diagonal_ratio(pc, ref, cnt) <= 1.0
        else:
            dq, sd, lens = R.schur_diagonals(Qf, A, sigma, dw)
            s_diag = ws.download_compact_vector("s_diag")
            _note("diagonals", Dq=R.diagonal_ratio(pc, dq, np.zeros(n)), schur=R.diagonal_ratio(s_diag, sd, lens))
            assert R.diagonal_ratio(pc, dq, np.zeros(n)) <= 1.0 and R.diagonal_ratio(s_diag, sd, lens) <= 1.0
    finally:
        ws.delete()


SOLVE_K = {k: v[2] for k, v in R.SOLVE_CASES.items()}


def test_schur_inner_fold_on_and_off_give_the_same_bits(gpu_required, monkeypatch):
    Qf, A, sigma, dw, env, route = R.solve_case("schur_k600")
    b = R.solve_rhs(Qf, A, sigma, dw)["random"]
    out = []
    for fold in ("1", "0"):
        ws = _workspace(monkeypatch, Qf, A, {"QPDO_INNER_FOLD": fold})
        try:
            out.append(ws.pcg_solve(dw, sigma, b))
        finally:
            ws.delete()
    (x1, i1), (x0, i0) = out
    assert i1["schur"] and i0["schur"] and (i1["iters"], i1["outer"]) == (i0["iters"], i0["outer"])
    assert np.array_equal(x1.view(np.uint64), x0.view(np.uint64))


def test_graph_replay_on_and_off_give_the_same_bits(gpu_required, monkeypatch):
    Qf, A, sigma, dw, env, route = R.solve_case("jacobi_k200")
    b = R.solve_rhs(Qf, A, sigma, dw)["random"]
    out = []
    for graph in ("1", "0"):
        ws = _workspace(monkeypatch, Qf, A, {"QPDO_PCG_GRAPH": graph})
        try:
            out.append(ws.pcg_solve(dw, sigma, b))
        finally:
            ws.delete()
    (x1, i1), (x0, i0) = out
    assert not i1["schur"] and i1["iters"] == i0["iters"] and np.array_equal(x1.view(np.uint64), x0.view(np.uint64))


def test_deflated_solve(gpu_required, monkeypatch):
    Qf, A, sigma, dw = R.deflation_case()
    n = Qf.shape[0]
    knorm = _knorm("deflation", Qf, A, sigma, dw)
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_PCG_SCHUR": "0"})
    try:
        for rname, b in R.solve_rhs(Qf, A, sigma, dw).items():
            x, info = check_solve(ws, Qf, A, sigma, dw, b, knorm, "deflated", rname)
            assert info["defl_r"] == 40 and not info["schur"] and info["kact"] == 1500, info
            if rname == "zero":
                assert info["iters"] == 0 and not x.any()
        ix = R.index_space(dw)
        thr = R.deflation_threshold(ix["dc"])
        heavy = np.flatnonzero(ix["dc"] > thr)
        assert np.array_equal(ws.download_compact_vector("defl_list"), heavy)
        # P: the Jacobi diagonal of the remainder (the floor is not active on this system, tests/test_pcg_checks_cpu.py)
        P = ws.download_compact_vector("pc_diag")
        ref, cnt = R.jacobi_diagonal(Qf, A, sigma, np.where(dw > thr, 0.0, dw))
        _, cnt_full = R.jacobi_diagonal(Qf, A, sigma, dw)
        _note("diagonals", deflated_P=R.diagonal_ratio(P, ref, cnt_full))
        assert R.diagonal_ratio(P, ref, cnt_full) <= 1.0
        S = R.deflation_S(A, dw, ix["rows"], heavy, P).astype(np.float64)
        Sinv = ws.download_compact_vector("defl_Sinv")[:40, :40]
        err, kappa = float(np.abs(Sinv @ S - np.eye(40)).max()), float(np.linalg.cond(S))
        _note("deflated", Sinv_error_over_kappa=err / kappa)
        assert err <= 1e-10 * kappa, (err, kappa)
        # A_h': the heavy columns of A_c', same numbering
        Ath = ws.download_compact_matrix("Ath")
        _, arc, atc = R.compact_matrices(A, dw)
        keep = np.isin(atc["ci"], heavy)
        assert np.array_equal(Ath["ci"], atc["ci"][keep]) and np.array_equal(Ath["val"].view(np.uint64), atc["val"][keep].view(np.uint64))
    finally:
        ws.delete()


def test_capped_solve_is_refused_not_returned(gpu_required, monkeypatch):
    """the hook-level twin of test_pcg_that_cannot_converge_is_an_error_not_a_silent_step"""
    Qf, A, sigma, dw, env, route = R.solve_case("jacobi_schur_off")
    b = R.solve_rhs(Qf, A, sigma, dw)["random"]
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_PCG_SCHUR": "0", "QPDO_PCG_MAXIT": "3"})
    try:
        with pytest.raises(solver.PcgNotConverged) as e:
            ws.pcg_solve(dw, sigma, b)
        assert "did not converge" in str(e.value)
        x, info = ws.pcg_solve(dw, sigma, np.zeros(len(b)))            # and the workspace still serves the next call
        assert info["iters"] == 0 and not x.any()
    finally:
        ws.delete()


def test_probes_refuse_a_dense_workspace(gpu_required, monkeypatch):
    Qf, A = R.system(100, 80, 9)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    ws = solver.QPDO().setup(Qf, np.zeros(100), A, -np.ones(80), np.ones(80), scaling=0, verbose=0)
    try:
        with pytest.raises(RuntimeError) as e:
            ws.pcg_solve(np.ones(80), 1.0, np.ones(100))
        assert not isinstance(e.value, (solver.PcgNotConverged, solver.PcgNaN)) and "not PCG" in str(e.value)
        with pytest.raises(RuntimeError):
            ws.pcg_K_product(np.ones(80), 1.0, np.ones(100))
        with pytest.raises(RuntimeError):
            ws.compact_geometry()
    finally:
        ws.delete()


def test_probe_calls_leave_no_trace_on_the_next_solve(gpu_required, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    p = problems.random_qp(21, 600, 900, 0.02, 30)

    def make():
        return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p.get("Qstype", -1), c=p.get("c", 0.0), verbose=0)

    s1 = make()
    r1, t1, st1 = s1.solve(), s1.trace(), s1.stats()
    s1.delete()
    s2 = make()
    try:
        rng = np.random.default_rng(3)
        n, m = p["n"], p["m"]
        dw = R.k_weights(m, 400, 3)                                                  # 256 <= k <= 0.8 n: the Schur mode's state moves too
        s2.pcg_K_product(dw, 0.5, rng.standard_normal(n))
        _, i = s2.pcg_solve(dw, 0.5, rng.standard_normal(n))
        assert i["schur"]
        s2.pcg_solve(np.where(np.arange(m) < 100, 3.0, 0.0), 0.25, rng.standard_normal(n))
        s2.download_compact_matrix("Atc")
        r2, t2, st2 = s2.solve(), s2.trace(), s2.stats()
        s2.pcg_solve(dw, 0.25, rng.standard_normal(n))
        r3 = s2.solve()
    finally:
        s2.delete()
    s4 = make()
    s4.solve(); r4b = s4.solve()
    s4.delete()
    for a, b in ((r1, r2), (r4b, r3)):
        assert a["info"]["iterations"] == b["info"]["iterations"] and a["info"]["status_val"] == b["info"]["status_val"]
        assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
        assert np.array_equal(a["y"].view(np.uint64), b["y"].view(np.uint64))
    assert [tr["tau"] for tr in t1] == [tr["tau"] for tr in t2] and [tr["lin_iters"] for tr in t1] == [tr["lin_iters"] for tr in t2]
    for k in ("lin_iters", "spmv_calls", "inner_solves", "inner_steps", "schur_passes", "pcg_max_relres", "pcg_soft_accepts"):
        assert st1[k] == st2[k], (k, st1[k], st2[k])


# ---- the compaction branch for m > 327680 (placed last: it ran in no test, fixture or benchmark before this file) -----------------------------
def test_compaction_above_the_lds_table_limit(gpu_required, monkeypatch):
    """m = 330000 > 327680: the flags and the renumbering no longer fit the LDS tables, k_count_flagged / k_compact_rows with remap = cidx
    run instead.  The result must be what tests/pcg_ref.py gives -- the same reference the LDS-table branch is held to above."""
    n, m = 512, 330000
    rng = np.random.default_rng(77)
    import scipy.sparse as sp
    rows = np.concatenate([np.arange(m), rng.choice(m, m // 2, replace=False)])
    cols = rng.integers(0, n, len(rows))
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(m, n))
    A.sum_duplicates()
    A.sort_indices()
    Qf = R.dominant_Q(rng, n)
    ws = _workspace(monkeypatch, Qf, A)
    try:
        p = R.probe_vectors(n)["random"]
        val = 0.1 + 9.9 * rng.random(m)
        for name, dw in (("random30", np.where(rng.random(m) < 0.3, val, 0.0)), ("all", val), ("last", np.where(np.arange(m) == m - 1, val, 0.0))):
            check_probe(ws, Qf, A, 1.0, dw, p, "m = 330000", name)
    finally:
        ws.delete()


def test_zz_report():
    """prints the largest measured ratios per group (the figures quoted in the module docstring)"""
    print("\npcg pieces ratios: " + json.dumps(REPORT, sort_keys=True))
    out = os.environ.get("QPDO_PCG_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
