"""The Schur mode's refined inner solve (QPDO_PCG_INNER_REFINE, the default): the inner CG streams fp32 copies of the compact matrix
values and only proposes corrections; a solve is accepted on the residual formed with the fp64 matrices, against the same tolerance tau
as the fp64 inner CG.

(a) The slab kernel's fp32-stream instances on their own (qpdo_amd_pcg_probe modes 32 / 33, qpdo_amd_download_compact) against numpy with
the compact values rounded to float32, products and sums in longdouble: |y - y_ref| <= 1e-13 (|M32| |v|) componentwise.  The row sums are
fp64 sums of at most a few hundred exact-to-1-ulp products, so the worst-case bound is (row length + 1) 2^-53 (|M32| |v|) = 8e-14 for the
longest row here (700 entries) and 1e-13 holds for every row.  Shapes: 1, 2 and 5 / 6 column slabs, rows longer than one 256-entry trip
of a lane group, empty rows and empty (row, slab) segments, 20 rows per workgroup.
(b) Whole solves with the slab kernels forced, refinement on against QPDO_PCG_INNER_REFINE=0 and against the CPU oracle: the same
integers, iterates within ITERATE_RTOL_PCG, every accepted inner solve within tau on the fp64 residual, no fallback.
(c) QPDO_SCHUR_TAU=1e-10 forces second sweeps (one fp32 sweep cannot reach 1e-10 on the fp64 residual: the rounded matrix is 6e-8 away);
QPDO_INNER_REFINE_MAXSWEEP=1 with that tau forces the fallback to the fp64 CG.  (d) Fold on / off and repeated runs: bit for bit."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import pcg_ref as R
from helpers import ITERATE_RTOL_PCG, close_vec
from oracle import binding as ob
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

INFO_KEYS = ("status_val", "iterations", "oterations")
ENV_KEYS = ("QPDO_PCG_INNER_REFINE", "QPDO_PCG_INNER_F32", "QPDO_INNER_REFINE_MAXSWEEP", "QPDO_INNER_REFINE_THETA", "QPDO_SCHUR_TAU",
            "QPDO_INNER_FOLD", "QPDO_SLAB_NT", "QPDO_IDX16", "QPDO_SLAB_OVERLAP")


def _slab_env(monkeypatch, **env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    monkeypatch.setenv("QPDO_SPMV", "slab")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- (a) the products ---------------------------------------------------------------------------------------------------------------
def _matrix(rng, m, n, long_rows=(), long_cols=(), empty_rows=(), empty_cols=()):
    """three entries per row; rows / columns with many more (more than one trip of a lane group inside one slab); empty rows / columns"""
    A = sp.random(m, n, density=3.0 / n, random_state=rng, format="lil", data_rvs=rng.standard_normal)
    for r, cnt in long_rows:
        A[r, rng.choice(n, cnt, replace=False)] = rng.standard_normal(cnt)
    for c, cnt in long_cols:
        A[rng.choice(m, cnt, replace=False), c] = rng.standard_normal(cnt)
    for r in empty_rows:
        A[r, :] = 0
    for c in empty_cols:
        A[:, c] = 0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def _ref_product(M, x):
    """(M32 x, |M32| |x|, M x) from a downloaded compact matrix, in longdouble; M32 = the values rounded to float32"""
    rp, ci, val = M["rp"].astype(np.int64), M["ci"], M["val"]
    row_of = np.repeat(np.arange(M["nrows"]), np.diff(rp))
    xl = x.astype(np.longdouble)[ci]
    v32 = val.astype(np.float32).astype(np.longdouble)
    y32, ab, y64 = (np.zeros(M["nrows"], np.longdouble) for _ in range(3))
    np.add.at(y32, row_of, v32 * xl)
    np.add.at(ab, row_of, np.abs(v32 * xl))
    np.add.at(y64, row_of, val.astype(np.longdouble) * xl)
    return y32, ab, y64


SHAPES = {
    # name: n, m, k, slabs of A_c, slabs of A_c', rows per workgroup of A_c
    "one_slab_20_rows": (6000, 6000, 5000, 1, 1, 20),
    "two_slabs": (30000, 30000, 24000, 2, 2, 94),
    "six_slabs": (110000, 120000, 85000, 6, 5, 333),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fp32_stream_products_against_rounded_numpy(shape, gpu_required, monkeypatch):
    n, m, k, slabs_r, slabs_t, rows_wg = SHAPES[shape]
    _slab_env(monkeypatch)
    rng = np.random.default_rng(n + 3 * m)
    # weighted rows: the first k.  Long rows / columns among them: 300 and 700 entries (one slab holds more than 256 of them in the
    # one-slab shape: a second trip; a ragged one, 700 = 2 * 256 + 188); empty rows 7 and k - 1, empty columns 11 and n - 1
    A = _matrix(rng, m, n, long_rows=((3, 300), (k // 2, 700)), long_cols=((5, 300), (n // 2, 700)), empty_rows=(7, k - 1), empty_cols=(11, n - 1))
    Qf = R.dominant_Q(rng, n)
    dw = np.zeros(m)
    dw[:k] = 0.1 + rng.random(k)
    ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    try:
        v = rng.standard_normal(n)
        for name, nslabs in (("Arc", slabs_r), ("Atc", slabs_t)):
            y, kk = ws.pcg_f32_product(dw, name, v)
            assert kk == k
            M = ws.download_compact_matrix(name)
            assert M["use_slab"] == 1 and M["has_ci16"] == 1 and M["nslabs"] == nslabs, (name, M["nslabs"])
            if name == "Arc":
                assert (k + 255) // 256 == rows_wg
            seglen = np.diff(M["sp"].astype(np.int64), axis=1)
            assert seglen.max() > 256 or nslabs > 1                  # a segment longer than one trip (one-slab shape) ...
            assert (seglen == 0).any() and (np.diff(M["rp"]) == 0).any()      # ... empty segments and empty rows
            y32, ab, y64 = _ref_product(M, v[:M["ncols"]])
            err = np.abs(y.astype(np.longdouble) - y32)
            bound = 1e-13 * ab
            worst = float((err / np.where(ab > 0, bound, 1)).max())
            print("%s %s: k = %d, %d slabs, longest segment %d, worst |y - y32| / (1e-13 |M32||v|) = %.3g" % (shape, name, k, nslabs, seglen.max(), worst))
            assert (err <= bound).all(), (name, worst)
            # the check tells the two value widths apart: the fp64 product is far outside the bound
            assert (np.abs(y64 - y32) > bound).sum() > M["nrows"] // 2
            y2, _ = ws.pcg_f32_product(dw, name, v)
            assert np.array_equal(y2.view(np.uint64), y.view(np.uint64))
        if shape == "one_slab_20_rows":
            assert seglen.max() > 512
    finally:
        ws.delete()


# ---- (b) .. (d) whole solves -----------------------------------------------------------------------------------------------------------
PROBLEMS = {"n800": (62, 800, 1500, 0.03, 0),          # (k < 4096: A_c stays on the plain kernel, the fp64 inner CG runs either way)
            "n6400": (0, 6400, 20000, 0.003, 0)}       # passes with 4096 <= k <= 5120: both compact matrices on the slab kernel
_cache = {}


def _problem(name):
    if name not in _cache:
        _cache[name] = problems.random_qp(*PROBLEMS[name])
    return _cache[name]


def _solve(name, monkeypatch, **env):
    key = (name,) + tuple(sorted(env.items()))
    _slab_env(monkeypatch, **env)
    if key not in _cache:
        _cache[key] = solver.solve_problem(_problem(name), verbose=0)
    return _cache[key]


def _assert_same_outcome(r, ref):
    for k in INFO_KEYS:
        assert r["info"][k] == ref["info"][k], k
    assert [t["n_active"] for t in r["trace"]] == [t["n_active"] for t in ref["trace"]]
    assert close_vec(r["x"], ref["x"], ITERATE_RTOL_PCG), np.abs(r["x"] - ref["x"]).max()
    assert close_vec(r["y"], ref["y"], ITERATE_RTOL_PCG), np.abs(r["y"] - ref["y"]).max()


def _assert_accepted(st):
    assert st["schur_passes"] > 0 and st["inner_solves"] > 0
    assert 0.0 <= st["inner_refine_max_res_over_tol"] <= 1.0, st["inner_refine_max_res_over_tol"]


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_refined_solve_matches_fp64_inner_cg_and_oracle(name, gpu_required, monkeypatch):
    r1 = _solve(name, monkeypatch)
    r0 = _solve(name, monkeypatch, QPDO_PCG_INNER_REFINE="0")
    st = r1["stats"]
    print(name, {k: st[k] for k in st if k.startswith("inner_")}, "fp64:", {k: r0["stats"][k] for k in ("inner_solves", "inner_steps")})
    _assert_accepted(st)
    assert st["inner_refine_fallbacks"] == 0
    assert r0["stats"]["inner_refine_sweeps"] == 0 and r0["stats"]["inner_refine_fp64_applies"] == 0
    if name == "n6400":
        assert st["inner_refine_sweeps"] >= 1 and st["inner_refine_fp64_applies"] == st["inner_refine_sweeps"]
        assert st["inner_refine_max_res_over_tol"] > 0.0
    _assert_same_outcome(r1, r0)
    if name == "n6400":     # the oracle's solve of this instance (default settings; 50 s on the CPU), recorded once: x, y and the three
        # integers of ob.OracleSolver(problems.random_qp(0, 6400, 20000, 0.003, 0), ob.default_settings()).solve(), np.savez_compressed
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_random_qp_0_6400_20000.npz"))
        ro = dict(info={k: int(z[k]) for k in INFO_KEYS}, x=z["x"], y=z["y"])
    else:
        o = ob.OracleSolver(_problem(name), ob.default_settings())
        ro = o.solve()
        o.close()
    for k in INFO_KEYS:
        assert r1["info"][k] == ro["info"][k], k
    assert close_vec(r1["x"], ro["x"], ITERATE_RTOL_PCG) and close_vec(r1["y"], ro["y"], ITERATE_RTOL_PCG)


def _refined_solves(st):
    """inner solves that went through the refinement = those on passes where both compact matrices take the slab kernel; every one of
    them has at least one sweep unless its first sweep failed (a fallback)"""
    return st["inner_refine_sweeps"] + st["inner_refine_fallbacks"]


def test_tight_tau_forces_second_sweeps(gpu_required, monkeypatch):
    r1 = _solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10")
    r0 = _solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10", QPDO_PCG_INNER_REFINE="0")
    st = r1["stats"]
    print({k: st[k] for k in st if k.startswith("inner_")})
    _assert_accepted(st)
    assert st["inner_refine_sweeps"] > st["inner_solves"]
    assert st["inner_refine_fallbacks"] == 0
    _assert_same_outcome(r1, r0)


def test_sweep_cap_falls_back_to_the_fp64_cg(gpu_required, monkeypatch):
    r1 = _solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10", QPDO_INNER_REFINE_MAXSWEEP="1")
    r0 = _solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10", QPDO_PCG_INNER_REFINE="0")
    st = r1["stats"]
    print({k: st[k] for k in st if k.startswith("inner_")})
    assert st["inner_refine_fallbacks"] > 0
    assert 0.0 <= st["inner_refine_max_res_over_tol"] <= 1.0
    _assert_same_outcome(r1, r0)


def test_fold_on_and_off_and_repeats_are_bitwise(gpu_required, monkeypatch):
    a = _solve("n6400", monkeypatch)
    b = _solve("n6400", monkeypatch, QPDO_INNER_FOLD="0")
    _slab_env(monkeypatch)
    c = solver.solve_problem(_problem("n6400"), verbose=0)                  # (not from the cache: a second run)
    assert a["stats"]["inner_refine_sweeps"] > 0
    for r in (b, c):
        for k in INFO_KEYS + ("objective", "res_prim_norm", "res_dual_norm"):
            assert r["info"][k] == a["info"][k], k
        for k in ("lin_iters", "inner_steps", "inner_solves", "inner_refine_sweeps", "inner_refine_fallbacks", "inner_refine_max_res_over_tol"):
            assert r["stats"][k] == a["stats"][k], k
        assert np.array_equal(r["x"], a["x"]) and np.array_equal(r["y"], a["y"])
