"""The slab SpMV with the next slab's first loads issued before its barriers (the default) against the old schedule
(QPDO_SLAB_OVERLAP=0), bit for bit: only the time at which a load is issued moves, never a row's arithmetic."""
import numpy as np
import pytest
import scipy.sparse as sp

from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu


def _matrix_a(seed, m, n):
    """random rows (~12 entries), plus rows whose segments are longer than one trip of a lane group (> 256 entries in one
    slab), rows with entries in the first slab only (empty segments in every other slab) and empty rows"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    per = 12
    rows.append(np.repeat(np.arange(m), per)); cols.append(rng.integers(0, n, m * per))
    for r in range(0, min(m, 40), 3):                      # long segments: 300 .. 2000 consecutive-ish columns
        c = np.unique(rng.integers(0, min(n, 2000 + 37 * r), 600 + 40 * r))
        rows.append(np.full(c.size, r)); cols.append(c)
    for r in range(41, min(m, 60)):                        # first-slab-only rows
        c = np.unique(rng.integers(0, min(n, 500), 30))
        rows.append(np.full(c.size, r)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    keep = ~np.isin(rows, np.arange(61, min(m, 70)))       # empty rows
    vals = rng.standard_normal(keep.sum())
    A = sp.csc_matrix((vals, (rows[keep], cols[keep])), shape=(m, n))
    A.sum_duplicates()
    return A


def _problem(seed, n, m):
    rng = np.random.default_rng(seed + 1)
    A = _matrix_a(seed, m, n)
    i, j = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    lo = i > j
    L = sp.csc_matrix((0.1 * rng.standard_normal(lo.sum()), (i[lo], j[lo])), shape=(n, n))
    Q = (L + sp.diags(1.0 + rng.random(n))).tocsc()        # lower triangle (Qstype -1)
    Q.sum_duplicates()
    return dict(n=n, m=m, Q=Q, A=A, q=rng.standard_normal(n), l=-1.0 - rng.random(m), u=1.0 + rng.random(m))


def _products(p, monkeypatch, overlap, vecs):
    monkeypatch.setenv("QPDO_SLAB_OVERLAP", overlap)
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
    out = [s.spmv(which, v) for which, v in vecs]
    s.delete()
    return out


# (n, m): A with 1 slab and fewer rows per workgroup than lane groups; A and Q with 2 slabs; A and Q with 6 slabs
@pytest.mark.parametrize("idx16", ["1", "0"])
@pytest.mark.parametrize("shape", [(3000, 5000), (30000, 6000), (110000, 20000)])
def test_slab_products_match_old_schedule_bitwise(shape, idx16, gpu_required, monkeypatch):
    monkeypatch.setenv("QPDO_SPMV", "slab")
    monkeypatch.setenv("QPDO_IDX16", idx16)
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    n, m = shape
    p = _problem(7 + n, n, m)
    rng = np.random.default_rng(3)
    vecs = [(0, rng.standard_normal(n)), (1, rng.standard_normal(m)), (2, rng.standard_normal(n))]
    old = _products(p, monkeypatch, "0", vecs)
    new = _products(p, monkeypatch, "1", vecs)
    for which, (a, b) in enumerate(zip(old, new)):
        assert np.array_equal(a, b), (which, np.abs(a - b).max())
    ref = [p["A"] @ vecs[0][1], p["A"].T @ vecs[1][1]]
    for a, r in zip(new[:2], ref):
        assert np.allclose(a, r, rtol=1e-12, atol=1e-12)


def test_schur_mode_compact_products_match_old_schedule_bitwise(gpu_required, monkeypatch):
    """the Schur-complement mode of the PCG with the slab kernels: the compact A_c / A_c' products of its inner CG (k >= 4096
    active rows take the slab kernel) and the outer products; the whole solve must not move by a bit"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    monkeypatch.setenv("QPDO_SPMV", "slab")
    p = problems.random_qp(8200, 3000, 16000, 0.004, 0)
    res = []
    for overlap in ("0", "1"):
        monkeypatch.setenv("QPDO_SLAB_OVERLAP", overlap)
        res.append(solver.solve_problem(p, verbose=0))
    r0, r1 = res
    assert r0["stats"]["schur_passes"] > 0
    for k in ("status_val", "iterations", "oterations", "objective", "res_prim_norm", "res_dual_norm"):
        assert r0["info"][k] == r1["info"][k], k
    assert r0["stats"]["lin_iters"] == r1["stats"]["lin_iters"]
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["y"], r1["y"])
