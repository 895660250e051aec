"""The coarse sweeps of the Schur mode's refined inner solve (QPDO_INNER_H16, the default): the first sweeps stream HALF-PRECISION copies of
the compact matrix values -- (half)(float)(a 2^e), one power of two per workspace with max |a_ij| 2^e in [2^14, 2^15) -- through the
pair-wide instance k_spmv_slab<_Float16, float>, which undoes the scale on the finished row sums; every sweep is still followed by the
residual of the fp64 matrices, on which alone a solve is accepted.

(a) The instance on its own (qpdo_amd_pcg_probe modes 36 / 37) on the three shapes of test_gpu_inner_refine.SHAPES (1 slab, 2 slabs, 6 / 5
slabs) and on the n6400 problem under QPDO_SLAB_MAX_W=1280.  Reference: numpy in longdouble with the values rounded as the image holds
them and x rounded to float32.  An 11-bit value times a 24-bit operand is exact in double and the scale is a power of two, so the only
rounding is that of the fp64 row sum: |y - y_ref|_i <= (len_i + 2) 2^-53 (|M16| |x32|)_i.  The longest rows have 1300 entries: with a lane
group's trip of 256 entries five whole trips and a ragged sixth, with one of 512 two and a ragged third.  The same product with the
float32 values lies outside the bound on more than half the rows; a second launch gives the same bits.
(b) The image: the downloaded half-precision values are numpy's rounding bit for bit; a matrix with entries from 1e-7 to 3e5 (beyond
half's 65504 without the scale) gives finite products within the bound of (a); the exponent puts the maximum into [2^14, 2^15).
(c) Whole solves of the n6400 problem, plain and under QPDO_SLAB_MAX_W=1280: the default against QPDO_INNER_H16=0 and the oracle's
record; no fallback; accepted within tau; fold on / off and a repeat bit for bit; QPDO_SCHUR_TAU=1e-10 without a fallback."""
import os

import numpy as np
import pytest

import pcg_ref as R
import test_gpu_inner_refine as T
from helpers import ITERATE_RTOL_PCG, close_vec
from qpdo_amd import solver

pytestmark = pytest.mark.gpu

H16_ENV = ("QPDO_INNER_H16", "QPDO_INNER_H16_ETA", "QPDO_INNER_H16_MAXSWEEP", "QPDO_INNER_X32", "QPDO_SLAB_MAX_W")
_probe_cache = {}


def _env(monkeypatch, **env):
    for k in H16_ENV:
        monkeypatch.delenv(k, raising=False)
    T._slab_env(monkeypatch, **env)


def _round_h16(val, e):
    """the half-precision image of val: (half)(float)(val 2^e), numpy's conversions round to nearest even and keep subnormals"""
    return np.ldexp(val, e).astype(np.float32).astype(np.float16)


def _ref(M, x, e):
    """(2^-e M16 x32, 2^-e |M16| |x32|, M32 x32, row lengths) from a downloaded compact matrix, in longdouble"""
    rp, ci = M["rp"].astype(np.int64), M["ci"]
    row_of = np.repeat(np.arange(M["nrows"]), np.diff(rp))
    v16 = np.ldexp(_round_h16(M["val"], e).astype(np.longdouble), -e)
    v32 = M["val"].astype(np.float32).astype(np.longdouble)
    x32 = x.astype(np.float32).astype(np.longdouble)[ci]
    y, ab, y32 = (np.zeros(M["nrows"], np.longdouble) for _ in range(3))
    np.add.at(y, row_of, v16 * x32)
    np.add.at(ab, row_of, np.abs(v16 * x32))
    np.add.at(y32, row_of, v32 * x32)
    return y, ab, y32, np.diff(rp)


def _probe(ws, dw, v):
    """both half-precision products (twice each), the compact matrices and their images, from one workspace"""
    out = {}
    for name in ("Arc", "Atc"):
        y, kk, e = ws.pcg_h16_product(dw, name, v)
        M = ws.download_compact_matrix(name)
        img = ws.download_compact_image(name)
        y2, _, _ = ws.pcg_h16_product(dw, name, v)
        out[name] = dict(y=y, y2=y2, k=kk, e=e, M=M, img=img)
    return out


def _check_products(tag, res, v, k, amax):
    for name in ("Arc", "Atc"):
        p = res[name]
        M, y, e = p["M"], p["y"], p["e"]
        assert p["k"] == k and M["use_slab"] == 1 and M["has_ci16"] == 1
        assert 2.0 ** 14 <= amax * 2.0 ** e < 2.0 ** 15, (amax, e)           # (b) the exponent
        yr, ab, y32, length = _ref(M, v[:M["ncols"]], e)
        assert np.isfinite(y).all()
        err = np.abs(y.astype(np.longdouble) - yr)
        bound = (length + 2) * np.longdouble(2.0 ** -53) * ab
        worst = float((err / np.where(ab > 0, bound, 1)).max())
        print("%s %s: k = %d, %d slabs, longest row %d, scale 2^%d, worst |y - y_ref| / ((len + 2) 2^-53 |M16||x32|) = %.3g" % (
            tag, name, k, M["nslabs"], length.max(), e, worst))
        assert (err <= bound).all(), (name, worst)
        assert (np.abs(y32 - yr) > bound).sum() > M["nrows"] // 2              # the float32 values are far outside: the widths are told apart
        assert np.array_equal(p["y2"].view(np.uint64), y.view(np.uint64))
        # (b) the image, bit for bit: the half-precision values of the fp64 image's values, in the same places
        img = p["img"]
        assert img["h16_e"] == e and img["vsm16"] is not None
        assert np.array_equal(img["vsm16"].view(np.uint16), _round_h16(img["vsm"], e).view(np.uint16)), name


def _shape_probe(shape):
    if shape not in _probe_cache:
        n, m, k, _, _, _ = T.SHAPES[shape]
        rng = np.random.default_rng(n + 3 * m + 16)
        A = T._matrix(rng, m, n, long_rows=((3, 300), (k // 2, 700), (9, 1300)), long_cols=((5, 300), (n // 2, 700), (13, 1300)),
                      empty_rows=(7, k - 1), empty_cols=(11, n - 1))
        Qf = R.dominant_Q(rng, n)
        dw = np.zeros(m)
        dw[:k] = 0.1 + rng.random(k)
        v = rng.standard_normal(n)
        ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
        try:
            _probe_cache[shape] = (_probe(ws, dw, v), v, float(np.abs(A.data).max()))
        finally:
            ws.delete()
    return _probe_cache[shape]


# ---- (a) the products, (b) the image ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(T.SHAPES))
def test_half_precision_products_and_image_against_rounded_numpy(shape, gpu_required, monkeypatch):
    n, m, k, slabs_r, slabs_t, _ = T.SHAPES[shape]
    _env(monkeypatch)
    res, v, amax = _shape_probe(shape)
    assert res["Arc"]["M"]["nslabs"] == slabs_r and res["Atc"]["M"]["nslabs"] == slabs_t
    _check_products(shape, res, v, k, amax)
    if shape == "one_slab_20_rows":     # one slab: the 1300-entry row and column are single segments, a ragged last trip at either trip length
        for name in ("Arc", "Atc"):
            assert np.diff(res[name]["M"]["rp"]).max() > 1024                  # (of column 13's 1300 entries, those in weighted rows)


def test_half_precision_products_with_capped_slab_width(gpu_required, monkeypatch):
    """QPDO_SLAB_MAX_W=1280 at n = 6400: 5 slabs for A_c (two pairs and a single slab), 4 for A_c' -- the geometry of the capped solves of (c)"""
    _env(monkeypatch, QPDO_SLAB_MAX_W="1280")
    p = T._problem("n6400")
    n, m, k = p["n"], p["m"], 5000
    rng = np.random.default_rng(6416)
    dw = np.zeros(m)
    dw[:k] = 0.1 + rng.random(k)
    v = rng.standard_normal(n)
    ws = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
    try:
        res = _probe(ws, dw, v)
    finally:
        ws.delete()
    assert res["Arc"]["M"]["nslabs"] == 5 and res["Atc"]["M"]["nslabs"] == 4 and res["Arc"]["M"]["W"] == 1280
    _check_products("capped", res, v, k, float(np.abs(p["A"].data).max()))


def test_scale_keeps_a_wide_range_of_entries_finite(gpu_required, monkeypatch):
    """entries from 1e-7 to 3e5, scaling = 0: without the scale the largest are beyond half's 65504; with it (2^-4) they are finite, and
    what falls below half's normal range is kept as subnormals (or zero) at an absolute error that the bound of (a) does not even see"""
    _env(monkeypatch)
    n, m, k, _, _, _ = T.SHAPES["one_slab_20_rows"]
    rng = np.random.default_rng(316)
    A = T._matrix(rng, m, n, long_rows=((3, 300),), long_cols=((5, 300),))
    A.data = np.sign(A.data) * 10.0 ** rng.uniform(-7.0, np.log10(3e5), A.nnz)
    A.data[rng.integers(A.indptr[3], A.indptr[4])] = 3e5                      # (row 3, a weighted row of 300 entries, holds the maximum itself)
    Qf = R.dominant_Q(rng, n)
    dw = np.zeros(m)
    dw[:k] = 0.1 + rng.random(k)
    v = rng.standard_normal(n)
    ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    try:
        res = _probe(ws, dw, v)
    finally:
        ws.delete()
    assert res["Arc"]["e"] == -4 and res["Atc"]["e"] == -4
    for name in ("Arc", "Atc"):
        h = res[name]["img"]["vsm16"]
        assert np.isfinite(h.astype(np.float64)).all() and np.abs(h.astype(np.float64)).max() >= 2.0 ** 14
    _check_products("wide range", res, v, k, 3e5)


# ---- (c) whole solves ----------------------------------------------------------------------------------------------------------------
def _oracle_n6400():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_random_qp_0_6400_20000.npz"))
    return dict(info={k: int(z[k]) for k in T.INFO_KEYS}, x=z["x"], y=z["y"])


@pytest.mark.parametrize("cap", ["plain", "max_w_1280"])
def test_coarse_sweeps_match_the_fp32_sweeps_and_oracle(cap, gpu_required, monkeypatch):
    env = {} if cap == "plain" else {"QPDO_SLAB_MAX_W": "1280"}
    _env(monkeypatch)
    r1 = T._solve("n6400", monkeypatch, **env)
    r0 = T._solve("n6400", monkeypatch, QPDO_INNER_H16="0", **env)
    st, st0 = r1["stats"], r0["stats"]
    print(cap, {k: st[k] for k in st if k.startswith("inner_")}, "h16 off:", {k: st0[k] for k in st0 if k.startswith("inner_")})
    for r in (r1, r0):
        T._assert_accepted(r["stats"])
        assert r["stats"]["inner_refine_fallbacks"] == 0 and r["stats"]["inner_refine_sweeps"] >= 1
        assert r["stats"]["inner_refine_fp64_applies"] == r["stats"]["inner_refine_sweeps"]
        assert r["stats"]["inner_refine_max_res_over_tol"] <= 1.0
    assert 0 < st["inner_h16_steps"] <= st["inner_x32_steps"] <= st["inner_steps"]
    assert 0 < st["inner_h16_sweeps"] <= st["inner_refine_sweeps"]
    # the switch off: no coarse step, every refined step a pair-wide fp32 one, as before the coarse sweeps existed
    assert st0["inner_h16_steps"] == 0 and st0["inner_h16_sweeps"] == 0 and 0 < st0["inner_x32_steps"] <= st0["inner_steps"]
    # ... and the same solve as with the images present but no coarse sweep allowed: the same counters, the same bits
    rz = T._solve("n6400", monkeypatch, QPDO_INNER_H16_MAXSWEEP="0", **env)
    for k in ("lin_iters", "inner_solves", "inner_steps", "inner_x32_steps", "inner_h16_steps", "inner_h16_sweeps", "inner_refine_sweeps",
              "inner_refine_fp64_applies", "inner_refine_fallbacks", "inner_refine_max_res_over_tol"):
        assert rz["stats"][k] == st0[k], k
    assert np.array_equal(rz["x"], r0["x"]) and np.array_equal(rz["y"], r0["y"])
    T._assert_same_outcome(r1, r0)
    ro = _oracle_n6400()
    for r in (r1, r0):
        for k in T.INFO_KEYS:
            assert r["info"][k] == ro["info"][k], k
        assert close_vec(r["x"], ro["x"], ITERATE_RTOL_PCG) and close_vec(r["y"], ro["y"], ITERATE_RTOL_PCG)


def test_x32_off_switches_the_coarse_sweeps_off(gpu_required, monkeypatch):
    _env(monkeypatch)
    r = T._solve("n6400", monkeypatch, QPDO_INNER_X32="0")
    assert r["stats"]["inner_h16_steps"] == 0 and r["stats"]["inner_h16_sweeps"] == 0 and r["stats"]["inner_x32_steps"] == 0
    assert r["stats"]["inner_refine_sweeps"] >= 1 and r["stats"]["inner_refine_fallbacks"] == 0


def test_single_fp32_solve_mode_carries_no_half_precision_images(gpu_required, monkeypatch):
    """QPDO_PCG_INNER_F32=1 (one fp32 inner solve, no sweeps) cannot run a coarse sweep: no image is allocated or written for it"""
    _env(monkeypatch, QPDO_PCG_INNER_F32="1")
    p = T._problem("n6400")
    rng = np.random.default_rng(6432)
    dw = np.zeros(p["m"])
    dw[:5000] = 0.1 + rng.random(5000)
    v = rng.standard_normal(p["n"])
    ws = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
    try:
        ws.pcg_f32_product(dw, "Arc", v)                       # (the fp32 images are there)
        for name in ("Arc", "Atc"):
            img = ws.download_compact_image(name)
            assert img["vsm16"] is None and img["h16_e"] is None
        with pytest.raises(RuntimeError, match="half-precision"):
            ws.pcg_h16_product(dw, "Arc", v)
    finally:
        ws.delete()


@pytest.mark.parametrize("cap", ["plain", "max_w_1280"])
def test_h16_fold_on_and_off_and_repeats_are_bitwise(cap, gpu_required, monkeypatch):
    env = {} if cap == "plain" else {"QPDO_SLAB_MAX_W": "1280"}
    _env(monkeypatch)
    a = T._solve("n6400", monkeypatch, **env)
    b = T._solve("n6400", monkeypatch, QPDO_INNER_FOLD="0", **env)
    _env(monkeypatch, **env)
    c = solver.solve_problem(T._problem("n6400"), verbose=0)                  # (not from the cache: a second run)
    assert a["stats"]["inner_h16_steps"] > 0
    for r in (b, c):
        for k in T.INFO_KEYS + ("objective", "res_prim_norm", "res_dual_norm"):
            assert r["info"][k] == a["info"][k], k
        for k in ("lin_iters", "inner_steps", "inner_x32_steps", "inner_h16_steps", "inner_h16_sweeps", "inner_solves", "inner_refine_sweeps",
                  "inner_refine_fallbacks", "inner_refine_max_res_over_tol"):
            assert r["stats"][k] == a["stats"][k], k
        assert np.array_equal(r["x"], a["x"]) and np.array_equal(r["y"], a["y"])


def test_tight_tau_is_reached_without_a_fallback(gpu_required, monkeypatch):
    _env(monkeypatch)
    r1 = T._solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10")
    r0 = T._solve("n6400", monkeypatch, QPDO_SCHUR_TAU="1e-10", QPDO_PCG_INNER_REFINE="0")
    st = r1["stats"]
    print({k: st[k] for k in st if k.startswith("inner_")})
    T._assert_accepted(st)
    assert st["inner_refine_fallbacks"] == 0 and st["inner_h16_steps"] > 0
    assert st["inner_refine_sweeps"] > st["inner_h16_sweeps"] > 0              # 1e-10 is beyond three coarse sweeps: fp32 sweeps finish
    T._assert_same_outcome(r1, r0)
