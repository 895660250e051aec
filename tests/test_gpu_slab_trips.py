"""The row trips of the slab SpMV (k_spmv_slab, dev/spmv.inc: row_seg / fma_trip) bit for bit.

(a) Every stream width against a numpy EMULATION OF THE KERNEL'S SUMMATION ORDER, built from the downloaded image (download_compact_image:
seg, the values, the slab-local indices) and the instance's trip shape (solver.slab_trip_shape: EPL, UNR, NSA, TPR -- no constant of the
kernel is written down here).  A lane group of TPR lanes walks a row's segment of a slab (of a slab pair: the two adjacent segments as
one) in trips of EPL UNR TPR entries from the segment's start rounded down to EPL; the entry at offset o from there belongs to trip
o / STEP, load u = (o mod STEP) / (EPL TPR), lane ((o mod STEP) mod (EPL TPR)) / EPL, slot e = o mod EPL, and is added -- value times operand,
both as doubles -- to the lane's partial sum (EPL u + e) mod NSA, trips and loads in ascending order; entry slots outside the segment add
+0.0.  Then t = 0; t += sa[2 i] + sa[2 i + 1] in order, the shuffle tree t[l] += t[l + o] for o = TPR / 2 .. 1, acc[row] += t[0] in slab
(pair) order, and the half-precision instance's power of two.  The emulation ran against the kernel from before the trips were made
branch-free and passed there unchanged: that is its proof.  Instances: fp32 values with the fp64 operand (probe modes 32 / 33), pair-wide
fp32 (34 / 35), pair-wide half precision (36 / 37), and the fp64 instance through the K product of mode 0 with a diagonal Q (Q p is then
exact whatever kernel runs it): K p = (q p + sigma p) + A_c' (d_c (A_c p)), both compact products by the fp64 instance on the same
images.  (The full matrices' images of qpdo_amd_spmv, the entry of test_gpu_slab_overlap, cannot be downloaded, and where a lane starts
depends on the image position of a segment: the K product reaches the same instance on images that can.)
Shapes: a seeded matrix C (4096 x 6400, QPDO_SLAB_MAX_W=1280: five slabs = two pairs and a single one, 16 rows per workgroup; for the
transposed case 4096 x 4096, four slabs, since the narrow products need k <= n) whose row r
has a first pair segment of r mod (2 STEP + EPL + 2) entries -- every length from 0 to 2 STEP + EPL + 1 -- split between the pair's two
slabs at 0, at its end and at every point between, as A (A_c = C) and transposed (A_c' = C); the test asserts from the image that
starts and splits hit every residue mod EPL.  And the three shapes of test_gpu_inner_refine.SHAPES.  Every product runs twice: same bits.
(b) Masked slots: NaN at one column of the operand and Inf at another; rows without an entry there equal the clean product bit for
bit, the others are not finite.
(c) Whole solves of the n6400 problem, plain and under QPDO_SLAB_MAX_W=1280: x, y, the info's integers and every counter of stats()
equal the record tests/golden/slab_trips_n6400.npz, taken with the build before the change (tests/golden/make_slab_trips_golden.py)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_inner_refine as T
from qpdo_amd import solver

pytestmark = pytest.mark.gpu

ENV = ("QPDO_INNER_H16", "QPDO_INNER_H16_ETA", "QPDO_INNER_H16_MAXSWEEP", "QPDO_INNER_X32", "QPDO_SLAB_MAX_W")
# instance: (value bytes, operand bytes)
INSTANCES = {"f32_x64": (4, 8), "f32_x32": (4, 4), "h16_x32": (2, 4), "f64_x64": (8, 8)}
_cache = {}


def _env(monkeypatch, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    T._slab_env(monkeypatch, **env)


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------
def emulate(img, geo, vals, x, shape, pairwide, rscale=1.0):
    """acc[row] of k_spmv_slab for the image img (seg, idx), its values `vals` and the operand x as doubles (already rounded to the
    width the instance reads), in the kernel's order of operations"""
    EPL, UNR, NSA, TPR = shape
    STEP = EPL * UNR * TPR
    seg, idx = img["seg"].astype(np.int64), img["idx"].astype(np.int64)
    nrows, nslabs, W = geo["nrows"], geo["nslabs"], geo["W"]
    acc = np.zeros(nrows)
    for s in range((nslabs + 1) // 2 if pairwide else nslabs):
        if pairwide:
            beg = seg[:, 2 * s, 0]
            mid = beg + seg[:, 2 * s, 1]
            if 2 * s + 1 < nslabs:
                end = mid + seg[:, 2 * s + 1, 1]
                assert (seg[:, 2 * s + 1, 0] == mid).all()      # pair order: the two segments are adjacent
            else:
                end = mid
            c0 = 2 * s * W
        else:
            beg = seg[:, s, 0]
            end = beg + seg[:, s, 1]
            mid, c0 = end, s * W
        rows = np.nonzero(end > beg)[0]           # (an empty segment adds t = +0.0)
        if rows.size == 0:
            continue
        L = (end - beg)[rows]
        rr = np.repeat(np.arange(rows.size), L)
        p = beg[rows][rr] + np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
        o = p - (beg[rows] & ~(EPL - 1))[rr]
        trip, w = o // STEP, o % STEP
        u, lane, e = w // (EPL * TPR), (w % (EPL * TPR)) // EPL, o % EPL
        prod = vals[p] * x[idx[p] + c0 + np.where(p >= mid[rows][rr], W, 0)]
        # the partial sums sa[row, lane, j], each a sum in (trip, load) order from +0.0
        rl, rl_inv = np.unique(rr * TPR + lane, return_inverse=True)
        g = rl_inv * NSA + (EPL * u + e) % NSA
        order = np.lexsort((trip * UNR + u, g))
        gs = g[order]
        first = np.r_[0, np.nonzero(np.diff(gs))[0] + 1]
        rank = np.arange(gs.size) - np.repeat(first, np.diff(np.r_[first, gs.size]))
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.r_[0, np.cumsum(np.bincount(rank))]
        sa = np.zeros(rl.size * NSA)
        for k in range(cuts.size - 1):
            sel = order[by_rank[cuts[k]:cuts[k + 1]]]
            sa[g[sel]] = sa[g[sel]] + prod[sel]       # (one entry per sum and round: no index repeats)
        sa = sa.reshape(rl.size, NSA)
        tl = np.zeros(rl.size)
        for i in range(NSA // 2):
            tl = tl + (sa[:, 2 * i] + sa[:, 2 * i + 1])
        t = np.zeros((rows.size, TPR))
        t[rl // TPR, rl % TPR] = tl
        off = TPR // 2
        while off > 0:
            t[:, :TPR - off] = t[:, :TPR - off] + t[:, off:]
            off //= 2
        acc[rows] = acc[rows] + t[:, 0]
    return acc * rscale


def _values(inst, img):
    if inst == "h16_x32":
        return img["vsm16"].astype(np.float64), 2.0 ** -img["h16_e"]
    if inst == "f64_x64":
        return img["vsm"], 1.0
    return img["vsm"].astype(np.float32).astype(np.float64), 1.0


def _operand(inst, v):
    return v.astype(np.float32).astype(np.float64) if INSTANCES[inst][1] == 4 else v


def _device_product(ws, inst, dw, name, v):
    if inst == "h16_x32":
        return ws.pcg_h16_product(dw, name, v)[0]
    return ws.pcg_f32_product(dw, name, v, x32=(inst == "f32_x32"))[0]


def _emulated_product(inst, img, geo, v):
    vals, rscale = _values(inst, img)
    return emulate(img, geo, vals, _operand(inst, v)[:geo["ncols"]], solver.slab_trip_shape(*INSTANCES[inst]), INSTANCES[inst][1] == 4, rscale)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _run(key, A, q, dw, v, sigma):
    """one workspace: every narrow product of both compact matrices twice, the K product twice, the geometry, the images and d_c"""
    if key in _cache:
        return _cache[key]
    m, n = A.shape
    ws = solver.QPDO().setup(sp.diags(q).tocsc(), np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    try:
        out = {"y": {}, "y2": {}}
        for inst in ("f32_x64", "f32_x32", "h16_x32"):
            for name in ("Arc", "Atc"):
                out["y"][inst, name] = _device_product(ws, inst, dw, name, v)
                out["y2"][inst, name] = _device_product(ws, inst, dw, name, v)
        out["K"], out["K2"] = ws.pcg_K_product(dw, sigma, v)[0], ws.pcg_K_product(dw, sigma, v)[0]
        out["geo"] = {name: ws.download_compact_matrix(name) for name in ("Arc", "Atc")}
        out["img"] = {name: ws.download_compact_image(name) for name in ("Arc", "Atc")}
        out["dc"] = ws.download_compact_vector("dc")
    finally:
        ws.delete()
    _cache[key] = out
    return out


def _check(out, inst, q, v, sigma, k):
    """the instance's products of both compact matrices against the emulation, and the repeat"""
    for name in ("Arc", "Atc"):
        assert out["geo"][name]["use_slab"] == 1 and out["geo"][name]["has_ci16"] == 1 and out["img"][name] is not None, name
    if inst == "f64_x64":
        shape = solver.slab_trip_shape(8, 8)
        s1 = emulate(out["img"]["Arc"], out["geo"]["Arc"], out["img"]["Arc"]["vsm"], v, shape, False)
        s2 = emulate(out["img"]["Atc"], out["geo"]["Atc"], out["img"]["Atc"]["vsm"], out["dc"] * s1, shape, False)
        ref = (q * v + sigma * v) + s2
        bad = np.nonzero(out["K"] != ref)[0]
        print("K product: %d rows, %d differ from the emulation" % (ref.size, bad.size))
        assert bad.size == 0, (bad[:8], out["K"][bad[:8]], ref[bad[:8]])
        assert _same_bits(out["K"], out["K2"])
        return
    for name in ("Arc", "Atc"):
        y = out["y"][inst, name]
        x = v if name == "Arc" else v[:k]
        ref = _emulated_product(inst, out["img"][name], out["geo"][name], np.r_[x, np.zeros(max(0, out["geo"][name]["ncols"] - x.size))])
        bad = np.nonzero(y != ref)[0]
        print("%s %s: %d rows, %d slabs, %d differ from the emulation" % (inst, name, y.size, out["geo"][name]["nslabs"], bad.size))
        assert y.size == ref.size and bad.size == 0, (name, bad[:8], y[bad[:8]], ref[bad[:8]])
        assert _same_bits(y, out["y2"][inst, name]), name


# ---- (a) the seeded matrix: every segment length, start and split ------------------------------------------------------------------------
ROWS, COLS, MAX_W = 4096, 6400, 1280


def _longest_trip():
    """STEP and EPL of the pair-wide instances (the longest segments are built for the larger of them)"""
    shapes = [solver.slab_trip_shape(*INSTANCES[i]) for i in ("f32_x32", "h16_x32")]
    return max(s[0] * s[1] * s[3] for s in shapes), max(s[0] for s in shapes)


def _crafted(cols, W):
    """C, ROWS x cols for slabs of W columns: row r has r mod (2 STEP + EPL + 2) entries in the first slab pair (columns [0, 2 W)), the
    first a_r of them in the first slab: a_r runs through 0, the whole length and every point between (within what a slab holds); a few
    in the second pair and, where there is one, in the single last slab"""
    if ("C", cols) not in _cache:
        STEP, EPL = _longest_trip()
        nlen = 2 * STEP + EPL + 2
        rng = np.random.default_rng(cols + nlen)
        rows, cc = [], []
        for r in range(ROWS):
            L = r % nlen
            lo, hi = max(0, L - W), min(L, W)
            a = (lo, hi, lo + (r // nlen + 3 * r) % (hi - lo + 1))[r % 3] if L else 0
            c = np.r_[np.sort(rng.choice(W, a, replace=False)), W + np.sort(rng.choice(W, L - a, replace=False)),
                      2 * W + np.sort(rng.choice(2 * W, (5 * r) % 23, replace=False)),
                      4 * W + np.sort(rng.choice(cols - 4 * W, (7 * r) % 11, replace=False)) if cols > 4 * W else []].astype(np.int64)
            rows.append(np.full(c.size, r)); cc.append(c)
        rows, cc = np.concatenate(rows), np.concatenate(cc)
        C = sp.csr_matrix((rng.standard_normal(rows.size), (rows, cc)), shape=(ROWS, cols))
        C.sort_indices()
        _cache["C", cols] = C
    return _cache["C", cols]


# orientation: (columns of C, slab width and slab count under the cap).  "rows": A = C, A_c = C, five slabs -- two pairs and a single one;
# "transposed": A = C' with a square C (the narrow products need k <= n), A_c' = C, four slabs
ORIENT = {"rows": (COLS, MAX_W, 5), "transposed": (ROWS, 1024, 4)}


def _crafted_run(orient):
    cols, W, _ = ORIENT[orient]
    assert W % 64 == 0 and (cols + MAX_W - 1) // MAX_W * W >= cols > ((cols + MAX_W - 1) // MAX_W - 1) * W
    C = _crafted(cols, W)
    A = C if orient == "rows" else sp.csr_matrix(C.T)
    m, n = A.shape
    rng = np.random.default_rng(17 + m)
    q, dw, v = 1.0 + rng.random(n), 0.1 + rng.random(m), rng.standard_normal(n)
    return _run(("crafted", orient), A, q, dw, v, 0.375), q, dw, v, A


@pytest.mark.parametrize("inst", sorted(INSTANCES))
@pytest.mark.parametrize("orient", ["rows", "transposed"])
def test_products_match_the_emulated_summation_order(orient, inst, gpu_required, monkeypatch):
    _env(monkeypatch, QPDO_SLAB_MAX_W=str(MAX_W))
    out, q, dw, v, A = _crafted_run(orient)
    name = "Arc" if orient == "rows" else "Atc"          # the compact matrix that is C
    geo, seg = out["geo"][name], out["img"][name]["seg"].astype(np.int64)
    assert geo["nrows"] == ROWS and (geo["ncols"], geo["W"], geo["nslabs"]) == ORIENT[orient]
    assert 16 <= (ROWS + 255) // 256 <= 20
    EPL, UNR, NSA, TPR = solver.slab_trip_shape(*INSTANCES[inst])
    STEP = EPL * UNR * TPR
    # the first pair's segments: every length, every start residue, the split at the start, at the end and at every residue
    beg, mid, end = seg[:, 0, 0], seg[:, 0, 0] + seg[:, 0, 1], seg[:, 0, 0] + seg[:, 0, 1] + seg[:, 1, 1]
    assert set(range(2 * STEP + EPL + 2)) <= set((end - beg).tolist())
    some = end > beg
    assert set((beg[some] % EPL).tolist()) == set(range(EPL)) and set((mid[some] % EPL).tolist()) == set(range(EPL))
    assert (mid[some] == beg[some]).any() and (mid[some] == end[some]).any() and ((mid > beg) & (mid < end)).any()
    _check(out, inst, q, v, 0.375, A.shape[0])


@pytest.mark.parametrize("inst", sorted(INSTANCES))
@pytest.mark.parametrize("shape", sorted(T.SHAPES))
def test_products_match_the_emulation_on_the_refine_shapes(shape, inst, gpu_required, monkeypatch):
    n, m, k, slabs_r, slabs_t, _ = T.SHAPES[shape]
    _env(monkeypatch)
    if ("shape", shape) not in _cache:
        rng = np.random.default_rng(n + 3 * m + 5)
        A = T._matrix(rng, m, n, long_rows=((3, 300), (k // 2, 700), (9, 1300)), long_cols=((5, 300), (n // 2, 700), (13, 1300)),
                      empty_rows=(7, k - 1), empty_cols=(11, n - 1))
        dw = np.zeros(m)
        dw[:k] = 0.1 + rng.random(k)
        _cache["shape", shape, "in"] = (1.0 + rng.random(n), dw, rng.standard_normal(n), A)
    q, dw, v, A = _cache["shape", shape, "in"]
    out = _run(("shape", shape), A, q, dw, v, 0.375)
    assert out["geo"]["Arc"]["nslabs"] == slabs_r and out["geo"]["Atc"]["nslabs"] == slabs_t
    _check(out, inst, q, v, 0.375, k)


# ---- (b) masked slots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", ["f32_x64", "f32_x32", "h16_x32"])
def test_nan_and_inf_reach_only_the_rows_that_touch_their_columns(inst, gpu_required, monkeypatch):
    _env(monkeypatch, QPDO_SLAB_MAX_W=str(MAX_W))
    out, q, dw, v, A = _crafted_run("rows")
    C = _crafted(COLS, MAX_W)
    c_nan, c_inf = 777, 4 * MAX_W + 100                  # first pair (long segments: most masked slots hold its indices); the single last slab
    vb = v.copy()
    vb[c_nan], vb[c_inf] = np.nan, np.inf
    m, n = A.shape
    ws = solver.QPDO().setup(sp.diags(q).tocsc(), np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    try:
        y = _device_product(ws, inst, dw, "Arc", vb)
    finally:
        ws.delete()
    touched = np.asarray((C[:, [c_nan, c_inf]] != 0).sum(axis=1)).ravel() > 0
    assert 0 < touched.sum() < ROWS
    clean = out["y"][inst, "Arc"]
    assert _same_bits(y[~touched], clean[~touched])
    assert not np.isfinite(y[touched]).any()


# ---- (c) whole solves against the record of the build before the change -------------------------------------------------------------------
@pytest.mark.parametrize("cap", ["plain", "max_w_1280"])
def test_whole_solve_reproduces_the_recorded_bits_and_counters(cap, gpu_required, monkeypatch):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slab_trips_n6400.npz"))
    _env(monkeypatch)
    r = T._solve("n6400", monkeypatch, **({} if cap == "plain" else {"QPDO_SLAB_MAX_W": "1280"}))
    for k in T.INFO_KEYS:
        assert r["info"][k] == int(z[cap + "_" + k]), k
    counters = [f[len(cap) + 7:] for f in z.files if f.startswith(cap + "_stats_")]
    assert len(counters) > 30 and "inner_steps" in counters and "inner_h16_steps" in counters
    ctype = dict(solver.Stats._fields_)
    for k in counters:
        want = z[cap + "_stats_" + k].item()
        assert r["stats"][k] == want and (ctype[k] is ctypes.c_long) == isinstance(want, int), (k, r["stats"][k], want)
    assert r["stats"]["inner_h16_steps"] > 0 and r["stats"]["inner_x32_steps"] > 0        # the narrow instances ran
    assert _same_bits(r["x"], z[cap + "_x"]) and _same_bits(r["y"], z[cap + "_y"])
