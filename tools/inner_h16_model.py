"""CPU model of the Schur mode's refined inner solve with COARSE sweeps on a half-precision copy of the matrix (numpy / scipy, no GPU).

The solve of schur_inner_solve (host_pcg.inc): s = 0, rho = b; per sweep the single-reduction Jacobi-PCG of tools/inner_x32_model.py runs
on a ROUNDED copy of A with right-hand side rho and operands rounded to float32 where they enter a product, s += e, rho = b - S' s with
the unrounded A, accepted when ||rho|| <= tau ||b||.  S' = D^-1 + A Dq^-1 A'.
  "f" sweep: A rounded to float32, stops at a recursive residual of theta tau ||b||                       (today's sweep)
  "h" sweep: A rounded as DevCsr::vsm16 holds it -- (half)(float)(a 2^e), one power of two 2^e per matrix with max|a| 2^e in [2^14, 2^15),
             subnormals kept, the row sums multiplied by 2^-e -- stops at max(theta tau ||b||, eta ||rho||)
Policy: sweep i is an "h" sweep while i < cap (QPDO_INNER_H16_MAXSWEEP), an "f" sweep afterwards; at most MAXSWEEP sweeps.
Inputs varied: eta in ETAS, cap in CAPS (None: every sweep coarse).  cap = 0 is today's solve.

Cost of a solve in units of one fp32 iteration (two pair-wide products of 6 B per nonzero): an "h" iteration H_COST (4 B per nonzero at
90 % bytes, 10 % per-row overhead), an "f" iteration 1, every sweep SWEEP_COST (two fp64 products of 10 B per nonzero, slab by slab, and a
host read).  The default (eta, cap) is the cheapest over the tau = 3e-6 and 3e-8 cases among those that are accepted within MAXSWEEP at
every case, tau = 1e-10 included.

usage: inner_h16_model.py [small]      (prints the tables; profiles/inner_h16_model.txt is the output without arguments)"""
import sys

import numpy as np
import scipy.sparse as sp

f32 = lambda v: v.astype(np.float32).astype(np.float64)
ETAS = (5e-4, 1e-3, 2e-3, 5e-3, 1e-2)
CAPS = (2, 3, None)
THETA, MAXSWEEP = 0.8, 6
H_COST, SWEEP_COST = 0.72, 1.5
MODEL_ETA, MODEL_CAP = 1e-3, 3              # what pick_default chose on the committed table
# What the library ships (QPDO_INNER_H16_ETA, QPDO_INNER_H16_MAXSWEEP): the model's eta, and ONE coarse sweep less than its pick.  On the
# complete C4 solve two coarse sweeps reach tau in all but 26 of 401 inner solves, so the cap costs nothing there (docs/LAB_NOTES.md); a
# third sweep, where one is needed, is an fp32 sweep and lands at theta tau like every sweep before the coarse ones existed.  The reason
# for the smaller cap is one assertion of the suite on the complete C4 record, whose margin is a draw from a wide spread and fragile:
# docs/LAB_NOTES.md, "16-bit matrix stream".
DEFAULT_ETA, DEFAULT_CAP = 1e-3, 2
# n, k, tau; d = 10^U[0, 6], A at 1 % fill
CASES = ((20000, 13000, 3e-6), (20000, 13000, 3e-8), (10000, 6600, 1e-10), (20000, 16000, 1e-10))
SMALL = ((4000, 2640, 3e-6), (4000, 2640, 1e-10))


def h16_exponent(amax):
    """e with amax 2^e in [2^14, 2^15); None where amax is 0, inf or NaN (the 16-bit path stays off)"""
    if not (amax > 0.0 and np.isfinite(amax)):
        return None
    return 14 - int(np.floor(np.log2(amax)))


def round_h16(val, e):
    """the values of vsm16 as doubles, scale undone: (half)(float)(v 2^e) 2^-e, each conversion round-to-nearest-even"""
    return np.ldexp(np.ldexp(val, e).astype(np.float32).astype(np.float16).astype(np.float64), -e)


def cg(Aw, ATw, d, dq, diag, b, tol):
    """Chronopoulos-Gear Jacobi-PCG (pcg_kernels.inc: cgcg_scalars / cgcg_elem), operands rounded to fp32 where they enter a product;
    stops when the recursive residual is <= tol ||b||"""
    k = len(b)
    x, r, p, s = np.zeros(k), b.copy(), np.zeros(k), np.zeros(k)
    u = r / diag
    gam_old = alp_old = 0.0
    bnorm = np.sqrt(r @ r)
    for j in range(4000):
        tn = ATw @ f32(u)
        t = tn / dq
        w = u / d + Aw @ f32(t)
        gam, rr, delta = r @ u, r @ r, (u * u / d).sum() + tn @ t
        if np.sqrt(rr) <= tol * bnorm:
            break
        beta = 0.0 if j == 0 else gam / gam_old
        alpha = gam / delta if j == 0 else gam / (delta - beta * gam / alp_old)
        gam_old, alp_old = gam, alpha
        p = u + beta * p
        s = w + beta * s
        x += alpha * p
        r -= alpha * s
        u = r / diag
    return x, j


class Problem:
    def __init__(self, n, k, dens=0.01, seed=0):
        rng = np.random.default_rng(seed)
        A = sp.random(k, n, density=dens, random_state=1, data_rvs=lambda cnt: rng.standard_normal(cnt)).tocsr()
        self.A, self.AT = A, A.T.tocsr()
        self.d = 10 ** rng.uniform(0, 6, k)
        self.dq = 1e-1 + rng.uniform(0, 1, n)
        self.diag = 1 / self.d + np.asarray(A.multiply(A).dot(1 / self.dq)).ravel()
        self.b = rng.standard_normal(k)
        self.e = h16_exponent(np.abs(A.data).max())
        self.W = {}
        for name, data in (("f", f32(A.data)), ("h", round_h16(A.data, self.e))):
            M = sp.csr_matrix((data, A.indices, A.indptr), shape=A.shape)
            self.W[name] = (M, M.T.tocsr())

    def solve(self, tau, eta, cap, theta=THETA, maxsweep=MAXSWEEP):
        """the sweeps as [(kind, iterations, ||rho|| / (tau ||b||) after it)], accepted or not"""
        b, bn = self.b, np.linalg.norm(self.b)
        s, rho, rn = np.zeros_like(b), b.copy(), bn
        sweeps = []
        for i in range(maxsweep):
            coarse = cap is None or i < cap
            tol = theta * tau * bn / rn
            if coarse:
                tol = max(tol, eta)
            e, it = cg(*self.W["h" if coarse else "f"], self.d, self.dq, self.diag, rho, tol)
            s += e
            rho = b - (s / self.d + self.A @ ((self.AT @ s) / self.dq))
            rn = np.linalg.norm(rho)
            sweeps.append(("h" if coarse else "f", it, rn / (tau * bn)))
            if rn <= tau * bn:
                return sweeps, True
        return sweeps, False


def cost(sweeps):
    return sum((H_COST if kind == "h" else 1.0) * it + SWEEP_COST for kind, it, _ in sweeps)


def fmt(sweeps, ok):
    return " ".join("%s%d" % (kind, it) for kind, it, _ in sweeps) + ("" if ok else " NOT ACCEPTED")


def table(cases, out=print):
    """prints the table; returns {(case, eta, cap): (sweeps, accepted)} with (case, None, 0) = today's solve"""
    res, probs = {}, {}
    for case in cases:
        n, k, tau = case
        P = probs.setdefault((n, k), Problem(n, k))
        res[(case, None, 0)] = P.solve(tau, 0.0, 0)
        sw, ok = res[(case, None, 0)]
        out("n = %d, k = %d, tau = %g, scale 2^%d: today %s = %d iterations, cost %.1f" % (n, k, tau, P.e, fmt(sw, ok), sum(s[1] for s in sw), cost(sw)))
        for cap in CAPS:
            for eta in ETAS:
                res[(case, eta, cap)] = P.solve(tau, eta, cap)
                sw, ok = res[(case, eta, cap)]
                out("    cap %-4s eta %-6g: %-36s %4d iterations, cost %6.1f, decades per h sweep %s" % (
                    "inf" if cap is None else cap, eta, fmt(sw, ok), sum(s[1] for s in sw), cost(sw),
                    " ".join("%.2f" % d for d in h_decades(sw, tau))))
    return res


def h_decades(sweeps, tau):
    """log10 reduction of the true residual over each coarse sweep that did not stop on theta tau"""
    out, prev = [], 1.0 / tau
    for kind, _, ratio in sweeps:
        if kind == "h" and ratio > 1.0:
            out.append(np.log10(prev / ratio))
        prev = ratio
    return out


def pick_default(res, cases):
    """(eta, cap) of least summed cost over the cases with tau >= 1e-8, among those accepted at every case; a tie goes to the smaller cap
    (fewer coarse sweeps in front of the fp32 sweeps when tau is tight: three fp32 sweeps stay in hand under MAXSWEEP = 6)"""
    best = None
    for cap in CAPS:
        for eta in ETAS:
            if not all(res[(c, eta, cap)][1] for c in cases):
                continue
            loose = [c for c in cases if c[2] >= 1e-8] or list(cases)
            total = sum(cost(res[(c, eta, cap)][0]) for c in loose)
            if best is None or total < best[0] - 1e-9:
                best = (total, eta, cap)
    return best


if __name__ == "__main__":
    cases = SMALL if len(sys.argv) > 1 and sys.argv[1] == "small" else SMALL + CASES
    print("Refined inner solve, coarse (h) sweeps on A rounded to fp16 with one power-of-two scale, then fp32 (f) sweeps; A at 1 % fill, d over six decades,")
    print("theta = %g, at most %d sweeps, operands rounded to fp32.  cost: h iteration %.2f, f iteration 1, sweep %.1f" % (THETA, MAXSWEEP, H_COST, SWEEP_COST))
    res = table(cases, lambda s: print(s, flush=True))
    total, eta, cap = pick_default(res, cases)
    today = sum(cost(res[(c, None, 0)][0]) for c in cases if c[2] >= 1e-8)
    print("default: eta = %g, cap = %s (cost over the tau >= 1e-8 cases %.1f, today's %.1f)" % (eta, "inf" if cap is None else cap, total, today))
    shipped = sum(cost(res[(c, DEFAULT_ETA, DEFAULT_CAP)][0]) for c in cases if c[2] >= 1e-8)
    print("shipped: eta = %g, cap = %d (cost over the same cases %.1f)" % (DEFAULT_ETA, DEFAULT_CAP, shipped))
