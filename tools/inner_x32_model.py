"""CPU model of the Schur mode's fp32 inner sweep with fp32 OPERAND vectors (numpy, no GPU).

The single-reduction (Chronopoulos-Gear) Jacobi-PCG of pcg_kernels.inc on S' = D^-1 + A Dq^-1 A', recurrences as cgcg_scalars / cgcg_elem:
    tn = A32' u;  t = tn / Dq;  w = u / d + A32 t;  gamma = (r, u);  delta = sum u^2 / d + sum tn t
    beta = gamma / gamma_old;  alpha = gamma / (delta - beta gamma / alpha_old)
    p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  u = r / diag
A32 = A rounded to float32 (what the sweep streams today).  Variant "x64": u and t enter the products as they are.  Variant "x32": u and t
are rounded to float32 where they enter a product (the pair-wide product stages fp32 copies); everything else -- the u / d term, delta's
two sums (formed from the product's own tn, t), the recurrences, the stopping test -- stays fp64.  Each sweep stops on the recursive
residual at theta tau ||b||; reported: its iterations and the TRUE residual ||b - S' x|| / (tau ||b||) with the unrounded A, which is what
schur_inner_solve accepts on (<= 1: accepted after this one sweep).

usage: inner_x32_model.py            (prints the table; profiles/inner_x32_model.txt is its output)"""
import numpy as np
import scipy.sparse as sp

f32 = lambda v: v.astype(np.float32).astype(np.float64)


def sweep(A, A32, d, dq, diag, b, tau, theta, x32):
    AT32 = A32.T.tocsr()
    k = len(b)
    x, r, p, s = np.zeros(k), b.copy(), np.zeros(k), np.zeros(k)
    u = r / diag
    gam_old = alp_old = 0.0
    bnorm = np.sqrt(r @ r)
    for j in range(4000):
        tn = AT32 @ (f32(u) if x32 else u)
        t = tn / dq
        w = u / d + A32 @ (f32(t) if x32 else t)
        gam, rr, delta = r @ u, r @ r, (u * u / d).sum() + tn @ t
        if np.sqrt(rr) <= theta * tau * bnorm:
            break
        beta = 0.0 if j == 0 else gam / gam_old
        alpha = gam / delta if j == 0 else gam / (delta - beta * gam / alp_old)
        gam_old, alp_old = gam, alpha
        p = u + beta * p
        s = w + beta * s
        x += alpha * p
        r -= alpha * s
        u = r / diag
    true = np.linalg.norm(b - (x / d + A @ ((A.T @ x) / dq))) / bnorm
    return j, np.sqrt(rr) / bnorm / tau, true / tau


def case(n, k, dens, dlo, dhi, tau, theta, seed=0):
    rng = np.random.default_rng(seed)
    A = sp.random(k, n, density=dens, random_state=1, data_rvs=lambda cnt: rng.standard_normal(cnt)).tocsr()
    d = 10 ** rng.uniform(dlo, dhi, k)
    dq = 1e-1 + rng.uniform(0, 1, n)
    A32 = A.astype(np.float32).astype(np.float64)
    diag = 1 / d + np.asarray(A.multiply(A).dot(1 / dq)).ravel()
    b = rng.standard_normal(k)
    return [sweep(A, A32, d, dq, diag, b, tau, theta, x32) for x32 in (False, True)]


if __name__ == "__main__":
    print("Chronopoulos-Gear Jacobi-PCG on S' = D^-1 + A Dq^-1 A', A at 1 % fill rounded to fp32, d over six decades")
    print("%-34s %-6s | %-24s | %-24s" % ("n, k, log10 d, tau", "theta", "x64: it, rec/tau, TRUE/tau", "x32: it, rec/tau, TRUE/tau"))
    for theta in (0.8, 0.65):
        for n, k, dlo, dhi, tau in ((10000, 6600, 0, 6, 3e-6), (20000, 13000, -2, 4, 3e-6), (10000, 6600, 2, 8, 3e-8), (20000, 13000, 0, 6, 3e-8)):
            a, b = case(n, k, 0.01, dlo, dhi, tau, theta)
            print("%-34s %-6g | %4d  %.3f  %8.3f      | %4d  %.3f  %8.3f" % ("%d, %d, [%g, %g], %g" % (n, k, dlo, dhi, tau), theta, *a, *b), flush=True)
