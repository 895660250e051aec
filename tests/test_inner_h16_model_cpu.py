"""tools/inner_h16_model.py at its smallest case (n = 4000, k = 2640; no GPU): at the default eta and cap of coarse sweeps that the model
picked, with the cap the library ships (one coarse sweep less than the model's pick: tools/inner_h16_model.py) -- the defaults of
QPDO_INNER_H16_ETA and QPDO_INNER_H16_MAXSWEEP -- the refined solve is accepted within the sweep cap at
tau = 3e-6 and at tau = 1e-10, reproduces the sweeps recorded in profiles/inner_h16_model.txt, and needs no more iterations than today's
single-width solve plus a margin.  The margin is read off that file: over its six cases the chosen policy needs at most 7.9 % more
iterations than today's solve (96 against 89 at this very case; 93 against 88 and 128 against 129 at n = 20000; fewer at tau = 1e-10), so
10 % is the cap."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inner_h16_model as M  # noqa: E402

MARGIN = 0.10


def _recorded():
    """{(n, k, tau): {"today": "f89", (cap, eta): "h50 h46"}} from the committed table"""
    out, cur = {}, None
    for line in open(os.path.join(ROOT, "profiles", "inner_h16_model.txt")):
        m = re.match(r"n = (\d+), k = (\d+), tau = (\S+), scale 2\^(-?\d+): today (.*) = \d+ iterations", line)
        if m:
            cur = out.setdefault((int(m.group(1)), int(m.group(2)), float(m.group(3))), {"today": m.group(5), "e": int(m.group(4))})
            continue
        m = re.match(r"\s+cap (\S+)\s+eta (\S+)\s*: ((?:[hf]\d+ ?)+)", line)
        if m and cur is not None:
            cur[(None if m.group(1) == "inf" else int(m.group(1)), float(m.group(2)))] = m.group(3).strip()
    return out


def test_default_policy_is_the_models_choice_and_is_accepted_within_the_cap():
    rec = _recorded()
    last = open(os.path.join(ROOT, "profiles", "inner_h16_model.txt")).read().strip().splitlines()[-2:]
    assert last[0].startswith("default: eta = %g, cap = %d " % (M.MODEL_ETA, M.MODEL_CAP)), last
    assert last[1].startswith("shipped: eta = %g, cap = %d " % (M.DEFAULT_ETA, M.DEFAULT_CAP)), last
    assert M.DEFAULT_ETA == M.MODEL_ETA and M.DEFAULT_CAP <= M.MODEL_CAP
    n, k, _ = M.SMALL[0]
    P = M.Problem(n, k)
    assert 2.0 ** 14 <= np.abs(P.A.data).max() * 2.0 ** P.e < 2.0 ** 15
    for case in M.SMALL:
        tau = case[2]
        today, ok0 = P.solve(tau, 0.0, 0)
        sweeps, ok = P.solve(tau, M.DEFAULT_ETA, M.DEFAULT_CAP)
        it0, it1 = sum(s[1] for s in today), sum(s[1] for s in sweeps)
        print("tau = %g: today %s (%d), coarse %s (%d)" % (tau, M.fmt(today, ok0), it0, M.fmt(sweeps, ok), it1))
        assert ok0 and ok and len(sweeps) <= M.MAXSWEEP
        assert sweeps[-1][2] <= 1.0                                     # accepted on the residual of the unrounded matrix
        assert all(kind == "h" for kind, _, _ in sweeps[:M.DEFAULT_CAP]) and all(kind == "f" for kind, _, _ in sweeps[M.DEFAULT_CAP:])
        assert it1 <= (1.0 + MARGIN) * it0, (it1, it0)
        assert M.fmt(today, ok0) == rec[case]["today"] and M.fmt(sweeps, ok) == rec[case][(M.DEFAULT_CAP, M.DEFAULT_ETA)]
        assert rec[case]["e"] == P.e


def test_rounding_of_the_model_is_the_images():
    """(half)(float)(v 2^e) 2^-e: eleven significant bits, subnormals kept, nothing overflows under the scale"""
    v = np.array([3e5, -3e5, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-7, 0.0, -2.5e-3])
    e = M.h16_exponent(np.abs(v).max())
    assert e == -4 and M.h16_exponent(0.0) is None and M.h16_exponent(np.inf) is None and M.h16_exponent(np.nan) is None
    r = M.round_h16(v, e)
    assert np.isfinite(r).all() and r[0] == -r[1] and abs(r[0] - 3e5) <= 3e5 * 2.0 ** -11
    # entries 2^e a < 2^-14 are subnormals of half: absolute error <= 2^-25 2^-e, i.e. 2^-25 ... 2^-24 of the largest entry's magnitude class
    assert np.all(np.abs(r - v) <= np.maximum(np.abs(v) * 2.0 ** -11, 2.0 ** -25 * 2.0 ** -e))
    assert r[5] != 0.0 or 1e-7 * 2.0 ** e < 2.0 ** -25                  # 1e-7 2^-4 = 6e-9 is below half of the smallest subnormal: zero
