"""A/B timing of builds of libqpdo_amd.so on one box: the C4 cold-start solve, alternating processes.
usage: ab_c4.py libA.so libB.so [more sides ...] [reps]
A side is a library, or VAR=VALUE,VAR=VALUE@library: that build with those environment switches (e.g. QPDO_INNER_FOLD=0@libqpdo_amd.so).
Per solve: wall time, passes, status, linear-solver iterations, inner solves of the Schur mode and, for the refined inner solve
(QPDO_PCG_INNER_REFINE), its sweeps, fallbacks and the largest accepted ||rho|| / (tau ||b||); the inner CG's steps and how many of them
staged fp32 operand vectors (QPDO_INNER_X32; 0 from a library older than the counter); the steps and sweeps of the coarse sweeps on the
half-precision images (QPDO_INNER_H16: h16, h16sw; 0 from an older library).
With QPDO_SETUP_PROF=1 among them (or in the environment) the set-up's "[setup] ..." timing lines are printed under the side's line."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = r"""
import sys, time, json
sys.path.insert(0, %r)
from qpdo_amd import problems, solver
p = problems.config_qp("C4")
s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
out = []
for _ in range(2):
    t0 = time.time(); r = s.solve(); solver.lib().qpdo_amd_sync(s._w); dt = time.time() - t0
    st = s.stats()
    out.append(dict(t=dt, it=r["info"]["iterations"], st=r["info"]["status_val"], cg=st["lin_iters"], inner=st["inner_solves"],
                    sweeps=st["inner_refine_sweeps"], fallbacks=st["inner_refine_fallbacks"], worst=round(st["inner_refine_max_res_over_tol"], 3),
                    steps=st["inner_steps"], x32=st["inner_x32_steps"], h16=st["inner_h16_steps"], h16sw=st["inner_h16_sweeps"]))
print(json.dumps(out))
""" % ROOT
args = sys.argv[1:]
reps = int(args.pop()) if args and args[-1].isdigit() else 2
for rep in range(reps):
    for side in args:
        switches, _, lib = side.rpartition("@")
        env = dict(os.environ, QPDO_AMD_LIB=os.path.abspath(lib))
        env.update(kv.split("=", 1) for kv in switches.split(",") if kv)
        o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
        line = [l for l in o.stdout.splitlines() if l.startswith("[")]
        print((switches + " " if switches else "") + os.path.basename(lib), line[-1] if line else o.stderr[-500:], flush=True)
        for l in o.stderr.splitlines():
            if l.startswith("[setup]"):
                print("    " + l, flush=True)
