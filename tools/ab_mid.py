"""A/B timing of builds of libqpdo_amd.so on one box at mid size: C2 (n = 1e4, m = 2e4: dense LDL' path) and a chain-structured QP
(n = 2e4, m = 39999: band solver), three cold-start solves each per process, alternating processes.  Both take the radix path of the
linesearch (2m > 8192) and neither the PCG path.
usage: ab_mid.py libA.so libB.so [reps]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = r"""
import sys, time, json
sys.path.insert(0, %r)
from qpdo_amd import problems, solver
out = {}
for name, p in (("C2", problems.config_qp("C2")), ("banded20k", problems.banded_qp(7, 20000))):
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    ts = []
    for _ in range(3):
        t0 = time.time(); r = s.solve(); solver.lib().qpdo_amd_sync(s._w); ts.append(round(time.time() - t0, 5))
    out[name] = dict(t=ts, it=r["info"]["iterations"], st=r["info"]["status_val"], linsolve=s.stats()["linsolve"], m=p["m"])
    s.delete()
print(json.dumps(out))
""" % ROOT
libs = sys.argv[1:3]
for rep in range(int(sys.argv[3]) if len(sys.argv) > 3 else 2):
    for lib in libs:
        env = dict(os.environ, QPDO_AMD_LIB=os.path.abspath(lib))
        o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=280)
        line = [l for l in o.stdout.splitlines() if l.startswith("{")]
        print(os.path.basename(lib), line[-1] if line else o.stderr[-800:], flush=True)
        if o.returncode != 0:
            sys.exit(o.returncode if o.returncode > 0 else 1)
