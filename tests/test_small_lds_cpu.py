"""The dynamic-LDS plan of the fused small-QP kernels (qpdo_amd/csrc/small_lds.h: the one definition the kernels carve their pointers from
and the host sizes its launches from) on the CPU.  A stand-alone C program (tests/small_lds_driver.c) includes only that header and sweeps
every n in 1..1024, m in 0..1024 and both column-buffer counts: regions in the documented order, none on top of another, each aligned to its
element type, the linesearch's regions inside U, the vector area 16-byte aligned and ending at the reported total, nothing shrinking as n
or m grows.  tests/golden/small_lds_table.json was recorded from the sizing functions of the commit before the header existed
(small_lds_bytes, small_vec_lds): rows for a list of shapes -- both sides of the packed-fits boundaries among them -- and a checksum of the
whole sweep; the header must reproduce both.  The same program runs a second time under AddressSanitizer + UBSan."""
import json
import os
import subprocess

import pytest

from qpdo_amd import _build

ROOT = os.path.dirname(_build.INCLUDE)
REQUIRED = {(1, 0), (1, 1), (120, 360), (200, 300), (256, 384), (1024, 1024)}
# the largest n whose packed factor fits beside (one set, two sets) of column buffers: both sides are rows of the table
BOUNDARY = {"m = 0": (193, 185), "m = n": (191, 184)}


def build_driver(out_dir, sanitize):
    exe = os.path.join(out_dir, "small_lds_driver" + ("_asan" if sanitize else ""))
    san = ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else ["-O2"]
    subprocess.check_call(["gcc", "-std=gnu11", *san, "-Wall", "-Werror", "-I", _build.CSRC, os.path.join(ROOT, "tests", "small_lds_driver.c"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "golden", "small_lds_table.json")) as f:
        return json.load(f)


def run(exe, table, **kw):
    shapes = sorted({(r[0], r[1]) for r in table["rows"]})
    out = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=600, **kw)
    return out.returncode, out.stdout + out.stderr


@pytest.fixture(scope="module")
def job(tmp_path_factory, table):
    d = tmp_path_factory.mktemp("small_lds")
    rc, txt = run(build_driver(str(d), False), table)
    return dict(dir=d, rc=rc, txt=txt)


def test_the_header_is_listed_for_the_build():
    assert "small_lds.h" in _build.HEADERS


def test_every_layout_of_the_sweep_keeps_its_invariants(job):
    assert job["rc"] == 0 and "swept %d triples, 0 violations" % (1024 * 1025 * 2) in job["txt"], job["txt"][-3000:]


def test_the_table_has_the_shapes_it_must_have(table):
    rows = {(r[0], r[1], r[2]): r for r in table["rows"]}
    assert all((n, m, s) in rows for n, m in REQUIRED for s in (1, 2))
    fits = table["columns"].index("packed_fits")
    for rule, last in BOUNDARY.items():
        for s in (1, 2):
            n = last[s - 1]
            assert rows[(n, 0 if rule == "m = 0" else n, s)][fits] == 1 and rows[(n + 1, 0 if rule == "m = 0" else n + 1, s)][fits] == 0, (rule, s)
    assert rows[(120, 360, 1)][3:] == [12768, 58080, 1, 70848, 66736] and rows[(120, 360, 2)][3:] == [20448, 58080, 1, 78528, 66736]
    assert rows[(1, 1, 1)][3:5] == [120, 128] and rows[(1, 1, 2)][3:5] == [184, 128] and rows[(1, 1, 1)][7] == 276


def test_the_header_reproduces_the_recorded_rows_and_the_checksum_of_the_sweep(job, table):
    got = [[int(v) for v in ln.split()[1:]] for ln in job["txt"].splitlines() if ln.startswith("row ")]
    assert sorted(got) == sorted(table["rows"]) and len(got) == len(table["rows"])
    assert "fnv1a64 %s" % table["fnv1a64"] in job["txt"], job["txt"][-300:]


def test_the_same_sweep_under_address_and_ub_sanitizers(job, table):
    exe = build_driver(str(job["dir"]), True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rc, txt = run(exe, table, env=env)
    assert rc == 0 and txt == job["txt"], txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
