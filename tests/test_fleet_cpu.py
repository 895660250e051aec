"""The fleet entry points (qpdo_amd_fleet_*, include/qpdo_amd_ext.h) where no device is needed: every invalid call is refused by the
argument checks of the host driver (qpdo_api.c) before the library initialises a device, and the Python mirror of QPDOAmdFleetStats has
the C layout.  The same calls again from a compiled C program with the host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np

from qpdo_amd import _build, problems, solver


def make_data(p, keep):
    img = solver.Batch([p])
    keep.append(img)
    return img.items[0].data


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


def test_create_refuses_invalid_arguments_without_a_device(monkeypatch):
    # no device is visible to this process from here on: a create that got as far as the device would say "no HIP device"
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.setenv(v, "-1")
    L, keep = solver.lib(), []
    st = solver.default_settings(verbose=0)
    ok = make_data(problems.random_qp(3, 12, 20, 0.3), keep)
    one = (C.POINTER(solver.QPDOData) * 1)(ok)
    for count in (0, -2):
        assert not L.qpdo_amd_fleet_create(count, one, C.byref(st)) and "count must be positive" in last_error()
    assert not L.qpdo_amd_fleet_create(1, None, C.byref(st)) and "NULL data array" in last_error()
    assert not L.qpdo_amd_fleet_create(1, one, None) and "NULL settings" in last_error()
    assert not L.qpdo_amd_fleet_create(1, one, C.byref(solver.default_settings(verbose=0, rho=2.0))) and "invalid settings" in last_error()
    assert not L.qpdo_amd_fleet_create(1, one, C.byref(solver.default_settings(verbose=0, eps_abs=0.0))) and "invalid settings" in last_error()
    two = (C.POINTER(solver.QPDOData) * 2)(ok, make_data(problems.random_qp(41, 1500, 10, 0.002), keep))
    assert not L.qpdo_amd_fleet_create(2, two, C.byref(st)) and "item 1 does not fit the fused kernel" in last_error()
    p = problems.random_qp(3, 12, 20, 0.3)
    p["l"] = p["u"] + 1.0
    two = (C.POINTER(solver.QPDOData) * 2)(make_data(p, keep), ok)
    assert not L.qpdo_amd_fleet_create(2, two, C.byref(st)) and "item 0 has a lower bound above its upper bound" in last_error()


def test_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    s, info = solver.FleetStats(), (solver.QPDOInfo * 1)()
    assert L.qpdo_amd_fleet_get_stats(None, C.byref(s)) != 0 and "NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_update(None, None, None, None) != 0 and "qpdo_amd_fleet_update: NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_warm_start(None, None, None) != 0 and "qpdo_amd_fleet_warm_start: NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_warm_start_last(None) != 0 and "qpdo_amd_fleet_warm_start_last: NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_solve(None, None, None, info) != 0 and "qpdo_amd_fleet_solve: NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_get_certificates(None, 0, None, None) != 0 and "NULL fleet" in last_error()
    L.qpdo_amd_fleet_destroy(None)


def test_stats_mirror_has_the_c_layout():
    assert C.sizeof(solver.FleetStats) == 6 * 8
    assert [f for f, _ in solver.FleetStats._fields_] == ["count", "matrix_bytes_uploaded", "vector_bytes_uploaded_last_call", "solve_launches",
                                                          "solves", "last_kernel_seconds"]
    assert solver.FleetStats.last_kernel_seconds.offset == 40 and solver.FLEET_TABLE_BYTES == 16
    hdr = open(os.path.join(os.path.dirname(_build.INCLUDE), "include", "qpdo_amd_ext.h")).read()
    assert "#define QPDO_AMD_FLEET_TABLE_BYTES 16" in hdr


def test_python_front_end_checks_lengths_and_shapes_before_any_c_call():
    """Fleet._ptrs is the check (the C side cannot see lengths): exercised on an object that has no native fleet behind it"""
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims = None, 2, [(4, 3), (5, 0)]
    import pytest
    with pytest.raises(ValueError, match="expected a list of 2"):
        F._ptrs([np.zeros(4)], ("q", 0))
    with pytest.raises(ValueError, match=r"q\[1\]: expected shape \(5,\)"):
        F._ptrs([None, np.zeros(4)], ("q", 0))
    with pytest.raises(ValueError, match=r"l\[0\]"):
        F._ptrs([np.zeros((3, 1)), None], ("l", 1))
    arr, keep = F._ptrs([np.array([1.0, np.inf, -np.inf]), None], ("u", 1), clip=True)
    assert len(keep) == 1 and keep[0].tolist() == [1.0, 1e20, -1e20] and not arr[1]
    assert F._ptrs(None, ("q", 0)) == (None, [])


def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_args_driver.c")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    if sanitize:
        supp = tmp_path / "lsan.supp"
        supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\nleak:librccl\n")
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                   LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    return out.returncode, out.stdout + out.stderr


def test_argument_checks_from_a_c_caller(tmp_path):
    rc, txt = run_driver(tmp_path, False)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """the host driver (qpdo_api.c) and the C caller with -fsanitize=address,undefined, as a stand-alone program on the CPU"""
    rc, txt = run_driver(tmp_path, True)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
