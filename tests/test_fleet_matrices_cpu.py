"""The fleet's matrix-update entry points (qpdo_amd_fleet_create_ex, _update_matrices, _get_matrix_stats; include/qpdo_amd_ext.h) where no
device is needed: invalid calls are refused by the host driver (qpdo_api.c) before the library initialises a device, the Python mirror of
QPDOAmdFleetMatrixStats has the C layout, and the Python front end checks list lengths and matrix shapes itself.  The refusable calls
again from a compiled C program with the host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from qpdo_amd import _build, problems, solver


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


def test_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    assert L.qpdo_amd_fleet_update_matrices(None, None, None) != 0 and "qpdo_amd_fleet_update_matrices: NULL fleet" in last_error()
    assert L.qpdo_amd_fleet_get_matrix_stats(None, C.byref(solver.FleetMatrixStats())) != 0
    assert "qpdo_amd_fleet_get_matrix_stats: NULL fleet" in last_error()


def test_create_ex_refuses_invalid_arguments_without_a_device(monkeypatch):
    # no device is visible to this process from here on: a create that got as far as the device would say "no HIP device"
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.setenv(v, "-1")
    L = solver.lib()
    st = solver.default_settings(verbose=0)
    img = solver.Batch([problems.random_qp(3, 12, 20, 0.3), problems.random_qp(41, 1500, 10, 0.002)])
    one = (C.POINTER(solver.QPDOData) * 1)(img.items[0].data)
    two = (C.POINTER(solver.QPDOData) * 2)(img.items[0].data, img.items[1].data)
    flag = solver.FLEET_MATRIX_UPDATES
    for flags in (2, flag | 4, -1, 1 << 40):
        assert not L.qpdo_amd_fleet_create_ex(1, one, C.byref(st), flags) and "unknown flag bits" in last_error(), flags
    assert "QPDO_AMD_FLEET_MATRIX_UPDATES" in last_error()
    for flags in (0, flag):
        assert not L.qpdo_amd_fleet_create_ex(0, one, C.byref(st), flags) and "count must be positive" in last_error()
        assert not L.qpdo_amd_fleet_create_ex(1, None, C.byref(st), flags) and "NULL data array" in last_error()
        assert not L.qpdo_amd_fleet_create_ex(1, one, None, flags) and "NULL settings" in last_error()
        assert not L.qpdo_amd_fleet_create_ex(1, one, C.byref(solver.default_settings(verbose=0, rho=2.0)), flags) and "invalid settings" in last_error()
        assert not L.qpdo_amd_fleet_create_ex(2, two, C.byref(st), flags) and "item 1 does not fit the fused kernel" in last_error()


def test_stats_mirrors_have_the_c_layout():
    M = solver.FleetMatrixStats
    assert C.sizeof(M) == 5 * 8
    assert [f for f, _ in M._fields_] == ["calls", "items_last_call", "value_bytes_uploaded_last_call", "resident_extra_bytes", "last_kernel_seconds"]
    assert [getattr(M, f).offset for f, _ in M._fields_] == [0, 8, 16, 24, 32]
    assert C.sizeof(solver.FleetStats) == 48            # QPDOAmdFleetStats did not change
    hdr = open(os.path.join(os.path.dirname(_build.INCLUDE), "include", "qpdo_amd_ext.h")).read()
    assert "#define QPDO_AMD_FLEET_MATRIX_UPDATES 1L" in hdr and solver.FLEET_MATRIX_UPDATES == 1
    assert "#define QPDO_AMD_FLEET_MATRIX_TABLE_BYTES 8" in hdr and solver.FLEET_MATRIX_TABLE_BYTES == 8
    body = hdr[hdr.index("typedef struct {\n    long calls;"):hdr.index("} QPDOAmdFleetMatrixStats;")]
    assert [w for w in ("calls", "items_last_call", "value_bytes_uploaded_last_call", "resident_extra_bytes", "last_kernel_seconds")
            if (" %s;" % w) in body] == [f for f, _ in M._fields_]


def test_python_front_end_checks_lengths_and_shapes_before_any_c_call():
    """Fleet._mat_ptrs is the check (the C side cannot see list lengths): exercised on an object that has no native fleet behind it"""
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims, F._qstype = None, 2, [(4, 3), (5, 0)], [-1, 1]
    with pytest.raises(ValueError, match="Q: expected a list of 2 matrices, got 1"):
        F._mat_ptrs([sp.identity(4)], "Q")
    with pytest.raises(ValueError, match=r"Q\[1\]: expected shape \(5, 5\)"):
        F._mat_ptrs([None, sp.identity(4)], "Q")
    with pytest.raises(ValueError, match=r"A\[0\]: expected shape \(3, 4\)"):
        F._mat_ptrs([sp.csc_matrix((4, 3)), None], "A")
    with pytest.raises(ValueError, match=r"A\[1\]: expected shape \(0, 5\)"):
        F._mat_ptrs([None, sp.csc_matrix((1, 5))], "A")
    assert F._mat_ptrs(None, "A") == (None, [])
    arr, keep = F._mat_ptrs([None, sp.identity(5) * 2.0], "Q")
    assert not arr[0] and arr[1].contents.stype == 1 and (arr[1].contents.nrow, arr[1].contents.ncol) == (5, 5)
    assert np.ctypeslib.as_array(C.cast(arr[1].contents.x, C.POINTER(C.c_double)), (5,)).tolist() == [2.0] * 5
    arr, keep = F._mat_ptrs([sp.csc_matrix(np.arange(12.0).reshape(3, 4)), None], "A")
    assert arr[0].contents.stype == 0 and (arr[0].contents.nrow, arr[0].contents.ncol) == (3, 4) and not arr[1]


def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_matrices_args_driver.c")
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
