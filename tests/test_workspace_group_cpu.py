"""Groups of right-hand sides in the workspace adjoint / tangent (qpdo_amd_rhs_group, qpdo_amd_get_group_stats, qpdo_amd_spmv_group;
include/qpdo_amd_ext.h) where no device is needed: every check that comes before the backend is touched, by message, from a compiled C
program (tests/group_args_driver.c), plain and with the host driver under AddressSanitizer + UBSan; the symbols and the layout of the
stats; solver.QPDO.jacobian validates its names before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from qpdo_amd import _build, solver


def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="group_args_driver.c")
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


def test_the_symbols_and_the_stats_layout():
    L = solver.lib()
    for name in ("qpdo_amd_rhs_group", "qpdo_amd_get_group_stats", "qpdo_amd_spmv_group"):
        assert name in solver.EXT_SYMBOLS and hasattr(L, name)
    assert C.sizeof(solver.GroupStats) == 32
    assert [f for f, _ in solver.GroupStats._fields_] == ["group", "groups_run", "rounds_total", "scratch_bytes"]
    assert L.qpdo_amd_rhs_group(None) == -1
    s = solver.GroupStats(-5, -5, -5, -5)
    assert L.qpdo_amd_get_group_stats(None, C.byref(s)) != 0
    assert (L.qpdo_amd_last_error() or b"").decode() == "qpdo_amd_get_group_stats: NULL workspace"
    assert (s.group, s.groups_run, s.rounds_total, s.scratch_bytes) == (-5, -5, -5, -5)


def test_spmv_group_refuses_before_any_device_call():
    L = solver.lib()
    v, y = np.arange(8.0), np.full(8, 7.0)
    vp, yp = v.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double))
    for args, msg in (((None, 0, 0, 0, vp, yp), "nvec must be 1 .. 8"), ((None, 0, 9, 1, vp, yp), "nvec must be 1 .. 8"),
                      ((None, 1, 3, 0b1000, vp, yp), "live_mask names a vector >= nvec"), ((None, 2, 2, 3, None, yp), "v is NULL"),
                      ((None, 2, 2, 3, vp, None), "y is NULL"), ((None, 2, 2, 3, vp, yp), "NULL workspace")):
        assert L.qpdo_amd_spmv_group(*args) != 0
        assert (L.qpdo_amd_last_error() or b"").decode() == "qpdo_amd_spmv_group: " + msg
    assert (y == 7.0).all()


def test_jacobian_validates_before_any_library_call():
    """no workspace here (the handle is NULL and never reached): every refusal comes from the checks of the names"""
    qp = solver.QPDO()
    qp.n, qp.m = 5, 3
    with pytest.raises(ValueError, match=r"^wrt: unknown name 'Q'"):
        qp.jacobian(wrt=("q", "Q"))
    with pytest.raises(ValueError, match=r"^wrt: expected at least one name"):
        qp.jacobian(wrt=())
    with pytest.raises(ValueError, match=r"^wrt: expected a tuple of names"):
        qp.jacobian(wrt="q")
    with pytest.raises(ValueError, match=r"^wrt: a name is given twice"):
        qp.jacobian(wrt=("q", "q"))
    with pytest.raises(ValueError, match=r"^outputs: unknown name 'z'"):
        qp.jacobian(outputs=("x", "z"))
    with pytest.raises(ValueError, match=r"^outputs: expected at least one name"):
        qp.jacobian(outputs=())
    with pytest.raises(ValueError, match=r"^mode: expected 'auto', 'tangent' or 'adjoint', got 'forward'"):
        qp.jacobian(mode="forward")
    with pytest.raises(RuntimeError, match=r"^jacobian: no workspace"):
        qp.jacobian()
