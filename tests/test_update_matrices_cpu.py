"""qpdo_amd_update_matrices without a device: the exported symbol, the prototype in the public header (C99 and C++), and the subset-pattern
projection of the Python wrapper."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from qpdo_amd import _build, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_library_exports_update_matrices():
    L = ctypes.CDLL(_build.ensure_lib())
    assert hasattr(L, "qpdo_amd_update_matrices")
    assert "qpdo_amd_update_matrices" in solver.EXT_SYMBOLS


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99", "-Wall", "-Werror", "-x", "c"]), ("g++", ["-Wall", "-Werror", "-x", "c++"])])
def test_header_prototype_compiles(compiler, flags, tmp_path):
    if not shutil.which(compiler):
        pytest.skip("%s not installed" % compiler)
    src = tmp_path / "use_update.c"
    src.write_text('#include "qpdo.h"\n#include "qpdo_amd_ext.h"\n'
                   "int (*fp)(QPDOWorkspace *, const cholmod_sparse *, const cholmod_sparse *) = qpdo_amd_update_matrices;\n"
                   "int main(void) { return fp == 0; }\n")
    subprocess.check_call([compiler, *flags, "-I", INCLUDE, "-fsyntax-only", str(src)])


def _pattern(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


def test_projection_of_the_same_pattern_is_the_data():
    M = sp.random(30, 20, density=0.2, format="csc", random_state=1)
    M.sort_indices()
    p, i = _pattern(M)
    assert np.array_equal(solver.project_to_pattern(M, p, i), M.data)


def test_projection_of_a_subset_gives_explicit_zeros():
    M = sp.random(30, 20, density=0.3, format="csc", random_state=2)
    M.sort_indices()
    p, i = _pattern(M)
    S = M.copy()
    S.data[::3] = 0.0
    S.eliminate_zeros()
    x = solver.project_to_pattern(S, p, i)
    expect = M.data.copy()
    expect[::3] = 0.0
    assert np.array_equal(x, expect)
    # unsorted, duplicated input: summed and placed
    coo = S.tocoo()
    dup = sp.coo_matrix((np.concatenate([coo.data / 2, coo.data / 2]), (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))),
                        shape=S.shape)
    assert np.allclose(solver.project_to_pattern(dup, p, i), expect)


def test_projection_refuses_an_entry_outside_the_pattern():
    M = sp.csc_matrix(np.array([[1.0, 0.0], [2.0, 3.0]]))
    p, i = _pattern(M)
    with pytest.raises(ValueError):
        solver.project_to_pattern(sp.csc_matrix(np.array([[1.0, 4.0], [2.0, 3.0]])), p, i)
    with pytest.raises(ValueError):
        solver.project_to_pattern(sp.csc_matrix(np.ones((2, 3))), p, i)
