"""Where the fused small-QP kernel keeps the Newton matrix (qpdo_amd_small_factor_layout, include/qpdo_amd_ext.h): the rule is host
arithmetic and the launches go through the function the query goes through (small_plan, qpdo_small.hip), so it is checked here without a
device -- the half-bandwidths, the band layout for chain-structured items whose packed factor does not fit, every decision made before
the band layout existed, and the opt-out."""
import functools

import numpy as np

from qpdo_amd import problems, solver

GLOBAL, PACKED, BAND = solver.K_GLOBAL, solver.K_PACKED, solver.K_BAND
KINDS = (solver.KIND_BATCH, solver.KIND_STREAM, solver.KIND_FLEET)


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (problem, half-bandwidth): the chain-structured instances of the band layout's GPU tests"""
    return dict(A=(problems.banded_random_qp(1, 256, 12), 12), B=(problems.banded_qp(3, 301), 1), C=(problems.banded_random_qp(5, 333, 31), 31),
                D=(problems.banded_random_qp(4, 610, 5), 5), E=(problems.banded_qp(6, 512), 1), F=(problems.banded_random_qp(2, 200, 70), 70))


def layout(probs, kind):
    return solver.small_factor_layout(list(probs), kind, verbose=0)


def test_half_bandwidths_and_the_band_layout_for_every_kind():
    S = shapes()
    assert [(S[k][0]["n"], S[k][0]["m"]) for k in "ABCDEF"] == [(256, 384), (301, 601), (333, 499), (610, 915), (512, 1023), (200, 300)]
    for kind in KINDS:
        for k in "ABCDE":
            assert layout([S[k][0]], kind) == (BAND, [S[k][1]]), (k, kind)
        assert layout([S[k][0] for k in "ABCDE"], kind) == (BAND, [S[k][1] for k in "ABCDE"]), kind
        assert layout([S["F"][0]], kind) == (BAND, [70]), kind          # alone: 17 KB fixed + 114 KB band image
        assert layout([S[k][0] for k in "ABCDEF"], kind)[0] == GLOBAL, kind  # beside n 610, m 1023 F's image does not fit


def test_the_half_bandwidth_is_that_of_the_pattern():
    """the largest |i - j| over Q's stored entries and the largest column span of a row of A: equal to the bandwidth of the pattern of
    Q + A'A computed independently; an item with m = 0 takes Q's; a dense item is n - 1"""
    for p in (shapes()["A"][0], shapes()["D"][0], problems.random_qp(21, 30, 0, 0.2), problems.random_qp(23, 40, 60, 0.2, 10)):
        A, Q = abs(p["A"]).tocsr(), abs(problems.full_Q(p))
        Kp = (Q + A.T @ A).tocoo()
        Kp.data[:] = 1.0
        b = int(np.max(np.abs(Kp.row - Kp.col))) if Kp.nnz else 0
        assert layout([p], solver.KIND_BATCH)[1] == [b], (p["n"], p["m"])
    assert layout([problems.infeasibility_kat("primal_infeasible")], solver.KIND_FLEET)[1] == [1]


def test_decisions_made_before_the_band_layout_are_unchanged():
    for kind in KINDS:
        assert layout([problems.config_qp("C3", 0)], kind)[0] == PACKED, kind
    # the heterogeneous fleet of tests/test_gpu_fleet.py with its dense n = 200 item (fleet_problems(), re-stated): the packed factor does
    # not fit, and the dense item's band image is 200 * 200 * 8 B = 320 KB
    fleet = (problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"), problems.config_qp("C3", 0),
             problems.config_qp("C3", 5), problems.random_qp(21, 30, 0, 0.2), problems.random_qp(22, 200, 300, 0.05), problems.random_qp(23, 40, 60, 0.2, 10))
    for kind in KINDS:
        lay, bw = layout(fleet, kind)
        assert lay == GLOBAL and bw[5] == 199, (kind, lay, bw)
        assert layout(fleet[:5] + fleet[6:], kind)[0] == PACKED, kind


def test_a_mixed_launch_takes_the_band_layout():
    probs = [shapes()["A"][0], problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"), problems.random_qp(21, 30, 0, 0.2)]
    for kind in KINDS:
        lay, bw = layout(probs, kind)
        assert lay == BAND and bw[0] == 12 and bw[1] == 1 and bw[2] <= 1 and bw[3] <= 29, (kind, lay, bw)


def test_a_band_that_does_not_fit_goes_to_global_memory():
    p = problems.banded_random_qp(8, 400, 60)            # 400 * 61 * 8 B = 195 KB: more than a workgroup's LDS
    for kind in KINDS:
        assert layout([p], kind) == (GLOBAL, [60]), kind
        assert layout([shapes()["A"][0], p], kind)[0] == GLOBAL, kind      # one such item decides for the launch


def test_an_item_that_does_not_fit_the_fused_kernel_is_refused():
    p = problems.banded_qp(1, 1025)
    for kind in KINDS:
        assert layout([p], kind)[0] == -1
        assert layout([shapes()["A"][0], p], kind)[0] == -1
    assert "does not fit the fused kernel" in (solver.lib().qpdo_amd_last_error() or b"").decode()
    assert layout([shapes()["A"][0]], 3)[0] == -1        # an unknown kind


def test_the_opt_out_keeps_todays_choice(monkeypatch):
    S = shapes()
    monkeypatch.setenv("QPDO_SMALL_BAND", "0")
    for kind in KINDS:
        for k in "ABCDEF":
            assert layout([S[k][0]], kind) == (GLOBAL, [S[k][1]]), (k, kind)
        assert layout([problems.config_qp("C3", 0)], kind)[0] == PACKED
    monkeypatch.setenv("QPDO_SMALL_BAND", "1")
    assert layout([S["A"][0]], solver.KIND_BATCH)[0] == BAND


def test_the_python_constants_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(solver._build.INCLUDE, "qpdo_amd_ext.h")).read()
    for name, val in (("GLOBAL", GLOBAL), ("PACKED", PACKED), ("BAND", BAND)):
        assert re.search(r"#define QPDO_AMD_SMALL_K_%s\s+%d\b" % (name, val), hdr), name
    assert solver.lib().qpdo_amd_fleet_factor_layout(None) == -1 and "NULL fleet" in (solver.lib().qpdo_amd_last_error() or b"").decode()
