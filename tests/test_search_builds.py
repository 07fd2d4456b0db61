"""Which build of the search kernel a launch runs (ms_search_kernel<LV, WPS>: assignment in LDS or in the slab; compiled
for 1, 2 or 4 waves per SIMD): the selection rule as a table, evaluated through mi355sat_debug_search_build_rule of the
emulator library - host code only, nothing is launched.

The expected values are NOT taken from the product: they restate the comments of include/mi355sat.h (opts.one_per_simd,
opts.lds_val) and of choose_build in plain signed Python integers:
  waves per SIMD  1 for at most 1024 workers, 2 for at most 2048, else 4; one_per_simd = -1 always 4, 2 / 4 at least that;
  LDS             lds_val = 1 forces it, -1 forbids it; on auto the formula's bytes must fit 150 KB / (workers per CU) minus
                  the static reserve of a workgroup (14 KB up to 8 workers per CU: the builds with the sort buffer, else
                  6 KB), at most 64 KB.  From 26 workers per CU on (more than 6400 workers) that difference is negative:
                  nothing fits.  (Unsigned arithmetic wrapped there and picked the LDS build with up to 64 KB per workgroup.)
"""
import ctypes

import pytest

from helpers import emu_lib
from timberborn_support_solver_amd import Mi355Sat
from timberborn_support_solver_amd.solver import Mi355SatSearchBuild

KB = 1024


def budget(active):
    per_cu = (active + 255) // 256
    return min(64 * KB, 150 * KB // per_cu - (14 if per_cu <= 8 else 6) * KB)       # signed: may be negative


def expected(active, nbytes, lds_val, one_per_simd):
    wps = 4 if one_per_simd < 0 else (1 if active <= 1024 else (2 if active <= 2048 else 4))
    if one_per_simd in (2, 4):
        wps = max(wps, one_per_simd)
    if lds_val == 1:
        lds = nbytes <= 150 * KB          # what no CU can hold is never staged
    elif lds_val == -1:
        lds = False
    else:
        lds = nbytes <= budget(active)
    return dict(lds=int(lds), wps=wps, dyn_lds_bytes=nbytes if lds else 0, active=active, lds_val_bytes=nbytes)


def rule(active, nbytes, lds_val, one_per_simd, **kw):
    return Mi355Sat.debug_search_build_rule(active, nbytes, lds_val=lds_val, one_per_simd=one_per_simd, _lib_override=emu_lib(), **kw)


def check(active, nbytes, lds_val, one_per_simd):
    got = rule(active, nbytes, lds_val, one_per_simd)
    want = expected(active, nbytes, lds_val, one_per_simd)
    assert {k: got[k] for k in want} == want, (active, nbytes, lds_val, one_per_simd)
    assert got["launches"] == 0 and got["builds_seen"] == 0


@pytest.mark.parametrize("active", [1, 1024, 1025, 2048, 2049, 4096])
def test_waves_per_simd_and_lds_by_fleet_size(active):
    for one_per_simd in (-1, 0, 2, 4):
        for lds_val in (-1, 0, 1):
            for nbytes in (24, 3 * KB, 9 * KB, 40 * KB, 64 * KB, 64 * KB + 4, 150 * KB, 150 * KB + 4):
                check(active, nbytes, lds_val, one_per_simd)


@pytest.mark.parametrize("per_cu", [1, 8, 9, 16])
def test_lds_budget_edges(per_cu):
    """Just below, at and just above the budget, at both ends of the range of fleets with that many workers per CU."""
    want_budget = {1: 64 * KB, 8: 4864, 9: 10922, 16: 3456}[per_cu]      # 150 KB / per_cu - reserve, by hand
    for active in ((per_cu - 1) * 256 + 1, per_cu * 256):
        b = budget(active)
        assert b == want_budget
        for nbytes in (b - 4, b - 1, b, b + 1, b + 4):
            for one_per_simd in (-1, 0, 2, 4):
                check(active, nbytes, 0, one_per_simd)
            assert rule(active, nbytes, 0, 0)["lds"] == int(nbytes <= b)


@pytest.mark.parametrize("per_cu", [25, 26, 32])
def test_lds_budget_does_not_wrap_above_6400_workers(per_cu):
    """25 workers per CU: the share equals the reserve, budget 0.  26 and 32 (6656, 8192 workers): negative.  No formula's
    assignment (24 bytes for one variable) is staged in LDS on auto."""
    active = per_cu * 256
    assert budget(active) <= 0 and (budget(active) < 0) == (per_cu >= 26)
    for nbytes in (24, 1 * KB, 3 * KB, 40 * KB, 64 * KB, 64 * KB + 4):
        for one_per_simd in (-1, 0, 2, 4):
            check(active, nbytes, 0, one_per_simd)
            check(active, nbytes, -1, one_per_simd)
            check(active, nbytes, 1, one_per_simd)
        got = rule(active, nbytes, 0, 0)
        assert (got["lds"], got["wps"], got["dyn_lds_bytes"]) == (0, 4, 0)


def test_other_kernels_follow_the_handle_s_own_staging_decision():
    """BCP and probing launches (mode != 0) have no budget rule and no waves-per-SIMD builds: they stage the assignment
    when it is forced, or on auto when it fits 10 KB (16 workers per CU)."""
    for mode in (1, 2):
        for nbytes, lds_val, want in [(10 * KB, 0, 1), (10 * KB + 4, 0, 0), (64 * KB, 1, 1), (150 * KB + 4, 1, 0), (24, -1, 0)]:
            got = rule(4096, nbytes, lds_val, 0, mode=mode)
            assert (got["lds"], got["wps"], got["dyn_lds_bytes"]) == (want, 0, nbytes if want else 0)
    assert rule(256, 40 * KB, 0, 0, mode=1, staged=1)["lds"] == 1 and rule(256, 24, 0, 0, mode=1, staged=0)["lds"] == 0


def test_hook_struct_and_state():
    from timberborn_support_solver_amd.solver import SolverError
    assert ctypes.sizeof(Mi355SatSearchBuild) == 32
    with pytest.raises(SolverError):
        rule(0, 24, 0, 0)                                   # no launch has zero workers
    s = Mi355Sat(_lib_override=emu_lib(), simp=-1)
    with pytest.raises(SolverError):
        s.debug_last_search_build()                         # nothing launched yet
    s.add_clause([1, 2]); s.add_clause([-1, 2]); s.add_clause([1, -2]); s.add_clause([-1, -2])
    assert s.solve().name == "Unsat"
    b = s.debug_last_search_build()
    assert (b["lds"], b["wps"]) == (1, 1) and b["launches"] >= 1 and b["builds"] == {(1, 1)}
    assert b["dyn_lds_bytes"] == b["lds_val_bytes"] == 24   # 2 variables: one word of 2-bit values + five 1-bit maps
    s.close()
