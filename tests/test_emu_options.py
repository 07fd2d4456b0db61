"""tests/option_cases.py on the wave emulator (tests/emu)."""
import pytest

import option_cases as oc
from fuzz_cases import BUILD_IDS, BUILD_LIST
from helpers import emu_lib
from timberborn_support_solver_amd import Mi355Sat

BUILDS = pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **kw)


@BUILDS
@pytest.mark.parametrize("name", [oc.UNSAT_CASE, oc.SAT_CASE])
def test_emulated_vivify(tmp_path, name, one_per_simd, lds_val):
    oc.check_vivify(emu_solver, tmp_path, name, one_per_simd, lds_val)


@pytest.mark.parametrize("one_per_simd,lds_val", [(0, 1), (4, -1)], ids=["one-wave-build-lds", "full-fleet-build-slab"])
@pytest.mark.parametrize("rephase", [1, 2])
@pytest.mark.parametrize("name", oc.REPHASE_CASES)
def test_emulated_rephase(tmp_path, name, rephase, one_per_simd, lds_val):
    oc.check_rephase(emu_solver, tmp_path, name, rephase, one_per_simd, lds_val)


@pytest.mark.parametrize("one_per_simd,lds_val", [(0, 1), (4, -1)], ids=["one-wave-build-lds", "full-fleet-build-slab"])
@pytest.mark.parametrize("knob", oc.KNOBS, ids=oc.KNOB_IDS)
def test_emulated_exchange_and_restart_knobs(tmp_path, knob, one_per_simd, lds_val):
    oc.check_knob(emu_solver, tmp_path, oc.UNSAT_CASE, knob, one_per_simd, lds_val)


@pytest.mark.parametrize("one_per_simd,lds_val", [(0, 1), (2, -1)], ids=["one-wave-build-lds", "two-waves-build-slab"])
@pytest.mark.parametrize("max_groups", [1, 3])
@pytest.mark.parametrize("name", [oc.UNSAT_CASE, oc.SAT_CASE])
def test_emulated_search_with_max_groups(tmp_path, name, max_groups, one_per_simd, lds_val):
    oc.check_search_max_groups(emu_solver, tmp_path, name, max_groups, one_per_simd, lds_val)


@pytest.mark.parametrize("lds_val", [0, -1], ids=["assignment-in-lds", "assignment-in-slab"])
@pytest.mark.parametrize("max_groups", oc.MAX_GROUPS)
@pytest.mark.parametrize("which", ["long-lists", "encoder"])
def test_emulated_bcp_fixpoints_at_every_group_count(which, max_groups, lds_val):
    oc.check_bcp_max_groups(emu_solver, which, max_groups, lds_val)
