"""Differential tests of the warm incremental solve and of foreign ring records on the MI355X (run with -m gpu): the
emulator's sequences (tests/test_emu_incremental_fuzz.py) on all six builds of the search kernel - which build ran is
asserted through mi355sat_debug_last_search_build - plus a handful on larger bases (up to 300 variables, 25 solves, fleets of
1, 8 and 258 workers), and the records that collapse under the importer's simplification; judged by the oracle alone -
tests/incremental_cases.py and tests/import_cases.py say how.  Every search call runs under a deadline: running into it
fails the test."""
import pytest

import import_cases as im
import incremental_cases as ic
from simp_cases import within
from test_gpu_cores import assert_ran_the_build_asked_for
from timberborn_support_solver_amd import Mi355Sat, _lib

pytestmark = pytest.mark.gpu

LIMIT_S = 20.0


def release():
    _lib.solver_lib().mi355sat_release_cached_memory()


def step_within(s):
    return within(LIMIT_S, s, s.sweep_step)


@pytest.mark.parametrize("lds_val", [0, -1])
@pytest.mark.parametrize("one_per_simd", [0, 2, 4])
@pytest.mark.parametrize("name", list(ic.CASES))
def test_warm_sequence_on_every_search_build(tmp_path, name, one_per_simd, lds_val):
    c, e = ic.run_sequence(Mi355Sat, name, tmp_path, limit_s=LIMIT_S, release=release, one_per_simd=one_per_simd, lds_val=lds_val)
    assert_ran_the_build_asked_for(c.s, one_per_simd, lds_val)
    assert e.warm_attached > 0 and e.warm >= 2, (e.warm, e.cold)
    c.s.close()


@pytest.mark.parametrize("one_per_simd,lds_val", [(0, 0), (4, -1)])
@pytest.mark.parametrize("name", list(ic.GPU_ONLY_CASES))
def test_warm_sequence_on_a_larger_base(tmp_path, name, one_per_simd, lds_val):
    c, e = ic.run_sequence(Mi355Sat, name, tmp_path, limit_s=LIMIT_S, release=release, one_per_simd=one_per_simd, lds_val=lds_val)
    assert_ran_the_build_asked_for(c.s, one_per_simd, lds_val)
    assert e.warm_attached > 0 and e.warm >= 2, (e.warm, e.cold)
    c.s.close()


@pytest.mark.parametrize("simp", [0, 2])
@pytest.mark.parametrize("name", list(im.IMPORT_CASES))
def test_import_of_records_that_collapse(name, simp):
    s, _ = im.check_collapsing_imports(Mi355Sat, name, simp, step=step_within)
    s.close()


@pytest.mark.parametrize("simp_b", [0, 2])
@pytest.mark.parametrize("name", im.TWO_HANDLE_CASES)
def test_exchange_between_two_live_handles(name, simp_b):
    for s in im.check_two_live_handles(Mi355Sat, name, simp_b, step=step_within):
        s.close()
