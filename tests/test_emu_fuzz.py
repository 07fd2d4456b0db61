"""Random-CNF differential tests of the search kernel on the wave emulator (tests/emu): every case on all six builds
(ms_search_kernel<LV, WPS>), judged by the oracle - tests/fuzz_cases.py says how.  The suite's other formulas come from the
encoder or from long_list_formula; the first random formula tried (REPRODUCER) made the default build write past the end
of a worker's `toclear` array during conflict analysis (a literal resolved twice by the batched walk was listed twice)."""
import pytest

from fuzz_cases import BUILD_IDS, BUILD_LIST, EMU_CASES, REPRODUCER, REPRODUCER_OPTS, formula, solve_and_judge, verdict_mix
from helpers import emu_lib, random_cnf
from timberborn_support_solver_amd import Mi355Sat

BUILDS = pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def test_the_generator_reproduces_the_reported_formula():
    cl = random_cnf(1, 120, 516, (3,))
    assert len(cl) == 516 and all(len(c) == 3 and len({abs(l) for l in c}) == 3 and all(1 <= abs(l) <= 120 for l in c) for c in cl)
    assert cl[:3] == [[-61, 56, 91], [-33, 100, -18], [65, 120, 99]] and cl[-1] == [87, 3, 83]
    assert formula(REPRODUCER)[1] == 10                  # (and 635 oracle conflicts: asserted by formula())


def test_the_set_has_both_verdicts():
    n_sat, n_unsat = verdict_mix(EMU_CASES)
    assert n_sat >= 3 and n_unsat >= 3
    assert all(formula(c)[1] == c[6] for c in EMU_CASES.values())


@BUILDS
def test_emulated_reproducer_in_every_build(tmp_path, one_per_simd, lds_val):
    s, r, st = solve_and_judge(emu_solver, REPRODUCER, one_per_simd, lds_val, tmp_path, **REPRODUCER_OPTS)
    s.close()


@BUILDS
@pytest.mark.parametrize("name", list(EMU_CASES))
def test_emulated_random_cnf_in_every_build(tmp_path, name, one_per_simd, lds_val):
    s, r, st = solve_and_judge(emu_solver, EMU_CASES[name], one_per_simd, lds_val, tmp_path, slice_conflicts=100)
    s.close()
