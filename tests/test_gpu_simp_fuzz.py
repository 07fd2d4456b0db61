"""Differential tests of the simplification before search on the MI355X (run with -m gpu): the emulator's cases
(tests/test_emu_simp_fuzz.py) plus a handful of up to 300 variables and 1300 clauses - probing with several hundred workers,
ms_subsume_kernel in more than one block - every case with simp 0 and 2, both variable orders and both variants of the
probing kernel, and once with the default fleet; judged by the oracle alone - tests/simp_cases.py says how.  Every solve runs
under a deadline: running into it fails the test."""
import pytest

from simp_cases import GPU_CASES, N_SETS, assumption_mix, formula, judge, verdict_mix
from timberborn_support_solver_amd import Mi355Sat

pytestmark = pytest.mark.gpu

LIMIT_S = 20.0


def test_the_set_has_both_verdicts():
    n_sat, n_unsat = verdict_mix(GPU_CASES)
    assert n_sat >= 3 and n_unsat >= 3 and max(c[8] for c in GPU_CASES.values()) > 1000
    assert all(formula(c)[1] == c[7] for c in GPU_CASES.values())
    n_sat, n_unsat = assumption_mix(GPU_CASES)
    assert n_sat + n_unsat == N_SETS * len(GPU_CASES) and 4 * n_sat >= n_sat + n_unsat and 4 * n_unsat >= n_sat + n_unsat
    assert max(formula(c)[0].n_clauses for c in GPU_CASES.values()) > 4 * 256


@pytest.mark.parametrize("var_order,lds_val", [(0, 1), (0, -1), (1, 1), (1, -1)])
@pytest.mark.parametrize("simp", [0, 2])
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_simplification_of_structured_cnf(tmp_path, name, simp, var_order, lds_val):
    judge(Mi355Sat, GPU_CASES[name], simp, var_order, lds_val, tmp_path, limit_s=LIMIT_S)


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_the_default_fleet_attaches_to_a_simplified_formula(tmp_path, name):
    judge(Mi355Sat, GPU_CASES[name], 0, 0, 0, tmp_path, limit_s=LIMIT_S, workers=0)
