"""Random-CNF differential tests of the search kernel on the MI355X (run with -m gpu): the emulator's cases
(tests/test_emu_fuzz.py) plus a handful of up to a few thousand oracle conflicts, every case on all six builds, judged by the
oracle - tests/fuzz_cases.py says how.  Every solve runs under a deadline: running into it fails the test."""
import pytest

from fuzz_cases import BUILD_IDS, BUILD_LIST, GPU_CASES, REPRODUCER, REPRODUCER_OPTS, formula, solve_and_judge, verdict_mix
from test_gpu_parity import solve_within
from timberborn_support_solver_amd import Mi355Sat

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)
LIMIT_S = 20.0


def within(s):
    return solve_within(s, LIMIT_S)


def test_the_set_has_both_verdicts():
    n_sat, n_unsat = verdict_mix(GPU_CASES)
    assert n_sat >= 3 and n_unsat >= 3 and max(c[7] for c in GPU_CASES.values()) > 1000
    assert all(formula(c)[1] == c[6] for c in GPU_CASES.values())


@BUILDS
def test_reproducer_in_every_build(tmp_path, one_per_simd, lds_val):
    s, r, st = solve_and_judge(Mi355Sat, REPRODUCER, one_per_simd, lds_val, tmp_path, solve=within, **REPRODUCER_OPTS)
    print(f"reproducer, build ({one_per_simd}, {lds_val}): {r.name} after {st['conflicts']} conflicts")
    s.close()


@BUILDS
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_random_cnf_in_every_build(tmp_path, name, one_per_simd, lds_val):
    s, r, st = solve_and_judge(Mi355Sat, GPU_CASES[name], one_per_simd, lds_val, tmp_path, solve=within, slice_conflicts=100)
    s.close()
