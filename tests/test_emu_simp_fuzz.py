"""Differential tests of the simplification before search on the wave emulator (tests/emu): formulas with planted
equivalences, failed literals, subsumptions, strengthenings and elimination candidates (helpers.structured_cnf) through the
default pipeline - els_scc, ms_probe_kernel in its LDS and slab variant, ms_subsume_kernel, bve_eliminate / extend_model -
as a plain solve and as a batch under assumptions, judged by the oracle alone; tests/simp_cases.py says how.  Every case runs
with simp 0 and 2; the second variable order and the slab variant of the probing kernel run on simp_cases.MATRIX_CASES."""
import pytest

from helpers import STRUCTURE, emu_lib, structured_cnf
from simp_cases import EMU_CASES, FEATURE_COUNTER, MATRIX_CASES, N_SETS, assumption_mix, assumption_sets, formula, judge, verdict_mix
from timberborn_support_solver_amd import Mi355Sat


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def test_the_generator_is_seeded_and_plants_what_it_says():
    a, sa = structured_cnf(8, 110, 170, features=("equiv", "failed", "strengthen", "elim"))
    b, sb = structured_cnf(8, 110, 170, features=("equiv", "failed", "strengthen", "elim"))
    assert (a, sa) == (b, sb) and structured_cnf(9, 110, 170, features=("equiv", "failed", "strengthen", "elim"))[0] != a
    assert all(c and all(l != 0 and abs(l) <= 110 for l in c) for c in a) and max(abs(l) for c in a for l in c) == 110
    n_base = 110 - len(sa)
    assert sorted(sa) == list(range(n_base + 1, 111))                       # the gadgets' variables: every one above the base
    cl, _ = structured_cnf(5, 110, 100, features=("long",))
    assert sorted(len(c) for c in cl)[-3:] == [66, 70, 72]                   # the victim, the subsumer that is too long, its superset
    cl, _ = structured_cnf(7, 40, 110, features=("salt",))
    assert any(len(c) == 1 for c in cl) and any(len(set(c)) < len(c) for c in cl) and any(-l in c for c in cl for l in c)
    assert structured_cnf(3, 40, 100, features=())[0] == structured_cnf(3, 40, 100, features=())[0]
    for f in STRUCTURE:                                                     # every feature is a switch of its own
        assert structured_cnf(3, 140, 100, features=(f,))[0] != structured_cnf(3, 140, 100, features=())[0], f


def test_the_set_has_both_verdicts():
    n_sat, n_unsat = verdict_mix(EMU_CASES)
    assert n_sat >= 3 and n_unsat >= 3
    assert all(formula(c)[1] == c[7] for c in EMU_CASES.values())
    n_sat, n_unsat = assumption_mix(EMU_CASES)
    assert n_sat + n_unsat == N_SETS * len(EMU_CASES) and 4 * n_sat >= n_sat + n_unsat and 4 * n_unsat >= n_sat + n_unsat
    for c in EMU_CASES.values():
        sets = assumption_sets(c)[0]
        assert len(sets) == N_SETS and sets[0] == [] and len(set(sets[1])) < len(sets[1]) and any(-l in sets[2] for l in sets[2])
        assert all(1 <= len(a) <= 8 for a in sets[1:])
    assert set(MATRIX_CASES) <= set(EMU_CASES)


def test_every_planted_feature_is_named_by_a_case_s_counters():
    for f in STRUCTURE:
        assert any(f in c[4] and FEATURE_COUNTER[f] in c[9] for c in EMU_CASES.values()), f
    assert {c[5] for c in EMU_CASES.values()} == {None, "scc", "failed"}


@pytest.mark.parametrize("simp", [0, 2])
@pytest.mark.parametrize("name", list(EMU_CASES))
def test_emulated_simplification_of_structured_cnf(tmp_path, name, simp):
    judge(emu_solver, EMU_CASES[name], simp, 0, 1, tmp_path)


@pytest.mark.parametrize("var_order,lds_val", [(0, -1), (1, 1), (1, -1)])
@pytest.mark.parametrize("simp", [0, 2])
@pytest.mark.parametrize("name", MATRIX_CASES)
def test_emulated_simplification_in_the_other_variable_order_and_probe_variant(tmp_path, name, simp, var_order, lds_val):
    judge(emu_solver, EMU_CASES[name], simp, var_order, lds_val, tmp_path)
