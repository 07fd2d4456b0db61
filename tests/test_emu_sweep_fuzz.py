"""Differential tests of the stepwise sweep's schedule calls on the wave emulator (tests/emu): mi355sat_sweep_drop / _reopen /
_set_weights / _sweep_model_of between the slices of a sweep over random and structured formulas under arbitrary assumption
lists, driven by seeded schedules and judged by the oracle alone after every step - tests/sweep_cases.py says how.  Every run
is deterministic (opts.deterministic = 1): a failure repeats."""
import pytest

from fuzz_cases import BUILD_IDS, BUILD_LIST
from helpers import emu_lib
from sweep_cases import (ACTIONS, CASES, FINDING, FORMULA_UNSAT, LONG, LONG_LENS, MATRIX_CASES, OPTSETS, REPEATS, SEEDS, STALL_SCRIPTS,
                         UNSCHEDULED, VAR_ORDER_CASE, final_step, judge, lists, long_to_empty_and_back, options, seeded_schedule,
                         slice_cap, stop_at_first, verdict_mix)
from timberborn_support_solver_amd import Mi355Sat


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def emu_options(name, optset, **more):
    return options(name, optset, deterministic=1, **more)


def test_the_set_has_both_verdicts():
    for name in CASES:
        ls, verdicts = lists(name)
        assert 6 <= len(ls) <= 10 and ls[0] == [] and len(set(ls[1])) < len(ls[1]) and any(-l in ls[2] for l in ls[2])
        assert ls[3] == ls[4] and set(ls[3]) < set(ls[5])
        assert all(1 <= len(a) <= 8 for a in ls[1 + (name == REPEATS):6]) and (name != REPEATS or len(ls[1]) > CASES[name][2] >= len(set(ls[1])))          # (1 .. 6 random literals, plus the repeat / the pair / the superset's own)
        assert set(verdicts) == ({20} if name == FORMULA_UNSAT else {10, 20}), (name, verdicts)
    assert CASES[FORMULA_UNSAT][6] == 20 and all(c[6] == 10 for n, c in CASES.items() if n != FORMULA_UNSAT)
    n_sat, n_unsat = verdict_mix(CASES)
    assert n_sat + n_unsat == sum(c[8] for c in CASES.values()) and 10 * n_sat >= 3 * (n_sat + n_unsat) and 10 * n_unsat >= 3 * (n_sat + n_unsat)
    assert CASES[LONG][2] >= 140 and tuple(len(a) for a in lists(LONG)[0][-4:]) == LONG_LENS
    assert set(lists(LONG)[1][-4:]) == {10, 20}
    assert set(MATRIX_CASES) <= set(CASES) and FINDING in CASES and VAR_ORDER_CASE in CASES
    assert set(UNSCHEDULED) == set(CASES) and all(set(u) == set(OPTSETS) for u in UNSCHEDULED.values())


def test_the_schedules_make_every_action():
    assert len(SEEDS) >= 6
    for n in sorted({c[8] for c in CASES.values()}):
        scheds = [seeded_schedule(seed, n) for seed in SEEDS]
        assert scheds == [seeded_schedule(seed, n) for seed in SEEDS] and len({str(s) for s in scheds}) == len(SEEDS)
        for sched in scheds:
            kinds = [a[1] for a in sched]
            assert {"drop", "reopen", "weights", "drop_decided", "reopen_open", "models"} <= set(kinds)
            drops = [a[2] for a in sched if a[1] == "drop"]
            assert [] in drops and list(range(n)) in drops and any(len(d) == n - 1 for d in drops) and any(len(d) == 1 for d in drops)
            weights = [a[2] for a in sched if a[1] == "weights"]
            assert [0.0] * n in weights and any(max(w) == 50.0 for w in weights) and any(0.0 in w and max(w) > 0 for w in weights)
            assert any(a == b for a, b in zip(weights, weights[1:]))                  # the same vector twice
            assert all(0 <= i < n for a in sched if a[1] in ("drop", "reopen") for i in a[2])
            assert final_step(sched) >= 6
    assert len(ACTIONS) == 12


@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_sweep_without_schedule_calls(name, optset):
    """The run the liveness bound is measured against: it ends, in the slices the table says."""
    after, _, st = judge(emu_solver, name, emu_options(name, optset), [], cap=200)
    print(name, optset, "slices", after, "conflicts", st["conflicts"])
    assert after == UNSCHEDULED[name][optset]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_sweep_under_a_seeded_schedule(name, optset, seed):
    sched = seeded_schedule(seed, CASES[name][8])
    after, steps, st = judge(emu_solver, name, emu_options(name, optset), sched, cap=slice_cap(name, optset))
    print(name, optset, seed, "slices after the final act", after, "of", slice_cap(name, optset), "in all", steps, "conflicts", st["conflicts"])


@pytest.mark.parametrize("script", list(STALL_SCRIPTS))
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_sweep_under_the_scripts_that_stalled(name, script):
    optset, sched = STALL_SCRIPTS[script]
    after, steps, st = judge(emu_solver, name, emu_options(name, optset), sched, cap=slice_cap(name, optset))
    print(name, script, "slices after the final act", after, "of", slice_cap(name, optset))


@pytest.mark.parametrize("optset", ["default", "no-rebalance"])
def test_emulated_workers_move_from_130_literals_to_none_and_back(optset):
    judge(emu_solver, LONG, emu_options(LONG, optset), long_to_empty_and_back(LONG), cap=slice_cap(LONG, optset))


@pytest.mark.parametrize("seed", SEEDS[:2])
def test_emulated_sweep_in_the_other_variable_order(seed):
    sched = seeded_schedule(seed, CASES[VAR_ORDER_CASE][8])
    judge(emu_solver, VAR_ORDER_CASE, emu_options(VAR_ORDER_CASE, "default", var_order=1), sched, cap=slice_cap(VAR_ORDER_CASE, "default"))


@pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)
@pytest.mark.parametrize("name", MATRIX_CASES)
def test_emulated_sweep_in_every_build(name, one_per_simd, lds_val):
    opts = dict(emu_options(name, "default"), one_per_simd=one_per_simd, lds_val=lds_val)
    sched = long_to_empty_and_back(name) if name == LONG else seeded_schedule(SEEDS[0], CASES[name][8])
    judge(emu_solver, name, opts, sched, cap=slice_cap(name, "default"))


def test_emulated_batch_that_stops_at_the_first_verdict():
    res = stop_at_first(lambda **kw: emu_solver(deterministic=1, **kw))
    assert any(r.value == 0 for r in res)          # (ten conflicts a slice: the first verdicts fall before the last ones)
