"""tests/capacity_cases.py on the wave emulator (tests/emu), and the warm-start fallbacks that a small store decides."""
import pytest

import capacity_cases as cc
from helpers import emu_lib
from test_incremental import Checked
from timberborn_support_solver_amd import ColdReason, Mi355Sat, SolverError, SolverResult

SEEDS = pytest.mark.parametrize("seed", cc.SEEDS)


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **dict(cc.EMU_OPTS, **kw))


# ---- the hook itself --------------------------------------------------------------------------------------------------------
def test_capacity_hook_checks_its_arguments_and_reports_the_layout():
    s = emu_solver()
    with pytest.raises(SolverError) as e:
        s.debug_capacities()                         # before the first cold start
    assert e.value.code == cc.ERR_STATE
    for bad in (dict(learnt_cap=3), dict(learnt_cap=(1 << 17) + 1), dict(learnt_lit_cap=63), dict(learnt_lit_cap=(2 << 20) + 1),
                dict(pool_slack=(1 << 30) + 1), dict(proof_cap=7), dict(proof_cap=(1 << 23) + 1)):
        with pytest.raises(SolverError) as e:
            s.debug_set_capacities(**bad)
        assert e.value.code == -4, bad
    cnf, want = cc.formula(1)
    cc.load(s, cnf)
    assert s.solve().value == want
    rule = s.debug_capacities()                      # the sizing rules, as DESIGN.md states them
    assert rule["learnt_cap"] == 32768 and rule["learnt_lit_cap"] == 1 << 19 and rule["proof_cap"] == 0
    assert rule["pool_cap"] == (3 * (0 + 32768) + 4 * 80) * 3 // 2 + 65536          # (3-SAT: no clause of four literals)
    assert rule["pressure_reduces"] == rule["pool_rebuilds"] == rule["imports_dropped_full"] == 0
    s.debug_set_capacities(learnt_cap=4, learnt_lit_cap=64, pool_slack=1, proof_cap=8)     # the floors are accepted
    s.debug_set_capacities(64, 0, 400, 0)
    assert s.solve().value == want
    info = s.debug_capacities()
    assert (info["learnt_cap"], info["learnt_lit_cap"], info["pool_cap"]) == (64, 1 << 19, info["pool_initial"] + 400)
    s.debug_set_capacities(0, 0, 0, 0)
    assert s.solve().value == want
    assert {k: v for k, v in s.debug_capacities().items() if k.endswith("cap")} == {k: v for k, v in rule.items() if k.endswith("cap")}
    s.close()


# ---- (a) learnt slots, (b) literal store, (c) pool-low collection ------------------------------------------------------------
@SEEDS
def test_emulated_search_with_64_learnt_slots(tmp_path, seed):
    st, info, n_del = cc.check_case(emu_solver, "emu", "a", cc.SLOTS, seed, tmp_path)
    if seed in cc.UNSAT_SEEDS:                       # every one of them takes some worker far past 57 conflicts here
        cc.assert_pressure(st, info)
        assert n_del > 0                             # ... and its proof carries the deletion lines of those reductions


@pytest.mark.parametrize("seed", [0, 1])
def test_emulated_search_with_64_learnt_slots_assignment_in_the_slab(tmp_path, seed):
    st, info, n_del = cc.check_case(emu_solver, "emu-slab", "a", cc.SLOTS, seed, tmp_path, build=(0, -1))
    if seed in cc.UNSAT_SEEDS:
        cc.assert_pressure(st, info)


@pytest.mark.parametrize("seed", range(6))
def test_emulated_search_with_1024_learnt_literal_words(tmp_path, seed):
    st, info, n_del = cc.check_case(emu_solver, "emu", "b", cc.LITERALS, seed, tmp_path)
    if cc.pressure_must_show(st, info):
        cc.assert_pressure(st, info)


def test_emulated_literal_store_pressure_on_most_unsat_seeds(tmp_path):
    """Seeds 0, 2, 3, 5 of the case above (taken from there when it ran): the 128 slots never fill at 1024 literal words
    (a learnt clause of these formulas has 8 to 15 literals), so these reductions are the literal store's."""
    cc.check_pressure_on_most_unsat_seeds(emu_solver, "emu", "b", cc.LITERALS, tmp_path)


@SEEDS
def test_emulated_search_with_a_watch_pool_400_entries_above_its_lists(tmp_path, seed):
    st, info, n_del = cc.check_case(emu_solver, "emu", "c", cc.POOL_LOW, seed, tmp_path)
    if seed in cc.UNSAT_SEEDS:
        cc.assert_pressure(st, info)


def test_emulated_pool_low_collection_ran_somewhere_in_the_set(tmp_path):
    """Summed over the eight runs of the case above (taken from there when they ran, else run here)."""
    cc.check_pool_rebuilds_over_the_set(emu_solver, "emu", tmp_path)


def test_emulated_pool_low_collection_under_assumptions(tmp_path):
    """An UNSAT and a SAT seed; the collection ran in one of them at least (274 and 83 conflicts: the second may be done
    before its pool is three quarters full)."""
    assert sum(cc.check_pool_low_under_assumptions(emu_solver, seed, tmp_path) for seed in (0, 1)) > 0


# ---- (d) exhaustion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_emulated_watch_pool_exhaustion_is_a_clean_error(tmp_path, seed):
    cc.check_exhaustion(emu_solver, seed, cc.POOL_OUT, cc.POOL_TEXT, tmp_path, reduce_first=40, reduce_inc=10)


@pytest.mark.parametrize("seed", [0, 1])
def test_emulated_learnt_store_exhaustion_is_a_clean_error(tmp_path, seed):
    cc.check_exhaustion(emu_solver, seed, cc.SLOTS_OUT, cc.LEARNT_TEXT, tmp_path)


# ---- (e) imports ------------------------------------------------------------------------------------------------------------
def test_emulated_imports_never_fail_a_solve():
    cc.check_imports_never_fail_a_solve(emu_solver, *cc.IMPORT_CASE, **cc.IMPORT_OPTS)


# ---- (f) the proof log ------------------------------------------------------------------------------------------------------
def test_emulated_small_proof_log_drops_deletion_lines_only(tmp_path):
    cc.check_proof_log_drops_deletions(emu_solver, tmp_path)


def test_emulated_proof_log_that_loses_a_lemma_fails_the_solve(tmp_path):
    cc.check_proof_log(emu_solver, 0, cc.PROOF_CAP_TOO_SMALL, tmp_path, True, **cc.PROOF_OPTS)


# ---- (g) warm-start fallbacks -------------------------------------------------------------------------------------------------
def checked(n_vars, caps=None):
    return cc.checked(Checked, emu_solver, n_vars, caps)


def test_emulated_257_more_assumptions_start_cold():
    cc.check_cold_for_assumption_room(checked)


def test_emulated_seventeen_warm_clauses_at_64_slots_start_cold():
    cc.check_cold_for_pinned_share(checked)


def test_emulated_full_device_at_a_warm_attach_starts_that_solve_cold():
    cc.check_cold_for_a_full_device(checked)
