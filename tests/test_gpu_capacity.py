"""tests/capacity_cases.py on the MI355X (run with -m gpu): 64 workers in the deterministic mode, on all six builds of the
search kernel (which build ran is asserted through mi355sat_debug_last_search_build); every solve under a deadline."""
import threading

import pytest

import capacity_cases as cc
from test_incremental import Checked
from timberborn_support_solver_amd import Mi355Sat

pytestmark = pytest.mark.gpu

BUILD_SEEDS = pytest.mark.parametrize("build,seed", cc.BUILD_SEEDS, ids=cc.BUILD_SEED_IDS)


def gpu_solver(**kw):
    return Mi355Sat(**dict(cc.GPU_OPTS, **kw))


def within(s, assumptions=()):
    """solve() with a wall-clock limit: the interrupt turns a hang into a failed assertion."""
    tm = threading.Timer(30.0, s.interrupter().interrupt)
    tm.start()
    try:
        return s.solve(assumptions)
    finally:
        tm.cancel()


def step_within(s):
    tm = threading.Timer(30.0, s.interrupter().interrupt)
    tm.start()
    try:
        return s.sweep_step()
    finally:
        tm.cancel()


# ---- (a) learnt slots, (b) literal store, (c) pool-low collection ------------------------------------------------------------
@BUILD_SEEDS
def test_search_with_64_learnt_slots(tmp_path, build, seed):
    st, info, n_del = cc.check_case(gpu_solver, build, "a", cc.SLOTS, seed, tmp_path, build=build, solve=within)
    if cc.pressure_must_show(st, info):
        cc.assert_pressure(st, info)


def test_slot_pressure_on_most_unsat_seeds(tmp_path):
    """On the one-wave build (taken from the case above where it ran that seed on that build)."""
    cc.check_pressure_on_most_unsat_seeds(gpu_solver, cc.BUILDS[0], "a", cc.SLOTS, tmp_path, build=cc.BUILDS[0], solve=within)


@BUILD_SEEDS
def test_search_with_1024_learnt_literal_words(tmp_path, build, seed):
    st, info, n_del = cc.check_case(gpu_solver, build, "b", cc.LITERALS, seed, tmp_path, build=build, solve=within)
    if cc.pressure_must_show(st, info):
        cc.assert_pressure(st, info)


def test_literal_store_pressure_on_most_unsat_seeds(tmp_path):
    cc.check_pressure_on_most_unsat_seeds(gpu_solver, cc.BUILDS[5], "b", cc.LITERALS, tmp_path, build=cc.BUILDS[5], solve=within)


@BUILD_SEEDS
def test_search_with_a_watch_pool_400_entries_above_its_lists(tmp_path, build, seed):
    """400 entries is what the emulator's three workers were tried with; it is kept here.  What a worker needs at most is
    the dense layout of its lists with every slot in use, 3 * (clauses + learnt_cap) + 4 * n_vars = 3 * (0 + 64) + 4 * 80 =
    512 entries (3-SAT: no original clause is watched), 192 above the 320 of the empty lists - plus the holes that grown
    lists leave until the next collection, which is what the 3/4 rule bounds."""
    st, info, n_del = cc.check_case(gpu_solver, build, "c", cc.POOL_LOW, seed, tmp_path, build=build, solve=within)


def test_pool_low_collection_ran_on_every_build(tmp_path):
    for i, build in enumerate(cc.BUILDS):
        seeds = [seed for b, seed in cc.BUILD_SEEDS if b == build]
        cc.check_pool_rebuilds_over_the_set(gpu_solver, build, tmp_path, seeds=seeds, build=build, solve=within)


def test_pool_low_collection_under_assumptions(tmp_path):
    assert sum(cc.check_pool_low_under_assumptions(gpu_solver, seed, tmp_path, solve=within) for seed in (0, 1)) > 0


# ---- (d) exhaustion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [cc.BUILDS[0], cc.BUILDS[5]], ids=[cc.BUILD_IDS[0], cc.BUILD_IDS[5]])
@pytest.mark.parametrize("seed", [0, 1])
def test_watch_pool_exhaustion_is_a_clean_error(tmp_path, seed, build):
    cc.check_exhaustion(gpu_solver, seed, cc.POOL_OUT, cc.POOL_TEXT, tmp_path, solve=within, reduce_first=40, reduce_inc=10,
                        one_per_simd=build[0], lds_val=build[1])


@pytest.mark.parametrize("build", [cc.BUILDS[0], cc.BUILDS[5]], ids=[cc.BUILD_IDS[0], cc.BUILD_IDS[5]])
@pytest.mark.parametrize("seed", [0, 1])
def test_learnt_store_exhaustion_is_a_clean_error(tmp_path, seed, build):
    cc.check_exhaustion(gpu_solver, seed, cc.SLOTS_OUT, cc.LEARNT_TEXT, tmp_path, solve=within, one_per_simd=build[0], lds_val=build[1])


# ---- (e) imports, (f) the proof log, (g) a full device at a warm attach -------------------------------------------------------
def test_imports_never_fail_a_solve(tmp_path):
    cc.check_imports_never_fail_a_solve(gpu_solver, *cc.IMPORT_CASE, step=step_within, **cc.IMPORT_OPTS)


def test_a_small_proof_log_drops_deletion_lines_only(tmp_path):
    cc.check_proof_log_drops_deletions(gpu_solver, tmp_path, solve=within)


def test_a_proof_log_that_loses_a_lemma_fails_the_solve(tmp_path):
    cc.check_proof_log(gpu_solver, 0, cc.PROOF_CAP_TOO_SMALL, tmp_path, True, solve=within)


def test_a_full_device_at_a_warm_attach_starts_that_solve_cold():
    cc.check_cold_for_a_full_device(lambda n_vars, caps: cc.checked(Checked, gpu_solver, n_vars, caps))
