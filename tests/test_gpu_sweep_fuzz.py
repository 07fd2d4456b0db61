"""Differential tests of the stepwise sweep's schedule calls on the MI355X (run with -m gpu): the emulator's cases
(tests/test_emu_sweep_fuzz.py) with a fleet of 64 in all six builds of the search kernel - deterministic runs under the
emulator's slice caps (a deterministic run is a function of its inputs on both targets, and 64 workers need no more slices
than the emulator's 6 .. 20) - and one timed pass per case with the default options; judged by the oracle alone after every
step, tests/sweep_cases.py says how.  Every sweep runs under a deadline: running into it leaves instances undecided, which
fails the comparison with the oracle."""
import pytest

from fuzz_cases import BUILD_IDS, BUILD_LIST
from simp_cases import within
from sweep_cases import (CASES, LONG, OPTSETS, SEEDS, STALL_SCRIPTS, VAR_ORDER_CASE, judge, long_to_empty_and_back, options,
                         seeded_schedule, slice_cap, stop_at_first)
from timberborn_support_solver_amd import Mi355Sat

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)
LIMIT_S = 20.0
# the builds cover the two places of the assignment: the option sets that only choose one are left to the emulator
GPU_OPTSETS = [o for o in OPTSETS if o not in ("lds", "slab")]


def gpu_options(name, optset, one_per_simd, lds_val, **more):
    """The option set as on the emulator, with capacity_cases.GPU_OPTS' fleet: 64 workers, all from the first slice."""
    return dict(options(name, optset, **more), workers=64, ramp=-1, deterministic=1, one_per_simd=one_per_simd, lds_val=lds_val)


@BUILDS
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("optset", GPU_OPTSETS)
@pytest.mark.parametrize("name", list(CASES))
def test_sweep_under_a_seeded_schedule_in_every_build(name, optset, seed, one_per_simd, lds_val):
    sched = seeded_schedule(seed, CASES[name][8])
    after, steps, st = judge(Mi355Sat, name, gpu_options(name, optset, one_per_simd, lds_val), sched, cap=slice_cap(name, optset),
                             limit_s=LIMIT_S)
    print(name, optset, seed, "slices after the final act", after, "of", slice_cap(name, optset), "in all", steps, "conflicts", st["conflicts"])


@BUILDS
@pytest.mark.parametrize("script", list(STALL_SCRIPTS))
@pytest.mark.parametrize("name", list(CASES))
def test_sweep_under_the_scripts_that_stalled_in_every_build(name, script, one_per_simd, lds_val):
    optset, sched = STALL_SCRIPTS[script]
    judge(Mi355Sat, name, gpu_options(name, optset, one_per_simd, lds_val), sched, cap=slice_cap(name, optset), limit_s=LIMIT_S)


@BUILDS
@pytest.mark.parametrize("optset", ["default", "no-rebalance"])
def test_workers_move_from_130_literals_to_none_and_back_in_every_build(optset, one_per_simd, lds_val):
    judge(Mi355Sat, LONG, gpu_options(LONG, optset, one_per_simd, lds_val), long_to_empty_and_back(LONG), cap=slice_cap(LONG, optset),
          limit_s=LIMIT_S)


def test_sweep_in_the_other_variable_order():
    sched = seeded_schedule(SEEDS[0], CASES[VAR_ORDER_CASE][8])
    judge(Mi355Sat, VAR_ORDER_CASE, gpu_options(VAR_ORDER_CASE, "default", 0, 0, var_order=1), sched,
          cap=slice_cap(VAR_ORDER_CASE, "default"), limit_s=LIMIT_S)


@pytest.mark.parametrize("name", list(CASES))
def test_timed_sweep_with_the_default_options(name):
    """Not deterministic: time-bounded slices, the default fleet and its ramp-up; no slice cap, the deadline alone."""
    sched = seeded_schedule(SEEDS[1], CASES[name][8])
    after, steps, st = judge(Mi355Sat, name, dict(simp=CASES[name][5]), sched, cap=None, limit_s=LIMIT_S)
    print(name, "timed: slices after the final act", after, "in all", steps, "conflicts", st["conflicts"], "workers", st["workers"])


def test_batch_that_stops_at_the_first_verdict():
    stop_at_first(Mi355Sat, run=lambda s, fn: within(LIMIT_S, s, fn))
