"""The C ABI's contract at its edges, on the CPU through the wavefront emulator build of the solver (tests/emu): which
return code and which mi355sat_last_error text every refused call gets, what a refused call still does (assumptions
consumed, a core's length reported), that the timed entry points add to stats.solve_seconds, what core minimisation
leaves in stats, and the calls after which a warm incremental solve has to start cold.

One 3-variable formula throughout, (1 | 2) & (-1 | 3) & (-2 | 3): satisfiable, 3 is implied, UNSAT under [-3] and under
[-1, -2], where both assumptions are needed."""
import ctypes

import numpy as np
import pytest

from helpers import emu_lib
from timberborn_support_solver_amd import ColdReason, Mi355Sat, SolverError, SolverResult
from timberborn_support_solver_amd.solver import Mi355SatCoreMinInfo

ERR_OOM, ERR_HIP, ERR_STATE, ERR_ARG = -1, -2, -3, -4
CLAUSES = [[1, 2], [-1, 3], [-2, 3]]


def solver(formula=True, **kw):
    kw.setdefault("workers", 3)
    kw.setdefault("slice_conflicts", 100)
    s = Mi355Sat(_lib_override=emu_lib(), **kw)
    if formula:
        for c in CLAUSES:
            s.add_clause(c)
    return s


def err(s):
    return (s._L.mi355sat_last_error(s._h) or b"").decode()


def refused(s, code, text, fn, *args):
    """fn(*args) raises SolverError with that MI355SAT_ERR_* code; text (unless None) is what last_error says then."""
    with pytest.raises(SolverError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, str(e.value))
    if text is not None:
        assert err(s) == text


def i32(xs):
    return np.asarray(xs, dtype=np.int32)


def u64(xs):
    return np.asarray(xs, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data


def test_add_cnf_refuses_malformed_input_with_its_message():
    s = solver(formula=False)
    L, h = s._L, s._h
    lits = i32([1, 2, -1, 3])
    assert L.mi355sat_add_cnf(h, ptr(lits), ptr(u64([0, 2, 1])), 2) == ERR_ARG and err(s) == "offsets not monotone"
    lits0 = i32([1, 0, 3])
    assert L.mi355sat_add_cnf(h, ptr(lits0), ptr(u64([0, 3])), 1) == ERR_ARG and err(s) == "literal 0 inside a clause"
    big = i32([1, 2 ** 31 - 1])
    assert L.mi355sat_add_cnf(h, ptr(big), ptr(u64([0, 2])), 1) == ERR_ARG and err(s) == "variable index too large"
    assert L.mi355sat_add_cnf(h, ptr(lits), ptr(u64([0, 2, 4])), 2) == 0
    s.close()


def test_solve_inside_an_unterminated_clause_is_refused_and_consumes_the_assumptions():
    s = solver()
    assert s._L.mi355sat_add(s._h, 1) == 0          # clause [1 ... not terminated
    s.assume(-3)
    refused(s, ERR_STATE, "solve() called inside an unterminated clause", s.solve)
    assert s._L.mi355sat_add(s._h, 0) == 0
    assert s.solve() == SolverResult.Sat            # (UNSAT had -3 still been assumed)
    assert s.lit_val(3) == 3 and s.lit_val(1) == 1
    s.close()


NO_CORE = "no core: the last solve() did not return UNSAT"
NO_FAILED = "no failed assumptions: the last solve() did not return UNSAT"
NO_MIN = "no core to minimise: the last solve() did not return UNSAT"


def assert_no_core(s):
    refused(s, ERR_STATE, NO_CORE, s.core)
    refused(s, ERR_STATE, NO_FAILED, s.failed, -3)
    refused(s, ERR_STATE, NO_MIN, s.minimize_core)


def test_core_calls_need_an_unsat_answer_and_an_add_leaves_it():
    s = solver()
    assert_no_core(s)
    assert s.solve() == SolverResult.Sat
    assert_no_core(s)
    assert s.solve([-3]) == SolverResult.Unsat
    assert s.core() == [-3] and s.failed(-3) and not s.failed(3)
    s.add_clause([1, 2, 3])
    assert_no_core(s)
    s.close()


def test_core_buffer_one_too_small_reports_the_length():
    s = solver()
    assert s.solve([-1, -2]) == SolverResult.Unsat
    out, n = i32([0, 0]), ctypes.c_uint64(0)
    assert s._L.mi355sat_core(s._h, ptr(out), 1, ctypes.byref(n)) == ERR_ARG
    assert n.value == 2 and err(s) == "core buffer too small" and list(out) == [0, 0]
    assert s._L.mi355sat_core(s._h, ptr(out), 2, ctypes.byref(n)) == 0 and list(out) == [-1, -2]
    s.close()


NO_CORE_OF = "no core: instance out of range or not UNSAT in the last solve_batch()"
NO_MIN_OF = "no core to minimise: instance out of range or not UNSAT in the last solve_batch()"


def test_core_of_tells_no_batch_from_out_of_range_from_not_unsat():
    s = solver()
    refused(s, ERR_STATE, NO_CORE_OF, s.core_of, 0)
    refused(s, ERR_STATE, NO_MIN_OF, s.minimize_core_of, 0)
    refused(s, ERR_STATE, NO_CORE_OF, s.core_of, 5)            # before any batch nothing is "out of range"
    assert s.solve_batch([[-3], [3]]) == [SolverResult.Unsat, SolverResult.Sat]
    refused(s, ERR_ARG, NO_CORE_OF, s.core_of, 2)
    refused(s, ERR_ARG, NO_MIN_OF, s.minimize_core_of, 2)
    refused(s, ERR_STATE, NO_CORE_OF, s.core_of, 1)
    refused(s, ERR_STATE, NO_MIN_OF, s.minimize_core_of, 1)
    assert s.core_of(0) == [-3]
    assert s.minimize_core_of(0)["minimal"] == 1 and s.core_of(0) == [-3]
    s.close()


def test_models_need_a_sat_answer():
    s = solver()
    assert s.solve_batch([[-3], [3]]) == [SolverResult.Unsat, SolverResult.Sat]
    refused(s, ERR_STATE, "no model for that instance", s.solution_of, 0)
    refused(s, ERR_STATE, "no model for that instance", s.solution_of, 2)
    assert s.solution_of(1)[2] == 1
    assert s.solve([-3]) == SolverResult.Unsat
    refused(s, ERR_STATE, "no model (last result was not SAT)", s.full_solution)
    s.close()


def test_sweep_calls_need_a_sweep_and_check_their_arguments():
    s = solver()
    L, h = s._L, s._h
    one, w, m = u64([0]), np.asarray([1.0], dtype=np.float64), np.zeros(3, dtype=np.int8)
    assert L.mi355sat_sweep_step(h, None, None) == ERR_STATE
    assert L.mi355sat_sweep_drop(h, ptr(one), 1) == ERR_STATE
    assert L.mi355sat_sweep_reopen(h, ptr(one), 1) == ERR_STATE
    assert L.mi355sat_sweep_set_weights(h, ptr(w), 1) == ERR_STATE
    assert L.mi355sat_sweep_model_of(h, 0, ptr(m), 3) == ERR_STATE
    assert L.mi355sat_sweep_end(h) == ERR_STATE
    s.sweep_begin([[-3], [3]])
    refused(s, ERR_ARG, "instance out of range", s.sweep_drop, [2])
    refused(s, ERR_ARG, "instance out of range", s.sweep_reopen, [2])
    refused(s, ERR_ARG, "one weight per instance", s.sweep_set_weights, [1.0])
    refused(s, ERR_ARG, "weights must be >= 0", s.sweep_set_weights, [1.0, -1.0])
    refused(s, ERR_STATE, "no model for that instance", s.sweep_solution_of, 1)      # no verdict yet
    res, n = s.sweep_step()
    for _ in range(20):
        if n == 2:
            break
        res, n = s.sweep_step()
    assert res == [SolverResult.Unsat, SolverResult.Sat]
    refused(s, ERR_STATE, "no model for that instance", s.sweep_solution_of, 0)
    refused(s, ERR_STATE, "no model for that instance", s.sweep_solution_of, 2)
    assert s.sweep_solution_of(1)[2] == 1
    s.sweep_end()
    assert L.mi355sat_sweep_end(h) == ERR_STATE
    assert s.solution_of(1)[2] == 1                  # sweep_end keeps the models for model_of
    s.close()


def test_solve_seconds_grows_across_every_timed_entry_point():
    s = solver()
    t = [s.stats()["solve_seconds"]]

    def grew():
        t.append(s.stats()["solve_seconds"])
        return t[-1] > t[-2]

    assert t[0] == 0
    assert s.solve() == SolverResult.Sat and grew()
    assert s.solve_batch([[-3], [3]]) == [SolverResult.Unsat, SolverResult.Sat] and grew()
    confl, _, _ = s.propagate_batch([[-1, -2], [1]])
    assert list(confl) == [1, 0] and grew()
    s.sweep_begin([[-3], [3]])
    s.sweep_step()
    assert grew()
    s.sweep_end()
    assert s.solve([-1, -2]) == SolverResult.Unsat and grew()
    assert s.minimize_core()["rounds"] >= 1 and grew()
    s.close()


def test_minimize_core_keeps_the_stats_of_the_solve_before_it():
    s = solver(workers=3)
    assert s.solve([-1, -2]) == SolverResult.Unsat
    before = s.stats()
    assert before["workers"] == 3
    info = s.minimize_core()        # two candidates of one literal each: an upload of its own, with two workers
    assert info["rounds"] >= 1 and info["candidates"] == 2 and info["minimal"] == 1 and s.core() == [-1, -2]
    after = s.stats()
    for k in ("workers", "simp_units", "simp_equivalences", "simp_clauses_removed", "simp_eliminated", "n_sat", "n_unsat",
              "n_terminated", "n_clauses", "max_var"):
        assert after[k] == before[k], k
    assert after["kernel_launches"] > before["kernel_launches"] and after["solve_seconds"] > before["solve_seconds"]
    s.close()


def _propagate(s):
    s.propagate_batch([[1]])


def _minimize(s):
    assert s.minimize_core()["rounds"] >= 1


def _set_schedule(s):
    s.debug_set_schedule(0, 0, 0)


@pytest.mark.parametrize("between, reason", [(None, None), (_propagate, ColdReason.OTHER_SEARCH), (_minimize, ColdReason.OTHER_SEARCH),
                                             (_set_schedule, ColdReason.FIRST)],
                         ids=["nothing", "propagate_batch", "minimize_core", "debug_set_schedule"])
def test_what_makes_the_next_warm_solve_start_cold(between, reason):
    s = solver()
    s.set_incremental(True)
    assert s.solve([-1, -2]) == SolverResult.Unsat and s.core() == [-1, -2]
    d = s.debug_incremental()
    assert (d["cold_solves"], d["warm_solves"], d["last_cold_reason"]) == (1, 0, ColdReason.FIRST)
    if between:
        between(s)
    assert s.solve([-3]) == SolverResult.Unsat and s.core() == [-3]
    d = s.debug_incremental()
    if between is None:
        assert (d["cold_solves"], d["warm_solves"]) == (1, 1)
    else:
        assert (d["cold_solves"], d["warm_solves"], d["last_cold_reason"]) == (2, 0, reason)
    assert s.solve() == SolverResult.Sat and s.debug_incremental()["warm_solves"] == (2 if between is None else 1)
    s.close()
