"""The C ABI's contract at its edges, on the CPU through the wavefront emulator build of the solver (tests/emu): which
return code and which mi355sat_last_error text every refused call gets, what a refused call still does (assumptions
consumed, a core's length reported), that the timed entry points add to stats.solve_seconds, what core minimisation
leaves in stats, the calls after which a warm incremental solve has to start cold, and what the proof check / trim entries
refuse, with which text, and whether an earlier trim's result survives the refusal.

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


# ---- proof check and trim (mi355sat_check_proof / _trim_proof and their _file variants) ----------------------------------
# Clause (3) is RUP from the formula with an empty proof: trim_proof([], target=(3,)) is the smallest valid trim, its core
# all three clauses, no lemma needed.
DEL = -2 ** 31
PROOF_ENTRIES = ["check_proof", "check_proof_file", "trim_proof", "trim_proof_file"]
NO_TRIM = "no trimmed proof: the last call was not a mi355sat_trim_proof() that found the proof valid"


def drup_text(words):
    return "".join("d " if w == DEL else ("0\n" if w == 0 else f"{w} ") for w in words)


def proof_entry(s, entry, tmp_path):
    """(call(words, target=()), the entry's name in its messages); a _file variant gets the words as DRUP text."""
    fn, name = getattr(s, entry), entry.replace("_file", "")
    if not entry.endswith("_file"):
        return (lambda words, target=(): fn(words, target=target)), name

    def call(words, target=()):
        path = tmp_path / "proof.drup"
        path.write_text(drup_text(words))
        return fn(path, target=target)
    return call, name


def valid_trim(s):
    res = s.trim_proof([], target=(3,))
    assert res["check"]["valid"] == 1 and res["core"] == [0, 1, 2] and res["lemmas"] == []
    assert s.trim_core() == [0, 1, 2]


def trim_getters_refuse(s, tmp_path):
    refused(s, ERR_STATE, NO_TRIM, s.trim_core)
    refused(s, ERR_STATE, NO_TRIM, s.trim_lemmas)
    refused(s, ERR_STATE, NO_TRIM, s.trim_write_drup, tmp_path / "t.drup")
    refused(s, ERR_STATE, NO_TRIM, s.trim_write_lrat, tmp_path / "t.lrat")
    assert not (tmp_path / "t.drup").exists() and not (tmp_path / "t.lrat").exists()


def test_proof_entries_refuse_null_arguments_and_unknown_flags_and_leave_the_trim_result(tmp_path):
    from timberborn_support_solver_amd.solver import Mi355SatProofInfo, Mi355SatTrimInfo
    s = solver()
    L, h = s._L, s._h
    valid_trim(s)
    pi, ti = Mi355SatProofInfo(), Mi355SatTrimInfo()
    one, path = i32([3]), str(tmp_path / "proof.drup").encode()
    (tmp_path / "proof.drup").write_text("")
    for args in [(None, None, 0, ptr(one), 1, 0, pi), (h, None, 0, ptr(one), 1, 0, None), (h, None, 1, ptr(one), 1, 0, pi),
                 (h, None, 0, None, 1, 0, pi)]:
        assert L.mi355sat_check_proof(*args) == ERR_ARG, args
    for args in [(None, path, ptr(one), 1, 0, pi), (h, path, ptr(one), 1, 0, None), (h, None, ptr(one), 1, 0, pi),
                 (h, path, None, 1, 0, pi)]:
        assert L.mi355sat_check_proof_file(*args) == ERR_ARG, args
    for args in [(None, None, 0, ptr(one), 1, 0, 0, ti), (h, None, 0, ptr(one), 1, 0, 0, None), (h, None, 1, ptr(one), 1, 0, 0, ti),
                 (h, None, 0, None, 1, 0, 0, ti), (h, None, 0, ptr(one), 1, 0, 2, ti), (h, None, 0, ptr(one), 1, 0, 3, ti)]:
        assert L.mi355sat_trim_proof(*args) == ERR_ARG, args
    for args in [(None, path, ptr(one), 1, 0, 0, ti), (h, path, ptr(one), 1, 0, 0, None), (h, None, ptr(one), 1, 0, 0, ti),
                 (h, path, None, 1, 0, 0, ti), (h, path, ptr(one), 1, 0, 2, ti)]:
        assert L.mi355sat_trim_proof_file(*args) == ERR_ARG, args
    assert s.trim_core() == [0, 1, 2]
    s.close()


@pytest.mark.parametrize("entry", PROOF_ENTRIES)
def test_proof_entry_refusals_have_their_texts_and_leave_the_trim_result(entry, tmp_path):
    s = solver()
    call, name = proof_entry(s, entry, tmp_path)
    valid_trim(s)
    # a proof that does not parse
    refused(s, ERR_ARG, "proof: a variable the handle does not have", call, [4, 0], (3,))
    assert s.trim_core() == [0, 1, 2]
    refused(s, ERR_ARG, "proof: the last clause is not terminated", call, [3, 0, 1, 2], (3,))
    assert s.trim_core() == [0, 1, 2]
    if not entry.endswith("_file"):                 # (in a file a "d" inside a clause is no number: malformed, below)
        refused(s, ERR_ARG, "proof: a deletion marker inside a clause", call, [1, DEL, 2, 0], (3,))
        assert s.trim_core() == [0, 1, 2]
    # a bad target: refused after the earlier result was dropped
    refused(s, ERR_ARG, "proof target: literal 0 inside a clause", call, [], (1, 0, 2))
    trim_getters_refuse(s, tmp_path)
    valid_trim(s)
    refused(s, ERR_ARG, "proof target: literal 0 inside a clause", call, [], (1, DEL))
    trim_getters_refuse(s, tmp_path)
    valid_trim(s)
    refused(s, ERR_ARG, "proof target: a variable the handle does not have", call, [3, 0], (4,))
    trim_getters_refuse(s, tmp_path)
    # during a sweep (sweep_begin dropped the result already)
    valid_trim(s)
    s.sweep_begin([[-3], [3]])
    refused(s, ERR_STATE, f"{name}() called during a sweep", call, [], (3,))
    trim_getters_refuse(s, tmp_path)
    s.sweep_end()
    valid_trim(s)
    # inside an unterminated clause
    assert s._L.mi355sat_add(s._h, 1) == 0
    refused(s, ERR_STATE, f"{name}() called inside an unterminated clause", call, [], (3,))
    assert s.trim_core() == [0, 1, 2]
    assert s._L.mi355sat_add(s._h, 0) == 0          # (the clause added drops the result)
    trim_getters_refuse(s, tmp_path)
    s.close()


@pytest.mark.parametrize("entry", ["check_proof_file", "trim_proof_file"])
def test_proof_file_entries_refuse_a_missing_and_a_malformed_file(entry, tmp_path):
    s = solver()
    valid_trim(s)
    fn = getattr(s, entry)
    missing = tmp_path / "none.drup"
    refused(s, ERR_ARG, "cannot open proof file " + str(missing), fn, missing, (3,))
    for text in ["1 x 0\n", "2147483648 0\n", "-2147483648 0\n", "1 d 2 0\n"]:
        bad = tmp_path / "bad.drup"
        bad.write_text(text)
        refused(s, ERR_ARG, "malformed proof file " + str(bad), fn, bad, (3,))
        assert s.trim_core() == [0, 1, 2]
    (tmp_path / "ok.drup").write_text("d 1 2 0\n3 0\n")
    res = fn(tmp_path / "ok.drup", (3,))
    res = res.get("check", res)
    assert res["valid"] == 1 and res["n_lemmas"] == 1 and res["n_deletions_ignored"] == 1
    s.close()


def test_trim_readers_and_writers_refuse_with_their_texts(tmp_path):
    s = solver()
    trim_getters_refuse(s, tmp_path)                # before any trim
    assert s.trim_proof([1, 0], target=(3,))["check"]["valid"] == 0        # (1) is not RUP: no result either
    trim_getters_refuse(s, tmp_path)
    valid_trim(s)
    buf, n = u64([7, 7, 7]), ctypes.c_uint64(0)
    assert s._L.mi355sat_trim_core(s._h, ptr(buf), 2, ctypes.byref(n)) == ERR_ARG
    assert err(s) == "index buffer too small" and n.value == 3 and list(buf) == [7, 7, 7]
    refused(s, ERR_STATE, "trim_write_lrat(): the proof was trimmed without MI355SAT_TRIM_HINTS", s.trim_write_lrat, tmp_path / "t.lrat")
    assert not (tmp_path / "t.lrat").exists()
    for write in (s.trim_write_drup, s.trim_write_lrat):
        unwritable = tmp_path / "no_such_dir" / "t.out"
        if write == s.trim_write_lrat:
            assert s.trim_proof([], target=(3,), hints=True)["core"] == [0, 1, 2]
        refused(s, ERR_ARG, "cannot open " + str(unwritable), write, unwritable)
        assert not unwritable.exists() and s.trim_core() == [0, 1, 2]
    s.trim_write_lrat(tmp_path / "t.lrat")
    line = (tmp_path / "t.lrat").read_text().split()           # one line, the target's: id 4, (3), the three clauses as hints
    assert line[:3] == ["4", "3", "0"] and sorted(line[3:-1]) == ["1", "2", "3"] and line[-1] == "0"
    s.close()


def test_check_proof_and_trim_proof_are_timed_and_count_their_launches():
    s = solver()
    for call in (lambda: s.check_proof([], target=(3,)), lambda: s.trim_proof([], target=(3,))["check"]):
        before = s.stats()
        info = call()
        after = s.stats()
        assert info["valid"] == 1 and info["launches"] >= 1
        assert after["solve_seconds"] > before["solve_seconds"]
        assert after["kernel_launches"] == before["kernel_launches"] + info["launches"]
    s.close()
