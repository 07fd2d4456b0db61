"""Formulas with planted structure for the differential tests of the simplification before search
(tests/test_emu_simp_fuzz.py, test_gpu_simp_fuzz.py), and their judge (test infrastructure).

tests/fuzz_cases.py runs every formula with simp = -1, so that the search kernel decides it; here the default path runs:
els_scc, device_probe (ms_probe_kernel), device_subsume (ms_subsume_kernel), with simp = 2 bve_eliminate / extend_model,
the substitution walk of map_assumptions, the freezing of assumption variables and ms_final_kernel's cores on a simplified
formula.  helpers.structured_cnf plants what these steps live on.

The judge is the oracle alone, never the product:
  a. plain solve: the oracle's verdict; a model that oracle.check_model accepts against the ORIGINAL clauses; a DRUP proof
     (simplification lemmas first) that oracle.check_rup accepts against the original formula; implied ring records;
  b. the simplified formula (Mi355Sat.debug_simplified): the oracle refutes original AND NOT(c) for every clause c the
     workers receive and every clause kept for an eliminated variable (soundness, every simp level); with simp = 0 an oracle
     loaded with the simplified formula refutes NOT(c) for every original clause c (completeness: a clause lost to a wrong
     subsumption, strengthening or substitution shows here, not only when a model happens to violate it).  With simp = 2 the
     simplified formula is not equivalent (only one side of an eliminated variable is kept): the models of a. and c. cover it;
  c. solve_batch under 24 seeded assumption sets over ALL variables - substituted, fixed and eliminable ones too; one empty,
     one with a repeated literal, one with a contradicting pair: the oracle's verdict per set, models that satisfy clauses
     and assumptions, cores that are subsequences of the assumptions as given and that the oracle refutes;
  d. the counters the table names are non-zero, nothing is eliminated unless simp = 2, and a formula its structure refutes
     is answered without a search launch.

The table was sized with the oracle and the emulator on the CPU: verdict and conflicts are the oracle's (asserted by
formula()), the counter sets are what the pipeline raised on the emulator with simp = 2 (simp_eliminated: only then)."""
import threading

import numpy as np

from helpers import Csr, assert_ring_records_are_implied, structured_cnf
from oracle import oracle as ora
from timberborn_support_solver_amd import SolverResult
from timberborn_support_solver_amd.dimacs import read_drup
from timberborn_support_solver_amd.solver import SolverError

N_SETS = 24
EQ, UN, RM, EL = "simp_equivalences", "simp_units", "simp_clauses_removed", "simp_eliminated"
COUNTERS = (EQ, UN, RM, EL)

MIXED = (2, 3, 4, 5, 6)
ALL = ("equiv", "failed", "subsume", "strengthen", "elim", "salt")

# name -> (seed, n_vars, n_clauses and lengths of the base, features, refute, workers, oracle verdict, oracle conflicts,
#          counters > 0)
# The single-feature cases name the counter their feature raised on the emulator; the 3-SAT bases at 4.4 .. 4.9 clauses per
# base variable are refuted by the search on the simplified formula (35 .. 95 conflicts of the product), the two last ones by
# their planted structure alone.
EMU_CASES = {
    "equiv-n48-s1": (1, 48, 90, MIXED, ("equiv",), None, 2, 10, 0, frozenset({EQ})),
    "failed-n48-s2": (2, 48, 90, MIXED, ("failed",), None, 2, 10, 3, frozenset({UN, EQ})),
    "subsume-n40-s3": (3, 40, 100, MIXED, ("subsume",), None, 2, 10, 0, frozenset({RM})),
    "strengthen-n45-s4": (4, 45, 110, MIXED, ("strengthen",), None, 2, 10, 2, frozenset({RM, UN})),
    "long-n110-s5": (5, 110, 100, MIXED, ("long", "subsume"), None, 2, 10, 0, frozenset({RM, EL})),
    "elim-n50-s6": (6, 50, 110, MIXED, ("elim",), None, 2, 10, 9, frozenset({EL, RM})),
    "salt-n40-s7": (7, 40, 110, MIXED, ("salt", "subsume"), None, 1, 10, 4, frozenset({RM})),
    "all-n110-s8": (8, 110, 170, MIXED, ALL, None, 2, 10, 25, frozenset(COUNTERS)),
    "equiv-elim-n80-s42": (42, 80, 225, (3,), ("equiv", "elim"), None, 2, 20, 44, frozenset({EQ, RM, EL})),
    "equiv-elim-n90-s43": (43, 90, 290, (3,), ("equiv", "elim"), None, 2, 20, 27, frozenset({EQ, RM, EL})),
    "strengthen-elim-n75-s45": (45, 75, 260, (3,), ("strengthen", "elim"), None, 2, 20, 33, frozenset({UN, RM, EL})),
    "scc-n50-s10": (10, 50, 120, MIXED, ("equiv", "subsume"), "scc", 2, 20, 2, frozenset()),
    "failed-both-n50-s11": (11, 50, 120, MIXED, ("failed", "strengthen"), "failed", 2, 20, 2, frozenset({UN})),
}
# the option matrix beyond (var_order 0, lds_val 1) runs on these: one case per step of the pipeline, one that is searched
MATRIX_CASES = ("equiv-n48-s1", "failed-n48-s2", "strengthen-n45-s4", "elim-n50-s6", "equiv-elim-n80-s42", "failed-both-n50-s11")
# up to 300 variables and 1300 clauses: probing with several hundred workers, ms_subsume_kernel in several blocks of 256
ALL_LONG = ALL + ("long",)
GPU_ONLY_CASES = {
    "all-long-n300-s71": (71, 300, 560, (2, 3, 3, 3, 4, 4, 5, 6), ALL_LONG, None, 8, 10, 21, frozenset(COUNTERS)),
    "all-long-n300-s74": (74, 300, 600, (3,), ALL_LONG, None, 8, 10, 490, frozenset(COUNTERS)),
    "all-long-n300-s63": (63, 300, 800, (3,), ALL_LONG, None, 8, 20, 393, frozenset(COUNTERS)),
    "all-n300-s66": (66, 300, 1000, (3,), ALL, None, 8, 10, 7319, frozenset(COUNTERS)),
    "all-n300-s67": (67, 300, 1120, (3,), ALL, None, 8, 20, 3916, frozenset(COUNTERS)),
}
GPU_CASES = dict(EMU_CASES, **GPU_ONLY_CASES)
# the counter a planted feature (helpers.STRUCTURE) raises: some case with that feature names it
FEATURE_COUNTER = {"equiv": EQ, "failed": UN, "subsume": RM, "strengthen": RM, "long": RM, "elim": EL, "salt": RM}

_cache = {}


def oracle_for(cnf_or_clauses, n_vars):
    o = ora.OracleSolver()
    if isinstance(cnf_or_clauses, Csr):
        o.add_cnf(cnf_or_clauses.lits, cnf_or_clauses.offsets)
    else:
        o.add_cnf(*ora.to_csr(cnf_or_clauses))
    o.reserve(n_vars)
    return o


def formula(case):
    """(Csr, oracle verdict, special variables) of a case tuple, computed once; the table's verdict and conflict count are
    asserted, so that a changed generator cannot quietly change the set."""
    if case not in _cache:
        seed, n, m, lens, features, refute, _, verdict, conflicts, _ = case
        cl, special = structured_cnf(seed, n, m, lens, features=features, refute=refute)
        cnf = Csr(cl, n)
        o = oracle_for(cnf, n)
        want = o.solve()
        assert (want, o.stats()["conflicts"]) == (verdict, conflicts), (case, want, o.stats()["conflicts"])
        _cache[case] = (cnf, want, special)
    return _cache[case]


def assumption_sets(case):
    """The 24 assumption sets of a case with the oracle's verdict for each, computed once: 1..6 literals, every other one over
    the gadgets' variables (those the simplification substitutes, fixes or eliminates), the rest over all variables; set 0 is
    empty, set 1 repeats a literal, set 2 holds a contradicting pair."""
    key = ("sets", case)
    if key not in _cache:
        cnf, _, special = formula(case)
        rng = np.random.default_rng(7000 + case[0])
        sets = []
        for i in range(N_SETS):
            a = []
            for _ in range(int(rng.integers(1, 7))):
                v = int(rng.choice(special)) if special and rng.random() < 0.5 else int(rng.integers(cnf.n_vars)) + 1
                a.append(v if rng.random() < 0.5 else -v)
            if i == 0:
                a = []
            elif i == 1:
                a.insert(int(rng.integers(len(a) + 1)), a[0])
            elif i == 2:
                pair = int(rng.choice(special)) if special else 1
                a = [l for l in a if abs(l) != pair]
                a.insert(int(rng.integers(len(a) + 1)), pair)
                a.insert(int(rng.integers(len(a) + 1)), -pair)
            sets.append(a)
        o = oracle_for(cnf, cnf.n_vars)
        _cache[key] = (sets, [o.solve(a) for a in sets])
    return _cache[key]


def verdict_mix(cases):
    v = [c[7] for c in cases.values()]
    return v.count(10), v.count(20)


def assumption_mix(cases):
    """(SAT, UNSAT) by the oracle over the assumption sets of all cases."""
    v = [r for c in cases.values() for r in assumption_sets(c)[1]]
    return v.count(10), v.count(20)


def within(seconds, s, fn):
    """fn() on solver s with a wall-clock limit (test_gpu_parity.solve_within for any call): the interrupt turns a hang into
    an undecided answer, which the judge's comparison with the oracle fails."""
    tm = threading.Timer(seconds, s.interrupter().interrupt)
    tm.start()
    try:
        return fn()
    finally:
        tm.cancel()


def check_simplified(s, cnf, simp):
    """b. of the module's docstring."""
    clauses, elim_clauses = s.debug_simplified()
    o = oracle_for(cnf, cnf.n_vars)
    seen = set()
    for c in clauses + elim_clauses:
        assert all(l != 0 and abs(l) <= cnf.n_vars for l in c), c
        key = tuple(sorted(c))
        if key in seen:
            continue
        seen.add(key)
        assert o.solve([-l for l in c]) == 20, ("the simplified formula holds a clause the caller's formula does not imply", c)
    if simp < 2:
        assert not elim_clauses
        o = oracle_for(clauses, cnf.n_vars)
        for c in cnf.clauses:
            assert o.solve([-l for l in c]) == 20, ("the simplified formula does not imply the caller's clause", c)
    return clauses, elim_clauses


def is_subsequence(core, given):
    it = iter(given)
    return all(l in it for l in core)


def judge(make_solver, case, simp, var_order, lds_val, tmp_path, limit_s=None, workers=None):
    """One case under one option set, judged as the module's docstring says.  `make_solver(**opts)` makes a handle (emulator
    or GPU); workers overrides the case's worker count (0 = the default fleet); limit_s puts every solve under a deadline.
    Returns the plain solve's counters."""
    cnf, want, _ = formula(case)
    refute, counters = case[5], case[9]
    opts = dict(workers=case[6] if workers is None else workers, simp=simp, var_order=var_order, lds_val=lds_val, slice_conflicts=100)
    run = (lambda s, fn: within(limit_s, s, fn)) if limit_s else (lambda s, fn: fn())
    # a. plain solve
    s = make_solver(**opts)
    s.debug_keep_simplified()
    proof = str(tmp_path / "simp.drup")
    if want == 20:
        s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    r = run(s, s.solve)                               # (a SolverError - any MI355SAT_ERR_* - fails the test here)
    assert r.value == want, (r, want)
    if r == SolverResult.Sat:
        assert ora.check_model(cnf.lits, cnf.offsets, s.full_solution(cnf.n_vars)) == -1
    else:
        assert s.core() == []
        assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, read_drup(proof)) == 1
    st = s.stats()
    print("counters", {k: st[k] for k in COUNTERS}, "conflicts", st["conflicts"], "launches", st["kernel_launches"])
    assert st["propagations"] == st["n_deq"]
    if st["workers"] >= 2 and st["conflicts"]:
        assert_ring_records_are_implied(s, cnf)
    # d. path taken
    for k in counters:
        assert st[k] > 0 or (k == EL and simp != 2), (k, st[k])
    assert simp == 2 or st[EL] == 0
    if refute:
        assert st["conflicts"] == 0 and st["decisions"] == 0
        try:
            launches = s.debug_last_search_build()["launches"]
        except SolverError:
            launches = 0
        assert launches == 0                        # no search slice ran (kernel_launches counts the probing launches too)
    # b. the formula the workers received
    clauses, _ = check_simplified(s, cnf, simp)
    assert ([] in clauses) if refute else (want == 20 or [] not in clauses)
    s.close()
    # c. batch under assumptions
    sets, verdicts = assumption_sets(case)
    s = make_solver(**dict(opts, workers=max(opts["workers"], N_SETS) if opts["workers"] else 0))
    s.debug_keep_simplified()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    res = run(s, lambda: s.solve_batch(sets))
    o = oracle_for(cnf, cnf.n_vars)
    for i, (a, v, got) in enumerate(zip(sets, verdicts, res)):
        assert got.value == v, (i, a, got, v)
        if got == SolverResult.Sat:
            assert ora.check_model(*ora.to_csr(cnf.clauses + [[l] for l in a]), s.solution_of(i, cnf.n_vars)) == -1, (i, a)
        else:
            core = s.core_of(i)
            assert is_subsequence(core, a), (i, a, core)
            assert o.solve(core) == 20, ("the oracle satisfies the formula under the core", i, a, core)
    check_simplified(s, cnf, simp)                  # the batch's own simplification (the assumptions' variables frozen)
    assert simp == 2 or s.stats()[EL] == 0
    s.close()
    return st

