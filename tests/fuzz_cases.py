"""Random formulas for the differential tests of the search kernel (tests/test_emu_fuzz.py, test_gpu_fuzz.py and the option
tests), and their judge (test infrastructure).

The judge is never the product: the verdict is the oracle's (oracle.OracleSolver on the same CSR, computed once per
case), a SAT answer carries a model that oracle.check_model accepts, an UNSAT answer a DRUP proof that oracle.check_rup
accepts, and in fleets of two and more workers every record of the exchange ring is refuted by the oracle when negated.
Any MI355SAT_ERR_* is a SolverError and fails the test.

The instances were sized with the oracle on the CPU (its conflict counts are in the tables): the emulator makes 70-90
conflicts a second per worker, so its cases stay at a few hundred conflicts; the GPU gets the same ones plus a handful up to
a few thousand."""
from helpers import Csr, assert_ring_records_are_implied, assert_search_build, random_cnf, salt_cnf
from oracle import oracle as ora
from timberborn_support_solver_amd import SolverResult
from timberborn_support_solver_amd.dimacs import read_drup

BUILD_LIST = [(o, l) for o in (0, 2, 4) for l in (1, -1)]
BUILD_IDS = [f"{w}-{a}" for w in ("one-wave-build", "two-waves-build", "full-fleet-build") for a in ("lds", "slab")]
VIVIFY_BUILDS = [(o, l) for o, l in BUILD_LIST if o != 4]        # the full-fleet build is compiled without vivification
MIXED = (2, 3, 4, 5, 6)
MIXED_W = (2, 3, 3, 3, 4, 4, 5, 6)       # the same lengths, fewer binaries: these formulas take some search

# name -> (seed, n_vars, n_clauses, lens, salt seed or None, workers, oracle verdict, oracle conflicts)
# 3-SAT at 4.26 clauses per variable, n = 40 .. 120; mixed lengths 2 .. 6; salted = with duplicates, repeated literals,
# tautologies and units (helpers.salt_cnf)
EMU_CASES = {
    "3sat-n40-s3": (3, 40, 170, (3,), None, 2, 20, 50),
    "3sat-n50-s5": (5, 50, 213, (3,), None, 2, 10, 40),
    "3sat-n60-s2": (2, 60, 256, (3,), None, 2, 20, 105),
    "3sat-n70-s5": (5, 70, 298, (3,), None, 1, 10, 106),
    "3sat-n80-s4": (4, 80, 341, (3,), None, 1, 10, 117),
    "3sat-n110-s4": (4, 110, 469, (3,), None, 1, 10, 46),
    "mixed-n60-s100": (100, 60, 252, MIXED, None, 2, 10, 10),
    "mixed-n120-s102": (102, 120, 552, MIXED, None, 2, 20, 13),
    "mixedw-n90-s100": (100, 90, 450, MIXED_W, None, 2, 10, 38),
    "mixedw-n120-s102": (102, 120, 600, MIXED_W, None, 1, 20, 112),
    "salted-3sat-n60-s203": (203, 60, 240, (3,), 303, 2, 20, 84),
    "salted-3sat-n80-s200": (200, 80, 320, (3,), 300, 1, 10, 95),
    "salted-mixed-n100-s401": (401, 100, 380, MIXED, 501, 2, 10, 4),
}
GPU_ONLY_CASES = {
    "3sat-n120-s6": (6, 120, 511, (3,), None, 8, 10, 151),
    "3sat-n100-s6": (6, 100, 426, (3,), None, 8, 20, 810),
    "3sat-n110-s2": (2, 110, 469, (3,), None, 8, 10, 627),
    "3sat-n110-s3": (3, 110, 469, (3,), None, 8, 20, 1444),
    "3sat-n120-s2": (2, 120, 511, (3,), None, 8, 20, 1134),
    "3sat-n120-s5": (5, 120, 511, (3,), None, 8, 20, 1862),
    "salted-3sat-n100-s203": (203, 100, 400, (3,), 303, 8, 20, 429),
}
GPU_CASES = dict(EMU_CASES, **GPU_ONLY_CASES)
# The formula the default build first failed on (MS_ST_ERR_INTERNAL after 429 conflicts, the oracle: SAT after 635), with the
# options of that report.
REPRODUCER = (1, 120, 516, (3,), None, 1, 10, 635)
REPRODUCER_OPTS = dict(workers=1, simp=-1, slice_conflicts=500)

_cache = {}


def formula(case):
    """(Csr, oracle verdict 10 / 20) of a case tuple, computed once.  The table's verdict and conflict count are what the
    oracle said when the case was sized: asserted here, so that a changed generator cannot quietly change the set."""
    if case not in _cache:
        seed, n, m, lens, salt, _, verdict, conflicts = case
        cl = random_cnf(seed, n, m, lens)
        if salt is not None:
            cl = salt_cnf(cl, salt, n, n_units=2)
        cnf = Csr(cl, n)
        o = ora.OracleSolver()
        o.add_cnf(cnf.lits, cnf.offsets)
        o.reserve(n)
        want = o.solve()
        assert (want, o.stats()["conflicts"]) == (verdict, conflicts), (case, want, o.stats()["conflicts"])
        _cache[case] = (cnf, want)
    return _cache[case]


def verdict_mix(cases):
    v = [c[6] for c in cases.values()]
    return v.count(10), v.count(20)


def wanted_build(one_per_simd, lds_val):
    return (1 if lds_val == 1 else 0, max(1, one_per_simd))


def solve_and_judge(make_solver, case, one_per_simd, lds_val, tmp_path, schedule=None, ring=None, solve=None, **opts):
    """One solve of the case in the build given, judged as the module's docstring says.  `make_solver(**opts)` makes the
    handle (emulator or GPU); opts override the case's worker count.  Returns (solver, result, stats): the caller closes."""
    cnf, want = formula(case)
    opts.setdefault("workers", case[5])
    opts.setdefault("simp", -1)          # level-0 unit propagation only: the search kernel decides the formula
    s = make_solver(one_per_simd=one_per_simd, lds_val=lds_val, **opts)
    if schedule:
        s.debug_set_schedule(*schedule)
    proof = str(tmp_path / "fuzz.drup")
    if want == 20:
        s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    r = solve(s) if solve else s.solve()            # (a SolverError - any MI355SAT_ERR_* - fails the test here)
    assert r.value == want, (r, want)
    assert_search_build(s, *wanted_build(one_per_simd, lds_val))
    if r == SolverResult.Sat:
        assert ora.check_model(cnf.lits, cnf.offsets, s.full_solution(cnf.n_vars)) == -1
    else:
        assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, read_drup(proof)) == 1
    st = s.stats()
    assert st["propagations"] == st["n_deq"]
    if (opts["workers"] >= 2) if ring is None else ring:
        assert_ring_records_are_implied(s, cnf)
    return s, r, st
