"""Phase hints (mi355sat_phase / mi355sat_unphase / mi355sat_set_phases) on the CPU, through the wavefront emulator build
of the solver (tests/emu): ms_phase_kernel, the mapping of a hint through the simplification, the cold / warm rule and
solver_loop(phase_hints=True).

What makes the feature testable without a clock: let M be a model of the formula that agrees with the assumptions, and
let every variable be hinted to M.  Then every decision agrees with M, so every unit propagation agrees with M (M satisfies
the clause that became unit - an original one, or one the simplification or an earlier solve derived: all implied).  So the
solve ends SAT with ZERO conflicts and the model is M on every variable that was not eliminated.  M is the oracle's, made
different from what the unhinted solve finds by one assumption the product never hears of.

deterministic=1 everywhere; rephase and vivify stay at their defaults (off)."""
import numpy as np
import pytest

from fuzz_cases import EMU_CASES, formula, solve_and_judge
from helpers import VERDICTS, emu_lib, make_grid, platform_defs
from oracle import oracle as ora
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLayout, PlatformLimits, SolverError, SolverResult, solver_loop


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; simp = 0 / 2 have their own cases)
    kw.setdefault("workers", 1)
    kw.setdefault("deterministic", 1)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def golden_verdict(terrain, pset, k):
    v = [e for e in VERDICTS["verdicts"] if (e["terrain"], e["platforms"], e["k"]) == (terrain, pset, k)]
    assert len(v) == 1, (terrain, pset, k)
    return v[0]["verdict"]


def loaded(make_solver, cnf, **kw):
    s = make_solver(**kw)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    return s


_steer = {}


def steering_case(make_solver, terrain, pset, k):
    """(grid, enc, cnf, M) of a loose golden bound: M is the oracle's model under ONE extra assumption - a platform on a
    corner tile the unhinted solve leaves empty - which the product is never told.  Computed once per instance."""
    key = (terrain, pset, k)
    if key not in _steer:
        assert golden_verdict(terrain, pset, k) == "SAT"
        grid = make_grid(terrain)
        enc = Encoding.encode(platform_defs(pset), grid)
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        s = loaded(make_solver, cnf)
        assert s.solve() == SolverResult.Sat
        plain = s.full_solution(cnf.n_vars)
        s.close()
        corners = [(0, 0), (grid.width - 1, 0), (0, grid.height - 1), (grid.width - 1, grid.height - 1)]
        empty = [enc.platform_var(x, y, (1, 1)) for x, y in corners if plain[enc.platform_var(x, y, (1, 1)) - 1] < 0]
        assert empty, "the unhinted solve covers every corner with a 1x1 platform"
        o = ora.OracleSolver()
        o.add_cnf(cnf.lits, cnf.offsets)
        o.reserve(cnf.n_vars)
        assert o.solve([empty[0]]) == 10
        M = o.model(cnf.n_vars)
        assert M[empty[0] - 1] == 1 and ora.check_model(cnf.lits, cnf.offsets, M) == -1 and not np.any(M == 0)
        M.setflags(write=False)
        _steer[key] = (grid, enc, cnf, M)
    return _steer[key]


def assert_steered(make_solver, cnf, M, exact=True, guard=True, **opts):
    """Without hints these options find another model (the guard against a vacuous pass); hinted to M the solve makes no
    conflict and returns M (exact) or at least a model (variables were eliminated).  Returns the hinted handle, open."""
    if guard:
        s = loaded(make_solver, cnf, **opts)
        assert s.solve() == SolverResult.Sat
        assert not np.array_equal(s.full_solution(cnf.n_vars), M), "the unhinted solve finds M by itself: the case shows nothing"
        assert s.debug_phases() == dict(hinted=0, applied_cold=0, applied_warm=0, launches=0, mapped=0, dropped_eliminated=0, dropped_fixed=0)
        s.close()
    s = loaded(make_solver, cnf, **opts)
    s.set_phases(M)
    assert s.solve() == SolverResult.Sat
    st, ph, m = s.stats(), s.debug_phases(), s.full_solution(cnf.n_vars)
    print(opts, "conflicts", st["conflicts"], "decisions", st["decisions"], ph)
    assert st["conflicts"] == 0, (st["conflicts"], ph)
    assert ora.check_model(cnf.lits, cnf.offsets, m) == -1
    if exact:
        assert np.array_equal(m, M), np.flatnonzero(m != M)[:20]
    assert ph["hinted"] == cnf.n_vars and ph["applied_cold"] == 1 and ph["applied_warm"] == 0 and ph["launches"] >= 1
    assert ph["mapped"] + ph["dropped_eliminated"] + ph["dropped_fixed"] <= cnf.n_vars and ph["mapped"] > 0
    return s


# ---- 1. zero-conflict steering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase_mix", [0, 1])
@pytest.mark.parametrize("workers", [1, 4])
@pytest.mark.parametrize("pset", ["default", "1x1"])
def test_hinted_to_a_model_the_solve_makes_no_conflict_and_returns_it(pset, workers, phase_mix):
    """With 4 workers and phase_mix = 1 replicas 1 and 2 would start all TRUE / at random: a hint outranks that."""
    grid, enc, cnf, M = steering_case(emu_solver, "rect8x8", pset, 20)
    assert_steered(emu_solver, cnf, M, workers=workers, phase_mix=phase_mix).close()


# ---- 2. through the mappings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opts,exact", [("substitution", dict(simp=0), True), ("renumbering", dict(simp=-1, var_order=1), True),
                                             ("elimination", dict(simp=2), False)])
def test_hints_follow_their_variables_through_the_simplification(name, opts, exact):
    """simp = 0 substitutes equivalent literals (a hint may change sign on the way), var_order = 1 renumbers the device's
    variables, simp = 2 eliminates variables (their hints are dropped; the model is only clause-checked).  (The unhinted
    guard solve is made where it is cheap: probing runs through the fiber emulator in the other two, 20 s a solve; that the
    unhinted search does not find M is test 1's and this test's renumbering case.)"""
    grid, enc, cnf, M = steering_case(emu_solver, "rect8x8", "default", 20)
    s = assert_steered(emu_solver, cnf, M, exact=exact, guard=opts["simp"] == -1, workers=2, **opts)
    ph, st = s.debug_phases(), s.stats()
    if name == "elimination":
        assert 0 < ph["dropped_eliminated"] <= st["simp_eliminated"], (ph, st["simp_eliminated"])
    else:
        assert ph["dropped_eliminated"] == 0 and st["simp_eliminated"] == 0
    s.close()


# ---- 3. partial and conflicting hints never cost soundness --------------------------------------------------------------
def random_hints(n_vars, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, n_vars) * (2 * rng.integers(0, 2, n_vars) - 1)).astype(np.int8)     # half: none; else +-1


@pytest.mark.parametrize("name", list(EMU_CASES))
def test_random_hints_on_half_the_variables_change_no_verdict(tmp_path, name):
    """Every case of the emulator fuzz, judged as there: the oracle's verdict, SAT models clause-checked, and EVERY UNSAT
    answer with a DRUP proof (set_proof_path) that the oracle's RUP checker accepts."""
    case = EMU_CASES[name]
    cnf, want = formula(case)
    hints = random_hints(cnf.n_vars, 7000 + case[0])
    assert 0 < np.count_nonzero(hints) < cnf.n_vars and (hints > 0).any() and (hints < 0).any()
    seen = {}

    def hinted_solve(s):
        s.set_phases(hints)
        r = s.solve()
        seen.update(s.debug_phases())
        return r

    s, r, st = solve_and_judge(emu_solver, case, 0, 1, tmp_path, solve=hinted_solve, slice_conflicts=100)
    assert seen["hinted"] == np.count_nonzero(hints) and seen["applied_cold"] == 1
    assert seen["mapped"] + seen["dropped_fixed"] == seen["hinted"] and seen["launches"] == (1 if seen["mapped"] else 0)
    s.close()


# ---- 4. incremental -----------------------------------------------------------------------------------------------------
def warm_sequence(make_solver, terrain, pset, k, **opts):
    """Solve; exclude the model; hint to the oracle's model M2 of the accumulated formula; the next solve starts WARM, is
    seeded once, makes no conflict and returns M2; a third with unchanged hints launches nothing; without hints a fourth is
    still right."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    clauses = [[int(l) for l in cnf.lits[int(a):int(b)]] for a, b in zip(cnf.offsets[:-1], cnf.offsets[1:])]
    s = make_solver(**opts)
    s.set_incremental(True)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)

    def oracle():
        o = ora.OracleSolver()
        o.add_cnf(*ora.to_csr(clauses))
        o.reserve(cnf.n_vars)
        return o

    def exclude(m):     # on the platform variables: the next model is another LAYOUT
        pv = [enc.platform_var(x, y, d) for y in range(grid.height) for x in range(grid.width) for d in enc.platform_dims()]
        c = [-v if m[v - 1] > 0 else v for v in pv]
        clauses.append(c)
        s.add_clause(c)

    assert s.solve() == SolverResult.Sat
    m1 = s.full_solution(cnf.n_vars)
    assert ora.check_model(*ora.to_csr(clauses), m1) == -1
    exclude(m1)
    o = oracle()
    assert o.solve() == 10
    M2 = o.model(cnf.n_vars)
    s.set_phases(M2)
    i0, p0, c0 = s.debug_incremental(), s.debug_phases(), s.stats()["conflicts"]
    assert (p0["applied_cold"], p0["applied_warm"], p0["launches"]) == (0, 0, 0)
    assert s.solve() == SolverResult.Sat
    i1, p1, c1 = s.debug_incremental(), s.debug_phases(), s.stats()["conflicts"]
    assert i1["warm_solves"] == i0["warm_solves"] + 1 and i1["cold_solves"] == i0["cold_solves"], (i0, i1)
    assert p1["applied_warm"] == p0["applied_warm"] + 1 and p1["applied_cold"] == 0 and p1["launches"] >= 1, p1
    assert c1 - c0 == 0, (c0, c1)
    assert np.array_equal(s.full_solution(cnf.n_vars), M2)
    # unchanged hints: nothing is launched, the workers keep what they saved
    exclude(M2)
    assert s.solve().value == oracle().solve()
    i2, p2 = s.debug_incremental(), s.debug_phases()
    assert i2["warm_solves"] == i1["warm_solves"] + 1 and p2["launches"] == p1["launches"] and p2["applied_warm"] == p1["applied_warm"]
    # setting the same hints again changes nothing either
    s.set_phases(M2)
    exclude(s.full_solution(cnf.n_vars))
    assert s.solve().value == oracle().solve()
    assert s.debug_phases()["launches"] == p1["launches"]
    # no hints any more
    for v in range(1, cnf.n_vars + 1):
        s.unphase(v)
    assert s.debug_phases()["hinted"] == 0
    exclude(s.full_solution(cnf.n_vars))
    r = s.solve()
    assert r.value == oracle().solve()
    if r == SolverResult.Sat:
        assert ora.check_model(*ora.to_csr(clauses), s.full_solution(cnf.n_vars)) == -1
    assert s.debug_incremental()["warm_solves"] == i2["warm_solves"] + 2 and s.debug_phases()["launches"] == p1["launches"]
    return s


def test_a_warm_solve_is_seeded_once_when_the_hints_changed_and_never_again():
    warm_sequence(emu_solver, "rect8x8", "1x1", 20, workers=2).close()


# ---- 5. ABI edges -------------------------------------------------------------------------------------------------------
def test_literal_zero_is_an_argument_error():
    s = emu_solver()
    with pytest.raises(SolverError) as e:
        s.phase(0)
    assert e.value.code == -4            # MI355SAT_ERR_ARG
    with pytest.raises(SolverError) as e:
        s.unphase(0)
    assert e.value.code == -4
    s.close()


def test_a_hint_above_the_highest_variable_reserves_it():
    s = emu_solver()
    s.add_clause([1, 2])
    assert s.stats()["max_var"] == 2
    s.phase(-7)
    assert s.stats()["max_var"] == 7 and s.debug_phases()["hinted"] == 1
    assert s.solve() == SolverResult.Sat
    m = s.full_solution(7)
    assert m[6] == -1 and (m[0] == 1 or m[1] == 1)
    s.close()


def test_hints_set_before_any_clause_survive_to_the_first_solve():
    grid, enc, cnf, M = steering_case(emu_solver, "rect8x8", "1x1", 20)
    s = emu_solver()
    s.set_phases(M)
    for v in (3, 5):                     # (and literal by literal, both polarities; the same hint twice counts once)
        s.phase(int(M[v - 1]) * v)
    assert s.debug_phases()["hinted"] == cnf.n_vars
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Sat
    assert s.stats()["conflicts"] == 0 and np.array_equal(s.full_solution(cnf.n_vars), M)
    s.close()


def test_single_hints_steer_like_the_bulk_call():
    grid, enc, cnf, M = steering_case(emu_solver, "rect8x8", "1x1", 20)
    s = loaded(emu_solver, cnf)
    for v in range(1, cnf.n_vars + 1):
        s.phase(-v)
        s.phase(int(M[v - 1]) * v)         # the later hint wins
    assert s.solve() == SolverResult.Sat
    assert s.stats()["conflicts"] == 0 and np.array_equal(s.full_solution(cnf.n_vars), M)
    s.close()


def test_failed_and_core_stay_valid_after_a_hint():
    s = emu_solver()
    for c in ([1, 2], [-1, 3], [-2, 3], [4, 5]):
        s.add_clause(c)
    assert s.solve([-3, 4]) == SolverResult.Unsat
    core = s.core()
    assert core == [-3]
    s.phase(5)
    s.unphase(4)
    s.set_phases([1, -1, 0, 1])
    assert s.core() == core and s.failed(-3) and not s.failed(4)
    assert s.solve([4]) == SolverResult.Sat
    s.close()


def test_zeros_in_set_phases_clear_hints():
    s = emu_solver()
    s.set_phases([1, -1, 1, 0, -1])
    assert s.debug_phases()["hinted"] == 4
    s.set_phases([0, -1, 0])
    assert s.debug_phases()["hinted"] == 2           # 2 and 5 (beyond the array: kept)
    s.unphase(5)
    s.unphase(5)
    s.unphase(40)
    assert s.debug_phases()["hinted"] == 1
    s.set_phases(np.zeros(5, dtype=np.int8))
    assert s.debug_phases()["hinted"] == 0
    s.close()


# ---- 6. the loop --------------------------------------------------------------------------------------------------------
def hinted_loop(make_solver, terrain, pset, k0, kstar, **opts):
    """solver_loop(phase_hints=True) from k0 down to the optimum; every rung after the first was seeded once, with the
    encoder's variables of the model before.  (A rung that level-0 unit propagation refutes before anything is uploaded has
    no worker to seed - ex1 with the default platforms at k = 0 is one - so the instances here end in a searched rung.)
    Returns (history, per-rung debug_phases)."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    seen = []

    class Recording(Mi355Sat):
        def close(self):
            if getattr(self, "_h", None):
                seen.append(self.debug_phases())
            super().close()

    def make():
        return make_solver(_cls=Recording, **opts)

    lines = []
    hist = solver_loop(grid, enc, PlatformLimits({(1, 1): k0}), make_solver=make, out=lines.append, phase_hints=True)
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == kstar - 1, [(h["k"], h["result"]) for h in hist]
    sat = hist[:-1]
    assert sat and sat[-1]["count"] == kstar and all(h["result"] == SolverResult.Sat and h["valid"] and h["count"] <= h["k"] for h in sat)
    for h in sat:
        assert h["layout"].validate(grid).is_valid() and h["layout"].platform_count() == h["count"]
    assert "Solution validation FAILED" not in lines and lines[-1] == "No solution found for the current constraints"
    assert len(seen) == len(hist)
    assert seen[0]["hinted"] == 0 and seen[0]["applied_cold"] == 0 and seen[0]["launches"] == 0
    for p in seen[1:]:
        assert p["applied_cold"] == 1 and p["hinted"] == enc.n_vars and p["applied_warm"] == 0, p
    return hist, seen


def emu_solver_of(_cls=Mi355Sat, **kw):
    kw.setdefault("simp", -1)
    kw.setdefault("workers", 2)
    kw.setdefault("deterministic", 1)
    return _cls(_lib_override=emu_lib(), **kw)


def golden_kstar(terrain, pset):
    v = [e for e in VERDICTS["verdicts"] if (e["terrain"], e["platforms"]) == (terrain, pset)]
    kstar = min(e["k"] for e in v if e["verdict"] == "SAT")
    assert any(e["k"] == kstar - 1 and e["verdict"] == "UNSAT" for e in v)
    return kstar


@pytest.mark.parametrize("terrain,pset,k0", [("rect8x8", "1x1", 5), ("ex1", "1x1", 8)])
def test_the_hinted_loop_ends_at_the_golden_optimum(terrain, pset, k0):
    hist, seen = hinted_loop(emu_solver_of, terrain, pset, k0, golden_kstar(terrain, pset))
    assert len(hist) >= 2


def test_the_loop_hints_nothing_unless_asked():
    grid = make_grid("ex1")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    plain = []

    class Recording(Mi355Sat):
        def close(self):
            if getattr(self, "_h", None):
                plain.append(self.debug_phases()["hinted"])
            super().close()

    hist = solver_loop(grid, enc, PlatformLimits({(1, 1): 8}), make_solver=lambda: emu_solver_of(_cls=Recording), out=lambda l: None)
    assert len(plain) == len(hist) >= 2 and not any(plain)
