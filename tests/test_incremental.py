"""Warm incremental solve (mi355sat_set_incremental) on the CPU, through the wavefront emulator build of the solver
(tests/emu): ms_attach_kernel, the host's warm / cold rule and its fallbacks, and solver_loop_incremental.

Every verdict is compared with the oracle's CDCL on the ACCUMULATED formula plus the call's assumptions, every SAT model
is clause-checked against everything added so far, every core as tests/test_assumption_cores.py checks it (the oracle
refutes formula AND core; the core is a subset of the assumptions in the caller's order)."""
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import ROOT, VERDICTS, assert_ring_records_are_implied, assert_search_build, emu_lib, make_grid, platform_defs
from oracle import oracle as ora
from timberborn_support_solver_amd import (ColdReason, Encoding, Mi355Sat, PlatformLayout, PlatformLimits, SolverResult, solver_loop,
                                           solver_loop_incremental)

N_FRESH = 120      # variables above the encoder's that the sequences use, reserved before the first solve


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; simp = 0 / 2 have their own cases)
    kw.setdefault("workers", 2)
    kw.setdefault("slice_conflicts", 200)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


_cnfs = {}


def sweep_cnf(terrain, pset, k_max=8):
    key = (terrain, pset, k_max)
    if key not in _cnfs:
        grid = make_grid(terrain)
        enc = Encoding.encode(platform_defs(pset), grid)
        _cnfs[key] = (grid, enc, enc.with_limits_into_cnf(PlatformLimits({(1, 1): k_max}), sweep=True))
    return _cnfs[key]


class Checked:
    """A solver handle plus everything added to it so far; solve() checks the answer against the oracle."""

    def __init__(self, cnf, solver, incremental=True, n_vars=None, run=None):
        self.s = solver
        self.n_vars = (cnf.n_vars + N_FRESH) if n_vars is None else n_vars
        self.clauses = []
        self.base = cnf
        self.log = []
        self.run = run or (lambda fn: fn())        # e.g. every solve under a deadline (tests/incremental_cases.py)
        if incremental:
            self.s.set_incremental(True)
        self.s.add_cnf(cnf.lits, cnf.offsets)
        self.s.reserve(self.n_vars)

    def add(self, clause):
        self.clauses.append([int(l) for l in clause])
        self.s.add_clause(clause)
        self.n_vars = max(self.n_vars, max(abs(int(l)) for l in clause))

    def formula(self):
        extra = np.asarray([l for c in self.clauses for l in c], dtype=np.int32)
        lits = np.concatenate([np.asarray(self.base.lits, dtype=np.int32), extra])
        offs = np.concatenate([np.asarray(self.base.offsets, dtype=np.uint64),
                               np.uint64(self.base.offsets[-1]) + np.cumsum([len(c) for c in self.clauses], dtype=np.uint64)])
        return lits, offs

    def oracle(self):
        o = ora.OracleSolver()
        o.add_cnf(*self.formula())
        o.reserve(self.n_vars)
        return o

    def solve(self, assumptions=(), expect=None, may_stop=False):
        """may_stop: the solve may also end undecided (an interrupt the caller sent, a conflict budget): logged, not judged."""
        assumptions = [int(l) for l in assumptions]
        self.n_vars = max([self.n_vars] + [abs(l) for l in assumptions])
        r = self.run(lambda: self.s.solve(assumptions))
        if may_stop and r == SolverResult.Interrupted:
            self.log.append((r, None))
            return r
        want = self.oracle().solve(assumptions)
        assert r.value == want, (r, want, assumptions, self.s.debug_incremental())
        if expect is not None:
            assert r == expect, (r, assumptions)
        core = None
        if r == SolverResult.Sat:
            m = self.s.full_solution(self.n_vars)
            lits, offs = self.formula()
            assert ora.check_model(lits, offs, m) == -1
            assert all(m[abs(l) - 1] == (1 if l > 0 else -1) for l in assumptions), "the model breaks an assumption"
        else:
            core = self.s.core()
            assert len(set(core)) == len(core) and set(core) <= set(assumptions), (core, assumptions)
            first = {}
            for i, l in enumerate(assumptions):
                first.setdefault(l, i)
            assert core == sorted(core, key=first.__getitem__)
            assert self.oracle().solve(core) == 20, core
            assert [l for l in dict.fromkeys(assumptions) if self.s.failed(l)] == core
        self.log.append((r, core))
        return r

    def info(self):
        return self.s.debug_incremental()


def fresh(cnf, i):
    return cnf.n_vars + 1 + i


# ---- the test that fails without the feature -------------------------------------------------------------------------
def test_second_solve_after_an_added_unit_starts_warm_and_keeps_the_learnt_clauses():
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    c = Checked(cnf, emu_solver())
    c.solve(expect=SolverResult.Sat)
    conflicts = c.s.stats()["conflicts"]
    i = c.info()
    assert (i["enabled"], i["warm_solves"], i["cold_solves"], i["last_cold_reason"]) == (1, 0, 1, ColdReason.FIRST)
    c.add([-int(cnf.card_outputs[5])])
    c.solve(expect=SolverResult.Sat)
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"], i["attached_units"], i["attached_clauses"]) == (1, 1, 1, 0), i
    assert i["attach_launches"] >= 1
    assert conflicts > 0 and i["resident_learnts"] > 0, (conflicts, i)
    c.s.close()
    # the same sequence with the feature off: never warm
    c = Checked(cnf, emu_solver(), incremental=False)
    c.solve(expect=SolverResult.Sat)
    c.add([-int(cnf.card_outputs[5])])
    c.solve(expect=SolverResult.Sat)
    i = c.info()
    assert (i["enabled"], i["warm_solves"], i["cold_solves"], i["attach_launches"]) == (0, 0, 0, 0), i
    c.s.close()


# ---- scripted sequences ----------------------------------------------------------------------------------------------
def run_script(c, enc, cnf, grid, k_unsat, k_sat):
    """Units, binaries, ternaries and long clauses (one of 71 literals), assumption sets and solves, interleaved."""
    f = lambda i: fresh(cnf, i)
    p = [enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    card = [int(l) for l in cnf.card_outputs]
    c.solve(expect=SolverResult.Sat)
    c.add([-card[k_sat + 1]])                                        # a tighter bound as a unit
    c.solve(expect=SolverResult.Sat)
    c.add([f(0), f(1)])                                              # binary
    c.add([-f(0), f(2), p[0]])                                       # ternary
    c.solve([-f(1), -f(2)], expect=SolverResult.Sat)                 # forces a platform on tile 0
    long71 = [f(10 + i) for i in range(70)] + [-card[k_unsat]]       # 71 literals: two rounds of the attach kernel
    c.add(long71)
    c.solve([-f(10 + i) for i in range(70)], expect=SolverResult.Unsat)   # UNSAT because of the long clause only
    c.solve([-f(10 + i) for i in range(69)], expect=SolverResult.Sat)
    c.solve([-card[k_unsat], f(3)], expect=SolverResult.Unsat)
    late = [-p[0], f(4), f(5), f(6), f(7), -f(8)]                    # stays SAT; the model must satisfy it
    c.add(late)
    c.solve([-f(1), -f(2), -f(4), -f(5), -f(6), -f(7)], expect=SolverResult.Sat)
    c.solve([-f(1), -f(2), -f(4), -f(5), -f(6), -f(7), f(8)], expect=SolverResult.Unsat)
    for i in range(4):
        c.add([-f(20 + i)])                                          # level-0 facts ...
    c.solve(expect=SolverResult.Sat)
    c.add([f(20), f(21), f(22), f(23)])                              # ... that falsify this clause: the empty core
    c.solve([f(3), -f(4)], expect=SolverResult.Unsat)
    assert c.log[-1][1] == []
    c.solve(expect=SolverResult.Unsat)                               # the handle stays refuted
    c.add([f(30), f(31)])
    c.solve([f(30)], expect=SolverResult.Unsat)
    assert c.log[-1][1] == []


@pytest.mark.parametrize("terrain,pset,k_unsat,k_sat", [("ex1", "1x1", 2, 3), ("rect8x8", "1x1", 3, 4)], ids=lambda x: str(x))
def test_scripted_sequence_equals_the_cold_handle(terrain, pset, k_unsat, k_sat):
    grid, enc, cnf = sweep_cnf(terrain, pset)
    warm = Checked(cnf, emu_solver())
    run_script(warm, enc, cnf, grid, k_unsat, k_sat)
    i = warm.info()
    n_solves = len(warm.log)
    assert i["cold_solves"] == 1 and i["warm_solves"] == n_solves - 1, i
    assert i["attached_units"] == 5 and i["attached_clauses"] == 5, i      # (the last binary came after the refutation)
    cold = Checked(cnf, emu_solver(), incremental=False)
    run_script(cold, enc, cnf, grid, k_unsat, k_sat)
    assert [r for r, _ in warm.log] == [r for r, _ in cold.log]
    assert cold.info()["warm_solves"] == 0
    warm.s.close()
    cold.s.close()


def test_scripted_sequence_on_rect16_default():
    """The larger formula (5 000 variables, 19 000 clauses), with the bounds the emulator decides in seconds."""
    grid, enc, cnf = sweep_cnf("rect16x16", "default", 8)
    f = lambda i: fresh(cnf, i)
    card = [int(l) for l in cnf.card_outputs]
    p = enc.platform_var(3, 3, (1, 1))
    c = Checked(cnf, emu_solver(workers=1))
    c.solve(expect=SolverResult.Sat)
    c.add([-card[7]])
    c.add([f(0), f(1), -p])
    c.add([f(40 + i) for i in range(66)] + [p])
    c.solve([-f(40 + i) for i in range(66)] + [-f(0)], expect=SolverResult.Sat)       # p, hence f(1)
    c.solve([-f(40 + i) for i in range(66)] + [-f(0), -f(1)], expect=SolverResult.Unsat)
    c.add([-f(0)])
    c.add([-f(1)])
    c.solve([-f(40 + i) for i in range(66)], expect=SolverResult.Unsat)
    c.solve(expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["attached_units"], i["attached_clauses"]) == (1, 4, 3, 2), i
    c.s.close()


# ---- pinned clauses survive the learnt-clause reduction ----------------------------------------------------------------
def test_attached_clause_survives_reductions():
    """The attached clause is idle (satisfied by an assumption) through a refutation with many reductions, then decides
    the next solve.  Mutation check (reported in the pull request): attaching with LBD 3 instead of 1 loses it."""
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    f = lambda i: fresh(cnf, i)
    card = [int(l) for l in cnf.card_outputs]
    c = Checked(cnf, emu_solver(workers=1, reduce_first=8, reduce_inc=1))
    c.solve(expect=SolverResult.Sat)
    clause = [f(i) for i in range(6)] + [-f(6)]
    c.add(clause)
    before = c.s.stats()["reduce_dbs"]
    c.solve([f(0), f(1), -card[3]], expect=SolverResult.Unsat)            # warm; the clause is satisfied throughout
    c.solve([f(0), f(1), -card[4], -card[3]], expect=SolverResult.Unsat)
    c.solve([f(0), f(1), -card[4]], expect=SolverResult.Sat)
    c.solve([-f(i) for i in range(6)] + [f(6)], expect=SolverResult.Unsat)    # rests on the attached clause alone
    assert set(c.log[-1][1]) == {-f(i) for i in range(6)} | {f(6)}
    c.solve([-f(i) for i in range(6)], expect=SolverResult.Sat)
    assert c.s.stats()["reduce_dbs"] - before >= 5
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["attached_clauses"]) == (1, 5, 1), i
    c.s.close()


# ---- workers created after the attach ---------------------------------------------------------------------------------
def test_workers_grown_after_the_attach_get_the_attached_clauses():
    """258 workers with the ramp-up on: the first (cold) solve ends in its first slice, on the 256 slabs the ramp-up
    starts with; the warm solve grows the fleet after its first slice.  Without the attached bound the two late workers
    would answer SAT within a few conflicts."""
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    # (a slab buffer parked by an earlier handle of this process that has room for all 258 would give every worker its
    # slab at the cold start: nothing would grow, and the first attach would reach them all)
    emu_lib().mi355sat_release_cached_memory()
    c = Checked(cnf, emu_solver(workers=258, slice_conflicts=1, ramp=0))
    c.solve(expect=SolverResult.Sat)
    assert c.s.debug_last_search_build()["active"] == 256 and c.s.stats()["kernel_launches"] == 1
    c.add([-card[2]])                                                   # k = 2: UNSAT (golden), after some conflicts
    c.solve(expect=SolverResult.Unsat)
    i = c.info()
    assert c.s.debug_last_search_build()["active"] == 258, "the fleet did not grow during the warm solve"
    assert (i["cold_solves"], i["warm_solves"]) == (1, 1) and i["attach_launches"] == 2, i
    c.s.close()


# ---- cold fallbacks ------------------------------------------------------------------------------------------------------
def test_fallback_variable_above_the_upload():
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    nv = cnf.n_vars
    c = Checked(cnf, emu_solver(), n_vars=nv)            # nothing reserved beyond the formula
    c.solve(expect=SolverResult.Sat)
    c.add([nv + 1, nv + 2])
    c.solve([-(nv + 1)], expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (2, 0, ColdReason.NEW_VAR), i
    c.solve([nv + 5], expect=SolverResult.Sat)           # an assumption on a new variable
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (3, 0, ColdReason.NEW_VAR), i
    c.add([-(nv + 5), nv + 3])
    c.solve([nv + 5, -(nv + 3)], expect=SolverResult.Unsat)     # known variables now: warm
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"]) == (3, 1), i
    c.s.close()
    c = Checked(cnf, emu_solver(), n_vars=nv + 5)        # the same after reserve(): no fallback
    c.solve(expect=SolverResult.Sat)
    c.add([nv + 1, nv + 2])
    c.solve([-(nv + 1)], expect=SolverResult.Sat)
    c.solve([nv + 5], expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (1, 2, ColdReason.FIRST), i
    c.s.close()


def test_fallback_eliminated_variable():
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    c = Checked(cnf, emu_solver(simp=2))
    c.solve(expect=SolverResult.Sat)
    assert c.s.stats()["simp_eliminated"] > 0
    # some variable of the formula the elimination took: found through the hook, one candidate after the other
    hit = None
    for v in range(1, cnf.n_vars + 1):
        before = c.info()["cold_solves"]
        c.add([v, fresh(cnf, 0)])
        c.solve([-fresh(cnf, 0)])
        i = c.info()
        if i["cold_solves"] > before:
            hit = v
            assert i["last_cold_reason"] == ColdReason.ELIMINATED, i
            break
    assert hit is not None, "no clause named an eliminated variable"
    c.solve(expect=SolverResult.Sat)                     # after the cold start the handle is warm again
    assert c.info()["cold_solves"] == before + 1
    c.s.close()


def test_fallback_proof_path(tmp_path):
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    c = Checked(cnf, emu_solver())
    c.solve(expect=SolverResult.Sat)
    c.s.set_proof_path(str(tmp_path / "p.drup"))
    c.add([-int(cnf.card_outputs[2])])
    c.solve(expect=SolverResult.Unsat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (2, 0, ColdReason.PROOF), i
    assert open(str(tmp_path / "p.drup")).read().splitlines()[-1].strip() == "0"
    c.s.close()


def test_fallback_after_a_batch_in_between():
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    c = Checked(cnf, emu_solver())
    c.solve(expect=SolverResult.Sat)
    assert [r.name for r in c.s.solve_batch([[-card[2]], [-card[4]]])] == ["Unsat", "Sat"]
    c.add([-card[4]])
    c.solve(expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (2, 0, ColdReason.OTHER_SEARCH), i
    c.solve([-card[2]], expect=SolverResult.Unsat)       # warm again
    c.s.propagate_batch([[1], [-1]], n_vars=cnf.n_vars)
    c.solve([-card[3]], expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (3, 1, ColdReason.OTHER_SEARCH), i
    c.s.close()


def test_fallback_cube_split_and_simp_default():
    grid, enc, cnf = sweep_cnf("ex1", "1x1")
    c = Checked(cnf, emu_solver(workers=3, cube_split=1))
    c.solve(expect=SolverResult.Sat)
    c.add([-int(cnf.card_outputs[2])])
    c.solve(expect=SolverResult.Unsat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["last_cold_reason"]) == (2, 0, ColdReason.CUBE_SPLIT), i
    c.s.close()
    # the default simplification (equivalent literals, probing, subsumption) and the device's own variable order: warm
    c = Checked(cnf, emu_solver(simp=0, var_order=1))
    c.solve(expect=SolverResult.Sat)
    c.add([-int(cnf.card_outputs[3])])
    c.solve(expect=SolverResult.Sat)
    c.add([-int(cnf.card_outputs[2])])
    c.solve(expect=SolverResult.Unsat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"]) == (1, 2), i
    c.s.close()


# ---- interrupt, budget, ring, determinism --------------------------------------------------------------------------------
def test_interrupt_during_a_warm_solve_leaves_the_handle_warm():
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    c = Checked(cnf, emu_solver(workers=1, slice_conflicts=5))
    c.solve(expect=SolverResult.Sat)
    threading.Timer(0.3, c.s.interrupter().interrupt).start()
    assert c.s.solve([-card[3]]) == SolverResult.Interrupted           # (the refutation takes the emulator several seconds)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"]) == (1, 1), i
    c.solve([-card[6]], expect=SolverResult.Sat)
    c.solve([-card[3]], expect=SolverResult.Unsat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"]) == (1, 3), i
    # an interrupt that arrives between two solves stops the next one and is consumed by it
    c.s.interrupter().interrupt()
    assert c.s.solve() == SolverResult.Interrupted
    c.solve(expect=SolverResult.Sat)
    assert c.info()["warm_solves"] == 5
    c.s.close()
    # an exhausted conflict budget: counted per solve (the workers' counters run on), and the handle stays warm
    c = Checked(cnf, emu_solver(workers=1, slice_conflicts=5, conflict_budget=60))
    c.solve(expect=SolverResult.Sat)
    assert 0 < c.s.stats()["conflicts"] < 60
    assert c.s.solve([-card[3]]) == SolverResult.Interrupted
    assert c.s.stats()["conflicts"] >= 60
    c.solve([-card[6]], expect=SolverResult.Sat)
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"]) == (1, 2), i
    c.s.close()


def test_ring_records_after_three_warm_solves_follow_from_the_accumulated_formula():
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    c = Checked(cnf, emu_solver(workers=3, slice_conflicts=20))
    c.solve(expect=SolverResult.Sat)
    for k in (6, 5, 4):
        c.add([-card[k]])
        c.solve(expect=SolverResult.Sat)
    assert c.info()["warm_solves"] == 3

    class Acc:
        pass
    acc = Acc()
    acc.lits, acc.offsets = c.formula()
    acc.n_vars = c.n_vars
    assert assert_ring_records_are_implied(c.s, acc) > 0
    c.s.close()


def test_deterministic_warm_sequences_repeat_themselves():
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    runs = []
    for _ in range(2):
        c = Checked(cnf, emu_solver(workers=3, deterministic=1, slice_conflicts=20, seed=5))
        c.solve(expect=SolverResult.Sat)
        c.add([-card[5]])
        c.add([fresh(cnf, 0), fresh(cnf, 1), fresh(cnf, 2), -card[3]])
        c.solve(expect=SolverResult.Sat)
        c.solve([-fresh(cnf, 0), -fresh(cnf, 1), -fresh(cnf, 2)], expect=SolverResult.Unsat)
        st = c.s.stats()
        runs.append(({k: st[k] for k in ("propagations", "decisions", "conflicts", "restarts", "learnts", "n_watch", "n_enq", "shared_imported")},
                     c.info(), c.log))
        c.s.close()
    assert runs[0] == runs[1]
    assert runs[0][1]["warm_solves"] == 2


# ---- the six builds of the search kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("one_per_simd,lds_val", [(o, l) for o in (0, 2, 4) for l in (1, -1)],
                         ids=lambda v: str(v))
def test_warm_sequence_on_every_search_build(one_per_simd, lds_val):
    grid, enc, cnf = sweep_cnf("rect8x8", "1x1")
    card = [int(l) for l in cnf.card_outputs]
    f = lambda i: fresh(cnf, i)
    c = Checked(cnf, emu_solver(workers=4, slice_conflicts=10, one_per_simd=one_per_simd, lds_val=lds_val))
    c.solve(expect=SolverResult.Sat)
    c.add([-card[5]])
    c.add([f(i) for i in range(65)] + [-card[3]])
    c.solve([-f(i) for i in range(65)], expect=SolverResult.Unsat)
    c.solve([-f(i) for i in range(64)], expect=SolverResult.Sat)
    c.add([-card[4]])
    c.solve(expect=SolverResult.Sat)
    assert_search_build(c.s, 1 if lds_val == 1 else 0, max(1, one_per_simd))
    i = c.info()
    assert (i["cold_solves"], i["warm_solves"], i["attached_units"], i["attached_clauses"]) == (1, 3, 2, 1), i
    c.s.close()


# ---- the loop ----------------------------------------------------------------------------------------------------------
def golden_kstar(terrain, pset):
    sat = [v["k"] for v in VERDICTS["verdicts"] if (v["terrain"], v["platforms"]) == (terrain, pset) and v["verdict"] == "SAT"]
    unsat = [v["k"] for v in VERDICTS["verdicts"] if (v["terrain"], v["platforms"]) == (terrain, pset) and v["verdict"] == "UNSAT"]
    assert min(sat) == max(unsat) + 1
    return min(sat)


@pytest.mark.parametrize("terrain,pset,k0", [("ex1", "1x1", 8), ("rect8x8", "1x1", 8), ("rect16x16", "default", 5)], ids=lambda x: str(x))
def test_incremental_loop_is_the_sequential_loop_on_one_handle(terrain, pset, k0):
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    kstar = golden_kstar(terrain, pset)
    lines, ref_lines, handles = [], [], []

    def mk():
        handles.append(emu_solver(workers=1))
        return handles[-1]

    hist = solver_loop_incremental(grid, enc, PlatformLimits({(1, 1): k0}), make_solver=mk, out=lines.append)
    ref = solver_loop(grid, enc, PlatformLimits({(1, 1): k0}), make_solver=lambda: emu_solver(workers=1), out=ref_lines.append)
    assert [(h["k"], h["result"]) for h in hist] == [(h["k"], h["result"]) for h in ref]
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == kstar - 1
    sat = [h for h in hist if h["result"] == SolverResult.Sat]
    assert sat and sat[-1]["count"] == kstar
    for h in sat:       # every printed layout validates, by the product's validator and from the model itself
        assert h["valid"] and h["count"] <= h["k"]
        assert isinstance(h["layout"], PlatformLayout) and h["layout"].validate(grid).is_valid()
    assert lines == ref_lines and "Solution validation FAILED" not in lines
    assert lines[-1] == "No solution found for the current constraints"
    assert len(handles) == 1
    i = hist[-1]["incremental"]
    assert i["cold_solves"] == 1 and i["warm_solves"] == len(hist) - 1, i


def test_incremental_loop_with_a_first_bound_that_needs_no_totalizer():
    """-l1:1000 on ex1: nothing to tighten in the first CNF, so the second bound gets a handle of its own."""
    grid = make_grid("ex1")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    handles = []

    def mk():
        handles.append(emu_solver(workers=1))
        return handles[-1]

    hist = solver_loop_incremental(grid, enc, PlatformLimits({(1, 1): 1000}), make_solver=mk, out=lambda s: None)
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == 2 and hist[-2]["count"] == 3
    assert len(handles) == 2
    with pytest.raises(ValueError):
        solver_loop_incremental(grid, enc, PlatformLimits({(1, 1): 3}, weights={(1, 1): 2}, weight_limit=5))


# ---- the C header: tests/abi_incremental.c (the Rust shim's calls with set_incremental, replayed in C) --------------------
PKG = os.path.join(ROOT, "timberborn_support_solver_amd")


def build_abi_incremental(tmp_path, libdir, libname):
    exe = str(tmp_path / ("abi_incremental_" + libname))
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "abi_incremental.c"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir])
    return exe


def run_abi_incremental(exe, tmp_path, cnf, n_vars, workers, steps, timeout=600):
    """steps: ("c", clause) / ("a", assumptions).  Returns [(result, core or model)] per solve and the hook's last line."""
    path = str(tmp_path / "cnf.bin")
    with open(path, "wb") as f:
        np.array([n_vars, cnf.n_clauses], dtype=np.int64).tofile(f)
        np.asarray(cnf.offsets, dtype=np.uint64).tofile(f)
        np.asarray(cnf.lits, dtype=np.int32).tofile(f)
    spath = str(tmp_path / "steps.txt")
    with open(spath, "w") as f:
        for kind, lits in steps:
            f.write(kind + " " + " ".join(str(int(l)) for l in lits) + " 0\n")
    out = subprocess.run([exe, path, str(workers), spath], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr)
    answers = []
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "result":
            answers.append([int(t[1]), None])
        elif t[0] == "core":
            answers[-1][1] = [int(x) for x in t[2:]]
        elif t[0] == "model":
            answers[-1][1] = np.asarray([int(x) for x in t[1:]], dtype=np.int8)
    hook = dict(zip(*[iter(out.stdout.splitlines()[-1].split()[1:])] * 2))
    return answers, {k: int(v) for k, v in hook.items()}


def abi_steps_and_check(exe, tmp_path, terrain, workers, timeout=600):
    grid, enc, cnf = sweep_cnf(terrain, "1x1" if terrain != "rect16x16" else "default")
    card = [int(l) for l in cnf.card_outputs]
    f = lambda i: fresh(cnf, i)
    k_unsat = {"ex1": 2, "rect8x8": 3, "rect16x16": 3}[terrain]
    steps = [("c", [-card[k_unsat + 3]]), ("a", []), ("c", [f(0), f(1), f(2), f(3), -card[k_unsat]]),
             ("a", [-f(0), -f(1), -f(2), -f(3)]), ("a", [-f(0), -f(1), -f(2)]), ("c", [-card[k_unsat + 1]]), ("a", [f(5)])]
    n_vars = cnf.n_vars + N_FRESH
    answers, hook = run_abi_incremental(exe, tmp_path, cnf, n_vars, workers, steps, timeout)
    assert [r for r, _ in answers] == [10, 10, 20, 10, 10]
    assert hook == {"warm": 4, "cold": 1, "clauses": 1, "units": 2, "reason": int(ColdReason.FIRST)}, hook
    # replay on the oracle: accumulated formula, per-solve assumptions
    o = Checked.__new__(Checked)
    o.base, o.clauses, o.n_vars = cnf, [], n_vars
    solves = iter(answers[1:])
    assert ora.check_model(cnf.lits, cnf.offsets, answers[0][1]) == -1
    for kind, lits in steps:
        if kind == "c":
            o.clauses.append(lits)
            continue
        r, extra = next(solves)
        assert o.oracle().solve(lits) == r
        if r == 10:
            assert ora.check_model(*o.formula(), extra) == -1 and all(extra[abs(l) - 1] == (1 if l > 0 else -1) for l in lits)
        else:
            assert set(extra) <= set(lits) and o.oracle().solve(extra) == 20


def test_abi_incremental_builds_against_the_header_and_library(tmp_path):
    exe = build_abi_incremental(tmp_path, PKG, "mi355sat")
    assert subprocess.run([exe], capture_output=True).returncode == 2     # usage error: main() was reached


def test_abi_incremental_call_sequence_on_the_emulator(tmp_path):
    emu_lib()
    exe = build_abi_incremental(tmp_path, os.path.join(ROOT, "tests", "emu"), "mi355sat_emu")
    abi_steps_and_check(exe, tmp_path, "rect8x8", 2)


def test_abi_sizes_are_unchanged():
    import ctypes
    from timberborn_support_solver_amd.solver import Mi355SatOpts, Mi355SatStats
    L = emu_lib()
    L.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (L.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (ctypes.sizeof(Mi355SatOpts), ctypes.sizeof(Mi355SatStats)) == (128, 248)
