"""Phase hints on the MI355X (run with -m gpu): ms_phase_kernel in front of each of the six builds of the search kernel
(every build reads the phase byte in its own decision code), through the simplification's mappings, for the workers the
ramp-up creates later, for a batch, for a warm incremental solve and through `tbs_cli --phase-hints`.

The property is the one of tests/test_emu_phase.py: hinted to a model M of the formula, a solve makes no conflict and
returns M.  M is the oracle's; verdicts are the PicoSAT goldens'.  Every solve runs under solve_within."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, assert_search_build, check_sat_answer, make_grid, platform_defs
from oracle import oracle as ora
from test_emu_phase import assert_steered, golden_kstar, steering_case, warm_sequence
from test_gpu_builds import BUILDS, RECT16_1X1, wanted_build
from test_gpu_parity import HARD_RUNG_LIMIT_S, solve_within
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverResult

pytestmark = pytest.mark.gpu


class Limited(Mi355Sat):
    """solve() under the suite's wall-clock limit: an interrupt turns a hang into a failed assertion."""

    def solve(self, assumptions=()):
        for l in assumptions:
            self.assume(l)
        return solve_within(super(), HARD_RUNG_LIMIT_S)


def gpu_solver(**kw):
    kw.setdefault("workers", 256)
    kw.setdefault("ramp", -1)
    kw.setdefault("deterministic", 1)
    return Limited(**kw)


# ---- 1. each of the six search builds ---------------------------------------------------------------------------------
@BUILDS
def test_every_search_build_decides_by_the_hinted_phase(one_per_simd, lds_val):
    grid, enc, cnf, M = steering_case(gpu_solver, "rect8x8", "default", 20)
    s = assert_steered(gpu_solver, cnf, M, one_per_simd=one_per_simd, lds_val=lds_val, simp=-1)
    assert_search_build(s, *wanted_build(one_per_simd, lds_val))
    assert s.debug_phases()["launches"] == 1 and s.stats()["workers"] == 256
    s.close()


# ---- 2. through the mappings ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opts,exact", [("substitution", dict(simp=0), True), ("renumbering", dict(simp=-1, var_order=1), True),
                                             ("elimination", dict(simp=2), False)])
def test_hints_follow_their_variables_through_the_simplification(name, opts, exact):
    grid, enc, cnf, M = steering_case(gpu_solver, "rect16x16", "default", 40)
    s = assert_steered(gpu_solver, cnf, M, exact=exact, **opts)
    ph, st = s.debug_phases(), s.stats()
    if name == "elimination":
        assert 0 < ph["dropped_eliminated"] <= st["simp_eliminated"], (ph, st["simp_eliminated"])
    else:
        assert ph["dropped_eliminated"] == 0 and st["simp_eliminated"] == 0
    check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, 40)
    s.close()


# ---- 3. the workers the ramp-up creates later -------------------------------------------------------------------------
def test_workers_created_later_in_the_ramp_up_are_hinted_too():
    """Default ramp-up, 1024 workers: 256 have their slabs at the start, the others get theirs after 100 ms of kernel time
    (grow_workers) - and the hints.  The bound: rect 16x16 with 1x1 supports only at its optimum k = 15 (SAT; PicoSAT 67.5 s,
    test_gpu_builds.RECT16_1X1 / test_gpu_parity), which takes 0.3-0.7 s here.  The SAT bounds of verdicts.json do not
    outlast the first stage reliably: measured on the MI355X, k = 16 takes 42-145 ms of kernel time whatever the hints
    (all FALSE, all TRUE, random, a negated model, a loose layout), k = 18 / 20 20-60 ms.  The hints are the default
    spelled out (every variable FALSE first), so the search is the unhinted one; a conflict budget bounds the run.  The
    slabs an earlier handle parked would cover all 1024 workers from the start: released first."""
    from timberborn_support_solver_amd import _lib
    k = [v for v in RECT16_1X1 if v["verdict"] == "SAT"][0]["k"]
    assert k == 15
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    _lib.solver_lib().mi355sat_release_cached_memory()
    s = Limited(workers=1024, conflict_budget=50_000_000)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.set_phases(-np.ones(enc.n_vars, dtype=np.int8))
    r = s.solve()
    ph, st = s.debug_phases(), s.stats()
    print("ramp-up:", r, ph, "kernel s", st["kernel_seconds"], "conflicts", st["conflicts"], "workers", st["workers"])
    assert r == SolverResult.Sat
    check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
    assert ph["applied_cold"] == 1 and ph["launches"] >= 2, ph
    s.close()


# ---- 4. a batch ---------------------------------------------------------------------------------------------------------
def test_solve_batch_with_hints_gives_the_golden_verdicts():
    kstar = golden_kstar("rect16x16", "default")
    assert kstar == 4
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    ks = list(range(7, -1, -1))
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): ks[0]}), sweep=True)
    card = [int(l) for l in cnf.card_outputs]
    sets = [[-card[k]] if k < len(card) else [] for k in ks]
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(cnf.n_vars)
    assert o.solve(sets[ks.index(kstar)]) == 10
    M = o.model(cnf.n_vars)
    s = Mi355Sat(workers=64 * len(ks), conflict_budget=50_000_000)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.set_phases(M[:enc.n_vars])
    res = s.solve_batch(sets)
    ph = s.debug_phases()
    assert ph["applied_cold"] == 1 and ph["hinted"] == enc.n_vars and ph["launches"] >= 1 and ph["mapped"] > 0, ph
    for i, k in enumerate(ks):
        assert res[i] == (SolverResult.Sat if k >= kstar else SolverResult.Unsat), (k, res[i])
        if res[i] == SolverResult.Sat:
            check_sat_answer(cnf, s.solution_of(i, cnf.n_vars), enc, grid, k)
    s.close()


# ---- 5. warm incremental ------------------------------------------------------------------------------------------------
def test_a_warm_solve_is_seeded_once_when_the_hints_changed_and_never_again():
    warm_sequence(gpu_solver, "rect8x8", "1x1", 20).close()


# ---- 6. the command line ------------------------------------------------------------------------------------------------
def test_cli_with_phase_hints_ends_where_it_ends_without():
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    ends = []
    for flag in ([], ["--phase-hints"]):
        out = subprocess.run([cli, "rect", "16", "16", "-l1:16", "--workers", "256"] + flag, capture_output=True, text=True, timeout=120)
        lines = out.stdout.strip().splitlines()
        assert out.returncode == 0 and "Solution validation FAILED" not in lines and "Solution validation OK" in lines, out.stderr
        ends.append((lines[-1], [l for l in lines if l.startswith("Solution found")][-1]))
    assert ends[0] == ends[1] == ("No solution found for the current constraints", "Solution found (4 platforms total)")   # k* = 4
