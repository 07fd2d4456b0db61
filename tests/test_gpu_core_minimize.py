"""Irreducible failed-assumption cores on the MI355X: the rounds of mi355sat_minimize_core after the real search kernel
builds (which build ran is asserted through mi355sat_debug_last_search_build), ms_core_model_kernel on lists below and
above one ballot round, a 64-instance solve_batch, the interrupt and warm-mode rules and the C replay of the Rust shim's
call sequence.  The judge is the oracle alone (test_core_minimize.assert_minimal_core); every call runs under a deadline
whose interrupt would leave `minimal` 0, which the tests do not accept."""
import pytest

from oracle import oracle as ora
from simp_cases import within
from test_assumption_cores import PKG, assert_core, padded
from test_core_minimize import (anchors, assert_minimal_core, build_abi_core_minimize, minimized, run_abi_core_minimize,
                                wide_clause_case, with_padding)
from test_gpu_cores import assert_ran_the_build_asked_for, cached_sweep_cnf
from timberborn_support_solver_amd import Mi355Sat, SolverResult
from timberborn_support_solver_amd.solver import ColdReason

pytestmark = pytest.mark.gpu
LIMIT_S = 60


def minimized_within(s, a, cnf, n_vars):
    return within(LIMIT_S, s, lambda: minimized(s, a, cnf, n_vars))


@pytest.mark.parametrize("lds_val", [0, -1])
@pytest.mark.parametrize("one_per_simd", [0, 2, 4])
def test_forbidden_anchors_on_every_search_build(one_per_simd, lds_val):
    enc, cnf, a = anchors("rect16x16")
    s = Mi355Sat(one_per_simd=one_per_simd, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized_within(s, a, cnf, cnf.n_vars)
    assert_ran_the_build_asked_for(s, one_per_simd, lds_val)
    assert info["minimal"] == 1 and 0 < len(core) <= len(before) < len(a)
    assert within(LIMIT_S, s, s.solve) == SolverResult.Sat
    s.close()


def test_chunked_rounds_and_critical_literals_by_model():
    """Membership of the critical literals in the final core is checked by the substitute that
    test_core_minimize.test_chunked_rounds_and_critical_literals_by_model describes (the loop's own crit-inside-F check
    and the oracle's minimality check); the count alone is bounded here."""
    enc, cnf, a0 = anchors("rect16x16")
    a, nv = with_padding(a0, cnf.n_vars, 200)
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    s.debug_core_min_round(8)
    before, core, info = minimized_within(s, a, cnf, nv)
    assert not set(before) - set(a0)
    assert info["minimal"] == 1 and info["rounds"] > 1 and info["model_launches"] > 0
    assert info["critical_by_model"] <= len(core)
    s.close()


def test_lists_longer_than_one_ballot_round():
    cnf, a, want = wide_clause_case()
    s = Mi355Sat(simp=-1)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.set_phases([1] * (cnf.n_vars - 2))
    s.debug_core_min_round(2)
    before, core, info = minimized_within(s, a, cnf, cnf.n_vars)
    assert before == a
    assert core == want and info["minimal"] == 1
    assert info["model_launches"] > 0 and info["critical_by_model"] > 0 and info["candidates_unsat"] > 0
    s.close()


@pytest.mark.parametrize("terrain,k,k_max", [("rect16x16", 2, 8), ("rect16x16", 3, 8), ("rect24x24", 8, 12)])
def test_one_literal_core(terrain, k, k_max):
    enc, cnf = cached_sweep_cnf(terrain, "default", k_max)
    a, nv = padded(cnf, k)
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    before, core, info = minimized_within(s, a, cnf, nv)
    assert before == core == [-int(cnf.card_outputs[k])]
    assert info["minimal"] == 1 and info["candidates"] <= 1 and info["model_launches"] == 0
    s.close()


def test_batch_of_64_instances():
    enc, cnf = cached_sweep_cnf("rect16x16", "default", 8)
    nv = cnf.n_vars
    ks = [2, 3, 4, 5, 6, 3, 2, 7] * 8
    sets = [[nv + 1 + i, -int(cnf.card_outputs[k]), -(nv + 100 + i)] for i, k in enumerate(ks)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + 200)
    res = within(LIMIT_S, s, lambda: s.solve_batch(sets))
    assert [r == SolverResult.Unsat for r in res] == [k <= 3 for k in ks]
    cores = {i: s.core_of(i) for i, r in enumerate(res) if r == SolverResult.Unsat}
    for i in cores:
        info = within(LIMIT_S, s, lambda: s.minimize_core_of(i))
        assert info["minimal"] == 1 and s.core_of(i) == cores[i] == [-int(cnf.card_outputs[ks[i]])]
    model = s.solution_of(2, nv + 200)                      # the SAT instances' models stay readable
    assert ora.check_model(cnf.lits, cnf.offsets, model[:nv]) == -1
    s.close()


def test_interrupt_before_the_call_leaves_the_core():
    enc, cnf, a = anchors("rect16x16")
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    assert within(LIMIT_S, s, lambda: s.solve(a)) == SolverResult.Unsat
    before = s.core()
    s.interrupter().interrupt()
    info = s.minimize_core()
    assert info["minimal"] == 0 and info["candidates"] == 0 and s.core() == before
    assert_core(before, a, cnf, cnf.n_vars)
    info = within(LIMIT_S, s, s.minimize_core)              # the interrupt is consumed
    assert info["minimal"] == 1
    assert_minimal_core(s.core(), before, a, cnf, cnf.n_vars)
    assert within(LIMIT_S, s, s.solve) == SolverResult.Sat
    s.close()


def test_warm_mode_starts_cold_afterwards():
    enc, cnf, a = anchors("rect16x16")
    s = Mi355Sat()
    s.set_incremental(True)
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized_within(s, a, cnf, cnf.n_vars)
    assert info["minimal"] == 1 and info["candidates"] > 0
    assert within(LIMIT_S, s, lambda: s.solve(core[1:])) == SolverResult.Sat
    d = s.debug_incremental()
    assert d["last_cold_reason"] == ColdReason.OTHER_SEARCH and (d["warm_solves"], d["cold_solves"]) == (0, 2), d
    assert within(LIMIT_S, s, lambda: s.solve(core)) == SolverResult.Unsat and s.debug_incremental()["warm_solves"] == 1
    s.close()


def test_abi_core_minimize_call_sequence_on_the_device(tmp_path):
    exe = build_abi_core_minimize(tmp_path, PKG, "mi355sat")
    enc, cnf, a = anchors("rect16x16")
    before, core, info = run_abi_core_minimize(exe, tmp_path, cnf, 0, 8, a, timeout=300)
    assert info[0] == 1
    assert_minimal_core(core, before, a, cnf, cnf.n_vars)
