"""DRUP proofs of solve_batch and the stepwise sweep, ms_proof_gather_kernel and the check of several targets in one pass on
the MI355X (run with -m gpu).  Cases and judges: tests/sweep_proof_cases.py - every expectation is the oracle's or a
PicoSAT golden's, never the product's."""
import pytest

import lrat_check
import proof_check_cases as pc
import sweep_cases as sc
import sweep_proof_cases as sp
from fuzz_cases import BUILD_IDS, BUILD_LIST, EMU_CASES, wanted_build
from helpers import VERDICTS, assert_search_build, make_grid, platform_defs
from oracle import oracle as ora
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError

pytestmark = pytest.mark.gpu

UNSAT = pc.unsat_cases(EMU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def gpu_solver(**kw):
    kw.setdefault("simp", -1)
    return Mi355Sat(**kw)


@pytest.mark.parametrize("name", sp.BATCH_CASES)
def test_batch_logs_a_proof_that_certifies_every_unsat_instance(name, tmp_path):
    sp.run_batch_and_check(gpu_solver, name, tmp_path)


@pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST, ids=BUILD_IDS)
def test_batch_proof_in_every_build_of_the_search_kernel(one_per_simd, lds_val, tmp_path):
    sp.run_batch_and_check(gpu_solver, "3sat-n50-s5", tmp_path, one_per_simd=one_per_simd, lds_val=lds_val,
                           inspect=lambda s: assert_search_build(s, *wanted_build(one_per_simd, lds_val)))


def test_batch_proof_of_a_fleet_of_mostly_empty_logs(tmp_path):
    """2304 workers on 3sat-n50-s5, all from the first slice on (ramp = -1: the ramp-up would decide the batch with its
    first 256): the 4-waves build, and thousands of logs of which a slice fills some."""
    seen = {}

    def inspect(s):
        seen.update(s.debug_last_search_build(), workers=s.stats()["workers"])

    _, _, log = sp.run_batch_and_check(gpu_solver, "3sat-n50-s5", tmp_path, workers=2304, ramp=-1, inspect=inspect)
    print("fleet:", seen, "proof log:", log)
    assert seen["workers"] == 2304 and seen["active"] == 2304 and seen["wps"] == 4, seen
    assert 0 < log["logs"] < log["gathers"] * 2304, log


def test_scheduled_sweep_logs_a_proof(tmp_path):
    path = str(tmp_path / "sweep.drup")
    cnf, _ = sc.formula(sp.SCHEDULE_CASE)
    cores, _ = sp.run_scheduled_sweep(gpu_solver, sp.SCHEDULE_CASE, sp.SCHEDULE_SEEDS[0], path)
    order = sorted(cores)
    info = sp.check_targets_on_fresh_handle(gpu_solver, cnf, path, [sp.negated(cores[i]) for i in order])
    assert info["valid"] == 1 and info["target_valid"] == [1] * len(order), info


@LDS
def test_one_target_equals_check_proof(lds_val):
    sp.run_one_target_equals_check_proof(gpu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", list(sp.TARGET_CASES))
def test_targets_by_inspection(name, lds_val):
    sp.run_target_case(gpu_solver, name, lds_val=lds_val)


@LDS
def test_deleted_lemma_that_only_a_target_needs(lds_val):
    sp.run_deleted_lemma_only_a_target_needs(gpu_solver, lds_val=lds_val)


@pytest.mark.parametrize("name", list(UNSAT))
def test_targets_on_the_oracles_proofs(name):
    sp.run_fuzz_targets(gpu_solver, UNSAT[name])


def test_target_argument_and_state_errors():
    sp.run_target_errors(gpu_solver, SolverError)


def test_rect8_ladder_as_one_batch_is_certified_in_one_pass(tmp_path):
    """rect 8x8, 1x1 supports: the bounds 0 .. 6 as assumptions over one totalizer, as solver_loop_sweep poses them.  One
    file, one check_proof_targets_file call for every UNSAT bound; the lowest UNSAT bound trimmed to LRAT."""
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    k0 = 6
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    ks = list(range(k0, -1, -1))
    sets = [([-int(cnf.card_outputs[k])] if k < len(cnf.card_outputs) else []) for k in ks]
    golden = {v["k"]: v["verdict"] for v in VERDICTS["verdicts"] if (v["terrain"], v["platforms"]) == ("rect8x8", "1x1")}
    want = []
    for k, a in zip(ks, sets):
        if k in golden:
            want.append(10 if golden[k] == "SAT" else 20)
        else:
            o = ora.OracleSolver()
            o.add_cnf(cnf.lits, cnf.offsets)
            o.reserve(cnf.n_vars)
            want.append(o.solve(a))
    assert 20 in want
    path = str(tmp_path / "ladder.drup")
    s = Mi355Sat(workers=64)
    s.set_proof_path(path)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    res = s.solve_batch(sets)
    assert [r.value for r in res] == want, (res, want)
    unsat = [i for i, w in enumerate(want) if w == 20]
    cores = {i: s.core_of(i) for i in unsat}
    s.close()
    clauses = [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    info = s.check_proof_targets_file(path, [sp.negated(cores[i]) for i in unsat])
    assert info["valid"] == 1 and info["target_valid"] == [1] * len(unsat), info
    lowest = unsat[-1]                       # (the bounds come in decreasing order)
    target = sp.negated(cores[lowest])
    t = s.trim_proof_file(path, target=target, hints=True)
    assert t["check"]["valid"] == 1, t
    lrat = str(tmp_path / "lowest.lrat")
    s.trim_write_lrat(lrat)
    s.close()
    lrat_check.check(clauses, open(lrat).read())
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    got = s.check_lrat_file(lrat, target=target)
    s.close()
    assert (got["valid"], got["accepted"], got["derives_target"]) == (1, 1, 1), got
