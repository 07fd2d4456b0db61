"""mi355sat_check_proof on the MI355X: ms_rup_kernel in both builds, on the cases of tests/test_emu_proof_check.py plus the
larger fuzz proofs and the default fleet's own proofs.  Cases and judge: tests/proof_check_cases.py - every expectation is
the oracle's."""
import pytest

import proof_check_cases as pc
from fuzz_cases import GPU_CASES
from helpers import Csr, make_grid, platform_defs
from test_assumption_cores import padded, sweep_cnf
from timberborn_support_solver_amd import ColdReason, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult
from timberborn_support_solver_amd.dimacs import read_drup

pytestmark = pytest.mark.gpu

UNSAT = pc.unsat_cases(GPU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def gpu_solver(**kw):
    return Mi355Sat(**kw)


@LDS
@pytest.mark.parametrize("name", list(pc.INSPECTION))
def test_check_by_inspection(name, lds_val):
    pc.run_inspection(gpu_solver, name, lds_val=lds_val)


def test_check_argument_and_state_errors():
    pc.run_argument_errors(gpu_solver, SolverError)


@LDS
@pytest.mark.parametrize("n", pc.LONG_N)
def test_long_lemmas(n, lds_val):
    pc.run_long(gpu_solver, n, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("cut", pc.CUTS, ids=lambda c: f"segments-{c or 'all'}")
@pytest.mark.parametrize("name", list(UNSAT))
def test_verdict_does_not_depend_on_the_cut(name, cut, lds_val):
    pc.run_cut_independence(gpu_solver, UNSAT[name], lds_val, cuts=(cut,))


@pytest.mark.parametrize("kind", pc.MUTANT_KINDS)
@pytest.mark.parametrize("name", list(UNSAT))
def test_mutants(name, kind):
    pc.run_mutants(gpu_solver, UNSAT[name], kinds=(kind,))


def own_proof(tmp_path, terrain, pset, k, **opts):
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "own.drup")
    s = gpu_solver(**opts)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    st = s.stats()
    s.close()
    return cnf, proof, st


def test_check_of_the_products_own_proof(tmp_path):
    # (one worker and no probing before the search: the refutation falls with the worker's last lemmas, so that half of
    # the file is no proof - run_own_proof asserts that the oracle says so)
    cnf, proof, _ = own_proof(tmp_path, "rect8x8", "1x1", 1, workers=1, simp=-1)
    pc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof)


def test_check_of_a_proof_with_deletion_lines(tmp_path):
    cnf, proof, st = own_proof(tmp_path, "rect8x8", "1x1", 3, workers=3, slice_conflicts=16, reduce_first=25, reduce_inc=10,
                                deterministic=1)
    assert st["reduce_dbs"] > 0
    info = pc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof)
    assert info["n_deletions_ignored"] == sum(1 for line in open(proof) if line.startswith("d ")) > 0


def test_check_of_a_fleets_proof(tmp_path):
    """rect 16x16, default platforms, k = 3, 16 workers: device lemmas of many literals, clauses that crossed the exchange,
    and (with an early reduction) deletion lines.  Its slices are bounded by time, so the order of the file's lines differs
    from run to run and half of it may or may not be a proof: on the half, the device must say what the oracle says."""
    cnf, proof, st = own_proof(tmp_path, "rect16x16", "default", 3, workers=16, reduce_first=200, reduce_inc=50)
    info = pc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof, half_is_no_proof=False)
    lemmas, _ = pc.lemmas_of(read_drup(proof))
    print("fleet proof:", info, "longest lemma", max(len(c) for c in lemmas), "imported", st["shared_imported"])
    assert info["workers"] > 1


def test_check_of_a_proof_under_assumptions(tmp_path):
    enc, cnf = sweep_cnf("rect8x8", "default", 4)
    a, nv = padded(cnf, 1)
    proof = str(tmp_path / "p.drup")
    s = gpu_solver(workers=4)                  # (a short proof: the reference walks it lemma by lemma on the host)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    s.close()
    lemmas, _ = pc.lemmas_of(read_drup(proof))
    target = lemmas.pop()                      # the file's last line: the negated core
    assert sorted(target) == sorted(-l for l in core) and target
    clauses = [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]
    for tg in (target, target[1:]):
        want = pc.reference(clauses, nv, lemmas, tg, refuted=False)
        s = gpu_solver()
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(nv)
        info = s.check_proof(pc.flat(lemmas), target=tg)
        s.close()
        assert (info["valid"], info["first_failed"]) == want[:2], (tg, info, want)
        if tg == target:
            assert info["valid"] == 1


def test_check_takes_the_device_over_and_leaves_the_ipasir_state():
    cnf, lemmas, want = pc.oracle_proof(UNSAT["3sat-n40-s3"])
    sat = Csr(pc.OPEN, 4)
    s = gpu_solver(workers=2)
    s.set_incremental(True)
    s.add_cnf(sat.lits, sat.offsets)
    assert s.solve([-2]) == SolverResult.Unsat
    core = s.core()
    assert core == [-2]
    assert s.solve([-2]) == SolverResult.Unsat and s.debug_incremental()["warm_solves"] == 1
    before = s.stats()
    info = s.check_proof(pc.flat([[2]]), target=(2,))
    assert pc.answer(info) == (1, None, None)
    after = s.stats()
    assert s.core() == core and s.failed(-2)                       # the IPASIR state of the solve before
    assert [after[k] for k in ("n_sat", "n_unsat", "n_terminated")] == [before[k] for k in ("n_sat", "n_unsat", "n_terminated")]
    assert after["kernel_launches"] == before["kernel_launches"] + info["launches"] and info["launches"] >= 1
    assert after["solve_seconds"] > before["solve_seconds"] and after["kernel_seconds"] > before["kernel_seconds"]
    cold = s.debug_incremental()["cold_solves"]
    assert s.solve() == SolverResult.Sat
    inc = s.debug_incremental()
    assert inc["cold_solves"] == cold + 1 and inc["last_cold_reason"] == ColdReason.OTHER_SEARCH
    assert s.full_solution(4)[1] > 0
    # an interrupt that came before the call: Interrupted, nothing launched, and consumed
    s.interrupter().interrupt()
    stopped = s.check_proof(pc.flat([[2]]), target=(2,))
    assert stopped["interrupted"] and stopped["valid"] == -1 and stopped["launches"] == 0
    assert pc.answer(s.check_proof(pc.flat([[2]]), target=(2,))) == (1, None, None)
    s.close()
    # new, add_cnf, check_proof: the handle need not have solved anything
    assert pc.answer(pc.check(gpu_solver, cnf.clauses, cnf.n_vars, pc.flat(lemmas))) == want
