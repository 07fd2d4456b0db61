"""mi355sat_check_proof on the wavefront emulator (tests/emu): ms_rup_kernel in both builds, its host driver and the
bindings.  Cases and judge: tests/proof_check_cases.py - every expectation is the oracle's."""
import pytest

import proof_check_cases as pc
from fuzz_cases import EMU_CASES
from helpers import Csr, emu_lib, make_grid, platform_defs
from timberborn_support_solver_amd import ColdReason, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

UNSAT = pc.unsat_cases(EMU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; the checker never simplifies anyway)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def test_the_set_is_the_five_unsat_fuzz_cases():
    assert len(UNSAT) == 5
    sizes = [len(pc.oracle_proof(c)[1]) for c in UNSAT.values()]
    assert min(sizes) >= 12 and max(sizes) <= 111, sizes


@LDS
@pytest.mark.parametrize("name", list(pc.INSPECTION))
def test_emulated_check_by_inspection(name, lds_val):
    pc.run_inspection(emu_solver, name, lds_val=lds_val)


def test_emulated_check_argument_and_state_errors():
    pc.run_argument_errors(emu_solver, SolverError)


@LDS
@pytest.mark.parametrize("n", pc.LONG_N)
def test_emulated_long_lemmas(n, lds_val):
    pc.run_long(emu_solver, n, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("cut", pc.CUTS, ids=lambda c: f"segments-{c or 'all'}")
@pytest.mark.parametrize("name", list(UNSAT))
def test_emulated_verdict_does_not_depend_on_the_cut(name, cut, lds_val):
    pc.run_cut_independence(emu_solver, UNSAT[name], lds_val, cuts=(cut,))


@pytest.mark.parametrize("kind", pc.MUTANT_KINDS)
@pytest.mark.parametrize("name", list(UNSAT))
def test_emulated_mutants(name, kind):
    pc.run_mutants(emu_solver, UNSAT[name], kinds=(kind,))


def own_proof(tmp_path, pset, k, **opts):
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "own.drup")
    s = emu_solver(**opts)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    st = s.stats()
    s.close()
    return cnf, proof, st


def test_emulated_check_of_the_products_own_proof(tmp_path):
    cnf, proof, _ = own_proof(tmp_path, "1x1", 1, workers=1, slice_conflicts=40)
    pc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof)


def test_emulated_check_of_a_proof_with_deletion_lines(tmp_path):
    cnf, proof, st = own_proof(tmp_path, "1x1", 3, workers=3, slice_conflicts=16, reduce_first=25, reduce_inc=10,
                                deterministic=1)
    assert st["reduce_dbs"] > 0
    info = pc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof)
    assert info["n_deletions_ignored"] == sum(1 for line in open(proof) if line.startswith("d ")) > 0


def test_emulated_check_takes_the_device_over_and_leaves_the_ipasir_state():
    cnf, lemmas, want = pc.oracle_proof(UNSAT["3sat-n40-s3"])
    sat = Csr(pc.OPEN, 4)
    s = emu_solver(workers=2)
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
    assert after["solve_seconds"] > before["solve_seconds"]
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
    assert pc.answer(pc.check(emu_solver, cnf.clauses, cnf.n_vars, pc.flat(lemmas))) == want


def test_the_abi_sizes_are_unchanged():
    import ctypes
    L = emu_lib()
    L.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (L.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (128, 248)
