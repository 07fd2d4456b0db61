"""mi355sat_trim_proof on the wavefront emulator (tests/emu): the tracing build of ms_rup_kernel in both builds, the drain
of its dependency log, the host's backward reach and the bindings.  Cases and judges: tests/proof_trim_cases.py - the
oracle on the core and the needed lemmas alone, and the plain-Python LRAT checker tests/lrat_check.py, which is tested here
first."""
import pytest

import lrat_check
import proof_check_cases as pc
import proof_trim_cases as tc
from fuzz_cases import EMU_CASES
from helpers import emu_lib, make_grid, platform_defs
from timberborn_support_solver_amd import ColdReason, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

UNSAT = pc.unsat_cases(EMU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; the checker never simplifies anyway)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


# ---- judge (b) itself ---------------------------------------------------------------------------------------------------------
# XOR2 = (1 2) (-1 2) (1 -2) (-1 -2): 2 by clauses 1 and 2 under -2; then the empty clause by 5, 3 and 4
XOR2_LRAT = ["5 2 0 1 2 0", "6 0 5 3 4 0"]


def lrat(lines):
    return "".join(l + "\n" for l in lines)


def test_the_lrat_checker_accepts_a_refutation_written_by_hand():
    used, lines = lrat_check.check(pc.XOR2, lrat(XOR2_LRAT))
    assert used == {1, 2, 3, 4} and [l[0] for l in lines] == [5, 6] and lines[-1][1] == []


@pytest.mark.parametrize("name, lines", [
    ("a hint removed", ["5 2 0 1 2 0", "6 0 5 4 0"]),
    ("the only unit hint removed", ["5 2 0 2 0", "6 0 5 3 4 0"]),
    ("two hints swapped", ["5 2 0 1 2 0", "6 0 3 5 4 0"]),
    ("a hint that names a later line", ["5 2 0 1 6 0", "6 0 5 3 4 0"]),
    ("the last line dropped, its id hinted", ["5 2 0 1 2 0", "7 0 6 3 4 0"]),
    ("ids not increasing", ["6 2 0 1 2 0", "5 0 6 3 4 0"]),
    ("an id of an original", ["4 2 0 1 2 0"]),
    ("a satisfied hint", ["5 2 0 1 2 0", "6 0 5 5 3 4 0"]),
    ("a falsified hint before the last", ["5 2 0 1 2 0", "6 0 5 3 4 4 0"]),
    ("no hints", ["5 2 0 0"]),
])
def test_the_lrat_checker_rejects(name, lines):
    with pytest.raises(lrat_check.LratError):
        lrat_check.check(pc.XOR2, lrat(lines))


def test_the_lrat_checker_reports_a_file_that_does_not_reach_the_empty_clause():
    """Dropping the last line leaves a valid file that derives (2) only: the caller sees it in the lines returned."""
    used, lines = lrat_check.check(pc.XOR2, lrat(XOR2_LRAT[:1]))
    assert used == {1, 2} and lines[-1][1] == [2]


def test_the_set_is_the_five_unsat_fuzz_cases():
    assert len(UNSAT) == 5
    sizes = [len(pc.oracle_proof(c)[1]) for c in UNSAT.values()]
    assert min(sizes) >= 12 and max(sizes) <= 111, sizes


# ---- 1. by inspection -----------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_trim_case_a_exact_sets(lds_val):
    tc.run_case_a(emu_solver, lds_val=lds_val)


@LDS
def test_emulated_trim_case_b_the_stripped_literal(lds_val):
    tc.run_case_b(emu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", tc.INHERITED_VALID)
def test_emulated_trim_by_inspection(name, lds_val):
    tc.run_inherited_valid(emu_solver, name, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", tc.INHERITED_INVALID)
def test_emulated_trim_of_an_invalid_proof_leaves_no_result(name, lds_val):
    tc.run_inherited_invalid(emu_solver, SolverError, name, lds_val=lds_val)


# ---- 2. long reasons ------------------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n", tc.LONG_N)
def test_emulated_trim_long_reasons(n, lds_val):
    tc.run_long(emu_solver, n, lds_val=lds_val)


# ---- 3. padded fuzz proofs --------------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("cut", pc.CUTS, ids=lambda c: f"segments-{c or 'all'}")
@pytest.mark.parametrize("name", list(UNSAT))
def test_emulated_trim_of_the_padded_fuzz_proofs(name, cut, lds_val):
    tc.run_padded(emu_solver, UNSAT[name], lds_val, cuts=(cut,))


# ---- 4. the log at its edges --------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_trim_log_at_its_edges(lds_val):
    tc.run_log_edges(emu_solver, UNSAT["3sat-n40-s3"], lds_val)


# ---- 5. mutants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.MUTANT_KINDS)
def test_emulated_trim_mutants(kind):
    tc.run_mutants(emu_solver, SolverError, UNSAT["3sat-n40-s3"], kinds=(kind,))


# ---- 6. the product's own proofs ------------------------------------------------------------------------------------------------------
def test_emulated_trim_of_the_products_own_proof(tmp_path):
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 1}))
    proof = str(tmp_path / "own.drup")
    s = emu_solver(workers=1, slice_conflicts=40)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    s.close()
    tc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof, tmp_path)


# ---- 7. state and ABI ---------------------------------------------------------------------------------------------------------------
def test_emulated_trim_state_and_abi():
    tc.run_state_and_abi(emu_solver, SolverError, emu_lib())


def test_emulated_trim_takes_the_device_over_and_leaves_the_ipasir_state():
    tc.run_device_takeover(emu_solver, SolverResult, ColdReason)


def test_the_abi_sizes_are_unchanged():
    import ctypes
    L = emu_lib()
    L.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (L.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (128, 248)
