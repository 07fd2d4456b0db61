"""mi355sat_check_lrat on the wavefront emulator (tests/emu): ms_lrat_kernel in both builds - the assignment map in LDS and
the stamped one in HBM - the host's parser, the rewriting of hint ids and the bindings.  Cases and judge:
tests/lrat_device_cases.py; the judge is the plain-Python checker tests/lrat_check.py."""
import os
import subprocess

import pytest

import lrat_device_cases as lc
import proof_check_cases as pc
from fuzz_cases import EMU_CASES
from helpers import ROOT, emu_lib, make_grid, platform_defs
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

UNSAT = pc.unsat_cases(EMU_CASES)
LDS = pytest.mark.parametrize("lds_val", lc.LDS_BUILDS, ids=lc.LDS_IDS)
MUTATED = "3sat-n60-s2"


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; the checker never simplifies anyway)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


# ---- 1. by hand -----------------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_lrat_accepts_the_refutation_written_by_hand(lds_val):
    lc.run_xor2_accepted(emu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", list(lc.XOR2_REJECTED))
def test_emulated_lrat_rejects(name, lds_val):
    lc.run_xor2_rejected(emu_solver, name, lds_val=lds_val)


# ---- 2. the clause scan at its edges ------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n", lc.SCAN_N)
def test_emulated_lrat_clause_scan_edges(n, lds_val):
    lc.run_scan(emu_solver, n, lds_val=lds_val)


# ---- 3. the assignment map at its edges ----------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n_vars", lc.MAP_N)
def test_emulated_lrat_map_edges(n_vars, lds_val):
    lc.run_map_edges(emu_solver, n_vars, lds_val=lds_val)


# ---- 4. real files and their mutants ---------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("name", list(UNSAT))
def test_emulated_lrat_of_the_trimmed_fuzz_proofs(name, lds_val, tmp_path):
    lc.run_real_file(emu_solver, UNSAT[name], tmp_path, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("kind", lc.MUTANT_KINDS)
def test_emulated_lrat_mutants(kind, lds_val):
    lc.run_mutants(emu_solver, UNSAT[MUTATED], kind, lds_val=lds_val)


# ---- 5. independence of the cut ----------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_lrat_verdict_does_not_depend_on_the_cut(lds_val):
    lc.run_cut_independence(emu_solver, UNSAT[MUTATED], lds_val=lds_val)


# ---- 6. the product's own certificate ------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_lrat_of_the_products_own_certificate(lds_val, tmp_path):
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 1}))
    proof = str(tmp_path / "own.drup")
    s = emu_solver(workers=1, slice_conflicts=40)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    s.close()
    lc.run_own_certificate(emu_solver, cnf, cnf.n_vars, proof, tmp_path, lds_val=lds_val)


# ---- 7. state and ABI ------------------------------------------------------------------------------------------------------------------------
@LDS
def test_emulated_lrat_refuses_what_is_not_lrat(lds_val, tmp_path):
    lc.run_malformed(emu_solver, SolverError, tmp_path, lds_val=lds_val)


@LDS
def test_emulated_lrat_state_and_abi(lds_val, tmp_path):
    lc.run_state_and_abi(emu_solver, SolverError, emu_lib(), tmp_path, lds_val=lds_val)


@LDS
def test_emulated_lrat_leaves_the_handle_alone(lds_val, tmp_path):
    lc.run_leaves_the_handle_alone(emu_solver, SolverResult, tmp_path, lds_val=lds_val)


def test_the_lrat_parser_under_the_sanitizers(tmp_path):
    """The host's parser and validation, with the malformed inputs of item 7, in a stand-alone program built with
    -fsanitize=address,undefined from the emulator's translation unit (tests/lrat_parse_san.cpp): no Python, nothing preloaded."""
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else "clang++"
    src = os.path.join(ROOT, "timberborn_support_solver_amd", "csrc")
    emu = os.path.join(ROOT, "tests", "emu")
    exe = str(tmp_path / "lrat_parse_san")
    # (-O0: the build is the test's time; a UBSan report ends the program: no recovery at build time, halt_on_error at run time)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + emu, "-I" + src, "-Wno-unknown-pragmas", "-Wno-unused-command-line-argument",
                           "-DEMU_UCONTEXT", "-o", exe, os.path.join(ROOT, "tests", "lrat_parse_san.cpp"), os.path.join(emu, "emu.cpp"),
                           "-x", "c++", os.path.join(src, "mi355sat.hip")])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0",
                                  UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("lrat_parse_san OK"), (out.stdout, out.stderr[-4000:])
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
