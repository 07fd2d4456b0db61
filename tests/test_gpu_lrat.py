"""mi355sat_check_lrat on the MI355X: ms_lrat_kernel in both builds, on the cases of tests/test_emu_lrat.py plus the larger
fuzz proofs, the fleet's own certificates and `tbs_cli --certify PATH --verify`.  Cases and judge:
tests/lrat_device_cases.py; the judge is the plain-Python checker tests/lrat_check.py."""
import os
import subprocess

import pytest

import lrat_device_cases as lc
import proof_check_cases as pc
from fuzz_cases import GPU_CASES
from helpers import ROOT, make_grid, platform_defs
from test_assumption_cores import padded, sweep_cnf
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult, _lib
from timberborn_support_solver_amd.dimacs import read_drup

pytestmark = pytest.mark.gpu

UNSAT = pc.unsat_cases(GPU_CASES)
LDS = pytest.mark.parametrize("lds_val", lc.LDS_BUILDS, ids=lc.LDS_IDS)
MUTATED = ("3sat-n60-s2", "3sat-n120-s5")


def gpu_solver(**kw):
    return Mi355Sat(**kw)


# ---- 1. by hand -----------------------------------------------------------------------------------------------------------------
@LDS
def test_lrat_accepts_the_refutation_written_by_hand(lds_val):
    lc.run_xor2_accepted(gpu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", list(lc.XOR2_REJECTED))
def test_lrat_rejects(name, lds_val):
    lc.run_xor2_rejected(gpu_solver, name, lds_val=lds_val)


# ---- 2. the clause scan at its edges ------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n", lc.SCAN_N)
def test_lrat_clause_scan_edges(n, lds_val):
    lc.run_scan(gpu_solver, n, lds_val=lds_val)


# ---- 3. the assignment map at its edges ----------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n_vars", lc.MAP_N)
def test_lrat_map_edges(n_vars, lds_val):
    lc.run_map_edges(gpu_solver, n_vars, lds_val=lds_val)


# ---- 4. real files and their mutants ---------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("name", list(UNSAT))
def test_lrat_of_the_trimmed_fuzz_proofs(name, lds_val, tmp_path):
    lc.run_real_file(gpu_solver, UNSAT[name], tmp_path, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("kind", lc.MUTANT_KINDS)
@pytest.mark.parametrize("name", MUTATED)
def test_lrat_mutants(name, kind, lds_val):
    lc.run_mutants(gpu_solver, UNSAT[name], kind, lds_val=lds_val)


# ---- 5. independence of the cut ----------------------------------------------------------------------------------------------------------
@LDS
def test_lrat_verdict_does_not_depend_on_the_cut(lds_val):
    lc.run_cut_independence(gpu_solver, UNSAT[MUTATED[0]], lds_val=lds_val)


# ---- 6. the product's own certificates ------------------------------------------------------------------------------------------------------
@LDS
def test_lrat_of_the_products_own_certificate(lds_val, tmp_path):
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 1}))
    proof = str(tmp_path / "own.drup")
    s = gpu_solver(workers=1, simp=-1)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    s.close()
    lc.run_own_certificate(gpu_solver, cnf, cnf.n_vars, proof, tmp_path, lds_val=lds_val)


@LDS
def test_lrat_of_a_certificate_under_assumptions(lds_val, tmp_path):
    """rect 8x8, default platforms, under assumptions: the target is the negated core, the file's last line."""
    enc, cnf = sweep_cnf("rect8x8", "default", 4)
    a, nv = padded(cnf, 1)
    proof = str(tmp_path / "p.drup")
    s = gpu_solver(workers=4)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    s.close()
    lemmas, _ = pc.lemmas_of(read_drup(proof))
    target = lemmas.pop()                      # the file's last line: the negated core
    assert sorted(target) == sorted(-l for l in core) and target
    body = str(tmp_path / "body.drup")
    with open(body, "w") as f:
        f.writelines(open(proof).read().splitlines(keepends=True)[:-1])
    lc.run_own_certificate(gpu_solver, cnf, nv, body, tmp_path, target=target, wrong_target=(), lds_val=lds_val)


def test_cli_certify_verify_ends_with_the_verified_line(tmp_path):
    """`tbs_cli --certify PATH --verify` checks PATH.lrat on the device and says so in one more line; without --verify the
    `Certificate:` line stays the last."""
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    path = str(tmp_path / "bound.drup")
    base = [cli, "rect", "8", "8", "-l1:8", "--workers", "64", "--certify", path]
    out = subprocess.run(base + ["--verify"], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-2].startswith("Certificate: " + path + ".lrat - core "), (out.stdout, out.stderr)
    assert lines[-1].startswith("Verified: " + path + ".lrat - ") and lines[-1].endswith(" s"), lines
    n_lines, n_hints = (int(lines[-1].split(" - ")[1].split(", ")[i].split()[0]) for i in (0, 1))
    parsed = lc.lrat_check.parse(open(path + ".lrat").read())
    assert (n_lines, n_hints) == (len(parsed), sum(len(h) for _, _, h in parsed)) and n_lines > 0, lines[-1]
    out = subprocess.run(base, capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1].startswith("Certificate: " + path + ".lrat - core "), (out.stdout, out.stderr)
    assert not any(l.startswith("Verified") for l in lines), lines


# ---- 7. state and ABI ------------------------------------------------------------------------------------------------------------------------
@LDS
def test_lrat_refuses_what_is_not_lrat(lds_val, tmp_path):
    lc.run_malformed(gpu_solver, SolverError, tmp_path, lds_val=lds_val)


@LDS
def test_lrat_state_and_abi(lds_val, tmp_path):
    lc.run_state_and_abi(gpu_solver, SolverError, _lib.solver_lib(), tmp_path, lds_val=lds_val)


@LDS
def test_lrat_leaves_the_handle_alone(lds_val, tmp_path):
    lc.run_leaves_the_handle_alone(gpu_solver, SolverResult, tmp_path, lds_val=lds_val)
