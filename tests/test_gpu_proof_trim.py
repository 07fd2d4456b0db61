"""mi355sat_trim_proof on the MI355X: the tracing build of ms_rup_kernel in both builds, on the cases of
tests/test_emu_proof_trim.py plus the larger fuzz proofs and the default fleet's own proofs.  Cases and judges:
tests/proof_trim_cases.py - the oracle on the core and the needed lemmas alone, and the plain-Python LRAT checker."""
import os
import subprocess

import pytest

import lrat_check
import proof_check_cases as pc
import proof_trim_cases as tc
from fuzz_cases import GPU_CASES
from helpers import ROOT, make_grid, platform_defs
from test_assumption_cores import padded, sweep_cnf
from timberborn_support_solver_amd import ColdReason, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult, _lib
from timberborn_support_solver_amd.dimacs import read_drup

pytestmark = pytest.mark.gpu

UNSAT = pc.unsat_cases(GPU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def gpu_solver(**kw):
    return Mi355Sat(**kw)


def test_the_set_is_the_ten_unsat_fuzz_cases():
    assert len(UNSAT) == 10
    assert max(len(pc.oracle_proof(c)[1]) for c in UNSAT.values()) == 1861


# ---- 1. by inspection -----------------------------------------------------------------------------------------------------------
@LDS
def test_trim_case_a_exact_sets(lds_val):
    tc.run_case_a(gpu_solver, lds_val=lds_val)


@LDS
def test_trim_case_b_the_stripped_literal(lds_val):
    tc.run_case_b(gpu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", tc.INHERITED_VALID)
def test_trim_by_inspection(name, lds_val):
    tc.run_inherited_valid(gpu_solver, name, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", tc.INHERITED_INVALID)
def test_trim_of_an_invalid_proof_leaves_no_result(name, lds_val):
    tc.run_inherited_invalid(gpu_solver, SolverError, name, lds_val=lds_val)


# ---- 2. long reasons ------------------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("n", tc.LONG_N)
def test_trim_long_reasons(n, lds_val):
    tc.run_long(gpu_solver, n, lds_val=lds_val)


# ---- 3. padded fuzz proofs --------------------------------------------------------------------------------------------------------
@LDS
@pytest.mark.parametrize("cut", pc.CUTS, ids=lambda c: f"segments-{c or 'all'}")
@pytest.mark.parametrize("name", list(UNSAT))
def test_trim_of_the_padded_fuzz_proofs(name, cut, lds_val):
    tc.run_padded(gpu_solver, UNSAT[name], lds_val, cuts=(cut,))


# ---- 4. the log at its edges --------------------------------------------------------------------------------------------------------
@LDS
def test_trim_log_at_its_edges(lds_val):
    tc.run_log_edges(gpu_solver, UNSAT["3sat-n100-s6"], lds_val)


# ---- 5. mutants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.MUTANT_KINDS)
def test_trim_mutants(kind):
    tc.run_mutants(gpu_solver, SolverError, UNSAT["3sat-n60-s2"], kinds=(kind,))


# ---- 6. the product's own proofs ------------------------------------------------------------------------------------------------------
def own_proof(tmp_path, terrain, pset, k, **opts):
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "own.drup")
    s = gpu_solver(**opts)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    s.close()
    return cnf, proof


def test_trim_of_the_products_own_proof(tmp_path):
    cnf, proof = own_proof(tmp_path, "rect8x8", "1x1", 1, workers=1, simp=-1)
    tc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof, tmp_path)


def test_trim_of_a_proof_under_assumptions(tmp_path):
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
    tc.run_own_proof(gpu_solver, cnf, nv, body, tmp_path, target=target)      # (judge: the LRAT's last line is the target)


def test_trim_of_a_fleets_proof(tmp_path):
    """rect 16x16, default platforms, k = 3, 16 workers: long lemmas, exchanged clauses, deletion lines."""
    cnf, proof = own_proof(tmp_path, "rect16x16", "default", 3, workers=16, reduce_first=200, reduce_inc=50)
    res = tc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof, tmp_path)
    print("fleet proof:", len(res["lemmas"]), "of", res["check"]["n_lemmas"], "lemmas needed;", len(res["core"]), "of",
          len(cnf.offsets) - 1, "clauses in the core;", res["check"], res["dep_records"], "records", res["log_drains"], "drains")
    assert res["check"]["workers"] > 1


def test_cli_certify_writes_an_lrat_file_the_checker_accepts(tmp_path):
    """`tbs_cli --certify PATH`: the bound the loop ends on, its proof trimmed on a fresh handle, PATH.lrat judged by the
    plain-Python checker against the same bound's CNF from the encoder."""
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    path = str(tmp_path / "bound.drup")
    out = subprocess.run([cli, "rect", "8", "8", "-l1:8", "--workers", "64", "--certify", path], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and "No solution found for the current constraints" in lines, (out.stdout, out.stderr)
    assert lines[-1].startswith("Certificate: " + path + ".lrat - core "), lines
    k = int([l for l in lines if l.startswith("Solution found")][-1].split("(")[1].split()[0]) - 1
    enc = Encoding.encode(platform_defs("default"), make_grid("rect8x8"))
    clauses = tc.clauses_of(enc.with_limits_into_cnf(PlatformLimits({(1, 1): k})))
    used, lrat = lrat_check.check(clauses, open(path + ".lrat").read())
    assert lrat[-1][1] == [] and used, lrat[-1]
    assert f" of {len(clauses)} clauses" in lines[-1] and len(used) <= int(lines[-1].split("core ")[1].split()[0]) <= len(clauses), lines[-1]


# ---- 7. state and ABI ---------------------------------------------------------------------------------------------------------------
def test_trim_state_and_abi():
    tc.run_state_and_abi(gpu_solver, SolverError, _lib.solver_lib())


def test_trim_takes_the_device_over_and_leaves_the_ipasir_state():
    tc.run_device_takeover(gpu_solver, SolverResult, ColdReason)
