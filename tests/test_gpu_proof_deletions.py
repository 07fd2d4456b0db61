"""mi355sat_proof_deletions on the MI355X: ms_rup_kernel<LV, TRACE, true> in both LV builds, plain and tracing, on the cases
of tests/test_emu_proof_deletions.py, and `tbs_cli --certify PATH --honour-deletions`.  Cases and judge:
tests/proof_deletion_cases.py - every expectation is the reference's, which restates the semantics over the oracle's
unit propagation."""
import os
import subprocess

import pytest

import lrat_check
import proof_check_cases as pc
import proof_deletion_cases as dc
import proof_trim_cases as tc
from fuzz_cases import GPU_CASES
from helpers import ROOT, make_grid, platform_defs
from test_gpu_proof_check import gpu_solver, own_proof
from timberborn_support_solver_amd import ColdReason, Encoding, PlatformLimits, SolverError, SolverResult

pytestmark = pytest.mark.gpu

LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


@LDS
@pytest.mark.parametrize("name", list(dc.INSPECTION))
def test_deletions_by_inspection(name, lds_val):
    dc.run_inspection(gpu_solver, name, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("k", range(4), ids=["w4-g1", "w16-g4", "whalf-g8", "wall-g1"])
@pytest.mark.parametrize("name", dc.WINDOW_CASES)
def test_sliding_windows(name, k, lds_val):
    dc.run_window(gpu_solver, GPU_CASES, name, k, lds_val)


@LDS
@pytest.mark.parametrize("name", dc.WINDOW_CASES)
def test_trim_of_the_valid_windows(name, lds_val):
    dc.run_window_trims(gpu_solver, GPU_CASES, name, lds_val)


@LDS
def test_churn(lds_val):
    dc.run_churn(gpu_solver, lds_val=lds_val)


def test_deletions_in_the_products_own_proof(tmp_path):
    cnf, proof, st = own_proof(tmp_path, "rect8x8", "1x1", 3, workers=3, slice_conflicts=16, reduce_first=25, reduce_inc=10,
                                deterministic=1)
    assert st["reduce_dbs"] > 0
    dc.run_own_proof(gpu_solver, cnf, cnf.n_vars, proof)


def test_switch_off_is_the_checker_as_it_was():
    dc.run_switch_off(gpu_solver, SolverError)


def test_argument_errors_with_the_switch_on():
    pc.run_argument_errors(dc.switched_on(gpu_solver), SolverError)


def test_switch_leaves_the_ipasir_state():
    tc.run_device_takeover(dc.switched_on(gpu_solver), SolverResult, ColdReason)


def test_cli_certify_honouring_deletions_writes_an_lrat_file_the_checker_accepts(tmp_path):
    """`tbs_cli --certify PATH --honour-deletions`: as the certify test without the flag, plus the line about the deletions."""
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    path = str(tmp_path / "bound.drup")
    out = subprocess.run([cli, "rect", "8", "8", "-l1:8", "--workers", "64", "--certify", path, "--honour-deletions"],
                         capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and "No solution found for the current constraints" in lines, (out.stdout, out.stderr)
    assert lines[-1].startswith("Certificate: " + path + ".lrat - core ") and lines[-2].startswith("Deletions: "), lines
    k = int([l for l in lines if l.startswith("Solution found")][-1].split("(")[1].split()[0]) - 1
    enc = Encoding.encode(platform_defs("default"), make_grid("rect8x8"))
    clauses = tc.clauses_of(enc.with_limits_into_cnf(PlatformLimits({(1, 1): k})))
    used, lrat = lrat_check.check(clauses, open(path + ".lrat").read())
    assert lrat[-1][1] == [] and used, lrat[-1]
