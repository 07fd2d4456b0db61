"""mi355sat_proof_deletions on the wavefront emulator (tests/emu): ms_rup_kernel<LV, TRACE, true> in both LV builds, plain
and tracing, the host's resolution of the deletion lines and the bindings.  Cases and judge: tests/proof_deletion_cases.py -
every expectation is the reference's, which restates the semantics over the oracle's unit propagation."""
import pytest

import proof_check_cases as pc
import proof_deletion_cases as dc
from fuzz_cases import EMU_CASES
from helpers import emu_lib
from test_emu_proof_check import emu_solver, own_proof
from timberborn_support_solver_amd import SolverError

LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def test_the_rows_that_differ_are_the_five_and_the_windows_split():
    assert set(dc.DIFFERING) == {"deleted-before-use", "target-needs-it", "both-copies", "other-order-repeated-literal", "control"}
    ws = dc.judged_windows(EMU_CASES)
    peaks = [v[4]["peak_live_lemmas"] for v in ws.values()]
    assert min(peaks) == 4 and all(v[3][2] == len(v[1]) for v in ws.values()), peaks      # refuted_at = n throughout


@LDS
@pytest.mark.parametrize("name", list(dc.INSPECTION))
def test_emulated_deletions_by_inspection(name, lds_val):
    dc.run_inspection(emu_solver, name, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("cut", pc.CUTS, ids=lambda c: f"segments-{c or 'all'}")
@pytest.mark.parametrize("k", range(4), ids=["w4-g1", "w16-g4", "whalf-g8", "wall-g1"])
@pytest.mark.parametrize("name", dc.WINDOW_CASES)
def test_emulated_sliding_windows(name, k, cut, lds_val):
    dc.run_window(emu_solver, EMU_CASES, name, k, lds_val, cuts=(cut,))


@LDS
@pytest.mark.parametrize("name", dc.WINDOW_CASES)
def test_emulated_trim_of_the_valid_windows(name, lds_val):
    dc.run_window_trims(emu_solver, EMU_CASES, name, lds_val)


@LDS
def test_emulated_churn(lds_val):
    dc.run_churn(emu_solver, lds_val=lds_val)


def test_emulated_deletions_in_the_products_own_proof(tmp_path):
    cnf, proof, st = own_proof(tmp_path, "1x1", 3, workers=3, slice_conflicts=16, reduce_first=25, reduce_inc=10, deterministic=1)
    assert st["reduce_dbs"] > 0
    dc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof)


def test_emulated_switch_off_is_the_checker_as_it_was():
    dc.run_switch_off(emu_solver, SolverError)


def test_emulated_argument_errors_with_the_switch_on():
    pc.run_argument_errors(dc.switched_on(emu_solver), SolverError)


def test_emulated_switch_leaves_the_ipasir_state():
    from proof_trim_cases import run_device_takeover
    from timberborn_support_solver_amd import ColdReason, SolverResult
    run_device_takeover(dc.switched_on(emu_solver), SolverResult, ColdReason)


def test_the_abi_sizes_are_unchanged():
    import ctypes
    lib = emu_lib()
    lib.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (lib.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (128, 248)
