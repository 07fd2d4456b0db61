"""DRUP proofs of solve_batch and the stepwise sweep, the gather kernel that drains the logs, and the check of several
targets in one pass, on the wavefront emulator (tests/emu).  Cases and judges: tests/sweep_proof_cases.py - every
expectation is the oracle's."""
import pytest

import proof_check_cases as pc
import sweep_cases as sc
import sweep_proof_cases as sp
from fuzz_cases import EMU_CASES
from helpers import emu_lib, make_grid, platform_defs
import lrat_check
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

UNSAT = pc.unsat_cases(EMU_CASES)
LDS = pytest.mark.parametrize("lds_val", [1, -1], ids=["lds", "slab"])


def emu_solver(**kw):
    kw.setdefault("simp", -1)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


# ---- 1. / 3. solve_batch with a proof path --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sp.BATCH_CASES)
def test_emulated_batch_logs_a_proof_that_certifies_every_unsat_instance(name, tmp_path):
    cores, _, log = sp.run_batch_and_check(emu_solver, name, tmp_path, deterministic=1)
    assert log["core_lines"] == sum(1 for c in cores.values() if c and not sp.is_tautology(c))
    if name == sc.FORMULA_UNSAT:           # (instance 0 has no assumptions: its verdict is the formula's)
        assert cores[0] == [] and sum(1 for line in open(tmp_path / "batch.drup") if line.strip() == "0") == 1


@pytest.mark.parametrize("name", sp.BATCH_CASES)
def test_emulated_batch_proof_is_reproducible(name, tmp_path):
    a, b = str(tmp_path / "a.drup"), str(tmp_path / "b.drup")
    sp.run_batch(emu_solver, name, a, deterministic=1)
    sp.run_batch(emu_solver, name, b, deterministic=1)
    assert open(a, "rb").read() == open(b, "rb").read()


# ---- 2. the stepwise sweep under seeded schedules --------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sp.SCHEDULE_SEEDS)
def test_emulated_scheduled_sweep_logs_a_proof(seed, tmp_path):
    path = str(tmp_path / "sweep.drup")
    cnf, _ = sc.formula(sp.SCHEDULE_CASE)
    cores, _ = sp.run_scheduled_sweep(emu_solver, sp.SCHEDULE_CASE, seed, path, deterministic=1)
    order = sorted(cores)
    info = sp.check_targets_on_fresh_handle(emu_solver, cnf, path, [sp.negated(cores[i]) for i in order])
    assert info["valid"] == 1 and info["target_valid"] == [1] * len(order), info


def test_emulated_sweep_without_a_proof_path_launches_what_it_did():
    _, a = sp.run_scheduled_sweep(emu_solver, sp.SCHEDULE_CASE, 1, None, deterministic=1)
    _, b = sp.run_scheduled_sweep(emu_solver, sp.SCHEDULE_CASE, 1, None, deterministic=1)
    assert a["kernel_launches"] == b["kernel_launches"] and a["conflicts"] == b["conflicts"]


# ---- 4. the gather kernel's edges ------------------------------------------------------------------------------------------
def own_proof(tmp_path, proof_cap=0, k=3, **opts):
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "own.drup")
    s = emu_solver(**dict(sp.GATHER_OPTS, **opts))
    if proof_cap:
        s.debug_set_capacities(proof_cap=proof_cap)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    return s, cnf, proof


def test_emulated_gather_of_lemmas_and_deletion_lines(tmp_path):
    s, cnf, proof = own_proof(tmp_path)
    assert s.solve() == SolverResult.Unsat
    st, log = s.stats(), s.debug_proof_log()
    s.close()
    assert st["reduce_dbs"] > 0 and any(line.startswith("d ") for line in open(proof))
    assert log["gathers"] > 0 and log["logs"] >= log["gathers"] and log["words"] > 0
    pc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof)


def test_emulated_gather_from_a_log_that_is_just_large_enough(tmp_path):
    s, cnf, proof = own_proof(tmp_path, proof_cap=sp.PROOF_CAP_TIGHT)
    assert s.solve() == SolverResult.Unsat
    assert s.debug_capacities()["proof_cap"] == sp.PROOF_CAP_TIGHT
    s.close()
    pc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof, half_is_no_proof=False)


def test_emulated_proof_buffer_overflow_and_the_solve_after(tmp_path):
    s, cnf, proof = own_proof(tmp_path, proof_cap=sp.PROOF_CAP_TOO_SMALL)
    with pytest.raises(SolverError) as e:
        s.solve()
    assert "proof buffer overflow" in str(e.value)
    s.debug_set_capacities()
    assert s.solve() == SolverResult.Unsat
    s.close()
    pc.run_own_proof(emu_solver, cnf, cnf.n_vars, proof, half_is_no_proof=False)


def test_emulated_gather_with_an_empty_log_between_two_others(tmp_path):
    """3sat-n50-s5 with one worker per instance and no rebalancing: instance 2 (a contradictory pair) is decided at its
    first slice without a conflict, so worker 2's log stays empty between those of workers 1 and 3."""
    name = "3sat-n50-s5"
    cnf, _ = sc.formula(name)
    path = str(tmp_path / "batch.drup")
    cores, st, log = sp.run_batch(emu_solver, name, path, deterministic=1, workers=sc.CASES[name][8], rebalance=-1)
    assert log["gathers"] > 0 and log["logs"] < log["gathers"] * st["workers"]
    info = sp.check_targets_on_fresh_handle(emu_solver, cnf, path, [sp.negated(cores[i]) for i in sorted(cores)])
    assert info["valid"] == 1, info


# ---- 5. / 6. several targets -----------------------------------------------------------------------------------------------
@LDS
def test_emulated_one_target_equals_check_proof(lds_val):
    sp.run_one_target_equals_check_proof(emu_solver, lds_val=lds_val)


@LDS
@pytest.mark.parametrize("name", list(sp.TARGET_CASES))
def test_emulated_targets_by_inspection(name, lds_val):
    sp.run_target_case(emu_solver, name, lds_val=lds_val)


@LDS
def test_emulated_deleted_lemma_that_only_a_target_needs(lds_val):
    sp.run_deleted_lemma_only_a_target_needs(emu_solver, lds_val=lds_val)


@pytest.mark.parametrize("name", list(UNSAT))
def test_emulated_targets_on_the_oracles_proofs(name):
    sp.run_fuzz_targets(emu_solver, UNSAT[name])


# ---- 7. trim ---------------------------------------------------------------------------------------------------------------
def test_emulated_trim_of_one_instance_of_a_batch(tmp_path):
    name = "3sat-n50-s5"
    cnf, _ = sc.formula(name)
    path = str(tmp_path / "batch.drup")
    cores, _, _ = sp.run_batch(emu_solver, name, path, deterministic=1)
    i = max(cores, key=lambda j: len(cores[j]))
    target = sp.negated(cores[i])
    assert target and not sp.is_tautology(target)
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    t = s.trim_proof_file(path, target=target, hints=True)
    assert t["check"]["valid"] == 1, t
    lrat = str(tmp_path / "one.lrat")
    s.trim_write_lrat(lrat)
    _, lines = lrat_check.check(cnf.clauses, open(lrat).read())          # (raises where it rejects)
    assert set(lines[-1][1]) == set(target)
    info = s.check_lrat_file(lrat, target=target)
    assert (info["valid"], info["accepted"], info["derives_target"]) == (1, 1, 1), info
    s.close()


# ---- 8. / 9. errors, ABI ---------------------------------------------------------------------------------------------------
def test_emulated_target_argument_and_state_errors():
    sp.run_target_errors(emu_solver, SolverError)


def test_emulated_share_import_takes_nothing_while_a_proof_is_logged(tmp_path):
    name = "3sat-n50-s5"
    cnf, _ = sc.formula(name)
    ls, _ = sc.lists(name)
    records = [2, 1, 2, 0]
    taken = {}
    for logged in (False, True):
        s = emu_solver(**sp.batch_options(name, deterministic=1))
        if logged:
            s.set_proof_path(str(tmp_path / "sweep.drup"))
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        s.sweep_begin(ls)
        s.sweep_step()
        taken[logged] = s.share_import(records)
        s.sweep_end()
        s.close()
    assert taken == {False: 1, True: 0}


def test_the_abi_sizes_are_unchanged():
    import ctypes
    L = emu_lib()
    L.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (L.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (128, 248)
