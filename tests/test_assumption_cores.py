"""Failed-assumption cores (IPASIR assume / failed, rustsat `SolveIncremental`) on the CPU, through the wavefront
emulator build of the solver (tests/emu): ms_final_kernel's walk over a refuted worker's trail, its launch from the
host's slice processing and the mapping back to the caller's assumption list.  Every core is checked by the oracle:
it is a subset of the assumptions, in their order, and formula AND core is UNSAT."""
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import ROOT, emu_lib, make_grid, platform_defs
from oracle import oracle as ora
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

ERR_STATE = -3
PAD = 50
# (terrain, platform set, highest UNSAT bound, lowest SAT bound) - tests/golden/verdicts.json
CASES = [("ex1", "1x1", 2, 3), ("ex3", "1x1", 3, 4), ("rect8x8", "1x1", 3, 4), ("rect8x8", "default", 1, 2)]


def emu_solver(**kw):
    kw.setdefault("simp", -1)      # (probing through the fiber emulator is slow; the simp variants are tested below)
    kw.setdefault("workers", 2)
    kw.setdefault("slice_conflicts", 200)
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def sweep_cnf(terrain, pset, k_max=8):
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    return enc, enc.with_limits_into_cnf(PlatformLimits({(1, 1): k_max}), sweep=True)


def padded(cnf, k):
    """NOT card_outputs[k] between 50 literals over fresh variables on either side (nothing constrains those)."""
    nv = cnf.n_vars
    before = [nv + 1 + i for i in range(PAD)]
    after = [-(nv + 1 + PAD + i) for i in range(PAD)]
    return before + [-int(cnf.card_outputs[k])] + after, nv + 2 * PAD


def oracle_solver(cnf, n_vars, extra=()):
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    for c in extra:
        lits = np.asarray(c, dtype=np.int32)
        o.add_cnf(lits, np.asarray([0, len(lits)], dtype=np.uint64))
    o.reserve(n_vars)
    return o


def assert_core(core, assumptions, cnf, n_vars, extra=()):
    """core is a subset of the assumptions, without repeats, in the caller's order, and formula AND core is UNSAT."""
    assert len(set(core)) == len(core) and set(core) <= set(assumptions), (core, assumptions)
    first = {}
    for i, l in enumerate(assumptions):
        first.setdefault(l, i)
    assert core == sorted(core, key=first.__getitem__)
    assert oracle_solver(cnf, n_vars, extra).solve(core) == 20, core


def solve_padded(s, cnf, k):
    a, nv = padded(cnf, k)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    return s.solve(a), a, nv


@pytest.mark.parametrize("terrain,pset,k_unsat,k_sat", CASES, ids=lambda x: str(x))
def test_padding_is_not_in_the_core(terrain, pset, k_unsat, k_sat):
    enc, cnf = sweep_cnf(terrain, pset)
    s = emu_solver()
    r, a, nv = solve_padded(s, cnf, k_unsat)
    assert r == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, nv)
    assert core == [-int(cnf.card_outputs[k_unsat])] and len(core) < len(a)
    # the same handle at a SAT bound: SAT, and no core
    a2, _ = padded(cnf, k_sat)
    assert s.solve(a2) == SolverResult.Sat
    with pytest.raises(SolverError) as e:
        s.core()
    assert e.value.code == ERR_STATE
    with pytest.raises(SolverError):
        s.failed(a2[0])
    s.close()


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("lds_val", [0, -1])
def test_forbidden_anchors_core_is_a_proper_subset(seed, lds_val):
    """No platform anywhere on rect8x8 cannot support the terrain; the core names the anchors that matter."""
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({}))
    a = [-enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    assert all(l < 0 for l in a)
    s = emu_solver(seed=seed, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, cnf.n_vars)
    assert 0 < len(core) < len(a)
    s.close()


def test_contradicting_assumptions_on_a_sat_formula():
    enc, cnf = sweep_cnf("ex1", "1x1")
    x = enc.platform_var(1, 1, (1, 1))
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Sat
    assert s.solve([x, -x]) == SolverResult.Unsat
    assert s.core() == [x, -x]
    assert s.failed(x) and s.failed(-x)
    s.close()


def test_assumption_false_at_level_zero():
    enc, cnf = sweep_cnf("ex1", "1x1")
    y = cnf.n_vars + 7
    a, nv = padded(cnf, 6)           # (a SAT bound: only y can fail)
    a = a[:20] + [y] + a[20:]
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.add_clause([-y])
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Unsat
    assert s.core() == [y]
    s.close()


def test_formula_unsat_by_itself_has_the_empty_core():
    grid = make_grid("ex1")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 1}))   # UNSAT without any assumption
    nv = cnf.n_vars
    a = [nv + 1 + i for i in range(PAD)]
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + PAD)
    assert s.solve(a) == SolverResult.Unsat
    assert s.core() == [] and not any(s.failed(l) for l in a)
    s.close()
    s = emu_solver()                 # refuted before any search (two contradicting units)
    s.add_clause([1])
    s.add_clause([-1])
    assert s.solve([2, 3]) == SolverResult.Unsat and s.core() == []
    s.close()


def test_three_times_n_vars_duplicated_assumptions():
    """Repeated assumptions each opened a decision level of their own: a list longer than n_vars must not overrun the
    worker's trail_lim.  The core names one occurrence (the first)."""
    enc, cnf = sweep_cnf("ex1", "1x1")
    nv = cnf.n_vars
    sat_set = [-int(cnf.card_outputs[5]), nv + 1, -(nv + 2)]
    unsat = -int(cnf.card_outputs[2])
    n = 3 * (nv + 2)
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + 2)
    a = [sat_set[i % 3] for i in range(n)]
    assert s.solve(a) == SolverResult.Sat
    a = [sat_set[i % 3] for i in range(n // 2)] + [unsat] * (n - n // 2)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, nv + 2)
    assert unsat in core and nv + 1 not in core and -(nv + 2) not in core
    s.close()


def test_ipasir_sequencing():
    enc, cnf = sweep_cnf("rect8x8", "1x1")
    s = emu_solver()
    r, a, nv = solve_padded(s, cnf, 3)
    assert r == SolverResult.Unsat
    core = s.core()
    assert [l for l in a if s.failed(l)] == core
    assert not s.failed(12345) and not s.failed(-a[0])
    # the assumptions were for that solve only
    assert s.solve() == SolverResult.Sat
    with pytest.raises(SolverError):
        s.core()
    # solve -> add a clause -> assume -> solve
    assert s.solve([-int(cnf.card_outputs[3])]) == SolverResult.Unsat
    s.add_clause([nv + 1, nv + 2])
    with pytest.raises(SolverError) as e:   # adding leaves the UNSAT state
        s.core()
    assert e.value.code == ERR_STATE
    s.assume(-(nv + 1))
    s.assume(-int(cnf.card_outputs[4]))
    s.assume(-(nv + 2))
    assert s.solve() == SolverResult.Unsat
    core = s.core()
    assert_core(core, [-(nv + 1), -int(cnf.card_outputs[4]), -(nv + 2)], cnf, nv, extra=[[nv + 1, nv + 2]])
    assert core == [-(nv + 1), -(nv + 2)]
    # assume() on a variable above every one seen reserves it
    s.assume(nv + 50)
    assert s.solve() == SolverResult.Sat and s.stats()["max_var"] == nv + 50
    s.close()


def test_interrupted_or_exhausted_solve_has_no_core():
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 16}), sweep=True)   # k = 14: hard UNSAT, never finishes here
    a, nv = padded(cnf, 14)
    s = emu_solver(workers=1, slice_conflicts=5, conflict_budget=10)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Interrupted
    with pytest.raises(SolverError) as e:
        s.core()
    assert e.value.code == ERR_STATE
    s.close()
    s = emu_solver(workers=1, slice_conflicts=5)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    threading.Timer(0.5, s.interrupter().interrupt).start()
    assert s.solve(a) == SolverResult.Interrupted
    with pytest.raises(SolverError):
        s.failed(a[PAD])
    s.close()


@pytest.mark.parametrize("kw", [dict(simp=0), dict(simp=2), dict(var_order=1), dict(workers=1), dict(workers=3),
                                dict(workers=3, cube_split=1), dict(workers=3, cube_split=1, lds_val=-1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_cores_across_configurations(kw):
    enc, cnf = sweep_cnf("rect8x8", "1x1")
    s = emu_solver(**kw)
    r, a, nv = solve_padded(s, cnf, 3)
    assert r == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, nv)
    assert core == [-int(cnf.card_outputs[3])]
    s.close()
    # a core of several assumptions through the same configuration
    grid = make_grid("rect8x8")
    cnf = enc.with_limits_into_cnf(PlatformLimits({}))
    a = [-enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    s = emu_solver(**kw)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, cnf.n_vars)
    assert 0 < len(core) < len(a)
    s.close()


def test_deterministic_runs_give_the_same_core():
    grid = make_grid("rect8x8")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({}))
    a = [-enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    cores = []
    for _ in range(2):
        s = emu_solver(workers=3, deterministic=1, slice_conflicts=20)
        s.add_cnf(cnf.lits, cnf.offsets)
        assert s.solve(a) == SolverResult.Unsat
        cores.append(s.core())
        s.close()
    assert cores[0] == cores[1]
    assert_core(cores[0], a, cnf, cnf.n_vars)


def test_batch_cores():
    enc, cnf = sweep_cnf("rect8x8", "1x1")
    nv = cnf.n_vars
    ks = [2, 4, 3, 6, 1]
    sets = [[nv + 1 + i, -int(cnf.card_outputs[k]), -(nv + 10 + i)] for i, k in enumerate(ks)]
    sets.append([nv + 1, -(nv + 1)])
    s = emu_solver(workers=6)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + 20)
    res = s.solve_batch(sets)
    assert [r.name for r in res] == ["Unsat", "Sat", "Unsat", "Sat", "Unsat", "Unsat"]
    for i, r in enumerate(res):
        if r == SolverResult.Unsat:
            core = s.core_of(i)
            assert_core(core, sets[i], cnf, nv + 20)
            assert core == ([nv + 1, -(nv + 1)] if i == 5 else [-int(cnf.card_outputs[ks[i]])])
        else:
            with pytest.raises(SolverError) as e:
                s.core_of(i)
            assert e.value.code == ERR_STATE
    with pytest.raises(SolverError):
        s.core()          # (no plain solve() on this handle)
    s.close()


def test_proof_under_assumptions_ends_with_the_negated_core(tmp_path):
    from timberborn_support_solver_amd.dimacs import read_drup
    enc, cnf = sweep_cnf("rect8x8", "1x1")
    proof = str(tmp_path / "p.drup")
    s = emu_solver(workers=3, slice_conflicts=16, simp=0)
    s.set_proof_path(proof)
    r, a, nv = solve_padded(s, cnf, 3)
    assert r == SolverResult.Unsat
    core = s.core()
    s.close()
    assert_core(core, a, cnf, nv)
    last = open(proof).read().splitlines()[-1].split()
    assert last[-1] == "0" and sorted(int(t) for t in last[:-1]) == sorted(-l for l in core)
    lits = np.concatenate([np.asarray(cnf.lits, dtype=np.int32), np.asarray(core, dtype=np.int32)])
    offs = np.concatenate([np.asarray(cnf.offsets, dtype=np.uint64),
                           np.uint64(cnf.offsets[-1]) + np.arange(1, len(core) + 1, dtype=np.uint64)])
    p = read_drup(proof)
    assert ora.check_rup(lits, offs, nv, np.concatenate([p, np.zeros(1, dtype=np.int32)])) == 1
    # without assumptions the proof still ends with the empty clause
    cnf3 = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 3}))
    s = emu_solver(workers=3, slice_conflicts=16, simp=0)
    s.set_proof_path(proof)
    s.add_cnf(cnf3.lits, cnf3.offsets)
    assert s.solve() == SolverResult.Unsat and s.core() == []
    s.close()
    assert open(proof).read().splitlines()[-1].strip() == "0"
    assert ora.check_rup(cnf3.lits, cnf3.offsets, cnf3.n_vars, read_drup(proof)) == 1


# ---- the C header: tests/abi_cores.c (what the Rust shim's SolveIncremental calls, replayed in C)
PKG = os.path.join(ROOT, "timberborn_support_solver_amd")


def build_abi_cores(tmp_path, libdir, libname):
    exe = str(tmp_path / ("abi_cores_" + libname))
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "abi_cores.c"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir])
    return exe


def write_cnf(path, cnf):
    with open(path, "wb") as f:
        np.array([cnf.n_vars, cnf.n_clauses], dtype=np.int64).tofile(f)
        np.asarray(cnf.offsets, dtype=np.uint64).tofile(f)
        np.asarray(cnf.lits, dtype=np.int32).tofile(f)


def run_abi_cores(exe, tmp_path, cnf, workers, assumptions, timeout=600):
    path = str(tmp_path / "cnf.bin")
    write_cnf(path, cnf)
    out = subprocess.run([exe, path, str(workers)] + [str(l) for l in assumptions], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.stdout, out.stderr)
    line = [l for l in out.stdout.splitlines() if l.startswith("core")][0].split()
    return [int(t) for t in line[2:]], out.stdout


def test_abi_cores_builds_against_the_header_and_library(tmp_path):
    exe = build_abi_cores(tmp_path, PKG, "mi355sat")
    assert subprocess.run([exe], capture_output=True).returncode == 2     # usage error: main() was reached


def test_abi_cores_call_sequence_on_the_emulator(tmp_path):
    emu_lib()    # (builds tests/emu/libmi355sat_emu.so)
    exe = build_abi_cores(tmp_path, os.path.join(ROOT, "tests", "emu"), "mi355sat_emu")
    enc, cnf = sweep_cnf("rect8x8", "1x1")
    a, nv = padded(cnf, 3)
    core, out = run_abi_cores(exe, tmp_path, cnf, 2, a)
    assert "result 20" in out and "again 10" in out
    assert core == [-int(cnf.card_outputs[3])]
    assert_core(core, a, cnf, nv)
