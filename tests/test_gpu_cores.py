"""Failed-assumption cores on the MI355X: ms_final_kernel after the real search kernel builds (one worker per SIMD,
two and four waves per SIMD; assignment in LDS or in the slab, which also switches the final walk's marks between
LDS and a scratch row; which build ran is asserted through mi355sat_debug_last_search_build), a 64-instance solve_batch, a DRUP proof under assumptions and the C replay of the Rust
shim's SolveIncremental calls.  Every core is checked by the oracle."""
import numpy as np
import pytest

from helpers import make_grid, platform_defs
from oracle import oracle as ora
from test_assumption_cores import (ERR_STATE, assert_core, build_abi_cores, padded, run_abi_cores, sweep_cnf, PKG)
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

pytestmark = pytest.mark.gpu

_cnfs = {}


def cached_sweep_cnf(terrain, pset, k_max):
    key = (terrain, pset, k_max)
    if key not in _cnfs:
        _cnfs[key] = sweep_cnf(terrain, pset, k_max)
    return _cnfs[key]


def assert_ran_the_build_asked_for(s, one_per_simd, lds_val):
    """The default fleets of these formulas stay at or below 1024 workers, so one_per_simd = 0 / 2 / 4 means the 1- / 2- /
    4-waves build in every launch; with lds_val = 0 the last launch's LDS choice is the selection rule's for its fleet."""
    b = s.debug_last_search_build()
    assert b["wps"] == max(1, one_per_simd) and {w for _, w in b["builds"]} == {b["wps"]} and b["active"] <= 1024, b
    rule = Mi355Sat.debug_search_build_rule(b["active"], b["lds_val_bytes"], lds_val=lds_val, one_per_simd=one_per_simd)
    assert (b["lds"], b["dyn_lds_bytes"]) == (rule["lds"], rule["dyn_lds_bytes"]), (b, rule)
    if lds_val == -1:
        assert b["lds"] == 0 and {l for l, _ in b["builds"]} == {0}


@pytest.mark.parametrize("lds_val", [0, -1])
@pytest.mark.parametrize("one_per_simd", [0, 2, 4])
def test_cores_on_every_search_build(one_per_simd, lds_val):
    for terrain, k, k_max in [("rect16x16", 2, 8), ("rect16x16", 3, 8), ("rect24x24", 8, 12)]:
        enc, cnf = cached_sweep_cnf(terrain, "default", k_max)
        a, nv = padded(cnf, k)
        s = Mi355Sat(one_per_simd=one_per_simd, lds_val=lds_val)
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(nv)
        assert s.solve(a) == SolverResult.Unsat, (terrain, k)
        assert_ran_the_build_asked_for(s, one_per_simd, lds_val)
        core = s.core()
        assert core == [-int(cnf.card_outputs[k])], (terrain, k, core)
        assert_core(core, a, cnf, nv)
        assert [l for l in a if s.failed(l)] == core
        assert s.solve() == SolverResult.Sat                 # the assumptions are gone
        with pytest.raises(SolverError) as e:
            s.core()
        assert e.value.code == ERR_STATE
        s.close()
    # forbidden anchors: no platform anywhere cannot support rect16x16; the core names the anchors that matter
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({}))
    a = [-enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    s = Mi355Sat(one_per_simd=one_per_simd, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve(a) == SolverResult.Unsat
    assert_ran_the_build_asked_for(s, one_per_simd, lds_val)
    core = s.core()
    assert_core(core, a, cnf, cnf.n_vars)
    assert 0 < len(core) < len(a)
    s.close()


def test_cores_with_cube_splitting_on_the_device():
    enc, cnf = cached_sweep_cnf("rect16x16", "default", 8)
    a, nv = padded(cnf, 3)
    s = Mi355Sat(cube_split=1, workers=512)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Unsat
    core = s.core()
    assert_core(core, a, cnf, nv)
    assert core == [-int(cnf.card_outputs[3])]
    s.close()


def test_batch_of_64_instances_mixing_sat_and_unsat():
    enc, cnf = cached_sweep_cnf("rect16x16", "default", 8)
    nv = cnf.n_vars
    ks = [2, 3, 4, 5, 6, 3, 2, 7] * 8
    sets = [[nv + 1 + i, -int(cnf.card_outputs[k]), -(nv + 100 + i)] for i, k in enumerate(ks)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + 200)
    res = s.solve_batch(sets)
    assert [r == SolverResult.Unsat for r in res] == [k <= 3 for k in ks]
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(nv + 200)
    for i, r in enumerate(res):
        if r == SolverResult.Unsat:
            core = s.core_of(i)
            assert core == [-int(cnf.card_outputs[ks[i]])], (i, core)
            assert o.solve(core) == 20
        else:
            with pytest.raises(SolverError):
                s.core_of(i)
    s.close()


def test_proof_under_assumptions_on_the_device(tmp_path):
    from timberborn_support_solver_amd.dimacs import read_drup
    enc, cnf = cached_sweep_cnf("rect8x8", "default", 4)
    a, nv = padded(cnf, 1)
    proof = str(tmp_path / "p.drup")
    s = Mi355Sat()
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(a) == SolverResult.Unsat
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


def test_abi_cores_call_sequence_on_the_device(tmp_path):
    exe = build_abi_cores(tmp_path, PKG, "mi355sat")
    enc, cnf = cached_sweep_cnf("rect16x16", "default", 8)
    a, nv = padded(cnf, 3)
    core, out = run_abi_cores(exe, tmp_path, cnf, 0, a, timeout=300)
    assert "result 20" in out and "again 10" in out
    assert core == [-int(cnf.card_outputs[3])]
    assert_core(core, a, cnf, nv)
