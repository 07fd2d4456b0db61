"""Warm incremental solve on the MI355X: ms_attach_kernel between the real search kernel builds (which build ran is
asserted through mi355sat_debug_last_search_build), solver_loop_incremental down to known optima, a warm refutation of a
hard rung, and the C replay of the Rust shim's calls.  Verdicts, models and cores are checked against the oracle on the
accumulated formula, as in tests/test_incremental.py."""
import threading

import pytest

from helpers import check_sat_answer, golden, make_grid, platform_defs
from test_gpu_cores import assert_ran_the_build_asked_for
from test_incremental import PKG, Checked, abi_steps_and_check, build_abi_incremental, golden_kstar, run_script, sweep_cnf
from test_zz_hard_rungs import LIMITS
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverResult, solver_loop_incremental

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lds_val", [0, -1])
@pytest.mark.parametrize("one_per_simd", [0, 2, 4])
def test_scripted_sequence_on_every_search_build(one_per_simd, lds_val):
    grid, enc, cnf = sweep_cnf("rect16x16", "default", 8)
    c = Checked(cnf, Mi355Sat(one_per_simd=one_per_simd, lds_val=lds_val))
    run_script(c, enc, cnf, grid, 3, 4)
    assert_ran_the_build_asked_for(c.s, one_per_simd, lds_val)
    i = c.info()
    assert i["cold_solves"] == 1 and i["warm_solves"] == len(c.log) - 1, i
    assert i["attached_units"] == 5 and i["attached_clauses"] == 5 and i["resident_learnts"] > 0, i
    c.s.close()


@pytest.mark.parametrize("one_per_simd,lds_val", [(0, 0), (4, -1)])
def test_scripted_sequence_on_rect24(one_per_simd, lds_val):
    grid, enc, cnf = sweep_cnf("rect24x24", "default", 12)
    c = Checked(cnf, Mi355Sat(one_per_simd=one_per_simd, lds_val=lds_val))
    run_script(c, enc, cnf, grid, 8, 9)
    assert_ran_the_build_asked_for(c.s, one_per_simd, lds_val)
    i = c.info()
    assert i["cold_solves"] == 1 and i["warm_solves"] == len(c.log) - 1, i
    c.s.close()


@pytest.mark.parametrize("terrain,pset,k0,kstar", [("rect24x24", "default", 30, 9), ("rect16x16", "1x1", 40, 15)])
def test_incremental_loop_reaches_the_known_optimum(terrain, pset, k0, kstar):
    """rect 24: k* = 9 (golden); rect 16 with 1x1 supports only: k* = 15 (test_gpu_parity's README-semantics case)."""
    if pset == "default":
        assert golden_kstar(terrain, pset) == kstar
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    lines = []
    hist = solver_loop_incremental(grid, enc, PlatformLimits({(1, 1): k0}), out=lines.append)
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == kstar - 1, [(h["k"], h["result"]) for h in hist]
    sat = [h for h in hist if h["result"] == SolverResult.Sat]
    assert sat[-1]["count"] == kstar and all(h["valid"] and h["count"] <= h["k"] for h in sat)
    for h in sat:
        assert h["layout"].validate(grid).is_valid() and h["layout"].platform_count() == h["count"]
    assert f"Solution found ({kstar} platforms total)" in lines and "Solution validation FAILED" not in lines
    i = hist[-1]["incremental"]
    assert i["cold_solves"] == 1 and i["warm_solves"] == len(hist) - 1, i
    print(terrain, pset, [(h["k"], h["result"].name, round(h["seconds"], 2)) for h in hist])


def test_warm_refutation_of_rect26_k10():
    """A hard rung of tests/golden/verdicts_hard.json, reached by warm steps from k = 12: SAT, SAT, then the refutation,
    within the limit tests/test_zz_hard_rungs.py states for that rung."""
    hard = {(v["terrain"], v["k"]): v["verdict"] for v in golden("verdicts_hard.json")["verdicts"]}
    grid = make_grid("rect26x26")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 12}), sweep=True)
    s = Mi355Sat()
    s.set_incremental(True)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    assert s.solve() == SolverResult.Sat
    check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, 12)
    s.add_clause([-int(cnf.card_outputs[11])])
    assert s.solve() == SolverResult.Sat and hard[("rect26x26", 11)] == "SAT"
    check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, 11)
    s.add_clause([-int(cnf.card_outputs[10])])
    tm = threading.Timer(LIMITS[("rect26x26", 10)], s.interrupter().interrupt)
    tm.start()
    try:
        r = s.solve()
    finally:
        tm.cancel()
    st, i = s.stats(), s.debug_incremental()
    print(f"rect26x26 k=10 warm: {r.name}, {st['solve_seconds']:.1f} s for the three solves, {st['conflicts']:.3e} conflicts, {i}")
    assert r.name.upper() == hard[("rect26x26", 10)] == "UNSAT"
    assert s.core() == []
    assert (i["cold_solves"], i["warm_solves"], i["attached_units"]) == (1, 2, 2) and i["resident_learnts"] > 0, i
    s.close()


def test_abi_incremental_call_sequence_on_the_device(tmp_path):
    exe = build_abi_incremental(tmp_path, PKG, "mi355sat")
    abi_steps_and_check(exe, tmp_path, "rect16x16", 0, timeout=300)


def test_cli_incremental_prints_the_reference_loop():
    """`tbs_cli --incremental` (the C++ solver_loop_incremental): the reference's messages down to the known optima."""
    import os
    import subprocess
    from helpers import ROOT
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    for args, kstar in ((["rect", "8", "8", "-l1:20", "--workers", "64"], 2), (["rect", "16", "16", "-l1:40", "--workers", "512"], 4),
                        (["rect", "8", "8", "-l1:1000", "--platforms", "1x1"], 4)):     # (a first bound that needs no totalizer)
        out = subprocess.run([cli] + args + ["--incremental"], capture_output=True, text=True, timeout=120)
        lines = out.stdout.strip().splitlines()
        assert out.returncode == 0 and lines[-1] == "No solution found for the current constraints", (args, out.stdout[-500:], out.stderr[-500:])
        assert lines[0].startswith("Solution found (") and "Solution validation OK" in lines and "Solution validation FAILED" not in lines
        assert [l for l in lines if l.startswith("Solution found")][-1] == f"Solution found ({kstar} platforms total)"
