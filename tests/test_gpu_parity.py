"""GPU parity tests (run on a real MI355X with -m gpu).  Everything goes through the C ABI of
libmi355sat.so; the oracle (CPU) is the checker.  Bars: verdicts equal the golden / oracle verdicts;
every SAT model satisfies every clause, yields a layout that validates and has <= k platforms; BCP
fixpoints are bit-exact."""
import threading
import time

import numpy as np
import pytest

from helpers import VERDICTS, check_sat_answer, long_list_formula, make_grid, platform_defs, scripted_decisions
from oracle import oracle as ora
from timberborn_support_solver_amd import (Encoding, Mi355Sat, PlatformLayout, PlatformLimits, SolverResult,
                                           algorithmic_bytes, solver_loop)

pytestmark = pytest.mark.gpu

LADDER = VERDICTS["verdicts"]   # all of them, the hard rungs (ex2 1x1 k=13/14, rect24 k=8..12) included
HARD_RUNG_LIMIT_S = 120          # stated time limit of one rung; running into it fails the test


def solve_within(s, seconds):
    """solve() with a wall-clock limit: the interrupt turns a hang into a failed assertion."""
    tm = threading.Timer(seconds, s.interrupter().interrupt)
    tm.start()
    try:
        return s.solve()
    finally:
        tm.cancel()


@pytest.mark.parametrize("v", LADDER, ids=lambda v: f"{v['terrain']}-{v['platforms']}-k{v['k']}")
def test_golden_verdicts(v):
    grid = make_grid(v["terrain"])
    enc = Encoding.encode(platform_defs(v["platforms"]), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): v["k"]}))
    s = Mi355Sat(workers=64) if v["picosat_seconds"] < 1.0 else Mi355Sat()   # hard rungs: the default fleet
    s.add_cnf(cnf.lits, cnf.offsets)
    r = solve_within(s, HARD_RUNG_LIMIT_S)
    assert r.name.upper() == v["verdict"]
    if r == SolverResult.Sat:
        check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, v["k"])
    st = s.stats()
    assert st["propagations"] == st["n_deq"] and st["n_clauses"] == cnf.n_clauses and st["max_var"] == cnf.n_vars
    s.close()


@pytest.mark.parametrize("terrain,pset,k,n_dec", [("rect16x16", "default", 40, 12), ("ex3", "default", 20, 8),
                                                  ("rect16x16", "1x1", 40, 30), ("rect32x32", "default", 120, 16)])
def test_bcp_fixpoints_bit_exact(terrain, pset, k, n_dec):
    """BASELINE.json configs[1]: single-instance BCP from the formula's unit clauses and from scripted
    decision sequences (splitmix64 seeds 1..16), compared literal-for-literal with the oracle."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    scripts = [[]] + [scripted_decisions(enc, grid, seed, n_dec, p_positive=0.15) for seed in range(1, 17)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    confl, vals, tl = s.propagate_batch(scripts, n_vars=cnf.n_vars)
    n_fix = 0
    for i, dec in enumerate(scripts):
        c, v, n, _ = ora.bcp(cnf.lits, cnf.offsets, cnf.n_vars, dec)
        assert c == confl[i], (i, dec)
        if not c:
            n_fix += 1
            assert n == tl[i] and np.array_equal(v, vals[i]), i
    assert n_fix >= 4
    # idempotence: propagating a fixpoint's own literals changes nothing
    i = int(np.argmin(confl))
    fix = [int(v + 1) * int(vals[i][v]) for v in range(cnf.n_vars) if vals[i][v] != 0][:200]
    c2, v2, t2 = s.propagate_batch([scripts[i] + fix], n_vars=cnf.n_vars)
    assert c2[0] == 0 and np.array_equal(v2[0], vals[i])
    s.close()


def test_sweep_shares_one_clause_database():
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 12}), sweep=True)
    ks = [12, 8, 5, 4, 3, 2]
    s = Mi355Sat(workers=96)
    s.add_cnf(cnf.lits, cnf.offsets)
    res = s.solve_batch([[-int(cnf.card_outputs[k])] if k < 12 else [] for k in ks])
    assert [r.name for r in res] == ["Sat", "Sat", "Sat", "Sat", "Unsat", "Unsat"]      # k* = 4 (golden)
    for i, k in enumerate(ks):
        if res[i] == SolverResult.Sat:
            check_sat_answer(cnf, s.solution_of(i, cnf.n_vars), enc, grid, k)
    s.close()


@pytest.mark.parametrize("terrain,pset,k0,kstar", [("rect8x8", "default", 20, 2), ("ex3", "default", 20, 1),
                                                   ("ex3", "1x1", 20, 4), ("ex1", "default", 20, 1),
                                                   ("rect16x16", "default", 40, 4)])
def test_solver_loop_reaches_the_known_optimum(terrain, pset, k0, kstar):
    """configs[0] (through the GPU instead of the CPU reference) and configs[3]: the decreasing-k loop."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    lines = []
    hist = solver_loop(grid, enc, PlatformLimits({(1, 1): k0}), make_solver=lambda: Mi355Sat(workers=64), out=lines.append)
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == kstar - 1
    assert all(h["result"] == SolverResult.Sat and h["valid"] and h["count"] <= h["k"] for h in hist[:-1])
    assert hist[-2]["count"] == kstar
    assert lines[-1] == "No solution found for the current constraints"


def test_rect32_full_cdcl_harder_rungs():
    """configs[2] rungs that finish within seconds: rect 32x32 default at k = 120, 24 and 17 (SAT), and the
    refutations of k = 10 and k = 12 (optimum is 15 per SURVEY §6; PicoSAT needed 24.6 s for k = 12), cross-checked
    with the oracle.  The optimum rungs k = 14 (UNSAT) and k = 15 (SAT) are in tests/test_zz_hard_rungs.py."""
    grid = make_grid("rect32x32")
    enc = Encoding.encode(platform_defs("default"), grid)
    for k, want in [(120, SolverResult.Sat), (24, SolverResult.Sat), (17, SolverResult.Sat), (10, SolverResult.Unsat), (12, SolverResult.Unsat)]:
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        s = Mi355Sat(workers=256) if k not in (12, 17) else Mi355Sat()
        s.add_cnf(cnf.lits, cnf.offsets)
        r = solve_within(s, HARD_RUNG_LIMIT_S)
        assert r == want, k
        if r == SolverResult.Sat:
            check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
        else:
            o = ora.OracleSolver()
            o.add_cnf(cnf.lits, cnf.offsets)
            assert o.solve() == 20
        s.close()


def test_full_size_64x64_properties():
    """At BASELINE's full size the oracle is too slow to re-solve, so check size-independent
    properties: SAT models self-certify; BCP fixpoints equal the oracle's (BCP is cheap); counters add up."""
    grid = make_grid("rect64x64")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 200}))
    s = Mi355Sat(workers=256)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Sat                       # loose bound: "trivial to find" (README.md:23)
    lay = check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, 200)
    assert lay.platform_count() >= 43                          # area bound ceil(4096/97)
    st = s.stats()
    assert algorithmic_bytes(st) > 0 and st["kernel_seconds"] > 0
    s.close()
    scripts = [[]] + [scripted_decisions(enc, grid, seed, 24, p_positive=0.1) for seed in range(1, 8)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    confl, vals, tl = s.propagate_batch(scripts, n_vars=cnf.n_vars)
    for i, dec in enumerate(scripts):
        c, v, n, _ = ora.bcp(cnf.lits, cnf.offsets, cnf.n_vars, dec)
        assert c == confl[i]
        if not c:
            assert n == tl[i] and np.array_equal(v, vals[i])
    s.close()


def test_cube_splitting_mode_gives_the_same_verdicts():
    """Opt-in work stealing: the cubes partition the search space, so verdicts must not change."""
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    for k, want in [(3, SolverResult.Unsat), (4, SolverResult.Sat)]:
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        s = Mi355Sat(workers=256, cube_split=1, slice_ms=2)
        s.add_cnf(cnf.lits, cnf.offsets)
        assert s.solve() == want
        if want == SolverResult.Sat:
            check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
        s.close()


@pytest.mark.parametrize("terrain,pset,k", [("ex3", "1x1", 3), ("rect8x8", "default", 1), ("rect16x16", "default", 3),
                                             ("rect16x16", "1x1", 10)])
def test_unsat_verdicts_carry_a_checked_drup_proof(tmp_path, terrain, pset, k):
    """UNSAT parity beyond agreement of solvers: the GPU's own derivation (DRUP log of the clauses ALL its workers
    learnt, in the default configuration: simplification, the default fleet, clause exchange on) is verified by the
    oracle's forward RUP checker against the caller's formula."""
    from timberborn_support_solver_amd.dimacs import read_drup
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "p.drup")
    # the long refutation with 16 workers: the proof holds every worker's clauses and the oracle's checker is a
    # plain occurrence-list propagator (the default fleet's log of this one takes it many minutes)
    long_one = (terrain, pset, k) == ("rect16x16", "1x1", 10)
    # ... with vivification on, so that its lemmas (learnt clauses re-derived shorter under unit propagation) are in the
    # checked proof too
    s = Mi355Sat(workers=16, slice_ms=5, vivify=16) if long_one else Mi355Sat()
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Unsat
    st = s.stats()
    s.close()
    assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, read_drup(proof)) == 1
    if long_one:       # long enough for the exchange to matter: the checked derivation used other workers' clauses
        assert st["shared_imported"] + st["shared_imported_units"] > 0


def test_cpp_solver_loop_cli_prints_the_reference_messages(tmp_path):
    """The compiled host side (csrc/host/solver_loop.cpp + cli.cpp) over the C ABI: `rect 8 8 -l1:20`
    is BASELINE.json configs[0] run on the GPU; ex3 from a project file is configs[3]."""
    import os
    import subprocess
    from helpers import ROOT, terrain_rows
    cli = os.path.join(ROOT, "timberborn_support_solver_amd", "tbs_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "timberborn_support_solver_amd", "csrc"), "../tbs_cli"])
    out = subprocess.run([cli, "rect", "8", "8", "-l1:20", "--workers", "64"], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "No solution found for the current constraints"
    assert lines[0].startswith("Solution found (") and "Solution validation OK" in lines
    assert "Solution validation FAILED" not in lines
    assert [l for l in lines if l.startswith("Solution found")][-1] == "Solution found (2 platforms total)"   # k* = 2
    toml = str(tmp_path / "ex3_test.toml")
    with open(toml, "w") as f:
        f.write("[world]\ngrid = [\n" + "".join(f'    "{r}",\n' for r in terrain_rows("ex3")) + "]\n")
    out = subprocess.run([cli, "file", toml, "-l1:20", "--platforms", "1x1", "--workers", "64"], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "No solution found for the current constraints"
    assert [l for l in lines if l.startswith("Solution found")][-1] == "Solution found (4 platforms total)"   # k* = 4 with 1x1 only
    # the same refinement as one batch on the device (solver_loop_sweep)
    out = subprocess.run([cli, "rect", "16", "16", "-l1:40", "--workers", "512", "--sweep"], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "No solution found for the current constraints"
    assert [l for l in lines if l.startswith("Solution found")][-1] == "Solution found (4 platforms total)"   # k* = 4
    assert "Solution validation FAILED" not in lines


def test_rect16_with_1x1_supports_only_k15_sat_k14_unsat():
    """README semantics (1x1 supports only, README.md:5,29) on BASELINE configs[1]'s terrain: k* = 15
    (the refutation of k = 14 took PicoSAT 67.5 s, the CPU restatement 7.6 s / 1.8e5 conflicts).
    Stated limit per rung: HARD_RUNG_LIMIT_S."""
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    for k, want in [(15, SolverResult.Sat), (14, SolverResult.Unsat)]:
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        s = Mi355Sat()
        s.add_cnf(cnf.lits, cnf.offsets)
        assert solve_within(s, HARD_RUNG_LIMIT_S) == want, k
        if want == SolverResult.Sat:
            check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
        s.close()


def test_interrupt_and_budget():
    """rect 32x32 at k = 14 is a refutation no solver here finishes in minutes (PicoSAT 515 s):
    an interrupt after 1 s must come back as Interrupted within a few slices (20 ms each), from the
    default fleet; the handle then runs again (the interrupt is consumed by the solve it stops)."""
    grid = make_grid("rect32x32")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 14}))
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    intr = s.interrupter()
    fired = []
    tm = threading.Timer(1.0, lambda: (fired.append(time.time()), intr.interrupt()))
    tm.start()
    r = s.solve()
    t_back = time.time()
    tm.cancel()
    assert r == SolverResult.Interrupted and fired
    assert t_back - fired[0] < 2.0, f"solve() returned {t_back - fired[0]:.2f} s after the interrupt"
    assert s.stats()["n_terminated"] == 1
    # an interrupt that arrives while nothing runs stops the next solve at once, and only that one
    intr.interrupt()
    t0 = time.time()
    assert s.solve() == SolverResult.Interrupted and time.time() - t0 < 5
    s.close()
    s = Mi355Sat(workers=64, slice_conflicts=100, conflict_budget=3000)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve() == SolverResult.Interrupted
    s.close()


def test_exchange_ring_holds_only_consequences_of_the_formula():
    """The default configuration (many workers, exchange on, workers migrating between instances with
    different assumptions) relies on every record of the exchange ring being a consequence of the formula
    alone.  After a rect 16x16 sweep over all bounds the ring is read back and the oracle refutes
    formula AND NOT(record) for every record."""
    from helpers import assert_ring_records_are_implied
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    k0 = 10
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    ks = list(range(k0, -1, -1))
    s = Mi355Sat(workers=44 * len(ks), slice_ms=2, share_lbd=6)
    s.add_cnf(cnf.lits, cnf.offsets)
    res = s.solve_batch([([-int(cnf.card_outputs[k])] if k < k0 else []) for k in ks])
    assert [r.name for r in res] == ["Sat"] * 7 + ["Unsat"] * 4            # k* = 4
    st = s.stats()
    assert st["shared_exported"] > 0 and st["shared_imported"] + st["shared_imported_units"] > 0
    assert assert_ring_records_are_implied(s, cnf, max_records=3000) > 0
    s.close()


def test_degenerate_inputs_on_device():
    s = Mi355Sat()
    assert s.solve() == SolverResult.Sat
    s.close()
    s = Mi355Sat()
    s.add_clause([1, 2]); s.add_clause([-1, 2]); s.add_clause([1, -2]); s.add_clause([-1, -2])
    assert s.solve() == SolverResult.Unsat                     # needs one device conflict at level 0
    s.close()
    s = Mi355Sat()
    s.add_clause([1, 2, 3]); s.add_clause([-1, -2]); s.add_clause([-3]); s.reserve(7)
    assert s.solve() == SolverResult.Sat
    m = s.full_solution(7)
    assert m[2] == -1 and (m[0] == 1) != (m[1] == 1) or (m[0] == 1 and m[1] == -1) or (m[0] == -1 and m[1] == 1)
    s.close()


@pytest.mark.parametrize("kw", [dict(share=-1), dict(share=0, share_lbd=4), dict(var_order=1), dict(rebalance=-1),
                                dict(workers=2048), dict(workers=2048, ramp=-1)],
                         ids=["no-exchange", "exchange-lbd4", "locality-order", "no-rebalance", "ramp-2048", "no-ramp-2048"])
def test_exchange_order_and_rebalancing_never_change_an_answer(kw):
    """The learnt-clause exchange, the device's own variable numbering and the migration of workers
    are search strategy: verdicts equal the golden ones, models check against the caller's CNF."""
    for terrain, pset, k, want in [("rect16x16", "default", 3, "UNSAT"), ("rect16x16", "default", 4, "SAT"),
                                   ("ex2", "default", 3, "UNSAT"), ("rect8x8", "1x1", 3, "UNSAT")]:
        grid = make_grid(terrain)
        enc = Encoding.encode(platform_defs(pset), grid)
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        s = Mi355Sat(**{"workers": 256, "slice_ms": 2, **kw})
        s.add_cnf(cnf.lits, cnf.offsets)
        r = s.solve()
        assert r.name.upper() == want, (terrain, pset, k)
        if r == SolverResult.Sat:
            check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
        st = s.stats()
        if kw.get("share") == -1:
            assert st["shared_exported"] == 0 and st["shared_imported"] == 0
        s.close()


def test_locality_order_keeps_bcp_fixpoints_bit_exact():
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 40}))
    scripts = [[]] + [scripted_decisions(enc, grid, seed, 12, p_positive=0.15) for seed in range(1, 9)]
    s = Mi355Sat(var_order=1)
    s.add_cnf(cnf.lits, cnf.offsets)
    confl, vals, tl = s.propagate_batch(scripts, n_vars=cnf.n_vars)
    for i, dec in enumerate(scripts):
        c, v, n, _ = ora.bcp(cnf.lits, cnf.offsets, cnf.n_vars, dec)
        assert c == confl[i]
        if not c:
            assert n == tl[i] and np.array_equal(v, vals[i])
    s.close()


def test_sweep_with_exchange_migration_and_withdrawn_instances_finds_the_cut():
    """The whole ladder as one batch (rect 16x16, k* = 4): workers of decided instances move to the open
    ones, implied instances are withdrawn, exchanged clauses cross instance boundaries (they never
    depend on assumptions).  The cut and its model must be the golden ones."""
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    k0 = 10
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    ks = list(range(k0, -1, -1))
    sets = [([-int(cnf.card_outputs[k])] if k < k0 else []) for k in ks]
    s = Mi355Sat(workers=44 * len(ks), slice_ms=2)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.sweep_begin(sets)
    t0 = time.time()
    while time.time() - t0 < 60:
        res, _ = s.sweep_step()
        sat_k = min([k for k, r in zip(ks, res) if r == SolverResult.Sat], default=None)
        unsat_k = max([k for k, r in zip(ks, res) if r == SolverResult.Unsat], default=None)
        if sat_k is not None and unsat_k is not None and unsat_k + 1 >= sat_k:
            break
        s.sweep_drop([i for i, k in enumerate(ks) if res[i] == SolverResult.Interrupted and
                      ((sat_k is not None and k > sat_k) or (unsat_k is not None and k < unsat_k))])
    s.sweep_end()
    assert (sat_k, unsat_k) == (4, 3)
    check_sat_answer(cnf, s.solution_of(ks.index(4), cnf.n_vars), enc, grid, 4)
    for k, r in zip(ks, res):
        assert r in (SolverResult.Interrupted, SolverResult.Sat if k >= 4 else SolverResult.Unsat)
    assert s.stats()["shared_exported"] > 0
    s.close()


@pytest.mark.parametrize("terrain,pset,k0,kstar,kw", [("rect16x16", "default", 40, 4, dict(workers=1024, slice_ms=2)),
                                                      ("ex3", "default", 20, 1, dict(workers=1024, slice_ms=2)),
                                                      ("ex2", "default", 12, 4, dict(workers=1024, slice_ms=2)),
                                                      ("ex2", "default", 12, 4, dict(simp=2)),      # (variable elimination: the bounds' outputs are kept)
                                                      ("rect24x24", "default", 24, 9, dict())])
def test_solver_loop_sweep_reaches_the_same_optimum_as_the_sequential_loop(terrain, pset, k0, kstar, kw):
    """The last case runs with the default options long enough to leave the ramp-up: the fleet grows from one
    worker per CU to the default 1024 in flight (grow_workers: slabs allocated on demand, running workers moved)."""
    from timberborn_support_solver_amd import solver_loop_sweep
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    lines = []
    hist = solver_loop_sweep(grid, enc, PlatformLimits({(1, 1): k0}), out=lines.append, time_limit=120,
                             make_solver=lambda: Mi355Sat(**kw))
    sat = [h for h in hist if h["result"] == SolverResult.Sat]
    assert hist[-1]["result"] == SolverResult.Unsat and hist[-1]["k"] == kstar - 1 and len(sat) >= 1
    assert sat[-1]["count"] == kstar and all(h["valid"] for h in sat)
    assert f"Solution found ({kstar} platforms total)" in lines
    assert lines[-1] == "No solution found for the current constraints"


def test_weight_loop_on_the_gpu_reaches_the_oracle_optimum():
    """the GUI's weight-minimising loop (crates/gui/src/app.rs:235-245) over the PB weight bound
    (src/encoder.rs:654-663 -> generalized totalizer) on rect 8x8 with the default platform set and weights =
    tile area.  Every SAT step validated; the final bound refuted on the GPU and by the oracle on the oracle's
    own GTE CNF (encoder_oracle.with_weights / into_cnf)."""
    from oracle import encoder_oracle as eo
    from timberborn_support_solver_amd import PLATFORMS_DEFAULT, weight_loop
    grid = make_grid("rect8x8")
    enc = Encoding.encode(PLATFORMS_DEFAULT, grid)
    # nested types add up (platform_layout.rs:174-183): a larger platform also sets the smaller ones' variables
    weights = {d: 1 for d in PLATFORMS_DEFAULT}
    hist = weight_loop(grid, enc, PlatformLimits({}, weights, None), make_solver=lambda: Mi355Sat(workers=64), out=lambda s: None)
    assert hist[-1]["result"] == SolverResult.Unsat
    ws = [h["weight"] for h in hist[:-1]]
    assert ws and all(h["valid"] for h in hist[:-1]) and ws == sorted(ws, reverse=True) and len(set(ws)) == len(ws)
    assert hist[-1]["weight_limit"] == ws[-1] - 1
    o = eo.Encoding(list(PLATFORMS_DEFAULT), eo.grid_from_rows(grid.rows()))
    for wl, want in [(ws[-1] - 1, 20), (ws[-1], 10)]:
        cl, nv, cards, terms = eo.with_weights(o, {}, weights, wl)
        ocnf, onv, _ = eo.into_cnf(cl, nv, cards, pbs=[(terms, wl)])
        lits, offs = ora.to_csr(ocnf)
        so = ora.OracleSolver()
        so.add_cnf(lits, offs)
        so.reserve(onv)
        assert so.solve() == want, wl


def test_rectangular_type_limit_on_the_gpu():
    """`-l2x1:K` style limits on a non-square type go through fresh per-tile "either orientation" variables
    (src/encoder.rs:629-641).  rect 16x16, default platforms (k* = 4, needing four 5x5): at most k platforms in
    total (1x1 limit) AND at most r of size >= 5x5 / >= 1x6 in either orientation.  Verdicts against the oracle on the oracle's CNF; SAT models
    clause-checked, validated, and the limited type counted in the layout."""
    from oracle import encoder_oracle as eo
    from timberborn_support_solver_amd import PLATFORMS_DEFAULT
    grid = make_grid("rect16x16")
    enc = Encoding.encode(PLATFORMS_DEFAULT, grid)
    o = eo.Encoding(list(PLATFORMS_DEFAULT), eo.grid_from_rows(grid.rows()))
    seen = set()
    for lim in ({(1, 1): 4, (5, 5): 3}, {(1, 1): 5, (5, 5): 3, (1, 6): 4}, {(1, 1): 5, (5, 5): 2, (1, 6): 3}, {(1, 1): 5, (1, 6): 0},
                {(1, 1): 4, (5, 5): 0}):
        cnf = enc.with_limits_into_cnf(PlatformLimits(lim))
        cl, nv, cards = o.with_limits(lim)
        ocnf, onv, _ = eo.into_cnf(cl, nv, cards)
        lits, offs = ora.to_csr(ocnf)
        so = ora.OracleSolver()
        so.add_cnf(lits, offs)
        so.reserve(onv)
        want = so.solve()
        s = Mi355Sat(workers=64)
        s.add_cnf(cnf.lits, cnf.offsets)
        r = solve_within(s, HARD_RUNG_LIMIT_S)
        assert r.value == want, lim
        seen.add(want)
        if r == SolverResult.Sat:
            lay = check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, lim[(1, 1)])
            stats = lay.platform_stats()
            for d, n in lim.items():
                if d != (1, 1):   # "at most n platforms of size >= d" (REPL help, main.rs:59-67)
                    assert sum(c for (w, h), c in stats.items() if w >= d[0] and h >= d[1]) <= n, (lim, stats)
        s.close()
    assert seen == {10, 20}


@pytest.mark.parametrize("terrain,pset,k,want", [("rect16x16", "default", 3, "Unsat"), ("rect16x16", "default", 4, "Sat"),
                                                  ("ex2", "1x1", 14, "Sat"), ("ex3", "default", 1, "Sat"),
                                                  ("rect24x24", "default", 8, "Unsat"), ("rect24x24", "default", 9, "Sat")])
def test_simplification_before_search_keeps_verdicts_and_models(terrain, pset, k, want):
    """SURVEY 8 f3 (`simp::Glucose`, crates/repl/src/main.rs:17): with the device-side simplification on (the
    default: equivalent literals, failed-literal probing, subsumption), with bounded variable elimination on top
    (simp = 2: `SimpSolver::eliminate`) and off, the verdict is the golden one; models are in the caller's variables
    and satisfy the ORIGINAL clauses - eliminated variables included; the counters show what ran."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    for simp in (0, 2, -1):
        s = Mi355Sat(simp=simp)
        s.add_cnf(cnf.lits, cnf.offsets)
        r = solve_within(s, HARD_RUNG_LIMIT_S)
        assert r.name == want, (terrain, pset, k, simp)
        st = s.stats()
        assert (st["simp_units"] + st["simp_equivalences"] + st["simp_clauses_removed"] > 0) == (simp >= 0)
        assert (st["simp_eliminated"] > 0) == (simp == 2)
        if r == SolverResult.Sat:
            check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
        s.close()


@pytest.mark.parametrize("terrain,k", [("rect32x32", 120), ("rect64x64", 450)])
def test_large_terrains_with_1x1_supports_only(terrain, k):
    """README semantics (1x1 supports only, README.md:5,29) at BASELINE's larger sizes: configs[2]'s START_COUNT = 120
    on rect 32x32 and a loose bound on rect 64x64 are satisfiable; models self-certify (every clause, layout valid by
    product and oracle validators, count <= k), and the 1x1-only BCP fixpoints equal the oracle's."""
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    assert solve_within(s, HARD_RUNG_LIMIT_S) == SolverResult.Sat
    lay = check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, k)
    assert all((w, h) == (1, 1) for _, _, w, h, _ in lay.platforms())
    s.close()
    scripts = [[]] + [scripted_decisions(enc, grid, seed, 40, p_positive=0.3) for seed in range(1, 6)]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    confl, vals, tl = s.propagate_batch(scripts, n_vars=cnf.n_vars)
    for i, dec in enumerate(scripts):
        c, v, n, _ = ora.bcp(cnf.lits, cnf.offsets, cnf.n_vars, dec)
        assert c == confl[i]
        if not c:
            assert n == tl[i] and np.array_equal(v, vals[i])
    s.close()


def test_deterministic_mode_repeats_itself_on_the_gpu():
    """opts.deterministic = 1 (include/mi355sat.h): conflict-bounded slices, ordered clause collection, the whole fleet from
    the first slice, no early exits - two runs of the rect 24x24 k = 8 refutation (golden: UNSAT) with the default fleet
    and the exchange on report identical counters.  The default mode does not (slices are time-bounded)."""
    grid = make_grid("rect24x24")
    enc = Encoding.encode(platform_defs("default"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 8}))
    runs = []
    for _ in range(2):
        s = Mi355Sat(deterministic=1, seed=11)
        s.add_cnf(cnf.lits, cnf.offsets)
        assert solve_within(s, HARD_RUNG_LIMIT_S) == SolverResult.Unsat
        st = s.stats()
        runs.append((st["conflicts"], st["propagations"], st["decisions"], st["restarts"], st["shared_exported"], st["shared_imported"]))
        s.close()
    assert runs[0] == runs[1], runs
    assert runs[0][0] > 0 and runs[0][4] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("lds_val", [0, -1], ids=["assignment-in-lds", "assignment-in-slab"])
def test_bcp_fixpoints_long_clauses_and_long_watch_lists(lds_val):
    """propagate() on the MI355X against the oracle's occurrence-list BCP on formulas cut for the step's side paths
    (tests/helpers.py::long_list_formula: several clause tails per step, watch lists of 44 long clauses spread flat over the
    wave, moved watches, two groups meeting in one clause) - the emulator runs the same in tests/test_emu_kernels.py."""
    n_fix = n_conf = 0
    for seed in (11, 12, 13, 14):
        lits, offsets, n_vars, n_hubs, rng = long_list_formula(seed)
        scripts = []
        for _ in range(24):
            dec = [int(h + 1) for h in rng.permutation(n_hubs)[: int(rng.integers(1, n_hubs + 1))]]
            dec += [int(v + 1) * (1 if rng.random() < 0.5 else -1) for v in rng.choice(np.arange(n_hubs, n_vars), size=int(rng.integers(4, 110)), replace=False)]
            scripts.append([int(x) for x in rng.permutation(dec)])
        s = Mi355Sat(lds_val=lds_val, simp=-1)
        s.add_cnf(lits, offsets)
        confl, vals, tl = s.propagate_batch(scripts, n_vars=n_vars)
        for i, dec in enumerate(scripts):
            c, v, n, _ = ora.bcp(lits, offsets, n_vars, dec)
            assert c == confl[i], (seed, i)
            if c:
                n_conf += 1
            else:
                n_fix += 1
                assert np.array_equal(v, vals[i]) and n == tl[i], (seed, i)
        s.close()
    assert n_fix >= 10 and n_conf >= 5


@pytest.mark.gpu
def test_search_on_long_watch_lists_agrees_with_the_oracle():
    """CDCL on the same kind of formula (tight hub clauses, a random 3-SAT core): verdict = the oracle's, models satisfy
    every clause.  Default fleet, default options."""
    for seed in (21, 22, 25, 26):
        lits, offsets, n_vars, n_hubs, rng = long_list_formula(seed, n_vars=240, n_long=90, per_hub=40, hub_len=(3, 6))
        core = np.arange(n_hubs, n_hubs + 120)
        extra = []
        for _ in range(int(3.0 * 120)):
            vs = rng.choice(core, size=3, replace=False)
            extra.append([int(v + 1) * (1 if rng.random() < 0.5 else -1) for v in vs])
        for h in range(n_hubs):
            for _ in range(3):
                extra.append([-int(rng.choice(core) + 1), h + 1])
        lits = np.concatenate([lits, np.array([l for c in extra for l in c], dtype=np.int32)])
        offsets = np.concatenate([offsets, offsets[-1] + np.cumsum([len(c) for c in extra]).astype(np.uint64)])
        o = ora.OracleSolver()
        o.add_cnf(lits, offsets)
        want = o.solve()
        s = Mi355Sat()
        s.add_cnf(lits, offsets)
        r = s.solve()
        assert (r == SolverResult.Sat) == (want == 10) and r in (SolverResult.Sat, SolverResult.Unsat), (seed, r, want)
        if r == SolverResult.Sat:
            assert ora.check_model(lits, offsets, s.full_solution(n_vars)) == -1
        s.close()

