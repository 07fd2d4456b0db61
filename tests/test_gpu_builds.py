"""All six builds of the search kernel on the MI355X (run with -m gpu): ms_search_kernel<LV, WPS> with the assignment in LDS
or in the slab (LV), compiled for 1, 2 or 4 waves per SIMD (WPS).  The builds are not the same program (the 2-waves build
calls the per-conflict code on register copies; the 4-waves build calls it on the caller's context, has no sort buffer, no
recursive minimisation, no vivification, spills, and keeps its marks as bytes), and launch_slice picks one per launch.  Here
every build is FORCED (opts.one_per_simd, opts.lds_val) - or, for the full fleet, left to the rule - and every test asserts
through mi355sat_debug_last_search_build which build its launches really ran: if the selection rule changes, these tests
fail instead of quietly testing another build.

The judges are the PicoSAT goldens (tests/golden), the oracle (CPU CDCL, RUP checker) and self-certifying models, never
the product.  Every solve runs under solve_within / a deadline: running into the limit fails the test, it never hangs.
Where LDS is forced, workers per CU x (dynamic bytes + 13.2 KB static) stays under 160 KB (asserted from the hook).

Measured on an MI355X: the file takes 93 s (profiles/r04_gpu_builds_durations.log; the rest of the GPU suite 117 s).  The
rect 64x64 sweep decided both loose bounds after 215 steps / 14 s; its ring sample: 500 of 500 records decided (refuted) by
the oracle within the budget, 0 undecided, 0.5 s of oracle time.

The fleet of a batch is rounded down to a multiple of its instances, so a sweep over 25 bounds with workers=4096 runs 4075
workers and one over 10 bounds 4090 (16 waves per CU either way); the hook's `active` is asserted against that.
"""
import threading
import time

import pytest

from helpers import VERDICTS, assert_ring_records_are_implied, assert_search_build, check_sat_answer, make_grid, platform_defs
from oracle import oracle as ora
from test_gpu_parity import HARD_RUNG_LIMIT_S, solve_within
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult

pytestmark = pytest.mark.gpu

BUILD_LIST = [(o, l) for o in (0, 2, 4) for l in (1, -1)]
BUILDS = pytest.mark.parametrize("one_per_simd,lds_val", BUILD_LIST,
                                 ids=[f"{w}-{a}" for w in ("one-wave-build", "two-waves-build", "full-fleet-build") for a in ("lds", "slab")])
STATIC_LDS = 13.2 * 1024       # a workgroup's static LDS in the builds with the sort buffer (the largest)

QUICK = [v for v in VERDICTS["verdicts"] if v["terrain"] in ("rect16x16", "ex2", "rect24x24") and v["picosat_seconds"] < 1.0]
RECT24 = [v for v in VERDICTS["verdicts"] if (v["terrain"], v["platforms"]) == ("rect24x24", "default") and v["k"] in (8, 9, 10)]
# rect 16x16 1x1 k = 14 / 15 on the four called builds too: measured on the MI355X k = 15 (SAT) 0.3-0.7 s, k = 14 (UNSAT) 2.6 s
# (2 waves, LDS), 8.3 s (2 waves, slab), 8.2 s (4 waves, LDS), 11.7 s (4 waves, slab) - under a third of HARD_RUNG_LIMIT_S.
# (Verdicts as in test_gpu_parity.py::test_rect16_with_1x1_supports_only_k15_sat_k14_unsat: k* = 15, PicoSAT 67.5 s for k = 14.)
RECT16_1X1 = [dict(terrain="rect16x16", platforms="1x1", k=15, verdict="SAT", picosat_seconds=67.5),
              dict(terrain="rect16x16", platforms="1x1", k=14, verdict="UNSAT", picosat_seconds=67.5)]
VERDICT_CASES = [(v, o, l) for v in QUICK + RECT24 for o, l in BUILD_LIST] + [(v, o, l) for v in RECT16_1X1 for o, l in BUILD_LIST if o != 0]
BUILD_NAME = {0: "one-wave-build", 2: "two-waves-build", 4: "full-fleet-build"}


def wanted_build(one_per_simd, lds_val):
    return (1 if lds_val == 1 else 0, max(1, one_per_simd))


def assert_build_and_lds_room(s, one_per_simd, lds_val):
    b = assert_search_build(s, *wanted_build(one_per_simd, lds_val))
    per_cu = (b["active"] + 255) // 256
    assert b["dyn_lds_bytes"] == (b["lds_val_bytes"] if lds_val == 1 else 0)
    assert per_cu * (b["dyn_lds_bytes"] + STATIC_LDS) < 160 * 1024, b
    return b


def solve_in_build(cnf, proof=None, **kw):
    """Solve within the limit with the options given.  The default simplification (probing on the device) refutes the
    easiest bounds by itself, before any search launch - then nothing has been said about the build, and the solve is
    repeated with the simplification off (level-0 unit propagation only) so that the search kernel decides it.  Returns
    (solver, result); the solver has launched the search kernel."""
    for simp in (0, -1):
        s = Mi355Sat(simp=simp, **kw)
        if proof:
            s.set_proof_path(proof)
        s.add_cnf(cnf.lits, cnf.offsets)
        r = solve_within(s, HARD_RUNG_LIMIT_S)
        try:
            s.debug_last_search_build()
            return s, r
        except SolverError as e:
            assert e.code == -3 and simp == 0 and r == SolverResult.Unsat, (e, simp, r)   # MI355SAT_ERR_STATE: no search launch yet
            s.close()


def test_the_cases_are_the_ones_meant():
    assert len(RECT16_1X1) == 2 and len(VERDICT_CASES) == 22 * 6 + 2 * 4
    assert len(QUICK) == 19 and [(v["k"], v["verdict"]) for v in RECT24] == [(8, "UNSAT"), (9, "SAT"), (10, "SAT")]


@pytest.mark.parametrize("v,one_per_simd,lds_val", VERDICT_CASES,
                         ids=[f"{v['terrain']}-{v['platforms']}-k{v['k']}-{BUILD_NAME[o]}-{'lds' if l == 1 else 'slab'}" for v, o, l in VERDICT_CASES])
def test_golden_verdicts_in_every_build(v, one_per_simd, lds_val):
    """test_gpu_parity.py::test_golden_verdicts on each build: 256 workers for the quick entries, the default fleet (1024
    workers, after the ramp-up, for rect 24x24 k = 8 / 9 / 10; 256 for rect 16x16 1x1) for the others."""
    grid = make_grid(v["terrain"])
    enc = Encoding.encode(platform_defs(v["platforms"]), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): v["k"]}))
    quick = v["picosat_seconds"] < 1.0
    s, r = solve_in_build(cnf, workers=256 if quick else 0, one_per_simd=one_per_simd, lds_val=lds_val)
    st = s.stats()
    print(f"{v['terrain']} {v['platforms']} k={v['k']} build {wanted_build(one_per_simd, lds_val)}: {r.name} in {st['solve_seconds']:.2f} s")
    assert r.name.upper() == v["verdict"]
    assert_build_and_lds_room(s, one_per_simd, lds_val)
    if r == SolverResult.Sat:
        check_sat_answer(cnf, s.full_solution(cnf.n_vars), enc, grid, v["k"])
    assert st["propagations"] == st["n_deq"] and st["n_clauses"] == cnf.n_clauses and st["max_var"] == cnf.n_vars
    s.close()


@BUILDS
@pytest.mark.parametrize("terrain,pset,k", [("rect8x8", "default", 1), ("rect16x16", "default", 3), ("ex3", "1x1", 3)])
def test_unsat_proofs_of_every_build_pass_the_rup_checker(tmp_path, terrain, pset, k, one_per_simd, lds_val):
    """The build's own derivation - the DRUP log of everything its workers learnt, default options otherwise - verified by
    the oracle's forward RUP checker against the caller's formula."""
    from timberborn_support_solver_amd.dimacs import read_drup
    grid = make_grid(terrain)
    enc = Encoding.encode(platform_defs(pset), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
    proof = str(tmp_path / "p.drup")
    s, r = solve_in_build(cnf, proof=proof, one_per_simd=one_per_simd, lds_val=lds_val)
    assert r == SolverResult.Unsat
    assert_build_and_lds_room(s, one_per_simd, lds_val)
    s.close()
    assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, read_drup(proof)) == 1


@BUILDS
def test_exchange_ring_of_every_build_holds_only_consequences_of_the_formula(one_per_simd, lds_val):
    """test_gpu_parity.py::test_exchange_ring_holds_only_consequences_of_the_formula per build: what this build's workers
    export (and every other worker attaches under its own assumption) follows from the formula alone."""
    grid = make_grid("rect16x16")
    enc = Encoding.encode(platform_defs("default"), grid)
    k0 = 10
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    ks = list(range(k0, -1, -1))
    s = Mi355Sat(workers=44 * len(ks), slice_ms=2, share_lbd=6, one_per_simd=one_per_simd, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    tm = threading.Timer(HARD_RUNG_LIMIT_S, s.interrupter().interrupt)
    tm.start()
    try:
        res = s.solve_batch([([-int(cnf.card_outputs[k])] if k < k0 else []) for k in ks])
    finally:
        tm.cancel()
    assert [r.name for r in res] == ["Sat"] * 7 + ["Unsat"] * 4            # k* = 4
    assert_build_and_lds_room(s, one_per_simd, lds_val)
    st = s.stats()
    assert st["shared_exported"] > 0 and st["shared_imported"] + st["shared_imported_units"] > 0
    assert st["propagations"] == st["n_deq"]
    assert assert_ring_records_are_implied(s, cnf, max_records=3000) > 0
    s.close()


def run_cut_sweep(s, ks, sets, limit_s):
    """The decreasing-k sweep of test_sweep_with_exchange_migration_and_withdrawn_instances_finds_the_cut."""
    s.sweep_begin(sets)
    t0 = time.time()
    res, sat_k, unsat_k = None, None, None
    while time.time() - t0 < limit_s:
        res, _ = s.sweep_step()
        sat_k = min([k for k, r in zip(ks, res) if r == SolverResult.Sat], default=None)
        unsat_k = max([k for k, r in zip(ks, res) if r == SolverResult.Unsat], default=None)
        if sat_k is not None and unsat_k is not None and unsat_k + 1 >= sat_k:
            break
        s.sweep_drop([i for i, k in enumerate(ks) if res[i] == SolverResult.Interrupted and
                      ((sat_k is not None and k > sat_k) or (unsat_k is not None and k < unsat_k))])
    s.sweep_end()
    return res, sat_k, unsat_k


@pytest.mark.parametrize("lds_val", [0, -1], ids=["lds-auto", "slab"])
def test_full_fleet_as_it_really_runs_finds_the_rect24_cut(lds_val):
    """Nothing forced by one_per_simd: 4096 workers asked for, no ramp-up, so 16 waves per CU are co-resident and the rule
    itself picks the 4-waves build; on auto the LDS choice must be what the rule says for this formula without a launch.
    rect 24x24 default as one sweep over k = 24 ... 0: the cut is (9, 8), the model at 9 checks, no bound has a wrong
    verdict, the ring holds consequences only."""
    grid = make_grid("rect24x24")
    enc = Encoding.encode(platform_defs("default"), grid)
    k0 = 24
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    ks = list(range(k0, -1, -1))
    sets = [([-int(cnf.card_outputs[k])] if k < k0 else []) for k in ks]
    s = Mi355Sat(workers=4096, ramp=-1, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    res, sat_k, unsat_k = run_cut_sweep(s, ks, sets, HARD_RUNG_LIMIT_S)
    assert (sat_k, unsat_k) == (9, 8)
    b = s.debug_last_search_build()
    fleet = 4096 // len(ks) * len(ks)                       # 4075: a batch's fleet is a multiple of its instances
    st = s.stats()
    assert b["wps"] == 4 and b["active"] == fleet == st["workers"] and (b["active"] + 255) // 256 == 16
    rule = Mi355Sat.debug_search_build_rule(fleet, b["lds_val_bytes"], lds_val=lds_val, one_per_simd=0)
    assert (b["lds"], b["wps"], b["dyn_lds_bytes"]) == (rule["lds"], rule["wps"], rule["dyn_lds_bytes"])
    assert b["builds"] == {(rule["lds"], 4)}
    if lds_val == -1:
        assert b["lds"] == 0
    check_sat_answer(cnf, s.solution_of(ks.index(9), cnf.n_vars), enc, grid, 9)
    for k, r in zip(ks, res):
        assert r in (SolverResult.Interrupted, SolverResult.Sat if k >= 9 else SolverResult.Unsat), k
    assert st["shared_exported"] > 0 and st["propagations"] == st["n_deq"]
    assert assert_ring_records_are_implied(s, cnf, max_records=3000) > 0
    s.close()


def test_full_fleet_on_the_benchmark_s_workload_rect64():
    """BASELINE configs[4]'s workload - what bench.py times: rect 64x64 default, one sweep over k = 51 ... 44 with the whole
    fleet and the exchange on - plus two loose bounds (200, 120) that are decided.  The loose bounds are SAT with checked
    models of at least 43 platforms (area bound); no tight bound is expected to report in that time (the optimum is not
    known), one that reports SAT must carry a model that checks; counters add up; the hook says 4-waves build, whole fleet.  Ring sample: the first 500 distinct records, each posed to the oracle
    as formula AND NOT(record) with a budget of 20000 conflicts: a satisfiable negation fails at once, at most 10 % may
    stay undecided."""
    grid = make_grid("rect64x64")
    enc = Encoding.encode(platform_defs("default"), grid)
    k0 = 200
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
    loose, tight = [200, 120], list(range(51, 43, -1))
    ks = loose + tight
    sets = [([-int(cnf.card_outputs[k])] if k < k0 else []) for k in ks]
    s = Mi355Sat(workers=4096, ramp=-1)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    s.sweep_begin(sets)
    t0 = time.time()
    steps, res = 0, None
    while time.time() - t0 < HARD_RUNG_LIMIT_S:
        res, _ = s.sweep_step()
        steps += 1
        if steps >= 4 and all(res[i] != SolverResult.Interrupted for i in range(len(loose))):
            break
    t_sweep = time.time() - t0
    models = {i: s.sweep_solution_of(i, cnf.n_vars) for i, r in enumerate(res) if r == SolverResult.Sat}
    s.sweep_end()
    print(f"rect64 sweep: {steps} steps in {t_sweep:.1f} s, results {[r.name for r in res]}")
    assert steps >= 4 and [res[i] for i in range(len(loose))] == [SolverResult.Sat] * len(loose), (steps, t_sweep, res)
    for i, k in enumerate(ks):
        if i in models:                                           # a model is self-certifying, whatever the bound
            lay = check_sat_answer(cnf, models[i], enc, grid, k)
            assert lay.platform_count() >= 43                     # area bound ceil(4096 / 97)
    st = s.stats()
    assert st["propagations"] == st["n_deq"] and st["shared_exported"] > 0
    b = s.debug_last_search_build()
    fleet = 4096 // len(ks) * len(ks)                             # 4090
    assert b["wps"] == 4 and b["active"] == fleet == st["workers"] and (b["active"] + 255) // 256 == 16
    rule = Mi355Sat.debug_search_build_rule(fleet, b["lds_val_bytes"])
    assert (b["lds"], b["dyn_lds_bytes"]) == (rule["lds"], rule["dyn_lds_bytes"]) == (0, 0) and b["builds"] == {(0, 4)}
    # ring sample
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(cnf.n_vars)
    seen, decided, undecided = set(), 0, 0
    t0 = time.time()
    for c in s.debug_share_ring():
        key = tuple(sorted(c))
        if key in seen:
            continue
        seen.add(key)
        assert 1 <= len(c) <= 31 and all(l != 0 and abs(l) <= cnf.n_vars for l in c), c
        r = o.solve([-l for l in c], conflict_budget=20000)
        assert r != 10, ("exchange ring holds a clause the formula does not imply", c)
        decided += r == 20
        undecided += r == 0
        if len(seen) == 500:
            break
    print(f"rect64 ring sample: {decided} decided, {undecided} undecided of {len(seen)}, oracle {time.time() - t0:.1f} s")
    assert len(seen) > 0 and undecided * 10 <= len(seen), (decided, undecided)
    s.close()
