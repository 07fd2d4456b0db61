"""Irreducible failed-assumption cores (mi355sat_minimize_core / _core_of) on the CPU, through the wavefront emulator build
of the solver (tests/emu): the rounds of candidates posed into one resident sweep (sweep_repose), ms_core_model_kernel's
look-up of what a SAT candidate's model falsifies, and the mapping back to the caller's literals.  The judge is the oracle
alone: a minimised core is a core (assert_core), a subsequence of the core before, and the oracle satisfies the formula
under the core without any one of its literals.  Different irreducible cores have different sizes: no size is asserted."""
import os
import subprocess

import numpy as np
import pytest

import simp_cases as sc
from helpers import ROOT, Csr, emu_lib, make_grid, platform_defs
from oracle import oracle as ora
from test_assumption_cores import CASES, ERR_STATE, PAD, assert_core, emu_solver, oracle_solver, padded, sweep_cnf, write_cnf
from timberborn_support_solver_amd import Encoding, PlatformLimits, SolverError, SolverResult
from timberborn_support_solver_amd.solver import ColdReason

PKG = os.path.join(ROOT, "timberborn_support_solver_amd")
ERR_ARG = -4
_anchors = {}


def assert_minimal_core(core, before, assumptions, cnf, n_vars, extra=()):
    assert_core(core, assumptions, cnf, n_vars, extra)
    assert sc.is_subsequence(core, before), (core, before)
    o = oracle_solver(cnf, n_vars, extra)
    for c in core:
        assert o.solve([l for l in core if l != c]) == 10, ("the core is still one without", c, core)


def anchors(terrain):
    """(enc, cnf, "no platform at any anchor"): no platform anywhere cannot support the terrain."""
    if terrain not in _anchors:
        grid = make_grid(terrain)
        enc = Encoding.encode(platform_defs("1x1"), grid)
        cnf = enc.with_limits_into_cnf(PlatformLimits({}))
        _anchors[terrain] = (enc, cnf, [-enc.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)])
    return _anchors[terrain]


def with_padding(a, n_vars, n_pad):
    """n_pad literals over fresh, unconstrained variables spread among a."""
    out, step = [], -(-n_pad // len(a))
    pad = [(n_vars + 1 + i) * (1 if i % 2 else -1) for i in range(n_pad)]
    for i, l in enumerate(a):
        out.append(l)
        out.extend(pad[i * step:(i + 1) * step])
    assert len(out) == len(a) + n_pad
    return out, n_vars + n_pad


def no_core(s):
    for fn in (s.core, s.minimize_core):
        with pytest.raises(SolverError) as e:
            fn()
        assert e.value.code == ERR_STATE


def minimized(s, a, cnf, n_vars, extra=(), **kw):
    """solve(a) is UNSAT; minimise; the checks every case shares.  Returns (before, core, info)."""
    assert s.solve(a) == SolverResult.Unsat
    before = s.core()
    n0 = {k: v for k, v in s.stats().items() if k in ("n_sat", "n_unsat", "n_terminated", "workers", "simp_units", "simp_equivalences",
                                                     "simp_clauses_removed", "simp_eliminated")}
    info = s.minimize_core(**kw)
    core = s.core()
    print("core", len(before), "->", len(core), info)
    assert info["size_before"] == len(before) and info["size_after"] == len(core)
    assert info["candidates_sat"] + info["candidates_unsat"] <= info["candidates"]
    assert list(dict.fromkeys(l for l in a if s.failed(l))) == core     # (a may repeat literals; a core does not)
    assert {k: v for k, v in s.stats().items() if k in n0} == n0          # no results of the caller's; its solve's counters stay
    if info["minimal"]:
        assert_minimal_core(core, before, a, cnf, n_vars, extra)
    else:
        assert_core(core, a, cnf, n_vars, extra)
        assert sc.is_subsequence(core, before)
    return before, core, info


# 1. forbidden anchors
@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("lds_val", [0, -1])
def test_forbidden_anchors(seed, lds_val):
    enc, cnf, a = anchors("rect8x8")
    s = emu_solver(seed=seed, lds_val=lds_val, workers=3)
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized(s, a, cnf, cnf.n_vars)
    assert info["minimal"] == 1 and 0 < len(core) <= len(before) < len(a)
    assert s.solve() == SolverResult.Sat
    no_core(s)
    s.close()


# 2. rounds of chunks; what ms_core_model_kernel reads and how its bits map back
@pytest.mark.parametrize("workers,lds_val", [(2, 0), (4, -1)])
def test_chunked_rounds_and_critical_literals_by_model(workers, lds_val):
    """At most 4 candidates a round: chunks of several literals, so a SAT candidate names a critical literal only through
    its model.  "Every literal counted in critical_by_model is in the final core" is checked by a SUBSTITUTE: the info
    struct holds a count, no identities, so membership cannot be read from outside.  What stands in for it: the loop fails
    with MI355SAT_ERR_STATE when a core it adopts lacks a literal it holds critical (crit inside F), so a call that returns
    0 kept every one of them; and a literal the kernel or the mapping named wrongly, which is not critical, then sits in
    the final core, where the oracle's minimality check (assert_minimal_core) finds it.  The count is bounded by the core."""
    enc, cnf, a0 = anchors("rect8x8")
    a, nv = with_padding(a0, cnf.n_vars, 200)
    s = emu_solver(workers=workers, lds_val=lds_val)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    s.debug_core_min_round(4)
    before, core, info = minimized(s, a, cnf, nv)
    assert not set(before) - set(a0)                      # un-minimised, the padding is not in the core
    assert info["minimal"] == 1 and info["rounds"] > 1 and info["model_launches"] > 0
    assert 0 < info["critical_by_model"] <= len(core)     # (every critical literal is in every later core)
    s.close()


def wide_clause_case(n=130):
    """x_i -> y_i, one clause of all the NOT y_i, and x_64 AND x_65 refuted by a case split that unit propagation does not
    see.  Under x_1 .. x_n the final conflict is the wide clause: a core of all n literals, of which two are needed.  With
    two candidates a round the first leaves out x_1 .. x_65 - a list of more than 64 literals, as is what it assumes: both
    lists take ms_core_model_kernel through a second ballot round - and, every variable hinted TRUE, its model falsifies
    one of x_64 / x_65 alone: the bit at index 63 or 64."""
    x = list(range(1, n + 1))
    r1, r2 = 2 * n + 1, 2 * n + 2
    cl = [[-v, n + v] for v in x] + [[-(n + v) for v in x]] + [[-64, -65, p, q] for p in (r1, -r1) for q in (r2, -r2)]
    return Csr(cl, 2 * n + 2), x, [64, 65]


def test_lists_longer_than_one_ballot_round():
    cnf, a, want = wide_clause_case()
    s = emu_solver(workers=2)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.set_phases([1] * (cnf.n_vars - 2))
    s.debug_core_min_round(2)
    before, core, info = minimized(s, a, cnf, cnf.n_vars)
    assert before == a                                    # (what the case is built for)
    assert core == want and info["minimal"] == 1
    assert info["model_launches"] > 0 and info["critical_by_model"] > 0 and info["candidates_unsat"] > 0
    s.close()


# 3. already minimal
@pytest.mark.parametrize("terrain,pset,k_unsat,k_sat", CASES, ids=lambda x: str(x))
def test_one_literal_core(terrain, pset, k_unsat, k_sat):
    enc, cnf = sweep_cnf(terrain, pset)
    a, nv = padded(cnf, k_unsat)
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    before, core, info = minimized(s, a, cnf, nv)
    assert before == core == [-int(cnf.card_outputs[k_unsat])]
    assert info["minimal"] == 1 and info["candidates"] <= 1 and info["model_launches"] == 0
    s.close()


def test_one_literal_core_after_a_sat_answer_costs_nothing():
    """The refinement loop's sequence - a satisfiable bound, then the bound below it posed as an assumption: the handle
    knows that the formula alone has a model."""
    enc, cnf = sweep_cnf("ex1", "1x1")
    a, nv = padded(cnf, 2)
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    assert s.solve(padded(cnf, 3)[0]) == SolverResult.Sat
    assert s.solve(a) == SolverResult.Unsat
    launches = s.stats()["kernel_launches"]
    info = s.minimize_core()
    assert s.core() == [-int(cnf.card_outputs[2])] and info["minimal"] == 1 and info["candidates"] == 0
    assert s.stats()["kernel_launches"] == launches
    s.add_clause([nv, -nv])                               # a clause since: no longer known
    assert s.solve(a) == SolverResult.Unsat
    assert s.minimize_core()["candidates"] == 1 and s.core() == [-int(cnf.card_outputs[2])]
    s.close()


def test_contradicting_pair_stays():
    enc, cnf = sweep_cnf("ex1", "1x1")
    x = enc.platform_var(1, 1, (1, 1))
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized(s, [x, -x], cnf, cnf.n_vars)
    assert before == core == [x, -x] and info["minimal"] == 1 and info["candidates"] == 2
    s.close()


# 4. formula UNSAT alone
def test_formula_unsat_by_itself():
    grid = make_grid("ex1")
    enc = Encoding.encode(platform_defs("1x1"), grid)
    cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 1}))   # UNSAT without any assumption
    nv = cnf.n_vars
    s = emu_solver()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv + PAD)
    before, core, info = minimized(s, [nv + 1 + i for i in range(PAD)], cnf, nv + PAD)
    assert before == core == []
    assert (info["minimal"], info["candidates"], info["model_launches"], info["rounds"]) == (1, 0, 0, 0)
    s.close()


# 5. repeats and equivalent literals
@pytest.mark.parametrize("simp", [-1, 0])
def test_repeats_and_equivalent_literals(simp):
    """Every anchor assumed twice, and next to the first eight a fresh variable that two binary clauses make equivalent to
    it (simp = 0 substitutes it: both literals are one on the device; simp = -1 leaves two variables that imply each other)."""
    enc, cnf, a0 = anchors("rect8x8")
    nv = cnf.n_vars
    extra, a = [], []
    for i, l in enumerate(a0):
        a += [l, l]
        if i < 8:
            e = nv + 1 + i
            extra += [[-e, -l], [e, l]]          # e == var(l)
            a += [-e, l]
    s = emu_solver(simp=simp, workers=3)
    s.add_cnf(cnf.lits, cnf.offsets)
    for c in extra:
        s.add_clause(c)
    before, core, info = minimized(s, a, cnf, nv + 8, extra=extra)
    assert info["minimal"] == 1
    s.close()


# 6. state rules
def test_state_rules():
    enc, cnf, a = anchors("rect8x8")
    s = emu_solver(workers=3)
    no_core(s)                                            # before any solve
    s.add_cnf(cnf.lits, cnf.offsets)
    no_core(s)
    assert s.solve() == SolverResult.Sat
    no_core(s)                                            # after SAT
    before, core, info = minimized(s, a, cnf, cnf.n_vars)
    assert info["minimal"] == 1
    again = s.minimize_core()                             # the flag is kept with the core: nothing is posed again
    assert s.core() == core and again["minimal"] == 1 and again["candidates"] == 0 and again["size_before"] == len(core)
    s.assume(a[0])
    no_core(s)                                            # an assumption since
    assert s.solve(a) == SolverResult.Unsat
    s.add_clause([1, 2])
    no_core(s)                                            # a clause since
    with pytest.raises(SolverError):
        s.minimize_core(conflict_budget=-1)
    # batch: a SAT instance has no core to minimise; an instance out of range neither
    res = s.solve_batch([a, a[:3]])
    assert [r.name for r in res] == ["Unsat", "Sat"]
    with pytest.raises(SolverError) as e:
        s.minimize_core_of(1)
    assert e.value.code == ERR_STATE
    with pytest.raises(SolverError) as e:
        s.minimize_core_of(2)
    assert e.value.code == ERR_ARG                        # (as core_of: out of range after a batch)
    no_core(s)                                            # (the plain solve's core went with the clause)
    s.close()


# 7. interrupt
def test_interrupt_before_the_call_leaves_the_core():
    enc, cnf, a = anchors("rect8x8")
    s = emu_solver(workers=3)
    s.add_cnf(cnf.lits, cnf.offsets)
    assert s.solve(a) == SolverResult.Unsat
    before = s.core()
    launches = s.stats()["kernel_launches"]
    s.interrupter().interrupt()
    info = s.minimize_core()
    assert info["minimal"] == 0 and info["candidates"] == 0 and s.core() == before
    assert s.stats()["kernel_launches"] == launches
    assert_core(before, a, cnf, cnf.n_vars)
    info = s.minimize_core()                              # the interrupt is consumed
    assert info["minimal"] == 1
    assert_minimal_core(s.core(), before, a, cnf, cnf.n_vars)
    s.interrupter().interrupt()
    s.minimize_core()
    assert s.solve() == SolverResult.Sat                  # ... also for the solve that follows
    s.close()


# 8. budget
def test_conflict_budget():
    enc, cnf, a = anchors("rect8x8")
    s = emu_solver(workers=3, seed=3)
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized(s, a, cnf, cnf.n_vars, conflict_budget=1)     # (judged by `minimal`, either way)
    assert len(core) <= len(before)
    s.close()


# 9. batch
def test_batch():
    """Forbidden-anchor subsets and padded bounds over one formula (ex1: the rect8x8 sets take the emulator a minute)."""
    grid = make_grid("ex1")
    enc2, cnf2 = sweep_cnf("ex1", "1x1")
    a = [-enc2.platform_var(x, y, (1, 1)) for y in range(grid.height) for x in range(grid.width)]
    nv = cnf2.n_vars + 20
    bound = lambda k, i: [cnf2.n_vars + 1 + i, -int(cnf2.card_outputs[k]), -(cnf2.n_vars + 10 + i)]
    sets = [a, bound(2, 0), bound(4, 1), a[:len(a) // 2], a[3:] + bound(6, 2), bound(1, 3), a[::2], a[::-1]]
    o = oracle_solver(cnf2, nv)
    want = [o.solve(x) for x in sets]
    assert want.count(10) >= 2 and want.count(20) >= 4
    s = emu_solver(workers=8)
    s.add_cnf(cnf2.lits, cnf2.offsets)
    s.reserve(nv)
    res = s.solve_batch(sets)
    assert [r.value for r in res] == want
    cores = {i: s.core_of(i) for i, r in enumerate(res) if r == SolverResult.Unsat}
    for i in cores:
        info = s.minimize_core_of(i)
        core = s.core_of(i)
        print(i, len(cores[i]), "->", len(core), info)
        assert info["minimal"] == 1 and info["size_after"] == len(core)
        assert_minimal_core(core, cores[i], sets[i], cnf2, nv)
        for j in cores:                                   # the others stay readable and unchanged
            if j > i:
                assert s.core_of(j) == cores[j]
    for j, r in enumerate(res):                           # the models of the SAT instances too
        if r == SolverResult.Sat:
            m = s.solution_of(j, nv)
            assert ora.check_model(cnf2.lits, cnf2.offsets, m[:cnf2.n_vars]) == -1
            assert all(m[abs(l) - 1] == (1 if l > 0 else -1) for l in sets[j])
    s.close()


# 10. simplification and variable order
@pytest.mark.parametrize("kw", [dict(simp=0), dict(simp=2), dict(var_order=1), dict(simp=2, var_order=1, workers=4)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_across_configurations(kw):
    enc, cnf, a0 = anchors("rect8x8")
    a, nv = with_padding(a0, cnf.n_vars, 30)
    s = emu_solver(**dict(dict(workers=3), **kw))
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(nv)
    s.debug_core_min_round(3)
    before, core, info = minimized(s, a, cnf, nv)
    assert info["minimal"] == 1
    assert s.solve(core[1:]) == SolverResult.Sat          # models in the caller's variables
    assert ora.check_model(cnf.lits, cnf.offsets, s.full_solution(cnf.n_vars)) == -1
    s.close()


# 11. fuzz: planted-structure formulas (helpers.structured_cnf through simp_cases) under seeded assumption sets
# (case of simp_cases.EMU_CASES, seed): chosen with the oracle alone - UNSAT under the set, and the oracle's own deletion
# leaves at least 3 literals
FUZZ = [("equiv-n48-s1", 6), ("failed-n48-s2", 2), ("failed-n48-s2", 19), ("failed-n48-s2", 25), ("subsume-n40-s3", 21),
        ("subsume-n40-s3", 35), ("strengthen-n45-s4", 16), ("strengthen-n45-s4", 32), ("elim-n50-s6", 17), ("elim-n50-s6", 18),
        ("salt-n40-s7", 4), ("salt-n40-s7", 22)]


def fuzz_set(name, seed):
    case = sc.EMU_CASES[name]
    cnf, want, special = sc.formula(case)
    rng = np.random.default_rng(9000 + 100 * case[0] + seed)
    a = []
    for _ in range(int(rng.integers(8, 20))):
        v = int(rng.choice(special)) if special and rng.random() < 0.3 else int(rng.integers(cnf.n_vars)) + 1
        a.append(v if rng.random() < 0.5 else -v)
    return cnf, a


def oracle_deletion_core(o, a):
    core = list(dict.fromkeys(a))
    for l in list(core):
        rest = [x for x in core if x != l]
        if o.solve(rest) == 20:
            core = rest
    return core


def test_fuzz_inputs_are_what_they_were_chosen_for():
    assert len(FUZZ) >= 10
    for name, seed in FUZZ:
        cnf, a = fuzz_set(name, seed)
        o = sc.oracle_for(cnf, cnf.n_vars)
        assert o.solve(a) == 20 and len(oracle_deletion_core(o, a)) >= 3, (name, seed)


@pytest.mark.parametrize("name,seed", FUZZ)
@pytest.mark.parametrize("simp", [0, 2])
def test_fuzz(name, seed, simp):
    cnf, a = fuzz_set(name, seed)
    s = emu_solver(simp=simp, workers=3, slice_conflicts=100)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    s.debug_core_min_round(2 if seed % 2 else 0)
    before, core, info = minimized(s, a, cnf, cnf.n_vars)
    assert info["minimal"] == 1
    s.close()


# 12. warm mode
def test_warm_mode_starts_cold_afterwards():
    enc, cnf, a = anchors("rect8x8")
    s = emu_solver(workers=3)
    s.set_incremental(True)
    s.add_cnf(cnf.lits, cnf.offsets)
    before, core, info = minimized(s, a, cnf, cnf.n_vars)
    assert info["minimal"] == 1 and info["candidates"] > 0
    assert s.solve(core[1:]) == SolverResult.Sat
    d = s.debug_incremental()
    assert d["last_cold_reason"] == ColdReason.OTHER_SEARCH and (d["warm_solves"], d["cold_solves"]) == (0, 2), d
    assert s.solve(core) == SolverResult.Unsat and s.debug_incremental()["warm_solves"] == 1
    s.close()


# 13. the C header: tests/abi_core_minimize.c (what the Rust shim's minimize_core calls, replayed in C)
def build_abi_core_minimize(tmp_path, libdir, libname):
    exe = str(tmp_path / ("abi_core_minimize_" + libname))
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "abi_core_minimize.c"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir])
    return exe


def run_abi_core_minimize(exe, tmp_path, cnf, workers, max_candidates, assumptions, timeout=600):
    """(core before, core after, the info line's numbers)."""
    path = str(tmp_path / "cnf.bin")
    write_cnf(path, cnf)
    out = subprocess.run([exe, path, str(workers), str(max_candidates)] + [str(l) for l in assumptions], capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, (out.stdout, out.stderr)
    line = {l.split()[0]: [int(t) for t in l.split()[1:]] for l in out.stdout.splitlines()}
    assert line["result"] == [20] and line["again"] == [10], out.stdout
    return line["core"][1:], line["min"][1:], line["info"]


def test_abi_core_minimize_builds_against_the_header_and_library(tmp_path):
    exe = build_abi_core_minimize(tmp_path, PKG, "mi355sat")
    assert subprocess.run([exe], capture_output=True).returncode == 2     # usage error: main() was reached


def test_abi_core_minimize_call_sequence_on_the_emulator(tmp_path):
    emu_lib()    # (builds tests/emu/libmi355sat_emu.so)
    exe = build_abi_core_minimize(tmp_path, os.path.join(ROOT, "tests", "emu"), "mi355sat_emu")
    enc, cnf, a = anchors("rect8x8")
    before, core, info = run_abi_core_minimize(exe, tmp_path, cnf, 3, 4, a)
    assert info[0] == 1
    assert_minimal_core(core, before, a, cnf, cnf.n_vars)
