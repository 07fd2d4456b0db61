"""The search at the edges of a worker's device stores, written once for the emulator and the GPU
(tests/test_emu_capacity.py, test_gpu_capacity.py).

Every other test runs with stores thousands of times larger than it needs (32768 learnt-clause slots, 512 K literal words,
a watch pool for a dense layout of all of them, a million proof words), so the code that runs when one is nearly full -
the early reduction at 7/8, add_learnt's inline reduction, the watch-pool collection at 3/4, the clean errors when nothing
helps, the exchange's "no room" rule, a proof log that drops deletion lines - is reached through the test hook
mi355sat_debug_set_capacities only.  The judge is never the product: verdicts are the oracle's, models go through
oracle.check_model, proofs through oracle.check_rup with and without their deletion lines, ring records are refuted by the
oracle when negated, and the counters of mi355sat_debug_capacities prove that the path under test ran.

Formulas: uniform random 3-SAT, helpers.random_cnf(seed, 80, 344) for seeds 0..7 (4.3 clauses per variable; four of each
verdict, 75 .. 1055 conflicts of a three-worker emulator fleet at 64 slots), with reduce_first = 1000000: no reduction is
ever due by conflicts, so every one that happens is the store's doing."""
import numpy as np

from helpers import Csr, assert_ring_records_are_implied, assert_search_build, random_cnf
from oracle import oracle as ora
from timberborn_support_solver_amd import ColdReason, SolverError, SolverResult
from timberborn_support_solver_amd.dimacs import read_drup

SEEDS = tuple(range(8))
VERDICTS = {0: 20, 1: 10, 2: 20, 3: 20, 4: 10, 5: 20, 6: 10, 7: 10}       # the oracle's, asserted in formula()
UNSAT_SEEDS = tuple(s for s in SEEDS if VERDICTS[s] == 20)
SAT_SEEDS = tuple(s for s in SEEDS if VERDICTS[s] == 10)
NO_SCHEDULED_REDUCTION = dict(reduce_first=1000000)
EMU_OPTS = dict(workers=3, slice_conflicts=100, simp=-1)
GPU_OPTS = dict(workers=64, ramp=-1, deterministic=1, slice_conflicts=100, simp=-1)

# (one_per_simd, lds_val) of the six builds of the search kernel, and the waves per SIMD each one_per_simd selects in a fleet of 64
BUILDS = [(o, l) for l in (1, -1) for o in (0, 2, -1)]
BUILD_IDS = [f"{w}-{a}" for a in ("lds", "slab") for w in ("one-wave-build", "two-waves-build", "full-fleet-build")]
WPS = {0: 1, 2: 2, -1: 4}
# one UNSAT and one SAT seed per build, every seed on some build
BUILD_SEEDS = [(b, seed) for i, b in enumerate(BUILDS) for seed in (UNSAT_SEEDS[i % 4], SAT_SEEDS[i % 4])]
BUILD_SEED_IDS = [f"{BUILD_IDS[i // 2]}-seed{seed}" for i, (b, seed) in enumerate(BUILD_SEEDS)]

SLOTS = dict(learnt_cap=64)                                  # (a)
LITERALS = dict(learnt_cap=128, learnt_lit_cap=1024)         # (b)
POOL_LOW = dict(learnt_cap=64, pool_slack=400)               # (c)
POOL_OUT = dict(pool_slack=64)                               # (d), with reduce_first = 40, reduce_inc = 10
SLOTS_OUT = dict(learnt_cap=4)                               # (d)
ERR_OOM, ERR_STATE = -1, -3
POOL_TEXT, LEARNT_TEXT, PROOF_TEXT = "device watch pool exhausted", "device learnt-clause store exhausted", "proof buffer overflow"

_formulas = {}


def formula(seed, n_vars=80, n_clauses=344):
    """(Csr, the oracle's verdict) of random_cnf(seed, n_vars, n_clauses), computed once."""
    key = (seed, n_vars, n_clauses)
    if key not in _formulas:
        cnf = Csr(random_cnf(seed, n_vars, n_clauses), n_vars)
        want = oracle_of(cnf).solve()
        if (n_vars, n_clauses) == (80, 344):
            assert want == VERDICTS[seed], (seed, want)
        _formulas[key] = (cnf, want)
    return _formulas[key]


def oracle_of(cnf):
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(cnf.n_vars)
    return o


def load(s, cnf):
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)


def judge_answer(s, cnf, want, r, proof):
    """The verdict is the oracle's; a model satisfies every clause; a proof is RUP line by line - with its deletion lines
    (a reduction under pressure writes them while it moves the literals they name) and without them."""
    assert r.value == want, (r, want)
    if r == SolverResult.Sat:
        assert ora.check_model(cnf.lits, cnf.offsets, s.full_solution(cnf.n_vars)) == -1
    elif proof is not None:
        with_d, without_d = read_drup(proof), read_drup(proof, deletions=False)
        assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, with_d) == 1
        assert ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, without_d) == 1
        return int(np.count_nonzero(with_d == -2 ** 31))
    return 0


def solve_at(make_solver, seed, caps, tmp_path, build=None, solve=None, **opts):
    """One solve of formula(seed) with the stores sized by `caps`, judged; returns (solver, stats, capacity info, deletion
    lines in the proof).  The caller closes."""
    cnf, want = formula(seed)
    kw = dict(NO_SCHEDULED_REDUCTION, **opts)
    if build:
        kw.update(one_per_simd=build[0], lds_val=build[1])
    s = make_solver(**kw)
    s.debug_set_capacities(**caps)
    proof = str(tmp_path / "capacity.drup") if want == 20 else None
    if proof:
        s.set_proof_path(proof)
    load(s, cnf)
    r = solve(s) if solve else s.solve()
    n_del = judge_answer(s, cnf, want, r, proof)
    if build:
        assert_search_build(s, 1 if build[1] == 1 else 0, WPS[build[0]])
    assert_ring_records_are_implied(s, cnf)
    st, info = s.stats(), s.debug_capacities()
    print("seed", seed, caps, build, r.name, "conflicts", st["conflicts"], "reduce_dbs", st["reduce_dbs"], "learnts", st["learnts"],
          "literals", st["learnt_literals"], "deletion lines", n_del, info)
    W = st["workers"]
    for k, v in caps.items():
        if k != "pool_slack":
            assert info[k] == v, (k, info)
    if "pool_slack" in caps:
        assert info["pool_cap"] == info["pool_initial"] + caps["pool_slack"], info
    assert (info["proof_cap"] > 0) == (proof is not None)
    assert st["learnts"] <= W * info["learnt_cap"] and st["learnt_literals"] <= W * info["learnt_lit_cap"], (st, info)
    return s, st, info, n_del


def pressure_must_show(st, info):
    """Whether a run without a single pressure reduction would be a fault.  Some worker made at least the mean number of
    conflicts; at twice the slot count it cannot have stored its clauses without a reduction (the clauses a conflict does
    not store are units, and a formula of 80 variables does not survive 64 of them)."""
    return st["conflicts"] >= 2 * info["learnt_cap"] * st["workers"]


def assert_pressure(st, info, n_del=None):
    """The 7/8 rule ran: with no reduction ever due by conflicts, stats' reduce_dbs counts exactly the reductions that
    on_fixpoint_body started because the store passed 7/8; pressure_reduces counts those and add_learnt's inline ones."""
    assert info["pressure_reduces"] > 0 and st["reduce_dbs"] > 0, (st, info)
    assert info["pressure_reduces"] >= st["reduce_dbs"]


_tally = {}


def tallied(target, case, seed, run):
    """The counters of one (target, case, seed) run, computed once: the per-seed tests leave them here and the tests over
    the whole set (at least three of the four UNSAT seeds; a sum over the set) take them from here - or run what is missing,
    so that they do not depend on the order of the tests."""
    key = (target, case, seed)
    if key not in _tally:
        s, st, info, n_del = run()
        s.close()
        _tally[key] = (st, info, n_del)
    return _tally[key]


def check_case(make_solver, target, case, caps, seed, tmp_path, **kw):
    return tallied(target, case, seed, lambda: solve_at(make_solver, seed, caps, tmp_path, **kw))


def check_pressure_on_most_unsat_seeds(make_solver, target, case, caps, tmp_path, **kw):
    """A run in which no worker reached 57 conflicts proves nothing about the 7/8 rule, so: on at least three of the four
    UNSAT seeds."""
    hits = 0
    for seed in UNSAT_SEEDS:
        st, info, n_del = check_case(make_solver, target, case, caps, seed, tmp_path, **kw)
        hits += 1 if info["pressure_reduces"] > 0 and st["reduce_dbs"] > 0 else 0
    assert hits >= 3, hits


def check_pool_rebuilds_over_the_set(make_solver, target, tmp_path, seeds=SEEDS, **kw):
    total = sum(check_case(make_solver, target, "c", POOL_LOW, seed, tmp_path, **kw)[1]["pool_rebuilds"] for seed in seeds)
    assert total > 0


def check_pool_low_under_assumptions(make_solver, seed, tmp_path, solve=None, **opts):
    """(c) under assumptions.  The collection itself is one statement in on_fixpoint_body; what differs is how a fixpoint
    gets there.  Without assumptions and with no maintenance due, the search kernel's decision branch sends it there for
    the pool's sake alone (its own copy of the 3/4 test); while a worker stands below its assumption levels - after every
    restart and every backjump into them - the branch takes the full path anyway.  This case runs the second way in: two
    assumptions (more would decide these formulas before a pool fills), taken from a model of the oracle's where the formula has one (the answer stays SAT, the model must keep
    them), and the same literals negated where it has none."""
    cnf, want = formula(seed)
    o = oracle_of(cnf)
    if want == 10:
        assert o.solve() == 10
        m = o.model(cnf.n_vars)
        assumptions = [int(v) * (1 if m[v - 1] > 0 else -1) for v in (3, 43)]
    else:
        assumptions = [-3, 43]
    want_a = oracle_of(cnf).solve(assumptions)
    s = make_solver(**dict(NO_SCHEDULED_REDUCTION, **opts))
    s.debug_set_capacities(**POOL_LOW)
    load(s, cnf)
    r = solve(s, assumptions) if solve else s.solve(assumptions)
    assert r.value == want_a, (r, want_a)
    if r == SolverResult.Sat:
        m = s.full_solution(cnf.n_vars)
        assert ora.check_model(cnf.lits, cnf.offsets, m) == -1
        assert all(m[abs(l) - 1] == (1 if l > 0 else -1) for l in assumptions)
    else:
        core = s.core()
        assert set(core) <= set(assumptions) and oracle_of(cnf).solve(core) == 20, core
    assert_ring_records_are_implied(s, cnf)
    st, info = s.stats(), s.debug_capacities()
    print("seed", seed, "assumptions", assumptions, r.name, "conflicts", st["conflicts"], info)
    s.close()
    return info["pool_rebuilds"]


def check_exhaustion(make_solver, seed, caps, text, tmp_path, solve=None, **opts):
    """(d) A store that is too small may fail the solve - with MI355SAT_ERR_OOM and the store's name, never with a wrong
    verdict - and the handle survives: failed / core answer ERR_STATE, and with the rules back the same handle decides the
    same formula as the oracle does, from a cold start.  A build that gets through at these sizes must be right instead."""
    cnf, want = formula(seed)
    s = make_solver(**opts)
    s.set_incremental(True)
    s.debug_set_capacities(**caps)
    load(s, cnf)
    failed = False
    try:
        r = solve(s) if solve else s.solve()
        judge_answer(s, cnf, want, r, None)
    except SolverError as e:
        failed = True
        assert e.code == ERR_OOM and text in str(e), e
        for ask in (lambda: s.failed(1), s.core):
            try:
                ask()
                assert False, "failed / core answered after a failed solve"
            except SolverError as e2:
                assert e2.code == ERR_STATE, e2
    info = s.debug_capacities()
    print("seed", seed, caps, "failed" if failed else "decided", info)
    s.debug_set_capacities(0, 0, 0, 0)
    before = s.debug_incremental()
    r = solve(s) if solve else s.solve()
    judge_answer(s, cnf, want, r, None)
    i = s.debug_incremental()
    if failed:
        assert i["last_cold_reason"] == ColdReason.FIRST and i["cold_solves"] == before["cold_solves"] + 1, i
        assert s.debug_capacities()["learnt_cap"] >= 32768
    s.close()
    return failed


# ---- (e) an import never fails a solve ------------------------------------------------------------------------------------
CHAIN = 40


def chain_formula(seed, n_vars, n_clauses):
    """Implication chains a1 -> a2 -> ... -> a40 as binary clauses over the variables 1..40 (every (~a_i | a_j), i < j, is
    implied), next to a random 3-SAT part over the variables above them that takes a search."""
    chain = [[-i, i + 1] for i in range(1, CHAIN)]
    rest = [[l + CHAIN if l > 0 else l - CHAIN for l in c] for c in random_cnf(seed, n_vars, n_clauses)]
    return Csr(chain + rest, CHAIN + n_vars)


def implied_binaries(n=60):
    """n records [lbd 3, ~a_i, a_j, 0] with i + 1 < j, spread over the chain."""
    pairs = [(i, j) for i in range(1, CHAIN - 1) for j in range(i + 2, CHAIN + 1)]
    step = len(pairs) // n
    return [[3, -i, j, 0] for i, j in pairs[::step][:n]]


def check_imports_never_fail_a_solve(make_solver, case_seed, n_vars, n_clauses, step=None, **opts):
    """Eight learnt-clause slots, sixty implied binary clauses from another handle.  A binary clause is never reduced away,
    so a worker that attached all it was handed would have no slot left for the next clause it learns itself - which is
    MI355SAT_ERR_OOM - over clauses it could do without.  The exchange passes them over once the store is three quarters
    full (imports_dropped_full) and the sweep ends with the oracle's verdict."""
    cnf = chain_formula(case_seed, n_vars, n_clauses)
    want = oracle_of(cnf).solve()
    recs = implied_binaries()
    o = oracle_of(cnf)
    for rec in recs:
        assert o.solve([-l for l in rec[1:-1]]) == 20, rec       # as assert_ring_records_are_implied does
    s = make_solver(**opts)
    s.debug_set_capacities(learnt_cap=8)
    load(s, cnf)
    s.sweep_begin([[]])
    step = step or (lambda s: s.sweep_step())
    res, nd = step(s)
    assert nd == 0, "the formula was decided before the import: the case proves nothing"
    assert s.share_import(np.asarray([w for rec in recs for w in rec], dtype=np.int32)) == len(recs)
    n_steps = 1
    while nd == 0:
        res, nd = step(s)
        n_steps += 1
        assert n_steps < 400
    assert res[0].value == want, (res, want)
    if res[0] == SolverResult.Sat:
        assert ora.check_model(cnf.lits, cnf.offsets, s.sweep_solution_of(0, cnf.n_vars)) == -1
    assert_ring_records_are_implied(s, cnf)
    st, info = s.stats(), s.debug_capacities()
    s.sweep_end()
    print("verdict", res[0].name, "steps", n_steps, "conflicts", st["conflicts"], "imported", st["shared_imported"], info)
    assert info["learnt_cap"] == 8 and st["shared_imported"] > 0 and info["imports_dropped_full"] > 0, (st, info)
    assert st["learnts"] <= st["workers"] * 8
    s.close()


# Both targets run this case with three workers in the deterministic mode, in which a run is a function of its inputs on
# the emulator and on the GPU alike.  Eight slots are very few: the clauses a worker learns itself and may not drop (LBD <= 2,
# reasons) exhaust them on most formulas that take more than a few dozen conflicts, imports or not - which is the documented
# MI355SAT_ERR_OOM, not this case's subject.  random_cnf(1, 40, 170) next to the chains is SAT after 42 conflicts of this fleet
# without the imports, so that the imports are what the run with them is about.
IMPORT_CASE = (1, 40, 170)
IMPORT_OPTS = dict(workers=3, slice_conflicts=5, share_interval=1, deterministic=1, seed=7, simp=-1)


# ---- (f) the proof log ------------------------------------------------------------------------------------------------------
def check_proof_log(make_solver, case_seed, proof_cap, tmp_path, expect_overflow, solve=None, **opts):
    """Returns the number of deletion lines in the proof, or None after an overflow."""
    seed = case_seed
    cnf, want = formula(seed)
    assert want == 20
    s = make_solver(**dict(NO_SCHEDULED_REDUCTION, **opts))
    s.debug_set_capacities(learnt_cap=64, proof_cap=proof_cap)
    proof = str(tmp_path / "small-log.drup")
    s.set_proof_path(proof)
    load(s, cnf)
    n_del = None
    try:
        r = solve(s) if solve else s.solve()
        assert not expect_overflow, "a log of %d words held every lemma" % proof_cap
        n_del = judge_answer(s, cnf, want, r, proof)
        st, info = s.stats(), s.debug_capacities()
        print("seed", seed, "proof_cap", proof_cap, "deletion lines", n_del, "reduce_dbs", st["reduce_dbs"], info)
        assert info["proof_cap"] == proof_cap and info["pressure_reduces"] > 0
    except SolverError as e:
        assert expect_overflow, e
        assert e.code == ERR_OOM and PROOF_TEXT in str(e), e
        # the file is closed: what was written is on disk, complete lines only, and the path can be written again
        text = open(proof).read()
        assert text == "" or text.endswith("\n")
        s.set_proof_path(None)
        s.debug_set_capacities(0, 0, 0, 0)
        r = solve(s) if solve else s.solve()
        judge_answer(s, cnf, want, r, None)
    s.close()
    return n_del


# ---- (g) warm-start fallbacks that a store's size decides ------------------------------------------------------------------
def easy_formula(seed=11, n_vars=60, n_clauses=120):
    """Random 3-SAT at two clauses per variable: satisfiable, decided in a handful of conflicts - the cold solves of the
    cases below are not what they are about.  (Its clauses are ternary: they live in the shared CSR, the watch pool holds
    the empty lists only.)"""
    return formula(seed, n_vars, n_clauses)


def check_cold_for_assumption_room(checked_solver):
    """257 more assumptions than at the last cold start (which had none, and left room for 256)."""
    c = checked_solver(n_vars=60 + 300)
    c.solve(expect=SolverResult.Sat)
    c.solve([61 + i for i in range(256)], expect=SolverResult.Sat)
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"]) == (1, 1), i
    assert c.s.debug_capacities()["assump_cap"] == 256
    c.solve([61 + i for i in range(257)], expect=SolverResult.Sat)
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"], i["last_cold_reason"]) == (1, 2, ColdReason.ASSUMP_CAP), i
    assert c.s.debug_capacities()["assump_cap"] == 257 + 256
    c.s.close()


def check_cold_for_pinned_share(checked_solver):
    """Clauses attached warm are never reduced away: they may take a quarter of the 64 slots, 16, and no more."""
    c = checked_solver(n_vars=60 + 40, caps=dict(learnt_cap=64))
    c.solve(expect=SolverResult.Sat)
    for k in range(16):
        c.add([61 + k, -(62 + k)])
    c.solve(expect=SolverResult.Sat)
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"], i["attached_clauses"]) == (1, 1, 16), i
    c.add([61 + 16, -(62 + 16), 3])
    c.solve([-61], expect=SolverResult.Sat)
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"], i["last_cold_reason"], i["attached_clauses"]) == (1, 2, ColdReason.PINNED_SHARE, 16), i
    c.add([-61, -62])
    c.solve([-61], expect=SolverResult.Sat)          # the cold start took the 17 in as original clauses: room again
    assert c.info()["warm_solves"] == 2
    c.s.close()


def check_cold_for_a_full_device(checked_solver):
    """A watch pool 16 entries above its lists, and twelve warm clauses that all watch one literal: its list moves from its
    slot of 2 to one of 8, and the slot of 16 it wants next does not exist.  The attach ends in MS_ST_ERR_POOL, which is
    no error of the solve: it starts cold (the clauses go in as original ones) and answers as the oracle does."""
    c = checked_solver(n_vars=60 + 40, caps=dict(pool_slack=16))
    c.solve(expect=SolverResult.Sat)
    for k in range(12):
        c.add([-61, 62 + k])
    c.solve([61, -70])
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"], i["last_cold_reason"]) == (0, 2, ColdReason.DEVICE_FULL), i
    assert c.log[-1][0] == SolverResult.Unsat and sorted(c.log[-1][1], key=abs) == [61, -70], c.log[-1]
    c.solve([61], expect=SolverResult.Sat)           # ... and the handle is warm again
    i = c.info()
    assert (i["warm_solves"], i["cold_solves"]) == (1, 2), i
    c.s.close()


PROOF_OPTS = dict(workers=3, slice_conflicts=100, deterministic=1, seed=7, simp=-1)
PROOF_CAP_TOO_SMALL = 8
# The longest slice of that run is 757 lemma words of one worker (found on the emulator by bisection: the smallest log
# without an overflow - a log fails a solve exactly when a slice's lemmas alone do not fit it); the next multiple of 64.
# The run's 226 deletion lines all fit from 1269 words on; at 768 most are left out.  (The GPU's run of the same case is not
# the emulator's to the conflict: its longest slice is 733 words, 48 of its 213 deletion lines fit at 768.)
PROOF_CAP_LEMMAS_ONLY = 768


def check_proof_log_drops_deletions(make_solver, tmp_path, solve=None, proof_cap=PROOF_CAP_LEMMAS_ONLY):
    """Seed 0 in the deterministic mode (the same run on the emulator and on the GPU) with a log of `proof_cap` words per
    worker: every lemma fits, not every deletion line does.  The proof is checked as every other one; that lines were
    left out shows against the same run with the default log of a million words."""
    full = check_proof_log(make_solver, 0, 1 << 20, tmp_path, False, solve=solve, **PROOF_OPTS)
    small = check_proof_log(make_solver, 0, proof_cap, tmp_path, False, solve=solve, **PROOF_OPTS)
    assert 0 < full and small < full, (small, full)


def checked(Checked, make_solver, n_vars, caps=None):
    """A test_incremental.Checked handle on easy_formula(), with the stores sized by caps."""
    s = make_solver()
    if caps:
        s.debug_set_capacities(**caps)
    return Checked(easy_formula()[0], s, n_vars=n_vars)
