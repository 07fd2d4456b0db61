"""Formulas, assumption lists and seeded schedules for the differential tests of the stepwise sweep's schedule calls
(tests/test_emu_sweep_fuzz.py, test_gpu_sweep_fuzz.py), and their judge (test infrastructure).

What runs here is the scheduler between two slices - mi355sat_sweep_drop / _reopen / _set_weights / _sweep_model_of, behind
them rebalance_workers, schedule_cubes and ms_assign_kernel - on formulas that are not the Timberborn terrains and under
assumption lists that are not one totalizer output: workers swap lists of 0 .. 130 arbitrary literals and keep their learnt
clauses, which therefore have to follow from the formula alone.

The judge is the oracle alone, never the product.  After EVERY step:
  - a result that is not 0 is the oracle's verdict for that instance and never changes afterwards;
  - a withdrawn instance reports 0 for as long as it is withdrawn;
  - n_decided = instances with a verdict + withdrawn undecided ones;
  - the model of every instance that is SAT by now (mi355sat_sweep_model_of, mid-sweep) passes oracle.check_model against
    the clauses plus the instance's assumptions as units;
  - propagations == n_deq; no call raises (any MI355SAT_ERR_* is a SolverError and fails the test).
Every schedule ends with a final act - everything reopened, equal weights - after which the sweep has a bounded number of
slices (or a deadline) to decide EVERY instance: the oracle's verdict each, none left out.  After sweep_end the models are
checked again (solution_of) and, in fleets of two and more workers that made conflicts, every record of the exchange ring is
refuted by the oracle when negated (helpers.assert_ring_records_are_implied).

The tables were sized with the oracle and the emulator on the CPU: verdicts and conflicts are the oracle's (asserted by
formula() and lists()), UNSCHEDULED holds the slices the emulator needs for the same case and option set WITHOUT any schedule
call (asserted by the emulator tests: a changed generator cannot quietly change the set).  The liveness bound of a scheduled
run is 4 x that figure after the final act, at least 20: after a reopen one worker may carry an instance that the
unscheduled run gave fleet / instances workers, and seeds of one portfolio spread by about a factor of two."""
import time

import numpy as np

from fuzz_cases import EMU_CASES as FUZZ_CASES, formula as fuzz_formula
from helpers import Csr, assert_ring_records_are_implied, random_cnf, structured_cnf
from oracle import oracle as ora
from simp_cases import within
from timberborn_support_solver_amd import SolverResult

MIXED = (2, 3, 4, 5, 6)
ALL = ("equiv", "failed", "subsume", "strengthen", "elim", "salt")

# name -> (generator, seed, n_vars, n_clauses, lens, simp, oracle verdict, oracle conflicts, instances,
#          oracle verdict per instance, oracle conflicts per instance)
# 3-SAT at 4.26 clauses per variable in both verdicts (the first one is fuzz_cases' 3sat-n50-s5); "all-n110-s8" is
# simp_cases' formula with every planted feature, once with simp 0 and once with 2: the lists name substituted, fixed and
# eliminable variables; "long-n150" carries the lists of 63, 64, 65 and 130 literals (ms_assign_kernel copies a list with 64
# threads in a stride loop), cut from an oracle model with zero, one or a few literals flipped.
CASES = {
    "3sat-n50-s5": ("random", 5, 50, 213, (3,), -1, 10, 40, 8, (10, 10, 20, 20, 20, 20, 20, 10), (40, 11, 0, 14, 14, 5, 1, 3)),
    "3sat-n50-s17": ("random", 17, 50, 213, (3,), -1, 20, 42, 6, (20, 20, 20, 20, 20, 20), (42, 14, 0, 6, 6, 7)),
    "3sat-n80-s4": ("random", 4, 80, 341, (3,), -1, 10, 117, 6, (10, 20, 20, 10, 10, 20), (117, 21, 0, 38, 38, 50)),
    "all-n110-s8-simp0": ("structured", 8, 110, 170, MIXED, 0, 10, 25, 8, (10, 10, 20, 10, 10, 10, 20, 20), (25, 25, 0, 15, 15, 13, 12, 1)),
    "all-n110-s8-simp2": ("structured", 8, 110, 170, MIXED, 2, 10, 25, 8, (10, 10, 20, 10, 10, 10, 20, 20), (25, 25, 0, 15, 15, 13, 12, 1)),
    "long-n150-s20": ("random", 20, 150, 680, MIXED, -1, 10, 11, 10, (10, 10, 20, 10, 10, 10, 10, 20, 10, 20), (11, 9, 0, 2, 2, 2, 0, 0, 0, 0)),
}
FORMULA_UNSAT = "3sat-n50-s17"
LONG = "long-n150-s20"
LONG_LENS = (63, 64, 65, 130)
LONG_FLIPS = (0, 1, 1, 2)
FINDING = "3sat-n50-s5"
REPEATS = "3sat-n50-s5"             # its list 1 has more entries than the formula has variables (a worker has n_vars levels)
# the six builds and the second variable order run on these
MATRIX_CASES = ("3sat-n50-s5", LONG)

SEEDS = (1, 2, 3, 4, 5, 6)
N_SCHED_STEPS = 6                # a seeded schedule acts before the steps 0 .. 5, its final act comes before step 6
MIN_CAP = 20

_cache = {}


def oracle_for(cnf):
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(cnf.n_vars)
    return o


def formula(name):
    """(Csr, special variables) of a case, computed once; the oracle's verdict and conflict count are asserted."""
    key = ("formula", name)
    if key not in _cache:
        gen, seed, n, m, lens, _, verdict, conflicts = CASES[name][:8]
        if gen == "random":
            cl, special = random_cnf(seed, n, m, lens), []
        else:
            cl, special = structured_cnf(seed, n, m, lens, features=ALL)
        cnf = Csr(cl, n)
        o = oracle_for(cnf)
        want = o.solve()
        assert (want, o.stats()["conflicts"]) == (verdict, conflicts), (name, want, o.stats()["conflicts"])
        _cache[key] = (cnf, special)
    return _cache[key]


def make_lists(name):
    """The assumption lists of a case, seeded: [0] empty, [1] with a repeated literal (in REPEATS
    repeated until the list is longer than n_vars), [2] with a contradicting pair, [3] and
    [4] the same list, [5] a superset of it, the others random lists of 1 .. 6 literals over all variables (every other
    literal over the gadgets' variables where the formula has some); in the long case the last four are LONG_LENS literals
    of an oracle model in random order, with LONG_FLIPS of them flipped - in a list of more than 64 literals beyond the first
    64, so that the verdict rests on the part of the list that one pass of 64 threads does not copy."""
    cnf, special = formula(name)
    n_inst = CASES[name][8]
    rng = np.random.default_rng(9000 + CASES[name][1])

    def rand_list(k=None):
        a = []
        for _ in range(int(rng.integers(1, 7)) if k is None else k):
            v = int(rng.choice(special)) if special and rng.random() < 0.5 else int(rng.integers(cnf.n_vars)) + 1
            if v not in [abs(l) for l in a]:
                a.append(v if rng.random() < 0.5 else -v)
        return a

    lists = [[] for _ in range(n_inst)]
    for i in range(1, n_inst):
        lists[i] = rand_list()
    lists[1].insert(int(rng.integers(len(lists[1]) + 1)), lists[1][0])
    if name == REPEATS:                   # ... and the whole list over and over: four times as many entries as the formula has variables
        lists[1] = lists[1] * (4 * cnf.n_vars // len(lists[1]) + 1)
    pair = int(rng.choice(special)) if special else int(rng.integers(cnf.n_vars)) + 1
    lists[2] = [l for l in lists[2] if abs(l) != pair]
    lists[2].insert(int(rng.integers(len(lists[2]) + 1)), pair)
    lists[2].insert(int(rng.integers(len(lists[2]) + 1)), -pair)
    lists[4] = list(lists[3])
    lists[5] = list(lists[3]) + [l for l in rand_list(2) if abs(l) not in [abs(x) for x in lists[3]]]
    if name == LONG:
        o = oracle_for(cnf)
        assert o.solve() == 10
        model = o.model(cnf.n_vars)
        for j, (k, flips) in enumerate(zip(LONG_LENS, LONG_FLIPS)):
            vs = rng.permutation(cnf.n_vars)[:k]
            a = [int(v + 1) if model[v] > 0 else -int(v + 1) for v in vs]
            for f in rng.choice(np.arange(64 if k > 64 else 0, k), size=flips, replace=False):
                a[int(f)] = -a[int(f)]
            lists[n_inst - len(LONG_LENS) + j] = a
    return lists


def lists(name):
    """(assumption lists, oracle verdict per list) of a case, computed once; verdicts and conflicts are those of the table."""
    key = ("lists", name)
    if key not in _cache:
        cnf, _ = formula(name)
        ls = make_lists(name)
        verdicts, conflicts = [], []
        for a in ls:
            o = oracle_for(cnf)
            verdicts.append(o.solve(list(dict.fromkeys(a))))       # (each literal once: the oracle has one level per variable)
            conflicts.append(o.stats()["conflicts"])
        assert (tuple(verdicts), tuple(conflicts)) == CASES[name][9:11], (name, tuple(verdicts), tuple(conflicts))
        _cache[key] = (ls, verdicts)
    return _cache[key]


def verdict_mix(names):
    v = [r for n in names for r in lists(n)[1]]
    return v.count(10), v.count(20)


# ---- option sets ---------------------------------------------------------------------------------------------------------
# per case: a function of the number of instances n.  simp comes from the case; emulator runs add deterministic = 1.
OPTSETS = {
    "default": lambda n: dict(workers=2 * n),
    "no-rebalance": lambda n: dict(workers=n, rebalance=-1),
    "cube-split": lambda n: dict(workers=2 * n, cube_split=1),
    "liberal-exchange": lambda n: dict(workers=n, share_interval=1, import_pct=100, share_lbd=31),
    "lds": lambda n: dict(workers=n, lds_val=1),
    "slab": lambda n: dict(workers=n, lds_val=-1),
}
VAR_ORDER_CASE = "all-n110-s8-simp0"      # var_order = 1 on this one, in the default option set


def options(name, optset, **more):
    n = CASES[name][8]
    return dict(OPTSETS[optset](n), simp=CASES[name][5], slice_conflicts=10, **more)


# ---- schedules -------------------------------------------------------------------------------------------------------------
# A schedule is a list of (step, action, argument): the action is made BEFORE that step.  Actions:
#   drop / reopen (a list of instances, possibly empty), weights (a vector), drop_decided / reopen_open (the header's no-ops:
#   the judge picks an instance that has a verdict / that was never withdrawn), models (sweep_solution_of on every SAT one).
ACTIONS = ("drop", "drop_all_but_one", "drop_last", "reopen", "weights_some_zero", "weights_all_zero", "weights_one_50x",
           "weights_twice", "drop_decided", "reopen_open", "empty_lists", "models")


def seeded_schedule(seed, n):
    """Schedule `seed` for n instances: every action of ACTIONS once, in a seeded order, two before each of the steps
    0 .. N_SCHED_STEPS - 1 (what "drop all but one" and "drop everything" bring along comes one and two steps later)."""
    rng = np.random.default_rng(100 * n + seed)
    sched = []
    for slot, k in enumerate(rng.permutation(len(ACTIONS))):
        step, kind = slot // 2, ACTIONS[k]
        some = sorted(int(i) for i in rng.choice(n, size=int(rng.integers(1, n // 2 + 1)), replace=False))
        if kind == "drop":
            sched.append((step, "drop", some))
        elif kind == "drop_all_but_one":
            keep = int(rng.integers(n))
            sched.append((step, "drop", [i for i in range(n) if i != keep]))
            sched.append((step + 1, "drop", [keep]))                       # ... and then the last one
            sched.append((step + 2, "reopen", some))
        elif kind == "drop_last":
            sched.append((step, "drop", list(range(n))))                   # everything at once
            sched.append((step + 1, "reopen", some))
        elif kind == "reopen":
            sched.append((step, "reopen", some))
        elif kind == "weights_some_zero":
            sched.append((step, "weights", [0.0 if rng.random() < 0.4 else float(rng.integers(1, 5)) for _ in range(n)]))
        elif kind == "weights_all_zero":
            sched.append((step, "weights", [0.0] * n))
        elif kind == "weights_one_50x":
            big = int(rng.integers(n))
            sched.append((step, "weights", [50.0 if i == big else 1.0 for i in range(n)]))
        elif kind == "weights_twice":
            w = [float(rng.integers(1, 4)) for _ in range(n)]
            sched += [(step, "weights", w), (step, "weights", list(w))]
        elif kind == "empty_lists":
            sched += [(step, "drop", []), (step, "reopen", [])]
        else:
            sched.append((step, kind, None))
    sched.sort(key=lambda a: a[0])              # (stable: the actions of one step keep their order)
    return sched


def final_step(sched):
    return 1 + max([a[0] for a in sched], default=-1)


# The two scripts of the stalls the suite was written after, verbatim: (option set, schedule).
STALL_SCRIPTS = {
    "parked-worker-of-a-reopened-instance": ("no-rebalance", [(0, "drop", [1]), (2, "reopen", [1])]),
    "cube-closed-while-withdrawn": ("cube-split", [(0, "drop", [1, 3]), (6, "reopen", [1, 3])]),
}


def long_to_empty_and_back(name):
    """The long case: every worker goes to the empty list before the first slice, then all of them to the list of 130
    literals - also the workers that held the lists of 63, 64 and 65 - and back to the empty one."""
    n = CASES[name][8]
    return [(0, "drop", list(range(1, n))), (1, "reopen", [n - 1]), (1, "drop", [0]), (2, "reopen", [0]), (2, "drop", [n - 1])]


# name -> option set -> slices of the emulator's unscheduled run (deterministic = 1) to the last verdict
UNSCHEDULED = {
    "3sat-n50-s5": {"default": 2, "no-rebalance": 4, "cube-split": 3, "liberal-exchange": 3, "lds": 4, "slab": 3},
    "3sat-n50-s17": {"default": 5, "no-rebalance": 7, "cube-split": 5, "liberal-exchange": 5, "lds": 5, "slab": 6},
    "3sat-n80-s4": {"default": 5, "no-rebalance": 7, "cube-split": 5, "liberal-exchange": 6, "lds": 7, "slab": 6},
    "all-n110-s8-simp0": {"default": 1, "no-rebalance": 2, "cube-split": 2, "liberal-exchange": 2, "lds": 2, "slab": 1},
    "all-n110-s8-simp2": {"default": 1, "no-rebalance": 1, "cube-split": 1, "liberal-exchange": 1, "lds": 1, "slab": 1},
    "long-n150-s20": {"default": 1, "no-rebalance": 1, "cube-split": 1, "liberal-exchange": 1, "lds": 1, "slab": 1},
}


def slice_cap(name, optset):
    return max(MIN_CAP, 4 * UNSCHEDULED[name][optset])


# ---- the judge -------------------------------------------------------------------------------------------------------------
def judge(make_solver, name, opts, sched, cap=None, limit_s=None):
    """One sweep of the case under `opts`, driven by `sched` and judged as the module's docstring says.  cap: slices allowed
    after the final act (None: until the deadline); limit_s puts the whole sweep under a wall-clock limit (within(): the
    interrupt ends a step that hangs, the instances it leaves undecided fail the comparison with the oracle).  Returns
    (slices after the final act, slices in all, stats)."""
    s = make_solver(**opts)
    try:
        if limit_s:
            return within(limit_s, s, lambda: drive(s, name, sched, cap, time.monotonic() + limit_s))
        return drive(s, name, sched, cap, None)
    finally:
        s.close()


def drive(s, name, sched, cap, deadline):
    cnf, _ = formula(name)
    ls, want = lists(name)
    n = len(ls)
    units = [ora.to_csr(cnf.clauses + [[l] for l in a]) for a in ls]
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    s.sweep_begin(ls)                                  # (a SolverError - any MI355SAT_ERR_* - fails the test, here and below)
    withdrawn, ever_withdrawn, verdict = set(), set(), [0] * n
    final = final_step(sched)
    sched = list(sched) + [(final, "reopen", list(range(n))), (final, "weights", [1.0] * n)]
    step = after = 0
    while True:
        for _, kind, arg in [a for a in sched if a[0] == step]:
            if kind == "drop_decided":
                kind, arg = "drop", [i for i in range(n) if verdict[i]][:1]
            elif kind == "reopen_open":
                kind, arg = "reopen", [i for i in range(n) if i not in ever_withdrawn][:1]
            if kind == "drop":
                s.sweep_drop(arg)
                new = {i for i in arg if not verdict[i]}
                withdrawn |= new
                ever_withdrawn |= new
            elif kind == "reopen":
                s.sweep_reopen(arg)
                withdrawn -= set(arg)
            elif kind == "weights":
                s.sweep_set_weights(arg)
            elif kind == "models":
                for i in range(n):
                    if verdict[i] == 10:
                        assert ora.check_model(*units[i], s.sweep_solution_of(i, cnf.n_vars)) == -1, (step, i, ls[i])
        res, n_decided = s.sweep_step()
        for i in range(n):
            got = res[i].value
            if i in withdrawn:
                assert got == 0, ("a withdrawn instance reports a verdict", step, i, got)
                continue
            assert got == verdict[i] or (verdict[i] == 0 and got == want[i]), (step, i, ls[i], got, verdict[i], want[i])
            if got == 10 and not verdict[i]:
                assert ora.check_model(*units[i], s.sweep_solution_of(i, cnf.n_vars)) == -1, (step, i, ls[i])
            verdict[i] = got
        assert n_decided == sum(1 for v in verdict if v) + len(withdrawn), (step, n_decided, verdict, withdrawn)
        st = s.stats()
        assert st["propagations"] == st["n_deq"]
        step += 1
        if step > final:
            after += 1
            if all(verdict) or (cap is not None and after >= cap) or (deadline and time.monotonic() > deadline):
                break
    assert verdict == want, ("undecided after the final act", after, cap, verdict, want)
    for i in range(n):                                   # once more what was checked as it fell: the winners kept their slabs
        if verdict[i] == 10:
            assert ora.check_model(*units[i], s.sweep_solution_of(i, cnf.n_vars)) == -1, ("at the end", i, ls[i])
    s.sweep_end()
    for i in range(n):
        if verdict[i] == 10:
            assert ora.check_model(*units[i], s.solution_of(i, cnf.n_vars)) == -1, ("after sweep_end", i, ls[i])
    st = s.stats()
    assert st["propagations"] == st["n_deq"]
    if st["workers"] >= 2 and st["conflicts"]:
        assert_ring_records_are_implied(s, cnf)
    return after, step, st


def stop_at_first(make_solver, run=lambda s, fn: fn()):
    """solve_batch(stop_at_first = 1) on a fuzz formula under the lists of FINDING (the same formula): one verdict at least,
    every verdict the oracle's, models that check; the handle then answers a plain solve()."""
    cnf, want = fuzz_formula(FUZZ_CASES[FINDING])
    ls, verdicts = lists(FINDING)
    s = make_solver(workers=2 * len(ls), simp=-1, slice_conflicts=10)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    res = run(s, lambda: s.solve_batch(ls, stop_at_first=True))
    assert any(r.value for r in res), res
    for i, r in enumerate(res):
        assert r.value in (0, verdicts[i]), (i, ls[i], r, verdicts[i])
        if r == SolverResult.Sat:
            assert ora.check_model(*ora.to_csr(cnf.clauses + [[l] for l in ls[i]]), s.solution_of(i, cnf.n_vars)) == -1, (i, ls[i])
    r = run(s, s.solve)
    assert r.value == want
    assert ora.check_model(cnf.lits, cnf.offsets, s.full_solution(cnf.n_vars)) == -1
    s.close()
    return res
