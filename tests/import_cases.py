"""Records from another handle that collapse under the importer's own simplification (tests/test_emu_incremental_fuzz.py,
test_gpu_incremental_fuzz.py), and their judge (test infrastructure).

mi355sat_share_import sends a foreign record through device_literal, the mapping warm_begin uses for added clauses.  A
record that names both members of an equivalence class of the importer comes out of it with one device literal twice, or
with a literal and its negation, and the exporter cannot know: its own simplification "may have come out differently"
(include/mi355sat.h).  A clause in a worker's store holds every variable once: conflict analysis counts a variable that
two lanes of the wave present twice and walks off the trail, which ends the sweep in MS_ST_ERR_INTERNAL ("device solver
internal error") - on the MI355X, import-n100-s11 with simp = 2 does without the normalisation.  So mi355sat_share_import
normalises the mapped record as warm_begin does (sorted, repeats once, tautologies dropped and not counted).  Here such
records are imported into a running sweep, by hand and between two live handles of different simp levels, and the sweep is
judged by the oracle alone: its verdict, its model, every record of the ring - and no ring record names a variable twice,
the count share_import returns leaves the tautologies out, the record of 31 literals is taken with 31 distinct variables
and the record written as a unit arrives as one.

The formula is helpers.structured_cnf with equivalences of both polarities (x == y, u == ~v), level-0 facts and variables
that simp = 2 eliminates, over a 3-SAT base dense enough that the sweep is undecided after its first slice."""
import numpy as np

from helpers import Csr, assert_ring_records_are_implied, structured_cnf
from incremental_cases import binary_equivalences, mapped, oracle_on, substitution
from oracle import oracle as ora
from timberborn_support_solver_amd import SolverResult

MS_SHARE_MAXLEN = 31         # csrc/device/layout.h: the longest clause that is exchanged

# name -> (seed, n_vars, clauses of the 3-SAT base, oracle verdict, oracle conflicts)
IMPORT_CASES = {
    "import-n140-s20": (20, 140, 360, 10, 245),
    "import-n140-s18": (18, 140, 360, 10, 192),
    "import-n100-s5": (5, 100, 185, 20, 101),
    "import-n100-s11": (11, 100, 185, 20, 120),
}
# (import-n140-s20 is decided by a handle that simplifies before it has anything to pass on)
TWO_HANDLE_CASES = ("import-n140-s18", "import-n100-s5", "import-n100-s11")
FEATURES = ("equiv", "failed", "elim")
# three workers in the deterministic mode (a run is a function of its inputs on the emulator and on the GPU alike), slices of
# a few conflicts, every worker attaching everything at once, and learnt-clause reductions from the eighth conflict on
IMPORT_OPTS = dict(workers=3, slice_conflicts=4, share_interval=1, import_pct=100, deterministic=1, seed=7, reduce_first=8, reduce_inc=4)

_cache = {}


def formula(name):
    """(Csr, oracle verdict, special variables); the table's verdict and conflict count are asserted."""
    if name not in _cache:
        seed, n, m, verdict, conflicts = IMPORT_CASES[name]
        cl, special = structured_cnf(seed, n, m, (3,), features=FEATURES)
        cnf = Csr(cl, n)
        o = oracle_on(cl, n)
        want = o.solve()
        assert (want, o.stats()["conflicts"]) == (verdict, conflicts), (name, want, o.stats()["conflicts"])
        _cache[name] = (cnf, want, special)
    return _cache[name]


def collapsing_records(name, eliminated=None, alive=None, sub=None, facts=None):
    """[(what, literals)]: records the formula implies (the oracle proves each before use, as
    capacity_cases.check_imports_never_fail_a_solve does) that collapse under the substitution x == y, u == ~v and the level-0
    facts of a handle that simplifies: the equivalences are those of the binary implication graph, the facts the failed
    literals of the gadgets (unit propagation refutes their negation).  eliminated: a clause over a variable the importer
    resolved away; alive: the variables it did not (default: all) - every other record stays among these; sub, facts: the
    importer's substitution and its level-0 literals (default: the structure's own) - the record of 31 literals takes one
    variable per equivalence class, the unit record is made of facts the importer has and a literal it has not."""
    cnf, _, special = formula(name)
    rng = np.random.default_rng(500 + IMPORT_CASES[name][0])
    o = oracle_on(cnf.clauses, cnf.n_vars)
    lits, offs = ora.to_csr(cnf.clauses)
    gone = set(range(1, cnf.n_vars + 1)) - set(alive) if alive is not None else set()
    fixed = [l for v in special for l in (v, -v) if v not in gone and ora.bcp(lits, offs, cnf.n_vars, [-l])[0]]
    assert fixed, "no level-0 fact among the gadgets"
    fv = {abs(l) for l in fixed} | gone
    pairs = [(x, y) for x, y in binary_equivalences(cnf.clauses) if x not in fv and abs(y) not in fv]
    occurs = lambda l: [c for c in cnf.clauses if l in c and len(set(map(abs, c))) == len(c) >= 3 and not fv & set(map(abs, c))]
    recs = []
    for polarity, tag in ((1, "x == y"), (-1, "u == ~v")):
        # a clause with a literal s * x of the class: s * y says the same, so the clause with both is implied - one device literal twice
        p, q, c = next((p, q, occurs(p)[0]) for x, y in pairs if (y > 0) == (polarity > 0) for s in (1, -1)
                       for p, q in ((s * x, s * y), (s * y, s * x)) if occurs(p) and not any(abs(l) == abs(q) for l in occurs(p)[0]))
        recs.append((f"duplicate after mapping, {tag}", [p, q] + [l for l in c if l != p]))
        a = next(l for l in c if l != p)
        recs.append((f"tautology after mapping, {tag}", [p, -q, a]))         # (p | ~q) is half of the equivalence
    if facts is not None:        # the facts the importer found itself
        fixed = list({mapped(sub, l): l for l in fixed if mapped(sub, l) in facts}.values())      # (one per device literal)
        assert fixed, "the importer fixed none of the gadgets' failed literals at level 0"
    t = [int(l) for l in rng.permutation(fixed)]
    c = occurs(pairs[0][0])[0] if occurs(pairs[0][0]) else next(c for c in cnf.clauses if len(c) == 3 and not fv & set(map(abs, c)))
    recs.append(("the fixed literal true", [t[0]] + [l for l in c if abs(l) != abs(t[0])][:2]))
    recs.append(("the fixed literal false: shrinks", [-t[0]] + list(c)))
    # a literal every model has that neither unit propagation nor a failed literal gives away, where there is one
    hidden = [l for v in range(1, cnf.n_vars + 1) if v not in fv for l in (v, -v)
              if o.solve([-l]) == 20 and not ora.bcp(lits, offs, cnf.n_vars, [-l])[0]
              and (facts is None or (mapped(sub, l) not in facts and -mapped(sub, l) not in facts))]
    recs.append(("a unit after mapping and shrinking", list(dict.fromkeys([-t[0], -t[-1]])) + [hidden[0] if hidden else t[1 % len(t)]]))
    # padding: one variable per equivalence class (of the structure and of the importer), none of the clause's classes
    classes = {}
    for x, y in binary_equivalences(cnf.clauses):
        classes.setdefault(x, x)
        classes[abs(y)] = classes[x]
    rep_of = lambda v: (abs(mapped(sub or {}, v)), classes.get(v, v))
    used, used_cls, pad = {abs(l) for l in c}, set(), []
    for l in c:
        used_cls.update(rep_of(abs(l)))
    for v in rng.permutation(np.arange(1, cnf.n_vars + 1)):
        v = int(v)
        if v in used or v in fv or used_cls & set(rep_of(v)):
            continue
        used_cls.update(rep_of(v))
        pad.append(v if rng.random() < 0.5 else -v)
    recs.append((f"{MS_SHARE_MAXLEN} literals", list(c) + pad[:MS_SHARE_MAXLEN - len(c)]))
    recs.append(("one literal too long: refused", list(c) + pad[:MS_SHARE_MAXLEN + 1 - len(c)]))
    if eliminated is not None:
        recs.append(("over an eliminated variable: not attached", list(eliminated)))
    for what, rec in recs:
        assert o.solve([-l for l in rec]) == 20, ("the record does not follow from the formula", what, rec)
    return recs


def load(s, cnf):
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)


def run_to_the_end(s, cnf, want, step, res, nd):
    n_steps = 0
    while nd == 0:
        res, nd = step(s)             # (a SolverError - any MI355SAT_ERR_* - fails the test here)
        n_steps += 1
        assert n_steps < 2000, "the sweep does not end"
    assert res[0].value == want, (res, want)
    if res[0] == SolverResult.Sat:
        assert ora.check_model(cnf.lits, cnf.offsets, s.sweep_solution_of(0, cnf.n_vars)) == -1
    return res, n_steps


def check_collapsing_imports(make_solver, name, simp, step=None, **opts):
    """The hand-written records, imported after the first step of an undecided sweep of a handle that simplifies."""
    cnf, want, _ = formula(name)
    step = step or (lambda s: s.sweep_step())
    s = make_solver(**dict(IMPORT_OPTS, simp=simp, **opts))
    s.debug_keep_simplified()
    load(s, cnf)
    s.sweep_begin([[]])
    res, nd = step(s)
    assert nd == 0, "the formula was decided before the import: the case proves nothing"
    # the importer's own substitution and, with simp = 2, what it resolved away: read back from what the workers got
    kept, aside = s.debug_simplified()
    sub = substitution(kept)
    eliminated = alive = None
    if simp == 2:       # a clause kept for a variable that occurs nowhere in what the workers got
        left = {abs(l) for c in kept if not (len(c) == 2 and (abs(c[0]) in sub or abs(c[1]) in sub)) for l in c}
        alive = {v for v in range(1, cnf.n_vars + 1) if abs(mapped(sub, v)) in left}
        eliminated = next(c for c in aside if any(abs(l) not in left and abs(l) not in sub for l in c))
        assert s.stats()["simp_eliminated"] > 0
    facts = {c[0] for c in kept if len(c) == 1}
    recs = collapsing_records(name, eliminated, alive, sub, facts)
    # passed over and not counted: the record that is too long, the one over the eliminated variable and the two that hold a
    # literal and its negation in the importer's variables; every other record is taken
    taken = 0
    for what, rec in recs:
        m = [mapped(sub, l) for l in rec]
        taut = any(-l in m for l in m)
        assert taut == what.startswith("tautology"), (what, rec, m)
        assert (len(set(m)) < len(m)) == what.startswith("duplicate"), (what, rec, m)
        if what.endswith("31 literals"):
            assert len({abs(l) for l in m}) == len(rec) == MS_SHARE_MAXLEN, (what, m)
        if what.startswith("a unit"):       # every literal but one FALSE at level 0, that one free
            assert [l for l in m if -l not in facts] == [m[-1]] and m[-1] not in facts, (what, m)
        taken += not (taut or len(rec) > MS_SHARE_MAXLEN or what.startswith("over an eliminated"))
    assert taken == len(recs) - 3 - (eliminated is not None)
    words = np.asarray([w for _, rec in recs for w in [3] + rec + [0]], dtype=np.int32)
    assert s.share_import(words) == taken, [what for what, _ in recs]
    foreign = [c for c in s.debug_share_ring() if len({abs(l) for l in c}) < len(c)]
    assert not foreign, ("the ring holds a record with one variable twice: a clause in a worker's store may not", foreign)
    res, n_steps = run_to_the_end(s, cnf, want, step, res, nd)
    assert_ring_records_are_implied(s, cnf)
    ring = [tuple(sorted(c)) for c in s.debug_share_ring()]
    st = s.stats()
    s.sweep_end()
    print(name, "simp", simp, "verdict", res[0].name, "steps", n_steps, "conflicts", st["conflicts"], "imported", st["shared_imported"],
          "units", st["shared_imported_units"], "reduce_dbs", st["reduce_dbs"], "ring", len(ring))
    assert st["shared_imported"] > 0 and st["shared_imported_units"] > 0, st
    return s, st


def check_two_live_handles(make_solver, name, simp_b, step=None, **opts):
    """Handle A (simp = -1: no substitution, its records name every variable of the formula) and handle B (simp_b) sweep the
    same formula and pass their records to each other after every step, until both are decided."""
    cnf, want, _ = formula(name)
    step = step or (lambda s: s.sweep_step())
    handles = [make_solver(**dict(IMPORT_OPTS, simp=-1, **opts)), make_solver(**dict(IMPORT_OPTS, simp=simp_b, seed=11, **opts))]
    state = []
    for s in handles:
        load(s, cnf)
        s.sweep_begin([[]])
        state.append(([SolverResult.Interrupted], 0))
    passed = [0, 0]
    n_rounds = 0
    while any(nd == 0 for _, nd in state):
        for k, s in enumerate(handles):
            if state[k][1] == 0:
                state[k] = step(s)
        for k, s in enumerate(handles):
            buf, n = s.share_export()
            other = handles[1 - k]
            if n and state[1 - k][1] == 0:
                passed[1 - k] += other.share_import(buf)
        n_rounds += 1
        assert n_rounds < 2000, "the sweeps do not end"
    stats = []
    for k, s in enumerate(handles):
        res = state[k][0]
        assert res[0].value == want, (k, res, want)
        if res[0] == SolverResult.Sat:
            assert ora.check_model(cnf.lits, cnf.offsets, s.sweep_solution_of(0, cnf.n_vars)) == -1
        assert_ring_records_are_implied(s, cnf)
        twice = [c for c in s.debug_share_ring() if len({abs(l) for l in c}) < len(c)]
        assert not twice, ("the ring holds a record with one variable twice", k, twice)
        stats.append(s.stats())
        s.sweep_end()
    print(name, "simp", (-1, simp_b), "rounds", n_rounds, "records taken", passed, "conflicts", [st["conflicts"] for st in stats],
          "imported", [st["shared_imported"] for st in stats])
    assert min(passed) > 0 and all(st["shared_imported"] > 0 for st in stats), (passed, stats)
    return handles
