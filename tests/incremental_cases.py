"""Seeded sequences for the differential tests of the warm incremental solve (tests/test_emu_incremental_fuzz.py,
test_gpu_incremental_fuzz.py), and their judge (test infrastructure).

tests/test_incremental.py runs one hand-written sequence whose added clauses are made of fresh variables; here a seeded
generator adds the clauses that mi355sat_set_incremental has the most ways to get wrong - warm_begin's mapping through the
equivalent-literal substitution (device_literal), its sorting / deduplication / tautology test, ms_attach_kernel's rounds of
64 literals under the level-0 assignment, ms_assign_kernel and ms_final_kernel on workers that a model, a refuted assumption
set, an interrupt or an exhausted conflict budget left where they stood - and interleaves the handle's other entry points
between the warm solves (go_cold: "a missed call is a wrong warm start").

A case is a table row: seed, base formula, simp, workers, solver options, the menu of clause classes, the calls in between,
how the sequence ends, the number of solves and the oracle's verdict string - one letter per solve, S = SAT, U = UNSAT under
the assumptions (the formula alone has a model: the core is not empty), E = the accumulated formula itself is UNSAT (the empty
core).  sequence() asserts the string, so that a changed generator cannot quietly change the set.

The judge is the oracle alone, never the product: tests/test_incremental.py's Checked compares every verdict with the oracle's
CDCL on the ACCUMULATED formula plus the call's assumptions, clause-checks every model against everything added so far and
against the assumptions, and checks every core (a subsequence of the assumptions as given, refuted by the oracle, equal to
what failed() says).  On top of it run_sequence() keeps a model of what include/mi355sat.h documents about the warm state and
asserts warm_solves, cold_solves, last_cold_reason, attached_clauses and attached_units after every solve:
  - a solve is cold when it is the first, when a proof path is set, or when solve_batch / sweep_* / propagate_batch /
    check_proof / a minimize_core that launched candidates ran in between (MI355SAT_COLD_OTHER_SEARCH); after
    set_incremental(off, on), debug_set_schedule and a proof-logging solve nothing is resident (MI355SAT_COLD_FIRST);
    set_phases and an interrupt leave the handle warm; every other solve is warm;
  - with simp = 2 a solve that names a variable outside the ones known to be kept (those without an occurrence at the last
    cold start, and that solve's assumptions, which freeze) may also start cold with MI355SAT_COLD_ELIMINATED;
  - a warm solve hands every clause added since the solve before to the workers: mapped through the substitution the last
    cold start made (read back through mi355sat_debug_simplified), repeated literals dropped, a clause with a literal and
    its negation not counted at all, a clause of one mapped literal counted in attached_units, any other in
    attached_clauses;
  - a refuted handle answers UNSAT with the empty core and counts the call as warm.
The reserved variables and the few dozen added clauses stay far below a quarter of the default stores, so
MI355SAT_COLD_PINNED_SHARE and MI355SAT_COLD_DEVICE_FULL are never expected.  The header states each of these rules: the list
under mi355sat_set_incremental, and the paragraphs of mi355sat_minimize_core (when it launches nothing) and
mi355sat_check_proof / _trim_proof.
The sequences of 258 workers follow tests/test_incremental.py's recipe for workers created after an attach; that the fleet
grew during a warm solve and got a second attach is asserted on the emulator only (grows = True) - on the GPU the ramp-up
goes by kernel time and these formulas are decided long before it adds a worker.

The table was sized with the oracle on the CPU (the verdict strings) and the conflict budgets with the emulator."""
import collections

import numpy as np

import fuzz_cases
from helpers import Csr, assert_ring_records_are_implied, structured_cnf
from oracle import oracle as ora
from simp_cases import is_subsequence, within
from test_incremental import Checked
from timberborn_support_solver_amd import ColdReason, SolverResult

N_FALSE = 100      # reserved variables the sequences with long clauses fix FALSE by units (the "unit_block")
N_FRESH = 240      # variables above the base formula's, reserved before the first solve

# the classes of added clauses: every one occurs somewhere in the table
CLASSES = ("equiv_dup", "equiv_taut", "dup_lit", "taut", "fixed_sat", "fixed_binary", "fixed_unit", "fixed_empty",
           "contradict_learnt", "model_false", "model_true", "len1", "len2", "len3", "len63", "len64", "len65", "len130",
           "long_one_free", "long_two_free", "elim_var", "elim_kept")
BETWEEN = ("minimize_core", "propagate_batch", "solve_batch", "sweep", "check_proof", "set_phases", "proof_path",
           "set_schedule", "toggle_incremental", "interrupt")
A_KINDS = ("empty", "repeat", "contra")
LENGTHS = {"len1": 1, "len2": 2, "len3": 3, "len63": 63, "len64": 64, "len65": 65, "len130": 130}

Case = collections.namedtuple("Case", "seed base simp workers opts menu between end n_solves verdicts")

SHORT = ("dup_lit", "taut", "model_false", "model_true", "len1", "len2", "len3")
SUBST = ("equiv_dup", "equiv_taut", "equiv_dup", "equiv_taut")
FIXED = ("fixed_sat", "fixed_binary", "fixed_unit")
ROUNDS = ("len63", "len64", "len65", "len130")
LONG = ROUNDS + ("long_one_free", "long_two_free")
STRUCT = ("equiv", "failed", "subsume", "strengthen", "salt")
BUDGET = dict(deterministic=1, slice_conflicts=10, seed=3)

# base: ("structured", n_vars, clauses of the 3-SAT base, features) - helpers.structured_cnf over a base of 2.9 clauses per
# base variable - or ("random", name): a near-threshold 3-SAT formula of fuzz_cases.GPU_CASES.
# opts: options of mi355sat_new, plus p_model (how often an assumption literal follows a model of the accumulated formula)
# and n_fresh (variables reserved above the base formula's, where N_FRESH would only cost time).
CASES = {
    "subst-s0-n90": Case(11, ("structured", 90, 139, STRUCT), 0, 2, {}, SUBST + FIXED + SHORT,
                         ("propagate_batch", "set_phases", "minimize_core"), None, 12, "SSSUSUUUUSSS"),
    "subst-s1-n90": Case(12, ("structured", 90, 139, STRUCT), 1, 2, {}, SUBST + FIXED + SHORT,
                         ("sweep", "interrupt", "toggle_incremental"), "fixed_empty", 12, "SUSUUSSUUUEE"),
    "rounds-s0-n80": Case(13, ("structured", 80, 110, STRUCT), 0, 1, {}, LONG + SUBST + ("len1", "len3"),
                          ("solve_batch", "set_schedule"), None, 12, "SSSSSSUSUSSS"),
    "rounds-sm1-n60": Case(14, ("structured", 60, 52, STRUCT), -1, 2, {}, LONG + SUBST + SHORT,
                           ("check_proof", "proof_path", "minimize_core"), "contradict", 12, "SUUSSSSSSUEE"),
    "rounds-s1-n80": Case(15, ("structured", 80, 110, STRUCT), 1, 2, dict(var_order=1), LONG + FIXED + SUBST,
                          ("propagate_batch", "interrupt"), None, 10, "SSSSUSUUUS"),
    "elim-s2-n100": Case(25, ("structured", 100, 107, STRUCT + ("elim",)), 2, 2, {},
                         ("elim_kept", "elim_kept", "elim_var", "elim_var") + SUBST + FIXED + SHORT,
                         ("set_phases", "sweep", "minimize_core"), None, 12, "SSSSSSSSUSUU"),
    "elim-s2-n110": Case(17, ("structured", 110, 136, STRUCT + ("elim",)), 2, 1, {},
                         ("elim_kept", "elim_var", "elim_kept", "elim_var") + SUBST + ROUNDS + SHORT,
                         ("solve_batch", "toggle_incremental", "check_proof"), "fixed_empty", 12, "SSSSSSUUSUEE"),
    "plain-sm1-n70": Case(18, ("structured", 70, 81, STRUCT), -1, 2, {}, SHORT + SUBST + FIXED + ("len63", "len65"),
                          ("set_schedule", "proof_path", "propagate_batch", "minimize_core"), None, 12, "SSSUUUUSSSSU"),
    "ramp-sm1-n60": Case(30, ("structured", 60, 52, STRUCT), -1, 258, dict(ramp=0, slice_conflicts=1, n_fresh=24), SUBST + SHORT,
                         (), "contradict", 4, "SUEE"),
    "budget-n120-s6": Case(20, ("random", "3sat-n120-s6"), -1, 1, dict(BUDGET, conflict_budget=160, p_model=0.9),
                          SHORT + ("len64", "long_one_free"), (), "contradict", 14, "SSUSSUUSSUUUEE"),
    "budget-n70-s5": Case(21, ("random", "3sat-n70-s5"), -1, 2, dict(BUDGET, conflict_budget=50, p_model=0.9),
                          SHORT + ("len65", "long_two_free"), ("set_phases",), None, 14, "SSSSUSSUSSSSUU"),
    "budget-n80-s4": Case(22, ("random", "3sat-n80-s4"), 0, 2, dict(BUDGET, conflict_budget=25, p_model=0.9),
                          SHORT + ("len63",), (), None, 12, "SSSSSUSSUSSS"),
}
# the six builds of the search kernel run on these (as simp_cases.MATRIX_CASES): the substitution, the attach kernel's
# rounds, the elimination and a budget sequence
MATRIX_CASES = ("subst-s0-n90", "rounds-sm1-n60", "elim-s2-n100", "budget-n120-s6")
# larger bases, for the GPU only: up to 300 variables, 25 solves, fleets of 1, 8 and 258 workers
ALL_MENU = SUBST + FIXED + SHORT + LONG
GPU_ONLY_CASES = {
    "gpu-3sat-n110-w8": Case(31, ("random", "3sat-n110-s2"), 0, 8, {}, SHORT + LONG,
                             ("propagate_batch", "solve_batch", "sweep", "minimize_core", "set_phases", "interrupt"), "contradict", 25, "SSUSSSSSUSSUSSUSUSSUUUUEE"),
    "gpu-struct-n300-w8": Case(32, ("structured", 300, 748, STRUCT), 0, 8, {}, ALL_MENU + ALL_MENU,
                               ("check_proof", "proof_path", "set_schedule", "toggle_incremental", "minimize_core", "sweep"), "fixed_empty", 25, "SUSSSSSUSUSUSUUSUSUUSSSEE"),
    "gpu-elim-n300-w1": Case(33, ("structured", 300, 687, STRUCT + ("elim",)), 2, 1, {},
                             ("elim_kept", "elim_kept", "elim_var", "elim_var") + ALL_MENU,
                             ("solve_batch", "set_phases", "propagate_batch", "minimize_core"), None, 20, "SSSSSSSSSSSSUSUUSUUU"),
    "gpu-ramp-n300-w258": Case(34, ("structured", 300, 748, STRUCT), 1, 258, {}, ALL_MENU,
                               ("interrupt", "toggle_incremental", "minimize_core"), None, 12, "SSSSUUSSSSSS"),
    "gpu-budget-n110-w8": Case(35, ("random", "3sat-n110-s2"), -1, 8, dict(BUDGET, conflict_budget=160, p_model=0.9),
                               SHORT + ROUNDS, ("set_phases",), None, 16, "SSSSSUSSSSSSUUSS"),
}
GPU_CASES = dict(CASES, **GPU_ONLY_CASES)

_cache = {}


def base_formula(case):
    """(Csr, special variables) of a case's base formula, computed once."""
    key = ("base", case.seed, case.base)
    if key not in _cache:
        if case.base[0] == "structured":
            _, n, m, features = case.base
            cl, special = structured_cnf(case.seed, n, m, (3,), features=features)
            _cache[key] = (Csr(cl, n), special)
        else:
            _cache[key] = (fuzz_cases.formula(fuzz_cases.GPU_CASES[case.base[1]])[0], [])
    return _cache[key]


def oracle_on(clauses, n_vars):
    o = ora.OracleSolver()
    o.add_cnf(*ora.to_csr(clauses))
    o.reserve(n_vars)
    return o


def binary_equivalences(clauses):
    """Pairs (x, y): variable x and literal y of a higher variable that binary clauses alone make equivalent (both lie on
    one cycle of the implication graph) - what els_scc substitutes.  Literals that imply their own negation are left out."""
    adj = collections.defaultdict(set)
    for c in clauses:
        c = sorted(set(c))
        if len(c) == 2 and c[0] != -c[1]:
            adj[-c[0]].add(c[1])
            adj[-c[1]].add(c[0])

    def reach(l):
        seen, todo = set(), [l]
        while todo:
            for m in adj.get(todo.pop(), ()):
                if m not in seen:
                    seen.add(m)
                    todo.append(m)
        return seen

    R = {l: reach(l) for l in list(adj)}
    return [(l, m) for l in sorted(R) if l > 0 and -l not in R[l] and l not in R.get(-l, ())
            for m in sorted(R[l]) if abs(m) > l and l in R.get(m, ())]


class _Generator:
    def __init__(self, case):
        self.case = case
        self.rng = np.random.default_rng(77000 + case.seed)
        self.cnf, self.special = base_formula(case)
        self.nb = nb = self.cnf.n_vars
        n_fresh = case.opts.get("n_fresh", N_FRESH)      # (fewer: no unit block, no long clauses)
        n_false = N_FALSE if n_fresh == N_FRESH else 0
        self.false_pool = list(range(nb + 1, nb + 1 + n_false))
        self.free_pool = list(range(nb + 1 + n_false, nb + 1 + n_fresh))
        self.n_vars = nb + n_fresh
        self.acc = []
        self.classes, self.calls, self.kinds = collections.Counter(), collections.Counter(), collections.Counter()
        o = self.oracle()
        assert o.solve() == 10, "the base formula of a sequence has a model"
        self.fixed = [l for v in self.special for l in (v, -v) if o.solve([-l]) == 20]      # backbone literals of the gadgets
        fv = {abs(l) for l in self.fixed}
        self.pairs = [(x, y) for x, y in binary_equivalences(self.cnf.clauses) if x not in fv and abs(y) not in fv]
        features = case.base[3] if case.base[0] == "structured" else ()
        self.elim = self.special[-13:-9] if "elim" in features else []      # structured_cnf: 1..3 occurrences per polarity
        self.kept = [int(v) for v in self.rng.choice(nb - len(self.special), size=4, replace=False) + 1] if case.simp == 2 else []
        self.unused = list(self.free_pool[120:])         # reserved variables no clause has named so far
        self.block_done = False
        self.targets = []                                # literals that added clauses force
        self.last = None                                 # (assumptions, verdict letter) of the last solve

    # ---- helpers
    def oracle(self, extra=()):
        return oracle_on(self.cnf.clauses + self.acc + list(extra), self.n_vars)

    def sign(self, v):
        return int(v) if self.rng.random() < 0.5 else -int(v)

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def mixed(self, k, avoid=()):
        """k literals over distinct variables, half of them reserved ones, half from the base formula."""
        free = [v for v in self.free_pool[:60 if k <= 40 else 120] if v not in avoid]
        base = [v for v in range(1, self.nb + 1) if v not in avoid]
        n_free = max(min(k // 2 + int(self.rng.integers(0, 2)), len(free), k), k - len(base))
        vs = list(self.rng.choice(free, size=n_free, replace=False)) + list(self.rng.choice(base, size=k - n_free, replace=False))
        return [self.sign(vs[i]) for i in self.rng.permutation(k)]

    def shuffled(self, c):
        return [int(c[i]) for i in self.rng.permutation(len(c))]

    def unit_block(self):
        self.block_done = True
        return [("unit_block", [-f]) for f in self.false_pool]

    # ---- one clause of a class: (clauses, forced literal or None), or None where the class has nothing to offer now
    def candidate(self, cls):
        r = self.rng
        if cls in ("equiv_dup", "equiv_taut"):
            if not self.pairs:
                return None
            x, y = self.pick(self.pairs)
            s = 1 if r.random() < 0.5 else -1
            tail = self.mixed(int(r.integers(0, 3)), avoid=(x, abs(y)))
            if cls == "equiv_taut" and not tail:
                tail = self.mixed(1, avoid=(x, abs(y)))
            return [self.shuffled([s * x, (s if cls == "equiv_dup" else -s) * y] + tail)], None
        if cls == "dup_lit":
            c = self.mixed(int(r.integers(2, 4)))
            c.insert(int(r.integers(len(c) + 1)), self.pick(c))
            return [c], None
        if cls == "taut":
            c = self.mixed(int(r.integers(1, 4)))
            c.insert(int(r.integers(len(c) + 1)), -self.pick(c))
            return [c], None
        if cls.startswith("fixed"):
            if not self.fixed:
                return None
            t = [int(l) for l in r.permutation(self.fixed)[:int(r.integers(1, 3))]]
            av = [abs(l) for l in t]
            if cls == "fixed_sat":
                return [self.shuffled([t[0]] + self.mixed(2, avoid=av))], None
            if cls == "fixed_binary":
                return [self.shuffled([-l for l in t] + self.mixed(2, avoid=av))], None
            if cls == "fixed_unit":
                a = self.mixed(1, avoid=av)
                return [self.shuffled([-l for l in t] + a)], a[0]
            return [[-l for l in t]], None                                   # fixed_empty
        if cls in ("model_false", "model_true"):
            if not self.last or self.last[1] != "S" or not self.last[0]:
                return None
            a = list(dict.fromkeys(self.last[0]))
            if cls == "model_true":
                return [self.shuffled([self.pick(a)] + self.mixed(2, avoid=[abs(l) for l in a]))], None
            k = min(len(a), int(r.integers(1, 3)))
            return [[-int(l) for l in r.permutation(a)[:k]]], None           # every model of the last solve falsifies it
        if cls in LENGTHS:
            n = LENGTHS[cls]
            if n <= 3:
                c = self.mixed(n)
                return [c], (c[0] if n == 1 else None)
            pre = []
            if self.case.menu.count("long_one_free") + self.case.menu.count("long_two_free") and not self.block_done:
                pre = self.unit_block()
            if self.block_done:      # most literals FALSE at level 0, the live ones wherever the sort puts them
                n_false = min(n - int(r.integers(1, 4)), N_FALSE)
                c = [int(f) for f in r.permutation(self.false_pool)[:n_false]] + self.mixed(n - n_false)
            else:
                c = self.mixed(n)
            return pre + [self.shuffled(c)], None
        if cls in ("long_one_free", "long_two_free"):
            pre = [] if self.block_done else self.unit_block()
            n = int(self.pick((70, 85, 100)))
            g = self.sign(self.pick(self.free_pool[:60]))                     # (above every variable of the block)
            c = [int(f) for f in r.permutation(self.false_pool)[:n - 1]] + [g]
            if cls == "long_two_free":
                c.append(self.sign(int(r.integers(self.nb)) + 1))             # (below every variable of the block)
                return pre + [self.shuffled(c)], None
            return pre + [self.shuffled(c)], g
        if cls == "elim_var":
            if not self.elim:
                return None
            return [self.shuffled([self.sign(self.pick(self.elim))] + self.mixed(2, avoid=self.elim))], None
        if cls == "elim_kept":
            if not self.kept or len(self.unused) < 2:
                return None
            vs = [self.pick(self.kept), self.unused.pop(), self.unused.pop()] + ([self.pick(self.kept)] if r.random() < 0.5 else [])
            return [self.shuffled([self.sign(v) for v in dict.fromkeys(vs)])], None
        raise ValueError(cls)

    def emit(self, cls):
        """[(class, literals)] of a clause of the class that leaves the accumulated formula satisfiable (fixed_empty and
        contradict_learnt are the two that refute it, at the end of a sequence), or None."""
        for _ in range(8):
            state = (self.block_done, list(self.unused))
            cand = self.candidate(cls)
            if cand is None:
                return None
            clauses, forced = cand
            plain = [c if isinstance(c, list) else c[1] for c in clauses]
            if cls == "fixed_empty" or self.oracle(plain).solve() == 10:
                if forced is not None:
                    self.targets.append(forced)
                self.acc += plain
                self.classes[cls] += 1
                return [c if isinstance(c, tuple) else (cls, c) for c in clauses]
            self.block_done, self.unused = state
        return None

    def assumptions(self, kind):
        r = self.rng
        if kind == "empty":
            return []
        o = self.oracle()
        model = o.model(self.n_vars) if o.solve() == 10 else None
        if kind == "kept":       # (simp = 2) the first solve freezes these
            return [int(v) * int(model[v - 1]) for v in self.kept]
        p_model = self.case.opts.get("p_model", 0.8)
        a = []
        for _ in range(int(r.integers(1, 7))):
            u = r.random()
            if self.targets and u < 0.12:
                a.append(-self.pick(self.targets))
                continue
            if self.special and u < 0.5:
                v = int(self.pick(self.special))
            elif u < 0.62:
                v = int(self.pick(self.free_pool[:60]))
            else:
                v = int(r.integers(self.nb)) + 1
            follow = model is not None and model[v - 1] != 0 and r.random() < p_model
            a.append(v * int(model[v - 1]) if follow else self.sign(v))
        if kind == "repeat":
            a.insert(int(r.integers(len(a) + 1)), a[0])
        elif kind == "contra":
            v = int(self.pick(self.special)) if self.special else int(r.integers(self.nb)) + 1
            a = [l for l in a if abs(l) != v]
            a.insert(int(r.integers(len(a) + 1)), v)
            a.insert(int(r.integers(len(a) + 1)), -v)
        return a

    def hidden_backbone_literal(self):
        """A literal every model of the accumulated formula has, that unit propagation alone does not find: a worker learns
        it as a level-0 fact when it refutes its negation."""
        o = self.oracle()
        lits, offs = ora.to_csr(self.cnf.clauses + self.acc)
        _, vals, _, _ = ora.bcp(lits, offs, self.n_vars, [])
        for v in self.rng.permutation(self.nb):
            v = int(v) + 1
            if vals[v - 1] == 0:
                for l in (v, -v):
                    if o.solve([-l]) == 20:
                        return l
        raise AssertionError("no backbone literal beyond unit propagation: the case cannot end in 'contradict'")

    def between_payload(self, name):
        r = self.rng
        rand_sets = lambda n, hi: [[self.sign(int(r.integers(self.nb)) + 1) for _ in range(int(r.integers(1, hi)))] for _ in range(n)]
        if name == "propagate_batch":
            return rand_sets(3, 4)
        if name == "solve_batch":
            return [self.assumptions("rand") for _ in range(3)]
        if name == "sweep":
            return [self.assumptions("rand") for _ in range(2)]
        if name == "set_phases":
            return [int(x) for x in r.integers(-1, 2, size=self.n_vars)]
        if name == "set_schedule":
            return (int(r.integers(20, 80)), int(r.integers(10, 40)), int(r.integers(30, 90)))
        if name == "check_proof":
            # The accumulated formula is satisfiable wherever a call stands in between, so no cold handle has a refutation of
            # it to log: the proof is made by hand - two lemmas and a target that are supersets of clauses (RUP by
            # construction), checked, checked again with a lemma that is not implied, and trimmed (mi355sat_trim_proof)
            cl = self.cnf.clauses + self.acc
            sup = [list(self.pick(cl)) + [self.sign(int(r.integers(self.nb)) + 1)] for _ in range(3)]
            return sup, [self.unused[-1]]
        return None

    def run(self):
        case, r, n = self.case, self.rng, self.case.n_solves
        tail = 3 if case.end else 0                      # the solves an ending owns
        kinds = dict(zip([int(i) for i in r.permutation(np.arange(3 if case.simp == 2 else 1, n - tail))[:3]], A_KINDS))
        if case.simp == 2:      # the first solve freezes self.kept; the next two name nothing else and must stay warm
            kinds[0] = kinds[1] = kinds[2] = "kept"
        names = [b for b in case.between if b != "minimize_core"]
        gaps = dict(zip([int(i) for i in r.permutation(np.arange(2 if case.simp == 2 else 0, n - 1 - tail))[:len(names)]], names))
        want_minimize = case.between.count("minimize_core")
        queue = [case.menu[i] for i in r.permutation(len(case.menu))]
        queue.sort(key=lambda cls: cls != "elim_kept")      # (stable: those first, while the kept variables are known)
        tries = collections.Counter()
        steps = []
        backbone = None
        for i in range(n):
            clauses = []
            a = None
            if case.end and i == n - 3 and case.end == "contradict":
                backbone = self.hidden_backbone_literal()
                a = [-backbone]
            if case.end and i == n - 2:
                if case.end == "contradict":
                    clauses = [("contradict_learnt", [-backbone])]
                    self.acc.append([-backbone])
                    self.classes["contradict_learnt"] += 1
                else:
                    clauses = self.emit("fixed_empty")
                    assert clauses, "no fixed literal to end the sequence with"
            elif i > 0:
                left = max(1, n - tail - i)
                k = max(int(r.integers(0, 4)), -(-len(queue) // left))
                if case.simp == 2 and i <= 2:
                    k = min(1, queue.count("elim_kept"))
                for _ in range(k):
                    cls = queue.pop(0) if queue else self.pick(case.menu)
                    got = None if (case.end and i == n - 1) else self.emit(cls)
                    if got:
                        clauses += got
                    elif tries[cls] < 4 and not (case.end and i == n - 1):
                        tries[cls] += 1
                        queue.append(cls)
                if case.end and i == n - 1:
                    c = self.mixed(3)
                    self.acc.append(c)
                    clauses = [("len3", c)]          # after the refutation: never attached
            kind = kinds.get(i, "rand")
            if a is None:
                a = self.assumptions(kind)
            if kind in A_KINDS:
                self.kinds[kind] += 1
            o = self.oracle()
            v = o.solve(a)
            letter = "S" if v == 10 else ("E" if o.solve() == 20 else "U")
            step = dict(clauses=clauses, assumptions=a, verdict=letter, between=None, interrupted=False)
            if steps and steps[-1]["between"] and steps[-1]["between"][0] == "interrupt":
                step["interrupted"] = True
            else:
                self.last = (a, letter)
            name = gaps.get(i)
            if name is None and want_minimize and letter == "U" and i < n - 1 - tail and not step["interrupted"]:
                name, want_minimize = "minimize_core", want_minimize - 1
            if name:
                step["between"] = (name, self.between_payload(name))
                self.calls[name] += 1
            steps.append(step)
        return steps


def sequence(name):
    """The steps of a case, generated once: dicts with the clauses to add (class, literals), the assumptions, the oracle's
    verdict letter, the call made after the solve (name, payload) and whether an interrupt sent before it stops this solve.
    Also the generator's counters per clause class, call in between and kind of assumption set."""
    if name not in _cache:
        case = GPU_CASES[name]
        g = _Generator(case)
        steps = g.run()
        verdicts = "".join(st["verdict"] for st in steps)
        assert verdicts == case.verdicts, (name, verdicts)
        n_e = verdicts.count("E")
        assert n_e <= 2 and verdicts.endswith("E" * n_e), "a formula-level refutation only in the last two solves"
        _cache[name] = (steps, dict(classes=g.classes, calls=g.calls, kinds=g.kinds, pairs=g.pairs, fixed=g.fixed))
    return _cache[name]


def table_counts(cases):
    """Over the cases: Counter of clause classes, of calls in between, of assumption kinds, and of verdict letters (the
    solves an interrupt stops left out)."""
    tot = dict(classes=collections.Counter(), calls=collections.Counter(), kinds=collections.Counter(), verdicts=collections.Counter())
    for name in cases:
        steps, info = sequence(name)
        for k in ("classes", "calls", "kinds"):
            tot[k].update(info[k])
        tot["verdicts"].update(st["verdict"] for st in steps if not st["interrupted"])
    return tot


# ---- the judge ------------------------------------------------------------------------------------------------------------------
def substitution(simplified):
    """{variable: literal that replaced it} of a cold start, from mi355sat_debug_simplified's list 0: it ends with the two
    binary clauses (~v | r), (v | ~r) of every substituted v, which occurs nowhere else in the list."""
    occ = collections.Counter(abs(l) for c in simplified for l in c)
    sub = {}
    for a, b in zip(simplified, simplified[1:]):
        if len(a) == 2 and len(b) == 2 and a[0] < 0 and b == [-a[0], -a[1]] and occ[-a[0]] == 2 and abs(a[1]) != -a[0]:
            sub[-a[0]] = a[1]
    return sub


def mapped(sub, l):
    while abs(l) in sub:
        l = sub[abs(l)] if l > 0 else -sub[abs(l)]
    return l


class Expected:
    """What include/mi355sat.h says the warm mode does, step by step (the module's docstring)."""

    def __init__(self, case, c):
        self.case, self.c = case, c
        self.warm = self.cold = self.units = self.clauses = 0
        self.resident, self.why, self.refuted, self.proof = False, ColdReason.FIRST, False, False
        self.pending = []            # clauses added since the last solve
        self.sub, self.kept, self.facts = {}, set(), set()      # of the last cold start: substitution, kept variables, level-0 literals
        self.fixed_hits = collections.Counter()
        self.sat_at = -1             # clauses on the handle when it last answered SAT
        self.stops = self.decided_after_stop = self.elim_colds = self.warm_attached = 0
        self.subst_hits = collections.Counter()
        self.warm_classes = collections.Counter()        # clauses of each class that a warm solve attached
        self.attach_launches = self.most_attach_launches = 0     # (of one solve: a second one is grow_workers')

    def go_cold(self, why):
        self.resident, self.why = False, why

    def attach_counts(self):
        units = clauses = 0
        for cl in self.pending:
            m = {mapped(self.sub, l) for l in cl}
            if any(-l in m for l in m):
                continue
            if len(m) == 1:
                units += 1
            else:
                clauses += 1
        return units, clauses

    def solved(self, step, r):
        c, case = self.c, self.case
        i = c.info()
        d = (i["warm_solves"] - self.warm, i["cold_solves"] - self.cold)
        du, dc = i["attached_units"] - self.units, i["attached_clauses"] - self.clauses
        self.warm, self.cold, self.units, self.clauses = i["warm_solves"], i["cold_solves"], i["attached_units"], i["attached_clauses"]
        self.most_attach_launches = max(self.most_attach_launches, i["attach_launches"] - self.attach_launches)
        self.attach_launches = i["attach_launches"]
        names = {abs(l) for cl in self.pending for l in cl} | {abs(l) for l in step["assumptions"]}
        if self.refuted and not self.proof:
            # The oracle refutes the formula alone.  After a refutation without assumptions the handle answers at once, with
            # the empty core; otherwise (the workers may have refuted it under the assumptions only) it may also be a warm
            # solve like any other, with any core the oracle accepts, or one that stops on its budget.
            assert d == (1, 0), (d, i)
            if self.refuted == "plain":
                assert (du, dc) == (0, 0) and r == SolverResult.Unsat and c.log[-1][1] == [], (du, dc, r, c.log[-1])
            else:
                assert (du, dc) in ((0, 0), self.attach_counts()), (du, dc, i)
                assert r == SolverResult.Unsat or (r == SolverResult.Interrupted and case.opts.get("conflict_budget", 0) > 0), r
            if r == SolverResult.Unsat and not step["assumptions"]:
                self.refuted = "plain"
            self.pending = []
            return
        cold = self.proof or not self.resident
        if not cold and d == (0, 1) and case.simp == 2 and not names <= self.kept:
            assert i["last_cold_reason"] == ColdReason.ELIMINATED, i
            self.elim_colds += 1
            cold = True
        elif cold:
            assert d == (0, 1) and i["last_cold_reason"] == (ColdReason.PROOF if self.proof else self.why), (d, i, self.why)
        if cold:
            assert (du, dc) == (0, 0), i
            if self.proof:
                self.proof = False
                c.s.set_proof_path(None)
                self.go_cold(ColdReason.FIRST)
            else:
                self.resident = True
                simplified = c.s.debug_simplified()[0] if case.simp >= 0 else []      # (simp = -1 substitutes nothing)
                self.sub = substitution(simplified)
                self.facts = {cl[0] for cl in simplified if len(cl) == 1}
                used = {abs(l) for cl in c.base.clauses + c.clauses for l in cl}
                self.kept = (set(range(1, c.n_vars + 1)) - used) | {abs(l) for l in step["assumptions"]}
                if [] in simplified:
                    self.resident = False
        else:
            assert d == (1, 0), (d, i, step)
            assert (du, dc) == self.attach_counts(), ((du, dc), self.attach_counts(), self.pending, i)
            self.warm_attached += len(self.pending)
            self.warm_classes.update(cls for cls, _ in step["clauses"])
            for cls, cl in step["clauses"]:      # the classes that exist only through the substitution did go through it
                if cls in ("equiv_dup", "equiv_taut") and case.simp >= 0:
                    m = [mapped(self.sub, l) for l in cl]
                    assert (len(set(m)) < len(m)) if cls == "equiv_dup" else any(-l in m for l in m), (cls, cl, m)
                    self.subst_hits[cls] += 1
                if cls.startswith("fixed") and case.simp >= 0:      # ... and those over level-0 facts met facts the handle has
                    m = [mapped(self.sub, l) for l in cl]
                    assert any((l if cls == "fixed_sat" else -l) in self.facts for l in m), (cls, cl, m)
                    self.fixed_hits[cls] += 1
        self.pending = []
        if r == SolverResult.Sat:
            self.sat_at = len(c.clauses)
        if step["verdict"] == "E" and r == SolverResult.Unsat:
            self.refuted = "plain" if not step["assumptions"] else "under assumptions"


def call_between(c, e, name, payload, tmp_path):
    """One of the handle's other entry points between two solves, judged by the oracle where it has an answer; tells `e`
    what the header says the call does to the warm state."""
    s = c.s
    lits, offs = c.formula()
    if name == "minimize_core":
        before = s.core()
        launches = not (len(before) == 0 or (len(before) == 1 and e.sat_at == len(c.clauses)))
        info = c.run(s.minimize_core)
        core = s.core()
        assert is_subsequence(core, before) and len(set(core)) == len(core), (core, before)
        assert c.oracle().solve(core) == 20, core
        assert [l for l in dict.fromkeys(before) if s.failed(l)] == core
        assert (info["candidates"] > 0) == launches, (info, before)
        if info["minimal"]:
            for l in core:
                assert c.oracle().solve([x for x in core if x != l]) == 10, ("the core is not irreducible", core, l)
        if launches:
            e.go_cold(ColdReason.OTHER_SEARCH)
    elif name == "propagate_batch":
        confl, vals, tl = s.propagate_batch(payload, n_vars=c.n_vars)
        for k, dec in enumerate(payload):
            want, v, n, _ = ora.bcp(lits, offs, c.n_vars, dec)
            assert want == confl[k], (k, dec)
            if not want:
                assert np.array_equal(v, vals[k]) and n == tl[k], (k, dec)
        e.go_cold(ColdReason.OTHER_SEARCH)
    elif name == "solve_batch":
        res = c.run(lambda: s.solve_batch(payload))
        for k, (a, got) in enumerate(zip(payload, res)):
            assert got.value == c.oracle().solve(a), (k, a, got)
            if got == SolverResult.Sat:
                m = s.solution_of(k, c.n_vars)
                assert ora.check_model(lits, offs, m) == -1 and all(m[abs(l) - 1] == (1 if l > 0 else -1) for l in a), (k, a)
            else:
                core = s.core_of(k)
                assert is_subsequence(core, a) and c.oracle().solve(core) == 20, (k, a, core)
        e.go_cold(ColdReason.OTHER_SEARCH)
    elif name == "sweep":
        s.sweep_begin(payload)
        res, nd, n_steps = None, 0, 0
        while nd < len(payload):
            res, nd = c.run(s.sweep_step)
            n_steps += 1
            assert n_steps < 400, "the sweep in between does not end"
        for k, (a, got) in enumerate(zip(payload, res)):
            assert got.value == c.oracle().solve(a), (k, a, got)
            if got == SolverResult.Sat:
                m = s.sweep_solution_of(k, c.n_vars)
                assert ora.check_model(lits, offs, m) == -1 and all(m[abs(l) - 1] == (1 if l > 0 else -1) for l in a), (k, a)
        s.sweep_end()
        e.go_cold(ColdReason.OTHER_SEARCH)
    elif name == "check_proof":
        sup, not_implied = payload
        proof = [l for lemma in sup[:2] for l in lemma + [0]]
        info = s.check_proof(proof, target=sup[2])
        assert info["valid"] == 1 and info["n_lemmas"] == 2 and info["first_failed"] is None, info
        info = s.check_proof(proof + not_implied + [0], target=sup[2])
        assert info["valid"] == 0 and info["first_failed"] == 2, info
        trim = s.trim_proof(proof, target=sup[2])
        assert trim["check"]["valid"] == 1 and trim["core"] and set(trim["lemmas"]) <= {0, 1}, trim
        rests_on = [(c.base.clauses + c.clauses)[k] for k in trim["core"]]
        assert oracle_on(rests_on, c.n_vars).solve([-l for l in sup[2]]) == 20, "the trimmed core does not imply the target"
        e.go_cold(ColdReason.OTHER_SEARCH)
    elif name == "set_phases":
        s.set_phases(payload)                           # never makes a solve start cold
    elif name == "proof_path":
        s.set_proof_path(str(tmp_path / "between.drup"))
        e.proof = True
    elif name == "set_schedule":
        s.debug_set_schedule(*payload)
        e.go_cold(ColdReason.FIRST)
    elif name == "toggle_incremental":
        s.set_incremental(False)
        s.set_incremental(True)
        e.go_cold(ColdReason.FIRST)
    elif name == "interrupt":
        s.interrupter().interrupt()                     # stops the next solve, which consumes it
    else:
        raise ValueError(name)


def run_sequence(make_solver, name, tmp_path, limit_s=None, release=None, grows=False, **build):
    """One case on a handle of `make_solver` (emulator or GPU) in the build given; every solve, every call in between and
    the counters of the warm mode judged as the module's docstring says.  limit_s puts every search call under a deadline
    (a hang becomes an undecided answer, which fails the comparison); release() returns the process's parked slab buffer,
    which the sequence of 258 workers needs gone (tests/test_incremental.py says why).  Returns (Checked, Expected): the
    caller asserts the build and closes."""
    case = GPU_CASES[name]
    steps, _ = sequence(name)
    cnf, _ = base_formula(case)
    opts = dict(workers=case.workers, simp=case.simp, slice_conflicts=100)
    opts.update({k: v for k, v in case.opts.items() if k not in ("p_model", "n_fresh")})
    opts.update(build)
    if release and case.workers > 256:
        release()
    s = make_solver(**opts)
    s.debug_keep_simplified()
    c = Checked(cnf, s, n_vars=cnf.n_vars + case.opts.get("n_fresh", N_FRESH), run=(lambda fn: within(limit_s, s, fn)) if limit_s else None)
    e = Expected(case, c)
    budget = case.opts.get("conflict_budget", 0) > 0
    stopped = False
    for k, step in enumerate(steps):
        for _, cl in step["clauses"]:
            c.add(cl)
            e.pending.append(cl)
        r = c.solve(step["assumptions"], may_stop=budget or step["interrupted"])
        if step["interrupted"]:
            assert r == SolverResult.Interrupted, (k, r)
        elif r == SolverResult.Interrupted:
            e.stops += 1
            stopped = True
        elif stopped:
            e.decided_after_stop += 1
        e.solved(step, r)
        if step["between"]:
            call_between(c, e, *step["between"], tmp_path)
    if budget:      # some solve stops on the budget in the middle of a search path, a later one on the same workers is decided
        assert e.stops >= 1 and e.decided_after_stop >= 1 and 2 * e.stops <= len(steps), (e.stops, e.decided_after_stop, [r.name for r, _ in c.log])
    if case.workers > 256 and grows:     # the recipe of test_workers_grown_after_the_attach_get_the_attached_clauses
        assert s.debug_last_search_build()["active"] == case.workers, "the fleet did not grow"
        assert e.most_attach_launches == 2, "no warm solve attached its clauses a second time, to workers created after the attach"
    if case.workers >= 2:
        acc = collections.namedtuple("Acc", "lits offsets n_vars")(*c.formula(), c.n_vars)
        assert_ring_records_are_implied(s, acc)
    print(name, "".join({10: "S", 20: "U", 0: "-"}[r.value] for r, _ in c.log), c.info(), "budget stops", e.stops,
          "eliminated-variable cold starts", e.elim_colds)
    return c, e
