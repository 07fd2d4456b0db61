"""Shared helpers for the test-suite (test infrastructure)."""
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


VERDICTS = golden("verdicts.json")


def terrain_rows(name):
    if name.startswith("rect"):
        w, h = (int(v) for v in name[4:].split("x"))
        return ["X" * w] * h
    return VERDICTS["terrains"][name]


def make_grid(name):
    from timberborn_support_solver_amd import WorldGrid
    return WorldGrid.from_rows(terrain_rows(name))


def platform_defs(pset):
    from timberborn_support_solver_amd import PLATFORMS_DEFAULT
    return PLATFORMS_DEFAULT if pset == "default" else [(1, 1)]


_emu = None


def emu_lib():
    """The wavefront-emulator build of the solver library (tests/emu): CPU-side logic tests only."""
    global _emu
    if _emu is None:
        import subprocess
        d = os.path.join(ROOT, "tests", "emu")
        if os.environ.get("TBS_EMU_LIB"):     # e.g. the sanitizer build of tests/emu/asan.mk
            _emu = ctypes.CDLL(os.environ["TBS_EMU_LIB"])
            return _emu
        subprocess.check_call(["make", "-C", d, "libmi355sat_emu.so"], stdout=subprocess.DEVNULL)
        _emu = ctypes.CDLL(os.path.join(d, "libmi355sat_emu.so"))
    return _emu


def splitmix64(seed):
    z = seed & (2 ** 64 - 1)
    while True:
        z = (z + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        x = z
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        yield x ^ (x >> 31)


def scripted_decisions(enc, grid, seed, n_decisions, p_positive=0.35):
    """Seeded decision scripts over platform variables: mostly negative
    literals (a positive 5x5 forces a lot), so that many scripts reach a fixpoint."""
    g = splitmix64(seed)
    dims = enc.platform_dims()
    dec = []
    for _ in range(n_decisions):
        r = next(g)
        x, y = (r >> 8) % grid.width, (r >> 24) % grid.height
        d = dims[(r >> 40) % len(dims)]
        v = enc.platform_var(int(x), int(y), d)
        pos = ((r >> 52) % 1000) < int(1000 * p_positive)
        dec.append(v if pos else -v)
    return dec


_oracle_enc = {}


def oracle_encoding(enc, grid):
    """The oracle's literal restatement of the encoder for the same terrain / platform set (cached: it is
    pure Python).  Its variable numbering equals the product's (tests/test_encoder.py proves the CNFs
    bit-exact), so product models can be read through it."""
    from oracle import encoder_oracle as eo
    key = (tuple(grid.rows()), tuple(enc.defs))
    if key not in _oracle_enc:
        _oracle_enc[key] = eo.Encoding(list(enc.defs), eo.grid_from_rows(grid.rows()))
    return _oracle_enc[key]


def check_sat_answer(cnf, model, enc, grid, k):
    """A SAT answer is right iff the model satisfies every clause, the layout validates and has <= k
    platforms.  Layout and validity are derived twice: by the product (libtbs_host.so) and by the
    oracle's restatement of platform_layout.rs (oracle/layout_oracle.py) - on the GPU box the product's
    validator must not be its own judge."""
    from oracle import layout_oracle as lo, oracle as ora
    from timberborn_support_solver_amd import PlatformLayout
    assert ora.check_model(cnf.lits, cnf.offsets, model) == -1
    lay = PlatformLayout.from_assignment(model[:enc.n_vars], enc)
    assert lay.validate(grid).is_valid()
    assert lay.platform_count() <= k
    o = oracle_encoding(enc, grid)
    q = lo.from_assignment(np.asarray(model[:enc.n_vars]).tolist(), o)
    assert lo.is_valid(lo.validate(q, o.grid)) and lo.platform_count(q) <= k
    assert sorted(lay.platforms()) == sorted((x, y, d[0], d[1], int(r)) for (x, y), (d, r) in q.items())
    return lay


def assert_ring_records_are_implied(solver, cnf, max_records=None):
    """Exchange soundness: every clause in the learnt-clause exchange ring must follow from the caller's
    formula ALONE (workers attach ring records under any assumption set and declare UNSAT when one is
    falsified at level 0).  The oracle solver refutes formula AND NOT(clause) for each record."""
    from oracle import oracle as ora
    recs = solver.debug_share_ring()
    o = ora.OracleSolver()
    o.add_cnf(cnf.lits, cnf.offsets)
    o.reserve(cnf.n_vars)
    seen = set()
    for c in recs[:max_records]:
        assert 1 <= len(c) <= 31 and all(l != 0 and abs(l) <= cnf.n_vars for l in c), c
        key = tuple(sorted(c))
        if key in seen:
            continue
        seen.add(key)
        assert o.solve([-l for l in c]) == 20, ("exchange ring holds a clause the formula does not imply", c)
    return len(recs)


def assert_search_build(solver, lds, wps):
    """The handle's search launches all ran ms_search_kernel<lds, wps> (mi355sat_debug_last_search_build): the last one
    did, and no other build was launched since the handle was made.  Returns the hook's record."""
    b = solver.debug_last_search_build()
    assert (b["lds"], b["wps"]) == (lds, wps) and b["builds"] == {(lds, wps)} and b["launches"] > 0, (b, "wanted", (lds, wps))
    return b


def random_cnf(seed, n_vars, n_clauses, lens=(3,)):
    """Uniform random k-SAT as a list of clauses (DIMACS literals): every clause draws its length from `lens` (no draw when
    there is one length only), then that many distinct variables and a fair sign for each."""
    rng = np.random.default_rng(seed)
    cl = []
    for _ in range(n_clauses):
        k = lens[0] if len(lens) == 1 else int(rng.choice(lens))
        vs = rng.choice(n_vars, size=k, replace=False)
        cl.append([int(v + 1) * (1 if rng.random() < 0.5 else -1) for v in vs])
    return cl


def salt_cnf(clauses, seed, n_vars, n_each=6, n_units=3):
    """The same formula made awkward for a clause loader: `n_each` exact duplicates, clauses with one literal repeated,
    permuted duplicates, tautologies (x and -x in one clause: they constrain nothing) and `n_units` unit clauses, shuffled in
    among the others."""
    rng = np.random.default_rng(seed)
    out = [list(c) for c in clauses]
    pick = lambda: list(out[int(rng.integers(len(clauses)))])
    extra = []
    for _ in range(n_each):
        extra.append(pick())                                        # duplicate
        c = pick(); c.insert(int(rng.integers(len(c) + 1)), c[int(rng.integers(len(c)))]); extra.append(c)   # repeated literal
        c = pick(); extra.append([c[i] for i in rng.permutation(len(c))])                                     # permuted duplicate
        c = pick(); c.insert(int(rng.integers(len(c) + 1)), -c[int(rng.integers(len(c)))]); extra.append(c)  # tautology
        v = int(rng.integers(n_vars)) + 1; extra.append([v, -v])                                              # binary tautology
    for _ in range(n_units):
        extra.append([(int(rng.integers(n_vars)) + 1) * (1 if rng.random() < 0.5 else -1)])
    for c in extra:
        out.insert(int(rng.integers(len(out) + 1)), c)
    return out


STRUCTURE = ("equiv", "failed", "subsume", "strengthen", "long", "elim", "salt")


def structured_cnf(seed, n_vars, n_clauses, lens=(2, 3, 4, 5, 6), features=STRUCTURE, refute=None, glue=0.5):
    """A random_cnf base of n_clauses over the variables 1..n_base (mixed lengths, below the threshold) with the structure planted that
    the simplification before search lives on and uniform random k-SAT does not have.  Every feature is a switch (`features`,
    names of STRUCTURE), so that a case can isolate one:
      equiv       binary implication cycles of 2..5 literals with mixed signs; two cycles joined by a later binary clause; a
                  cycle whose representative a mutual pair then fixes; and - with "elim" - cycles whose representative is cheap
                  to eliminate, the other member sitting in a clause of its own
      failed      l -> a, l -> b, (~a | ~b) through binary and through ternary clauses; a -> m and ~a -> m; a -> m and
                  ~a -> ~m, both through paths that are not binary clauses
      subsume     supersets of existing clauses, exact and permuted duplicates
      strengthen  pairs (C | x), (D | ~x) with C inside D; a clause two others strengthen on different literals in one pass;
                  a strengthening that leaves a binary; the mutual pair (a | b), (a | ~b); all four sign patterns of (x, y)
                  next to a literal a (two passes of strengthening leave the unit a; unit propagation does not find it)
      long        a clause of 70 literals with a superset (too long to subsume: both stay) and a clause of 66 literals with a
                  binary subsumer
      elim        variables with 1..3 occurrences per polarity, pure literals, the gates x = a & b and x = a | b, all sixteen
                  sign patterns of four variables next to a literal (three passes of strengthening leave (x | a), (~x | a):
                  eliminating x makes the unit resolvent a)
      salt        salt_cnf: duplicates, repeated literals, tautologies, units
    The gadgets' own variables are n_base+1 .. n_vars (n_base = n_vars minus what the chosen gadgets need), their side literals
    come from the base, and `glue` * (number of gadget variables) random ternary clauses tie gadget variables to base variables.
    refute = "scc" puts x and ~x into one implication component, "failed" makes a literal fail in both polarities (through
    ternary clauses): the planted structure alone refutes the formula.
    Returns (clauses, special): special = the gadgets' variables - substituted, fixed or eliminated ones among them."""
    rng = np.random.default_rng(seed)
    need = {"equiv": 18 + (8 if "elim" in features else 0), "failed": 15, "strengthen": 9, "long": 72, "elim": 13}
    n_own = sum(need.get(f, 0) for f in features) + {None: 0, "scc": 3, "failed": 5}[refute]
    n_base = n_vars - n_own
    assert n_base >= 12, "structured_cnf: n_vars leaves too few variables for the base"
    cl = random_cnf(seed, n_base, n_clauses, lens)
    nxt = [n_base]
    special = []

    def fresh(k):
        vs = list(range(nxt[0] + 1, nxt[0] + k + 1))
        nxt[0] += k
        assert nxt[0] <= n_vars
        special.extend(vs)
        return vs

    def sign(v):
        return v if rng.random() < 0.5 else -v

    def base(k):                                    # k literals over distinct base variables
        return [sign(int(v) + 1) for v in rng.choice(n_base, size=k, replace=False)]

    def cycle(ls):                                  # l0 -> l1 -> ... -> l0
        return [[-ls[i], ls[(i + 1) % len(ls)]] for i in range(len(ls))]

    extra = []
    if "equiv" in features:
        for k in (2, 3, 4, 5):
            ls = [sign(v) for v in fresh(k - 1)] + base(1)
            extra += cycle([ls[i] for i in rng.permutation(k)])
        a, b = [sign(v) for v in fresh(2)], [sign(v) for v in fresh(3)]         # two cycles, joined below
        extra += cycle(a) + cycle(b)
        joined = [[-a[0], b[1]], [-b[2], a[1]]]
        r, q, x = fresh(3)                          # q == ~r, and r fixed by (r | x), (r | ~x): a failed literal, found after the cycle
        extra += cycle([-r, q]) + [[r, x], [r, -x]] + [[-q] + base(2)]
        if "elim" in features:
            for _ in range(4):                      # q == +-r; after the substitution r has three occurrences
                r, q = fresh(2)
                s = 1 if rng.random() < 0.5 else -1
                extra += cycle([r, s * q]) + [[r] + base(2), [-r] + base(1), [s * q] + base(2)]
    if "failed" in features:
        l, a, b = fresh(3)
        extra += [[-l, a], [-l, b], [-a, -b]]
        l, a, b, c = fresh(4)
        extra += [[-l, a], [-l, -a, b], [-a, -b, c], [-c, -l]]
        a, u, w, m = fresh(4)                       # a -> u, a & u -> m;  ~a -> w, ~a & w -> m
        extra += [[-a, u], [-a, -u, m], [a, w], [a, -w, m], [-m] + base(2)]
        a, u, w, m = fresh(4)                       # a -> u, a & u -> m;  ~a -> w, ~a & w -> ~m
        extra += [[-a, u], [-a, -u, m], [a, w], [a, -w, -m], [m] + base(2), [-m] + base(2)]
    if "subsume" in features:
        for _ in range(6):
            c = list(cl[int(rng.integers(len(cl)))])
            more = [l for l in base(3) if abs(l) not in {abs(x) for x in c}][:int(rng.integers(1, 4))]
            extra.append([c[i] for i in rng.permutation(len(c))] + more)
        for _ in range(4):
            c = cl[int(rng.integers(len(cl)))]
            extra += [list(c), [c[i] for i in rng.permutation(len(c))]]
    if "strengthen" in features:
        for _ in range(3):
            c, x = base(5), fresh(1)[0]
            extra += [c[:2] + [x], c[:2 + int(rng.integers(0, 3))] + [-x]]
        e = base(5)                                 # loses e[2] to the first and e[3] to the second
        extra += [e, [e[0], e[1], -e[2]], [e[0], e[1], -e[3]]]
        a, x = base(2)[0], fresh(1)[0]
        extra += [[a, x], [a] + base(1) + [-x]]     # leaves a binary
        a, b = fresh(2)
        extra += [[a, b], [a, -b], [-a] + base(2)]  # the mutual pair
        x, y, a = fresh(3)
        extra += [[sx * x, sy * y, a] for sx in (1, -1) for sy in (1, -1)] + [[-a] + base(2)]
    if "long" in features:
        fill = fresh(72)
        big = [sign(v) for v in fill]
        extra += [big[:70], big]
        a, b = base(2)
        extra.append([a, b] + [sign(v) for v in fill[:64]])
        extra.append([a, b])
    if "elim" in features:
        for n_pos, n_neg in ((1, 1), (1, 2), (2, 2), (3, 2)):
            x = fresh(1)[0]
            extra += [[x] + base(2) for _ in range(n_pos)] + [[-x] + base(2) for _ in range(n_neg)]
        for _ in range(2):
            x = sign(fresh(1)[0])
            extra += [[x] + base(2), [x] + base(3)]                                         # pure
        x, (a, b) = fresh(1)[0], base(2)
        extra += [[-x, a], [-x, b], [x, -a, -b], [x] + base(2), [-x] + base(2)]              # x = a & b
        x, (a, b) = fresh(1)[0], base(2)
        extra += [[x, -a], [x, -b], [-x, a, b], [x] + base(2), [-x] + base(2)]               # x = a | b
        w, x, y, z, a = fresh(5)
        extra += [[sw * w, sx * x, sy * y, sz * z, a] for sw in (1, -1) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
        extra.append([-a] + base(2))
    if refute == "scc":
        x, y, z = fresh(3)
        extra += cycle([x, y, -x, z])
    elif refute == "failed":
        l, a, b, c, d = fresh(5)
        extra += [[-l, a], [-l, b], [-a, -b, -l], [l, c], [l, d], [-c, -d, l]]
    assert nxt[0] == n_vars
    gadget_vars = list(range(n_base + 1, nxt[0] + 1))
    if "long" in features:
        gadget_vars = [v for v in gadget_vars if v not in fill]
    for _ in range(int(glue * len(gadget_vars))):
        extra.append([sign(int(rng.choice(gadget_vars)))] + base(2))
    out = [list(c) for c in cl]
    for c in extra:
        out.insert(int(rng.integers(len(out) + 1)), c)
    if "equiv" in features:
        out += joined                               # the binary clauses that join the two cycles come last
    if "salt" in features:
        out = salt_cnf(out, seed + 1000, n_base, n_each=3, n_units=2)
    return out, special


class Csr:
    """A clause list in the shape the tests pass around (like the encoder's Cnf: lits, offsets, n_vars, n_clauses)."""

    def __init__(self, clauses, n_vars):
        from oracle import oracle as ora
        self.clauses, self.n_vars, self.n_clauses = clauses, n_vars, len(clauses)
        self.lits, self.offsets = ora.to_csr(clauses)


def long_list_formula(seed, n_vars=360, n_long=140, n_hubs=6, per_hub=44, hub_len=(9, 40)):
    """A formula cut for the BCP step's side paths: clauses of 10..48 literals (tails to scan, several per step), a few
    hub literals watched by 44 long clauses each (watch lists far longer than a lane group: the flat remainder, its
    in-place compaction and the re-queueing when two groups meet in one clause), binary and ternary chains between."""
    rng = np.random.default_rng(seed)
    clauses = []

    def rand_clause(k, first=None):
        vs = rng.choice(np.arange(n_hubs, n_vars), size=k, replace=False)
        c = [int(v + 1) * (1 if rng.random() < 0.5 else -1) for v in vs]
        return ([first] + c) if first is not None else c

    for _ in range(n_long):
        clauses.append(rand_clause(int(rng.integers(10, 49))))
    for h in range(n_hubs):                          # -(h+1) in a watched position of every one of its clauses
        for _ in range(per_hub):
            c = rand_clause(int(rng.integers(hub_len[0], hub_len[1])), first=-(h + 1))
            if rng.random() < 0.5:
                c[0], c[1] = c[1], c[0]
            clauses.append(c)
    for _ in range(n_vars):                          # implication chains
        a, b, c = (int(x) for x in rng.choice(np.arange(n_hubs, n_vars), size=3, replace=False))
        sa, sb, sc = (1 if rng.random() < 0.5 else -1 for _ in range(3))
        clauses.append([sa * (a + 1), sb * (b + 1)] if rng.random() < 0.35 else [sa * (a + 1), sb * (b + 1), sc * (c + 1)])
    lits = np.array([l for c in clauses for l in c], dtype=np.int32)
    offsets = np.cumsum([0] + [len(c) for c in clauses]).astype(np.uint64)
    return lits, offsets, n_vars, n_hubs, rng
