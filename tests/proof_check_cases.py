"""Cases and judge of the device's DRUP proof checker, mi355sat_check_proof (tests/test_emu_proof_check.py on the wavefront
emulator, tests/test_gpu_proof_check.py on the MI355X; test infrastructure).

The judge is never the code under test.  What the checker must answer is defined by the oracle's occurrence-list unit
propagation (oracle.bcp) applied lemma by lemma - `reference()` - and, for the verdict of a proof of the empty clause, by
oracle.check_rup on the proof without its deletion records.  Proofs come from OracleSolver.enable_proof(): deterministic and
independent of the product; the tests that name the device's own proofs make those themselves."""
import random

import numpy as np

import fuzz_cases as fc
from helpers import Csr
from oracle import oracle as ora

DEL = -2 ** 31
ERR_STATE, ERR_ARG = -3, -4


def lemmas_of(proof):
    """Flat proof words (dimacs.read_drup's form) -> (lemmas as lists, number of deletion records)."""
    lemmas, n_del, cur, deleting = [], 0, [], False
    for x in (int(v) for v in proof):
        if x == DEL:
            deleting = True
        elif x == 0:
            if deleting:
                n_del += 1
            else:
                lemmas.append(cur)
            cur, deleting = [], False
        else:
            cur.append(x)
    assert not cur and not deleting, "unterminated proof"
    return lemmas, n_del


def flat(lemmas, deletions=()):
    """Lemma lists -> flat words; deletions: {index: [clauses deleted right before lemma `index`]}."""
    deletions = dict(deletions)
    out = []
    for i, c in enumerate(list(lemmas) + [None]):
        for d in deletions.get(i, ()):
            out += [DEL] + list(d) + [0]
        if c is not None:
            out += list(c) + [0]
    return np.asarray(out, dtype=np.int64).astype(np.int32)


def reference(clauses, n_vars, lemmas, target=(), refuted=True, start=0):
    """The oracle's answer: (valid, first_failed, refuted_at), indices as in mi355sat_proof_info (the target is lemma number
    len(lemmas); None = no such lemma).  first_failed: the smallest i for which oracle.bcp(F + lemmas[:i], negated lemma i)
    reports no conflict; refuted_at: the smallest i at which oracle.bcp(F + lemmas[:i]) alone reports one - from there on
    every lemma is RUP.  refuted = False: refuted_at is not wanted (None), and the walk ends at the first failure.
    start: the lemmas below it are known to be RUP (the same lemmas behind the same prefix in a proof already judged)."""
    items = [list(c) for c in lemmas] + [list(target)]
    lits, offs = ora.to_csr([list(c) for c in clauses] + items)      # every database is a prefix of this one
    first_failed = refuted_at = None
    for i, lem in enumerate(items):
        if i < start:
            continue
        n = len(clauses) + i
        db = (lits[:int(offs[n])], offs[:n + 1])
        if refuted and ora.bcp(*db, n_vars, [])[0]:
            refuted_at = i
            break
        if first_failed is None and not ora.bcp(*db, n_vars, [-l for l in lem])[0]:
            first_failed = i
            if not refuted:
                break
    return (1 if first_failed is None else 0), first_failed, refuted_at


def oracle_verdict(cnf, lemmas):
    """oracle.check_rup on a proof of the empty clause (no deletion records)."""
    return ora.check_rup(cnf.lits, cnf.offsets, cnf.n_vars, flat(lemmas))


def answer(info):
    return info["valid"], info["first_failed"], info["refuted_at"]


def check(make_solver, clauses, n_vars, proof, target=(), segments=0, chunk=0, **opts):
    """new, add_cnf, reserve, check_proof on a fresh handle: the info dict."""
    s = make_solver(**opts)
    try:
        cnf = Csr(clauses, n_vars)
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(n_vars)
        if chunk:
            s.debug_proof_check_chunk(chunk)
        return s.check_proof(proof, target=target, segments=segments)
    finally:
        s.close()


# ---- 1. by inspection ------------------------------------------------------------------------------------------------------
XOR2 = [[1, 2], [-1, 2], [1, -2], [-1, -2]]                 # refuted by one decision, not by propagation
OPEN = [[1, 2], [-1, 2], [3, 4]]                            # satisfiable; implies 2
CHAIN = [[1, 2], [-1, 2], [-2, 3, 4], [-2, 3, -4], [-3, 5], [-3, -5]]   # implies 2, then 3, then falls
# name: (clauses, n_vars, lemmas, deletions, target, (valid, first_failed, refuted_at))
INSPECTION = {
    "empty-proof-propagation-refutes": ([[1], [-1, 2], [-2]], 2, [], {}, (), (1, None, 0)),
    "empty-proof-contradictory-units": ([[1], [-1]], 1, [], {}, (), (1, None, 0)),
    "empty-proof-satisfiable": ([[1, 2]], 2, [], {}, (), (0, 0, None)),
    "first-lemma-not-rup": (XOR2, 3, [[3], [2]], {}, (), (0, 0, 2)),
    # a tautology, a repeated literal, one satisfied at level 0 (2 is a fact by then), one whose check meets a TRUE literal
    # behind an unassigned one; the target (2) is a level-0 fact
    "lemmas-that-count-as-rup": (OPEN, 5, [[5, -5], [2, 2], [2, 3], [1, 2]], {}, (2,), (1, None, None)),
    "the-same-without-a-target": (OPEN, 5, [[5, -5], [2, 2], [2, 3], [1, 2]], {}, (), (0, 4, None)),
    "units-refute-before-the-end": (CHAIN, 7, [[2], [3], [6], [7, -6]], {}, (), (1, None, 2)),
    # a tautological lemma, and a tautological target, standing where propagation alone refutes the database: the index
    # counts for refuted_at although the lemma itself is neither checked nor attached
    "tautology-at-the-refutation": (XOR2, 5, [[2], [5, -5], [3]], {}, (), (1, None, 1)),
    "tautology-right-before-the-refutation": (XOR2, 5, [[5, -5], [2], [4, -4], [3]], {}, (), (1, None, 2)),
    "tautological-target-at-the-refutation": (XOR2, 5, [[2]], {}, (5, -5), (1, None, 1)),
    "tautological-target-without-refutation": (OPEN, 5, [[2]], {}, (5, -5), (1, None, None)),
    "target-rup": (OPEN, 4, [], {}, (2,), (1, None, None)),
    "target-not-rup": (OPEN, 4, [], {}, (3,), (0, 0, None)),
    "target-rup-through-a-lemma": (CHAIN, 7, [[2]], {}, (3, 6), (1, None, None)),
    # honoured, the first deletion would leave (2) without support and the second would take the fact 2 away: ignored
    "deletions-are-counted-and-ignored": (CHAIN, 7, [[2], [3]], {0: [[1, 2]], 1: [[2], [-2, 3, 4]]}, (), (1, None, 2)),
}


def run_inspection(make_solver, name, **opts):
    clauses, n_vars, lemmas, dels, target, want = INSPECTION[name]
    n_del = sum(len(d) for d in dels.values())
    assert reference(clauses, n_vars, lemmas, target) == want, "the case's expectation is not the oracle's"
    if not target:
        assert oracle_verdict(Csr(clauses, n_vars), lemmas) == want[0]
    for segments in (0, 1, 2, 3):
        info = check(make_solver, clauses, n_vars, flat(lemmas, dels), target, segments=segments, **opts)
        assert answer(info) == want, (name, segments, info)
        assert info["n_lemmas"] == len(lemmas) and info["n_deletions_ignored"] == n_del, info
        assert not info["interrupted"]


def run_argument_errors(make_solver, solver_error):
    import pytest
    s = make_solver()
    cnf = Csr(OPEN, 4)
    s.add_cnf(cnf.lits, cnf.offsets)
    for proof, target in [([5, 0], ()), ([1, -5, 0], ()), ([1, 0], (1, 0, 2)), ([1, 0], (5,)), ([1, 2], ()), ([1, DEL, 2, 0], ())]:
        with pytest.raises(solver_error) as e:
            s.check_proof(np.asarray(proof, dtype=np.int32), target=target)
        assert e.value.code == ERR_ARG, (proof, target)
    s.reserve(5)                                  # raises the handle's highest variable
    assert s.check_proof(np.asarray([5, -5, 0], dtype=np.int32), target=(2,))["valid"] == 1
    s.sweep_begin([[1], [-1]])
    with pytest.raises(solver_error) as e:
        s.check_proof(np.asarray([2, 0], dtype=np.int32), target=(2,))
    assert e.value.code == ERR_STATE
    s.sweep_end()
    assert s.check_proof(np.asarray([2, 0], dtype=np.int32), target=(2,))["valid"] == 1
    s.close()


# ---- 2. long lemmas --------------------------------------------------------------------------------------------------------
LONG_N = (63, 64, 65, 70, 129)


def long_case(n):
    """F = (x1 .. xn), (~xn | y), (~y | w).  (x1 .. x(n-1) | y) is RUP with n literals, so is (x1 .. x(n-1) | w); without
    x(n-1) it is not RUP.  Returns (clauses, n_vars, lemma_y, lemma_w, lemma_w_short)."""
    y, w = n + 1, n + 2
    xs = list(range(1, n + 1))
    return [xs, [-n, y], [-y, w]], n + 2, xs[:-1] + [y], xs[:-1] + [w], xs[:-2] + [w]


def long_case_through_the_lemma(n):
    """X = x1 .. x(n-1);  F = (X | a | b), (X | a | ~b), (~a | d | e), (~a | d | ~e).  A = (X | a), n literals, is RUP; B = (X | d)
    is RUP only once A is attached (without it ~X, ~d propagate nothing).  Returns (clauses, n_vars, A, B)."""
    X = list(range(1, n))
    a, b, d, e = n, n + 1, n + 2, n + 3
    return [X + [a, b], X + [a, -b], [-a, d, e], [-a, d, -e]], n + 3, X + [a], X + [d]


def long_case_true_literal_late(n):
    """F = (t), (a | b).  L = (x1 .. x(n-1) | t) has its only TRUE literal in the last position - for n > 64 in a later lane
    round than the negations already on the trail, which the check then takes back; the lemmas behind it see a clean
    level 0: (a) is not RUP, (a | b | x1) is.  Returns (clauses, n_vars, L, not_rup, rup)."""
    t, a, b = n, n + 1, n + 2
    return [[t], [a, b]], n + 2, list(range(1, n)) + [t], [a], [a, b, 1]


def run_long(make_solver, n, **opts):
    clauses, nv, ly, lw, lw_short = long_case(n)
    clauses2, nv2, la, lb = long_case_through_the_lemma(n)
    # what the reference says, by inspection
    assert reference(clauses, nv, [ly, lw], lw) == (1, None, None)
    assert reference(clauses, nv, [ly, lw_short], lw) == (0, 1, None)
    assert reference(clauses, nv, [ly], lw_short) == (0, 1, None)
    assert reference(clauses2, nv2, [la, lb], lb) == (1, None, None)
    assert reference(clauses2, nv2, [lb, la], lb) == (0, 0, None)
    runs = [(clauses, nv, lemmas, target) for lemmas, target in
            [([ly, lw], lw), ([lw, ly], lw), ([ly, lw_short], lw), ([ly], lw), ([ly], lw_short)]]
    runs += [(clauses2, nv2, lemmas, target) for lemmas, target in [([la, lb], lb), ([lb, la], lb), ([la], lb), ([], lb)]]
    clauses3, nv3, lt, bad, good = long_case_true_literal_late(n)
    assert reference(clauses3, nv3, [lt, bad, good], lt) == (0, 1, None)
    assert reference(clauses3, nv3, [lt, good, lt], good) == (1, None, None)
    runs += [(clauses3, nv3, [lt, bad, good], lt), (clauses3, nv3, [lt, good, lt], good), (clauses3, nv3, [lt, lt, bad], bad)]
    for cl, v, lemmas, target in runs:
        want = reference(cl, v, lemmas, target)
        for segments in (1, 2, 3):
            info = check(make_solver, cl, v, flat(lemmas), target, segments=segments, **opts)
            assert answer(info) == want, (n, lemmas, segments, info, want)


# ---- 3. / 4. the oracle's proofs of the fuzz cases, and their mutants -----------------------------------------------------------
def unsat_cases(cases):
    return {name: c for name, c in cases.items() if c[6] == 20}


_proofs = {}


def oracle_proof(case):
    """(Csr, lemmas, reference answer) of an UNSAT fuzz case, computed once: the oracle solver's own DRUP log."""
    if case not in _proofs:
        cnf, want = fc.formula(case)
        assert want == 20
        o = ora.OracleSolver()
        o.enable_proof()
        o.add_cnf(cnf.lits, cnf.offsets)
        o.reserve(cnf.n_vars)
        assert o.solve() == 20
        lemmas, _ = lemmas_of(o.proof())
        ref = reference(cnf.clauses, cnf.n_vars, lemmas)
        assert ref[0] == 1 and oracle_verdict(cnf, lemmas) == 1
        _proofs[case] = (cnf, lemmas, ref)
    return _proofs[case]


CUTS = (1, 2, 7, None)                 # segments; None = one lemma each: n_lemmas + 1


def run_cut_independence(make_solver, case, lds_val, cuts=CUTS, **opts):
    cnf, lemmas, want = oracle_proof(case)
    proof = flat(lemmas)
    for segments in (len(lemmas) + 1 if c is None else c for c in cuts):
        for chunk in (0, 1, 5):
            info = check(make_solver, cnf.clauses, cnf.n_vars, proof, segments=segments, chunk=chunk, lds_val=lds_val, **opts)
            assert answer(info) == want, (segments, chunk, info, want)
            assert info["segments"] == segments == info["workers"] and info["n_lemmas"] == len(lemmas), info
            if chunk == 1:
                assert info["launches"] > 1, info
            assert info["lemmas_checked"] <= len(lemmas) + 1 and info["propagations"] > 0, info


MUTANT_KINDS = ("drop-lemma", "drop-literal", "negate-literal", "swap-lemmas", "lemma-to-front")
MUTANTS_PER_KIND = 12


def mutants(lemmas):
    """12 mutants of each kind, from random.Random(1234); a draw that would change nothing (swapping equal lemmas, moving
    the first one to the front) is drawn again."""
    rng = random.Random(1234)
    out = []
    for kind in MUTANT_KINDS:
        made = 0
        while made < MUTANTS_PER_KIND:
            m = [list(c) for c in lemmas]
            i = rng.randrange(len(m))
            if kind == "drop-lemma":
                del m[i]
            elif kind == "drop-literal":
                del m[i][rng.randrange(len(m[i]))]
            elif kind == "negate-literal":
                k = rng.randrange(len(m[i]))
                m[i][k] = -m[i][k]
            elif kind == "swap-lemmas":
                j = rng.randrange(len(m))
                m[i], m[j] = m[j], m[i]
            else:
                m.insert(0, m.pop(i))
            if m == [list(c) for c in lemmas]:
                continue
            out.append((kind, m))
            made += 1
    return out


_mutants = {}


def judged_mutants(case):
    """[(kind, lemmas, reference answer)] of a case, computed once, with the condition that keeps the test from being
    vacuous: by the oracle alone at least one mutant is still a proof and at least a third are not."""
    if case not in _mutants:
        cnf, lemmas, _ = oracle_proof(case)
        js = []
        for kind, m in mutants(lemmas):
            # the verdict: oracle.check_rup.  Where it says no, the first failure by oracle.bcp - the walk starts at the first
            # lemma the mutation changed: the lemmas before it stand behind the same prefix as in the proof judged above
            same = next((i for i, (x, y) in enumerate(zip(m, lemmas)) if x != y), min(len(m), len(lemmas)))
            if oracle_verdict(cnf, m):
                ref = (1, None, None)
            else:
                ref = reference(cnf.clauses, cnf.n_vars, m, refuted=False, start=same)
                assert ref[0] == 0, (kind, ref)
            if len(lemmas) <= 200:
                assert ref == reference(cnf.clauses, cnf.n_vars, m, refuted=False), (kind, ref)
            js.append((kind, m, ref))
        n_invalid = sum(1 for _, _, r in js if not r[0])
        assert n_invalid < len(js) and 3 * n_invalid >= len(js), (n_invalid, len(js))
        _mutants[case] = js
    return _mutants[case]


def run_mutants(make_solver, case, kinds=MUTANT_KINDS, **opts):
    cnf, _, _ = oracle_proof(case)
    for kind, m, want in judged_mutants(case):
        if kind not in kinds:
            continue
        info = check(make_solver, cnf.clauses, cnf.n_vars, flat(m), segments=3, **opts)
        assert (info["valid"], info["first_failed"]) == want[:2], (kind, info, want)


# ---- 5. the product's own proofs ---------------------------------------------------------------------------------------------
def run_own_proof(make_solver, cnf, n_vars, proof_path, target=(), half_is_no_proof=True, **check_opts):
    """A DRUP file the product wrote for `cnf` (deletion lines and all) on a fresh handle that holds only the CNF: valid, as
    the oracle says of the stripped proof; cut to the first half of its lines: not valid, failing at the target unless the
    oracle's reference says earlier (half_is_no_proof = False: only what the oracle says of the half).  Returns the info of
    the whole proof."""
    from timberborn_support_solver_amd.dimacs import read_drup
    clauses = [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]
    lemmas, n_del = lemmas_of(read_drup(proof_path))

    def on_fresh_handle(path):
        s = make_solver(**check_opts)
        try:
            s.add_cnf(cnf.lits, cnf.offsets)
            s.reserve(n_vars)
            return s.check_proof_file(path, target=target)
        finally:
            s.close()

    info = on_fresh_handle(proof_path)
    assert info["valid"] == 1 and info["first_failed"] is None, info
    assert info["n_lemmas"] == len(lemmas) and info["n_deletions_ignored"] == n_del, info
    if not target:
        assert ora.check_rup(cnf.lits, cnf.offsets, n_vars, read_drup(proof_path, deletions=False)) == 1
    lines = open(proof_path).read().splitlines(keepends=True)
    half = str(proof_path) + ".half"
    with open(half, "w") as f:
        f.writelines(lines[:len(lines) // 2])
    half_lemmas, _ = lemmas_of(read_drup(half))
    want = reference(clauses, n_vars, half_lemmas, target, refuted=False)
    cut = on_fresh_handle(half)
    print("half of the proof:", cut, "oracle:", want)
    assert (cut["valid"], cut["first_failed"]) == want[:2], (cut, want)
    if half_is_no_proof:     # (a solve whose file is the same in every run; a free-running fleet's half may be a proof)
        assert want[0] == 0, "the oracle accepts the first half of this proof: the case does not test what it is meant to"
        assert cut["valid"] == 0
    assert cut["valid"] == 1 or cut["first_failed"] == len(half_lemmas) or want[1] < len(half_lemmas)
    return info
