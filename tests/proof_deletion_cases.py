"""Cases and judge of the proof checker and trimmer with deletion lines honoured, mi355sat_proof_deletions
(tests/test_emu_proof_deletions.py on the wavefront emulator, tests/test_gpu_proof_deletions.py on the MI355X; test
infrastructure).

The judge is never the code under test: `reference_del` restates the semantics of include/mi355sat.h over the oracle's
occurrence-list unit propagation (oracle.bcp) - close() is a bcp without decisions whose values become unit clauses - and
resolves the deletion lines itself, in plain Python.  Every case asserts first that the reference says what the case
expects."""
import numpy as np

import proof_check_cases as pc
import proof_trim_cases as pt
from oracle import oracle as ora

ERR_STATE = -3


# ---- the reference ---------------------------------------------------------------------------------------------------------
def events_of(lemmas, deletions=()):
    """Lemma lists and {item: [clauses deleted in front of it]} (pc.flat's arguments) -> [("l" | "d", literals)] in file order."""
    deletions = dict(deletions)
    out = []
    for i in range(len(lemmas) + 1):
        out += [("d", list(d)) for d in deletions.get(i, ())]
        if i < len(lemmas):
            out.append(("l", list(lemmas[i])))
    return out


def events_of_words(proof):
    """Flat proof words (dimacs.read_drup's form) -> events."""
    out, cur, kind = [], [], "l"
    for x in (int(v) for v in proof):
        if x == pc.DEL:
            kind = "d"
        elif x == 0:
            out.append((kind, cur))
            cur, kind = [], "l"
        else:
            cur.append(x)
    assert not cur and kind == "l", "unterminated proof"
    return out


def flat_events(events):
    out = []
    for kind, c in events:
        out += ([pc.DEL] if kind == "d" else []) + list(c) + [0]
    return np.asarray(out, dtype=np.int64).astype(np.int32)


def resolve(clauses, events):
    """The deletion lines resolved: (lemmas, dying, counts).  dying: {item: [lemma indices that leave Live in front of it]},
    with a key for every item that has a group in front of it; counts: the figures that are functions of the proof alone."""
    originals = {frozenset(c) for c in clauses}
    lemmas, unmatched_lines, dying = [], {}, {}
    counts = dict(honoured=0, ignored_original=0, ignored_unmatched=0, groups=0, peak_live_lemmas=0)
    n_live, prev = 0, "l"
    for kind, c in events:
        key = frozenset(c)
        if kind == "l":
            unmatched_lines.setdefault(key, []).append(len(lemmas))      # lemma lines no deletion has matched yet, latest last
            if not pt.is_tautology(c):
                n_live += 1
                counts["peak_live_lemmas"] = max(counts["peak_live_lemmas"], n_live)
            lemmas.append(list(c))
        else:
            item = len(lemmas)
            if prev == "l":
                counts["groups"] += 1
            group = dying.setdefault(item, [])
            if unmatched_lines.get(key):
                i = unmatched_lines[key].pop()
                counts["honoured"] += 1
                if not pt.is_tautology(lemmas[i]):
                    group.append(i)
                    n_live -= 1
            elif key in originals:
                counts["ignored_original"] += 1
            else:
                counts["ignored_unmatched"] += 1
        prev = kind
    return lemmas, dying, counts


def reference_del(clauses, n_vars, events, target=()):
    """((valid, first_failed, refuted_at), counts): the semantics of mi355sat_proof_deletions, item by item."""
    lemmas, dying, counts = resolve(clauses, events)
    base_lits, base_offs = ora.to_csr([list(c) for c in clauses])
    live, facts = [], set()
    first_failed = refuted_at = None

    def bcp(assumed):
        tail_lits, tail_offs = ora.to_csr([sorted(set(lemmas[i])) for i in live] + [[f] for f in sorted(facts)])
        lits = np.concatenate([base_lits, tail_lits])
        offs = np.concatenate([base_offs, tail_offs[1:] + base_offs[-1]])
        return ora.bcp(lits, offs, n_vars, assumed)

    def close():
        confl, vals, _, _ = bcp([])
        if not confl:
            facts.update((v + 1) if vals[v] > 0 else -(v + 1) for v in range(n_vars) if vals[v] != 0)
        return confl

    for j, lem in enumerate(lemmas + [list(target)]):
        if j in dying:
            if close():
                refuted_at = j
                break
            live = [i for i in live if i not in dying[j]]
        if close():
            refuted_at = j
            break
        if pt.is_tautology(lem):
            continue
        if first_failed is None and not bcp([-l for l in sorted(set(lem))])[0]:
            first_failed = j
        if j < len(lemmas):
            live.append(j)
    return ((1 if first_failed is None else 0), first_failed, refuted_at), counts


# ---- running the device -------------------------------------------------------------------------------------------------------
def switched_on(make_solver):
    """make_solver whose handles honour deletion lines (for pc.check and pt.trim, which build their own)."""
    def make(**opts):
        s = make_solver(**opts)
        s.set_proof_deletions(True)
        return s
    return make


def check_on(make_solver, clauses, n_vars, proof, target=(), segments=0, chunk=0, **opts):
    """new, add_cnf, reserve, set_proof_deletions, check_proof on a fresh handle: (info dict, debug_proof_deletions dict)."""
    s = pt.solver_with(switched_on(make_solver), clauses, n_vars, chunk=chunk, **opts)
    try:
        info = s.check_proof(proof, target=target, segments=segments)
        return info, s.debug_proof_deletions()
    finally:
        s.close()


def assert_counts(dinfo, counts, info):
    for k, v in counts.items():
        assert dinfo[k] == v, (k, dinfo, counts)
    assert info["n_deletions_ignored"] == counts["ignored_original"] + counts["ignored_unmatched"], (info, counts)


def trim_on(make_solver, clauses, n_vars, lemmas, target, dels, segments, **opts):
    """trim_proof(hints=True) with the switch on, judged by pt.judge: the oracle on core + needed lemmas alone, the LRAT file
    by tests/lrat_check.py against the caller's clauses, the DRUP file line by line."""
    res = pt.trim(switched_on(make_solver), clauses, n_vars, lemmas, target, dels=dels, segments=segments, **opts)
    assert res["check"]["valid"] == 1, res
    return res


# ---- 1. by inspection ------------------------------------------------------------------------------------------------------
THRU = [[1, 2, 3], [1, 2, -3], [-2, 4, 5], [-2, 4, -5]]        # B = (1 4) is RUP only with A = (1 2) attached
A, B = [1, 2], [1, 4]
FACT = [[1], [-1, 2, 3, 4], [-1, 2, 3, -4], [-1, 2, -3, 4], [-1, 2, -3, -4]]
M, L = [2, 3], [-1, 2]
VALID = (1, None, None)
# name: (clauses, n_vars, lemmas, deletions, target, honoured answer, answer with deletions ignored, counts to expect)
INSPECTION = {
    "deleted-before-use": (THRU, 5, [A, B], {1: [A]}, B, (0, 1, None), VALID, dict(honoured=1)),
    "deleted-after-use": (THRU, 5, [A, B], {2: [A]}, B, VALID, VALID, dict(honoured=1)),
    "target-needs-it": (THRU, 5, [A], {1: [A]}, B, (0, 1, None), VALID, dict(honoured=1)),
    "one-of-two-copies": (THRU, 5, [A, A, B], {2: [A]}, B, VALID, VALID, dict(honoured=1)),
    "both-copies": (THRU, 5, [A, A, B], {2: [A, A]}, B, (0, 2, None), VALID, dict(honoured=2)),
    "other-order-repeated-literal": (THRU, 5, [A, B], {1: [[2, 1, 2]]}, B, (0, 1, None), VALID, dict(honoured=1)),
    "unmatched": (THRU, 5, [A, B], {1: [[1, 5]]}, B, VALID, VALID, dict(honoured=0, ignored_unmatched=1)),
    "originals": (THRU, 5, [A, B], {0: [[1, 2, 3]], 1: [[-2, 4, 5]]}, B, VALID, VALID, dict(honoured=0, ignored_original=2)),
    "deleted-twice": (THRU, 5, [A, B], {2: [A, A]}, B, VALID, VALID, dict(honoured=1, ignored_unmatched=1)),
    "re-added": (THRU, 5, [A, A, B], {1: [A]}, B, VALID, VALID, dict(honoured=1)),
    # the fact 2 that L gives outlives L and M; a worker that reaches the target through an unchecked prefix has it only
    # because it closes at the group
    "facts-outlive": (FACT, 4, [M, L], {2: [M, L]}, (2,), VALID, VALID, dict(honoured=2)),
    "control": (FACT, 4, [M], {1: [M]}, (2,), (0, 1, None), VALID, dict(honoured=1)),
    "deletions-are-counted-and-ignored": pc.INSPECTION["deletions-are-counted-and-ignored"][:5] +
                                         ((1, None, 2), (1, None, 2), dict(honoured=1, ignored_original=2)),
}
DIFFERING = tuple(n for n, c in INSPECTION.items() if c[5] != c[6])
SEGMENTS = (0, 1, 2, 3)


def run_inspection(make_solver, name, **opts):
    clauses, n_vars, lemmas, dels, target, want, want_ignored, want_counts = INSPECTION[name]
    ref, counts = reference_del(clauses, n_vars, events_of(lemmas, dels), target)
    assert ref == want, ("the case's expectation is not the reference's", ref)
    assert pc.reference(clauses, n_vars, lemmas, target) == want_ignored
    assert {k: counts[k] for k in want_counts} == want_counts, counts
    for segments in SEGMENTS:
        info, dinfo = check_on(make_solver, clauses, n_vars, pc.flat(lemmas, dels), target, segments=segments, **opts)
        assert pc.answer(info) == want, (name, segments, info, dinfo)
        assert info["n_lemmas"] == len(lemmas) and not info["interrupted"], info
        assert_counts(dinfo, counts, info)
        if name == "facts-outlive" and segments == 1:
            assert dinfo["skipped_locked"] >= 1, dinfo         # L is what gave the fact 2
        if want[0] == 1:
            trim_on(make_solver, clauses, n_vars, lemmas, target, dels, segments, **opts)


# ---- 2. the oracle's proofs with sliding-window deletions -------------------------------------------------------------------
WINDOW_CASES = ("3sat-n40-s3", "3sat-n60-s2", "mixedw-n120-s102", "salted-3sat-n60-s203")


def windows(n):
    return ((4, 1), (16, 4), (n // 2, 8), (n - 2, 1))


def window_deletions(lemmas, W, G):
    """In front of item i lemma i - W is due for deletion; the lines are flushed in groups of G."""
    dels, due = {}, []
    for i in range(W, len(lemmas) + 1):
        due.append(lemmas[i - W])
        if len(due) == G:
            dels[i], due = due, []
    return dels


_windows = {}


def judged_windows(cases):
    """{(name, window index): (cnf, lemmas, dels, reference answer, counts)} computed once, with the condition that keeps
    the test from being vacuous, asserted on the reference alone."""
    if not _windows:
        for name in WINDOW_CASES:
            cnf, lemmas, ignored = pc.oracle_proof(cases[name])
            assert ignored[0] == 1                         # all 16 are valid with deletions ignored
            for k, (W, G) in enumerate(windows(len(lemmas))):
                dels = window_deletions(lemmas, W, G)
                ref, counts = reference_del(cnf.clauses, cnf.n_vars, events_of(lemmas, dels), ())
                _windows[(name, k)] = (cnf, lemmas, dels, ref, counts)
        verdicts = [v[3][0] for v in _windows.values()]
        assert len(verdicts) == 16 and verdicts.count(0) >= 6 and verdicts.count(1) >= 6, verdicts
    return _windows


def run_window(make_solver, cases, name, k, lds_val, cuts=pc.CUTS, chunks=(0, 1, 5), **opts):
    cnf, lemmas, dels, want, counts = judged_windows(cases)[(name, k)]
    proof = pc.flat(lemmas, dels)
    print(name, windows(len(lemmas))[k], "reference:", want, counts)
    for segments in (len(lemmas) + 1 if c is None else c for c in cuts):
        for chunk in chunks:
            info, dinfo = check_on(make_solver, cnf.clauses, cnf.n_vars, proof, segments=segments, chunk=chunk, lds_val=lds_val, **opts)
            assert pc.answer(info) == want, (segments, chunk, info, want)
            assert info["segments"] == segments == info["workers"] and info["n_lemmas"] == len(lemmas), info
            assert_counts(dinfo, counts, info)
            assert dinfo["learnt_cap"] <= dinfo["peak_live_lemmas"] + cnf.n_vars + 1, dinfo


def run_window_trims(make_solver, cases, name, lds_val, **opts):
    """Section 4 on the windows of one case: every one the reference finds valid goes through the judged trim."""
    valid = [k for k in range(4) if judged_windows(cases)[(name, k)][3][0] == 1]
    assert valid, name
    for k in valid:
        cnf, lemmas, dels, want, counts = judged_windows(cases)[(name, k)]
        res = trim_on(make_solver, cnf.clauses, cnf.n_vars, lemmas, (), dels, 3, lds_val=lds_val, **opts)
        assert pc.answer(res["check"]) == want, (k, res, want)


# ---- 3. churn --------------------------------------------------------------------------------------------------------------
CHURN = 4000          # repetitions: with the closing A, B the proof has the 4002 lemmas the feature's issue gives
_churn = {}


def churn(last_a):
    """THRU with `A, d A` 4000 times, then (last_a) A, then B; target B: every slot reused thousands of times, a pass over the
    store at every item.  (events, reference answer, counts), computed once."""
    if last_a not in _churn:
        events = [("l", A), ("d", A)] * CHURN + ([("l", A)] if last_a else []) + [("l", B)]
        ref, counts = reference_del(THRU, 5, events, B)
        _churn[last_a] = (events, ref, counts)
    return _churn[last_a]


def run_churn(make_solver, **opts):
    for last_a, want, n_lemmas in ((True, VALID, CHURN + 2), (False, (0, CHURN, None), CHURN + 1)):
        events, ref, counts = churn(last_a)
        assert ref == want and counts["honoured"] == CHURN and counts["peak_live_lemmas"] == (2 if last_a else 1), (ref, counts)
        assert n_lemmas == sum(1 for k, _ in events if k == "l")
        for segments in (1, 3):
            info, dinfo = check_on(make_solver, THRU, 5, flat_events(events), B, segments=segments, **opts)
            assert pc.answer(info) == want and info["n_lemmas"] == n_lemmas, (segments, info)
            assert_counts(dinfo, counts, info)
            assert dinfo["learnt_cap"] <= 8, dinfo             # not sized from the 4002 lemmas
            assert dinfo["compactions"] >= CHURN, dinfo


# ---- 5. the product's own proofs -----------------------------------------------------------------------------------------------
def run_own_proof(make_solver, cnf, n_vars, proof_path, **opts):
    """A DRUP file of the product's, deletion lines and all, and its first half: the device's triple is the reference's -
    agreement is the assertion, not validity.  Returns (info, debug info) of the whole file."""
    from timberborn_support_solver_amd.dimacs import read_drup
    clauses = pt.clauses_of(cnf)
    lines = open(proof_path).read().splitlines(keepends=True)
    half = str(proof_path) + ".half"
    with open(half, "w") as f:
        f.writelines(lines[:len(lines) // 2])
    out = None
    for path in (proof_path, half):
        events = events_of_words(read_drup(path))
        want, counts = reference_del(clauses, n_vars, events, ())
        s = switched_on(make_solver)(**opts)
        try:
            s.add_cnf(cnf.lits, cnf.offsets)
            s.reserve(n_vars)
            info = s.check_proof_file(path)
            dinfo = s.debug_proof_deletions()
        finally:
            s.close()
        print(path, "device:", info, dinfo, "reference:", want, counts)
        assert pc.answer(info) == want, (path, info, want)
        assert_counts(dinfo, counts, info)
        assert dinfo["honoured"] > 0 and dinfo["peak_live_lemmas"] < info["n_lemmas"], dinfo
        out = out or (info, dinfo)
    return out


# ---- 6. contract -----------------------------------------------------------------------------------------------------------
def run_switch_off(make_solver, solver_error):
    """Off - by default, and after on and off again - is the checker as it was: the answer with deletions ignored, every
    deletion line counted, and no deletion info before the first check with the switch on."""
    import pytest
    clauses, n_vars, lemmas, dels, target, want, want_ignored, _ = INSPECTION["deleted-before-use"]
    proof = pc.flat(lemmas, dels)
    s = pt.solver_with(make_solver, clauses, n_vars)
    for toggled in (False, True):
        if toggled:
            s.set_proof_deletions(True)
            s.set_proof_deletions(False)
        info = s.check_proof(proof, target=target, segments=2)
        assert pc.answer(info) == want_ignored and info["n_deletions_ignored"] == 1, info
        res = s.trim_proof(proof, target=target, hints=True)
        assert pc.answer(res["check"]) == want_ignored and res["check"]["n_deletions_ignored"] == 1, res
        with pytest.raises(solver_error) as e:
            s.debug_proof_deletions()
        assert e.value.code == ERR_STATE
    s.set_proof_deletions(True)
    assert pc.answer(s.check_proof(proof, target=target, segments=2)) == want
    assert s.debug_proof_deletions()["honoured"] == 1
    s.set_proof_deletions(False)
    assert pc.answer(s.check_proof(proof, target=target)) == want_ignored
    assert s.debug_proof_deletions()["honoured"] == 1          # still the last check made with the switch on
    s.close()
