"""Cases and judge of the device's LRAT checker, mi355sat_check_lrat (tests/test_emu_lrat.py on the wavefront emulator,
tests/test_gpu_lrat.py on the MI355X; test infrastructure).

The judge is never the code under test: it is tests/lrat_check.py, imported as it is.  What it says in words is mapped here
to the codes of include/mi355sat.h (REASON_OF), and the line it rejects is found from the id in its message.  Every case
compares (accepted, first rejected line, reason) with the judge's; the cases written by hand also state what they expect, so
that the judge and the table check each other."""
import ctypes
import os
import random
import tempfile

import numpy as np

import lrat_check
import proof_check_cases as pc
from helpers import Csr

ERR_STATE, ERR_ARG = pc.ERR_STATE, pc.ERR_ARG
ID_ORDER, TAUTOLOGY, NO_HINTS, BAD_HINT, SATISFIED, NOT_UNIT, FALSIFIED_EARLY, LAST_NOT_FALSIFIED = range(1, 9)
# lrat_check.check's messages, in the order it raises them within a line
REASON_OF = (
    ("ids must be above the originals', unique and increasing", ID_ORDER),
    ("the clause holds a literal and its negation", TAUTOLOGY),
    ("no hints", NO_HINTS),
    ("is neither an original nor an earlier line", BAD_HINT),
    ("is satisfied at its turn", SATISFIED),
    ("free literals at its turn", NOT_UNIT),
    ("is falsified before the last hint", FALSIFIED_EARLY),
    ("is not falsified", LAST_NOT_FALSIFIED),
)
LDS_BUILDS = [1, -1]
LDS_IDS = ["lds", "hbm"]


def lrat(lines):
    return "".join(l + "\n" for l in lines)


def words(text):
    """LRAT text of integers -> the flat int32 form of mi355sat_check_lrat."""
    return np.asarray([int(t) for t in text.split()], dtype=np.int64).astype(np.int32)


def text_of(lines):
    """[(id, literals, hints)] -> LRAT text."""
    return lrat(" ".join(str(x) for x in [cid] + list(lits) + [0] + list(hints) + [0]) for cid, lits, hints in lines)


def judge(clauses, text):
    """The Python checker's verdict: (accepted, first rejected line index, reason, used caller clauses 0-based or None).
    "ARG" in place of the tuple where the text is not LRAT at all (lrat_check.parse refuses it)."""
    try:
        lines = lrat_check.parse(text)
    except lrat_check.LratError:
        return "ARG"
    try:
        used, _ = lrat_check.check(clauses, text)
        return 1, None, 0, sorted(u - 1 for u in used)
    except lrat_check.LratError as e:
        msg = str(e)
    codes = [code for part, code in REASON_OF if part in msg]
    assert len(codes) == 1 and msg.startswith("id "), msg
    cid = int(msg.split(":")[0].split()[1])
    ids = [l[0] for l in lines]
    last, order = len(clauses), len(ids)          # the first line whose id is not above its predecessor's
    for i, x in enumerate(ids):
        if x <= last:
            order = i
            break
        last = x
    if codes[0] == ID_ORDER:
        assert order < len(ids) and ids[order] == cid, (msg, ids)
        return 0, order, ID_ORDER, None
    at = ids.index(cid)
    assert at < order, (msg, ids)
    return 0, at, codes[0], None


def answer(info):
    return info["accepted"], info["first_rejected"], info["reason"]


def solver_with(make_solver, clauses, n_vars, chunk=None, **opts):
    s = make_solver(**opts)
    cnf = Csr(clauses, n_vars)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    if chunk is not None:
        s.debug_lrat_chunk(chunk)
    return s


def check(make_solver, clauses, n_vars, text, target=(), chunk=None, want_used=False, **opts):
    """new, add_cnf, reserve, check_lrat on a fresh handle: the info dict (and lrat_used() where every line was accepted)."""
    s = solver_with(make_solver, clauses, n_vars, chunk, **opts)
    try:
        info = s.check_lrat(words(text), target=target)
        assert info["lds"] == (1 if opts.get("lds_val") == 1 else 0), info
        assert info["valid"] == (1 if info["accepted"] == 1 and info["derives_target"] == 1 else 0), info
        if want_used:
            return info, (s.lrat_used() if info["accepted"] == 1 else None)
        return info
    finally:
        s.close()


def check_against_judge(make_solver, clauses, n_vars, text, target=(), expect=None, **opts):
    """One file on the device and by the judge: the same (accepted, line, reason), the same used originals; expect (may be
    None): (line, reason, hint position) or "accepted", stated by the case."""
    want = judge(clauses, text)
    assert want != "ARG", text
    info, used = check(make_solver, clauses, n_vars, text, target, want_used=True, **opts)
    assert answer(info) == want[:3], (text[:200], info, want)
    if want[0] == 1:
        assert used == want[3] and info["used_originals"] == len(used) and info["reject_hint"] is None, (info, used, want)
    else:
        assert info["used_originals"] == 0 and info["first_rejected_id"] == lrat_check.parse(text)[want[1]][0], info
        assert (info["reject_hint"] is None) == (info["reason"] < BAD_HINT), info
    if expect == "accepted":
        assert want[0] == 1, (text[:200], want)
    elif expect is not None:
        assert (info["first_rejected"], info["reason"], info["reject_hint"]) == tuple(expect), (text[:200], info, expect)
    return info


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------
# XOR2 = (1 2) (-1 2) (1 -2) (-1 -2) and its refutation, as tests/test_emu_proof_trim.py has them; for the ten variants
# that tests the Python checker with: (line index, reason, position of the offending hint)
XOR2 = pc.XOR2
XOR2_LRAT = ["5 2 0 1 2 0", "6 0 5 3 4 0"]
XOR2_REJECTED = {
    "a hint removed": (["5 2 0 1 2 0", "6 0 5 4 0"], (1, LAST_NOT_FALSIFIED, 1)),
    "the only unit hint removed": (["5 2 0 2 0", "6 0 5 3 4 0"], (0, LAST_NOT_FALSIFIED, 0)),
    "two hints swapped": (["5 2 0 1 2 0", "6 0 3 5 4 0"], (1, NOT_UNIT, 0)),
    "a hint that names a later line": (["5 2 0 1 6 0", "6 0 5 3 4 0"], (0, BAD_HINT, 1)),
    "the last line dropped, its id hinted": (["5 2 0 1 2 0", "7 0 6 3 4 0"], (1, BAD_HINT, 0)),
    "ids not increasing": (["6 2 0 1 2 0", "5 0 6 3 4 0"], (1, ID_ORDER, None)),
    "an id of an original": (["4 2 0 1 2 0"], (0, ID_ORDER, None)),
    "a satisfied hint": (["5 2 0 1 2 0", "6 0 5 5 3 4 0"], (1, SATISFIED, 1)),
    "a falsified hint before the last": (["5 2 0 1 2 0", "6 0 5 3 4 4 0"], (1, FALSIFIED_EARLY, 2)),
    "no hints": (["5 2 0 0"], (0, NO_HINTS, None)),
}


def run_xor2_accepted(make_solver, **opts):
    info, used = check(make_solver, XOR2, 2, lrat(XOR2_LRAT), want_used=True, **opts)
    assert (info["valid"], info["accepted"], info["derives_target"], info["reason"]) == (1, 1, 1, 0), info
    assert used == [0, 1, 2, 3] and info["used_originals"] == 4, (info, used)
    assert (info["n_lines"], info["n_hints"], info["longest_clause"], info["launches"]) == (2, 5, 2, 1), info
    assert info["first_rejected"] is None and info["first_rejected_id"] is None and info["reject_hint"] is None, info
    check_against_judge(make_solver, XOR2, 2, lrat(XOR2_LRAT), expect="accepted", **opts)
    # the first line alone is a valid file that derives (2), not the empty clause
    short = check(make_solver, XOR2, 2, lrat(XOR2_LRAT[:1]), **opts)
    assert (short["accepted"], short["derives_target"], short["valid"]) == (1, 0, 0), short
    assert check(make_solver, XOR2, 2, lrat(XOR2_LRAT[:1]), target=(2, 2), **opts)["valid"] == 1


def run_xor2_rejected(make_solver, name, **opts):
    lines, expect = XOR2_REJECTED[name]
    check_against_judge(make_solver, XOR2, 2, lrat(lines), expect=expect, **opts)


# ---- 2. the clause scan at its edges ---------------------------------------------------------------------------------------------
SCAN_N = (1, 63, 64, 65, 66, 128, 129, 130, 200)       # (66 and 130: the LINE's own clause then has 65 and 129 literals)


def scan_cases(n):
    """Hinted clauses of n literals, scanned 64 at a time.  C = (x1 .. xn) is clause 1; the line holds every x but the free
    ones, so under its negation C keeps exactly those.  Returns [(name, clauses, n_vars, lines, expectation)]."""
    xs = list(range(1, n + 1))
    t, y = n + 1, n + 2
    nv = n + 2
    out = []

    def without(*free):
        return [x for x in xs if x not in free]

    # the free literal first, last and on either side of a 64-literal step: C gives it, (-xp) falls
    for p in sorted({1, n, 64, 65} & set(xs)):
        out.append((f"unit-at-{p}", [xs, [-p]], nv, [(3, without(p), [1, 2])], "accepted"))
        out.append((f"unit-at-{p}-left-standing", [xs, [-p, y]], nv, [(3, without(p), [1, 2])], (0, LAST_NOT_FALSIFIED, 1)))
    if n >= 65:
        # the one free literal written twice, in two different steps: a unit all the same
        twice = [1] + xs[1:] + [1]
        out.append(("free-literal-repeated", [twice, [-1]], nv, [(3, without(1), [1, 2])], "accepted"))
        # two distinct free literals in two different steps
        out.append(("two-free-literals", [xs, [-1]], nv, [(3, without(1, n), [1, 2])], (0, NOT_UNIT, 0)))
        # the line's own clause across a step: x1 and -x1 64 literals apart
        out.append(("tautology-across-steps", [xs, [-1]], nv, [(3, [1] + without(1, 2) + [-1], [1, 2])], (0, TAUTOLOGY, None)))
    # a TRUE literal in the last position only: it wins, also over two literals left free before it
    sat = xs[:-1] + [t]
    out.append(("true-literal-last", [sat, [-1]], nv, [(3, [x for x in xs[1:-1]] + [-t], [1, 2])], (0, SATISFIED, 0)))
    if n >= 3:
        out.append(("true-literal-last-two-free-before", [sat, [-1]], nv, [(3, [x for x in xs[2:-1]] + [-t], [1, 2])], (0, SATISFIED, 0)))
    if n >= 2:
        out.append(("tautology-side-by-side", [xs, [-1]], nv, [(3, [2, -2] + without(1, 2), [1, 2])], (0, TAUTOLOGY, None)))
        out.append(("falsified-before-the-last", [xs, [-1]], nv, [(3, xs, [1, 2])], (0, FALSIFIED_EARLY, 0)))
    # an original that holds x and -x: satisfied once x is assigned, two free literals while it is not
    out.append(("x-and-not-x-assigned", [xs, [t, -t]], nv, [(3, [t], [2, 1])], (0, SATISFIED, 0)))
    out.append(("x-and-not-x-unassigned", [xs, [t, -t]], nv, [(3, [], [2, 1])], (0, NOT_UNIT, 0)))
    return out


def run_scan(make_solver, n, **opts):
    for name, clauses, nv, lines, expect in scan_cases(n):
        check_against_judge(make_solver, clauses, nv, text_of(lines), target=lines[-1][1], expect=expect, **opts)


# ---- 3. the assignment map at its edges --------------------------------------------------------------------------------------------
MAP_N = (15, 16, 17, 1023, 1024, 1025)          # (the 2-bit packing holds 16 variables per word)


def run_map_edges(make_solver, n_vars, **opts):
    """The highest variable N in the line's own clause, and as the unit a hint gives; then the same one variable lower with N
    reserved and in no clause."""
    for top, reserve in ((n_vars, n_vars), (n_vars - 1, n_vars)):
        in_line = [[top, 1], [-1, 2], [-2]]             # line (top): 1, then 2, then (-2) falls
        as_unit = [[1, top], [-top, 2], [-2]]           # line (1): top, then 2, then (-2) falls
        for clauses, lit in ((in_line, top), (as_unit, 1)):
            check_against_judge(make_solver, clauses, reserve, text_of([(4, [lit], [1, 2, 3])]), target=(lit,), expect="accepted", **opts)
            check_against_judge(make_solver, clauses, reserve, text_of([(4, [lit], [2, 1, 3])]), target=(lit,), expect=(0, NOT_UNIT, 0), **opts)
            check_against_judge(make_solver, clauses, reserve, text_of([(4, [lit, -top], [1, 2, 3])]), target=(lit,), **opts)


# ---- 4. real files: the trimmer's, and their mutants ---------------------------------------------------------------------------------
_files = {}


def trimmed_lrat(make_solver, case):
    """(Csr, LRAT text) of an UNSAT fuzz case: the oracle's proof trimmed with hints by the product on one segment, written by
    mi355sat_trim_write_lrat; made once per process and solver factory."""
    key = (make_solver, case)
    if key not in _files:
        cnf, lemmas, _ = pc.oracle_proof(case)
        s = solver_with(make_solver, cnf.clauses, cnf.n_vars)
        try:
            res = s.trim_proof(pc.flat(lemmas), segments=1, hints=True)
            assert res["check"]["valid"] == 1, res
            with tempfile.TemporaryDirectory() as d:
                s.trim_write_lrat(os.path.join(d, "t.lrat"))
                _files[key] = (cnf, open(os.path.join(d, "t.lrat")).read())
        finally:
            s.close()
    return _files[key]


def run_real_file(make_solver, case, tmp_path, **opts):
    cnf, text = trimmed_lrat(make_solver, case)
    want = judge(cnf.clauses, text)
    assert want[0] == 1, want
    lines = lrat_check.parse(text)
    path = str(tmp_path / "real.lrat")
    with open(path, "w") as f:
        f.write(text)
    s = solver_with(make_solver, cnf.clauses, cnf.n_vars, **opts)
    try:
        info = s.check_lrat_file(path)
        assert (info["accepted"], info["valid"], info["derives_target"]) == (1, 1, 1), info
        assert s.lrat_used() == want[3] and info["used_originals"] == len(want[3]), (info, want)
        assert (info["n_lines"], info["n_hints"]) == (len(lines), sum(len(h) for _, _, h in lines)), info
        assert info["longest_clause"] == max(len(c) for c in cnf.clauses + [l[1] for l in lines]), info
        assert s.check_lrat(words(text))["valid"] == 1            # (the flat form of the same file)
    finally:
        s.close()
    return info


MUTANT_KINDS = ("drop-hint", "swap-hints", "repeat-hint", "hint-to-later", "hint-to-unknown", "flip-literal", "drop-line", "lower-id")
MUTANTS_PER_KIND = 6
MUTANT_SEED = 11


def mutants(n_orig, lines, seed=MUTANT_SEED):
    """MUTANTS_PER_KIND mutants of each kind of a parsed file, from random.Random(seed): [(kind, LRAT text)].  A draw that
    cannot be made (swapping in a line of one hint, a literal of the empty clause) or changes nothing is drawn again.
    drop-hint: a random hint of a random line - and, every third draw, all hints of the line that has the fewest: the files
    the trimmer writes have no line with a single hint, so nothing else reaches "no hints".  repeat-hint: every second draw
    repeats the line's last hint.  hint-to-later: the id of the line itself or of a later one.  drop-line: a line some
    later line hints.  lower-id: an id not above the line before (the originals, for the first)."""
    rng = random.Random(seed)
    base = [(cid, list(lits), list(hints)) for cid, lits, hints in lines]
    hinted = [j for j, (cid, _, _) in enumerate(base) if any(cid in h for _, _, h in base[j + 1:])]
    out = []
    for kind in MUTANT_KINDS:
        made = 0
        while made < MUTANTS_PER_KIND:
            m = [(cid, list(lits), list(hints)) for cid, lits, hints in base]
            j = rng.randrange(len(m))
            cid, lits, hints = m[j]
            if kind == "drop-hint":
                if made % 3 == 2:
                    del min(m, key=lambda l: len(l[2]))[2][:]
                else:
                    del hints[rng.randrange(len(hints))]
            elif kind == "swap-hints":
                if len(hints) < 2:
                    continue
                k = rng.randrange(len(hints) - 1)
                hints[k], hints[k + 1] = hints[k + 1], hints[k]
            elif kind == "repeat-hint":
                k = len(hints) - 1 if made % 2 else rng.randrange(len(hints))
                hints.insert(k + 1, hints[k])
            elif kind == "hint-to-later":
                hints[rng.randrange(len(hints))] = m[rng.randrange(j, len(m))][0]
            elif kind == "hint-to-unknown":
                hints[rng.randrange(len(hints))] = m[-1][0] + 1 + rng.randrange(5)
            elif kind == "flip-literal":
                if not lits:
                    continue
                k = rng.randrange(len(lits))
                lits[k] = -lits[k]
            elif kind == "drop-line":
                del m[rng.choice(hinted)]
            else:
                m[j] = (rng.randrange(1, (m[j - 1][0] if j else n_orig) + 1), lits, hints)
            if m == base:
                continue
            out.append((kind, text_of(m)))
            made += 1
    return out


_judged = {}


def judged_mutants(make_solver, case):
    """[(kind, text, the judge's verdict)] of the case's file, judged once on the CPU - with the coverage that keeps the
    test from being hollow: every reason but the tautology occurs, and at least one mutant is still accepted."""
    key = (make_solver, case)
    if key not in _judged:
        cnf, text = trimmed_lrat(make_solver, case)
        js = [(kind, m, judge(cnf.clauses, m)) for kind, m in mutants(len(cnf.clauses), lrat_check.parse(text))]
        assert all(w != "ARG" for _, _, w in js)
        reasons = {w[2] for _, _, w in js if w[0] == 0}
        assert reasons >= {ID_ORDER, NO_HINTS, BAD_HINT, SATISFIED, NOT_UNIT, FALSIFIED_EARLY, LAST_NOT_FALSIFIED}, sorted(reasons)
        assert any(w[0] == 1 for _, _, w in js), "no mutant is still accepted"
        _judged[key] = js
    return _judged[key]


def run_mutants(make_solver, case, kind, **opts):
    cnf, _ = trimmed_lrat(make_solver, case)
    n = 0
    for k, text, want in judged_mutants(make_solver, case):
        if k != kind:
            continue
        info, used = check(make_solver, cnf.clauses, cnf.n_vars, text, want_used=True, **opts)
        assert answer(info) == want[:3] and used == want[3], (kind, info, want)
        n += 1
    assert n == MUTANTS_PER_KIND


# ---- 5. independence of the cut ------------------------------------------------------------------------------------------------------
VERDICT_FIELDS = ("valid", "accepted", "derives_target", "reason", "n_lines", "n_hints", "first_rejected", "first_rejected_id",
                  "reject_hint", "used_originals", "longest_clause", "lds", "dyn_lds_bytes")


def run_cut_independence(make_solver, case, **opts):
    """debug_lrat_chunk 1, 7 and 0 (the default) on the case's accepted file and on its first mutant that is rejected behind
    line 7: the same verdict fields, and the launches the cut implies (a rejection ends the call at its chunk)."""
    cnf, text = trimmed_lrat(make_solver, case)
    bad = next(m for _, m, w in judged_mutants(make_solver, case) if w[0] == 0 and w[1] > 7)
    for t in (text, bad):
        n = len(lrat_check.parse(t))
        want = judge(cnf.clauses, t)
        ran = n if want[0] == 1 else want[1] + 1          # lines up to and with the rejected one
        if want[0] == 0 and want[2] == ID_ORDER:
            ran -= 1                                      # (found on the host: that line is not uploaded)
        seen = []
        for chunk in (1, 7, 0):
            info = check(make_solver, cnf.clauses, cnf.n_vars, t, chunk=chunk, **opts)
            assert answer(info) == want[:3], (chunk, info, want)
            assert info["launches"] == (1 if chunk == 0 else (ran + chunk - 1) // chunk), (chunk, info, ran)
            assert 1 <= info["waves"] <= (chunk or n), info
            seen.append({k: info[k] for k in VERDICT_FIELDS})
        assert seen[0] == seen[1] == seen[2], seen


# ---- 6. the product's own certificate ----------------------------------------------------------------------------------------------
def run_own_certificate(make_solver, cnf, n_vars, proof_path, tmp_path, target=(), wrong_target=(1,), **opts):
    """solve wrote proof_path; here: trim_proof_file with hints, trim_write_lrat, check_lrat_file on a fresh handle - valid,
    judged accepted by the Python checker too, lrat_used() inside trim_core(); a wrong target: accepted, not derived."""
    clauses = [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]
    path = str(tmp_path / "own.lrat")
    s = make_solver(**opts)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    res = s.trim_proof_file(proof_path, target=target, hints=True)
    assert res["check"]["valid"] == 1, res
    s.trim_write_lrat(path)
    core = s.trim_core()
    s.close()
    want = judge(clauses, open(path).read())
    assert want[0] == 1, want
    s = make_solver(**opts)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    info = s.check_lrat_file(path, target=target)
    assert (info["valid"], info["accepted"], info["derives_target"]) == (1, 1, 1), info
    used = s.lrat_used()
    assert used == want[3] and set(used) <= set(core), (used, core)
    wrong = s.check_lrat_file(path, target=wrong_target)
    assert (wrong["valid"], wrong["accepted"], wrong["derives_target"]) == (0, 1, 0), wrong
    s.close()
    print(f"own certificate: {info['n_lines']} lines, {info['n_hints']} hints, {len(used)} of {len(core)} core clauses hinted, "
          f"{os.path.getsize(path)} bytes, {info['launches']} launches, {info['seconds']:.3f} s ({info['kernel_seconds']:.4f} s kernel)")
    return info


# ---- 7. state and ABI ------------------------------------------------------------------------------------------------------------------
# input that is not LRAT at all: (flat words, the same as text where text can say it)
MALFORMED_WORDS = {
    "the clause is not terminated": [5, 2],
    "the hints are not terminated": [5, 2, 0, 1, 2],
    "no hints section": [5, 2, 0],
    "a negative hint": [5, 2, 0, 1, -2, 0],
    "a negative id": [-5, 2, 0, 1, 2, 0],
    "a deletion marker": [5, pc.DEL, 1, 0, 0],
    "a variable the handle does not have": [5, 3, 0, 1, 2, 0],
    "a word behind the last line": [5, 2, 0, 1, 2, 0, 6],
}
MALFORMED_TEXT = {
    "not integers": "5 2 0 1 x 0\n",
    "a deletion line": "5 2 0 1 2 0\n5 d 1 0\n",
    "a zero hint": "5 2 0 1 0 2 0\n",
    "a negative hint": "5 2 0 1 -2 0\n",
    "a missing terminator": "5 2 0 1 2\n",
    "a line cut in two": "5 2 0 1\n2 0\n",
    "a variable the handle does not have": "5 -3 0 1 2 0\n",
}


def refused(solver_error, code, call):
    import pytest
    with pytest.raises(solver_error) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def run_malformed(make_solver, solver_error, tmp_path, **opts):
    s = solver_with(make_solver, XOR2, 2, **opts)
    ok = words(lrat(XOR2_LRAT))
    assert s.check_lrat(ok)["valid"] == 1 and s.lrat_used() == [0, 1, 2, 3]
    launches = s.stats()["kernel_launches"]
    for name, w in MALFORMED_WORDS.items():
        msg = refused(solver_error, ERR_ARG, lambda: s.check_lrat(np.asarray(w, dtype=np.int64).astype(np.int32)))
        assert "lrat" in msg, (name, msg)
        if name == "the clause is not terminated":
            refused(solver_error, ERR_STATE, s.lrat_used)         # a refused check is a check: the result before it is gone
            assert s.check_lrat(ok)["valid"] == 1 and s.lrat_used() == [0, 1, 2, 3]
            launches = s.stats()["kernel_launches"]
    for name, text in MALFORMED_TEXT.items():
        if "variable" not in name:
            assert judge(XOR2, text) == "ARG", name          # (the Python checker does not know the handle's variables)
        path = str(tmp_path / "bad.lrat")
        with open(path, "w") as f:
            f.write(text)
        msg = refused(solver_error, ERR_ARG, lambda: s.check_lrat_file(path))
        assert "lrat" in msg, (name, msg)
    refused(solver_error, ERR_ARG, lambda: s.check_lrat_file(str(tmp_path / "no-such-file")))
    refused(solver_error, ERR_ARG, lambda: s.check_lrat(words(lrat(XOR2_LRAT)), target=(3,)))
    refused(solver_error, ERR_ARG, lambda: s.check_lrat(words(lrat(XOR2_LRAT)), target=(1, 0)))
    assert s.stats()["kernel_launches"] == launches, "a refused input was launched"
    refused(solver_error, ERR_STATE, s.lrat_used)
    s.reserve(3)                                                # raises the handle's highest variable
    assert s.check_lrat(np.asarray([5, 3, 2, 0, 1, 2, 0], dtype=np.int32), target=(2, 3))["valid"] == 1
    s.close()


def run_state_and_abi(make_solver, solver_error, lib, tmp_path, **opts):
    ok, bad = words(lrat(XOR2_LRAT)), words(lrat(XOR2_REJECTED["a hint removed"][0]))
    s = solver_with(make_solver, XOR2, 2, **opts)
    refused(solver_error, ERR_STATE, s.lrat_used)                   # before any check
    assert s.check_lrat(bad)["accepted"] == 0
    refused(solver_error, ERR_STATE, s.lrat_used)                   # after a rejection
    assert s.check_lrat(ok)["valid"] == 1 and s.lrat_used() == [0, 1, 2, 3]
    # the sizing protocol of the C ABI, as mi355sat_trim_core's
    n = ctypes.c_uint64(99)
    assert lib.mi355sat_lrat_used(s._h, None, 0, ctypes.byref(n)) == 0 and n.value == 4
    buf = (ctypes.c_uint64 * 4)()
    assert lib.mi355sat_lrat_used(s._h, buf, 3, ctypes.byref(n)) == ERR_ARG and n.value == 4
    assert lib.mi355sat_lrat_used(s._h, buf, 4, None) == 0 and list(buf) == [0, 1, 2, 3]
    lib.mi355sat_abi_sizes.restype = ctypes.c_uint64
    st = ctypes.c_uint64(0)
    assert (lib.mi355sat_abi_sizes(ctypes.byref(st)), st.value) == (128, 248)
    from timberborn_support_solver_amd.solver import Mi355SatLratInfo
    assert ctypes.sizeof(Mi355SatLratInfo) == 112
    assert lib.mi355sat_check_lrat(s._h, None, 0, None, 0, None) == ERR_ARG
    # a pending interrupt: no verdict, nothing launched, consumed, no result
    launches = s.stats()["kernel_launches"]
    s.interrupter().interrupt()
    stopped = s.check_lrat(ok)
    assert stopped["interrupted"] and (stopped["accepted"], stopped["valid"], stopped["launches"]) == (-1, 0, 0), stopped
    assert s.stats()["kernel_launches"] == launches
    refused(solver_error, ERR_STATE, s.lrat_used)
    assert s.check_lrat(ok)["valid"] == 1 and s.lrat_used() == [0, 1, 2, 3]
    # ... also where the file needs no launch: an empty one, a first line whose id is an original's
    for text in ("", "4 2 0 1 2 0\n"):
        s.interrupter().interrupt()
        stopped = s.check_lrat(words(text))
        assert stopped["interrupted"] and (stopped["accepted"], stopped["valid"], stopped["launches"]) == (-1, 0, 0), (text, stopped)
        again = s.check_lrat(words(text))                             # consumed
        assert (again["accepted"], again["reason"], again["launches"]) == ((0, ID_ORDER, 0) if text else (1, 0, 0)), (text, again)
    assert s.check_lrat(ok)["valid"] == 1 and s.lrat_used() == [0, 1, 2, 3]
    # a refusal writes the info all the same: nothing accepted, nothing rejected
    info = Mi355SatLratInfo(valid=7, accepted=7, reason=7, first_rejected=7, n_lines=7)
    cut = (ctypes.c_int32 * 2)(5, 2)
    assert lib.mi355sat_check_lrat(s._h, cut, 2, None, 0, ctypes.byref(info)) == ERR_ARG
    assert (info.valid, info.accepted, info.reason, info.n_lines, info.first_rejected) == (0, 0, 0, 0, 2 ** 64 - 1)
    refused(solver_error, ERR_STATE, s.lrat_used)
    assert s.check_lrat(ok)["valid"] == 1
    # a clause added: the indices mean something else
    s.add_clause([1, 2])
    refused(solver_error, ERR_STATE, s.lrat_used)
    assert s.check_lrat(words(lrat(["6 2 0 1 2 0", "7 0 6 3 4 0"])))["valid"] == 1
    # during a sweep: MI355SAT_ERR_STATE; afterwards as before
    s.sweep_begin([[1], [-1]])
    refused(solver_error, ERR_STATE, lambda: s.check_lrat(ok))
    s.sweep_end()
    assert s.check_lrat(words(lrat(["6 2 0 1 2 0", "7 0 6 3 4 0"])))["valid"] == 1
    s.close()


def run_leaves_the_handle_alone(make_solver, result_enum, tmp_path, **opts):
    """What the call must not touch: the IPASIR state, a trim result, the answer counters - and what is resident for a warm
    incremental solve."""
    sat = Csr(pc.OPEN, 4)                       # (1 2) (-1 2) (3 4): implies 2
    line = lrat(["4 2 0 1 2 0"])                # under -2: (1 2) gives 1, (-1 2) falls
    s = make_solver(workers=2, **opts)
    s.add_cnf(sat.lits, sat.offsets)
    assert s.solve([-2]) == result_enum.Unsat and s.core() == [-2]
    res = s.trim_proof(pc.flat([[2]]), target=(2,), hints=True)
    assert res["check"]["valid"] == 1 and res["core"] == [0, 1], res
    path = str(tmp_path / "t.lrat")
    s.trim_write_lrat(path)
    before = s.stats()
    info = s.check_lrat_file(path, target=(2,))
    assert info["valid"] == 1 and s.lrat_used() == [0, 1], info
    after = s.stats()
    assert s.trim_core() == [0, 1] and s.trim_lemmas() == [0]          # trim, check_lrat_file, trim_core
    assert s.core() == [-2] and s.failed(-2)
    assert [after[k] for k in ("n_sat", "n_unsat", "n_terminated")] == [before[k] for k in ("n_sat", "n_unsat", "n_terminated")]
    assert after["kernel_launches"] == before["kernel_launches"] + info["launches"] and info["launches"] == 1
    assert after["solve_seconds"] > before["solve_seconds"] and after["kernel_seconds"] >= before["kernel_seconds"] + info["kernel_seconds"] - 1e-9
    s.close()
    # warm: solve, check_lrat, solve - the second solve starts warm
    s = make_solver(workers=2, **opts)
    s.set_incremental(True)
    s.add_cnf(sat.lits, sat.offsets)
    assert s.solve([-2]) == result_enum.Unsat
    inc = s.debug_incremental()
    assert s.check_lrat(words(line), target=(2,))["valid"] == 1
    assert s.core() == [-2]
    assert s.solve([-2]) == result_enum.Unsat
    now = s.debug_incremental()
    assert now["warm_solves"] == inc["warm_solves"] + 1 and now["cold_solves"] == inc["cold_solves"], (inc, now)
    assert now["last_cold_reason"] == inc["last_cold_reason"], (inc, now)
    s.close()
