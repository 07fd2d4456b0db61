"""Cases and judges of mi355sat_trim_proof (tests/test_emu_proof_trim.py on the wavefront emulator, tests/test_gpu_proof_trim.py
on the MI355X; test infrastructure).

The judge is never the code under test.  There are two:
  (a) the oracle, as in proof_check_cases.py: reference() - oracle.bcp lemma by lemma - and oracle.check_rup, applied to the
      core clauses ALONE as the formula and the needed lemmas ALONE as the proof.  That proves the core UNSAT (or that it
      implies the target) and the trimmed proof a proof of it;
  (b) tests/lrat_check.py, a strict LRAT checker in plain Python, on the file mi355sat_trim_write_lrat wrote against the
      caller's formula; the originals it uses must lie in the core.
Which clauses end up in a core may differ with the cut and from run to run (unit propagation picks among equal reasons):
nothing here compares cores between cuts.  Exact sets are asserted only where the oracle shows them forced."""
import os
import tempfile

import lrat_check
import proof_check_cases as pc
from helpers import Csr

ERR_STATE, ERR_ARG = pc.ERR_STATE, pc.ERR_ARG
SEGMENTS = (0, 1, 2, 3)


def solver_with(make_solver, clauses, n_vars, chunk=0, log_words=None, **opts):
    s = make_solver(**opts)
    cnf = Csr(clauses, n_vars)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    if chunk:
        s.debug_proof_check_chunk(chunk)
    if log_words is not None:
        s.debug_trim_log(log_words)
    return s


def read_drup_text(path):
    """A DRUP text file without deletion lines -> lemma lists."""
    out = []
    for line in open(path):
        tok = line.split()
        if tok:
            assert tok[-1] == "0" and tok[0] != "d", line
            out.append([int(t) for t in tok[:-1]])
    return out


def getters_refuse(s, solver_error):
    """All four getters answer MI355SAT_ERR_STATE and no file is written."""
    import pytest
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "none")
        for call in (s.trim_core, s.trim_lemmas, lambda: s.trim_write_drup(path), lambda: s.trim_write_lrat(path)):
            with pytest.raises(solver_error) as e:
                call()
            assert e.value.code == ERR_STATE
        assert not os.path.exists(path)


def is_tautology(clause):
    return any(-l in clause for l in clause)


def judge(clauses, n_vars, lemmas, target, res, lrat_text, drup_lemmas):
    """Judges (a) and (b) on one valid answer.  res: trim_proof's dict; lrat_text / drup_lemmas: what the two writers wrote."""
    core, needed = res["core"], res["lemmas"]
    target = list(target)
    assert core == sorted(set(core)) and all(0 <= i < len(clauses) for i in core), core
    assert needed == sorted(set(needed)) and all(0 <= j < len(lemmas) for j in needed), needed
    assert res["core_clauses"] == len(core) and res["lemmas_needed"] == len(needed), res
    # (a) the core alone, the needed lemmas alone
    core_clauses = [clauses[i] for i in core]
    proof = [lemmas[j] for j in needed]
    assert pc.reference(core_clauses, n_vars, proof, target)[0] == 1, ("the oracle rejects the trimmed proof", core, needed)
    if not target:
        assert pc.oracle_verdict(Csr(core_clauses, n_vars), proof) == 1, ("oracle.check_rup rejects the trimmed proof", core, needed)
    # the DRUP file: exactly the needed lemmas, then the target
    assert drup_lemmas == proof + [target], (drup_lemmas, proof, target)
    # (b) the LRAT file against the caller's formula
    used, lines = lrat_check.check(clauses, lrat_text)
    assert used <= {i + 1 for i in core}, (sorted(used), core)
    n = len(clauses)
    if is_tautology(target):
        assert not lines and not core and not needed, (lines, core, needed)
    else:
        assert [cid for cid, _, _ in lines] == [n + 1 + j for j in needed] + [n + 1 + len(lemmas)], lines
        assert [lits for _, lits, _ in lines] == proof + [target], lines


def trim(make_solver, clauses, n_vars, lemmas, target=(), dels=(), segments=0, judged=True, **opts):
    """new, add_cnf, reserve, trim_proof with the hints on a fresh handle; where the verdict is valid, both files are written
    and (judged) the judges applied.  Returns trim_proof's dict."""
    s = solver_with(make_solver, clauses, n_vars, **opts)
    try:
        res = s.trim_proof(pc.flat(lemmas, dels), target=target, segments=segments, hints=True)
        if res["check"]["valid"] == 1 and judged:
            with tempfile.TemporaryDirectory() as d:
                s.trim_write_lrat(os.path.join(d, "t.lrat"))
                s.trim_write_drup(os.path.join(d, "t.drup"))
                judge(clauses, n_vars, lemmas, target, res, open(os.path.join(d, "t.lrat")).read(),
                      read_drup_text(os.path.join(d, "t.drup")))
        return res
    finally:
        s.close()


# ---- 1. by inspection --------------------------------------------------------------------------------------------------------
CASE_A = (pc.CHAIN + [[8, 9]], 9, [[2], [8, 9, 2], [3], [6], [7, -6]], ())
B_FORMULA = [[1, 2], [-1, 2], [-2, 3, 4, 5], [-2, 3, 4, -5], [-4, 6, 7], [-4, 6, -7], [9, 10]]
B_LEMMAS = [[2], [2, 9], [-2, 3, 4]]
B_TARGET = (3, 6)
INHERITED_VALID = ("empty-proof-contradictory-units", "empty-proof-propagation-refutes", "target-rup",
                   "tautological-target-without-refutation", "deletions-are-counted-and-ignored")
INHERITED_INVALID = ("first-lemma-not-rup", "target-not-rup", "empty-proof-satisfiable")


def assert_case_a_by_the_oracle():
    clauses, nv, lemmas, target = CASE_A
    assert pc.reference(clauses, nv, lemmas, target) == (1, None, 3)
    for drop in range(6):       # the core is forced: without any one of the six the oracle rejects [[2], [3]]
        rest = [c for i, c in enumerate(clauses[:6]) if i != drop]
        assert pc.reference(rest, nv, [[2], [3]], ())[0] == 0, drop


def assert_case_b_by_the_oracle():
    assert pc.reference(B_FORMULA, 10, B_LEMMAS, B_TARGET) == (1, None, None)
    assert pc.reference(B_FORMULA, 10, B_LEMMAS[:2], B_TARGET) == (0, 2, None)
    assert pc.reference(B_FORMULA, 10, [[-2, 3, 4], [2]], B_TARGET) == (1, None, None)
    for drop, failed in enumerate((0, 0, 1, 1, 2, 2)):
        rest = [c for i, c in enumerate(B_FORMULA[:6]) if i != drop]
        assert pc.reference(rest, 10, [[2], [-2, 3, 4]], B_TARGET, refuted=False)[:2] == (0, failed), drop


def run_case_a(make_solver, **opts):
    assert_case_a_by_the_oracle()
    clauses, nv, lemmas, target = CASE_A
    for segments in SEGMENTS:
        res = trim(make_solver, clauses, nv, lemmas, target, segments=segments, **opts)
        assert pc.answer(res["check"]) == (1, None, 3), res
        assert res["lemmas"] == [0, 2] and res["core"] == [0, 1, 2, 3, 4, 5], (segments, res)


def target_hints(make_solver, clauses, n_vars, lemmas, target, segments, **opts):
    s = solver_with(make_solver, clauses, n_vars, **opts)
    try:
        assert s.trim_proof(pc.flat(lemmas), target=target, segments=segments, hints=True)["check"]["valid"] == 1
        with tempfile.TemporaryDirectory() as d:
            s.trim_write_lrat(os.path.join(d, "t.lrat"))
            return lrat_check.parse(open(os.path.join(d, "t.lrat")).read())[-1][2]
    finally:
        s.close()


def run_case_b(make_solver, **opts):
    """The stripped-literal case: (-2 3 4) is attached as (3 4) once 2 is a fact, and the derivation of 2 belongs to the cone
    of everything (3 4) implies.  A walk that expands the store's copy of the lemma loses it: judge (b) rejects the file."""
    assert_case_b_by_the_oracle()
    n = len(B_FORMULA)
    for lemmas, unit, tern in ((B_LEMMAS, 0, 2), ([[-2, 3, 4], [2]], 1, 0)):
        for segments in SEGMENTS:
            res = trim(make_solver, B_FORMULA, 10, lemmas, B_TARGET, segments=segments, **opts)
            assert pc.answer(res["check"]) == (1, None, None), res
            assert res["lemmas"] == sorted((unit, tern)) and res["core"] == [0, 1, 2, 3, 4, 5], (lemmas, segments, res)
            hints = target_hints(make_solver, B_FORMULA, 10, lemmas, B_TARGET, segments, **opts)
            assert hints.index(n + 1 + unit) < hints.index(n + 1 + tern), hints


def run_inherited_valid(make_solver, name, **opts):
    clauses, n_vars, lemmas, dels, target, want = pc.INSPECTION[name]
    assert pc.reference(clauses, n_vars, lemmas, target) == want and want[0] == 1
    for segments in SEGMENTS:
        res = trim(make_solver, clauses, n_vars, lemmas, target, dels=dels, segments=segments, **opts)
        assert pc.answer(res["check"]) == want, (name, segments, res)
        assert res["check"]["n_deletions_ignored"] == sum(len(d) for d in dels.values())


def run_inherited_invalid(make_solver, solver_error, name, **opts):
    clauses, n_vars, lemmas, dels, target, want = pc.INSPECTION[name]
    assert pc.reference(clauses, n_vars, lemmas, target) == want and want[0] == 0
    for segments in SEGMENTS:
        s = solver_with(make_solver, clauses, n_vars, **opts)
        res = s.trim_proof(pc.flat(lemmas, dels), target=target, segments=segments, hints=True)
        assert pc.answer(res["check"]) == want, (name, segments, res)
        assert res["core"] is None and res["lemmas"] is None and res["core_clauses"] == res["lemmas_needed"] == 0, res
        getters_refuse(s, solver_error)
        s.close()


# ---- 2. long reasons -----------------------------------------------------------------------------------------------------------
LONG_N = (63, 64, 65, 129)


def run_long(make_solver, n, **opts):
    """A, n literals, is RUP only from clauses 0 and 1; B only from A and clauses 2 and 3: the wave-wide marking loop on
    reasons of more than 8 and more than 64 literals, originals and a lemma."""
    clauses, nv, la, lb = pc.long_case_through_the_lemma(n)
    assert pc.reference(clauses, nv, [la, lb], lb) == (1, None, None)
    assert pc.reference(clauses, nv, [lb, la], lb)[0] == 0                      # B needs A ...
    for drop in range(4):                                                       # ... and the pair needs every clause
        rest = [c for i, c in enumerate(clauses) if i != drop]
        assert pc.reference(rest, nv, [la, lb], lb)[0] == 0, drop
    for segments in (1, 2):
        res = trim(make_solver, clauses, nv, [la, lb], lb, segments=segments, **opts)
        assert pc.answer(res["check"]) == (1, None, None), res
        assert res["core"] == [0, 1, 2, 3], (n, segments, res)
        assert 0 in res["lemmas"], (n, segments, res)       # (lemma 1 IS the target: needed or not, both are proofs)


# ---- 3. the oracle's proofs of the UNSAT fuzz cases, padded -------------------------------------------------------------------------
_padded = {}


def padded_proof(case):
    """(clauses, n_vars, lemmas, reference answer, indices of the padded clauses, indices of the padded lemmas): the oracle's
    proof of an UNSAT fuzz case with three clauses and two lemmas over four fresh variables - RUP, useless, and out of every
    cone's reach: the condition that keeps 'a subset came back' from being vacuous."""
    if case not in _padded:
        cnf, lemmas, _ = pc.oracle_proof(case)
        nv = cnf.n_vars
        clauses = [list(c) for c in cnf.clauses] + [[nv + 1, nv + 2], [-(nv + 1), nv + 2], [nv + 3, nv + 4]]
        mid = 1 + len(lemmas) // 2
        lem = [[nv + 2]] + [list(c) for c in lemmas]
        lem.insert(mid, [nv + 2, nv + 3])
        ref = pc.reference(clauses, nv + 4, lem)
        assert ref[0] == 1 and pc.oracle_verdict(Csr(clauses, nv + 4), lem) == 1
        _padded[case] = (clauses, nv + 4, lem, ref, list(range(len(cnf.clauses), len(clauses))), [0, mid])
    return _padded[case]


def comparable(info):
    """A check's dict without times and launch counts."""
    return {k: v for k, v in info.items() if k not in ("seconds", "kernel_seconds", "launches")}


def run_padded(make_solver, case, lds_val, cuts=pc.CUTS, **opts):
    clauses, nv, lemmas, want, pad_clauses, pad_lemmas = padded_proof(case)
    for segments in (len(lemmas) + 1 if c is None else c for c in cuts):
        res = trim(make_solver, clauses, nv, lemmas, segments=segments, lds_val=lds_val, **opts)
        plain = pc.check(make_solver, clauses, nv, pc.flat(lemmas), segments=segments, lds_val=lds_val,
                         **{k: v for k, v in opts.items() if k != "log_words"})
        assert comparable(res["check"]) == comparable(plain), (segments, res["check"], plain)
        assert pc.answer(res["check"]) == want, (segments, res, want)
        assert not set(pad_clauses) & set(res["core"]), (segments, res["core"])
        assert not set(pad_lemmas) & set(res["lemmas"]), (segments, res["lemmas"])
        print(f"segments {segments}: {len(res['lemmas'])} of {len(lemmas)} lemmas needed, {len(res['core'])} of {len(clauses)} "
              f"clauses in the core, {res['dep_records']} records, {res['log_drains']} drains")
    return res


# ---- 4. the log at its edges -------------------------------------------------------------------------------------------------------
def run_log_edges(make_solver, case, lds_val, **opts):
    """The smallest log the clamp allows (two items of the largest size) and one lemma per launch: a drain after every launch;
    then the default rule.  After a drain the verdict and the judges must hold - nothing about equality of sets."""
    clauses, nv, lemmas, want, pad_clauses, pad_lemmas = padded_proof(case)
    small = trim(make_solver, clauses, nv, lemmas, segments=3, chunk=1, log_words=1, lds_val=lds_val, **opts)
    assert pc.answer(small["check"]) == want, small
    assert small["log_words_per_worker"] == 8 * (nv + 3), small        # the clamp's minimum
    assert small["log_drains"] > 1 and small["check"]["launches"] > 1, small
    tight = trim(make_solver, clauses, nv, lemmas, segments=2, log_words=1, lds_val=lds_val, **opts)     # the log ends the launches
    assert pc.answer(tight["check"]) == want and tight["log_drains"] > 1 and tight["check"]["launches"] > 1, tight
    rule = trim(make_solver, clauses, nv, lemmas, segments=3, lds_val=lds_val, **opts)
    assert pc.answer(rule["check"]) == want and rule["log_words_per_worker"] > small["log_words_per_worker"], rule
    for res in (small, tight, rule):
        assert not set(pad_clauses) & set(res["core"]) and not set(pad_lemmas) & set(res["lemmas"]), res


# ---- 5. mutants ----------------------------------------------------------------------------------------------------------------
def run_mutants(make_solver, solver_error, case, kinds=pc.MUTANT_KINDS, **opts):
    """The 60 judged mutants of a case (12 of each kind; by the oracle at least a third are no proofs and at least one is)."""
    cnf, _, _ = pc.oracle_proof(case)
    for kind, m, want in pc.judged_mutants(case):
        if kind not in kinds:
            continue
        s = solver_with(make_solver, cnf.clauses, cnf.n_vars, **opts)
        res = s.trim_proof(pc.flat(m), segments=3, hints=True)
        assert (res["check"]["valid"], res["check"]["first_failed"]) == want[:2], (kind, res, want)
        if want[0]:
            with tempfile.TemporaryDirectory() as d:
                s.trim_write_lrat(os.path.join(d, "t.lrat"))
                s.trim_write_drup(os.path.join(d, "t.drup"))
                judge(cnf.clauses, cnf.n_vars, m, (), res, open(os.path.join(d, "t.lrat")).read(),
                      read_drup_text(os.path.join(d, "t.drup")))
        else:
            getters_refuse(s, solver_error)
        s.close()


# ---- 6. the product's own proofs and the round trip -----------------------------------------------------------------------------------
def clauses_of(cnf):
    return [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]


def run_own_proof(make_solver, cnf, n_vars, proof_path, tmp_path, target=(), round_trip=True, **opts):
    """trim_proof_file of a DRUP file the product wrote, judges (a) and (b); round trip: a fresh handle that holds only the core
    clauses, in order, finds the trimmed DRUP file valid.  Returns trim_proof_file's dict."""
    from timberborn_support_solver_amd.dimacs import read_drup
    clauses = clauses_of(cnf)
    lemmas, n_del = pc.lemmas_of(read_drup(proof_path))
    s = make_solver(**opts)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    res = s.trim_proof_file(proof_path, target=target, hints=True)
    assert res["check"]["valid"] == 1 and res["check"]["n_lemmas"] == len(lemmas) and res["check"]["n_deletions_ignored"] == n_del, res
    lrat, drup = str(tmp_path / "own.lrat"), str(tmp_path / "own.trimmed.drup")
    s.trim_write_lrat(lrat)
    s.trim_write_drup(drup)
    s.close()
    judge(clauses, n_vars, lemmas, target, res, open(lrat).read(), read_drup_text(drup))
    print(f"own proof: {len(res['lemmas'])} of {len(lemmas)} lemmas needed, {len(res['core'])} of {len(clauses)} clauses in the "
          f"core, LRAT file {os.path.getsize(lrat)} bytes")
    if round_trip:
        core = Csr([clauses[i] for i in res["core"]], n_vars)
        s = make_solver(**opts)
        s.add_cnf(core.lits, core.offsets)
        s.reserve(n_vars)
        lines = open(drup).read().splitlines(keepends=True)
        assert [int(t) for t in lines[-1].split()[:-1]] == list(target)
        with open(drup, "w") as f:            # (the target is the call's argument, not a lemma of the file)
            f.writelines(lines[:-1])
        back = s.check_proof_file(drup, target=target)
        s.close()
        assert back["valid"] == 1 and back["n_lemmas"] == len(res["lemmas"]), back
    return res


# ---- 7. state and ABI ----------------------------------------------------------------------------------------------------------
def run_state_and_abi(make_solver, solver_error, lib):
    import ctypes
    import pytest
    clauses, nv, lemmas, target = CASE_A
    proof = pc.flat(lemmas)
    s = solver_with(make_solver, clauses, nv)
    getters_refuse(s, solver_error)                                   # before any trim
    res = s.trim_proof(proof, hints=False)
    assert res["check"]["valid"] == 1 and res["core"] == [0, 1, 2, 3, 4, 5]
    with tempfile.TemporaryDirectory() as d:
        with pytest.raises(solver_error) as e:                        # no hints were kept
            s.trim_write_lrat(os.path.join(d, "t.lrat"))
        assert e.value.code == ERR_STATE and not os.path.exists(os.path.join(d, "t.lrat"))
        s.trim_write_drup(os.path.join(d, "t.drup"))
        assert read_drup_text(os.path.join(d, "t.drup")) == [[2], [3], []]
    # the sizing protocol of the C ABI
    n = ctypes.c_uint64(99)
    assert lib.mi355sat_trim_core(s._h, None, 0, ctypes.byref(n)) == 0 and n.value == 6
    buf = (ctypes.c_uint64 * 6)()
    assert lib.mi355sat_trim_core(s._h, buf, 5, ctypes.byref(n)) == ERR_ARG and n.value == 6
    assert lib.mi355sat_trim_core(s._h, buf, 6, ctypes.byref(n)) == 0 and list(buf) == [0, 1, 2, 3, 4, 5]
    assert lib.mi355sat_trim_lemmas(s._h, None, 0, ctypes.byref(n)) == 0 and n.value == 2
    assert lib.mi355sat_trim_lemmas(s._h, buf, 1, ctypes.byref(n)) == ERR_ARG
    assert lib.mi355sat_trim_lemmas(s._h, buf, 2, None) == 0 and list(buf)[:2] == [0, 2]
    # check_proof drops the result; so does a clause added
    assert s.check_proof(proof)["valid"] == 1
    getters_refuse(s, solver_error)
    assert s.trim_proof(proof)["lemmas"] == [0, 2]
    s.add_clause([8, -9])
    getters_refuse(s, solver_error)
    assert s.trim_proof(proof)["lemmas"] == [0, 2] and s.trim_core() == [0, 1, 2, 3, 4, 5]
    # an interrupt that came before the call: no verdict, nothing launched, consumed, no result
    s.interrupter().interrupt()
    stopped = s.trim_proof(proof, hints=True)
    assert stopped["check"]["interrupted"] and stopped["check"]["valid"] == -1 and stopped["check"]["launches"] == 0, stopped
    assert stopped["core"] is None
    getters_refuse(s, solver_error)
    assert s.trim_proof(proof)["check"]["valid"] == 1
    # during a sweep: MI355SAT_ERR_STATE; beginning one drops the result
    s.sweep_begin([[1], [-1]])
    with pytest.raises(solver_error) as e:
        s.trim_proof(proof)
    assert e.value.code == ERR_STATE
    getters_refuse(s, solver_error)
    s.sweep_end()
    assert s.trim_proof(proof)["check"]["valid"] == 1
    # argument errors, as check_proof's
    for bad, tg in [([10, 0], ()), ([1, 2], ()), ([1, pc.DEL, 2, 0], ()), ([1, 0], (1, 0, 2)), ([1, 0], (10,))]:
        with pytest.raises(solver_error) as e:
            s.trim_proof(bad, target=tg)
        assert e.value.code == ERR_ARG, (bad, tg)
    from timberborn_support_solver_amd.solver import Mi355SatTrimInfo
    info = Mi355SatTrimInfo()
    assert lib.mi355sat_trim_proof(s._h, None, 0, None, 0, 0, 2, info) == ERR_ARG        # an unknown flag
    s.close()


def run_device_takeover(make_solver, result_enum, cold_reason):
    """What check_proof leaves alone, trim_proof leaves alone: the IPASIR state of the solve before, the counters of answers."""
    sat = Csr(pc.OPEN, 4)
    s = make_solver(workers=2)
    s.set_incremental(True)
    s.add_cnf(sat.lits, sat.offsets)
    assert s.solve([-2]) == result_enum.Unsat
    core = s.core()
    assert core == [-2]
    assert s.solve([-2]) == result_enum.Unsat and s.debug_incremental()["warm_solves"] == 1
    before = s.stats()
    res = s.trim_proof(pc.flat([[2]]), target=(2,), hints=True)
    assert pc.answer(res["check"]) == (1, None, None) and res["lemmas"] == [0] and res["core"] == [0, 1], res
    after = s.stats()
    assert s.core() == core and s.failed(-2)
    assert [after[k] for k in ("n_sat", "n_unsat", "n_terminated")] == [before[k] for k in ("n_sat", "n_unsat", "n_terminated")]
    assert after["kernel_launches"] == before["kernel_launches"] + res["check"]["launches"] and res["check"]["launches"] >= 1
    assert after["solve_seconds"] > before["solve_seconds"]
    cold = s.debug_incremental()["cold_solves"]
    assert s.solve() == result_enum.Sat
    inc = s.debug_incremental()
    assert inc["cold_solves"] == cold + 1 and inc["last_cold_reason"] == cold_reason.OTHER_SEARCH
    assert s.trim_core() == [0, 1]                         # a solve is none of the calls that drop the result
    s.close()
