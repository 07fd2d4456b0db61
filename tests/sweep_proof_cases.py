"""Cases and judges for the DRUP proofs of batches and sweeps and for the check of several targets in one pass
(tests/test_emu_sweep_proof.py on the wavefront emulator, tests/test_gpu_sweep_proof.py on the MI355X; test infrastructure).

The judge is the oracle, never the product.  A batch's file is judged whole by oracle.check_rup - for an UNSAT instance
against the clauses plus the instance's core literals as unit clauses (the core line then refutes the database), for a
refuted formula against the clauses alone - and target by target by the oracle's unit propagation (target_reference, which
is proof_check_cases.reference's database and its rule applied to one more clause).  The formulas, the assumption lists and
their verdicts are sweep_cases' tables."""
import numpy as np

import proof_check_cases as pc
import sweep_cases as sc
from helpers import Csr
from oracle import oracle as ora
from timberborn_support_solver_amd.dimacs import read_drup

BATCH_CASES = ("3sat-n50-s5", "3sat-n50-s17", "all-n110-s8-simp0", "all-n110-s8-simp2", "long-n150-s20")
SCHEDULE_CASE = "3sat-n50-s5"
SCHEDULE_SEEDS = (1, 2, 3)

# The gather kernel's edges (rect 8x8 1x1, k = 3, three workers, reduce_first = 25, reduce_inc = 10, deterministic = 1,
# slice_conflicts = 16).  PROOF_CAP_TIGHT was found on the CPU by halving from the rule's value (2^20 + ...) for as long as
# the solve went through: 512 does, 256 ends with "proof buffer overflow" - the largest slice log of that run needs between
# the two.  It leaves no room for all deletion lines of a reduction: some are dropped, which a proof may always do.
GATHER_OPTS = dict(workers=3, slice_conflicts=16, reduce_first=25, reduce_inc=10, deterministic=1)
PROOF_CAP_TIGHT = 512
PROOF_CAP_TOO_SMALL = 8


def batch_options(name, **more):
    opts = sc.options(name, "default", **more)
    if name == sc.VAR_ORDER_CASE:
        opts["var_order"] = 1
    return opts


def negated(core):
    return [-l for l in core]


def is_tautology(clause):
    return any(-l in clause for l in clause)


def lines_of(path):
    """The lemma lines of a DRUP file as sorted literal tuples (deletion lines left out)."""
    lemmas, _ = pc.lemmas_of(read_drup(path))
    return [tuple(sorted(set(c))) for c in lemmas]


def target_reference(clauses, n_vars, lemmas, target):
    """The oracle's verdict on one target behind ALL lemmas: 1 if it holds a literal and its negation, if unit propagation
    alone refutes clauses + lemmas, or if it does under the negated target; else 0."""
    if is_tautology(list(target)):
        return 1
    db = ora.to_csr([list(c) for c in clauses] + [list(c) for c in lemmas])
    if ora.bcp(*db, n_vars, [])[0]:
        return 1
    return 1 if ora.bcp(*db, n_vars, [-l for l in dict.fromkeys(target)])[0] else 0


def judge_file(cnf, path, cores):
    """oracle.check_rup on the file: per UNSAT instance with its core as unit clauses; cores: {instance: core}."""
    proof = read_drup(path, deletions=False)
    for i, core in cores.items():
        lits, offs = ora.to_csr(cnf.clauses + [[l] for l in core])
        assert ora.check_rup(lits, offs, cnf.n_vars, proof) == 1, ("the oracle rejects the file for instance", i, core)


def assert_core_lines(path, cores):
    """Every UNSAT instance's negated core is a line of the file (as a literal set) - except a tautological core, and the
    empty core, for which the file holds exactly one empty clause."""
    lines = lines_of(path)
    for i, core in cores.items():
        clause = negated(core)
        if not clause:
            assert lines.count(()) == 1, ("empty clauses in the file", lines.count(()))
        elif not is_tautology(clause):
            assert tuple(sorted(set(clause))) in lines, ("no core line for instance", i, core)
    assert lines.count(()) <= 1


def check_targets_on_fresh_handle(make_solver, cnf, path, targets, **opts):
    s = make_solver(**opts)
    try:
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        return s.check_proof_targets_file(path, targets)
    finally:
        s.close()


def cut_file(path, keep_num, keep_den):
    """The file without its last lines: the first keep_num / keep_den of them."""
    lines = open(path).read().splitlines(keepends=True)
    cut = str(path) + ".cut"
    with open(cut, "w") as f:
        f.writelines(lines[:len(lines) * keep_num // keep_den])
    return cut


def run_batch(make_solver, name, path, inspect=None, **more):
    """solve_batch of a case with a proof path, judged as the module's docstring says; inspect (may be None) gets the
    solver after the batch.  Returns (cores, stats, debug_proof_log)."""
    cnf, _ = sc.formula(name)
    ls, want = sc.lists(name)
    s = make_solver(**batch_options(name, **more))
    s.set_proof_path(str(path))
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    res = s.solve_batch(ls)
    assert [r.value for r in res] == list(want), (res, want)
    cores = {i: s.core_of(i) for i in range(len(ls)) if want[i] == 20}
    st = s.stats()
    log = s.debug_proof_log()
    if inspect:
        inspect(s)
    s.close()
    for i, core in cores.items():
        assert set(core) <= set(ls[i]), (i, core, ls[i])
    assert_core_lines(path, cores)
    judge_file(cnf, path, cores)
    return cores, st, log


def run_batch_and_check(make_solver, name, tmp_path, check_opts=None, inspect=None, **more):
    """run_batch, then the file on a fresh handle that holds only the CNF: every target valid; and the file with its last
    third of lines cut off: what the oracle says of each target."""
    cnf, _ = sc.formula(name)
    path = str(tmp_path / "batch.drup")
    cores, st, log = run_batch(make_solver, name, path, inspect=inspect, **more)
    order = sorted(cores)
    targets = [negated(cores[i]) for i in order]
    assert targets, "the case has no UNSAT instance"
    check_opts = dict(check_opts or {})
    info = check_targets_on_fresh_handle(make_solver, cnf, path, targets, **check_opts)
    assert info["valid"] == 1 and info["target_valid"] == [1] * len(targets), info
    lemmas, n_del = pc.lemmas_of(read_drup(path))
    assert info["n_lemmas"] == len(lemmas) and info["n_deletions_ignored"] == n_del, info
    cut = cut_file(path, 2, 3)
    cut_lemmas, _ = pc.lemmas_of(read_drup(cut))
    want = [target_reference(cnf.clauses, cnf.n_vars, cut_lemmas, t) for t in targets]
    got = check_targets_on_fresh_handle(make_solver, cnf, cut, targets, **check_opts)
    print("cut file:", got["target_valid"], "oracle:", want)
    assert got["target_valid"] == want, (got, want)
    return cores, st, log


def run_scheduled_sweep(make_solver, name, seed, path, **more):
    """The stepwise sweep of a case under a seeded schedule with a proof path: sweep_core_of for each UNSAT instance at the
    step that reports it, the file judged after sweep_end.  Returns (cores, stats)."""
    cnf, _ = sc.formula(name)
    ls, want = sc.lists(name)
    n = len(ls)
    sched = sc.seeded_schedule(seed, n)
    final = sc.final_step(sched)
    sched = [a for a in sched if a[1] in ("drop", "reopen", "weights")]
    sched += [(final, "reopen", list(range(n))), (final, "weights", [1.0] * n)]
    s = make_solver(**batch_options(name, **more))
    if path:
        s.set_proof_path(str(path))
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    s.sweep_begin(ls)
    verdict, cores, withdrawn = [0] * n, {}, set()
    step = after = 0
    while True:
        for _, kind, arg in [a for a in sched if a[0] == step]:
            if kind == "drop":
                s.sweep_drop(arg)
                withdrawn |= {i for i in arg if not verdict[i]}
            elif kind == "reopen":
                s.sweep_reopen(arg)
                withdrawn -= set(arg)
            else:
                s.sweep_set_weights(arg)
        res, _ = s.sweep_step()
        for i in range(n):
            got = res[i].value
            if i in withdrawn:
                continue
            assert got in (0, want[i]), (step, i, got, want[i])
            if got == 20 and not verdict[i] and path:
                cores[i] = s.sweep_core_of(i)
                assert set(cores[i]) <= set(ls[i]), (i, cores[i], ls[i])
            verdict[i] = got
        step += 1
        if step > final:
            after += 1
            if all(verdict) or after >= sc.slice_cap(name, "default"):
                break
    assert verdict == list(want), (verdict, want)
    st = s.stats()
    s.sweep_end()
    s.close()
    if path:
        assert sorted(cores) == [i for i in range(n) if want[i] == 20]
        assert_core_lines(path, cores)
        judge_file(cnf, path, cores)
    return cores, st


# ---- several targets, by inspection ---------------------------------------------------------------------------------------
def targets_check(make_solver, clauses, n_vars, proof, targets, segments=0, chunk=0, deletions=False, **opts):
    s = make_solver(**opts)
    try:
        cnf = Csr(clauses, n_vars)
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(n_vars)
        if chunk:
            s.debug_proof_check_chunk(chunk)
        if deletions:
            s.set_proof_deletions(True)
        return s.check_proof_targets(proof, targets, segments=segments)
    finally:
        s.close()


def expected(clauses, n_vars, lemmas, targets):
    """(target_valid, valid, first_failed) by the oracle: the lemmas by reference() without a target's help (an always-true
    target), each target by target_reference()."""
    lemma_ref = pc.reference(clauses, n_vars, lemmas, target=(1, -1), refuted=True)
    tv = [target_reference(clauses, n_vars, lemmas, t) for t in targets]
    first = lemma_ref[1]
    if first is None and 0 in tv:
        first = len(lemmas) + tv.index(0)
    return tv, (1 if first is None else 0), first


def long_target_case(n):
    """pc.long_case(n): the lemma (x1 .. x(n-1) | y) and two targets of n literals, one RUP and one not."""
    clauses, nv, ly, lw, lw_short = pc.long_case(n)
    return clauses, nv, [ly], [lw, lw_short, ly]


# name: (clauses, n_vars, lemmas, targets)
TARGET_CASES = {
    "three-targets-the-middle-one-not-rup": (pc.CHAIN, 7, [[2]], [[3, 6], [6], [2, 7]]),
    "a-tautological-target": (pc.OPEN, 5, [[2]], [[5, -5], [3], [2]]),
    "zero-lemmas": (pc.OPEN, 4, [], [[2], [3], [1, 2]]),
    "targets-behind-refuted-at": (pc.CHAIN, 7, [[2], [3], [6]], [[7], [-7], []]),
    "targets-do-not-see-each-other": (pc.OPEN, 4, [], [[3], [3, 4], [3]]),
    "a-target-of-65-literals": long_target_case(65),
    "a-target-of-130-literals": long_target_case(130),
}
TARGET_WANT = {"three-targets-the-middle-one-not-rup": ([1, 0, 1], 0, 2)}      # (by inspection; the others: the oracle's)


def run_target_case(make_solver, name, **opts):
    clauses, n_vars, lemmas, targets = TARGET_CASES[name]
    want = expected(clauses, n_vars, lemmas, targets)
    if name in TARGET_WANT:
        assert want == TARGET_WANT[name], (want, "the case's expectation is not the oracle's")
    n_items = len(lemmas) + len(targets)
    for segments in (1, 2, n_items):
        for chunk in (0, 1):
            info = targets_check(make_solver, clauses, n_vars, pc.flat(lemmas), targets, segments=segments, chunk=chunk, **opts)
            assert (info["target_valid"], info["valid"], info["first_failed"]) == want, (name, segments, chunk, info, want)
            assert info["n_lemmas"] == len(lemmas) and info["segments"] == min(segments, n_items), info


def run_one_target_equals_check_proof(make_solver, **opts):
    """n_targets = 1: every field equals check_proof's (the times aside) on every inspection case of proof_check_cases."""
    for name, (clauses, n_vars, lemmas, dels, target, _) in pc.INSPECTION.items():
        for segments in (0, 1, 2):
            a = pc.check(make_solver, clauses, n_vars, pc.flat(lemmas, dels), target, segments=segments, **opts)
            b = targets_check(make_solver, clauses, n_vars, pc.flat(lemmas, dels), [list(target)], segments=segments, **opts)
            tv = b.pop("target_valid")
            for k in a:
                if k not in ("seconds", "kernel_seconds"):
                    assert a[k] == b[k], (name, segments, k, a, b)
            assert tv == [target_reference(clauses, n_vars, lemmas, target)], (name, tv)


def run_deleted_lemma_only_a_target_needs(make_solver, **opts):
    """F = (1 | 2 | 3), (~1 | 2 | 3), (~3 | 4 | 5), (~3 | 4 | ~5), (6 | 7).  The lemma (2 | 3) is RUP; the target (2 | 4) is RUP
    only through it (~2 and ~4 alone propagate nothing); the target (6 | 7) needs no lemma.  A deletion line takes (2 | 3)
    away behind the last lemma: honoured, the first target turns invalid; ignored, it stays valid.  Judge: target_reference()
    on the lemma list with the deletion applied."""
    clauses, n_vars = [[1, 2, 3], [-1, 2, 3], [-3, 4, 5], [-3, 4, -5], [6, 7]], 7
    lemmas = [[2, 3], [6, 7, 1]]
    targets = [[2, 4], [6, 7]]
    proof = pc.flat(lemmas, {2: [[2, 3]]})
    kept = [lemmas[1]]
    want_ignored = [target_reference(clauses, n_vars, lemmas, t) for t in targets]
    want_honoured = [target_reference(clauses, n_vars, kept, t) for t in targets]
    assert (want_ignored, want_honoured) == ([1, 1], [0, 1]), (want_ignored, want_honoured)
    assert pc.reference(clauses, n_vars, lemmas, target=(1, -1))[0] == 1
    for segments in (1, 2, 4):
        info = targets_check(make_solver, clauses, n_vars, proof, targets, segments=segments, **opts)
        assert info["target_valid"] == want_ignored and info["valid"] == 1, info
        info = targets_check(make_solver, clauses, n_vars, proof, targets, segments=segments, deletions=True, **opts)
        assert info["target_valid"] == want_honoured and info["first_failed"] == len(lemmas), info


def run_fuzz_targets(make_solver, case, **opts):
    """An UNSAT fuzz case and the oracle's proof of it.  Targets: the empty clause, two of the proof's lemmas, and one
    clause the oracle says does not follow by propagation (a unit).  Each target_valid[t] is reference(..., target = t)[0]:
    behind the first three quarters of the proof, where the database is not refuted yet and the verdicts differ, and
    behind the whole proof, where it is and every target holds."""
    cnf, lemmas, ref = pc.oracle_proof(case)
    assert ref[0] == 1
    # cut the proof in front of its last quarter: the database is then not refuted yet, and the verdicts differ by target
    body = lemmas[:max(1, 3 * len(lemmas) // 4)]
    not_implied = next(([v] for v in range(1, cnf.n_vars + 1)
                        if pc.reference(cnf.clauses, cnf.n_vars, body, target=[v])[0] == 0), None)
    assert not_implied is not None
    targets = [[], body[0], body[len(body) // 2], not_implied]
    want = [pc.reference(cnf.clauses, cnf.n_vars, body, target=t)[0] for t in targets]
    assert want[1:3] == [1, 1] and want[3] == 0, want
    info = targets_check(make_solver, cnf.clauses, cnf.n_vars, pc.flat(body), targets, segments=3, **opts)
    assert info["target_valid"] == want, (info, want)
    # and the whole proof: the database is refuted by the end, so every target holds
    full = [pc.reference(cnf.clauses, cnf.n_vars, lemmas, target=t)[0] for t in targets]
    assert full == [1, 1, 1, 1]
    info = targets_check(make_solver, cnf.clauses, cnf.n_vars, pc.flat(lemmas), targets, segments=3, **opts)
    assert info["target_valid"] == full and info["valid"] == 1, info


def run_target_errors(make_solver, solver_error):
    import pytest
    s = make_solver()
    cnf = Csr(pc.OPEN, 4)
    s.add_cnf(cnf.lits, cnf.offsets)
    proof = np.asarray([2, 0], dtype=np.int32)
    for targets in ([], [[2], [1, 0, 2]], [[2], [5]]):
        with pytest.raises(solver_error) as e:
            s.check_proof_targets(proof, targets)
        assert e.value.code == pc.ERR_ARG, targets
    assert s.check_proof_targets(proof, [[2], [3]])["target_valid"] == [1, 0]
    s.sweep_begin([[1], [-1]])
    with pytest.raises(solver_error) as e:
        s.check_proof_targets(proof, [[2]])
    assert e.value.code == pc.ERR_STATE
    with pytest.raises(solver_error) as e:             # a sweep without a proof path computes no cores
        s.sweep_core_of(0)
    assert e.value.code == pc.ERR_STATE
    s.sweep_end()
    with pytest.raises(solver_error) as e:
        s.sweep_core_of(0)
    assert e.value.code == pc.ERR_STATE
    assert s.check_proof_targets(proof, [[2], [3]])["target_valid"] == [1, 0]
    s.close()
