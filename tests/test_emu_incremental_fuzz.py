"""Differential tests of the warm incremental solve and of foreign ring records on the wave emulator (tests/emu): seeded
sequences of added clauses, assumption sets and calls in between over formulas with planted equivalences, level-0 facts and
elimination candidates (tests/incremental_cases.py), and records from another handle that collapse under the importer's own
simplification (tests/import_cases.py) - judged by the oracle alone; the two modules say how.  Every sequence runs on one
build of the search kernel, incremental_cases.MATRIX_CASES on the other five."""
import pytest

import import_cases as im
import incremental_cases as ic
from fuzz_cases import BUILD_IDS, BUILD_LIST, wanted_build
from helpers import assert_search_build, emu_lib
from timberborn_support_solver_amd import Mi355Sat


def emu_solver(**kw):
    return Mi355Sat(_lib_override=emu_lib(), **kw)


def release():
    emu_lib().mi355sat_release_cached_memory()


def run(name, one_per_simd, lds_val, tmp_path):
    c, e = ic.run_sequence(emu_solver, name, tmp_path, release=release, grows=True, one_per_simd=one_per_simd, lds_val=lds_val)
    assert_search_build(c.s, *wanted_build(one_per_simd, lds_val))
    c.s.close()
    return c, e


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_the_generator_is_seeded():
    a = ic._Generator(ic.CASES["subst-s0-n90"]).run()
    assert a == ic._Generator(ic.CASES["subst-s0-n90"]).run() == ic.sequence("subst-s0-n90")[0]
    assert a != ic._Generator(ic.CASES["subst-s0-n90"]._replace(seed=12)).run()


@pytest.mark.parametrize("cases", [ic.CASES, ic.GPU_CASES], ids=["emulator-cases", "all-cases"])
def test_the_table_meets_its_conditions(cases):
    tot = ic.table_counts(cases)
    print({k: dict(v) for k, v in tot.items()})
    assert all(tot["classes"][cls] > 0 for cls in ic.CLASSES), [cls for cls in ic.CLASSES if not tot["classes"][cls]]
    assert all(tot["calls"][b] > 0 for b in ic.BETWEEN), [b for b in ic.BETWEEN if not tot["calls"][b]]
    v, n = tot["verdicts"], sum(tot["verdicts"].values())
    assert 3 * v["S"] >= n and 5 * v["U"] >= n, v                           # a third SAT, a fifth UNSAT with a non-empty core
    for name in cases:
        steps, info = ic.sequence(name)                                       # (asserts the verdict string; E only in the last two)
        case = cases[name]
        assert len(steps) == case.n_solves <= 25 and not steps[0]["clauses"]
        if case.n_solves >= 10:     # one empty assumption set, one with a repeated literal, one with a contradicting pair
            assert all(info["kinds"][k] == 1 for k in ic.A_KINDS), (name, info["kinds"])
            sets = [st["assumptions"] for st in steps]
            assert [] in sets and any(len(set(a)) < len(a) for a in sets) and any(-l in a for a in sets for l in a)
        assert all(len(st["assumptions"]) <= 8 for st in steps)
        added = sum(len(st["clauses"]) for st in steps)
        assert added <= 3 * case.n_solves + ic.N_FALSE + 3                    # 0 .. 3 clauses per step, and the unit block
    for simp in (-1, 0, 1, 2):
        assert sum(c.simp == simp for c in cases.values()) >= 2, simp
    assert sum(c.opts.get("conflict_budget", 0) > 0 for c in cases.values()) >= 2
    assert sum(c.workers == 258 and c.opts.get("ramp", 0) == 0 for c in cases.values()) >= 1
    assert set(ic.MATRIX_CASES) <= set(ic.CASES) and len(ic.MATRIX_CASES) == 4
    if cases is ic.GPU_CASES:
        assert {c.workers for c in cases.values()} >= {1, 2, 8, 258}
        assert max(c.n_solves for c in cases.values()) == 25
        assert max(ic.base_formula(c)[0].n_vars for c in cases.values()) == 300


def test_the_long_clauses_reach_the_second_round_of_the_attach_kernel():
    """What the classes promise, checked on the generated clauses: with the caller's variable order the host sorts a clause
    by variable, so a literal over a variable above the unit block's stands at position 64 or later."""
    seen = set()
    for name in ic.CASES:
        steps, _ = ic.sequence(name)
        nb = ic.base_formula(ic.CASES[name])[0].n_vars
        false = set(range(nb + 1, nb + 1 + ic.N_FALSE))
        for st in steps:
            for cls, cl in st["clauses"]:
                if cls in ic.LENGTHS:
                    assert len(cl) == ic.LENGTHS[cls] and len({abs(l) for l in cl}) == len(cl)
                if cls in ("long_one_free", "long_two_free"):
                    order = sorted(cl, key=abs)
                    free = [k for k, l in enumerate(order) if abs(l) not in false]
                    assert all(l > 0 for l in cl if abs(l) in false) and len(cl) >= 70
                    assert (free == [len(cl) - 1]) if cls == "long_one_free" else (free == [0, len(cl) - 1]), (cls, free)
                    seen.add(cls)
    assert seen == {"long_one_free", "long_two_free"}


# ---- warm sequences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ic.CASES))
def test_emulated_warm_sequence(tmp_path, name):
    c, e = run(name, 0, 1, tmp_path)
    case = ic.CASES[name]
    assert e.warm_attached > 0 and e.warm >= 2, (e.warm, e.cold)
    if case.simp in (0, 1) and "equiv_dup" in case.menu:
        # both members of an equivalence class reached a warm attach: as one device literal twice, as a tautology
        assert e.subst_hits["equiv_dup"] > 0 and e.subst_hits["equiv_taut"] > 0, e.subst_hits
    if case.simp in (0, 1) and "fixed_sat" in case.menu:
        assert sum(e.fixed_hits.values()) > 0, e.fixed_hits                 # a clause over literals the simplification fixed
    if case.simp == 2:
        assert e.warm_classes["elim_kept"] > 0, e.warm_classes             # a clause over kept variables stays warm


@pytest.mark.parametrize("one_per_simd,lds_val", [b for b in BUILD_LIST if b != (0, 1)],
                         ids=[i for b, i in zip(BUILD_LIST, BUILD_IDS) if b != (0, 1)])
@pytest.mark.parametrize("name", ic.MATRIX_CASES)
def test_emulated_warm_sequence_on_every_search_build(tmp_path, name, one_per_simd, lds_val):
    run(name, one_per_simd, lds_val, tmp_path)


# ---- foreign records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("simp", [0, 2])
@pytest.mark.parametrize("name", list(im.IMPORT_CASES))
def test_emulated_import_of_records_that_collapse(name, simp):
    s, _ = im.check_collapsing_imports(emu_solver, name, simp)
    s.close()


@pytest.mark.parametrize("simp_b", [0, 2])
@pytest.mark.parametrize("name", im.TWO_HANDLE_CASES)
def test_emulated_exchange_between_two_live_handles(name, simp_b):
    for s in im.check_two_live_handles(emu_solver, name, simp_b):
        s.close()
