"""The option-matrix tests of the search kernel, written once for the emulator and the GPU (tests/test_emu_options.py,
test_gpu_options.py): mi355sat_opts fields that switch on kernel code - vivify, rephase, phase_mix, share_interval,
import_pct, share_len, restart_k_pct, restart_k2_pct, max_groups - each run against the oracle's verdict, a checked model
or RUP-checked proof and an implied exchange ring (tests/fuzz_cases.py), and each proven to have taken its path by a counter
of mi355sat_debug_heuristics where it has one.  vivify and rephase run on a lowered schedule (mi355sat_debug_set_schedule):
their defaults (1500 / 400 / 2000 conflicts of one worker) are out of a quick test's reach."""
import numpy as np

from fuzz_cases import GPU_CASES, solve_and_judge
from helpers import long_list_formula, make_grid, platform_defs, scripted_decisions
from oracle import oracle as ora
from timberborn_support_solver_amd import Encoding, PlatformLimits

# Vivification, rephasing and the import all happen at decision level 0, that is after a restart, and whether a worker restarts
# before a small formula is decided is luck (Glucose's test compares two LBD averages; on the GPU the two workers of
# "3sat-n60-s2" refuted it, and a SAT case of 627 oracle conflicts was satisfied after 83, before either had restarted).  So
# these tests do not wait for luck: RESTARTS makes the test true whenever the window of 50 LBDs is full - a restart every 50
# conflicts of a worker - and REPEATABLE runs the solve in the deterministic mode (conflict-bounded slices, ordered
# exchange, fixed seed), in which a run's counters are a function of its inputs on the emulator and on the GPU alike
# (tests/test_gpu_parity.py::test_deterministic_mode_repeats_itself_on_the_gpu).
UNSAT_CASE, SAT_CASE = "3sat-n60-s2", "3sat-n70-s5"            # 105 / 106 oracle conflicts
REPHASE_CASES = ("mixedw-n120-s102", "3sat-n70-s5")            # UNSAT / SAT
RESTARTS = dict(restart_k_pct=1000)
REPEATABLE = dict(deterministic=1, seed=7)
VIVIFY_SCHEDULE = (20, 20, 0)
REPHASE_SCHEDULE = (0, 0, 10)
KNOBS = [dict(phase_mix=1), dict(share_interval=5), dict(import_pct=1), dict(import_pct=100), dict(share_len=2), dict(share_len=31),
         dict(restart_k_pct=70), dict(restart_k2_pct=130)]
KNOB_IDS = ["-".join(f"{k}={v}" for k, v in kw.items()) for kw in KNOBS]
MAX_GROUPS = [1, 2, 3, 8, 31, 32, 100]


def check_vivify(make_solver, tmp_path, name, one_per_simd, lds_val, **kw):
    """Exchange on (two workers): what vivification rewrites in place is logged as a lemma (the proof checks), exported (the
    ring stays implied) and watched anew (the verdict, the model).  The full-fleet build has no vivification code."""
    s, r, st = solve_and_judge(make_solver, GPU_CASES[name], one_per_simd, lds_val, tmp_path, vivify=8, schedule=VIVIFY_SCHEDULE,
                               workers=2, ring=True, slice_conflicts=50, **RESTARTS, **REPEATABLE, **kw)
    h = s.debug_heuristics()
    print(name, (one_per_simd, lds_val), r.name, st["conflicts"], h)
    if one_per_simd == 4:
        assert h["n_vivified"] == 0 and h["n_viv_lits"] == 0
    else:
        assert h["n_vivified"] > 0 and h["n_viv_lits"] >= h["n_vivified"]
    assert st["shared_exported"] > 0
    s.close()


def check_rephase(make_solver, tmp_path, name, rephase, one_per_simd, lds_val, **kw):
    s, r, st = solve_and_judge(make_solver, GPU_CASES[name], one_per_simd, lds_val, tmp_path, rephase=rephase, schedule=REPHASE_SCHEDULE,
                               workers=2, slice_conflicts=50, **RESTARTS, **REPEATABLE, **kw)
    h = s.debug_heuristics()
    print(name, rephase, r.name, st["conflicts"], st["restarts"], h)
    assert h["n_rephase"] > 0 and h["n_rephase"] <= st["restarts"]         # (a rephasing happens at a restart)
    s.close()


def check_knob(make_solver, tmp_path, name, knob, one_per_simd, lds_val, **kw):
    """Three workers, short slices (the exchange is collected between slices).  Counters: share_interval -> imports forced
    in mid-search; import_pct = 1 -> records skipped, = 100 -> none skipped and some attached; share_len = 2 -> no ring
    record longer.  Restarts every 50 conflicts (RESTARTS) so that the workers do import - except where the knob is the restart
    factor itself.  phase_mix and the restart factors have no counter of their own: verdict, proof and ring only."""
    s, r, st = solve_and_judge(make_solver, GPU_CASES[name], one_per_simd, lds_val, tmp_path, workers=3, slice_conflicts=25,
                               **({} if any(k.startswith("restart_k") for k in knob) else RESTARTS), **REPEATABLE, **knob, **kw)
    h = s.debug_heuristics()
    ring = s.debug_share_ring()
    print(knob, r.name, st["conflicts"], st["restarts"], st["shared_exported"], st["shared_imported"], h, max(len(c) for c in ring))
    assert st["shared_exported"] > 0 and len(ring) > 0
    if "share_interval" in knob:
        assert h["forced_imports"] > 0
    else:
        assert h["forced_imports"] == 0          # off by default: imports wait for a restart
    if knob.get("import_pct") == 1:
        assert h["import_skipped"] > 0
    if knob.get("import_pct") == 100:
        assert h["import_skipped"] == 0 and st["shared_imported"] + st["shared_imported_units"] > 0
    if "share_len" in knob:
        assert max(len(c) for c in ring) <= knob["share_len"]
        if knob["share_len"] == 31:
            assert max(len(c) for c in ring) > 2
    s.close()


def check_search_max_groups(make_solver, tmp_path, name, max_groups, one_per_simd, lds_val, **kw):
    s, r, st = solve_and_judge(make_solver, GPU_CASES[name], one_per_simd, lds_val, tmp_path, workers=2, slice_conflicts=50,
                               max_groups=max_groups, **REPEATABLE, **kw)
    if max_groups == 1:
        assert st["bcp_requeued"] == 0 and st["bcp_steps"] == st["propagations"]     # one literal per step: no two groups to meet
    s.close()


_bcp = {}


def bcp_inputs(which):
    """(lits, offsets, n_vars, scripts, the oracle's answers), computed once and shared by the max_groups values."""
    if which not in _bcp:
        if which == "long-lists":
            lits, offsets, n_vars, n_hubs, rng = long_list_formula(11)
            scripts = []
            for _ in range(24):         # (shorter scripts than test_emu_kernels.py's: more of them reach a fixpoint)
                dec = [int(h + 1) for h in rng.permutation(n_hubs)[: int(rng.integers(1, n_hubs + 1))]]
                dec += [int(v + 1) * (1 if rng.random() < 0.5 else -1) for v in rng.choice(np.arange(n_hubs, n_vars), size=int(rng.integers(4, 60)), replace=False)]
                scripts.append([int(x) for x in rng.permutation(dec)])
        else:
            grid = make_grid("rect8x8")
            enc = Encoding.encode(platform_defs("default"), grid)
            cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): 6}))
            lits, offsets, n_vars = cnf.lits, cnf.offsets, cnf.n_vars
            scripts = [scripted_decisions(enc, grid, 100 + i, 3 + i) for i in range(5)]               # mostly conflicts
            scripts += [scripted_decisions(enc, grid, 100 + i, 2 + i, p_positive=0.1) for i in range(10)]  # mostly fixpoints
        want = [ora.bcp(lits, offsets, n_vars, dec) for dec in scripts]
        assert sum(1 for w in want if not w[0]) >= 3 and sum(1 for w in want if w[0]) >= 3       # fixpoints and conflicts
        _bcp[which] = (lits, offsets, n_vars, scripts, want)
    return _bcp[which]


def check_bcp_max_groups(make_solver, which, max_groups, lds_val):
    """propagate_batch with max_groups queue literals per BCP step: the fixpoint is unique, so it must equal the oracle's
    bit for bit whatever the group count (values above 32 are clamped).  With one group per step no two groups can meet in
    a clause (bcp_requeued == 0); with 32 they do on the encoder formula (see below for the long-list one)."""
    lits, offsets, n_vars, scripts, want = bcp_inputs(which)
    s = make_solver(lds_val=lds_val, simp=-1, max_groups=max_groups)
    s.add_cnf(lits, offsets)
    confl, vals, tl = s.propagate_batch(scripts, n_vars=n_vars)
    for i, (c, v, n, _) in enumerate(want):
        assert c == confl[i], (which, max_groups, i)
        if not c:
            assert np.array_equal(v, vals[i]) and n == tl[i], (which, max_groups, i)
    st = s.stats()
    print(which, max_groups, "steps", st["bcp_steps"], "requeued", st["bcp_requeued"], "propagations", st["propagations"])
    if max_groups == 1:
        assert st["bcp_requeued"] == 0 and st["bcp_steps"] == st["propagations"]
    else:
        assert st["bcp_steps"] < st["propagations"]           # some step took more than one queue literal
    # Two groups meet in a clause only when two literals of one step watch it.  The encoder formula's scripts do that (one
    # placed platform implies a run of literals at once: 127 re-queued at 32 groups, measured on the emulator).  The
    # long-list formula's do not: propagate_batch enqueues ONE scripted decision per level and that formula's binary /
    # ternary chains rarely imply two literals at once (925 steps for 996 propagations at any group count above 1), so no
    # step ever holds both watches of a clause and bcp_requeued stays 0 there at every group count.
    if max_groups == 32 and which == "encoder":
        assert st["bcp_requeued"] > 0
    s.close()
