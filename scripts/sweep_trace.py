#!/usr/bin/env python3
"""Step-by-step trace of the sweep scheduler on the wave emulator, for comparing two builds of the host code.

    python scripts/sweep_trace.py path/to/libmi355sat_emu.so [group ...] > trace.txt

Runs, on the emulator library given by path, the deterministic suites that pin the scheduler between two slices:
  sweep:<case>    every option set x (no schedule, every seed) of tests/sweep_cases.py for the case, the two stall scripts
                  and, for the long case, long_to_empty_and_back
  incremental     the sequences of tests/incremental_cases.py (but the one whose fleet grows by kernel time)
  coremin         the cases of tests/test_core_minimize.py that run on a handle (not the C program's)
(no group: all of them).  After every sweep_step / solve / solve_batch / minimize_core it prints the results, n_decided and
the counters conflicts, decisions, propagations, kernel_launches of stats(); after an UNSAT answer the core, when a handle is
closed its incremental info.  Two builds that schedule alike print the same bytes: diff the outputs, or their sha256.
The ramp-up (grow_workers, then rebalance_workers for the new workers) goes by kernel time and is not traced here."""
import ctypes
import itertools
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import helpers  # noqa: E402

helpers._emu = ctypes.CDLL(os.path.abspath(sys.argv[1]))      # what helpers.emu_lib() answers with from now on

import incremental_cases as ic  # noqa: E402
import sweep_cases as sw  # noqa: E402
import test_core_minimize as tcm  # noqa: E402
from timberborn_support_solver_amd import Mi355Sat, SolverError, SolverResult  # noqa: E402

COUNTERS = ("conflicts", "decisions", "propagations", "kernel_launches")


def timeless(d):
    return {k: v for k, v in sorted(d.items()) if "seconds" not in k}


class Traced(Mi355Sat):
    def __init__(self, **kw):
        super().__init__(_lib_override=helpers.emu_lib(), **kw)

    def line(self, what, *answer):
        st = self.stats()
        print(what, *answer, *(st[k] for k in COUNTERS), flush=True)

    def sweep_step(self):
        res, n = super().sweep_step()
        self.line("step", [r.value for r in res], n)
        return res, n

    def solve(self, assumptions=()):
        r = super().solve(assumptions)
        self.line("solve", r.value, self.core() if r == SolverResult.Unsat else "")
        return r

    def solve_batch(self, assumption_sets, stop_at_first=False):
        res = super().solve_batch(assumption_sets, stop_at_first)
        self.line("batch", [r.value for r in res], [self.core_of(i) for i, r in enumerate(res) if r == SolverResult.Unsat])
        return res

    def minimize_core(self, conflict_budget=0):
        info = super().minimize_core(conflict_budget)
        self.line("minimize", timeless(info), self.core())
        return info

    def minimize_core_of(self, instance, conflict_budget=0):
        info = super().minimize_core_of(instance, conflict_budget)
        self.line("minimize_of", instance, timeless(info), self.core_of(instance))
        return info

    def close(self):
        if getattr(self, "_h", None):
            try:
                print("close", timeless(self.debug_incremental()), flush=True)
            except SolverError as e:
                print("close", e.code, flush=True)
        super().close()

    __del__ = close


def sweep_group(name):
    for optset in sw.OPTSETS:
        opts = sw.options(name, optset, deterministic=1)
        scheds = [("none", [])] + [(seed, sw.seeded_schedule(seed, sw.CASES[name][8])) for seed in sw.SEEDS]
        for tag, sched in scheds:
            print("##", name, optset, tag, flush=True)
            sw.judge(Traced, name, opts, sched, cap=200 if tag == "none" else sw.slice_cap(name, optset))
    scripts = dict(sw.STALL_SCRIPTS)
    if name == sw.LONG:
        scripts.update({"long-to-empty-and-back-" + o: (o, sw.long_to_empty_and_back(name)) for o in ("default", "no-rebalance")})
    for tag, (optset, sched) in scripts.items():
        print("##", name, tag, flush=True)
        sw.judge(Traced, name, sw.options(name, optset, deterministic=1), sched, cap=sw.slice_cap(name, optset))


def incremental_group():
    for name, case in ic.CASES.items():
        if case.opts.get("ramp", -1) >= 0:      # its fleet grows by kernel time
            continue
        print("##", name, flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            c, _ = ic.run_sequence(Traced, name, pathlib.Path(tmp))
            c.s.close()


def coremin_group():
    defaults = dict(simp=-1, workers=2, slice_conflicts=200)          # (test_assumption_cores.emu_solver's)
    tcm.emu_solver = lambda **kw: Traced(**dict(defaults, **kw))
    tcm.print = lambda *a, **kw: None         # (the tests' own reports carry wall-clock seconds)
    for fname, fn in vars(tcm).items():
        if not fname.startswith("test_") or "tmp_path" in fn.__code__.co_varnames[:fn.__code__.co_argcount]:
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        axes = []
        for m in marks:
            names = [a.strip() for a in m.args[0].split(",")]
            axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
        for combo in itertools.product(*axes):
            kw = {k: v for d in combo for k, v in d.items()}
            print("##", fname, kw, flush=True)
            fn(**kw)


def main():
    groups = sys.argv[2:] or ["sweep:" + n for n in sw.CASES] + ["incremental", "coremin"]
    for g in groups:
        if g.startswith("sweep:"):
            sweep_group(g[6:])
        else:
            {"incremental": incremental_group, "coremin": coremin_group}[g]()


if __name__ == "__main__":
    main()
