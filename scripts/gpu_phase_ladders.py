#!/usr/bin/env python3
"""The plain refinement loop (solver_loop: a fresh solver per bound, -l1:M on rect M x M) with and without phase hints,
alternating, `reps` runs each way in one session; per rung and for the whole ladder.  GPU box only.
usage: gpu_phase_ladders.py 24,26,28 [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timberborn_support_solver_amd import PLATFORMS_DEFAULT, Encoding, Mi355Sat, PlatformLimits, SolverResult, WorldGrid, solver_loop
sizes = [int(x) for x in sys.argv[1].split(",")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
for m in sizes:
    g = WorldGrid.rect(m, m)
    e = Encoding.encode(PLATFORMS_DEFAULT, g)
    totals = {False: [], True: []}
    for rep in range(reps):
        for hints in (False, True):
            t0 = time.perf_counter()
            hist = solver_loop(g, e, PlatformLimits({(1, 1): m}), out=lambda l: None, phase_hints=hints)
            dt = time.perf_counter() - t0
            ok = hist[-1]["result"] == SolverResult.Unsat and all(h["valid"] for h in hist[:-1])
            totals[hints].append(dt)
            print(f"rect {m} run {rep} phase_hints={int(hints)}: {dt:.2f} s ok={ok} k*={hist[-1]['k'] + 1} rungs", [(h["k"], h["result"].name, h["count"], round(h["seconds"], 2), h["stats"]["conflicts"]) for h in hist], flush=True)
    for hints in (False, True):
        print(f"rect {m} -l1:{m} phase_hints={int(hints)}: whole ladder {min(totals[hints]):.2f}-{max(totals[hints]):.2f} s over {reps} runs", flush=True)
