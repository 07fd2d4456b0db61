"""What logging a batch's proof costs, and what checking all its targets in one pass buys, measured (DESIGN.md §4;
profiles/r12_sweep_proof.log is this script's output).  Three runs each way, alternating.  A record, not a gate.

  (a) the drain: rect 24x24 k = 8 with a proof path, 1024 workers - the solve's wall time and, from this tree's library,
      the wall time inside proof_drain (mi355sat_debug_proof_log).  With --parent-lib PATH (a libmi355sat.so built from
      the parent commit, which copies every worker's log by itself) the same solve runs through that library, by its C
      ABI alone: the totals compare, the parent has no drain timer.
  (b) the logging overhead: the rect 24x24 ladder k = K0 .. 0 as one stepwise sweep (the bounds tbs_cli --sweep poses) with
      and without a proof path, deterministic = 1 so that both make the same decisions: time per step, and the share of
      the drains in it.
  (c) the targets: one check_proof_targets_file over all UNSAT bounds of that sweep's file against one check_proof_file per
      bound.

    python scripts/gpu_sweep_proof.py [--parent-lib PATH] [--size N] [--k K] [--k0 K0]
"""
import ctypes
import os
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timberborn_support_solver_amd import PLATFORMS_DEFAULT, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult, WorldGrid  # noqa: E402

LIMIT_S = 60


def within(s, fn):
    tm = threading.Timer(LIMIT_S, s.interrupter().interrupt)
    tm.start()
    try:
        return fn()
    finally:
        tm.cancel()


def solve_parent(tag, cnf, proof, lib, workers):
    from timberborn_support_solver_amd.solver import Mi355SatOpts
    vp = ctypes.c_void_p
    lib.mi355sat_new.restype = vp
    lib.mi355sat_new.argtypes = [ctypes.POINTER(Mi355SatOpts)]
    lib.mi355sat_free.argtypes = [vp]
    lib.mi355sat_add_cnf.argtypes = [vp, vp, vp, ctypes.c_uint64]
    lib.mi355sat_set_proof_path.argtypes = [vp, ctypes.c_char_p]
    lib.mi355sat_solve.argtypes = [vp]
    opts = Mi355SatOpts()
    opts.device = -1
    opts.workers = workers
    lits, offs = np.ascontiguousarray(cnf.lits, dtype=np.int32), np.ascontiguousarray(cnf.offsets, dtype=np.uint64)
    h = lib.mi355sat_new(ctypes.byref(opts))
    try:
        lib.mi355sat_add_cnf(h, lits.ctypes.data, offs.ctypes.data, len(offs) - 1)
        lib.mi355sat_set_proof_path(h, proof.encode())
        t = time.time()
        rc = lib.mi355sat_solve(h)
        print(f"(a) {tag}: solve rc {rc} in {time.time() - t:.3f} s, proof file {os.path.getsize(proof)} bytes", flush=True)
    finally:
        lib.mi355sat_free(h)


def solve_here(tag, cnf, proof, workers):
    s = Mi355Sat(workers=workers)
    s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    t = time.time()
    r = within(s, s.solve)
    dt = time.time() - t
    log, st = s.debug_proof_log(), s.stats()
    s.close()
    per = 1e3 * log["drain_seconds"] / max(1, log["drains"])
    print(f"(a) {tag}: solve {r.name} in {dt:.3f} s, {st['kernel_launches']} launches, proof file {os.path.getsize(proof)} bytes; "
          f"{log['drains']} drains {log['drain_seconds']:.3f} s in all ({per:.3f} ms each), {log['gathers']} gathers, "
          f"{log['logs']} non-empty logs, {log['words']} words", flush=True)


def sweep(tag, cnf, sets, proof, workers):
    s = Mi355Sat(workers=workers, deterministic=1)
    if proof:
        s.set_proof_path(proof)
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    t0 = time.time()
    s.sweep_begin(sets)
    t1 = time.time()
    steps, res, nd = 0, [], 0
    while nd < len(sets) and time.time() - t1 < LIMIT_S:
        res, nd = s.sweep_step()
        steps += 1
    t2 = time.time()
    cores = {i: s.sweep_core_of(i) for i, r in enumerate(res) if proof and r == SolverResult.Unsat}
    log, st = s.debug_proof_log(), s.stats()
    s.sweep_end()
    s.close()
    line = (f"(b) {tag}: begin {t1 - t0:.3f} s, {steps} steps in {t2 - t1:.3f} s ({1e3 * (t2 - t1) / max(1, steps):.2f} ms each), decided {nd} of "
            f"{len(sets)}, conflicts {st['conflicts']}")
    if proof:
        line += (f"; drains {log['drain_seconds']:.3f} s = {100 * log['drain_seconds'] / max(1e-9, t2 - t1):.1f} % of the steps, "
                 f"{log['words']} words, {log['core_lines']} core lines, file {os.path.getsize(proof)} bytes")
    print(line, flush=True)
    return [r.value for r in res], cores


def targets(run, cnf, proof, cores):
    order = sorted(cores)
    tg = [[-l for l in cores[i]] for i in order]
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    t = time.time()
    info = within(s, lambda: s.check_proof_targets_file(proof, tg))
    one = time.time() - t
    s.close()
    print(f"(c) run {run}: one pass over {len(tg)} targets: {one:.3f} s (kernel {info['kernel_seconds']:.3f} s)  valid {info['valid']}  "
          f"target_valid {info['target_valid']}  lemmas {info['n_lemmas']}  segments {info['segments']}", flush=True)
    each, kernel, valid = 0.0, 0.0, []
    for c in tg:
        s = Mi355Sat()
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        t = time.time()
        info = within(s, lambda: s.check_proof_file(proof, target=c))
        each += time.time() - t
        kernel += info["kernel_seconds"]
        valid.append(info["valid"])
        s.close()
    print(f"(c) run {run}: one check_proof_file per target: {each:.3f} s in all (kernel {kernel:.3f} s)  valid {valid}", flush=True)


def main():
    args = sys.argv[1:]
    parent, size, k, k0 = None, 24, 8, 12
    while args:
        flag, val, args = args[0], args[1], args[2:]
        if flag == "--parent-lib":
            parent = ctypes.CDLL(val)
        elif flag == "--size":
            size = int(val)
        elif flag == "--k":
            k = int(val)
        elif flag == "--k0":
            k0 = int(val)
        else:
            raise SystemExit(__doc__)
    grid = WorldGrid.from_rows(["X" * size] * size)
    enc = Encoding.encode(PLATFORMS_DEFAULT, grid)
    with tempfile.TemporaryDirectory() as d:
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
        print(f"rect{size}x{size} default k={k}: {cnf.n_vars} variables, {len(cnf.offsets) - 1} clauses", flush=True)
        for run in range(3):
            if parent is not None:
                solve_parent(f"run {run}: parent", cnf, os.path.join(d, "parent.drup"), parent, 1024)
            solve_here(f"run {run}: gather", cnf, os.path.join(d, "here.drup"), 1024)
        cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k0}), sweep=True)
        sets = [([-int(cnf.card_outputs[j])] if j < len(cnf.card_outputs) else []) for j in range(k0, -1, -1)]
        proof = os.path.join(d, "sweep.drup")
        cores = {}
        for run in range(3):
            sweep(f"run {run}: no proof", cnf, sets, None, 1024)
            _, cores = sweep(f"run {run}: proof   ", cnf, sets, proof, 1024)
        if cores:
            for run in range(3):
                try:
                    targets(run, cnf, proof, cores)
                except SolverError as e:          # (a file the checker's stores do not hold is a finding of this record)
                    print(f"(c) run {run}: {e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
