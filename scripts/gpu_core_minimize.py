"""Core minimisation on the device, measured: for each case the solve that produces the core, then
mi355sat_minimize_core on the resident sweep against the same deletion loop driven from Python with one cold solve_batch
per round (what a caller could do before), three runs each way, alternating.  Prints one line per run.
The two loops are not the same in detail: the Python one reads whole models (solution_of) where the call looks a chunk's
literals up on the device, and both take the smallest of a round's cores.  The only time limit is a 120 s interrupt per call.

    python scripts/gpu_core_minimize.py [rect sizes ...]        (default 16 24 32)
"""
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timberborn_support_solver_amd import Encoding, Mi355Sat, PlatformLimits, SolverResult, WorldGrid  # noqa: E402

LIMIT_S = 120


def within(s, fn):
    tm = threading.Timer(LIMIT_S, s.interrupter().interrupt)
    tm.start()
    try:
        return fn()
    finally:
        tm.cancel()


def solved(cnf, a, n_vars):
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(n_vars)
    t = time.time()
    r = within(s, lambda: s.solve(a))
    return s, r, time.time() - t


def resident(cnf, a, n_vars):
    s, r, t_solve = solved(cnf, a, n_vars)
    assert r == SolverResult.Unsat, r
    before = s.core()
    t = time.time()
    info = within(s, s.minimize_core)
    dt = time.time() - t
    s.close()
    return (f"resident  solve {t_solve:.3f} s  core {len(before)} -> {info['size_after']}  minimal {info['minimal']}  rounds {info['rounds']}"
            f"  candidates {info['candidates']} (unsat {info['candidates_unsat']}, sat {info['candidates_sat']})"
            f"  critical_by_model {info['critical_by_model']}  conflicts {info['conflicts']}  minimize_core {dt:.3f} s")


def batches(cnf, a, n_vars, width=64):
    """The same deletion by rounds, every round one cold solve_batch on a fresh formula upload."""
    s, r, t_solve = solved(cnf, a, n_vars)
    assert r == SolverResult.Unsat, r
    K = s.core()
    n0, crit, c, rounds, cands = len(K), set(), None, 0, 0
    t = time.time()
    while time.time() - t < LIMIT_S:
        free = [l for l in K if l not in crit]
        if not free:
            break
        m = min(width, len(free))
        even = -(-len(free) // m)
        if c is None or even <= c:
            c = even
            chunks = [free[len(free) * j // m:len(free) * (j + 1) // m] for j in range(m)]
        else:
            chunks = [free[c * j:c * (j + 1)] for j in range(m)]
        sets = [[l for l in K if l not in set(ch)] for ch in chunks]
        res = within(s, lambda: s.solve_batch(sets))
        rounds += 1
        cands += m
        new = 0
        for j, rj in enumerate(res):
            if rj == SolverResult.Sat:
                model = s.solution_of(j, n_vars)
                d = [l for l in chunks[j] if model[abs(l) - 1] != (1 if l > 0 else -1)]
                if len(d) == 1:
                    crit.add(d[0])
                    new += 1
        unsat = [s.core_of(j) for j, rj in enumerate(res) if rj == SolverResult.Unsat]
        if unsat:
            K = min(unsat, key=len)
        elif not new:
            c = max(1, c // 2)
    dt = time.time() - t
    s.close()
    return f"batches   solve {t_solve:.3f} s  core {n0} -> {len(K)}  minimal {int(set(K) == crit)}  rounds {rounds}  candidates {cands}  loop {dt:.3f} s"


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [16, 24, 32]
    for n in sizes:
        grid = WorldGrid.from_rows(["X" * n] * n)
        enc = Encoding.encode([(1, 1)], grid)
        cnf = enc.with_limits_into_cnf(PlatformLimits({}))
        a = [-enc.platform_var(x, y, (1, 1)) for y in range(n) for x in range(n)]
        for run in range(3):
            for fn in (resident, batches):
                print(f"rect{n}x{n} 1x1 anchors {len(a)} run {run}: {fn(cnf, a, cnf.n_vars)}", flush=True)


if __name__ == "__main__":
    main()
