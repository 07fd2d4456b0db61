"""What tracing costs, measured: for each case one solve of the default fleet that writes its DRUP proof, then
mi355sat_check_proof_file against mi355sat_trim_proof_file (hints kept) on fresh handles, three runs each way, alternating;
the proof's lemmas against the needed ones, the formula's clauses against the core, the size of the LRAT file.  One
process; every call is interrupted after LIMIT_S seconds, and anything but the expected answer ends the run there.
A record, not a gate.

    python scripts/gpu_proof_trim.py [SIZE:K ...]        (default 16:3 24:8, rect SIZE x SIZE, default platforms, bound K)
"""
import os
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timberborn_support_solver_amd import PLATFORMS_DEFAULT, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult, WorldGrid  # noqa: E402

LIMIT_S = 240


def within(s, fn):
    tm = threading.Timer(LIMIT_S, s.interrupter().interrupt)
    tm.start()
    try:
        return fn()
    finally:
        tm.cancel()


def fresh(cnf):
    s = Mi355Sat()
    s.add_cnf(cnf.lits, cnf.offsets)
    s.reserve(cnf.n_vars)
    return s


def main():
    cases = [tuple(int(x) for x in a.split(":")) for a in sys.argv[1:]] or [(16, 3), (24, 8)]
    with tempfile.TemporaryDirectory() as d:
        for n, k in cases:
            name = f"rect{n}x{n} default k={k}"
            grid = WorldGrid.from_rows(["X" * n] * n)
            enc = Encoding.encode(PLATFORMS_DEFAULT, grid)
            cnf = enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))
            proof = os.path.join(d, f"rect{n}.drup")
            s = Mi355Sat(workers=16, reduce_first=200, reduce_inc=50)
            s.set_proof_path(proof)
            s.add_cnf(cnf.lits, cnf.offsets)
            t = time.time()
            r = within(s, s.solve)
            st = s.stats()
            s.close()
            print(f"{name}: {cnf.n_vars} variables, {len(cnf.offsets) - 1} clauses; solve {r.name} in {time.time() - t:.3f} s, "
                  f"{st['conflicts']} conflicts, proof file {os.path.getsize(proof)} bytes", flush=True)
            if r != SolverResult.Unsat:
                print(f"{name}: not UNSAT within {LIMIT_S} s - the run ends here", flush=True)
                return 1
            for run in range(3):
                s = fresh(cnf)
                t = time.time()
                try:
                    info = within(s, lambda: s.check_proof_file(proof))
                except SolverError as e:          # (a proof the checker's stores do not hold is a finding of this record)
                    print(f"{name} run {run}: check_proof  {e} - the run ends here", flush=True)
                    return 1
                finally:
                    s.close()
                dt = time.time() - t
                print(f"{name} run {run}: check_proof  {dt:.3f} s (kernel {info['kernel_seconds']:.3f} s, {info['launches']} launches)  valid "
                      f"{info['valid']}  lemmas {info['n_lemmas']}  deletions ignored {info['n_deletions_ignored']}  workers "
                      f"{info['workers']}  propagations {info['propagations']}", flush=True)
                if info["valid"] != 1:
                    return 1
                s = fresh(cnf)
                t = time.time()
                try:
                    res = within(s, lambda: s.trim_proof_file(proof, hints=True))
                except SolverError as e:
                    print(f"{name} run {run}: trim_proof   {e} - the run ends here", flush=True)
                    return 1
                dt = time.time() - t
                if res["check"]["valid"] != 1:
                    print(f"{name} run {run}: trim_proof valid {res['check']['valid']} - the run ends here", flush=True)
                    return 1
                lrat = os.path.join(d, "t.lrat")
                s.trim_write_lrat(lrat)
                s.close()
                c = res["check"]
                print(f"{name} run {run}: trim_proof   {dt:.3f} s (kernel {c['kernel_seconds']:.3f} s, {c['launches']} launches)  valid "
                      f"{c['valid']}  lemmas needed {len(res['lemmas'])} of {c['n_lemmas']}  core {len(res['core'])} of "
                      f"{len(cnf.offsets) - 1} clauses  records {res['dep_records']}  drains {res['log_drains']}  log words per worker "
                      f"{res['log_words_per_worker']}  LRAT file {os.path.getsize(lrat)} bytes", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
