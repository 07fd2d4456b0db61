"""mi355sat_check_lrat beside the plain-Python checker tests/lrat_check.py on the same files, measured: for each
case one solve of the 16-worker fleet that writes its DRUP proof, one mi355sat_trim_proof_file with the deletion lines
honoured and the hints kept (timed: it is what produced the file), the LRAT file written; then mi355sat_check_lrat_file on a
fresh handle and lrat_check.check in a child process, three runs each way, alternating; last three runs of the device's
other build (lds_val = -1: the assignment map in HBM).  The Python side has a wall-clock
limit: a run that hits it is reported as "not finished in N s".  A record, not a gate.

    python scripts/gpu_lrat_check.py [--py-limit SECONDS] [SIZE:K ...]     (default 16:3 24:8, rect SIZE x SIZE, bound K)
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timberborn_support_solver_amd import PLATFORMS_DEFAULT, Encoding, Mi355Sat, PlatformLimits, SolverError, SolverResult, WorldGrid  # noqa: E402


def bound_cnf(n, k):
    enc = Encoding.encode(PLATFORMS_DEFAULT, WorldGrid.from_rows(["X" * n] * n))
    return enc.with_limits_into_cnf(PlatformLimits({(1, 1): k}))


def python_side(n, k, lrat):
    """(child process; no device) the judge on the file: one line of output."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lrat_check
    cnf = bound_cnf(n, k)
    clauses = [[int(l) for l in cnf.lits[int(cnf.offsets[c]):int(cnf.offsets[c + 1])]] for c in range(len(cnf.offsets) - 1)]
    text = open(lrat).read()
    t = time.time()
    try:
        used, lines = lrat_check.check(clauses, text)
        verdict = f"accepted, last line {'empty' if lines and not lines[-1][1] else 'NOT empty'}, {len(used)} originals used"
    except lrat_check.LratError as e:
        verdict = f"rejected: {e}"
    print(f"{time.time() - t:.3f} s  {verdict}", flush=True)
    return 0


def device_side(name, tag, cnf, lrat, **opts):
    s = Mi355Sat(**opts)
    try:
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        t = time.time()
        i = s.check_lrat_file(lrat)
        dt = time.time() - t
        print(f"{name} {tag}: device  {dt:.3f} s (call {i['seconds']:.3f} s, kernel {i['kernel_seconds']:.4f} s, {i['launches']} launches, "
              f"{i['waves']} waves, build {'lds' if i['lds'] else 'hbm'} {i['dyn_lds_bytes']} B)  valid {i['valid']}  accepted {i['accepted']}  "
              f"lines {i['n_lines']}  hints {i['n_hints']}  longest clause {i['longest_clause']}  originals used {i['used_originals']}", flush=True)
    except SolverError as e:
        print(f"{name} {tag}: device  {e}", flush=True)
    finally:
        s.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--python-side":
        return python_side(int(args[1]), int(args[2]), args[3])
    py_limit = 120
    if args and args[0] == "--py-limit":
        py_limit = int(args[1])
        args = args[2:]
    cases = [tuple(int(x) for x in a.split(":")) for a in args] or [(16, 3), (24, 8)]
    with tempfile.TemporaryDirectory() as d:
        for n, k in cases:
            name = f"rect{n}x{n} default k={k}"
            cnf = bound_cnf(n, k)
            proof, lrat = os.path.join(d, f"rect{n}.drup"), os.path.join(d, f"rect{n}.lrat")
            s = Mi355Sat(workers=16, reduce_first=200, reduce_inc=50)
            s.set_proof_path(proof)
            s.add_cnf(cnf.lits, cnf.offsets)
            t = time.time()
            r = s.solve()
            s.close()
            print(f"{name}: {cnf.n_vars} variables, {len(cnf.offsets) - 1} clauses; solve {r.name} in {time.time() - t:.3f} s, proof file "
                  f"{os.path.getsize(proof)} bytes", flush=True)
            if r != SolverResult.Unsat:
                continue
            s = Mi355Sat()
            s.add_cnf(cnf.lits, cnf.offsets)
            s.reserve(cnf.n_vars)
            s.set_proof_deletions(True)
            t = time.time()
            try:
                res = s.trim_proof_file(proof, hints=True)
            except SolverError as e:
                print(f"{name} trim: {e}", flush=True)
                s.close()
                continue
            dt = time.time() - t
            if res["check"]["valid"] != 1:
                print(f"{name} trim: not valid {res['check']}", flush=True)
                s.close()
                continue
            t = time.time()
            s.trim_write_lrat(lrat)
            s.close()
            print(f"{name} trim with hints (deletions honoured): {dt:.3f} s, {len(res['lemmas'])} of {res['check']['n_lemmas']} lemmas needed, core "
                  f"{len(res['core'])} clauses; LRAT file {os.path.getsize(lrat)} bytes written in {time.time() - t:.3f} s", flush=True)
            for run in range(3):
                device_side(name, f"run {run}", cnf, lrat)
                t = time.time()
                try:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--python-side", str(n), str(k), lrat],
                                         capture_output=True, text=True, timeout=py_limit)
                    print(f"{name} run {run}: python  {out.stdout.strip() or out.stderr.strip()[-300:]}  (process {time.time() - t:.1f} s)", flush=True)
                except subprocess.TimeoutExpired:
                    print(f"{name} run {run}: python  not finished in {py_limit} s", flush=True)
            for run in range(3):          # the other build: the assignment map in HBM (lds_val = -1)
                device_side(name, f"run {run}, lds_val -1", cnf, lrat, lds_val=-1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
