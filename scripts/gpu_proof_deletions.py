"""What honouring deletion lines costs and buys, measured: for each case one solve of the default fleet that
writes its DRUP proof, then mi355sat_check_proof_file on fresh handles with mi355sat_proof_deletions off and on, three runs
each way, alternating: times, the peak of the live lemmas against their number, what the slabs were laid out with, the
segments; then one mi355sat_trim_proof_file with the switch on and the hints kept, and the LRAT file written.  With
--parent-lib PATH (a libmi355sat.so built from the parent commit) the switch-off check is also run through that library,
alternating with this tree's, three runs each: the same kernel build, so the two should sit inside each other's spread.
One process; every call is interrupted after LIMIT_S seconds.  A record, not a gate: a call that ends in an error is
printed and the case goes on.

    python scripts/gpu_proof_deletions.py [--parent-lib PATH] [SIZE:K ...]     (default 16:3 24:8, rect SIZE x SIZE, bound K)
"""
import ctypes
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


def check_parent(name, tag, cnf, proof, lib):
    """The switch-off check through another build of the library, by its C ABI alone (it has no deletions switch to bind)."""
    from timberborn_support_solver_amd.solver import Mi355SatProofInfo
    vp = ctypes.c_void_p
    lib.mi355sat_new.restype = vp
    lib.mi355sat_new.argtypes = [vp]
    lib.mi355sat_free.argtypes = [vp]
    lib.mi355sat_add_cnf.argtypes = [vp, vp, vp, ctypes.c_uint64]
    lib.mi355sat_reserve.argtypes = [vp, ctypes.c_uint64]
    lib.mi355sat_check_proof_file.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(Mi355SatProofInfo)]
    import numpy as np
    lits, offs = np.ascontiguousarray(cnf.lits, dtype=np.int32), np.ascontiguousarray(cnf.offsets, dtype=np.uint64)
    h = lib.mi355sat_new(None)
    try:
        rc = lib.mi355sat_add_cnf(h, lits.ctypes.data, offs.ctypes.data, len(offs) - 1)
        lib.mi355sat_reserve(h, cnf.n_vars)
        info = Mi355SatProofInfo()
        t = time.time()
        rc = rc or lib.mi355sat_check_proof_file(h, proof.encode(), None, 0, 0, ctypes.byref(info))
        dt = time.time() - t
        print(f"{name} {tag}: {dt:.3f} s (kernel {info.kernel_seconds:.3f} s, {info.launches} launches)  rc {rc}  valid {info.valid}  lemmas "
              f"{info.n_lemmas}  deletions ignored {info.n_deletions_ignored}  segments {info.segments}  propagations {info.propagations}",
              flush=True)
    finally:
        lib.mi355sat_free(h)


def check(name, tag, cnf, proof, on):
    s = Mi355Sat()
    try:
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        if on:
            s.set_proof_deletions(True)
        t = time.time()
        info = within(s, lambda: s.check_proof_file(proof))
        dt = time.time() - t
        line = (f"{name} {tag}: {dt:.3f} s (kernel {info['kernel_seconds']:.3f} s, {info['launches']} launches)  valid {info['valid']}  "
                f"first_failed {info['first_failed']}  lemmas {info['n_lemmas']}  deletions ignored {info['n_deletions_ignored']}  "
                f"segments {info['segments']}  propagations {info['propagations']}")
        if on:
            d = s.debug_proof_deletions()
            slab = 4 * d["learnt_lit_cap"] + 16 * d["pool_cap"] + 24 * d["learnt_cap"]
            line += (f"  honoured {d['honoured']}  groups {d['groups']}  peak live {d['peak_live_lemmas']} lemmas / {d['peak_live_words']} words"
                     f"  learnt_cap {d['learnt_cap']}  learnt_lit_cap {d['learnt_lit_cap']}  pool_cap {d['pool_cap']}  (stores + pool "
                     f"{slab / 2 ** 20:.1f} MiB per worker)  skipped_locked {d['skipped_locked']}  compactions {d['compactions']}")
        print(line, flush=True)
    except SolverError as e:              # (a proof the checker's stores do not hold is a finding of this record)
        print(f"{name} {tag}: {e}", flush=True)
    finally:
        s.close()


def trim(name, cnf, proof, lrat):
    s = Mi355Sat()
    try:
        s.add_cnf(cnf.lits, cnf.offsets)
        s.reserve(cnf.n_vars)
        s.set_proof_deletions(True)
        t = time.time()
        res = within(s, lambda: s.trim_proof_file(proof, hints=True))
        dt = time.time() - t
        c = res["check"]
        line = (f"{name} trim, switch on: {dt:.3f} s (kernel {c['kernel_seconds']:.3f} s, {c['launches']} launches)  valid {c['valid']}  "
                f"segments {c['segments']}")
        if c["valid"] == 1:
            s.trim_write_lrat(lrat)
            line += (f"  lemmas needed {len(res['lemmas'])} of {c['n_lemmas']}  core {len(res['core'])} of {len(cnf.offsets) - 1} clauses  "
                     f"records {res['dep_records']}  drains {res['log_drains']}  LRAT file {os.path.getsize(lrat)} bytes")
        print(line, flush=True)
    except SolverError as e:
        print(f"{name} trim, switch on: {e}", flush=True)
    finally:
        s.close()


def main():
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent-lib":
        parent = ctypes.CDLL(args[1])
        args = args[2:]
    cases = [tuple(int(x) for x in a.split(":")) for a in args] or [(16, 3), (24, 8)]
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
            n_del = sum(1 for line in open(proof) if line.startswith("d "))
            print(f"{name}: {cnf.n_vars} variables, {len(cnf.offsets) - 1} clauses; solve {r.name} in {time.time() - t:.3f} s, "
                  f"{st['conflicts']} conflicts, {st['reduce_dbs']} reductions, proof file {os.path.getsize(proof)} bytes, {n_del} deletion lines",
                  flush=True)
            if r != SolverResult.Unsat:
                print(f"{name}: not UNSAT within {LIMIT_S} s - the case ends here", flush=True)
                continue
            for run in range(3):
                if parent is not None:
                    check_parent(name, f"run {run}: parent, off", cnf, proof, parent)
                check(name, f"run {run}: switch off ", cnf, proof, False)
                check(name, f"run {run}: switch on  ", cnf, proof, True)
            trim(name, cnf, proof, os.path.join(d, "t.lrat"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
