"""Python view of the solver boundary (include/mi355sat.h).

`Mi355Sat` mirrors the part of rustsat's `Solve + Interrupt + SolveStats` that
the reference exercises:

    GlucoseSimp::default()            crates/repl/src/main.rs:295      -> Mi355Sat()
    solver.add_cnf(cnf)               crates/repl/src/solver_runner.rs:12
    solver.interrupter()              crates/repl/src/solver_runner.rs:13
    interrupter.interrupt()           crates/repl/src/main.rs:316
    solver.solve() -> SolverResult    crates/repl/src/solver_runner.rs:16
    solver.full_solution()            crates/repl/src/main.rs:329
    solver.stats()                    crates/repl/src/main.rs:363

plus the two batched entry points the sharded sweep and the BCP configuration
use (solve_batch / propagate_batch).  Errors come back as `SolverError`, the
analogue of the reference's `anyhow::Result`.
"""
import ctypes
import enum
import threading

import numpy as np

from . import _lib


class SolverResult(enum.Enum):  # rustsat::solvers::SolverResult
    Sat = 10
    Unsat = 20
    Interrupted = 0


class SolverError(RuntimeError):
    pass


class Mi355SatOpts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("workers", ctypes.c_int32), ("conflict_budget", ctypes.c_int64),
                ("slice_conflicts", ctypes.c_int32), ("seed", ctypes.c_uint64), ("verbose", ctypes.c_int32),
                ("reduce_first", ctypes.c_int32), ("reduce_inc", ctypes.c_int32), ("lds_val", ctypes.c_int32),
                ("max_groups", ctypes.c_int32), ("slice_ms", ctypes.c_int32), ("cube_split", ctypes.c_int32), ("share", ctypes.c_int32), ("share_lbd", ctypes.c_int32), ("share_len", ctypes.c_int32),
                ("share_interval", ctypes.c_int32), ("var_order", ctypes.c_int32), ("ramp", ctypes.c_int32), ("one_per_simd", ctypes.c_int32), ("simp", ctypes.c_int32), ("phase_mix", ctypes.c_int32), ("rephase", ctypes.c_int32), ("restart_k_pct", ctypes.c_int32), ("restart_k2_pct", ctypes.c_int32), ("import_pct", ctypes.c_int32), ("vivify", ctypes.c_int32), ("rebalance", ctypes.c_int32), ("deterministic", ctypes.c_int32)]


class Mi355SatStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("propagations", "decisions", "conflicts", "restarts", "learnts", "learnt_literals",
                 "reduce_dbs", "n_clauses", "max_var")] + \
               [("avg_clause_len", ctypes.c_double), ("solve_seconds", ctypes.c_double),
                ("kernel_seconds", ctypes.c_double), ("kernel_launches", ctypes.c_uint64)] + \
               [(n, ctypes.c_uint64) for n in
                ("n_deq", "n_watch", "n_cl_lit", "n_move", "n_enq", "n_sat", "n_unsat", "n_terminated",
                 "bcp_steps", "bcp_requeued")] + \
               [("shared_exported", ctypes.c_uint64), ("shared_imported", ctypes.c_uint64), ("shared_imported_units", ctypes.c_uint64),
                ("simp_units", ctypes.c_uint64), ("simp_equivalences", ctypes.c_uint64), ("simp_clauses_removed", ctypes.c_uint64),
                ("workers", ctypes.c_uint64), ("simp_eliminated", ctypes.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Mi355SatSearchBuild(ctypes.Structure):   # mi355sat_search_build (test hook)
    _fields_ = [("lds", ctypes.c_int32), ("wps", ctypes.c_int32), ("dyn_lds_bytes", ctypes.c_uint32), ("active", ctypes.c_uint32),
                ("lds_val_bytes", ctypes.c_uint32), ("builds_seen", ctypes.c_uint32), ("launches", ctypes.c_uint64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        # every (lds, wps) the handle has launched so far
        d["builds"] = {(l, w) for l in (0, 1) for i, w in enumerate((1, 2, 4)) if d["builds_seen"] >> (3 * l + i) & 1}
        return d


class Mi355SatIncrementalInfo(ctypes.Structure):   # mi355sat_incremental_info (test hook)
    _fields_ = [("enabled", ctypes.c_int32), ("last_cold_reason", ctypes.c_int32)] + \
               [(n, ctypes.c_uint64) for n in ("warm_solves", "cold_solves", "attached_clauses", "attached_units",
                                               "resident_learnts", "attach_launches")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Mi355SatHeuristicsInfo(ctypes.Structure):   # mi355sat_heuristics_info (test hook)
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_vivified", "n_viv_lits", "n_rephase", "import_skipped", "forced_imports")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Mi355SatCapacityInfo(ctypes.Structure):   # mi355sat_capacity_info (test hook)
    _fields_ = [(n, ctypes.c_uint32) for n in ("learnt_cap", "learnt_lit_cap", "pool_cap", "pool_initial", "proof_cap", "assump_cap",
                                               "vm_cap", "pad")] + \
               [(n, ctypes.c_uint64) for n in ("pressure_reduces", "pool_rebuilds", "imports_dropped_full")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class Mi355SatPhaseInfo(ctypes.Structure):   # mi355sat_phase_info (test hook)
    _fields_ = [(n, ctypes.c_uint64) for n in ("hinted", "applied_cold", "applied_warm", "launches", "mapped",
                                               "dropped_eliminated", "dropped_fixed")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Mi355SatCoreMinInfo(ctypes.Structure):   # mi355sat_core_min_info
    _fields_ = [("size_before", ctypes.c_uint64), ("size_after", ctypes.c_uint64), ("minimal", ctypes.c_int32),
                ("rounds", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("candidates", "candidates_unsat", "candidates_sat", "critical_by_model",
                                               "model_launches", "conflicts")] + [("seconds", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Mi355SatProofInfo(ctypes.Structure):   # mi355sat_proof_info
    _fields_ = [("valid", ctypes.c_int32), ("pad", ctypes.c_int32)] + \
               [(n, ctypes.c_uint64) for n in ("n_lemmas", "n_deletions_ignored", "first_failed", "refuted_at", "segments",
                                               "workers", "lemmas_checked", "lemmas_attached", "propagations", "launches")] + \
               [("seconds", ctypes.c_double), ("kernel_seconds", ctypes.c_double)]

    def as_dict(self):
        """first_failed / refuted_at: None where the C struct says UINT64_MAX (no such lemma); interrupted: the check was
        stopped and there is no verdict (valid = -1)."""
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}
        for k in ("first_failed", "refuted_at"):
            if d[k] == 2 ** 64 - 1:
                d[k] = None
        d["interrupted"] = d["valid"] < 0
        return d


class Mi355SatProofLogInfo(ctypes.Structure):   # mi355sat_proof_log_info
    _fields_ = [(n, ctypes.c_uint64) for n in ("drains", "gathers", "logs", "words", "core_lines")] + [("drain_seconds", ctypes.c_double)]


class Mi355SatTrimInfo(ctypes.Structure):   # mi355sat_trim_info
    _fields_ = [("check", Mi355SatProofInfo)] + \
               [(n, ctypes.c_uint64) for n in ("core_clauses", "lemmas_needed", "dep_records", "log_drains", "log_words_per_worker")]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "check"}
        d["check"] = self.check.as_dict()
        return d


class Mi355SatProofDelInfo(ctypes.Structure):   # mi355sat_proof_del_info
    _fields_ = [(n, ctypes.c_uint64) for n in ("honoured", "ignored_original", "ignored_unmatched", "groups", "peak_live_lemmas",
                                               "peak_live_words", "learnt_cap", "learnt_lit_cap", "pool_cap", "skipped_locked",
                                               "compactions")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LratReason(enum.IntEnum):  # MI355SAT_LRAT_*: why check_lrat rejected a line
    NONE = 0
    ID_ORDER = 1
    TAUTOLOGY = 2
    NO_HINTS = 3
    BAD_HINT = 4
    HINT_SATISFIED = 5
    HINT_NOT_UNIT = 6
    HINT_FALSIFIED_EARLY = 7
    LAST_NOT_FALSIFIED = 8


class Mi355SatLratInfo(ctypes.Structure):   # mi355sat_lrat_info
    _fields_ = [(n, ctypes.c_int32) for n in ("valid", "accepted", "derives_target", "reason")] + \
               [(n, ctypes.c_uint64) for n in ("n_lines", "n_hints", "first_rejected", "first_rejected_id", "reject_hint",
                                               "used_originals", "longest_clause")] + \
               [("lds", ctypes.c_int32), ("dyn_lds_bytes", ctypes.c_uint32), ("waves", ctypes.c_uint64), ("launches", ctypes.c_uint64),
                ("seconds", ctypes.c_double), ("kernel_seconds", ctypes.c_double)]

    def as_dict(self):
        """first_rejected / first_rejected_id / reject_hint: None where there is none; interrupted: the check was stopped
        and there is no verdict (accepted = -1)."""
        d = {n: getattr(self, n) for n, _ in self._fields_}
        if d["first_rejected"] == 2 ** 64 - 1:
            d["first_rejected"] = d["first_rejected_id"] = None
        if d["reject_hint"] == 2 ** 64 - 1:
            d["reject_hint"] = None
        d["interrupted"] = d["accepted"] < 0
        return d


TRIM_HINTS = 1   # MI355SAT_TRIM_HINTS


class ColdReason(enum.IntEnum):  # MI355SAT_COLD_*: why a solve() with the incremental mode on started cold
    NONE = 0
    FIRST = 1
    NEW_VAR = 2
    ELIMINATED = 3
    PROOF = 4
    CUBE_SPLIT = 5
    PINNED_SHARE = 6
    OTHER_SEARCH = 7
    ASSUMP_CAP = 8
    DEVICE_FULL = 9


def algorithmic_bytes(stats):
    """12*n_deq + 9*n_watch + 5*n_cl_lit + 8*n_move + 13*n_enq."""
    return (12 * stats["n_deq"] + 9 * stats["n_watch"] + 5 * stats["n_cl_lit"] + 8 * stats["n_move"]
            + 13 * stats["n_enq"])


def _bind(L):
    vp = ctypes.c_void_p
    L.mi355sat_abi_sizes.restype = ctypes.c_uint64
    L.mi355sat_abi_sizes.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    st_size = ctypes.c_uint64(0)
    if (L.mi355sat_abi_sizes(ctypes.byref(st_size)), st_size.value) != (ctypes.sizeof(Mi355SatOpts), ctypes.sizeof(Mi355SatStats)):
        raise RuntimeError("libmi355sat was built from another include/mi355sat.h than this binding mirrors (struct sizes differ)")
    L.mi355sat_new.restype = vp
    L.mi355sat_new.argtypes = [ctypes.POINTER(Mi355SatOpts)]
    L.mi355sat_free.argtypes = [vp]
    L.mi355sat_signature.restype = ctypes.c_char_p
    L.mi355sat_last_error.restype = ctypes.c_char_p
    L.mi355sat_last_error.argtypes = [vp]
    L.mi355sat_add_cnf.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.mi355sat_add.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_reserve.argtypes = [vp, ctypes.c_uint64]
    L.mi355sat_solve.argtypes = [vp]
    L.mi355sat_assume.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_failed.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_core.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_core_of.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_minimize_core.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(Mi355SatCoreMinInfo)]
    L.mi355sat_minimize_core_of.argtypes = [vp, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(Mi355SatCoreMinInfo)]
    L.mi355sat_debug_core_min_round.argtypes = [vp, ctypes.c_uint32]
    L.mi355sat_solve_batch.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_int]
    L.mi355sat_sweep_begin.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.mi355sat_sweep_step.argtypes = [vp, vp, vp]
    L.mi355sat_sweep_end.argtypes = [vp]
    L.mi355sat_sweep_drop.argtypes = [vp, vp, ctypes.c_uint64]
    L.mi355sat_sweep_reopen.argtypes = [vp, vp, ctypes.c_uint64]
    L.mi355sat_sweep_set_weights.argtypes = [vp, vp, ctypes.c_uint64]
    L.mi355sat_sweep_model_of.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    L.mi355sat_propagate_batch.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, ctypes.c_int32]
    L.mi355sat_val.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_val.restype = ctypes.c_int32
    L.mi355sat_model.argtypes = [vp, vp, ctypes.c_uint64]
    L.mi355sat_model_of.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    L.mi355sat_interrupt.argtypes = [vp]
    L.mi355sat_stats.argtypes = [vp, ctypes.POINTER(Mi355SatStats)]
    L.mi355sat_set_proof_path.argtypes = [vp, ctypes.c_char_p]
    L.mi355sat_debug_share_ring.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_debug_keep_simplified.argtypes = [vp, ctypes.c_int]
    L.mi355sat_debug_simplified.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_debug_last_search_build.argtypes = [vp, ctypes.POINTER(Mi355SatSearchBuild)]
    L.mi355sat_debug_search_build_rule.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.POINTER(Mi355SatSearchBuild)]
    L.mi355sat_check_proof.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(Mi355SatProofInfo)]
    L.mi355sat_check_proof_file.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(Mi355SatProofInfo)]
    L.mi355sat_check_proof_targets.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp,
                                               ctypes.POINTER(Mi355SatProofInfo)]
    L.mi355sat_check_proof_targets_file.argtypes = [vp, ctypes.c_char_p, vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp,
                                                    ctypes.POINTER(Mi355SatProofInfo)]
    L.mi355sat_sweep_core_of.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_debug_proof_log.argtypes = [vp, ctypes.POINTER(Mi355SatProofLogInfo)]
    L.mi355sat_debug_proof_check_chunk.argtypes = [vp, ctypes.c_uint32]
    L.mi355sat_proof_deletions.argtypes = [vp, ctypes.c_int]
    L.mi355sat_debug_proof_deletions.argtypes = [vp, ctypes.POINTER(Mi355SatProofDelInfo)]
    L.mi355sat_trim_proof.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.POINTER(Mi355SatTrimInfo)]
    L.mi355sat_trim_proof_file.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(Mi355SatTrimInfo)]
    L.mi355sat_trim_core.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_trim_lemmas.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_trim_write_drup.argtypes = [vp, ctypes.c_char_p]
    L.mi355sat_trim_write_lrat.argtypes = [vp, ctypes.c_char_p]
    L.mi355sat_debug_trim_log.argtypes = [vp, ctypes.c_uint32]
    L.mi355sat_check_lrat.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(Mi355SatLratInfo)]
    L.mi355sat_check_lrat_file.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_uint64, ctypes.POINTER(Mi355SatLratInfo)]
    L.mi355sat_lrat_used.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_debug_lrat_chunk.argtypes = [vp, ctypes.c_uint32]
    L.mi355sat_set_incremental.argtypes = [vp, ctypes.c_int]
    L.mi355sat_debug_incremental.argtypes = [vp, ctypes.POINTER(Mi355SatIncrementalInfo)]
    L.mi355sat_debug_heuristics.argtypes = [vp, ctypes.POINTER(Mi355SatHeuristicsInfo)]
    L.mi355sat_debug_set_schedule.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.mi355sat_debug_set_capacities.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.mi355sat_debug_capacities.argtypes = [vp, ctypes.POINTER(Mi355SatCapacityInfo)]
    L.mi355sat_phase.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_unphase.argtypes = [vp, ctypes.c_int32]
    L.mi355sat_set_phases.argtypes = [vp, vp, ctypes.c_uint64]
    L.mi355sat_debug_phases.argtypes = [vp, ctypes.POINTER(Mi355SatPhaseInfo)]
    L.mi355sat_share_export.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.mi355sat_share_import.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    return L


_bound = {}


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


class Interrupter:
    """`S::Interrupter`: Send + 'static, callable from another thread while solve() runs."""

    def __init__(self, lib, handle_ref, lock):
        self._lib, self._ref, self._lock = lib, handle_ref, lock

    def interrupt(self):
        with self._lock:   # close() clears the reference under the same lock before it frees the handle
            h = self._ref[0]
            if h:
                self._lib.mi355sat_interrupt(h)


class Mi355Sat:
    def __init__(self, device=-1, workers=0, conflict_budget=0, slice_conflicts=0, seed=0, verbose=0,
                 reduce_first=0, reduce_inc=0, lds_val=0, max_groups=0, slice_ms=0, cube_split=0, share=0, share_lbd=0, share_len=0, share_interval=0, rebalance=0, var_order=0, ramp=0, one_per_simd=0, simp=0, phase_mix=0, rephase=0, restart_k_pct=0, restart_k2_pct=0, import_pct=0, vivify=0, deterministic=0, _lib_override=None):
        # _lib_override: test hook (the wavefront-emulator build under tests/emu); the product
        # always binds the HIP library and fails loudly without it.
        raw = _lib_override if _lib_override is not None else _lib.solver_lib()
        if id(raw) not in _bound:
            _bound[id(raw)] = _bind(raw)
        self._L = _bound[id(raw)]
        opts = Mi355SatOpts(device=device, workers=workers, conflict_budget=conflict_budget,
                            slice_conflicts=slice_conflicts, seed=seed, verbose=verbose,
                            reduce_first=reduce_first, reduce_inc=reduce_inc, lds_val=lds_val, max_groups=max_groups, slice_ms=slice_ms, cube_split=cube_split, share=share, share_lbd=share_lbd, share_len=share_len, share_interval=share_interval, rebalance=rebalance, var_order=var_order, ramp=ramp, one_per_simd=one_per_simd, simp=simp, phase_mix=phase_mix, rephase=rephase, restart_k_pct=restart_k_pct, restart_k2_pct=restart_k2_pct, import_pct=import_pct, vivify=vivify, deterministic=deterministic)
        self._h = self._L.mi355sat_new(ctypes.byref(opts))
        if not self._h:
            raise SolverError("mi355sat_new failed: " + (self._L.mi355sat_last_error(None) or b"").decode())
        self._ref = [self._h]
        self._lock = threading.Lock()
        self._n_vars = 0

    def close(self):
        if getattr(self, "_h", None):
            with self._lock:   # no interrupter may still be inside mi355sat_interrupt(), none may enter afterwards
                self._ref[0] = None
            self._L.mi355sat_free(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            e = SolverError(f"{what} failed ({rc}): " + (self._L.mi355sat_last_error(self._h) or b"").decode())
            e.code = rc     # the MI355SAT_ERR_* value
            raise e
        return rc

    @staticmethod
    def signature():
        return _bind(_lib.solver_lib()).mi355sat_signature().decode()

    # ---- Solve
    def add_cnf(self, lits, offsets):
        lits = np.ascontiguousarray(lits, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self._L.mi355sat_add_cnf(self._h, _p(lits), _p(offsets), len(offsets) - 1), "add_cnf")
        if lits.size:
            self._n_vars = max(self._n_vars, int(np.abs(lits).max()))

    def add_clause(self, clause):
        for l in clause:
            self._check(self._L.mi355sat_add(self._h, int(l)), "add")
            self._n_vars = max(self._n_vars, abs(int(l)))
        self._check(self._L.mi355sat_add(self._h, 0), "add")

    def reserve(self, n_vars):
        self._check(self._L.mi355sat_reserve(self._h, n_vars), "reserve")
        self._n_vars = max(self._n_vars, n_vars)

    def interrupter(self):
        return Interrupter(self._L, self._ref, self._lock)

    def solve(self, assumptions=()):
        """Solve (rustsat `solve`), or under DIMACS assumption literals that hold for this call only (`solve_assumps`)."""
        for l in assumptions:
            self.assume(l)
        return SolverResult(self._check(self._L.mi355sat_solve(self._h), "solve"))

    # ---- SolveIncremental (IPASIR assume / failed)
    def assume(self, lit):
        """Assumption for the next solve() only."""
        self._check(self._L.mi355sat_assume(self._h, int(lit)), "assume")
        self._n_vars = max(self._n_vars, abs(int(lit)))

    def failed(self, lit):
        """After solve() returned Unsat: whether assumption `lit` is in the core."""
        return self._check(self._L.mi355sat_failed(self._h, int(lit)), "failed") == 1

    def _core(self, fn, *args):
        n = ctypes.c_uint64(0)
        self._check(fn(self._h, *args, None, 0, ctypes.byref(n)), "core")
        out = np.zeros(n.value, dtype=np.int32)
        self._check(fn(self._h, *args, _p(out), n.value, ctypes.byref(n)), "core")
        return [int(l) for l in out[:n.value]]

    def core(self):
        """After solve() returned Unsat: the assumptions (DIMACS literals, in the order given) the refutation rests on;
        formula AND core is UNSAT.  Raises SolverError in any other state."""
        return self._core(self._L.mi355sat_core)

    def core_of(self, instance):
        """The same for an Unsat instance of the last solve_batch()."""
        return self._core(self._L.mi355sat_core_of, instance)

    def minimize_core(self, conflict_budget=0):
        """After solve() returned Unsat: shrink the core until no literal can be left out (deletion by rounds of
        candidates, side by side on the device: include/mi355sat.h); core() / failed() answer with the new core.
        conflict_budget > 0 bounds the conflicts summed over workers.  Returns mi355sat_core_min_info as a dict; its
        "minimal" is 0 if the budget or an interrupt ended the call early (the core is still a core then)."""
        info = Mi355SatCoreMinInfo()
        self._check(self._L.mi355sat_minimize_core(self._h, int(conflict_budget), ctypes.byref(info)), "minimize_core")
        return info.as_dict()

    def minimize_core_of(self, instance, conflict_budget=0):
        """The same for an Unsat instance of the last solve_batch(); core_of(instance) answers with the new core."""
        info = Mi355SatCoreMinInfo()
        self._check(self._L.mi355sat_minimize_core_of(self._h, int(instance), int(conflict_budget), ctypes.byref(info)),
                    "minimize_core_of")
        return info.as_dict()

    def debug_core_min_round(self, max_candidates=0):
        """Test hook: at most max_candidates candidates per round of minimize_core (0 = the default)."""
        self._check(self._L.mi355sat_debug_core_min_round(self._h, int(max_candidates)), "debug_core_min_round")

    # ---- certificates: DRUP proofs checked on the device (include/mi355sat.h)
    def check_proof(self, proof, target=(), segments=0):
        """Forward RUP check (deletion lines ignored unless set_proof_deletions() is on) of `proof` - flat int32, lemmas 0-terminated, as dimacs.read_drup
        returns it - against this handle's clauses; `target` is the clause it must derive (default: the empty clause; for
        a solve under assumptions the negated core).  segments: into how many parts the lemma list is cut, one wavefront
        each (0 = the default); the verdict does not depend on it.  Returns mi355sat_proof_info as a dict: "valid" is the
        verdict, "first_failed" / "refuted_at" are None where there is no such lemma, "interrupted" is True (and "valid"
        -1) if an interrupt ended the check."""
        pr = np.ascontiguousarray(proof, dtype=np.int32)
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatProofInfo()
        self._check(self._L.mi355sat_check_proof(self._h, _p(pr), pr.size, _p(tg), tg.size, int(segments), ctypes.byref(info)),
                    "check_proof")
        return info.as_dict()

    def check_proof_file(self, path, target=(), segments=0):
        """The same for a DRUP text file as set_proof_path() writes it."""
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatProofInfo()
        self._check(self._L.mi355sat_check_proof_file(self._h, str(path).encode(), _p(tg), tg.size, int(segments),
                                                      ctypes.byref(info)), "check_proof_file")
        return info.as_dict()

    @staticmethod
    def _target_lists(targets):
        targets = [list(t) for t in targets]
        offs = np.zeros(len(targets) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(t) for t in targets])
        flat = np.asarray([l for t in targets for l in t], dtype=np.int32)
        return flat, offs, np.zeros(max(1, len(targets)), dtype=np.int32)

    def check_proof_targets(self, proof, targets, segments=0):
        """check_proof() for several targets in one pass - what certifies every UNSAT verdict of a batch or a sweep from
        the one file it logged: `targets` is a list of clauses, each checked against the formula and ALL lemmas of `proof`
        (targets do not see each other).  Returns check_proof's dict ("valid": every lemma and every target passes;
        "first_failed" counts target t as n_lemmas + t) plus "target_valid": per target 1 (RUP, a tautology, or the
        database is refuted by then), 0, or -1 after an interrupt."""
        pr = np.ascontiguousarray(proof, dtype=np.int32)
        flat, offs, valid = self._target_lists(targets)
        info = Mi355SatProofInfo()
        self._check(self._L.mi355sat_check_proof_targets(self._h, _p(pr), pr.size, _p(flat), _p(offs), len(offs) - 1, int(segments),
                                                         _p(valid), ctypes.byref(info)), "check_proof_targets")
        return dict(info.as_dict(), target_valid=[int(v) for v in valid[:len(offs) - 1]])

    def check_proof_targets_file(self, path, targets, segments=0):
        """The same for a DRUP text file as set_proof_path() writes it."""
        flat, offs, valid = self._target_lists(targets)
        info = Mi355SatProofInfo()
        self._check(self._L.mi355sat_check_proof_targets_file(self._h, str(path).encode(), _p(flat), _p(offs), len(offs) - 1,
                                                              int(segments), _p(valid), ctypes.byref(info)), "check_proof_targets_file")
        return dict(info.as_dict(), target_valid=[int(v) for v in valid[:len(offs) - 1]])

    def debug_proof_log(self):
        """Test hook: mi355sat_proof_log_info of the proof file open now or closed last, as a dict."""
        info = Mi355SatProofLogInfo()
        self._check(self._L.mi355sat_debug_proof_log(self._h, ctypes.byref(info)), "debug_proof_log")
        return {n: getattr(info, n) for n, _ in info._fields_}

    def debug_proof_check_chunk(self, max_lemmas_per_launch=0):
        """Test hook: at most this many lemmas per worker and launch of check_proof (0 = the default, time-bounded)."""
        self._check(self._L.mi355sat_debug_proof_check_chunk(self._h, int(max_lemmas_per_launch)), "debug_proof_check_chunk")

    def set_proof_deletions(self, on=True):
        """Honour the proof's deletion lines in check_proof / trim_proof and their _file forms (off by default: they are
        counted and ignored).  A worker then holds only the live lemmas, its stores are sized from their peak, and a proof
        that uses a lemma after deleting it is not valid.  The semantics: include/mi355sat.h, mi355sat_proof_deletions."""
        self._check(self._L.mi355sat_proof_deletions(self._h, 1 if on else 0), "set_proof_deletions")

    def debug_proof_deletions(self):
        """mi355sat_proof_del_info of the last check or trim made with set_proof_deletions() on, as a dict (SolverError
        ERR_STATE before the first one).  skipped_locked and compactions may differ from cut to cut and run to run."""
        info = Mi355SatProofDelInfo()
        self._check(self._L.mi355sat_debug_proof_deletions(self._h, ctypes.byref(info)), "debug_proof_deletions")
        return info.as_dict()

    # ---- trimmed proofs: the clause core, the needed lemmas, LRAT (include/mi355sat.h)
    def _indices(self, fn, what):
        n = ctypes.c_uint64(0)
        self._check(fn(self._h, None, 0, ctypes.byref(n)), what)
        out = np.zeros(n.value, dtype=np.uint64)
        self._check(fn(self._h, _p(out), n.value, ctypes.byref(n)), what)
        return [int(i) for i in out[:n.value]]

    def trim_core(self):
        """After a trim_proof() that found the proof valid: the 0-based indices of this handle's clauses the derivation of
        the target rests on, ascending.  Raises SolverError (ERR_STATE) in any other state."""
        return self._indices(self._L.mi355sat_trim_core, "trim_core")

    def trim_lemmas(self):
        """... and the 0-based indices of the lemmas it needs, ascending."""
        return self._indices(self._L.mi355sat_trim_lemmas, "trim_lemmas")

    def _trimmed(self, info):
        d = info.as_dict()
        valid = d["check"]["valid"] == 1
        d["core"] = self.trim_core() if valid else None
        d["lemmas"] = self.trim_lemmas() if valid else None
        return d

    def trim_proof(self, proof, target=(), segments=0, hints=False):
        """check_proof() in the tracing build of the checker: "check" is check_proof's dict for the same inputs; where it
        says valid, "core" and "lemmas" are the clauses of this handle and the lemmas of the proof that the derivation of
        `target` rests on (None otherwise).  hints = True keeps what trim_write_lrat() needs.  Which clauses make the core
        may differ with `segments` and from run to run; the verdict does not."""
        pr = np.ascontiguousarray(proof, dtype=np.int32)
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatTrimInfo()
        self._check(self._L.mi355sat_trim_proof(self._h, _p(pr), pr.size, _p(tg), tg.size, int(segments),
                                                TRIM_HINTS if hints else 0, ctypes.byref(info)), "trim_proof")
        return self._trimmed(info)

    def trim_proof_file(self, path, target=(), segments=0, hints=False):
        """The same for a DRUP text file as set_proof_path() writes it."""
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatTrimInfo()
        self._check(self._L.mi355sat_trim_proof_file(self._h, str(path).encode(), _p(tg), tg.size, int(segments),
                                                     TRIM_HINTS if hints else 0, ctypes.byref(info)), "trim_proof_file")
        return self._trimmed(info)

    def trim_write_drup(self, path):
        """The needed lemmas in order, then the target, as DRUP text."""
        self._check(self._L.mi355sat_trim_write_drup(self._h, str(path).encode()), "trim_write_drup")

    def trim_write_lrat(self, path):
        """The same lines as LRAT: clause i of this handle has id i + 1, lemma j has n_clauses + 1 + j.  Needs hints = True."""
        self._check(self._L.mi355sat_trim_write_lrat(self._h, str(path).encode()), "trim_write_lrat")

    def debug_trim_log(self, words=0):
        """Test hook: words per worker of trim_proof's dependency log (0 = the rule; never below two items of the largest size)."""
        self._check(self._L.mi355sat_debug_trim_log(self._h, int(words)), "debug_trim_log")

    # ---- LRAT files checked on the device (include/mi355sat.h)
    def check_lrat(self, lines, target=()):
        """Strict LRAT check of `lines` - flat int32, `id, literals, 0, hints, 0` per line - against this handle's clauses
        (clause i, 0-based, has id i + 1); `target` is the clause the last line must be (default: the empty clause).
        Returns mi355sat_lrat_info as a dict: "accepted" 1 / 0 / -1 (interrupted), "valid" = accepted and the target
        derived, "first_rejected" / "reason" (LratReason) / "reject_hint" of the first rejected line, None where there is
        none.  What is not LRAT at all raises SolverError (ERR_ARG)."""
        ln = np.ascontiguousarray(lines, dtype=np.int32)
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatLratInfo()
        self._check(self._L.mi355sat_check_lrat(self._h, _p(ln), ln.size, _p(tg), tg.size, ctypes.byref(info)), "check_lrat")
        return info.as_dict()

    def check_lrat_file(self, path, target=()):
        """The same for an LRAT text file as trim_write_lrat() writes it."""
        tg = np.ascontiguousarray(list(target), dtype=np.int32)
        info = Mi355SatLratInfo()
        self._check(self._L.mi355sat_check_lrat_file(self._h, str(path).encode(), _p(tg), tg.size, ctypes.byref(info)),
                    "check_lrat_file")
        return info.as_dict()

    def lrat_used(self):
        """After a check_lrat() that accepted every line: the 0-based indices of this handle's clauses some line hinted,
        ascending.  Raises SolverError (ERR_STATE) in any other state."""
        return self._indices(self._L.mi355sat_lrat_used, "lrat_used")

    def debug_lrat_chunk(self, max_lines_per_launch=0):
        """Test hook: at most this many lines per launch of check_lrat (0 = the default)."""
        self._check(self._L.mi355sat_debug_lrat_chunk(self._h, int(max_lines_per_launch)), "debug_lrat_chunk")

    # ---- phase hints (rustsat PhaseLit's place; seeded, not forced: include/mi355sat.h)
    def phase(self, lit):
        """Hint: the first time var(lit) is decided, it is decided as lit.  Seeds the workers' saved phase at the next
        solve; phase saving takes over from there.  Kept until unphase()."""
        self._check(self._L.mi355sat_phase(self._h, int(lit)), "phase")
        self._n_vars = max(self._n_vars, abs(int(lit)))

    def unphase(self, var):
        """Drop the hint of variable `var`."""
        self._check(self._L.mi355sat_unphase(self._h, int(var)), "unphase")

    def set_phases(self, phases):
        """Bulk hints for variables 1..len(phases): > 0 TRUE first, < 0 FALSE first, 0 none (clears one) - a model as
        full_solution() returns it is a valid argument."""
        ph = np.ascontiguousarray(np.sign(np.asarray(phases)), dtype=np.int8)
        self._check(self._L.mi355sat_set_phases(self._h, _p(ph), len(ph)), "set_phases")
        nz = np.flatnonzero(ph)
        if nz.size:
            self._n_vars = max(self._n_vars, int(nz[-1]) + 1)

    def debug_phases(self):
        """Test hook: hinted variables now; cold / warm starts that seeded their workers; ms_phase_kernel launches; at the
        last application the device variables seeded per worker and the hints dropped (eliminated / fixed variables)."""
        info = Mi355SatPhaseInfo()
        self._check(self._L.mi355sat_debug_phases(self._h, ctypes.byref(info)), "debug_phases")
        return info.as_dict()

    def solve_batch(self, assumption_sets, stop_at_first=False):
        """assumption_sets: list of lists of DIMACS literals.  Returns [SolverResult]."""
        offs = np.zeros(len(assumption_sets) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(a) for a in assumption_sets])
        flat = np.asarray([l for a in assumption_sets for l in a], dtype=np.int32)
        res = np.zeros(len(assumption_sets), dtype=np.int32)
        self._check(self._L.mi355sat_solve_batch(self._h, _p(flat), _p(offs), len(assumption_sets), _p(res),
                                                 1 if stop_at_first else 0), "solve_batch")
        return [SolverResult(int(r)) for r in res]

    # stepwise form of solve_batch (one kernel slice per step); bench.py times these
    def sweep_begin(self, assumption_sets):
        offs = np.zeros(len(assumption_sets) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(a) for a in assumption_sets])
        flat = np.asarray([l for a in assumption_sets for l in a], dtype=np.int32)
        self._sweep_n = len(assumption_sets)
        self._check(self._L.mi355sat_sweep_begin(self._h, _p(flat), _p(offs), self._sweep_n), "sweep_begin")

    def sweep_step(self):
        """Returns ([SolverResult per instance], n_decided)."""
        res = np.zeros(self._sweep_n, dtype=np.int32)
        nd = ctypes.c_uint64(0)
        self._check(self._L.mi355sat_sweep_step(self._h, _p(res), ctypes.byref(nd)), "sweep_step")
        return [SolverResult(int(r)) for r in res], nd.value

    def sweep_drop(self, instances):
        """Withdraw instances (their answer is implied); their workers join the open ones."""
        idx = np.asarray(list(instances), dtype=np.uint64)
        if len(idx):
            self._check(self._L.mi355sat_sweep_drop(self._h, _p(idx), len(idx)), "sweep_drop")

    def sweep_set_weights(self, weights):
        """Share of the fleet per instance (only the open ones count); takes effect at the next step."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._check(self._L.mi355sat_sweep_set_weights(self._h, _p(w), len(w)), "sweep_set_weights")

    def sweep_reopen(self, instances):
        """Take withdrawn, still undecided instances up again (idle workers move to them)."""
        idx = np.asarray(list(instances), dtype=np.uint64)
        if len(idx):
            self._check(self._L.mi355sat_sweep_reopen(self._h, _p(idx), len(idx)), "sweep_reopen")

    def sweep_solution_of(self, instance, n_vars=None):
        """Model of an instance that already reported Sat, while the sweep is running."""
        n_vars = self._n_vars if n_vars is None else n_vars
        out = np.zeros(n_vars, dtype=np.int8)
        self._check(self._L.mi355sat_sweep_model_of(self._h, instance, _p(out), n_vars), "sweep_solution_of")
        return out

    def sweep_core_of(self, instance):
        """The core of an instance that already reported Unsat, while a sweep that logs a proof (set_proof_path) is
        running; SolverError in any other state - a sweep computes cores only for its proof's sake."""
        return self._core(self._L.mi355sat_sweep_core_of, instance)

    def sweep_end(self):
        self._check(self._L.mi355sat_sweep_end(self._h), "sweep_end")

    def propagate_batch(self, decision_sets, n_vars=None, repeat=1, want_values=True):
        """Scripted BCP: returns (conflict int32[n], values int8[n, n_vars] or None, trail_len int32[n])."""
        n = len(decision_sets)
        n_vars = self._n_vars if n_vars is None else n_vars
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(a) for a in decision_sets])
        flat = np.asarray([l for a in decision_sets for l in a], dtype=np.int32)
        confl = np.zeros(n, dtype=np.int32)
        tl = np.zeros(n, dtype=np.int32)
        vals = np.zeros((n, n_vars), dtype=np.int8) if want_values else None
        self._check(self._L.mi355sat_propagate_batch(self._h, _p(flat), _p(offs), n, _p(vals) if want_values else None,
                                                     n_vars, _p(confl), _p(tl), repeat), "propagate_batch")
        return confl, vals, tl

    def debug_share_ring(self):
        """Test hook: the clauses in the learnt-clause exchange ring, as lists of DIMACS literals."""
        n = ctypes.c_uint64(0)
        cap = 1 << 16
        while True:
            buf = np.zeros(cap, dtype=np.int32)
            rc = self._L.mi355sat_debug_share_ring(self._h, _p(buf), cap, ctypes.byref(n))
            if rc == -4:
                cap *= 4
                continue
            self._check(rc, "debug_share_ring")
            break
        out, cur = [], []
        for l in buf.tolist():
            if len(out) == n.value:
                break
            if l == 0:
                out.append(cur)
                cur = []
            else:
                cur.append(l)
        return out

    def debug_keep_simplified(self, on=True):
        """Test hook: keep a copy of what the simplification before search leaves, from the next solve / batch on."""
        self._check(self._L.mi355sat_debug_keep_simplified(self._h, 1 if on else 0), "debug_keep_simplified")

    def debug_simplified(self):
        """Test hook: (clauses, elim_clauses) of the last solve with debug_keep_simplified() armed, as lists of DIMACS
        literals in the caller's variables: the formula the workers received (remaining clauses, level-0 facts as units,
        both binaries of every substitution; the empty clause [] among them if it was refuted), and the clauses kept for the eliminated variables."""
        lists = []
        for which in (0, 1):
            nw, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
            self._check(self._L.mi355sat_debug_simplified(self._h, which, None, 0, ctypes.byref(nw), ctypes.byref(nc)), "debug_simplified")
            buf = np.zeros(max(nw.value, 1), dtype=np.int32)
            self._check(self._L.mi355sat_debug_simplified(self._h, which, _p(buf), nw.value, ctypes.byref(nw), ctypes.byref(nc)), "debug_simplified")
            out, cur = [], []
            for l in buf[:nw.value].tolist():
                if l == 0:
                    out.append(cur)
                    cur = []
                else:
                    cur.append(l)
            assert not cur and len(out) == nc.value
            lists.append(out)
        return tuple(lists)

    def debug_last_search_build(self):
        """Test hook: the build of the search kernel this handle's last search launch ran, as a dict (lds 0/1, wps 1/2/4,
        dyn_lds_bytes, active, lds_val_bytes, launches, builds = every (lds, wps) launched so far)."""
        b = Mi355SatSearchBuild()
        self._check(self._L.mi355sat_debug_last_search_build(self._h, ctypes.byref(b)), "debug_last_search_build")
        return b.as_dict()

    @staticmethod
    def debug_search_build_rule(active, lds_val_bytes, lds_val=0, one_per_simd=0, mode=0, staged=-1, _lib_override=None):
        """Test hook: the selection rule alone (nothing is launched): the build a launch of `active` workers would run."""
        raw = _lib_override if _lib_override is not None else _lib.solver_lib()
        if id(raw) not in _bound:
            _bound[id(raw)] = _bind(raw)
        b = Mi355SatSearchBuild()
        rc = _bound[id(raw)].mi355sat_debug_search_build_rule(active, lds_val_bytes, staged, lds_val, one_per_simd, mode, ctypes.byref(b))
        if rc < 0:
            raise SolverError(f"debug_search_build_rule failed ({rc})")
        return b.as_dict()

    def share_export(self, max_words=1 << 20):
        """The clauses this handle's workers passed on since the last call, for handles on OTHER GPUs that search the same
        formula: int32 array of [lbd, DIMACS literals ..., 0] records (caller's variables); what does not fit max_words waits."""
        buf = np.zeros(max_words, dtype=np.int32)
        nw, nr = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._L.mi355sat_share_export(self._h, _p(buf), max_words, ctypes.byref(nw), ctypes.byref(nr)), "share_export")
        return buf[:nw.value].copy(), nr.value

    def share_import(self, records):
        """Append records exported by another handle (share_export's format) to this handle's exchange ring; returns how
        many were taken."""
        records = np.ascontiguousarray(records, dtype=np.int32)
        nr = ctypes.c_uint64(0)
        self._check(self._L.mi355sat_share_import(self._h, _p(records), len(records), ctypes.byref(nr)), "share_import")
        return nr.value

    def set_proof_path(self, path):
        """DRUP proof of the next solve(), solve_batch() or sweep_begin() .. sweep_end(), in its default configuration: all
        workers, clause exchange on (one log per worker, drained after every slice with one kernel and one copy).  A batch
        or a sweep writes ONE file: the lemmas of all workers of all instances, and behind the slice that decides an
        instance Unsat the clause of its negated core (core_of / sweep_core_of), so that check_proof_targets_file() with
        the negated cores as targets certifies every Unsat verdict in one pass and trim_proof_file() works per instance.
        The empty clause is written at most once, nothing for a tautological core; share_import() takes no record while
        a proof is logged.  The file is closed when the call ends (sweep_end for a sweep).  include/mi355sat.h."""
        self._check(self._L.mi355sat_set_proof_path(self._h, path.encode() if path else None), "set_proof_path")

    def set_incremental(self, on=True):
        """Warm incremental solve: with it on, a solve() after clauses and / or assumptions were added goes on with the
        workers of the solve before - their learnt clauses, saved phases and decision order - instead of preparing the
        formula from scratch; where that is not possible it silently starts cold (include/mi355sat.h lists when).
        reserve() the variables of later clauses before the first solve."""
        self._check(self._L.mi355sat_set_incremental(self._h, 1 if on else 0), "set_incremental")

    def debug_incremental(self):
        """Test hook: warm / cold solves so far, clauses and units attached warm, learnt clauses resident when the last
        warm solve began, reason (ColdReason) of the last cold start."""
        info = Mi355SatIncrementalInfo()
        self._check(self._L.mi355sat_debug_incremental(self._h, ctypes.byref(info)), "debug_incremental")
        return info.as_dict()

    def debug_heuristics(self):
        """Test hook: what the optional heuristics did, summed over the workers of the last solve: clauses vivified and
        literals removed from them, rephasings, exchanged records skipped by import_pct, imports that share_interval forced
        above level 0."""
        info = Mi355SatHeuristicsInfo()
        self._check(self._L.mi355sat_debug_heuristics(self._h, ctypes.byref(info)), "debug_heuristics")
        return info.as_dict()

    def debug_set_schedule(self, first_vivify=0, vivify_every=0, rephase_every=0):
        """Test hook: conflicts of one worker before its first vivification pass, between passes, and before its first
        rephasing (0 = the defaults 1500 / 400 / 2000), from the next solve on."""
        self._check(self._L.mi355sat_debug_set_schedule(self._h, first_vivify, vivify_every, rephase_every), "debug_set_schedule")

    def debug_set_capacities(self, learnt_cap=0, learnt_lit_cap=0, pool_slack=0, proof_cap=0):
        """Test hook: the sizes of a worker's stores from the next cold start of a search on (0 = the sizing rule): learnt-clause
        slots, learnt literal words, watch-pool entries beyond the initial lists, proof-log words."""
        self._check(self._L.mi355sat_debug_set_capacities(self._h, learnt_cap, learnt_lit_cap, pool_slack, proof_cap), "debug_set_capacities")

    def debug_capacities(self):
        """Test hook: the store sizes of the last cold start, and - summed over the workers of the last search - the
        reductions that store pressure made due, the watch-pool collections of a pool three quarters full, the exchanged
        records passed over for want of room."""
        info = Mi355SatCapacityInfo()
        self._check(self._L.mi355sat_debug_capacities(self._h, ctypes.byref(info)), "debug_capacities")
        return info.as_dict()

    def lit_val(self, lit):
        return self._L.mi355sat_val(self._h, int(lit))

    def full_solution(self, n_vars=None):
        """Assignment for vars 1..n_vars as int8: 1 true, -1 false, 0 unknown."""
        n_vars = self._n_vars if n_vars is None else n_vars
        out = np.zeros(n_vars, dtype=np.int8)
        self._check(self._L.mi355sat_model(self._h, _p(out), n_vars), "full_solution")
        return out

    def solution_of(self, instance, n_vars=None):
        n_vars = self._n_vars if n_vars is None else n_vars
        out = np.zeros(n_vars, dtype=np.int8)
        self._check(self._L.mi355sat_model_of(self._h, instance, _p(out), n_vars), "solution_of")
        return out

    # ---- SolveStats
    def stats(self):
        st = Mi355SatStats()
        self._check(self._L.mi355sat_stats(self._h, ctypes.byref(st)), "stats")
        return st.as_dict()

    def max_var(self):
        return self._n_vars
