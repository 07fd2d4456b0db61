//! `rustsat::solvers::Solve` over libmi355sat.so - the same kind of wrapper rustsat-glucose is over its
//! vendored C++ solver (an IPASIR-shaped C API), so the reference swaps backends in two lines:
//!
//! ```text
//! - use rustsat_glucose::simp::Glucose as GlucoseSimp;     // crates/repl/src/main.rs:17, crates/gui/src/main.rs:2
//! + use mi355sat::Mi355Sat as GlucoseSimp;
//! ```
//!
//! Trait surface = what the reference exercises: `Default`, `add_cnf` / `add_clause_ref`,
//! `interrupter`, `solve`, `full_solution` (through `lit_val` + `max_var`), `stats`; plus `SolveIncremental`
//! (`solve_assumps`, `core`: IPASIR assume / failed) for rustsat's incremental encodings and core-guided code.
use std::os::raw::{c_char, c_int, c_void};

use rustsat::instances::Cnf;
use rustsat::solvers::{Interrupt, InterruptSolver, Solve, SolveIncremental, SolveStats, SolverResult, SolverStats};
use rustsat::types::{Assignment, Cl, Clause, Lit, TernaryVal, Var};

/// Mirror of `mi355sat_opts` (include/mi355sat.h); zero = defaults.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct Opts {
    pub device: i32, pub workers: i32, pub conflict_budget: i64, pub slice_conflicts: i32, pub seed: u64,
    pub verbose: i32, pub reduce_first: i32, pub reduce_inc: i32, pub lds_val: i32, pub max_groups: i32,
    pub slice_ms: i32, pub cube_split: i32, pub share: i32, pub share_lbd: i32, pub share_len: i32,
    pub share_interval: i32, pub var_order: i32, pub ramp: i32, pub one_per_simd: i32, pub simp: i32, pub phase_mix: i32, pub rephase: i32, pub restart_k_pct: i32, pub restart_k2_pct: i32, pub import_pct: i32, pub vivify: i32, pub rebalance: i32, pub deterministic: i32,
}

/// Mirror of `mi355sat_stats_t`.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct Stats {
    pub propagations: u64, pub decisions: u64, pub conflicts: u64, pub restarts: u64, pub learnts: u64,
    pub learnt_literals: u64, pub reduce_dbs: u64, pub n_clauses: u64, pub max_var: u64, pub avg_clause_len: f64,
    pub solve_seconds: f64, pub kernel_seconds: f64, pub kernel_launches: u64, pub n_deq: u64, pub n_watch: u64,
    pub n_cl_lit: u64, pub n_move: u64, pub n_enq: u64, pub n_sat: u64, pub n_unsat: u64, pub n_terminated: u64,
    pub bcp_steps: u64, pub bcp_requeued: u64, pub shared_exported: u64, pub shared_imported: u64,
    pub shared_imported_units: u64, pub simp_units: u64, pub simp_equivalences: u64, pub simp_clauses_removed: u64, pub workers: u64, pub simp_eliminated: u64,
}

/// Mirror of `mi355sat_core_min_info`: what `minimize_core` did.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct CoreMinInfo {
    pub size_before: u64, pub size_after: u64,
    /// 1: every literal of the core is proved necessary; 0: stopped early (budget / interrupt), the core is still a core
    pub minimal: i32,
    pub rounds: u32, pub candidates: u64, pub candidates_unsat: u64, pub candidates_sat: u64,
    pub critical_by_model: u64, pub model_launches: u64, pub conflicts: u64, pub seconds: f64,
}

/// Mirror of `mi355sat_proof_info`: what `check_proof` found.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct ProofInfo {
    /// 1: every lemma is RUP in order and the target is RUP at the end; 0: not; -1: the check was interrupted
    pub valid: i32,
    pub pad: i32,
    pub n_lemmas: u64, pub n_deletions_ignored: u64,
    /// smallest lemma index that is not RUP (the target is lemma number `n_lemmas`); `u64::MAX` if none
    pub first_failed: u64,
    /// smallest lemma index at which formula + lemmas before it are refuted by unit propagation alone; `u64::MAX` if never
    pub refuted_at: u64,
    pub segments: u64, pub workers: u64, pub lemmas_checked: u64, pub lemmas_attached: u64, pub propagations: u64,
    pub launches: u64, pub seconds: f64, pub kernel_seconds: f64,
}

/// Mirror of `mi355sat_trim_info`: what `trim_proof` found.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct TrimInfo {
    /// exactly what `check_proof` reports for the same inputs
    pub check: ProofInfo,
    /// sizes of the clause core and of the set of needed lemmas (0 unless `check.valid == 1`)
    pub core_clauses: u64, pub lemmas_needed: u64,
    pub dep_records: u64, pub log_drains: u64, pub log_words_per_worker: u64,
}
/// `MI355SAT_TRIM_HINTS`: keep what `write_lrat` needs.
pub const TRIM_HINTS: u32 = 1;

/// Mirror of `mi355sat_lrat_info`: what `check_lrat_file` found.
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct LratInfo {
    /// `accepted && derives_target`
    pub valid: i32,
    /// 1: every line accepted; 0: one rejected; -1: the check was interrupted
    pub accepted: i32,
    pub derives_target: i32,
    /// `MI355SAT_LRAT_*` of the first rejected line (1 id order .. 8 last hint not falsified), 0 if none
    pub reason: i32,
    pub n_lines: u64, pub n_hints: u64,
    /// 0-based index of the first rejected line and its id as written; `u64::MAX` if none
    pub first_rejected: u64, pub first_rejected_id: u64,
    /// position of the offending hint in that line (reasons 4..8), else `u64::MAX`
    pub reject_hint: u64,
    pub used_originals: u64, pub longest_clause: u64,
    pub lds: i32, pub dyn_lds_bytes: u32,
    pub waves: u64, pub launches: u64, pub seconds: f64, pub kernel_seconds: f64,
}

extern "C" {
    fn mi355sat_new(opts: *const Opts) -> *mut c_void;
    fn mi355sat_free(s: *mut c_void);
    fn mi355sat_abi_sizes(stats_size: *mut u64) -> u64;
    fn mi355sat_last_error(s: *const c_void) -> *const c_char;
    fn mi355sat_add_cnf(s: *mut c_void, lits: *const i32, offsets: *const u64, n: u64) -> c_int;
    fn mi355sat_add(s: *mut c_void, lit_or_0: i32) -> c_int;
    fn mi355sat_reserve(s: *mut c_void, n_vars: u64) -> c_int;
    fn mi355sat_solve(s: *mut c_void) -> c_int;
    fn mi355sat_val(s: *mut c_void, lit: i32) -> i32;
    fn mi355sat_assume(s: *mut c_void, lit: i32) -> c_int;
    fn mi355sat_core(s: *mut c_void, out: *mut i32, cap: u64, n: *mut u64) -> c_int;
    fn mi355sat_minimize_core(s: *mut c_void, conflict_budget: i64, out: *mut CoreMinInfo) -> c_int;
    fn mi355sat_check_proof(s: *mut c_void, proof: *const i32, n_words: u64, target: *const i32, n_target: u64, segments: u32,
                            out: *mut ProofInfo) -> c_int;
    fn mi355sat_trim_proof(s: *mut c_void, proof: *const i32, n_words: u64, target: *const i32, n_target: u64, segments: u32,
                           flags: u32, out: *mut TrimInfo) -> c_int;
    fn mi355sat_proof_deletions(s: *mut c_void, on: c_int) -> c_int;
    fn mi355sat_trim_core(s: *mut c_void, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    fn mi355sat_trim_lemmas(s: *mut c_void, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    fn mi355sat_trim_write_lrat(s: *mut c_void, path: *const c_char) -> c_int;
    fn mi355sat_check_lrat_file(s: *mut c_void, path: *const c_char, target: *const i32, n_target: u64, out: *mut LratInfo) -> c_int;
    fn mi355sat_lrat_used(s: *mut c_void, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    fn mi355sat_interrupt(s: *mut c_void);
    fn mi355sat_stats(s: *const c_void, out: *mut Stats) -> c_int;
    fn mi355sat_set_incremental(s: *mut c_void, on: c_int) -> c_int;
    fn mi355sat_phase(s: *mut c_void, lit: i32) -> c_int;
    fn mi355sat_unphase(s: *mut c_void, var: i32) -> c_int;
    fn mi355sat_set_phases(s: *mut c_void, phases: *const i8, n_vars: u64) -> c_int;
}

pub struct Mi355Sat { h: *mut c_void }
// The handle may move between OS threads between calls (solver_runner.rs:15 moves the solver into tokio's
// blocking pool); every entry point of the library binds its device itself.
unsafe impl Send for Mi355Sat {}

impl Mi355Sat {
    pub fn with_opts(opts: &Opts) -> anyhow::Result<Self> {
        let mut st_size = 0u64;
        let opt_size = unsafe { mi355sat_abi_sizes(&mut st_size) };
        anyhow::ensure!(opt_size as usize == std::mem::size_of::<Opts>() && st_size as usize == std::mem::size_of::<Stats>(),
                        "libmi355sat was built from another include/mi355sat.h than this crate mirrors");
        let h = unsafe { mi355sat_new(opts) };
        if h.is_null() {
            let m = unsafe { std::ffi::CStr::from_ptr(mi355sat_last_error(std::ptr::null())) };
            anyhow::bail!("mi355sat_new failed: {}", m.to_string_lossy());
        }
        Ok(Self { h })
    }
    /// Warm incremental solve (`mi355sat_set_incremental`): with it on, a `solve` / `solve_assumps` after clauses or
    /// assumptions were added goes on with the workers of the solve before - learnt clauses, phases, decision order -
    /// instead of preparing the formula from scratch (silently cold where that is not possible: include/mi355sat.h).
    /// Users of `SolveIncremental` want it on; `reserve` the variables of later clauses before the first solve.
    /// Replayed in C by tests/abi_incremental.c.
    pub fn set_incremental(&mut self, on: bool) -> anyhow::Result<()> {
        if unsafe { mi355sat_set_incremental(self.h, on as c_int) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Phase hint (`mi355sat_phase`): the first time `lit`'s variable is decided, it is decided as `lit`.  The hint SEEDS
    /// the workers' saved phase at the next solve and phase saving takes over from there - it is not forced for every
    /// later decision as Glucose's `setPolarity` is, which is why these are inherent methods and not rustsat's `PhaseLit`
    /// (INTEGRATION.md).  Kept on the handle until cleared; failed / core stay valid; never makes a warm solve start cold.
    pub fn phase_hint(&mut self, lit: Lit) -> anyhow::Result<()> {
        if unsafe { mi355sat_phase(self.h, ipasir(lit)) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Drops the hint of `var` (`mi355sat_unphase`).  What the hint seeded stays the workers' saved phase.
    pub fn clear_phase_hint(&mut self, var: Var) -> anyhow::Result<()> {
        if unsafe { mi355sat_unphase(self.h, var.idx32() as i32 + 1) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Bulk hints (`mi355sat_set_phases`) for the variables 0..=max_var of `assign`: True / False first, DontCare clears
    /// the variable's hint.  The refinement loop's lever: hint the next bound's fresh solver to the model of the last
    /// one, restricted to the encoder's variables.
    pub fn set_phase_hints(&mut self, assign: &Assignment) -> anyhow::Result<()> {
        let n = assign.max_var().map_or(0, |v| v.idx() + 1);
        let phases: Vec<i8> = (0..n).map(|i| match assign.var_value(Var::new(i as u32)) {
            TernaryVal::True => 1, TernaryVal::False => -1, TernaryVal::DontCare => 0 }).collect();
        if unsafe { mi355sat_set_phases(self.h, phases.as_ptr(), n as u64) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Irreducible core (`mi355sat_minimize_core`): after `solve_assumps` returned `Unsat`, shrinks the core until no
    /// literal can be left out; `core()` answers with the new one, a subsequence of the old.  `budget`: conflicts summed
    /// over the workers (None: no limit); with `minimal == 0` the budget or an interrupt ended the call early and the
    /// core is still a valid core.  An error (`MI355SAT_ERR_STATE`) where `core()` would give one.  What core-guided code
    /// wants before it adds a totalizer per core literal.  Replayed in C by tests/abi_core_minimize.c.
    pub fn minimize_core(&mut self, budget: Option<u64>) -> anyhow::Result<CoreMinInfo> {
        let mut info = CoreMinInfo::default();
        let b = budget.map_or(0, |b| b.clamp(1, i64::MAX as u64) as i64);
        if unsafe { mi355sat_minimize_core(self.h, b, &mut info) } < 0 { return Err(self.err()); }
        Ok(info)
    }
    /// Certificate check (`mi355sat_check_proof`): forward RUP, deletion lines ignored, of a DRUP proof - flat words, lemmas
    /// 0-terminated, a deletion line = `i32::MIN`, the clause, 0 - against this handle's clauses as they were added.
    /// `target`: the clause the proof must derive (empty: the empty clause; after `solve_assumps`, the negated core).
    /// `segments`: parts the lemma list is cut into, one wavefront each (0: the default); the verdict does not depend on
    /// it.  `valid == -1`: an interrupt ended the check.  The next warm solve starts cold.
    pub fn check_proof(&mut self, proof: &[i32], target: &[i32], segments: u32) -> anyhow::Result<ProofInfo> {
        let mut info = ProofInfo::default();
        let rc = unsafe {
            mi355sat_check_proof(self.h, proof.as_ptr(), proof.len() as u64, target.as_ptr(), target.len() as u64, segments, &mut info)
        };
        if rc < 0 { return Err(self.err()); }
        Ok(info)
    }
    /// Honour the proof's deletion lines in `check_proof` / `trim_proof` (`mi355sat_proof_deletions`; off by default:
    /// counted and ignored).  A worker then holds only the live lemmas and its stores are sized from their peak, so long
    /// proofs fit; a proof that uses a lemma after deleting it is not valid.  Semantics: include/mi355sat.h.
    pub fn set_proof_deletions(&mut self, on: bool) -> anyhow::Result<()> {
        if unsafe { mi355sat_proof_deletions(self.h, on as c_int) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Trimmed certificate (`mi355sat_trim_proof`): `check_proof` in the tracing build of the checker.  Where
    /// `check.valid == 1`, `trim_core` / `trim_lemmas` name the clauses of this handle (0-based, in the order they were
    /// added) and the lemmas the derivation of `target` rests on; with `hints`, `write_lrat` writes an LRAT file a checker
    /// without search verifies.  Which clauses make the core may differ with `segments` and from run to run.
    pub fn trim_proof(&mut self, proof: &[i32], target: &[i32], segments: u32, hints: bool) -> anyhow::Result<TrimInfo> {
        let mut info = TrimInfo::default();
        let rc = unsafe {
            mi355sat_trim_proof(self.h, proof.as_ptr(), proof.len() as u64, target.as_ptr(), target.len() as u64, segments,
                                if hints { TRIM_HINTS } else { 0 }, &mut info)
        };
        if rc < 0 { return Err(self.err()); }
        Ok(info)
    }
    fn indices(&mut self, get: unsafe extern "C" fn(*mut c_void, *mut u64, u64, *mut u64) -> c_int) -> anyhow::Result<Vec<u64>> {
        let mut n = 0u64;
        if unsafe { get(self.h, std::ptr::null_mut(), 0, &mut n) } < 0 { return Err(self.err()); }
        let mut out = vec![0u64; n as usize];
        if unsafe { get(self.h, out.as_mut_ptr(), n, &mut n) } < 0 { return Err(self.err()); }
        Ok(out)
    }
    /// The clause core of the last valid `trim_proof`, ascending; an error (`MI355SAT_ERR_STATE`) in any other state.
    pub fn trim_core(&mut self) -> anyhow::Result<Vec<u64>> { self.indices(mi355sat_trim_core) }
    /// The lemmas it needs, ascending.
    pub fn trim_lemmas(&mut self) -> anyhow::Result<Vec<u64>> { self.indices(mi355sat_trim_lemmas) }
    /// The needed lemmas and the target as LRAT (clause i has id i + 1, lemma j has n_clauses + 1 + j).
    pub fn write_lrat(&mut self, path: &std::path::Path) -> anyhow::Result<()> {
        let p = std::ffi::CString::new(path.to_string_lossy().as_bytes())?;
        if unsafe { mi355sat_trim_write_lrat(self.h, p.as_ptr()) } < 0 { return Err(self.err()); }
        Ok(())
    }
    /// Strict LRAT check on the device (`mi355sat_check_lrat_file`) of a file as `write_lrat` writes it, against this
    /// handle's clauses (clause i, 0-based in add order, has id i + 1): `valid == 1` iff every line is accepted and the
    /// last one is `target` (empty: the empty clause).  The kernel shares nothing with the solver's propagation; the call
    /// leaves the handle's solve state, cores and trim result alone.  Input that is not LRAT at all is an error.
    pub fn check_lrat_file(&mut self, path: &std::path::Path, target: &[i32]) -> anyhow::Result<LratInfo> {
        let p = std::ffi::CString::new(path.to_string_lossy().as_bytes())?;
        let mut info = LratInfo::default();
        let rc = unsafe { mi355sat_check_lrat_file(self.h, p.as_ptr(), target.as_ptr(), target.len() as u64, &mut info) };
        if rc < 0 { return Err(self.err()); }
        Ok(info)
    }
    /// After a `check_lrat_file` that accepted every line: the clauses of this handle some line hinted, ascending; an
    /// error (`MI355SAT_ERR_STATE`) in any other state.
    pub fn lrat_used(&mut self) -> anyhow::Result<Vec<u64>> { self.indices(mi355sat_lrat_used) }
    fn err(&self) -> anyhow::Error {
        let m = unsafe { std::ffi::CStr::from_ptr(mi355sat_last_error(self.h)) };
        anyhow::anyhow!(m.to_string_lossy().into_owned())
    }
    fn raw_stats(&self) -> Stats {
        let mut st = Stats::default();
        unsafe { mi355sat_stats(self.h, &mut st) };
        st
    }
}

impl Default for Mi355Sat {                    // S::default(): main.rs:295, solver_backend.rs:79
    fn default() -> Self { Self::with_opts(&Opts { device: -1, ..Opts::default() }).expect("no usable HIP device") }
}
impl Drop for Mi355Sat { fn drop(&mut self) { unsafe { mi355sat_free(self.h) } } }

fn ipasir(l: Lit) -> i32 { let v = l.vidx32() as i32 + 1; if l.is_neg() { -v } else { v } }
fn from_ipasir(l: i32) -> Lit { let v = Var::new(l.unsigned_abs() - 1); if l < 0 { v.neg_lit() } else { v.pos_lit() } }

impl Solve for Mi355Sat {
    fn signature(&self) -> &'static str { "mi355sat (HIP/gfx950 wave-parallel CDCL)" }
    fn add_clause_ref<C: AsRef<Cl> + ?Sized>(&mut self, c: &C) -> anyhow::Result<()> {
        for l in c.as_ref().iter() {
            if unsafe { mi355sat_add(self.h, ipasir(*l)) } < 0 { return Err(self.err()); }
        }
        if unsafe { mi355sat_add(self.h, 0) } < 0 { return Err(self.err()); }
        Ok(())
    }
    // Bulk override of the per-literal default (solver_runner.rs:12): one CSR hand-over, one FFI call.
    fn add_cnf(&mut self, cnf: Cnf) -> anyhow::Result<()> {
        let mut lits: Vec<i32> = Vec::new();
        let mut offsets: Vec<u64> = vec![0];
        for cl in cnf.iter() {
            lits.extend(cl.iter().map(|l| ipasir(*l)));
            offsets.push(lits.len() as u64);
        }
        if unsafe { mi355sat_add_cnf(self.h, lits.as_ptr(), offsets.as_ptr(), (offsets.len() - 1) as u64) } < 0 {
            return Err(self.err());
        }
        Ok(())
    }
    fn reserve(&mut self, max_var: Var) -> anyhow::Result<()> {
        if unsafe { mi355sat_reserve(self.h, max_var.idx() as u64 + 1) } < 0 { return Err(self.err()); }
        Ok(())
    }
    fn solve(&mut self) -> anyhow::Result<SolverResult> {            // solver_runner.rs:16
        match unsafe { mi355sat_solve(self.h) } {
            10 => Ok(SolverResult::Sat),
            20 => Ok(SolverResult::Unsat),
            0 => Ok(SolverResult::Interrupted),
            _ => Err(self.err()),                                     // negative codes -> anyhow error
        }
    }
    fn lit_val(&self, lit: Lit) -> anyhow::Result<TernaryVal> {      // full_solution(): main.rs:329, app.rs:154
        let l = ipasir(lit);
        Ok(match unsafe { mi355sat_val(self.h, l) } { v if v == l => TernaryVal::True, 0 => TernaryVal::DontCare, _ => TernaryVal::False })
    }
}

/// IPASIR assume / failed, as rustsat-glucose wraps them: the assumptions hold for one `solve_assumps` call; `core`
/// after an Unsat answer returns the NEGATED failed assumptions - a clause the formula implies (rustsat's convention).
/// Replayed in C by tests/abi_cores.c.
impl SolveIncremental for Mi355Sat {
    fn solve_assumps(&mut self, assumps: &[Lit]) -> anyhow::Result<SolverResult> {
        for l in assumps {
            if unsafe { mi355sat_assume(self.h, ipasir(*l)) } < 0 { return Err(self.err()); }
        }
        self.solve()
    }
    fn core(&mut self) -> anyhow::Result<Vec<Lit>> {
        let mut n = 0u64;
        if unsafe { mi355sat_core(self.h, std::ptr::null_mut(), 0, &mut n) } < 0 { return Err(self.err()); }
        let mut out = vec![0i32; n as usize];
        if unsafe { mi355sat_core(self.h, out.as_mut_ptr(), n, &mut n) } < 0 { return Err(self.err()); }
        Ok(out.into_iter().map(|l| !from_ipasir(l)).collect())
    }
}

impl Extend<Clause> for Mi355Sat {
    fn extend<T: IntoIterator<Item = Clause>>(&mut self, it: T) { for c in it { self.add_clause_ref(&c).expect("add_clause") } }
}
impl<'a> Extend<&'a Clause> for Mi355Sat {
    fn extend<T: IntoIterator<Item = &'a Clause>>(&mut self, it: T) { for c in it { self.add_clause_ref(c).expect("add_clause") } }
}

/// `S::Interrupter`: `Send + 'static`, called through `&self` from another task while `solve()` runs
/// (main.rs:298-323).  It only sets a flag; the solver must outlive it, as with rustsat-glucose - true at both
/// call sites (the solver comes back from the blocking task, solver_runner.rs:15-17).
pub struct Interrupter(*mut c_void);
unsafe impl Send for Interrupter {}
unsafe impl Sync for Interrupter {}
impl InterruptSolver for Interrupter { fn interrupt(&self) { unsafe { mi355sat_interrupt(self.0) } } }     // main.rs:316
impl Interrupt for Mi355Sat {
    type Interrupter = Interrupter;
    fn interrupter(&mut self) -> Interrupter { Interrupter(self.h) }                                       // solver_runner.rs:13
}

impl SolveStats for Mi355Sat {                                                                            // main.rs:363, app.rs:148-151
    fn stats(&self) -> SolverStats {
        let st = self.raw_stats();
        SolverStats {
            n_sat: st.n_sat as usize, n_unsat: st.n_unsat as usize, n_terminated: st.n_terminated as usize,
            n_clauses: st.n_clauses as usize, max_var: (st.max_var > 0).then(|| Var::new(st.max_var as u32 - 1)),
            avg_clause_len: st.avg_clause_len as f32, cpu_solve_time: std::time::Duration::from_secs_f64(st.solve_seconds),
        }
    }
    fn max_var(&self) -> Option<Var> { let m = self.raw_stats().max_var; (m > 0).then(|| Var::new(m as u32 - 1)) }
}
