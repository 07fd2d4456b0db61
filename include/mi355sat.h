/*
 * mi355sat.h — C ABI of the MI355X-native SAT solve loop (libmi355sat.so).
 *
 * This is the drop-in boundary behind timberborn_support_solver's solver
 * backend.  The reference is generic over `S: Solve + Interrupt (+ Default +
 * SolveStats) + Send + 'static` and instantiates it with
 * `rustsat_glucose::simp::Glucose`:
 *
 *   crates/repl/src/solver_runner.rs:8-20   run_solver<S>: add_cnf, interrupter, solve
 *   crates/repl/src/main.rs:17,295          GlucoseSimp::default()
 *   crates/repl/src/main.rs:329,363         full_solution(), stats()
 *   crates/gui/src/solver_backend.rs:69-97  S::default(), add_cnf, interrupter, solve
 *   crates/gui/src/main.rs:2,26             App::<GlucoseSimp>
 *
 * rustsat-glucose talks to its C++ solver through an IPASIR-shaped C API
 * (init / add / assume / solve / val / failed / interrupt / release; solve
 * returns 10/20/0).  The functions below have the same shape so that a Rust
 * `Solve` + `SolveIncremental` impl over this library is a thin clone of that
 * wrapper.
 *
 * Conventions
 *   - literals are IPASIR/DIMACS: +v / -v, v >= 1; 0 terminates a clause in
 *     mi355sat_add().  (rustsat `Lit` = (idx<<1)|neg with 0-based idx maps to
 *     ±(idx+1).)
 *   - no exceptions cross the ABI; errors are negative return codes and
 *     mi355sat_last_error() gives the text.
 *   - a handle may be moved between OS threads between calls
 *     (solver_runner.rs:15 moves the solver into tokio's blocking pool); every
 *     entry point binds its device itself.  The ONLY function that may run
 *     concurrently with another call on the same handle is
 *     mi355sat_interrupt() (main.rs:310-317 calls it from another task while
 *     solve() runs).
 *   - clause memory is copied on add; the caller may free it immediately
 *     (add_cnf consumes its argument, solver_runner.rs:12).
 *   - there is NO CPU fallback: if no HIP device is usable, mi355sat_new()
 *     returns NULL and mi355sat_last_error(NULL) says why.
 */
#ifndef MI355SAT_H
#define MI355SAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355SAT_SAT 10
#define MI355SAT_UNSAT 20
#define MI355SAT_INTERRUPTED 0
#define MI355SAT_ERR_OOM (-1)
#define MI355SAT_ERR_HIP (-2)
#define MI355SAT_ERR_STATE (-3)
#define MI355SAT_ERR_ARG (-4)

typedef struct mi355sat mi355sat;

/* Options for mi355sat_new(); zero-initialise and set what you need.
 * A NULL pointer means all defaults. */
typedef struct mi355sat_opts {
    int32_t device;            /* HIP device ordinal; -1 = current device (default 0) */
    int32_t workers;           /* concurrent search workers (one wavefront each); 0 = default: 4096 (16 per CU) above
                                  100k clauses, 1024 above 20k, else 256 */
    int64_t conflict_budget;   /* per-solve conflict limit summed over workers; 0 = none.
                                  Exhausted budget -> MI355SAT_INTERRUPTED */
    int32_t slice_conflicts;   /* conflicts per worker per kernel launch; 0 = default */
    uint64_t seed;             /* diversification seed (phases / decision order of workers > 0) */
    int32_t verbose;           /* 0 quiet, 1 progress on stderr */
    int32_t reduce_first;      /* conflicts before the first learnt-clause reduction; 0 = 2000 */
    int32_t reduce_inc;        /* growth of the reduction interval; 0 = 300 */
    int32_t lds_val;           /* assignment in LDS (2 bits/var): 0 auto, 1 force, -1 never */
    int32_t max_groups;        /* queue literals propagated per BCP step: 1..32; 0 = 32 */
    int32_t slice_ms;          /* wall-time bound of one kernel launch in ms (all workers stop together); 0 = default: 20 in a
                                  solve's first second of kernel time, then 50, after ten seconds 100 */
    int32_t cube_split;        /* 0 (default): portfolio, every worker of an instance searches the whole instance with its
                                  own decision order; 1: idle workers steal sub-cubes of running ones between slices
                                  (correct but, as measured in round 1, slower: DESIGN.md) */
    int32_t share;             /* learnt-clause exchange between the workers of one GPU (units, binaries and clauses of
                                  at most share_len literals with LBD <= share_lbd, passed on between kernel launches):
                                  0 = default (on), -1 = off.  Off automatically with one worker.  (A proof log keeps it on: every worker
                                  logs what it learns, mi355sat_set_proof_path.) */
    int32_t share_lbd;         /* 0 = 4 (measured: rect 24 k=8 1.0 vs 1.3 s, rect 16 1x1 k=14 14-18 vs 24 s with 2; 6-12 no better) */
    int32_t share_len;         /* longest exchanged clause, <= 31; 0 = 31 */
    int32_t share_interval;    /* > 0: a worker with unseen exchanged clauses restarts to attach them after this many of its
                                  own conflicts; 0 = default: only at its own (Glucose) restarts - forced restarts measured
                                  3-10x slower on the rect 24x24 ladder */
    int32_t var_order;         /* 0 = default: the device keeps the caller's variable numbering; 1 = it renumbers variables so
                                  that those meeting in clauses are neighbours (256-variable blobs grown breadth-first
                                  through the clauses).  Invisible at this interface: literals, models and proofs are
                                  always in the caller's numbering.  Measured on rect 64x64: no gain. */
    int32_t ramp;              /* 0 = default (on): the first 100 ms of kernel time of a solve run 256 workers (one per
                                  CU, each ~3x faster than one of 16), the next 300 ms 1024, then all - easy instances
                                  are decided by one worker's few hundred conflicts; -1 = the whole fleet at once */
    int32_t one_per_simd;      /* 0 = default: a launch of at most 1024 workers (one per SIMD) runs the build of the search
                                  kernel that owns the SIMD's whole register file (no spills, everything inlined), one of at
                                  most 2048 the 2-waves-per-SIMD build, larger ones the 4-waves build;
                                  -1 = always the 4-waves-per-SIMD build, 2 / 4 = at least the 2- / 4-waves build (A/B) */
    int32_t simp;              /* formula simplification before search (the reference's backend is `simp::Glucose`): 0 = default
                                  (on): equivalent-literal substitution, failed-literal probing on the device, subsumption and
                                  self-subsuming resolution on the device; 2 = the same plus bounded variable elimination
                                  (`SimpSolver::eliminate`: grow 0, resolvents of at most 20 literals; the variables of the
                                  assumptions are kept, eliminated ones get their values back when a model is read);
                                  -1 = only level-0 unit propagation.  Invisible at this interface: models, assumptions and
                                  proofs stay in the caller's variables. */
    int32_t phase_mix;         /* 0 = default: every worker starts with all saved phases FALSE (no platform anywhere);
                                  1 = portfolio of initial phases: a quarter of the workers start TRUE, a quarter at random */
    int32_t rephase;           /* rephasing to the best assignment (the polarities of the longest conflict-free assignment a worker
                                  has seen become its saved phases every 2000, 4000, 6000, ... conflicts, at a restart):
                                  0 = default: off (measured on rect 28x28 k = 12, a hard satisfiable bound: 4.3-6.3 s without,
                                  5.4-7.5 s with), 1 = every worker, 2 = every second worker */
    int32_t restart_k_pct;     /* Glucose's restart factor K in percent (restart when the LBD average of the last 50 conflicts times
                                  K exceeds the global average); 0 = 100 (round 3, with the sorted bump order: rect 28 k = 11 / rect 32
                                  k = 14 with 1024 workers 11.2 / 15.7 s at 100, 11.2-12.9 / 16.4-17.6 s at 90, 14.3 / 21.7 s at 80,
                                  20.0 / 34.5 s at 70, 11.7 / 17.8 s at 110; profiles/r03_m_knob_sweep*.log) */
    int32_t restart_k2_pct;    /* > 0: every second worker uses this K instead (a portfolio of restart policies); 0 = same K */
    int32_t import_pct;        /* share (percent) of the exchanged clauses of 3 and more literals each worker attaches (every worker
                                  another share; units and binaries always); 0 = default 50: a worker that attaches everything
                                  1023 others export spends its time on their clauses (measured, 1024 workers: rect 16 1x1 k = 14
                                  9.8-10.2 s at 50 %, 9.0-9.8 s at 25 %, 10.0-13.2 s at 100 %; rect 26 k = 10 46-56 s at 50 %,
                                  60-72 s at 100 %; rect 28 k = 11 within the run-to-run spread) */
    int32_t vivify;            /* vivification of learnt clauses: at a restart, every 400 conflicts, up to this many recent learnt
                                  clauses of LBD <= 6 (at most 64 literals) are re-derived literal by literal under unit
                                  propagation and replaced by the shorter clause that implies them (a RUP lemma, exported like a
                                  freshly learnt clause); > 0 = that many per pass; 0 = default: off (round 2 measured a quarter less
                                  time with 4 per pass; on top of round 3's recursive minimisation it is the other way round: rect 28
                                  k = 11 / rect 32 k = 14 10.5 / 15.9 s without, 12.9 / 17.6 s with, profiles/r03_m_knob_sweep2.log).  No effect in
                                  launches of more than 2048 workers: the full-fleet build leaves the code out */
    int32_t rebalance;         /* batched solves: 0 = default (on): workers of decided / withdrawn instances move to the open
                                  ones; -1 = they park, and a worker parked for a withdrawn instance resumes that instance
                                  (no other) when mi355sat_sweep_reopen takes it up again */
    int32_t deterministic;     /* 0 = default: time-bounded slices (all workers stop together; what a worker does in a slice, and
                                  with it the whole trajectory, depends on timing); 1 = a reproducible mode for benchmarks and
                                  A/B comparisons: slices are bounded by conflicts per worker (slice_conflicts, default 200), no
                                  worker leaves a slice because another one finished, the exchanged clauses are collected in
                                  worker order by one thread, the whole fleet runs from the first slice (no ramp-up): two runs
                                  with the same options and seed make the same decisions and report the same counters.  Slower
                                  (a conflict-bounded slice waits for its slowest worker). */
} mi355sat_opts;

/* Counters.  n_deq .. n_enq are the five event counters of SURVEY.md §8(d)
 * from which algorithmic bytes are computed:
 *   bytes_alg = 12*n_deq + 9*n_watch + 5*n_cl_lit + 8*n_move + 13*n_enq      */
typedef struct mi355sat_stats_t {
    uint64_t propagations;     /* trail literals dequeued by BCP (== n_deq) */
    uint64_t decisions;
    uint64_t conflicts;
    uint64_t restarts;
    uint64_t learnts;          /* learnt clauses currently kept (sum over workers) */
    uint64_t learnt_literals;
    uint64_t reduce_dbs;
    uint64_t n_clauses;        /* clauses added by the caller (rustsat SolverStats.n_clauses) */
    uint64_t max_var;          /* highest variable index seen, 1-based (0 = none) */
    double   avg_clause_len;
    double   solve_seconds;    /* wall-clock inside solve()/solve_batch()/propagate_batch() */
    double   kernel_seconds;   /* device time of the search / BCP kernels (HIP events) */
    uint64_t kernel_launches;
    uint64_t n_deq, n_watch, n_cl_lit, n_move, n_enq;
    uint64_t n_sat, n_unsat, n_terminated; /* rustsat SolverStats: results returned so far */
    uint64_t bcp_steps;        /* BCP steps; each propagates up to 32 queue literals (one per lane group) */
    uint64_t bcp_requeued;     /* literals re-queued because two groups met in one clause */
    uint64_t shared_exported;  /* clauses workers offered to the exchange / clauses (and units) attached from it, */
    uint64_t shared_imported;  /* summed over workers */
    uint64_t shared_imported_units;
    uint64_t simp_units;           /* simplification before search: failed literals + necessary assignments found by probing */
    uint64_t simp_equivalences;    /* variables replaced by an equivalent literal */
    uint64_t simp_clauses_removed; /* clauses subsumed or strengthened */
    uint64_t workers;              /* search workers (wavefronts) of the last solve / batch / sweep: what was asked for, or
                                      what device memory had room for */
    uint64_t simp_eliminated;      /* variables resolved away before search (bounded variable elimination) */
} mi355sat_stats_t;

/* --- lifecycle (Default::default / Drop) --------------------------------- */
mi355sat* mi355sat_new(const mi355sat_opts* opts);
void mi355sat_free(mi355sat* s);
/* mi355sat_free parks the handle's worker slabs (the one large device allocation: up to 147 GiB, 2-5 s of
 * hipMalloc) for the next handle of the process on the same device - the refinement loop makes a fresh
 * solver per bound (crates/repl/src/main.rs:295).  This returns the parked buffer to the driver. */
void mi355sat_release_cached_memory(void);
const char* mi355sat_signature(void);                 /* Solve::signature */
/* sizeof(mi355sat_opts) (returned) and sizeof(mi355sat_stats_t) (*stats_size) of THIS build: a binding whose
 * mirror structs have other sizes was written against another header and must refuse to run. */
uint64_t mi355sat_abi_sizes(uint64_t* stats_size);
const char* mi355sat_last_error(const mi355sat* s);   /* s may be NULL (error of the last failed new) */

/* --- clause input (Solve::add_cnf / add_clause_ref) ---------------------- */
/* Bulk CSR: clause i = lits[offsets[i] .. offsets[i+1]), offsets has n_clauses+1 entries. */
int mi355sat_add_cnf(mi355sat* s, const int32_t* lits, const uint64_t* offsets, uint64_t n_clauses);
/* IPASIR-style incremental add: literals, then 0 to close the clause. */
int mi355sat_add(mi355sat* s, int32_t lit_or_0);
/* Make sure variables 1..n exist even if they occur in no clause (rustsat reserve). */
int mi355sat_reserve(mi355sat* s, uint64_t n_vars);

/* --- solve (Solve::solve) ------------------------------------------------- */
/* Returns MI355SAT_SAT / MI355SAT_UNSAT / MI355SAT_INTERRUPTED or a negative error. */
int mi355sat_solve(mi355sat* s);

/* --- assumptions and failed-assumption cores (SolveIncremental) ----------- */
/* IPASIR assume: lit holds for the next mi355sat_solve() only, which consumes the list whatever it returns.  A
 * variable above the highest one seen is reserved (as mi355sat_reserve).  Assumptions may repeat or contradict each
 * other. */
int mi355sat_assume(mi355sat* s, int32_t lit);
/* IPASIR failed: after mi355sat_solve() returned UNSAT, 1 if lit is in the core, else 0; MI355SAT_ERR_STATE in any
 * other state (no solve yet, SAT, interrupted, exhausted budget, a clause or an assumption added since). */
int mi355sat_failed(mi355sat* s, int32_t lit);
/* The core of the last UNSAT solve(): a subset of the assumptions as the caller gave them, in their order, such that
 * formula AND core is UNSAT (empty if the formula alone is).  As the final conflict left it: mi355sat_minimize_core()
 * shrinks it to an irreducible one.  out may be NULL to size the buffer;
 * *n receives the length; MI355SAT_ERR_ARG if cap is too small, MI355SAT_ERR_STATE as for mi355sat_failed(). */
int mi355sat_core(mi355sat* s, int32_t* out, uint64_t cap, uint64_t* n);
/* The same for instance i of the last mi355sat_solve_batch() that reported UNSAT (MI355SAT_ERR_STATE otherwise). */
int mi355sat_core_of(mi355sat* s, uint64_t instance, int32_t* out, uint64_t cap, uint64_t* n);

/* --- irreducible cores ------------------------------------------------------- */
/* Shrinks the core of the last UNSAT solve() (mi355sat_minimize_core_of: of instance i of the last solve_batch()) until no
 * literal can be left out: afterwards mi355sat_core / _failed / _core_of answer with the new core - a subset of the old
 * one, in the caller's order, without repeats, formula AND core still UNSAT - until the next solve or add, as before.
 * Valid exactly where mi355sat_core / _core_of is, MI355SAT_ERR_STATE otherwise (and during a mi355sat_sweep_*); as
 * mi355sat_core_of, _minimize_core_of answers an instance index beyond the last batch with MI355SAT_ERR_ARG, and a
 * negative conflict_budget is MI355SAT_ERR_ARG too.
 * Returns 0 or a negative error; after an error the core is the one from before the call.
 *   - Deletion by rounds, on the device: a round poses up to min(64, workers) candidates "the core without this chunk"
 *     side by side as the instances of ONE resident sweep - the formula is simplified and uploaded once per call, the
 *     workers move from candidate to candidate and keep their learnt clauses, phases and the exchange ring (all
 *     consequences of the formula alone).  An UNSAT candidate's own final-conflict core becomes the working core; a SAT
 *     candidate that left out one literal proves it necessary, one that left out more proves a literal necessary if it is
 *     the only one its model falsifies (critical_by_model).  Rounds of SAT answers that prove nothing halve the chunks.
 *   - minimal = 1: formula AND (core without c) is SAT for every c in the core.  minimal = 0: the call stopped early -
 *     conflict_budget (> 0: conflicts summed over workers; opts.conflict_budget does not apply) or mi355sat_interrupt(),
 *     which the call consumes; an interrupt that came before the call leaves the core unchanged.  The core is then a
 *     valid core no larger than before.
 *   - Nothing is launched or allocated for an empty core, for a core this call (or an earlier one) already proved
 *     irreducible (the flag is kept with the core: candidates = 0), and for a one-literal core when the handle has
 *     answered SAT since the last clause was added (the formula alone has a model: the loop's bound posed as an
 *     assumption after a satisfiable one).  Any other one-literal core costs one candidate, the empty set.
 *   - opts and stats keep their layout.  Candidates do not count in n_sat / n_unsat / n_terminated; solve_seconds,
 *     kernel_seconds, kernel_launches and the event counters accumulate; simp_* and workers keep describing the caller's
 *     last solve / batch, while learnts / learnt_literals and the test hooks that describe "the last search"
 *     (mi355sat_debug_last_search_build, _debug_heuristics, _debug_share_ring, an armed _debug_keep_simplified) then
 *     describe the call's own sweep, which is what is on the device.  No proof lines are written.  opts.cube_split does
 *     not apply.
 *     For the warm incremental mode the call is another search in between: the next solve() starts cold
 *     (MI355SAT_COLD_OTHER_SEARCH).
 * Measured on the MI355X (profiles/r07_core_minimize.log: "no platform at any anchor", 1x1 platforms, rect 16 / 24 / 32 with
 * 256 / 576 / 1024 assumptions, three runs each way, alternating): the final conflict's core has 10 literals and is
 * irreducible already, so the call is one round of ten candidates - 11 / 23 / 23-24 ms beside a solve() of 3-9 ms - and the
 * same deletion loop driven from outside with one cold mi355sat_solve_batch per round takes the same 11 / 23 / 23-24 ms:
 * with one round the resident sweep gains nothing.  Cores that shrink over several rounds have not been measured on the
 * device. */
typedef struct mi355sat_core_min_info {
    uint64_t size_before, size_after;
    int32_t  minimal;            /* 1: every literal of the core is proved necessary; 0: stopped early (budget / interrupt) */
    uint32_t rounds;
    uint64_t candidates;         /* assumption sets posed */
    uint64_t candidates_unsat, candidates_sat;
    uint64_t critical_by_model;  /* literals proved necessary by a SAT candidate that dropped MORE than that one literal */
    uint64_t model_launches;     /* launches of ms_core_model_kernel */
    uint64_t conflicts;
    double   seconds;
} mi355sat_core_min_info;
int mi355sat_minimize_core(mi355sat* s, int64_t conflict_budget, mi355sat_core_min_info* out /* may be NULL */);
int mi355sat_minimize_core_of(mi355sat* s, uint64_t instance, int64_t conflict_budget, mi355sat_core_min_info* out);
/* Test hook: at most max_candidates candidates per round (0 = the default, min(64, workers)): forces rounds of chunks of
 * several literals on cores that one round would hold. */
int mi355sat_debug_core_min_round(mi355sat* s, uint32_t max_candidates);

/* --- phase hints (rustsat PhaseLit's place; seeded, not forced) ------------- */
/* A hint tells the search which polarity to try FIRST for a variable: the first time var(lit) is decided, it is decided
 * as lit.  The refinement loop poses one bound after another to fresh solvers (crates/repl/src/main.rs:290-346) and holds
 * a model of the bound before: hinted to it, the next solve starts its search at the last layout instead of at "no
 * platform anywhere".  Hints stay on the handle until mi355sat_unphase() / a 0 in mi355sat_set_phases().
 *   - A hint SEEDS the worker's saved phase; it is not forced.  Phase saving overwrites it the first time the variable is
 *     assigned, exactly as it overwrites the FALSE default.  That is the difference from Glucose's setPolarity (rustsat
 *     `phase_lit`), which pins the polarity of every later decision - and why this is not offered as `PhaseLit`
 *     (INTEGRATION.md).  The search kernel is the same with and without hints.
 *   - Hints take precedence over opts.phase_mix for the hinted variables, in every worker and replica; unhinted variables
 *     behave exactly as without any hint.
 *   - A variable above the highest one seen is reserved (as mi355sat_assume does).  Literal 0: MI355SAT_ERR_ARG.
 *   - Setting or clearing a hint does not touch the IPASIR state (failed / core stay valid) and never makes an incremental
 *     solve start cold.
 *   - Cold start (mi355sat_solve, mi355sat_solve_batch, mi355sat_sweep_begin; not mi355sat_propagate_batch): every worker
 *     is seeded after it got its assumptions and decision order - also the workers the ramp-up creates later.
 *     Warm start (mi355sat_set_incremental): the resident workers are seeded only if a hint was set or changed since they
 *     last were; a warm solve with unchanged hints launches nothing and keeps the phases the workers saved.  A cleared
 *     hint takes nothing back: what it seeded is the worker's saved phase by then.
 *   - A hint follows its variable through the simplification as an assumption does: through the equivalent-literal
 *     substitution (which may flip its sign), then the device's variable order.  In increasing variable order: of two
 *     hints that meet on one representative with opposite signs the later one wins.  A variable that opts.simp = 2
 *     eliminated has no phase to seed (its value is computed from the others when a model is read), one fixed at level 0
 *     none either: both hints are dropped and counted.
 *   - The first model found is not necessarily the hinted one; but if the hints ARE a model of the formula that agrees
 *     with the assumptions, every decision and with it every propagation agrees with it: the solve ends SAT without a
 *     single conflict, with that model (tests/test_emu_phase.py, tests/test_gpu_phase.py).
 *   Measured on the MI355X (profiles/r06_phase_hint_ladders.log: the plain refinement loop -l1:M, a fresh solver per bound,
 *   every rung hinted to the model of the rung before on the encoder's variables, against the same binary without hints,
 *   three runs each way, alternating): rect 24 2.6-3.0 s without, 1.7-1.8 s with; rect 26 10.4-11.0 s without, 10.1-10.8 s
 *   with (within the spread: 8 of the 10 s are the last, UNSAT rung, which no hint helps); rect 28 15.5-18.3 s without,
 *   14.1-15.5 s with.  What is gained is gained on the SAT rungs (rect 24 1.9-2.3 -> 0.9-1.2 s, rect 26 2.2-2.5 -> 1.6-2.3 s,
 *   rect 28 6.7-9.3 -> 5.4-6.2 s); the easy ones take half the conflicts, the ones just above the optimum spread widely
 *   either way.  Opt-in in the loops (solver_loop(phase_hints), tbs_cli --phase-hints). */
int mi355sat_phase(mi355sat* s, int32_t lit);
int mi355sat_unphase(mi355sat* s, int32_t var);
/* Bulk: phases[v-1] = 1 (TRUE first) / -1 (FALSE first) / 0 (no hint; clears one) for v = 1..n_vars.  Variables above
 * n_vars keep their hints. */
int mi355sat_set_phases(mi355sat* s, const int8_t* phases, uint64_t n_vars);
/* Test hook: what the hints did on this handle so far. */
typedef struct mi355sat_phase_info {
    uint64_t hinted;               /* variables with a hint now */
    uint64_t applied_cold;         /* cold starts that seeded their workers (one per solve / batch / sweep with a hint set) */
    uint64_t applied_warm;         /* warm starts that did (the hints had changed) */
    uint64_t launches;             /* ms_phase_kernel launches so far (the ramp-up's later workers have their own) */
    uint64_t mapped;               /* at the last application: device variables seeded in every worker, */
    uint64_t dropped_eliminated;   /*   hints on variables that were eliminated, */
    uint64_t dropped_fixed;        /*   hints on variables the formula fixes at level 0 */
} mi355sat_phase_info;
int mi355sat_debug_phases(const mi355sat* s, mi355sat_phase_info* out);

/* Batched solve under assumptions: instance i = formula AND assumption literals
 * assumps[assump_offsets[i] .. assump_offsets[i+1]).  This is what the sharded
 * decreasing-k sweep uses: the clause database (base CNF + one totalizer built
 * for k_max) is uploaded once and instance i assumes the negated totalizer
 * output for its own bound (solver_loop, crates/repl/src/main.rs:290-346, solves
 * one fresh CNF per k; the k's are independent).  results[i] receives
 * 10/20/0.  If stop_at_first != 0 the call returns as soon as one instance has a
 * verdict (others report 0).  Returns 0 or a negative error. */
int mi355sat_solve_batch(mi355sat* s, const int32_t* assumps, const uint64_t* assump_offsets,
                         uint64_t n_instances, int32_t* results, int stop_at_first);

/* The same batch, one kernel slice at a time (what bench.py times): begin uploads
 * the formula and creates the workers, each step runs every worker for
 * `slice_conflicts` conflicts (or to its verdict) and refreshes results / stats,
 * end fetches the models of SAT instances (mi355sat_model_of) and drops the batch. */
int mi355sat_sweep_begin(mi355sat* s, const int32_t* assumps, const uint64_t* assump_offsets, uint64_t n_instances);
int mi355sat_sweep_step(mi355sat* s, int32_t* results /* may be NULL */, uint64_t* n_decided /* may be NULL */);
/* Withdraw instances whose answer the caller no longer needs (in the decreasing-k sweep: every k above a
 * SAT one and every k below an UNSAT one is implied).  Their result stays 0 for as long as they are withdrawn, they
 * count as decided, and their workers move to the instances still open - as do the workers of every instance that gets
 * its verdict (opts.rebalance = -1: they park).  Withdrawing a decided or withdrawn instance, or none, changes nothing.
 * opts.cube_split = 1: the cubes of a withdrawn instance stay with their workers, which go on searching and splitting
 * them; the closed-cube accounting is kept - a cube that closes (or finds a model) while its instance is withdrawn stays
 * with its worker, and is counted, the verdict with it, at the first mi355sat_sweep_step after mi355sat_sweep_reopen. */
int mi355sat_sweep_drop(mi355sat* s, const uint64_t* instances, uint64_t n);
/* Priorities: open instance i gets about weights[i] / sum(weights of open instances) of the workers from the next
 * step on (workers move between open instances if need be; they keep their learnt clauses).  The decreasing-k loop
 * concentrates the fleet on the two bounds that decide it: the highest open one (a model there lowers the ceiling)
 * and the lowest open one (a refutation there raises the floor).  n must be the number of instances. */
int mi355sat_sweep_set_weights(mi355sat* s, const double* weights, uint64_t n);
/* Take withdrawn, still undecided instances up again: idle workers (parked, or of decided / withdrawn instances)
 * move to them.  With opts.rebalance = -1 nothing moves, but a worker that parked when its OWN instance was withdrawn
 * goes back to that instance's list, from level 0.  A reopened instance is decided again in every mode; its verdict is
 * reported by the steps that follow (at once, as UNSAT, if a worker has refuted the formula itself meanwhile).
 * Reopening an instance that is not withdrawn, or none, changes nothing.  The sharded sweep (one process per GPU,
 * SURVEY 8e) begins every rank with all bounds, withdraws the other ranks' shards, and reopens the bounds still open
 * anywhere once its own shard is decided. */
int mi355sat_sweep_reopen(mi355sat* s, const uint64_t* instances, uint64_t n);
/* Model of an instance that already reported SAT, while the sweep is still running (the loop needs the
 * layout's platform count to know which bounds it answers). */
int mi355sat_sweep_model_of(mi355sat* s, uint64_t instance, int8_t* out, uint64_t n_vars);
int mi355sat_sweep_end(mi355sat* s);

/* Batched unit propagation (BCP only, no search): instance i enqueues its
 * decision literals one decision level at a time, propagating to fixpoint after
 * each, and stops at the first conflict.  out_conflict[i] = 0 (fixpoint) or 1.
 * out_values (may be NULL) is n_instances rows of n_vars bytes:
 * 1 true, -1 false, 0 unassigned; for a conflicting instance the row holds the
 * assignment at the moment the conflict was found and is not comparable.
 * out_trail_len[i] (may be NULL) = number of assigned literals.
 * `repeat` > 1 re-runs the same batch that many times inside the call (device
 * state reset each time) for timing.  Returns 0 or a negative error. */
int mi355sat_propagate_batch(mi355sat* s, const int32_t* decisions, const uint64_t* decision_offsets,
                             uint64_t n_instances, int8_t* out_values, uint64_t n_vars,
                             int32_t* out_conflict, int32_t* out_trail_len, int32_t repeat);

/* --- model (Solve::lit_val / full_solution) ------------------------------ */
/* After SAT: returns +lit if lit is true, -lit if false, 0 if unknown var / no model. */
int32_t mi355sat_val(mi355sat* s, int32_t lit);
/* Bulk model: out[v-1] = 1 / -1 (0 for a variable the solver never saw). */
int mi355sat_model(mi355sat* s, int8_t* out, uint64_t n_vars);
/* Model of instance i of the last mi355sat_solve_batch(). */
int mi355sat_model_of(mi355sat* s, uint64_t instance, int8_t* out, uint64_t n_vars);

/* --- Interrupt::interrupter / InterruptSolver::interrupt ------------------ */
/* Async, thread-safe, idempotent: only sets a flag that solve() polls between
 * kernel launches (and the kernels poll from pinned host memory).  The solve it stops returns
 * MI355SAT_INTERRUPTED and consumes the flag; an interrupt that arrives while no solve is running
 * stops the next solve / batch / sweep at once (it is not lost) and is consumed by that one. */
void mi355sat_interrupt(mi355sat* s);

/* --- SolveStats::stats ----------------------------------------------------- */
int mi355sat_stats(const mi355sat* s, mi355sat_stats_t* out);

/* Test hook: the learnt clauses currently in the exchange ring of the last solve / batch / sweep, as DIMACS
 * literals, each clause 0-terminated.  out may be NULL to size the buffer; *n_records receives the number of
 * clauses.  Every one of them must be a consequence of the caller's formula alone (workers attach them under
 * any assumption set) - tests/ prove that with the oracle.  Returns 0, or MI355SAT_ERR_ARG if cap_words is
 * too small. */
int mi355sat_debug_share_ring(mi355sat* s, int32_t* out, uint64_t cap_words, uint64_t* n_records);

/* Test hooks: the formula the workers actually receive.  Armed (on != 0) before a solve / batch / sweep, the handle keeps
 * a copy of what the simplification before search (opts.simp) left at that call's cold start; it costs nothing unless
 * armed, and on = 0 drops the copy.  mi355sat_debug_simplified() hands it out as clauses of DIMACS literals in the caller's
 * variables, each clause 0-terminated:
 *   which 0: the remaining clauses, every level-0 fact as a one-literal clause, both binary clauses of every
 *            substitution by an equivalent literal - and the empty clause (a lone 0) if the simplification refuted the formula;
 *   which 1: the clauses kept aside for the eliminated variables (opts.simp = 2), from which a model gets their values.
 * Every clause of both lists is a consequence of the caller's formula; without elimination list 0 is equivalent to it -
 * tests/ prove both with the oracle.  out may be NULL to size the buffer; *n_words receives the length in words,
 * *n_clauses the number of clauses.  MI355SAT_ERR_ARG if cap_words is too small, MI355SAT_ERR_STATE if nothing was kept. */
int mi355sat_debug_keep_simplified(mi355sat* s, int on);
int mi355sat_debug_simplified(mi355sat* s, int which, int32_t* out, uint64_t cap_words, uint64_t* n_words, uint64_t* n_clauses);

/* Test hooks: which build of the search kernel a launch runs.  ms_search_kernel<LV, WPS> exists in six builds (assignment
 * staged in LDS or left in the worker's slab; compiled for 1, 2 or 4 waves per SIMD) and every launch picks one from the
 * number of workers it runs, opts.one_per_simd, opts.lds_val and an LDS budget (150 KB per CU shared by the launch's
 * workers per CU, minus a workgroup's static LDS, at most 64 KB).  tests/ force each build and assert here that it ran. */
typedef struct mi355sat_search_build {
    int32_t  lds;              /* 1 = assignment and marks in LDS, 0 = in the slab */
    int32_t  wps;              /* waves per SIMD the build was compiled for: 1, 2 or 4 (0: not a search launch) */
    uint32_t dyn_lds_bytes;    /* dynamic LDS per workgroup of the launch (0 unless lds) */
    uint32_t active;           /* workers (workgroups of one wavefront) the launch ran */
    uint32_t lds_val_bytes;    /* what staging this formula's assignment and marks takes */
    uint32_t builds_seen;      /* bit (3 * lds + {wps 1: 0, 2: 1, 4: 2}) set for every build the handle has launched so far */
    uint64_t launches;         /* search launches of the handle so far */
} mi355sat_search_build;
/* The build of the handle's last search launch; MI355SAT_ERR_STATE before the first one. */
int mi355sat_debug_last_search_build(const mi355sat* s, mi355sat_search_build* out);
/* The selection rule alone, nothing is launched (no handle, no device): what a launch of `active` >= 1 workers would run for
 * a formula of lds_val_bytes under opts.lds_val / opts.one_per_simd.  mode 0 = search (else BCP / probing: wps 0).  staged =
 * the handle's own LDS decision for the kernels without a budget rule (1 / 0), or -1 to derive it as a solve does.
 * builds_seen and launches stay 0. */
int mi355sat_debug_search_build_rule(uint32_t active, uint32_t lds_val_bytes, int32_t staged, int32_t lds_val,
                                     int32_t one_per_simd, int32_t mode, mi355sat_search_build* out);

/* --- warm incremental solve ------------------------------------------------ */
/* on != 0: mi355sat_solve() keeps what the solve before it built and learnt.  Default off: every solve prepares the
 * formula from scratch, as documented above.  With it on, a solve starts WARM when the workers of the handle's previous
 * mi355sat_solve() are still on the device and only clauses and / or assumptions were added since: no simplification,
 * no upload, no reset - the new clauses are mapped to device literals and attached to every resident worker
 * (ms_attach_kernel), the assumptions are rewritten, and the search goes on with every worker's learnt clauses, saved
 * phases, decision order, restart averages and the exchange ring.  Otherwise it starts COLD (the path above, unchanged);
 * the fallback is silent and counted (mi355sat_debug_incremental).  A solve starts cold when
 *   - it is the handle's first, or the one before it failed;
 *   - a new clause or assumption names a variable above the highest one of the last cold start (mi355sat_reserve()
 *     the variables you are going to need BEFORE the first solve to avoid this);
 *   - a new clause or assumption names a variable that opts.simp = 2 eliminated;
 *   - there are more assumptions than the slabs have room for (the count at the last cold start + 256);
 *   - a proof path is set, or opts.cube_split is on;
 *   - the clauses attached warm since the last cold start would take more than a quarter of a worker's learnt-clause
 *     slots or literal store (they are kept there for ever), or a worker's store or watch pool ran full attaching them;
 *   - mi355sat_solve_batch(), mi355sat_sweep_begin() or mi355sat_propagate_batch() ran on the handle in between (they
 *     stay cold and take the device state over), or mi355sat_check_proof() / _trim_proof(), or a
 *     mi355sat_minimize_core() that posed candidates: MI355SAT_COLD_OTHER_SEARCH;
 *   - the mode was switched off in between (that drops what is resident, also when it is switched on again at once), or
 *     mi355sat_debug_set_schedule() changed what a worker's state depends on, or the solve before logged a proof (it
 *     leaves nothing resident): MI355SAT_COLD_FIRST.
 * mi355sat_phase() / _set_phases() and an interrupt never make a solve start cold.
 * A handle whose formula was refuted without assumptions answers every later solve UNSAT with the empty core at once.
 * The IPASIR state rules do not change: assumptions are consumed, failed / core are valid straight after UNSAT only,
 * an interrupt is not lost; an interrupted or budget-exhausted solve leaves the handle warm.  Returns 0. */
int mi355sat_set_incremental(mi355sat* s, int on);

#define MI355SAT_COLD_NONE 0            /* no cold start yet */
#define MI355SAT_COLD_FIRST 1           /* nothing resident: first solve, or the solve before failed */
#define MI355SAT_COLD_NEW_VAR 2
#define MI355SAT_COLD_ELIMINATED 3
#define MI355SAT_COLD_PROOF 4
#define MI355SAT_COLD_CUBE_SPLIT 5
#define MI355SAT_COLD_PINNED_SHARE 6
#define MI355SAT_COLD_OTHER_SEARCH 7    /* solve_batch / sweep_* / propagate_batch / check_proof / trim_proof / minimize_core in between */
#define MI355SAT_COLD_ASSUMP_CAP 8
#define MI355SAT_COLD_DEVICE_FULL 9     /* a worker's learnt store or watch pool ran full during the attach */
/* Test hook: what the incremental mode did on this handle so far. */
typedef struct mi355sat_incremental_info {
    int32_t  enabled;
    int32_t  last_cold_reason;     /* MI355SAT_COLD_* of the last solve() that started cold with the mode on */
    uint64_t warm_solves;          /* solve() calls that started warm (or were answered from a refuted formula) */
    uint64_t cold_solves;          /* solve() calls that started cold with the mode on */
    uint64_t attached_clauses;     /* clauses of two and more literals handed to the resident workers so far */
    uint64_t attached_units;       /* one-literal clauses handed to them so far */
    uint64_t resident_learnts;     /* learnt clauses in the workers' stores when the last warm solve began, summed */
    uint64_t attach_launches;      /* ms_attach_kernel launches so far */
} mi355sat_incremental_info;
int mi355sat_debug_incremental(const mi355sat* s, mi355sat_incremental_info* out);

/* Test hook: what the optional heuristics did, summed over the workers of the last solve / batch / sweep. */
typedef struct mi355sat_heuristics_info {
    uint64_t n_vivified;           /* opts.vivify: learnt clauses a vivification pass shortened */
    uint64_t n_viv_lits;           /*              literals it removed from them */
    uint64_t n_rephase;            /* opts.rephase: times a worker reset its saved phases to its best assignment */
    uint64_t import_skipped;       /* opts.import_pct: exchanged records of three and more literals a worker passed over */
    uint64_t forced_imports;       /* opts.share_interval: imports for which a worker gave up its search path (backtracked
                                    * to level 0 in mid-search) */
} mi355sat_heuristics_info;
int mi355sat_debug_heuristics(const mi355sat* s, mi355sat_heuristics_info* out);
/* Test hook: when the optional heuristics run, in conflicts of one worker: the first vivification pass (default 1500) and
 * the distance between passes (400); the first rephasing, the n-th one following n + 1 times as long after its
 * predecessor (2000).  0 keeps the default; the two periods are at most 65535.  Takes effect with the next solve. */
int mi355sat_debug_set_schedule(mi355sat* s, uint32_t first_vivify, uint32_t vivify_every, uint32_t rephase_every);

/* --- when a device store is full ------------------------------------------- */
/* Every worker has four stores of fixed size, laid out at a cold start: learnt-clause slots, learnt literals, the watch
 * pool and (with a proof path) its proof log.  The default sizes are thousands of times what a short solve needs.
 *   - Learnt store (slots or literals): a worker reduces its clause database early once either passes 7/8 of its
 *     capacity, and again on the spot when a clause finds the store full.  A reduction keeps binary clauses, clauses of
 *     LBD <= 2, clauses used since the last reduction with LBD <= 6 and the reasons of assigned literals.  If nothing
 *     could go, a clause the worker learnt itself (or one the caller added warm) ends the solve: MI355SAT_ERR_OOM, "device
 *     learnt-clause store exhausted".  A clause received from another worker (the exchange, mi355sat_share_import) is
 *     optional and never ends a solve: it is attached only while a quarter of the slots and of the literal words stays
 *     free (one of three and more literals: only while the slots are at most half full); otherwise it is passed over
 *     (three quarters full: counted, imports_dropped_full below) and the solve goes on.
 *   - Watch pool: lists that outgrow their slot move to the top of the pool; the holes are collected at every reduction
 *     and whenever the top passes 3/4 of the pool.  A list that cannot grow, or a collection that does not fit, ends the
 *     solve: MI355SAT_ERR_OOM, "device watch pool exhausted".
 *   - Proof log (drained after every slice): lemmas fill it from the bottom, deletion lines from the top; deletion lines
 *     that do not fit are left out, and those in the way of a lemma are given up - the proof stays valid without them.
 *     Only when the lemmas of one slice alone do not fit does the solve end: MI355SAT_ERR_OOM, "proof buffer overflow
 *     ..."; the proof file is closed, truncated.  In the file a slice's deletion lines follow its lemmas.
 * After any of these the handle is usable: failed / core answer MI355SAT_ERR_STATE, and the next solve starts cold
 * (MI355SAT_COLD_FIRST with the incremental mode on).  During a warm attach a full store is no error: that solve starts
 * cold instead (MI355SAT_COLD_DEVICE_FULL).
 *
 * Test hooks: the sizes of those stores.  mi355sat_debug_set_capacities() replaces the sizing rules from the next cold start
 * of mi355sat_solve / _solve_batch / _sweep_begin / _minimize_core on (mi355sat_check_proof keeps sizing its stores from the
 * proof; mi355sat_propagate_batch keeps the rules); each argument 0 = the rule.  learnt_cap: clause slots per worker, 4 ..
 * 2^17; learnt_lit_cap: literal words, 64 .. 2^21; pool_slack: the watch pool is the initial lists (pool_initial below)
 * plus that many entries, at most 2^30; proof_cap: words per worker, 8 .. 2^23.  Anything else: MI355SAT_ERR_ARG.  Workers
 * that are resident (incremental mode) keep the layout they have. */
int mi355sat_debug_set_capacities(mi355sat* s, uint32_t learnt_cap, uint32_t learnt_lit_cap, uint32_t pool_slack, uint32_t proof_cap);
typedef struct mi355sat_capacity_info {
    uint32_t learnt_cap, learnt_lit_cap, pool_cap, pool_initial, proof_cap, assump_cap, vm_cap, pad;
    uint64_t pressure_reduces;     /* reduce_db runs that conflicts did not make due: the 7/8 rule and add_learnt's inline one */
    uint64_t pool_rebuilds;        /* rebuild_watches because pool_top passed 3/4 of pool_cap */
    uint64_t imports_dropped_full; /* exchanged records passed over because the store had no room to spare */
} mi355sat_capacity_info;
/* The layout of the last cold start of a search (proof_cap 0: no proof was logged) and the three counts summed over the
 * workers of the last solve / batch / sweep; MI355SAT_ERR_STATE before the first cold start. */
int mi355sat_debug_capacities(const mi355sat* s, mi355sat_capacity_info* out);

/* Clause exchange BETWEEN handles that search the SAME formula - the replicas of the sharded loop's last bounds, one
 * handle per GPU (every rank poses the reference's next bound, crates/repl/src/main.rs:292-295, with its own
 * seed).  Inside one handle the workers pass their short / low-LBD learnt clauses on through a ring on the device;
 * export hands out the records that entered the ring since the last export (never one that was imported), import
 * appends records from another handle so that this handle's workers attach them like each other's.  Wire format, in
 * the caller's variables: [lbd >= 1, DIMACS literals ..., 0] per clause.  Every record is a consequence of the
 * caller's formula alone (the tests prove it with the oracle), so it may be attached under any assumptions.  Both
 * calls are made between two mi355sat_sweep_step() of a running sweep; without one (or with the exchange off) they
 * do nothing.  export: out may be NULL to size the buffer (nothing is consumed); records that do not fit cap_words
 * wait for the next call.  import: *n_records counts the records taken; a record is passed over when it is longer than
 * the ring's 31 literals, names a variable this handle does not know or has eliminated (opts.simp = 2), or holds a
 * literal and its negation once it is written in this handle's variables (its own equivalent-literal substitution may
 * join what the exporter kept apart); a literal that the substitution makes appear twice is kept once. */
int mi355sat_share_export(mi355sat* s, int32_t* out, uint64_t cap_words, uint64_t* n_words, uint64_t* n_records);
int mi355sat_share_import(mi355sat* s, const int32_t* clauses, uint64_t n_words, uint64_t* n_records /* may be NULL */);

/* Optional DRUP proof (text, DIMACS literals, one lemma per line, the empty clause last) of the next plain
 * solve() - under assumptions, the clause of the negated core literals instead of the empty clause - in its default
 * configuration: all workers, clause exchange on.  Order of the lines: what the
 * simplification derived, then after every kernel slice the clauses each worker learnt in it; every line is a
 * RUP consequence of the lines before it (the exchange only hands on clauses of earlier slices).  Deletion lines
 * ("d ...") are written for the clauses a worker drops when it reduces its clause database - except those another
 * worker may hold a copy of (exchanged or imported ones).  Must be called before solve(); path NULL disables.
 * A slice's logs come back in one piece: ms_proof_gather_kernel packs the non-empty logs, rewritten to the caller's
 * literals, into one buffer and one copy fetches it (one wavefront per non-empty log; a plain solve's file is byte for
 * byte what the copy per worker wrote before).
 *
 * mi355sat_solve_batch() and mi355sat_sweep_begin() .. _sweep_end() log ONE file for the whole call in the same way: the
 * lemmas of all workers of all instances are one derivation from the caller's formula (assumptions are decisions, so a
 * learnt clause follows from the formula alone), and behind the lemmas of the slice that decides an instance UNSAT stands
 * one more line for it: the clause of its negated core, in the caller's literals; several in one slice in instance order.
 * Every line is RUP with respect to the lines before it; a core line is never the subject of a deletion line.  The empty
 * clause - the core of a formula that is refuted whatever the assumptions, by a worker or by the simplification - is
 * written at most once per file; for a core that holds a literal and its negation (a tautology) nothing is written; an
 * instance answered UNSAT at once when it is reopened adds no line.  So the file certifies every UNSAT verdict of the
 * call: mi355sat_check_proof_targets_file() with the negated cores as targets checks them all in one pass, and
 * mi355sat_trim_proof_file() works per instance, each core line being an ordinary lemma of the file.  The file is closed
 * at the end of solve_batch, by mi355sat_sweep_end, by an error of a step (it then ends where the error came, as a failed
 * solve()'s) and by mi355sat_free; after an interrupt or an exhausted budget it is a valid prefix.  A sweep computes
 * final-conflict cores only while it logs a proof (mi355sat_sweep_core_of); without a path it launches what it did
 * before.  While a proof is logged mi355sat_share_import takes no record (*n_records = 0): a foreign clause has no
 * derivation in this file.  opts.cube_split = 1 with more than one instance is refused under a proof path, the warm
 * incremental mode stays cold, mi355sat_minimize_core logs nothing. */
int mi355sat_set_proof_path(mi355sat* s, const char* path);
/* The core of an instance that has reported UNSAT in the running sweep, between mi355sat_sweep_begin and _sweep_end of a
 * sweep that logs a proof; sizing and errors as mi355sat_core_of.  In any other state: MI355SAT_ERR_STATE. */
int mi355sat_sweep_core_of(mi355sat* s, uint64_t instance, int32_t* out, uint64_t cap, uint64_t* n);
/* Test hook: what writing the proof file open now (or closed last) took.  drains: calls after a slice, drain_seconds their
 * wall time (lengths, kernel, copy, text); gathers: those that found a non-empty log and launched ms_proof_gather_kernel;
 * logs / words: non-empty logs and words they packed; core_lines: negated cores written (the empty clause not counted). */
typedef struct mi355sat_proof_log_info {
    uint64_t drains, gathers, logs, words, core_lines;
    double   drain_seconds;
} mi355sat_proof_log_info;
int mi355sat_debug_proof_log(const mi355sat* s, mi355sat_proof_log_info* out);

/* Check a DRUP proof on the device: a certificate for an UNSAT answer (ms_rup_kernel).
 * Semantics: forward RUP with deletions ignored.  Lemma i must follow by unit propagation from the handle's clauses plus
 * the lemmas before i; `target` - the clause the proof must derive, n_target = 0: the empty clause; for a solve under
 * assumptions the negated core, which is the last line of the file mi355sat_set_proof_path writes - is checked as the last
 * lemma, number n_lemmas.  Deletion lines are parsed, counted and ignored: every clause in the database is an original or
 * a checked lemma and unit propagation is monotone, so this is sound, every valid DRUP proof passes, and the verdict is a
 * function of formula, proof and target alone - not of `segments`, the worker count or the build.  A lemma that holds a
 * literal and its negation counts as RUP.  Once formula + lemmas are refuted by propagation alone (refuted_at) every later
 * lemma is RUP trivially.
 * Trusted base: the handle's clauses as the caller added them - no simplification, the caller's variable order; the
 * handle need not have solved anything (new, add_cnf, check_proof is a valid sequence).
 * How: the lemma list (target included) is cut into `segments` contiguous parts (0 = the default: as many as the handle
 * would use workers, at most n_lemmas + 1, fewer if device memory does not hold that many slabs); one wavefront per part
 * attaches the lemmas before its part unchecked and checks its own.  Each worker holds a private copy of the lemmas
 * up to the end of its part.
 * proof: flat int32, lemmas 0-terminated, a deletion line = INT32_MIN, then the clause, then 0 (what the Python
 * dimacs.read_drup returns).  A literal whose variable is above the handle's highest (mi355sat_reserve raises that), or an
 * INT32_MIN inside a clause, is MI355SAT_ERR_ARG, found on the host before anything is uploaded.
 * Returns 0 when the check ran to its end: out->valid is the verdict.  An interrupted check returns
 * MI355SAT_INTERRUPTED (which is 0 as well) with out->valid = -1: no verdict; the call consumes the interrupt, and one
 * that arrived before the call stops it before the first launch, as for a solve.  During a mi355sat_sweep_*:
 * MI355SAT_ERR_STATE.  The call takes the device over as solve_batch does (with the incremental mode on, the next
 * solve() starts cold: MI355SAT_COLD_OTHER_SEARCH); assumptions, failed / core and the phase hints are untouched;
 * n_sat / n_unsat / n_terminated do not count it; solve_seconds, kernel_seconds and kernel_launches accumulate. */
typedef struct mi355sat_proof_info {
    int32_t  valid;              /* 1: every lemma is RUP in order and the target is RUP at the end; 0: not; -1: interrupted */
    int32_t  pad;
    uint64_t n_lemmas;           /* lemma lines (deletion lines not counted); the target is lemma number n_lemmas */
    uint64_t n_deletions_ignored;
    uint64_t first_failed;       /* smallest lemma index (0-based, target = n_lemmas) that is not RUP; UINT64_MAX if none */
    uint64_t refuted_at;         /* smallest lemma index at which formula + lemmas before it are refuted by unit propagation alone; UINT64_MAX if never */
    uint64_t segments, workers;  /* how the proof was cut, and how many wavefronts checked it */
    uint64_t lemmas_checked, lemmas_attached;   /* summed over workers (attached counts the unchecked prefixes) */
    uint64_t propagations;
    uint64_t launches;
    double   seconds, kernel_seconds;
} mi355sat_proof_info;
int mi355sat_check_proof(mi355sat* s, const int32_t* proof, uint64_t n_words,
                         const int32_t* target, uint64_t n_target, uint32_t segments, mi355sat_proof_info* out);
/* The same for a DRUP text file as mi355sat_set_proof_path writes it ("d ..." = a deletion line). */
int mi355sat_check_proof_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target,
                              uint32_t segments, mi355sat_proof_info* out);
/* Several targets in one pass: what certifies every UNSAT verdict of a batch or a sweep from the one file it logged
 * (mi355sat_set_proof_path).  The lemmas are checked exactly as mi355sat_check_proof checks them; target t =
 * targets[target_offsets[t] .. target_offsets[t + 1]) is item number n_lemmas + t.  Each target is checked against the
 * formula plus ALL lemmas; none is ever attached, so targets do not see each other.  target_valid[t] = 1 when target t
 * is RUP, or holds a literal and its negation, or the database is refuted by then; 0 otherwise; every entry is -1 when
 * the call was interrupted.  out->valid = 1 iff every lemma and every target passes; first_failed is the smallest failing
 * item, a target counting as n_lemmas + t.  refuted_at, segments (the n_lemmas + n_targets items are cut as before), the
 * counters, the argument and state errors, "takes the device over", the interrupt and the statistics are those of
 * mi355sat_check_proof; n_targets = 0 is MI355SAT_ERR_ARG; with n_targets = 1 every field equals what
 * mi355sat_check_proof reports for the same inputs.  With mi355sat_proof_deletions on, all targets are checked after
 * the last line: the deletion lines behind the last lemma are honoured once, each target is then propagated over the
 * caller's clauses, the live lemmas and the facts, and none joins.  Trimming stays per target (mi355sat_trim_proof).
 * Measured (MI355X, profiles/r12_sweep_proof.log): logging rect 24x24 k = 8 with 1024 workers, a solve takes
 * 3.9-4.4 s with the gathered drain beside 5.2-5.4 s with the parent commit's copies per worker (134-144 ms per slice in
 * the drain, nearly all of it text); a deterministic sweep of the rect 24x24 bounds 10 .. 0 takes 1064 ms per step with a
 * proof beside 152 ms without (87 % in the drains: a file of 962 MB).  One pass over that file's 9 targets against one
 * check per bound: unmeasured - with deletion lines ignored its 1 958 730 lemmas do not fit the checker's stores. */
int mi355sat_check_proof_targets(mi355sat* s, const int32_t* proof, uint64_t n_words, const int32_t* targets,
                                 const uint64_t* target_offsets, uint64_t n_targets, uint32_t segments,
                                 int32_t* target_valid /* n_targets */, mi355sat_proof_info* out);
int mi355sat_check_proof_targets_file(mi355sat* s, const char* path, const int32_t* targets, const uint64_t* target_offsets,
                                      uint64_t n_targets, uint32_t segments, int32_t* target_valid /* n_targets */,
                                      mi355sat_proof_info* out);
/* Test hook: at most this many lemmas (checked or attached) per worker per launch, and no time bound; 0 = the default
 * (launches of about 20 ms). */
int mi355sat_debug_proof_check_chunk(mi355sat* s, uint32_t max_lemmas_per_launch);

/* Honour the deletion lines of a proof (on != 0) in mi355sat_check_proof / _check_proof_file / _trim_proof /
 * _trim_proof_file and what _trim_write_drup / _trim_write_lrat write of such a trim.  A switch on the handle, off by
 * default; off is the behaviour described above, bit for bit.  With it on a worker keeps only the lemmas that are live, so
 * its clause store and watch pool are sized from the PEAK of the live lemmas instead of their number: proofs whose
 * lemmas do not fit a worker's stores all at once become checkable, and a proof that uses a lemma after deleting it is
 * found out.  The verdict stays a function of formula, proof and target alone.
 * Resolution, on the host before anything is uploaded.  A deletion line names a clause by its literals as a set (order
 * and repeats do not matter).  It is matched to the latest lemma line before it with the same literal set that is still
 * live; two lemma lines with the same literals are two clauses and one deletion removes one of them.  A line without a
 * live match that equals one of the caller's clauses is counted ignored_original and has no effect (original clauses are
 * never deleted: sound, and the same in every worker); any other line without a match - a deletion before its lemma, a
 * second deletion of one copy - is counted ignored_unmatched.  A match to a tautological lemma counts as honoured and
 * does nothing: such a lemma is never attached.
 * State.  Live: a set of lemma indices.  Facts: a set of literals that only grows.  close() sets Facts to the
 * unit-propagation closure of originals + Live + Facts; a conflict there is refuted_at = min(.., the item in front of
 * which it happened).
 * Run, items in file order.  A maximal run of consecutive deletion lines in front of item j is a group: close() once,
 * then the group's matched lemmas leave Live.  At item j: close(); lemma j is RUP iff propagating its negation over
 * originals + Live + Facts ends in a conflict; then j joins Live (a failed lemma too, the target not; a tautology counts
 * as RUP without joining).  Facts outlive the clauses that gave them: deleting a unit lemma, or the clause behind a
 * level-0 fact, takes nothing back (drat-trim's default reading).  A clause that is the reason of a fact is therefore
 * satisfied for ever, and whether a worker keeps or drops it changes no verdict: the device keeps it ("locked").
 * valid, first_failed, refuted_at and n_lemmas keep their meaning; n_deletions_ignored = ignored_original +
 * ignored_unmatched.  Sizes: learnt_cap = peak_live_lemmas + min(n_vars + 1, honoured lemmas) - the slack is for locked
 * clauses, one per variable at most - and the literal store likewise with the longest of the deleted lemmas as slack; the
 * watch pool follows learnt_cap.  A store that still fills ends the call with MI355SAT_ERR_OOM, never with a verdict.
 * A trim keeps its formats (ids as before, no deletion lines written); a hint names a lemma the proof had deleted by
 * then only if that lemma was locked.
 * Measured (MI355X, profiles/r10_proof_deletions.log).  rect 16x16 k = 3, the 16-worker fleet's proof (2468
 * lemmas, no deletion line): 0.009 s with the switch off - the parent commit's library takes the same - and 0.013 s with
 * it on, the same slabs and 256 segments.  rect 24x24 k = 8, the fleet's proof (157 278 lemmas, 136 460 deletion lines,
 * 150 MB; solved in 5.1 s): off, MI355SAT_ERR_OOM as before; on, valid in 4.5 s with 1024 segments, at most 22 310 lemmas
 * live, learnt_cap 34 526, 22.6 MiB of stores and pool per worker; the trim with hints takes 10.8 s. */
int mi355sat_proof_deletions(mi355sat* s, int on);
typedef struct mi355sat_proof_del_info {
    /* functions of the proof (and the caller's clauses) alone */
    uint64_t honoured, ignored_original, ignored_unmatched;
    uint64_t groups;                    /* maximal runs of consecutive deletion lines */
    uint64_t peak_live_lemmas;          /* the largest Live ever gets */
    uint64_t peak_live_words;           /* ... in literal words, each lemma (repeats dropped) rounded up to 4 as the store rounds it */
    /* what the slabs were laid out with (0: the call needed no launch) */
    uint64_t learnt_cap, learnt_lit_cap, pool_cap;
    /* summed over workers: they may differ from cut to cut and from run to run, as the core of a trim does */
    uint64_t skipped_locked;            /* deleted lemmas a worker kept: the reason of a fact when they died, or a fact from
                                           the moment they were attached (one free literal) */
    uint64_t compactions;               /* passes over a worker's store, one per group that names an attachable lemma */
} mi355sat_proof_del_info;
/* The last check or trim made with the switch on; MI355SAT_ERR_STATE before the first one. */
int mi355sat_debug_proof_deletions(const mi355sat* s, mi355sat_proof_del_info* out);


/* Trim a DRUP proof while it is checked: which of the caller's clauses and which lemmas the derivation of the target
 * rests on, and - with MI355SAT_TRIM_HINTS - an LRAT file that a checker without watch lists, search or GPU verifies
 * (DESIGN.md 4).  The check is mi355sat_check_proof's, in a tracing build of the same kernel: `check` holds exactly what
 * mi355sat_check_proof reports for the same inputs, and argument errors, the interrupt, "takes the device over", the
 * IPASIR state, the phase hints and n_sat / n_unsat / n_terminated behave as there.  Whenever a check ends in a
 * conflict the worker walks its trail back from it and writes the clauses it passes to a log of its own; the host
 * drains the logs after every launch, maps them to the caller's clauses and, once the proof is found valid, reaches
 * backwards from the target.
 * Indices: caller clause i is the i-th clause the handle was given, 0-based (mi355sat_add_cnf order, each clause closed by
 * mi355sat_add(0)); a clause given twice is named by its first index.  Lemma j is the j-th lemma line, 0-based.  LRAT
 * ids: clause i has id i + 1, lemma j has n_clauses + 1 + j, the target n_clauses + 1 + n_lemmas; a line is
 * "id literals 0 hints 0"; the needed lemmas in order, then the target; no deletion lines.  A tautological target rests
 * on nothing: empty core, no lemma, no LRAT line.  When the caller's clauses hold an empty clause or two contradictory
 * units, the core is that clause or pair and the file is the target's line alone.
 * The verdict, first_failed and refuted_at are functions of formula, proof and target alone.  WHICH clauses end up in
 * the core is not: unit propagation picks one of several clauses that give the same literal at the same moment, so the
 * sets may differ with `segments` and from run to run.  Every one of them passes the checks named above.
 * The result stays on the handle until the next mi355sat_trim_proof / mi355sat_check_proof, a clause added, a sweep begun
 * or mi355sat_free; without one - also after a trim whose verdict was not valid == 1 or that was interrupted - the four
 * calls below return MI355SAT_ERR_STATE.  Both index calls: out NULL sizes (*n), a cap too small is MI355SAT_ERR_ARG. */
#define MI355SAT_TRIM_HINTS 1u          /* keep the hints: needed for mi355sat_trim_write_lrat */
typedef struct mi355sat_trim_info {
    mi355sat_proof_info check;          /* exactly what mi355sat_check_proof reports for the same inputs */
    uint64_t core_clauses, lemmas_needed;      /* sizes of the two sets (0 unless check.valid == 1) */
    uint64_t dep_records;               /* records drained from the device */
    uint64_t log_drains;                /* launches after which a region was non-empty */
    uint64_t log_words_per_worker;
} mi355sat_trim_info;
int mi355sat_trim_proof(mi355sat* s, const int32_t* proof, uint64_t n_words, const int32_t* target, uint64_t n_target,
                        uint32_t segments, uint32_t flags, mi355sat_trim_info* out);
int mi355sat_trim_proof_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target,
                             uint32_t segments, uint32_t flags, mi355sat_trim_info* out);
int mi355sat_trim_core(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n);     /* caller clause indices, ascending */
int mi355sat_trim_lemmas(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n);   /* lemma indices, ascending */
int mi355sat_trim_write_drup(mi355sat* s, const char* path);   /* the needed lemmas in order, then the target */
int mi355sat_trim_write_lrat(mi355sat* s, const char* path);   /* MI355SAT_ERR_STATE without MI355SAT_TRIM_HINTS */
/* Test hook: words per worker of the dependency log; 0 = the rule (2^18, less for large fleets); never below two items of
 * the largest size (8 * (n_vars + 3) words): a worker ends its launch when less than that is free. */
int mi355sat_debug_trim_log(mi355sat* s, uint32_t words_per_worker);

/* Check an LRAT file on the device: the certificate at the end of the chain (ms_lrat_kernel).  What
 * mi355sat_trim_write_lrat writes is verified here by a kernel that shares nothing with the propagation code whose answer
 * it certifies - and by any LRAT checker a third party brings.
 * Semantics: strict, exactly those of tests/lrat_check.py.  Trusted base: the handle's clauses as the caller added them;
 * clause i, 0-based in add order, has id i + 1; no simplification, the caller's variables; new, add_cnf, check_lrat is a
 * valid sequence.  A line is `id literals 0 hints 0`.  It is accepted when, under the negation of its literals, the hinted
 * clauses are, in the order given, unit one after the other, and the last one is falsified.  Free literals count as a
 * set (a clause that repeats its one free literal is unit); a hinted clause that holds x and -x is satisfied if x is
 * assigned and has two free literals if not.  The smallest rejected line index is the file's verdict; within a line the
 * reasons have this precedence: */
#define MI355SAT_LRAT_ID_ORDER 1               /* id not above the originals' / not increasing */
#define MI355SAT_LRAT_TAUTOLOGY 2              /* the line's clause holds a literal and its negation */
#define MI355SAT_LRAT_NO_HINTS 3
#define MI355SAT_LRAT_BAD_HINT 4               /* at its turn: the hint is neither an original nor an earlier line */
#define MI355SAT_LRAT_HINT_SATISFIED 5         /* at its turn: the hinted clause has a true literal (free ones or not) */
#define MI355SAT_LRAT_HINT_NOT_UNIT 6          /* two or more DISTINCT free literals */
#define MI355SAT_LRAT_HINT_FALSIFIED_EARLY 7   /* falsified before the last hint */
#define MI355SAT_LRAT_LAST_NOT_FALSIFIED 8     /* the last hint leaves a free literal */
/* target as in mi355sat_check_proof (n_target = 0: the empty clause): derives_target = 1 iff the last line's literals
 * equal the target as a set; a tautological target is derived by any file (the trimmer writes no line for one).
 * valid = accepted && derives_target.
 * lines: flat int32, `id, literals, 0, hints, 0` per line.  Input that is not LRAT at all is MI355SAT_ERR_ARG, found on the
 * host before anything is uploaded or launched, with the text in mi355sat_last_error: a line that is not integers, a
 * missing terminator, a deletion line (`id d ...`), a zero or negative hint or id, a literal whose variable is above the
 * handle's highest (mi355sat_reserve raises that).
 * How: the caller's clauses and the lines are one read-only database; every hint id is rewritten on the host to a clause
 * index of it (an id that names nothing earlier: a sentinel the device reports at the hint's turn).  One wavefront per
 * line, workgroups of one wavefront, the lines of a launch strided over at most 4096 of them; lines go in file order in
 * launches of 2^24 hints (about 20 ms at the measured 7e8 hints a second), the interrupt is polled between launches, and the
 * first launch with a rejection ends the call.
 * The wave's assignment map is 2 bits per variable in LDS, cleared per line, when opts.lds_val forces it (up to 64 KB) or, on
 * auto, when it takes at most 9.4 KB (16 workgroups per CU in the 150 KB the search builds budget); else one stamped word per
 * variable and wave in HBM that is never cleared.  A hostile file can produce a rejection and nothing else: after the
 * host's validation no index the kernel uses comes unvalidated from the file, and the kernel itself refuses a hint that is
 * not below the line's own index.
 * Returns 0 when the check ran to its end; MI355SAT_INTERRUPTED (0 as well) with accepted = -1 when interrupted: the call
 * consumes the interrupt, and one that arrived before the call stops it before the first launch (also a call whose file
 * needs no launch).  A call refused with an error still writes *out (nothing accepted, nothing rejected) once its
 * arguments are not NULL, and ends the result mi355sat_lrat_used held.  During a
 * mi355sat_sweep_*: MI355SAT_ERR_STATE.  The call owns its device buffers and does not touch the worker slabs: assumptions,
 * failed / core, the phase hints, a trim result on the handle (trim, check_lrat_file, trim_core in sequence works) and what
 * is resident for a warm incremental solve all stay - the next solve() still starts warm.  n_sat / n_unsat / n_terminated
 * do not count the call; solve_seconds, kernel_seconds and kernel_launches accumulate.
 * Measured (MI355X, profiles/r11_lrat_check.log: scripts/gpu_lrat_check.py, beside tests/lrat_check.py on the same file, three
 * runs each way, alternating).  rect 16x16 k = 3, the fleet's trimmed proof (144 lines, 25 873 hints, 163 KB):
 * 0.001-0.002 s, kernel 0.9 ms, beside 0.016-0.018 s in Python.  rect 24x24 k = 8 (30 845 lines, 7 558 306 hints, clauses of up
 * to 466 literals, 52.9 MB): 0.16-0.17 s for the call - kernel 10.3 ms on 4096 waves, 0.028 s behind the parser, the rest the
 * host reading 53 MB of text - beside 5.0-5.1 s in Python and 7.0 s for the trim that produced the file.  Another solve of
 * that bound (42 296 lines, 9 789 662 hints, 71.0 MB): 0.18 s, kernel 8.9 ms in one launch, Python 6.1-6.3 s, trim 13.2 s;
 * with the map in HBM (lds_val = -1) the same 0.18 s and 8.7-8.8 ms. */
typedef struct mi355sat_lrat_info {
    int32_t  valid, accepted;        /* accepted: 1 every line accepted, 0 one rejected, -1 interrupted */
    int32_t  derives_target, reason; /* reason: MI355SAT_LRAT_* of the first rejected line, 0 if none */
    uint64_t n_lines, n_hints;       /* of the file */
    uint64_t first_rejected;         /* line index, 0-based; UINT64_MAX if none */
    uint64_t first_rejected_id;      /* its id as written */
    uint64_t reject_hint;            /* position of the offending hint in that line (reasons 4..8), else UINT64_MAX */
    uint64_t used_originals;         /* distinct caller clauses hinted (0 unless accepted == 1) */
    uint64_t longest_clause;         /* literals, over the caller's clauses and the lines uploaded */
    int32_t  lds;  uint32_t dyn_lds_bytes;   /* which build ran, as mi355sat_search_build reports it */
    uint64_t waves, launches;        /* wavefronts of the largest launch; launches */
    double   seconds, kernel_seconds;
} mi355sat_lrat_info;
int mi355sat_check_lrat(mi355sat* s, const int32_t* lines, uint64_t n_words, const int32_t* target, uint64_t n_target,
                        mi355sat_lrat_info* out);
/* The same for an LRAT text file, one line per clause, as mi355sat_trim_write_lrat writes it. */
int mi355sat_check_lrat_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target, mi355sat_lrat_info* out);
/* After a check that accepted every line (accepted == 1), until the next check or a clause added: the caller clauses some
 * line hinted, 0-based indices, ascending.  out NULL sizes (*n), a cap too small is MI355SAT_ERR_ARG, any other state
 * MI355SAT_ERR_STATE - as mi355sat_trim_core. */
int mi355sat_lrat_used(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n);
/* Test hook: at most this many lines per launch; 0 = the default (launches of about 20 ms: 2^24 hints). */
int mi355sat_debug_lrat_chunk(mi355sat* s, uint32_t max_lines_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* MI355SAT_H */
