/*
 * TEST INFRASTRUCTURE: replays, against the C ABI of libmi355sat.so, what the Rust shim (rust/mi355sat/src/lib.rs) calls
 * for a `SolveIncremental` user with `set_incremental(true)`:
 *
 *   new -> set_incremental(1) -> add_cnf -> reserve -> solve                              (cold)
 *       -> per step: add (per literal, 0 closes) -> assume x n -> solve -> core if UNSAT   (warm)
 *       -> debug_incremental -> free
 *
 * usage: abi_incremental <cnf.bin> <workers> <steps.txt>
 * cnf.bin:   int64 n_vars, int64 n_clauses, uint64 offsets[n_clauses+1], int32 lits[]   (DIMACS literals)
 * steps.txt: one step per line: "c l1 l2 ... 0" adds a clause, "a l1 l2 ... 0" solves under those assumptions
 * Prints "result R" per solve (+ "core N l1 ..." after UNSAT, "model v1 v2 ..." after SAT: the value of every variable),
 * then "incremental warm W cold C clauses A units U reason R"; exit 0 when every check passed.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/mi355sat.h"

static int solve_and_print(mi355sat* s, int64_t n_vars) {
    const int r = mi355sat_solve(s);
    if (r < 0) { fprintf(stderr, "solve failed (%d): %s\n", r, mi355sat_last_error(s)); return -1; }
    printf("result %d\n", r);
    uint64_t n = 0;
    if (r == MI355SAT_UNSAT) {
        if (mi355sat_core(s, NULL, 0, &n) != 0) return -1;
        int32_t* core = malloc(sizeof(int32_t) * (n + 1));
        if (mi355sat_core(s, core, n, &n) != 0) return -1;
        printf("core %llu", (unsigned long long)n);
        for (uint64_t k = 0; k < n; k++) {
            printf(" %d", core[k]);
            if (mi355sat_failed(s, core[k]) != 1) return -1;
        }
        printf("\n");
        free(core);
    } else {
        if (mi355sat_core(s, NULL, 0, &n) != MI355SAT_ERR_STATE) return -1;
        if (r == MI355SAT_SAT) {
            int8_t* m = malloc((size_t)n_vars + 1);
            if (mi355sat_model(s, m, (uint64_t)n_vars) != 0) return -1;
            printf("model");
            for (int64_t v = 0; v < n_vars; v++) printf(" %d", m[v]);
            printf("\n");
            free(m);
        }
    }
    return r;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[2];
    if (fread(h, 8, 2, f) != 2) return 2;
    const int64_t nv = h[0], nc = h[1];
    uint64_t* offs = malloc(8 * (size_t)(nc + 1));
    if (fread(offs, 8, (size_t)nc + 1, f) != (size_t)nc + 1) return 2;
    int32_t* lits = malloc(4 * (size_t)offs[nc] + 4);
    if (fread(lits, 4, offs[nc], f) != offs[nc]) return 2;
    fclose(f);

    mi355sat_opts o;
    memset(&o, 0, sizeof o);
    o.device = -1;
    o.workers = atoi(argv[2]);
    o.simp = -1;
    mi355sat* s = mi355sat_new(&o);
    if (!s) { fprintf(stderr, "mi355sat_new: %s\n", mi355sat_last_error(NULL)); return 3; }
    mi355sat_incremental_info info;
    if (mi355sat_debug_incremental(s, &info) != 0 || info.enabled != 0) return 4;       /* default: off */
    if (mi355sat_set_incremental(s, 1) != 0) return 4;
    if (mi355sat_add_cnf(s, lits, offs, (uint64_t)nc) < 0) return 4;
    if (mi355sat_reserve(s, (uint64_t)nv) != 0) return 4;
    int rc = 0;
    uint64_t solves = 1;
    if (solve_and_print(s, nv) < 0) return 5;
    if (mi355sat_debug_incremental(s, &info) != 0 || info.enabled != 1 || info.cold_solves != 1 || info.warm_solves != 0) rc = 6;

    FILE* st = fopen(argv[3], "r");
    if (!st) return 2;
    char kind;
    while (fscanf(st, " %c", &kind) == 1) {
        long l;
        while (fscanf(st, "%ld", &l) == 1 && l != 0) {
            if (kind == 'c' ? mi355sat_add(s, (int32_t)l) < 0 : mi355sat_assume(s, (int32_t)l) != 0) return 7;
        }
        if (kind == 'c') {
            if (mi355sat_add(s, 0) < 0) return 7;
        } else {
            if (solve_and_print(s, nv) < 0) return 8;
            solves++;
        }
    }
    fclose(st);
    if (mi355sat_debug_incremental(s, &info) != 0 || info.warm_solves + info.cold_solves != solves) rc = rc ? rc : 9;
    printf("incremental warm %llu cold %llu clauses %llu units %llu reason %d\n", (unsigned long long)info.warm_solves,
           (unsigned long long)info.cold_solves, (unsigned long long)info.attached_clauses, (unsigned long long)info.attached_units,
           info.last_cold_reason);
    mi355sat_stats_t stats;
    if (mi355sat_stats(s, &stats) != 0 || stats.n_sat + stats.n_unsat + stats.n_terminated != solves) rc = rc ? rc : 10;
    uint64_t st_size = 0;
    if (mi355sat_abi_sizes(&st_size) != sizeof(mi355sat_opts) || st_size != sizeof(mi355sat_stats_t)) rc = rc ? rc : 11;
    mi355sat_free(s);
    free(offs); free(lits);
    return rc;
}
