/*
 * TEST INFRASTRUCTURE: replays, against the C ABI of libmi355sat.so, the calls the Rust shim's `minimize_core`
 * (rust/mi355sat/src/lib.rs) makes after a `solve_assumps` that came back UNSAT:
 *
 *   new -> add (per literal) -> minimize_core (MI355SAT_ERR_STATE: no solve yet) -> assume x n -> solve (20) -> core ->
 *   minimize_core -> core (a subsequence of the one before) -> failed x n (agrees with the new core) ->
 *   minimize_core (the flag is kept: no candidates) -> solve (the assumptions are gone: 10) ->
 *   minimize_core (MI355SAT_ERR_STATE) -> free
 *
 * usage: abi_core_minimize <cnf.bin> <workers> <max candidates per round, 0 = default> <assumption literals...>
 * cnf.bin: int64 n_vars, int64 n_clauses, uint64 offsets[n_clauses+1], int32 lits[]   (DIMACS literals)
 * Prints "result R", "core N l1 ...", "min N l1 ...", "info minimal rounds candidates unsat sat by_model launches",
 * "again R2"; exit 0 when every check passed.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/mi355sat.h"

static uint64_t read_core(mi355sat* s, int32_t** out, int* rc, int code) {
    uint64_t n = 0, n2 = 0;
    if (mi355sat_core(s, NULL, 0, &n) != 0) *rc = *rc ? *rc : code;
    *out = malloc(sizeof(int32_t) * (n + 1));
    if (mi355sat_core(s, *out, n, &n2) != 0 || n2 != n) *rc = *rc ? *rc : code;
    return n;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[2];
    if (fread(h, 8, 2, f) != 2) return 2;
    const int64_t nc = h[1];
    uint64_t* offs = malloc(8 * (size_t)(nc + 1));
    if (fread(offs, 8, (size_t)nc + 1, f) != (size_t)nc + 1) return 2;
    int32_t* lits = malloc(4 * (size_t)offs[nc] + 4);
    if (fread(lits, 4, offs[nc], f) != offs[nc]) return 2;
    fclose(f);
    const int n_a = argc - 4;
    int32_t* a = malloc(sizeof(int32_t) * (size_t)n_a);
    for (int i = 0; i < n_a; i++) a[i] = (int32_t)atol(argv[4 + i]);

    mi355sat_opts o;
    memset(&o, 0, sizeof o);
    o.device = -1;
    o.workers = atoi(argv[2]);
    o.simp = -1;
    mi355sat* s = mi355sat_new(&o);
    if (!s) { fprintf(stderr, "mi355sat_new: %s\n", mi355sat_last_error(NULL)); return 3; }
    for (int64_t c = 0; c < nc; c++) {
        for (uint64_t k = offs[c]; k < offs[c + 1]; k++)
            if (mi355sat_add(s, lits[k]) < 0) return 4;
        if (mi355sat_add(s, 0) < 0) return 4;
    }
    int rc = 0;
    mi355sat_core_min_info info;
    if (mi355sat_debug_core_min_round(s, (uint32_t)atoi(argv[3])) != 0) rc = 5;
    if (mi355sat_minimize_core(s, 0, &info) != MI355SAT_ERR_STATE) rc = rc ? rc : 5;      /* no solve yet */
    if (mi355sat_minimize_core(s, -1, NULL) != MI355SAT_ERR_ARG) rc = rc ? rc : 5;
    for (int i = 0; i < n_a; i++)
        if (mi355sat_assume(s, a[i]) != 0) return 6;
    const int r = mi355sat_solve(s);
    if (r < 0) { fprintf(stderr, "solve failed (%d): %s\n", r, mi355sat_last_error(s)); return 7; }
    printf("result %d\n", r);
    if (r != MI355SAT_UNSAT) return 8;
    mi355sat_stats_t st0, st1;
    if (mi355sat_stats(s, &st0) != 0) rc = rc ? rc : 9;
    int32_t *before, *core;
    const uint64_t nb = read_core(s, &before, &rc, 9);
    printf("core %llu", (unsigned long long)nb);
    for (uint64_t k = 0; k < nb; k++) printf(" %d", before[k]);
    printf("\n");
    const int m = mi355sat_minimize_core(s, 0, &info);
    if (m != 0) { fprintf(stderr, "minimize_core failed (%d): %s\n", m, mi355sat_last_error(s)); return 10; }
    const uint64_t n = read_core(s, &core, &rc, 11);
    printf("min %llu", (unsigned long long)n);
    for (uint64_t k = 0; k < n; k++) printf(" %d", core[k]);
    printf("\n");
    printf("info %d %u %llu %llu %llu %llu %llu\n", info.minimal, info.rounds, (unsigned long long)info.candidates,
           (unsigned long long)info.candidates_unsat, (unsigned long long)info.candidates_sat,
           (unsigned long long)info.critical_by_model, (unsigned long long)info.model_launches);
    if (info.minimal != 1 || info.size_before != nb || info.size_after != n || n > nb) rc = rc ? rc : 12;
    if (info.candidates < info.candidates_sat + info.candidates_unsat) rc = rc ? rc : 12;   /* (a round ends at its first UNSAT) */
    /* the new core is a subsequence of the old one */
    uint64_t j = 0;
    for (uint64_t k = 0; k < n; k++) {
        while (j < nb && before[j] != core[k]) j++;
        if (j++ >= nb) rc = rc ? rc : 13;
    }
    /* failed() agrees with the new core */
    for (int i = 0; i < n_a; i++) {
        int in = 0;
        for (uint64_t k = 0; k < n; k++) in |= core[k] == a[i];
        if (mi355sat_failed(s, a[i]) != in) rc = rc ? rc : 14;
    }
    /* candidates are no results of the caller's */
    if (mi355sat_stats(s, &st1) != 0 || st1.n_sat != st0.n_sat || st1.n_unsat != st0.n_unsat || st1.n_terminated != st0.n_terminated)
        rc = rc ? rc : 15;
    /* an irreducible core is not minimised again */
    if (mi355sat_minimize_core(s, 0, &info) != 0 || info.minimal != 1 || info.candidates != 0 || info.size_after != n) rc = rc ? rc : 16;
    free(before);
    free(core);
    /* the assumptions held for that solve only */
    const int r2 = mi355sat_solve(s);
    printf("again %d\n", r2);
    if (r2 != MI355SAT_UNSAT && mi355sat_minimize_core(s, 0, NULL) != MI355SAT_ERR_STATE) rc = rc ? rc : 17;
    if (mi355sat_stats(s, &st1) != 0 || st1.n_sat + st1.n_unsat + st1.n_terminated != 2) rc = rc ? rc : 18;
    mi355sat_free(s);
    free(offs); free(lits); free(a);
    return rc;
}
