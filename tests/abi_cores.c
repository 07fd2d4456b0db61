/*
 * TEST INFRASTRUCTURE: replays, against the C ABI of libmi355sat.so, the calls the Rust shim's `SolveIncremental`
 * impl (rust/mi355sat/src/lib.rs) makes: solve_assumps = assume x n, then solve; core = mi355sat_core sized with
 * out = NULL, then filled (the shim returns the negated literals, rustsat's convention).  The IPASIR state rules are
 * checked on the way:
 *
 *   new -> add (per literal) -> assume x n -> solve -> failed x n, core -> solve (the assumptions are gone) ->
 *   core (MI355SAT_ERR_STATE unless that solve was UNSAT) -> free
 *
 * usage: abi_cores <cnf.bin> <workers> <assumption literals...>
 * cnf.bin: int64 n_vars, int64 n_clauses, uint64 offsets[n_clauses+1], int32 lits[]   (DIMACS literals)
 * Prints "result R", "core N l1 l2 ...", "again R2"; exit 0 when every check passed.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/mi355sat.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
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
    const int n_a = argc - 3;
    int32_t* a = malloc(sizeof(int32_t) * (size_t)n_a);
    for (int i = 0; i < n_a; i++) a[i] = (int32_t)atol(argv[3 + i]);

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
    uint64_t n = 0;
    if (mi355sat_core(s, NULL, 0, &n) != MI355SAT_ERR_STATE) rc = 5;           /* no solve yet */
    for (int i = 0; i < n_a; i++)
        if (mi355sat_assume(s, a[i]) != 0) return 6;
    const int r = mi355sat_solve(s);
    if (r < 0) { fprintf(stderr, "solve failed (%d): %s\n", r, mi355sat_last_error(s)); return 7; }
    printf("result %d\n", r);
    if (r == MI355SAT_UNSAT) {
        if (mi355sat_core(s, NULL, 0, &n) != 0) rc = rc ? rc : 8;
        int32_t* core = malloc(sizeof(int32_t) * (n + 1));
        uint64_t n2 = 0;
        if (n > 0 && mi355sat_core(s, core, n - 1, &n2) != MI355SAT_ERR_ARG) rc = rc ? rc : 9;   /* buffer too small */
        if (mi355sat_core(s, core, n, &n2) != 0 || n2 != n) rc = rc ? rc : 10;
        printf("core %llu", (unsigned long long)n);
        for (uint64_t k = 0; k < n; k++) printf(" %d", core[k]);
        printf("\n");
        /* failed() agrees with core(); every core literal is an assumption */
        for (int i = 0; i < n_a; i++) {
            int in = 0;
            for (uint64_t k = 0; k < n; k++) in |= core[k] == a[i];
            if (mi355sat_failed(s, a[i]) != in) rc = rc ? rc : 11;
        }
        for (uint64_t k = 0; k < n; k++) {
            int in = 0;
            for (int i = 0; i < n_a; i++) in |= core[k] == a[i];
            if (!in) rc = rc ? rc : 12;
        }
        free(core);
    } else if (mi355sat_failed(s, a[0]) != MI355SAT_ERR_STATE) rc = rc ? rc : 13;
    /* the assumptions held for that solve only */
    const int r2 = mi355sat_solve(s);
    printf("again %d\n", r2);
    if (r2 != MI355SAT_UNSAT && mi355sat_core(s, NULL, 0, &n) != MI355SAT_ERR_STATE) rc = rc ? rc : 14;
    mi355sat_stats_t st;
    if (mi355sat_stats(s, &st) != 0 || st.n_sat + st.n_unsat + st.n_terminated != 2) rc = rc ? rc : 15;
    mi355sat_free(s);
    free(offs); free(lits); free(a);
    return rc;
}
