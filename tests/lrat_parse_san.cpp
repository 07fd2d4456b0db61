// TEST INFRASTRUCTURE ONLY: the host side of mi355sat_check_lrat - parser, validation, the rewriting of hint ids - driven
// through the C ABI from a program of its own, built with -fsanitize=address,undefined together with the wavefront
// emulator's translation unit (tests/test_emu_lrat.py builds and runs it; CPU only, nothing preloaded).  It feeds the
// malformed inputs of tests/lrat_device_cases.py, hostile hint ids, and one accepted and one rejected file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mi355sat.h"

#define REQUIRE(x)                                                                     \
    do {                                                                               \
        if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } \
    } while (0)

static std::string g_dir;

static int check_words(mi355sat* s, const std::vector<int32_t>& w, mi355sat_lrat_info* info) {
    return mi355sat_check_lrat(s, w.data(), w.size(), nullptr, 0, info);
}

static int check_text(mi355sat* s, const char* text, mi355sat_lrat_info* info) {
    const std::string path = g_dir + "/san.lrat";
    FILE* f = fopen(path.c_str(), "w");
    REQUIRE(f);
    fputs(text, f);
    fclose(f);
    return mi355sat_check_lrat_file(s, path.c_str(), nullptr, 0, info);
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2);
    g_dir = argv[1];
    for (int lds_val = -1; lds_val <= 1; lds_val += 2) {
        mi355sat_opts opts{};
        opts.lds_val = lds_val;
        mi355sat* s = mi355sat_new(&opts);
        REQUIRE(s);
        const int32_t lits[] = {1, 2, -1, 2, 1, -2, -1, -2};
        const uint64_t offs[] = {0, 2, 4, 6, 8};
        REQUIRE(mi355sat_add_cnf(s, lits, offs, 4) == 0);
        mi355sat_lrat_info info{};
        mi355sat_stats_t st{};
        const std::vector<std::vector<int32_t>> bad_words = {
            {5, 2}, {5, 2, 0, 1, 2}, {5, 2, 0}, {5, 2, 0, 1, -2, 0}, {-5, 2, 0, 1, 2, 0}, {5, INT32_MIN, 1, 0, 0}, {INT32_MIN, 1, 0, 0},
            {5, 3, 0, 1, 2, 0}, {5, 2, 0, 1, 2, 0, 6}, {0}, {5}};
        for (const auto& w : bad_words) {
            REQUIRE(check_words(s, w, &info) == MI355SAT_ERR_ARG);
            REQUIRE(strstr(mi355sat_last_error(s), "lrat"));
        }
        const char* bad_text[] = {"5 2 0 1 x 0\n", "5 2 0 1 2 0\n5 d 1 0\n", "5 2 0 1 0 2 0\n", "5 2 0 1 -2 0\n", "5 2 0 1 2\n", "5 2 0 1\n2 0\n",
                                  "5 -3 0 1 2 0\n", "5 99999999999999999999 0 1 0\n", "5 2 0 1 2 0\n6", "d\n", "5 2 0 12345678901234567890 0\n"};
        for (const char* t : bad_text) {
            REQUIRE(check_text(s, t, &info) == MI355SAT_ERR_ARG);
            REQUIRE(strstr(mi355sat_last_error(s), "lrat"));
        }
        REQUIRE(mi355sat_check_lrat_file(s, (g_dir + "/no-such-file").c_str(), nullptr, 0, &info) == MI355SAT_ERR_ARG);
        REQUIRE(mi355sat_stats(s, &st) == 0 && st.kernel_launches == 0);
        uint64_t n = 0;
        REQUIRE(mi355sat_lrat_used(s, nullptr, 0, &n) == MI355SAT_ERR_STATE);
        // the refutation, as words and as text (blank lines and a last line without a newline are fine)
        REQUIRE(check_words(s, {5, 2, 0, 1, 2, 0, 6, 0, 5, 3, 4, 0}, &info) == 0);
        REQUIRE(info.valid == 1 && info.accepted == 1 && info.n_lines == 2 && info.n_hints == 5 && info.used_originals == 4);
        REQUIRE(info.lds == (lds_val > 0 ? 1 : 0));
        REQUIRE(check_text(s, "\n5 2 0 1 2 0\r\n\n  6 0\t5 3 4 0", &info) == 0 && info.valid == 1);
        uint64_t used[4];
        REQUIRE(mi355sat_lrat_used(s, used, 4, &n) == 0 && n == 4 && used[0] == 0 && used[3] == 3);
        REQUIRE(check_text(s, "", &info) == 0 && info.accepted == 1 && info.valid == 0 && info.n_lines == 0 && info.launches == 0);
        // hostile hints: ids far beyond the file, the line's own, a later line's, ids at the edge of 64 bits (text only)
        REQUIRE(check_words(s, {5, 2, 0, 1, 2147483647, 0}, &info) == 0);
        REQUIRE(info.accepted == 0 && info.reason == MI355SAT_LRAT_BAD_HINT && info.first_rejected == 0 && info.reject_hint == 1);
        REQUIRE(check_words(s, {5, 2, 0, 5, 0}, &info) == 0 && info.reason == MI355SAT_LRAT_BAD_HINT && info.reject_hint == 0);
        REQUIRE(check_words(s, {5, 2, 0, 1, 6, 0, 6, 0, 5, 3, 4, 0}, &info) == 0 && info.reason == MI355SAT_LRAT_BAD_HINT);
        REQUIRE(check_text(s, "5 2 0 1 4611686018427387904 0\n", &info) == 0 && info.reason == MI355SAT_LRAT_BAD_HINT);
        REQUIRE(check_text(s, "4611686018427387904 2 0 1 2 0\n", &info) == 0 && info.accepted == 1 && info.first_rejected == UINT64_MAX);
        REQUIRE(check_words(s, {6, 2, 0, 1, 2, 0, 5, 0, 6, 3, 4, 0}, &info) == 0);
        REQUIRE(info.accepted == 0 && info.reason == MI355SAT_LRAT_ID_ORDER && info.first_rejected == 1 && info.first_rejected_id == 5);
        mi355sat_free(s);
    }
    mi355sat_release_cached_memory();
    puts("lrat_parse_san OK");
    return 0;
}
