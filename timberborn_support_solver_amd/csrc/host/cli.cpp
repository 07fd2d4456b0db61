// tbs_cli — minimal command-line driver of the solve path (NOT the reference's REPL/UI):
//   tbs_cli rect W H [-l1:K] [--platforms default|1x1] [--workers N] [--sweep | --incremental | --phase-hints] [--gpu N] [--seed N] [--verbose] [--no-simp] [--eliminate] [--certify PATH [--honour-deletions] [--verify]]
//   tbs_cli file PATH.toml [-l1:K] ...
// Mirrors `solve -l<dims>:<n>` of crates/repl/src/main.rs:44-75,248-261: encode once, then solver_loop.
// Ctrl-C calls mi355sat_interrupt (main.rs:297-324).
// --certify PATH: when the loop ends on a bound that is UNSAT, that bound is solved once more with its DRUP proof written to
// PATH, the proof is checked and trimmed on a fresh handle (mi355sat_trim_proof_file) and PATH.lrat is written: a certificate
// that a checker of a few dozen lines verifies against the bound's CNF.  --honour-deletions: the check honours the proof's
// deletion lines (mi355sat_proof_deletions): a worker's stores hold the live lemmas only; the output gains one line.
// --verify: PATH.lrat is then checked on another fresh handle that holds the bound's CNF (mi355sat_check_lrat_file, a kernel
// that shares nothing with the solver's propagation); one more line, `Verified: ...`, and a rejection exits non-zero.
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "solver_loop.hpp"

static std::atomic<mi355sat*> g_current{nullptr};
static std::atomic<int> g_interrupted{0};
// The UNSAT bound once more with a proof, trimmed on a fresh handle.  Returns false if the answer was not UNSAT again.
static bool certify(const tbs::Cnf& cnf, const mi355sat_opts& opts, const std::string& path, bool honour_deletions, bool verify) {
    auto fail = [](mi355sat* s, const char* ctx) {
        const std::string m = std::string(ctx) + ": " + mi355sat_last_error(s);
        mi355sat_free(s);
        throw std::runtime_error(m);
    };
    mi355sat* s = mi355sat_new(&opts);
    if (!s) throw std::runtime_error(std::string("Failed to create solver: ") + mi355sat_last_error(nullptr));
    if (mi355sat_set_proof_path(s, path.c_str()) < 0) fail(s, "set_proof_path");
    if (mi355sat_add_cnf(s, cnf.lits.data(), cnf.offsets.data(), cnf.n_clauses()) < 0) fail(s, "Failed to add CNF");
    mi355sat_reserve(s, cnf.n_vars);
    g_current.store(s);
    const int rc = mi355sat_solve(s);
    g_current.store(nullptr);
    if (rc < 0) fail(s, "solve");
    mi355sat_free(s);
    if (rc != MI355SAT_UNSAT) return false;
    s = mi355sat_new(&opts);
    if (!s) throw std::runtime_error(std::string("Failed to create solver: ") + mi355sat_last_error(nullptr));
    if (mi355sat_add_cnf(s, cnf.lits.data(), cnf.offsets.data(), cnf.n_clauses()) < 0) fail(s, "Failed to add CNF");
    mi355sat_reserve(s, cnf.n_vars);
    mi355sat_trim_info info{};
    if (honour_deletions) mi355sat_proof_deletions(s, 1);
    g_current.store(s);
    const int tr = mi355sat_trim_proof_file(s, path.c_str(), nullptr, 0, 0, MI355SAT_TRIM_HINTS, &info);
    g_current.store(nullptr);
    if (tr < 0) fail(s, "trim_proof");
    if (info.check.valid != 1) {
        std::cout << (info.check.valid < 0 ? "Certificate: interrupted" : "Certificate: the proof was NOT accepted") << std::endl;
        mi355sat_free(s);
        return false;
    }
    const std::string lrat = path + ".lrat";
    if (mi355sat_trim_write_lrat(s, lrat.c_str()) < 0) fail(s, "trim_write_lrat");
    mi355sat_proof_del_info del{};
    if (honour_deletions && mi355sat_debug_proof_deletions(s, &del) == 0)
        std::cout << "Deletions: " << del.honoured << " honoured, " << del.ignored_original + del.ignored_unmatched << " ignored, at most "
                  << del.peak_live_lemmas << " of " << info.check.n_lemmas << " lemmas live" << std::endl;
    mi355sat_free(s);
    std::cout << "Certificate: " << lrat << " - core " << info.core_clauses << " of " << cnf.n_clauses() << " clauses, "
              << info.lemmas_needed << " of " << info.check.n_lemmas << " lemmas needed (checked in " << info.check.seconds
              << " s)" << std::endl;
    if (!verify) return true;
    s = mi355sat_new(&opts);
    if (!s) throw std::runtime_error(std::string("Failed to create solver: ") + mi355sat_last_error(nullptr));
    if (mi355sat_add_cnf(s, cnf.lits.data(), cnf.offsets.data(), cnf.n_clauses()) < 0) fail(s, "Failed to add CNF");
    mi355sat_reserve(s, cnf.n_vars);
    mi355sat_lrat_info li{};
    g_current.store(s);
    const int lr = mi355sat_check_lrat_file(s, lrat.c_str(), nullptr, 0, &li);
    g_current.store(nullptr);
    if (lr < 0) fail(s, "check_lrat");
    mi355sat_free(s);
    if (li.valid != 1) {
        // (`Verified:` begins the line of a success only)
        if (li.accepted < 0) std::cout << "Verification interrupted" << std::endl;
        else if (li.accepted == 1) std::cout << "Verification failed: " << lrat << " does NOT derive the empty clause" << std::endl;
        else std::cout << "Verification failed: " << lrat << " was NOT accepted - line " << li.first_rejected << " (id " << li.first_rejected_id
                       << "), reason " << li.reason << std::endl;
        return false;
    }
    std::cout << "Verified: " << lrat << " - " << li.n_lines << " lines, " << li.n_hints << " hints, " << li.seconds << " s" << std::endl;
    return true;
}

static void on_sigint(int) {
    g_interrupted.store(1);
    mi355sat* s = g_current.load();
    if (s) mi355sat_interrupt(s);
}

int main(int argc, char** argv) {
    using namespace tbs;
    try {
        if (argc < 3) {
            fprintf(stderr, "usage: %s rect W H | file PATH [-l<dims>:<n>]... [--platforms default|1x1] [--workers N] [--sweep | --incremental | --phase-hints] [--gpu N] [--seed N] "
                            "[--verbose] [--no-simp] [--eliminate] [--certify PATH [--honour-deletions] [--verify]]\n", argv[0]);
            return 2;
        }
        WorldGrid grid;
        int a = 1;
        if (!strcmp(argv[a], "rect") && argc >= 4) { grid = WorldGrid::rect(atoi(argv[a + 1]), atoi(argv[a + 2])); a += 3; }
        else if (!strcmp(argv[a], "file")) { grid = WorldGrid::from_toml_file(argv[a + 1]); a += 2; }
        else throw std::runtime_error("expected `rect W H` or `file PATH`");
        std::vector<Dims> defs = platforms_default();
        PlatformLimits limits;
        mi355sat_opts opts{};
        opts.device = -1;
        bool sweep = false, incremental = false, phase_hints = false;
        std::string certify_path;
        bool honour_deletions = false, verify = false;
        for (; a < argc; a++) {
            std::string arg = argv[a];
            if (arg.rfind("-l", 0) == 0) {             // -l<dims>:<n>, dims = AxB or A (=AxA), main.rs:120-142
                std::string kv = arg.substr(2);
                size_t c = kv.find(':');
                if (c == std::string::npos) throw std::runtime_error("missing/invalid delimiter");
                std::string d = kv.substr(0, c);
                size_t x = d.find('x');
                Dims dims = x == std::string::npos ? Dims{atoi(d.c_str()), atoi(d.c_str())}
                                                   : Dims{atoi(d.substr(0, x).c_str()), atoi(d.substr(x + 1).c_str())};
                limits.card_limits[dims] = (size_t)atol(kv.substr(c + 1).c_str());
            } else if (arg == "--platforms" && a + 1 < argc) {
                if (!strcmp(argv[++a], "1x1")) defs = {Dims{1, 1}};
            } else if (arg == "--workers" && a + 1 < argc) opts.workers = atoi(argv[++a]);
            else if (arg == "--gpu" && a + 1 < argc) opts.device = atoi(argv[++a]);          // HIP device ordinal (one process per GPU)
            else if (arg == "--seed" && a + 1 < argc) opts.seed = strtoull(argv[++a], nullptr, 10);   // diversification seed
            else if (arg == "--verbose") opts.verbose = 1;
            else if (arg == "--no-simp") opts.simp = -1;
            else if (arg == "--eliminate") opts.simp = 2;     // + bounded variable elimination before every search
            else if (arg == "--sweep") sweep = true;   // the bounds below the first one as one batch on the device
            else if (arg == "--incremental") incremental = true;   // one warm handle for the whole ladder (mi355sat_set_incremental)
            else if (arg == "--phase-hints") phase_hints = true;   // every rung starts its search at the layout of the rung before (mi355sat_set_phases)
            else if (arg == "--certify" && a + 1 < argc) certify_path = argv[++a];
            else if (arg == "--honour-deletions") honour_deletions = true;
            else if (arg == "--verify") verify = true;
            else throw std::runtime_error("unknown argument " + arg);
        }
        Encoding enc = Encoding::encode(defs, grid);
        signal(SIGINT, on_sigint);
        auto print = [](const std::string& l) { std::cout << l << std::endl; };
        auto hist = incremental ? solver_loop_incremental(grid, enc, limits, &opts, print, [](mi355sat* s) { g_current.store(s); })
                    : sweep ? solver_loop_sweep(grid, enc, limits, &opts, print, [](mi355sat* s) { g_current.store(s); }, &g_interrupted)
                            : solver_loop(grid, enc, limits, &opts, print, [](mi355sat* s) { g_current.store(s); }, (size_t)-1, phase_hints);
        if (!certify_path.empty() && !hist.empty() && hist.back().result == SolverResult::Unsat && !g_interrupted.load()) {
            PlatformLimits bound = limits;
            if (hist.back().k != (size_t)-1) bound.card_limits[Dims{1, 1}] = hist.back().k;
            if (!certify(enc.with_limits(bound).into_cnf(), opts, certify_path, honour_deletions, verify)) return 1;
        }
        return hist.empty() ? 1 : 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}
