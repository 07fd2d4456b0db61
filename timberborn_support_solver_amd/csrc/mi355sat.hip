// mi355sat.hip — libmi355sat.so: the C ABI of include/mi355sat.h over the HIP
// kernels in device/kernels.hip.h.  Host duties only: clause intake and
// normalisation, building the immutable clause database and the per-worker slab
// template, replicating it into HBM, launching slices of the search kernel, and
// reading verdicts / models / counters back.  There is no CPU solving path: if
// HIP is unavailable every entry point fails.
//
// Reference call sites this file serves (see include/mi355sat.h for the mapping):
//   crates/repl/src/solver_runner.rs:12-16, crates/repl/src/main.rs:295,316,329,363,
//   crates/gui/src/solver_backend.rs:78-90.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <queue>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/mi355sat.h"
#include "device/kernels.hip.h"

namespace {

std::string g_new_error;
std::mutex g_new_error_mu;

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct HipErr { std::string msg; int code = MI355SAT_ERR_HIP; };
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            throw HipErr{std::string(#x) + ": " + hipGetErrorString(e_)};                            \
    } while (0)

// ---- auxiliary kernels ---------------------------------------------------------
// Per-worker customisation after the template slab has been replicated:
// assumptions, scripted decisions and a worker-specific initial decision order
// (affine permutation of the variables; worker group 0 keeps the canonical order).
__global__ void ms_customize_kernel(MsLayout L, char* slabs, uint32_t n_workers, const int32_t* assump_data,
                                    const uint64_t* assump_off, const int32_t* script_data,
                                    const uint64_t* script_off, uint32_t n_instances, uint64_t seed, int32_t park_from,
                                    uint32_t wid0, int32_t phase_mix) {
    const uint32_t wid = blockIdx.x + wid0;   // workers [wid0, n_workers)
    if (wid >= n_workers) return;
    char* slab = slabs + (size_t)wid * L.slab_bytes;
    MsState* st = (MsState*)(slab + L.state);
    const uint32_t inst = n_instances ? wid % n_instances : 0;
    const uint32_t replica = n_instances ? wid / n_instances : wid;
    if (assump_off) {
        uint64_t a0 = assump_off[inst], a1 = assump_off[inst + 1];
        int32_t* dst = (int32_t*)(slab + L.assumps);
        for (uint64_t i = threadIdx.x; i < a1 - a0; i += blockDim.x) dst[i] = assump_data[a0 + i];
        if (threadIdx.x == 0) st->n_assumps = (int32_t)(a1 - a0);
    }
    if (script_off) {
        uint64_t a0 = script_off[inst], a1 = script_off[inst + 1];
        int32_t* dst = (int32_t*)(slab + L.script);
        for (uint64_t i = threadIdx.x; i < a1 - a0; i += blockDim.x) dst[i] = script_data[a0 + i];
        if (threadIdx.x == 0) st->n_script = (int32_t)(a1 - a0);
    }
    if (threadIdx.x == 0) {
        st->rng = seed * 0x9E3779B97F4A7C15ull + wid;
        if (park_from >= 0 && (int32_t)wid >= park_from) st->status = MS_ST_PARKED;  // idle until it steals a cube
    }
    if (replica > 0 && L.n_vars > 2) {
        // splitmix64 -> multiplier coprime to n_vars, offset
        uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(replica + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const uint32_t n = L.n_vars;
        uint32_t a = (uint32_t)(z % n) | 1u, b = (uint32_t)((z >> 32) % n);
        for (;;) {
            uint32_t x = a, y = n;
            while (y) { uint32_t t = x % y; x = y; y = t; }
            if (x == 1) break;
            a += 2;
            if (a >= n) a = 1;
        }
        int32_t* order = (int32_t*)(slab + L.vm_order);
        MsVarRec* vrec = (MsVarRec*)(slab + L.vrec);
        // initial saved phases (phase_mix): replica % 4 == 1 decides every variable TRUE first, == 2 at random;
        // the others keep FALSE (the template)
        const uint32_t pm = phase_mix > 0 ? replica & 3u : 0u;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            uint32_t v = (uint32_t)(((uint64_t)a * i + b) % n);
            order[i] = (int32_t)v;
            ((int32_t*)(slab + L.vm_pos))[v] = (int32_t)i;
            if (pm == 1) vrec[v].phase = 0;
            else if (pm == 2) vrec[v].phase = (uint8_t)((((uint64_t)v * 0x9E3779B97F4A7C15ull + z) >> 40) & 1);
        }
    }
}

// Replicates the template slab (its head and the initially used part of the watch pool) into
// every worker slab with 16-byte copies: one launch instead of two memcpys per worker.
__global__ void ms_replicate_kernel(const char* tmpl, char* slabs, uint64_t slab_bytes, uint64_t head_bytes,
                                    uint64_t pool_off, uint64_t pool_bytes) {
    char* dst = slabs + (size_t)blockIdx.y * slab_bytes;
    const uint64_t n_head = head_bytes / 16, n_pool = (pool_bytes + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_head + n_pool; i += stride) {
        const uint64_t off = i < n_head ? i * 16 : pool_off + (i - n_head) * 16;
        *(uint4*)(dst + off) = *(const uint4*)(tmpl + off);
    }
}

// Phase hints (mi355sat_phase / mi355sat_set_phases): seeds the saved phase of every hinted, still unassigned variable of
// workers [wid0, n_workers).  hints[v]: 0 none, 1 TRUE first, 2 FALSE first, one byte per device variable.  One variable
// per thread, grid = (ceil(n_vars / 256), workers): a coalesced read of the hint bytes; only a hinted variable touches the
// worker's slab (its assignment byte, then one byte store).  An assigned variable's phase byte is its polarity now
// (layout.h, MsVarRec) and is left alone.  Runs between slices only, when the slab is the whole truth in every build of
// the search kernel.
__global__ __launch_bounds__(256) void ms_phase_kernel(MsLayout L, char* slabs, uint32_t wid0, uint32_t n_workers,
                                                       const uint8_t* hints) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t wid = wid0 + blockIdx.y;
    if (v >= L.n_vars || wid >= n_workers) return;
    const uint8_t h = ((Gp<const uint8_t>)hints)[v];
    if (!h) return;
    Gp<char> slab = (Gp<char>)(slabs + (size_t)wid * L.slab_bytes);
    if (((Gp<const uint8_t>)(slab + L.val))[v] != MS_ASG_UNDEF) return;
    ((Gp<MsVarRec>)(slab + L.vrec))[v].phase = (uint8_t)(h - 1);   // device literal 2*v + phase: phase 1 = the negative one
}

// Applies the scheduler's decisions between two slices: update u = (worker, status, restart_req,
// n_assumps, data offset); the worker's assumption list (its cube) is rewritten from data[].
__global__ void ms_assign_kernel(MsLayout L, char* slabs, uint32_t n_upd, const int32_t* upd, const int32_t* data) {
    const uint32_t u = blockIdx.x;
    if (u >= n_upd) return;
    const int32_t worker = upd[5 * u], status = upd[5 * u + 1], restart = upd[5 * u + 2], n = upd[5 * u + 3],
                  off = upd[5 * u + 4];
    char* slab = slabs + (size_t)worker * L.slab_bytes;
    MsState* st = (MsState*)(slab + L.state);
    int32_t* dst = (int32_t*)(slab + L.assumps);
    for (int32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = data[off + i];
    if (threadIdx.x == 0) {
        st->n_assumps = n;
        st->status = status;
        if (restart) st->restart_req = 1;
        st->n_split = 0;
    }
}

__global__ void ms_gather_states_kernel(MsLayout L, const char* slabs, uint32_t n_workers, MsState* out) {
    const uint32_t wid = blockIdx.x * blockDim.x + threadIdx.x;
    if (wid >= n_workers) return;
    out[wid] = *(const MsState*)(slabs + (size_t)wid * L.slab_bytes + L.state);
}

// Between two slices: move the clauses the workers exported during the last slice into the global
// ring, once each (a 64-bit order-independent signature in a hash set filters what many workers
// learnt alike).  One thread per worker; nothing else runs on the stream meanwhile.
__device__ inline unsigned long long share_mix(unsigned long long x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
__global__ void ms_share_collect_kernel(MsLayout L, char* slabs, uint32_t n_workers, int32_t* pool, uint32_t slots,
                                        unsigned long long* share_n, unsigned long long* hash, uint32_t hash_mask,
                                        uint32_t* intake, uint32_t intake_cap, int ordered) {
    // ordered (opts.deterministic): ONE thread takes the workers in index order, so ring order, the hash set's races and the
    // intake cut-off do not depend on timing
    uint32_t wid = blockIdx.x * blockDim.x + threadIdx.x;
    if (ordered) {
        if (wid != 0) return;
    } else if (wid >= n_workers) return;
  for (; wid < n_workers; wid++) {
    char* slab = slabs + (size_t)wid * L.slab_bytes;
    MsState* st = (MsState*)(slab + L.state);
    const uint32_t n = st->exp_n;
    if (!n) { if (ordered) continue; return; }
    const int32_t* exp = (const int32_t*)(slab + L.exp);
    for (uint32_t r = 0; r < n && r < MS_EXPORT_RECS; r++) {
        const int32_t* rec = exp + r * MS_SHARE_REC;
        const int sz = rec[0] & 63;
        if (sz < 1 || sz > MS_SHARE_MAXLEN) continue;
        unsigned long long h = (unsigned long long)sz * 0xd6e8feb86659fd93ull;
        for (int j = 0; j < sz; j++) h += share_mix((unsigned long long)(uint32_t)rec[1 + j]);
        if (!h) h = 1;
        bool fresh = true;
        uint32_t i = (uint32_t)(h >> 20) & hash_mask;
        for (int probe = 0; probe < 16; probe++) {
            unsigned long long prev = atomicCAS(&hash[i], 0ull, h);
            if (prev == 0ull) break;
            if (prev == h) { fresh = false; break; }
            i = (i + 1) & hash_mask;
        }
        if (!fresh) continue;
        // every worker attaches every record: units and binaries always pass, of the longer clauses only
        // intake_cap per collection (first come), so that attaching stays a small part of a slice
        if (sz > 2 && atomicAdd(intake, 1u) >= intake_cap) continue;
        const unsigned long long slot = atomicAdd(share_n, 1ull) % slots;
        int32_t* dst = pool + slot * MS_SHARE_REC;
        for (int j = 0; j <= sz; j++) dst[j] = rec[j];
    }
    st->exp_n = 0;
    if (!ordered) return;
  }
}

// Subsumption and self-subsuming resolution (the other half of what `simp::Glucose` does before search; its
// variable elimination is not restated: measured to remove < 15 % of these encodings' variables).  One thread per
// clause C (literals sorted): every clause D in the occurrence list of C's rarest literal p is merged against C -
// C inside D: D is subsumed;  C inside D except ONE literal x that D has negated: D loses ~x (the resolvent of C and
// D on x subsumes D).  The list of ~p finds the D's that lose ~p.  sig = 64-bit signature over VARIABLES
// (sig(C) & ~sig(D) != 0 rules D out without touching its literals).
__device__ inline int subsume_check(const int32_t* lits, const uint64_t* offs, uint32_t c, uint32_t d) {
    // 0 no, 1 C subsumes D, 2 + x: D can drop literal ~x  (returned as 2 + (~x))
    uint64_t i = offs[c], ie = offs[c + 1], j = offs[d], je = offs[d + 1];
    int flip = -1;
    for (; i < ie; i++) {
        const int32_t a = lits[i];
        while (j < je && (lits[j] >> 1) < (a >> 1)) j++;
        if (j == je || (lits[j] >> 1) != (a >> 1)) return 0;
        if (lits[j] != a) {
            if (flip >= 0) return 0;
            flip = lits[j];
        }
        j++;
    }
    return flip < 0 ? 1 : 2 + flip;
}
__global__ void ms_subsume_kernel(uint32_t n_clauses, const int32_t* lits, const uint64_t* offs, const unsigned long long* sig,
                                  const uint32_t* occ_off, const uint32_t* occ, uint32_t max_size, uint32_t* subsumed,
                                  int32_t* drop_lit) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clauses) return;
    const uint32_t sz = (uint32_t)(offs[c + 1] - offs[c]);
    if (sz > max_size) return;
    int32_t p = lits[offs[c]];
    uint32_t best = 0xffffffffu;
    for (uint64_t k = offs[c]; k < offs[c + 1]; k++) {
        const int32_t l = lits[k];
        const uint32_t n = (occ_off[l + 1] - occ_off[l]) + (occ_off[(l ^ 1) + 1] - occ_off[l ^ 1]);
        if (n < best) { best = n; p = l; }
    }
    const unsigned long long sc = sig[c];
    for (int side = 0; side < 2; side++) {
        const int32_t q = side ? (p ^ 1) : p;
        for (uint32_t e = occ_off[q]; e < occ_off[q + 1]; e++) {
            const uint32_t d = occ[e];
            if (d == c || (sc & ~sig[d]) != 0) continue;
            const uint32_t dz = (uint32_t)(offs[d + 1] - offs[d]);
            if (dz < sz) continue;
            const int r = subsume_check(lits, offs, c, d);
            if (r == 1) { if (dz > sz || c < d) subsumed[d] = 1; }          // equal clauses: the lower index stays
            else if (r >= 2) atomicMax((int*)&drop_lit[d], r - 2);          // one literal per clause and pass (the largest: the choice does not depend on timing)
        }
    }
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
    }
    void upload(const std::vector<T>& v, hipStream_t s) {
        alloc(v.size());
        if (!v.empty()) HIPCHK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void upload_nonempty(const std::vector<T>& v, hipStream_t s) {   // an empty list as one zero element: the buffer has an address
        upload(v.empty() ? std::vector<T>(1) : v, s);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The worker slabs are by far the largest allocation (4096 x 37 MiB = 147 GiB at rect 64x64) and hipMalloc
// of that size takes 2-5 s on MI355X (measured; 33 GB/s) - more than most solves of the refinement loop, which
// makes a FRESH solver per bound (main.rs:295).  So a freed handle parks its slab buffer here, one per device,
// and the next handle of the process takes it over if it is large enough.  mi355sat_release_cached_memory()
// returns it to the driver.
struct SlabCache {
    std::mutex mu;
    char* p[64] = {nullptr};
    size_t bytes[64] = {0};
};
SlabCache g_slab_cache;

struct SlabBuf {
    char* p = nullptr;
    size_t n = 0;        // bytes in use
    size_t cap = 0;      // bytes allocated
    int dev = 0;
    static size_t cached_bytes(int dev) {
        std::lock_guard<std::mutex> g(g_slab_cache.mu);
        return dev >= 0 && dev < 64 ? g_slab_cache.bytes[dev] : 0;
    }
    void alloc(size_t bytes, int device) {
        release();
        dev = device;
        if (!bytes) return;
        {
            std::lock_guard<std::mutex> g(g_slab_cache.mu);
            if (dev >= 0 && dev < 64 && g_slab_cache.p[dev]) {
                if (g_slab_cache.bytes[dev] >= bytes) { p = g_slab_cache.p[dev]; cap = g_slab_cache.bytes[dev]; }
                else (void)hipFree(g_slab_cache.p[dev]);     // too small: make room before the larger request
                g_slab_cache.p[dev] = nullptr;
                g_slab_cache.bytes[dev] = 0;
            }
        }
        if (!p) { HIPCHK(hipMalloc((void**)&p, bytes)); cap = bytes; }
        n = bytes;
    }
    void release() {
        if (p) {
            std::lock_guard<std::mutex> g(g_slab_cache.mu);
            if (dev >= 0 && dev < 64 && g_slab_cache.bytes[dev] < cap) {
                if (g_slab_cache.p[dev]) (void)hipFree(g_slab_cache.p[dev]);
                g_slab_cache.p[dev] = p;
                g_slab_cache.bytes[dev] = cap;
            } else (void)hipFree(p);
        }
        p = nullptr;
        n = cap = 0;
    }
    ~SlabBuf() { release(); }
};

}  // namespace

// One eliminated variable: literal x of it and the clauses (elim_lits[begin, end), -1 terminated, x included) that held x.
struct MsElim { int32_t x; uint32_t begin, end; };

// A failed-assumption core: caller's literals, in the order of the caller's assumption list.  valid: the answer it belongs
// to was UNSAT and still stands; minimal: mi355sat_minimize_core proved it irreducible (it is not minimised again).
struct Core {
    std::vector<int32_t> lits;
    bool valid = false, minimal = false;
};

struct mi355sat {
    mi355sat_opts opts{};
    int device = 0;
    // clause intake (DIMACS literals)
    std::vector<int32_t> lits;
    std::vector<uint64_t> offs{0};
    std::vector<int32_t> pending;
    uint64_t max_var = 0;
    // results
    std::vector<int8_t> model;                 // plain solve
    std::vector<std::vector<int8_t>> batch_models;
    mi355sat_stats_t stats{};
    std::string err;
    std::string proof_path;
    // interrupt flag: pinned host memory the kernels poll
    int32_t* stop_flag = nullptr;
    std::atomic<int> interrupted{0};
    // device
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<int32_t> d_cl_lits, d_bin_lits, d_tern_owner;
    DevBuf<ms_int2> d_tern_pairs;
    bool lds_val = false;                      // assignment staged in LDS (2 bits/var)
    uint32_t lds_val_bytes = 0;
    mi355sat_search_build last_build{};        // build of the last search launch (mi355sat_debug_last_search_build)
    DevBuf<char> d_template;
    SlabBuf d_slabs;
    DevBuf<MsState> d_states;
    DevBuf<int32_t> d_any_done, d_assump, d_script, d_proof;
    DevBuf<uint32_t> d_proof_len;
    uint32_t proof_cap = 0;                    // words per worker in d_proof
    FILE* proof_file = nullptr;                // open while a solve, a batch or a sweep logs its DRUP proof
    bool proof_empty = false;                  // the open file holds the empty clause already (written at most once)
    // proof_drain: the non-empty logs as jobs, the packed words (ms_proof_gather_kernel) - both grow when needed and stay -
    // and inverse_order(perm) of the cold start that allocated the logs
    DevBuf<uint32_t> d_proof_jobs, d_proof_inv;
    DevBuf<int32_t> d_proof_out;
    mi355sat_proof_log_info proof_log{};       // test hook (mi355sat_debug_proof_log): the drains since the file was opened
    DevBuf<uint64_t> d_assump_off, d_script_off;
    // learnt-clause exchange between workers (layout.h MS_SHARE_*)
    DevBuf<int32_t> d_share_pool;
    DevBuf<unsigned long long> d_share_n, d_share_hash;
    DevBuf<uint32_t> d_share_intake;
    uint32_t share_slots = 0, share_hash_n = 0;
    uint64_t share_slices = 0;
    uint64_t share_export_pos = 0;             // ring records below this were handed out by mi355sat_share_export already
    MsShared sh{};
    MsLayout L{};
    uint32_t n_workers = 0;
    uint32_t n_alloc = 0;                      // workers [0, n_alloc) have their slab (the rest is allocated on demand)
    uint64_t pool_init = 0;                    // watch-pool entries in use in the template
    // prepared formula facts
    bool trivially_unsat = false;
    std::vector<int8_t> fixed;                 // per var: 0 free, 1 true, -1 false (level-0 facts)
    uint32_t n_vars = 0;
    std::vector<uint32_t> perm;                // caller's variable index -> device variable index (Prepared::perm)
    std::vector<int32_t> subst;                // per caller variable: the literal (2*var + neg) that replaced it, or itself
    std::vector<int32_t> simp_proof;           // DRUP lemmas of the simplification (internal literals, -1 terminated)
    std::vector<MsElim> elims;                 // variables eliminated before search and the clauses that rebuild their values
    std::vector<int32_t> elim_lits;
    struct SweepHolder* sweep = nullptr;        // stepwise sweep in progress (mi355sat_sweep_*)
    // IPASIR assumptions (mi355sat_assume) of the next solve(), and the failed-assumption cores
    std::vector<int32_t> assumps;
    Core core;                                 // of the last solve(), valid after UNSAT until the next add / assume / solve
    std::vector<Core> batch_cores;             // of the last solve_batch(), per instance
    // core minimisation (mi355sat_minimize_core): the formula is known to be satisfiable while no clause was added since
    // a SAT answer; test hook (mi355sat_debug_core_min_round): at most this many candidates per round, 0 = the default
    uint64_t sat_clauses = UINT64_MAX;         // stats.n_clauses when a solve / batch last answered SAT
    uint32_t core_min_round = 0;
    uint32_t proof_chunk = 0;                  // test hook (mi355sat_debug_proof_check_chunk): lemmas per worker and launch of a proof check
    uint32_t trim_log_words = 0;               // test hook (mi355sat_debug_trim_log): words per worker of a traced check's dependency log
    bool proof_del = false;                    // mi355sat_proof_deletions: checks and trims honour the proof's deletion lines
    bool proof_del_have = false;               // proof_del_info describes a check or trim made with the switch on
    mi355sat_proof_del_info proof_del_info{};
    // What the last mi355sat_trim_proof found a valid proof to rest on; dropped by the next trim_proof / check_proof, a clause
    // added, a sweep begun.  Indices: caller clauses 0-based in the order they were added, lemmas 0-based, both ascending.
    struct Trim {
        bool valid = false, hints = false;
        bool no_lines = false;                 // a tautological target: nothing to derive
        uint64_t n_clauses = 0, n_lemmas = 0;
        std::vector<uint64_t> core, lemmas;
        std::vector<int32_t> lits;             // DIMACS literals of the needed lemmas in order, then the target's
        std::vector<uint64_t> offs{0};
        std::vector<std::vector<uint64_t>> hint;   // (hints) per needed lemma, then the target: LRAT ids in the order a checker propagates them
        void drop() { *this = Trim(); }
    } trim;
    // warm incremental solve (mi355sat_set_incremental): what the last mi355sat_solve() left on the device, and what was
    // attached to it since
    struct Incremental {
        bool on = false;
        bool resident = false;                 // the slabs hold the workers of the last solve(); they know clauses [0, n_clauses)
        bool refuted = false;                  // the formula is UNSAT whatever the assumptions (it only grows)
        int why_not = MI355SAT_COLD_FIRST;     // why nothing is resident
        size_t n_clauses = 0;                  // clauses of lits / offs above that the resident workers hold: uploaded or attached
        std::vector<uint8_t> eliminated;       // per caller variable: resolved away before the upload (opts.simp = 2)
        std::vector<int32_t> lits;             // every clause attached since the upload, device literals: workers created
        std::vector<uint32_t> offs{0};         // later (ramp-up, grow_workers) start from the template and get all of them
        uint64_t pinned = 0, pinned_lits = 0;  // those of two and more literals, and the room they take in a worker's lc_lits
        std::vector<MsState> base;             // the workers' counters when the last solve ended (they run on)
        mi355sat_incremental_info info{};
    } inc;
    // What the last mi355sat_check_lrat found every line of a file to rest on (mi355sat_lrat_used): caller clause indices,
    // ascending; valid after a call with accepted == 1 until the next one or a clause added.  Test hook
    // (mi355sat_debug_lrat_chunk): lines per launch, 0 = the rule.
    struct Lrat {
        bool valid = false;
        std::vector<uint64_t> used;
    } lrat;
    uint32_t lrat_chunk = 0;
    DevBuf<int32_t> d_inc_lits;
    DevBuf<uint32_t> d_inc_offs;
    // phase hints (mi355sat_phase / mi355sat_set_phases): kept on the handle in the caller's variables; every cold start maps
    // them to the device's (map_phases) and seeds every worker's saved phases with them (ms_phase_kernel)
    struct Phases {
        std::vector<int8_t> hint;              // per caller variable (index v - 1): 0 none, 1 TRUE first, -1 FALSE first
        uint64_t version = 0;                  // bumped whenever a hint changes ...
        uint64_t applied = 0;                  // ... and the one the workers on the device were last seeded with
        std::vector<uint8_t> dev_fixed;        // per device variable: assigned at level 0 by the last cold start's upload
        bool on_device = false;                // d_phase holds the current hints in the current mapping (mapped > 0 of them)
        mi355sat_phase_info info{};
    } ph;
    DevBuf<uint8_t> d_phase;
    // test hooks: the optional heuristics' counters over the workers of the last solve; their schedule (0 = the defaults)
    mi355sat_heuristics_info heur{};
    uint32_t first_vivify = 0, vivify_every = 0, rephase_every = 0;
    // test hook (mi355sat_debug_set_capacities): the store sizes of the next cold start of a search (0 = the rule), the
    // layout the last one got (mi355sat_debug_capacities), and the workers' three store-pressure counters of the last search
    uint32_t want_learnt_cap = 0, want_learnt_lit_cap = 0, want_pool_slack = 0, want_proof_cap = 0;
    mi355sat_capacity_info cap_info{};
    bool cap_info_valid = false;
    uint64_t cap_events[3] = {0, 0, 0};
    // test hook (mi355sat_debug_keep_simplified): what simplify_formula left at the last cold start, as 0-terminated clauses
    // of DIMACS literals in the caller's variables; [0] the formula the workers get, [1] the kept sides of the eliminations
    bool keep_simplified = false, kept_valid = false;
    std::vector<int32_t> kept[2];
    uint64_t kept_n[2] = {0, 0};
};

namespace {

// What the kernels other than the search kernel (BCP, probing) do with the assignment, and the search kernel when
// opts.lds_val is not on auto: staged in LDS if forced, or on auto when it fits the round-1 budget of 16 workers per CU.
inline bool staged_in_lds(int opt_lds_val, uint32_t lds_val_bytes) {
    if (lds_val_bytes > 150 * 1024) return false;
    return opt_lds_val == 1 || (opt_lds_val == 0 && lds_val_bytes <= 10 * 1024);
}

// ---- formula preparation ---------------------------------------------------------
struct Prepared {
    uint32_t n_vars = 0;
    bool unsat = false;
    std::vector<int32_t> units;                 // internal literals fixed at level 0 (trail prefix)
    std::vector<uint32_t> perm;                 // caller's variable index (0-based) -> device variable index
    bool units_propagated = false;              // true if simplification ran (queue starts empty)
    std::vector<MsClauseHdr> cl_hdr;            // long clauses (>= 4 literals)
    std::vector<int32_t> cl_lits;               // each clause 16-byte aligned, padded with its first literal
    std::vector<MsLitHdr> lit_hdr;              // 2*n_vars
    std::vector<int32_t> bin_lits;
    std::vector<ms_int2> tern_pairs;
    std::vector<int32_t> tern_owner;
};

inline uint64_t var_of(int32_t d) { return (uint64_t)(d < 0 ? -(int64_t)d : d); }      // |d|: a DIMACS literal's variable
inline int32_t to_internal(int32_t d) { return d > 0 ? 2 * (d - 1) : 2 * (-d - 1) + 1; }
inline int32_t to_dimacs(int32_t l) { return (l & 1) ? -((l >> 1) + 1) : ((l >> 1) + 1); }      // and back
inline int32_t to_device(const std::vector<uint32_t>& perm, int32_t d) {   // DIMACS literal -> device literal
    return d > 0 ? 2 * (int32_t)perm[d - 1] : 2 * (int32_t)perm[-d - 1] + 1;
}
inline std::vector<uint32_t> inverse_order(const std::vector<uint32_t>& perm) {   // device variable -> caller's (0-based)
    std::vector<uint32_t> inv(perm.size());
    for (uint32_t e = 0; e < perm.size(); e++) inv[perm[e]] = e;
    return inv;
}
// A device literal as the caller's DIMACS literal, through the inverse of the device's variable order (inverse_order(perm)).
inline int32_t to_dimacs(const std::vector<uint32_t>& inv, int32_t l) { return to_dimacs(2 * (int32_t)inv[l >> 1] | (l & 1)); }
// The same for a formula that went through the simplification - the one route of assumptions, clauses attached warm, phase
// hints and imported records: the equivalent-literal substitution (which may flip the sign), then the device's variable
// order (perm: s.perm once uploaded).  The caller has checked the range.  gone (may be null), per caller variable: resolved
// away before the upload - such a representative has no device variable, and the answer is -1.
inline int32_t device_literal(const mi355sat& s, const std::vector<uint32_t>& perm, int32_t d, const std::vector<uint8_t>* gone = nullptr) {
    int32_t l = to_internal(d);
    while ((size_t)(l >> 1) < s.subst.size() && s.subst[l >> 1] != 2 * (l >> 1)) l = s.subst[l >> 1] ^ (l & 1);
    if (gone && (*gone)[l >> 1]) return -1;
    return 2 * (int32_t)perm[l >> 1] | (l & 1);
}

// (warm incremental solve) What is on the device is no solve()'s to go on with: the next one starts cold, for this reason.
// Whatever rewrites the slabs or changes what a worker's state depends on comes through here - a missed call is a wrong
// warm start.
inline void go_cold(mi355sat& s, int why) {
    s.inc.resident = false;
    s.inc.why_not = why;
}

// The one way an entry point of the C ABI runs code that may throw: nothing crosses the extern "C" boundary.  The body
// returns the call's result; a HipErr becomes MI355SAT_ERR_HIP with its text, std::bad_alloc MI355SAT_ERR_OOM.  On the
// device (all but GUARD_HOST) the handle's device is selected first; GUARD_TIMED adds the call's time to
// stats.solve_seconds, whichever way it ends.
enum GuardKind { GUARD_HOST, GUARD_DEVICE, GUARD_TIMED };
template <class F>
int guarded(mi355sat* s, GuardKind kind, F&& body) {
    const double t0 = kind == GUARD_TIMED ? now_s() : 0;
    int rc;
    try {
        if (kind != GUARD_HOST) HIPCHK(hipSetDevice(s->device));
        rc = body();
    } catch (HipErr& he) {
        s->err = he.msg;
        rc = he.code;
    } catch (std::bad_alloc&) {
        s->err = "out of host memory";
        rc = MI355SAT_ERR_OOM;
    }
    if (kind == GUARD_TIMED) s->stats.solve_seconds += now_s() - t0;
    return rc;
}

// What in stats describes the caller's last solve / batch - what the simplification did to the formula, the fleet's size -
// and not an upload made on the side (a running sweep's totals, core minimisation).
inline void keep_last_solve_stats(mi355sat_stats_t& dst, const mi355sat_stats_t& src) {
    dst.simp_units = src.simp_units; dst.simp_equivalences = src.simp_equivalences;
    dst.simp_clauses_removed = src.simp_clauses_removed; dst.simp_eliminated = src.simp_eliminated;
    dst.workers = src.workers;
}

inline void tally_answer(mi355sat& s, int result) {
    if (result == MI355SAT_SAT) { s.stats.n_sat++; s.sat_clauses = s.offs.size(); }
    else if (result == MI355SAT_UNSAT) s.stats.n_unsat++;
    else s.stats.n_terminated++;
}

// A caller's lists (data[offsets[i] .. offsets[i + 1]) for i < n; offsets[0] need not be 0) as a copy with offsets from 0.
inline void copy_lists(const int32_t* data, const uint64_t* offsets, uint64_t n, std::vector<int32_t>& out, std::vector<uint64_t>& off) {
    off.assign(offsets, offsets + n + 1);
    for (auto& o : off) o -= offsets[0];
    out.clear();
    if (off.back()) out.assign(data + offsets[0], data + offsets[n]);
}

// Variable order for the device: every per-variable array (the 2-bit assignment: 256 variables per
// 64-byte line; records, watch and list headers: 4 per line) is gathered by variable index, so
// variables that meet in clauses should be neighbours.  The caller's numbering is by encoder family;
// this one grows blobs of 256 variables breadth-first through the clauses (variable - clause -
// variable), each new blob seeded on the border of an earlier one, so a blob is a compact patch of the
// variable interaction graph (for the support grids: a few neighbouring tiles with all their
// variables, or a subtree of the totalizer).  Fixed and unused variables go last.
void locality_order(uint32_t nv, const std::vector<int32_t>& nl, const std::vector<uint64_t>& no,
                    const std::vector<int8_t>& val, std::vector<uint32_t>& perm) {
    const uint32_t NONE = 0xffffffffu, BLOB = 256;
    const size_t nn = no.size() - 1;
    perm.assign(nv, NONE);
    std::vector<uint32_t> occ_off((size_t)nv + 1, 0);
    for (size_t c = 0; c < nn; c++) {
        if (no[c + 1] - no[c] > 64) continue;
        for (uint64_t k = no[c]; k < no[c + 1]; k++) occ_off[(nl[k] >> 1) + 1]++;
    }
    for (size_t i = 0; i < nv; i++) occ_off[i + 1] += occ_off[i];
    std::vector<uint32_t> occ(occ_off[nv]), fill(occ_off.begin(), occ_off.end() - 1);
    for (size_t c = 0; c < nn; c++) {
        if (no[c + 1] - no[c] > 64) continue;
        for (uint64_t k = no[c]; k < no[c + 1]; k++) occ[fill[nl[k] >> 1]++] = (uint32_t)c;
    }
    std::vector<uint32_t> vstamp(nv, 0), cstamp(nn, 0), frontier, q;
    std::vector<uint8_t> pending(nv, 0);
    size_t fhead = 0;
    uint32_t next = 0, blob = 0, scan = 0;
    for (;;) {
        uint32_t seed = NONE;
        while (fhead < frontier.size()) { uint32_t v = frontier[fhead++]; if (perm[v] == NONE) { seed = v; break; } }
        if (seed == NONE) {
            while (scan < nv && (perm[scan] != NONE || val[scan] != 0 || occ_off[scan] == occ_off[scan + 1])) scan++;
            if (scan == nv) break;
            seed = scan;
        }
        blob++;
        q.clear();
        q.push_back(seed);
        vstamp[seed] = blob;
        size_t h = 0;
        uint32_t cnt = 0;
        while (h < q.size() && cnt < BLOB) {
            const uint32_t v = q[h++];
            perm[v] = next++;
            cnt++;
            for (uint32_t e = occ_off[v]; e < occ_off[v + 1]; e++) {
                const uint32_t c = occ[e];
                if (cstamp[c] == blob) continue;
                cstamp[c] = blob;
                for (uint64_t k = no[c]; k < no[c + 1]; k++) {
                    const uint32_t u = (uint32_t)(nl[k] >> 1);
                    if (perm[u] != NONE || vstamp[u] == blob || val[u] != 0) continue;
                    vstamp[u] = blob;
                    q.push_back(u);
                }
            }
        }
        for (; h < q.size(); h++)   // the blob is full: its border seeds later blobs
            if (!pending[q[h]]) { pending[q[h]] = 1; frontier.push_back(q[h]); }
    }
    for (uint32_t v = 0; v < nv; v++) if (perm[v] == NONE) perm[v] = next++;
}

// The caller's clauses in normal form (internal literals 2*var + neg, caller's numbering; sorted, no duplicate
// literals, no tautologies, no units): what the simplification steps work on.
struct Formula {
    uint32_t nv = 0;
    bool unsat = false;
    std::vector<int32_t> nl;                 // literals
    std::vector<uint64_t> no{0};             // clause offsets
    std::vector<int8_t> val;                 // level-0 facts: 0 unassigned, 1 true, -1 false
    std::vector<int32_t> units;              // the same as a list, in derivation order
    size_t units_done = 0;                   // units[0..units_done) have been propagated through nl / no
    std::vector<int32_t> subst;              // per variable: the literal that replaces it (2*v = itself)
    std::vector<int32_t> proof;              // DRUP lemmas justifying units / equivalences / rewritten clauses (-1 terminated)
    bool log_proof = false;
    std::vector<int32_t> frozen_lits;        // internal literals (caller's numbering) whose variables must survive: the assumptions
    std::vector<MsElim> elims;               // eliminated variables in elimination order + the clauses that rebuild their value
    std::vector<int32_t> elim_lits;
    uint64_t n_failed = 0, n_necessary = 0, n_equiv = 0, n_subsumed = 0, n_strengthened = 0, n_eliminated = 0;
    size_t n_clauses() const { return no.size() - 1; }
    int8_t lv(int32_t l) const { int8_t v = val[l >> 1]; return (l & 1) ? (int8_t)-v : v; }
    bool assign_unit(int32_t l) {            // false on contradiction
        const int8_t want = (l & 1) ? -1 : 1;
        int8_t& v = val[l >> 1];
        if (v == 0) { v = want; units.push_back(l); return true; }
        return v == want;
    }
    void lemma(std::initializer_list<int32_t> c) { if (log_proof) { proof.insert(proof.end(), c); proof.push_back(-1); } }
    void lemma(const std::vector<int32_t>& c) { if (log_proof) { proof.insert(proof.end(), c.begin(), c.end()); proof.push_back(-1); } }
};

// Sort / dedupe / drop tautologies of one clause; units go to F.val.  Returns false if the clause is dropped.
bool normal_clause(Formula& F, std::vector<int32_t>& tmp) {
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    for (size_t i = 0; i + 1 < tmp.size(); i++) if ((tmp[i] ^ 1) == tmp[i + 1]) return false;
    if (tmp.empty()) { F.unsat = true; return false; }
    if (tmp.size() == 1) { if (!F.assign_unit(tmp[0])) F.unsat = true; return false; }
    return true;
}

void normalise(const mi355sat& s, Formula& F) {
    F.nv = (uint32_t)s.max_var;
    F.val.assign(F.nv, 0);
    F.subst.resize(F.nv);
    for (uint32_t v = 0; v < F.nv; v++) F.subst[v] = 2 * (int32_t)v;
    const size_t nc = s.offs.size() - 1;
    F.nl.reserve(s.lits.size());
    std::vector<int32_t> tmp;
    for (size_t c = 0; c < nc && !F.unsat; c++) {
        tmp.clear();
        for (uint64_t k = s.offs[c]; k < s.offs[c + 1]; k++) tmp.push_back(to_internal(s.lits[k]));
        if (!normal_clause(F, tmp)) continue;
        F.nl.insert(F.nl.end(), tmp.begin(), tmp.end());
        F.no.push_back(F.nl.size());
    }
}

// Level-0 unit propagation over occurrence lists, then strip satisfied clauses and false literals.
void propagate_units(Formula& F) {
    if (F.unsat || F.units_done == F.units.size()) return;
    const uint32_t nv = F.nv;
    const size_t nn = F.n_clauses();
    std::vector<uint32_t> occ_off(2 * (size_t)nv + 1, 0);
    for (int32_t l : F.nl) occ_off[l + 1]++;
    for (size_t i = 0; i < 2 * (size_t)nv; i++) occ_off[i + 1] += occ_off[i];
    std::vector<uint32_t> occ(F.nl.size()), fill(occ_off.begin(), occ_off.end() - 1);
    for (size_t c = 0; c < nn; c++)
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) occ[fill[F.nl[k]]++] = (uint32_t)c;
    size_t qh = F.units_done;
    while (qh < F.units.size() && !F.unsat) {
        const int32_t f = F.units[qh++] ^ 1;
        for (uint32_t e = occ_off[f]; e < occ_off[f + 1] && !F.unsat; e++) {
            const uint32_t c = occ[e];
            int32_t unit = -1;
            int nfree = 0;
            bool sat = false;
            for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) {
                const int8_t v = F.lv(F.nl[k]);
                if (v > 0) { sat = true; break; }
                if (v == 0) { nfree++; unit = F.nl[k]; }
            }
            if (sat) continue;
            if (nfree == 0) F.unsat = true;
            else if (nfree == 1 && !F.assign_unit(unit)) F.unsat = true;
        }
    }
    if (F.unsat) return;
    F.units_done = F.units.size();
    std::vector<int32_t> nl2;
    std::vector<uint64_t> no2{0};
    nl2.reserve(F.nl.size());
    for (size_t c = 0; c < nn; c++) {
        bool sat = false;
        const size_t start = nl2.size();
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) {
            const int8_t v = F.lv(F.nl[k]);
            if (v > 0) { sat = true; break; }
            if (v == 0) nl2.push_back(F.nl[k]);
        }
        if (sat) { nl2.resize(start); continue; }
        no2.push_back(nl2.size());
    }
    F.nl.swap(nl2);
    F.no.swap(no2);
}

// Device form of the formula: variable order, binary / ternary CSRs, long clauses.
// identity_order: the caller's variable order whatever opts.var_order says (the proof checker's trusted base).
void build_csr(const mi355sat& s, const Formula& F, bool units_propagated, Prepared& P, bool identity_order = false) {
    const uint32_t nv = F.nv;
    P.n_vars = nv;
    P.unsat = F.unsat;
    P.units = F.units;
    P.units_propagated = units_propagated;
    if (P.unsat) return;
    std::vector<int32_t> nl = F.nl;
    const std::vector<uint64_t>& no = F.no;
    const size_t nn = F.n_clauses();
    // device variable order
    if (s.opts.var_order > 0 && !identity_order) locality_order(nv, nl, no, F.val, P.perm);
    else { P.perm.resize(nv); for (uint32_t v = 0; v < nv; v++) P.perm[v] = v; }
    for (auto& l : nl) l = 2 * (int32_t)P.perm[l >> 1] | (l & 1);
    for (auto& l : P.units) l = 2 * (int32_t)P.perm[l >> 1] | (l & 1);
    // split: binary -> implication CSR, ternary -> pair CSR, >= 4 literals -> watched clauses
    std::vector<std::pair<int32_t, int32_t>> bins;
    std::vector<std::array<int32_t, 3>> terns;
    for (size_t c = 0; c < nn; c++) {
        uint64_t len = no[c + 1] - no[c];
        if (len == 2) bins.push_back({nl[no[c]], nl[no[c] + 1]});
        else if (len == 3) terns.push_back({nl[no[c]], nl[no[c] + 1], nl[no[c] + 2]});
        else {
            P.cl_hdr.push_back(MsClauseHdr{(uint32_t)P.cl_lits.size(), (uint32_t)len});
            P.cl_lits.insert(P.cl_lits.end(), nl.begin() + no[c], nl.begin() + no[c + 1]);
            while (P.cl_lits.size() % 4) P.cl_lits.push_back(nl[no[c]]);
        }
    }
    for (int k = 0; k < 4; k++) P.cl_lits.push_back(0);  // a lane may read one 16-byte group past the last clause
    for (auto& b : bins) if (b.first > b.second) std::swap(b.first, b.second);
    std::sort(bins.begin(), bins.end());
    bins.erase(std::unique(bins.begin(), bins.end()), bins.end());
    for (auto& c : terns) std::sort(c.begin(), c.end());
    std::sort(terns.begin(), terns.end());
    terns.erase(std::unique(terns.begin(), terns.end()), terns.end());
    P.lit_hdr.assign(2 * (size_t)nv, MsLitHdr{0, 0, 0, 0});
    for (auto& b : bins) { P.lit_hdr[b.first ^ 1].bin_n++; P.lit_hdr[b.second ^ 1].bin_n++; }
    for (auto& c : terns)
        for (int k = 0; k < 3; k++) P.lit_hdr[c[k] ^ 1].tern_n++;
    {
        uint32_t bo = 0, to = 0;
        for (auto& hd : P.lit_hdr) { hd.bin_off = bo; bo += hd.bin_n; hd.tern_off = to; to += hd.tern_n; }
    }
    P.bin_lits.resize(2 * bins.size());
    {
        std::vector<uint32_t> fill(2 * (size_t)nv);
        for (size_t i = 0; i < fill.size(); i++) fill[i] = P.lit_hdr[i].bin_off;
        for (auto& b : bins) {
            P.bin_lits[fill[b.first ^ 1]++] = b.second;   // ~a -> b
            P.bin_lits[fill[b.second ^ 1]++] = b.first;   // ~b -> a
        }
    }
    P.tern_pairs.resize(3 * terns.size());
    P.tern_owner.resize(3 * terns.size());
    {
        std::vector<uint32_t> fill(2 * (size_t)nv);
        for (size_t i = 0; i < fill.size(); i++) fill[i] = P.lit_hdr[i].tern_off;
        for (auto& c : terns)
            for (int k = 0; k < 3; k++) {
                uint32_t e = fill[c[k] ^ 1]++;          // list of the literal that makes c[k] false
                P.tern_pairs[e] = ms_int2{c[(k + 1) % 3], c[(k + 2) % 3]};
                P.tern_owner[e] = c[k] ^ 1;
            }
    }
}

void prepare(const mi355sat& s, bool simplify, Prepared& P, bool identity_order = false) {
    Formula F;
    normalise(s, F);
    if (simplify) propagate_units(F);
    build_csr(s, F, simplify, P, identity_order);
}

// ---- slab template -----------------------------------------------------------------
// learnt_cap / learnt_lit_cap: 0 = the rule below (what a search wants); the proof checker sizes both stores from its proof.
// pool_slack (test hook, mi355sat_debug_set_capacities): the watch pool is the initial lists plus that many entries; 0 = the rule.
void build_layout_and_template(mi355sat& s, const Prepared& P, uint32_t assump_cap, uint32_t script_cap,
                               std::vector<char>& tmpl, uint32_t learnt_cap = 0, uint32_t learnt_lit_cap = 0, uint32_t pool_slack = 0) {
    const uint32_t nv = P.n_vars, no = (uint32_t)P.cl_hdr.size();
    MsLayout& L = s.L;
    memset(&L, 0, sizeof L);
    L.n_vars = nv;
    L.n_orig = no;
    // capacities
    const uint64_t base_lits = P.cl_lits.size() + 3 * P.tern_pairs.size() / 3;
    L.learnt_cap = (uint32_t)std::min<uint64_t>(1u << 17, std::max<uint64_t>(1u << 15, 2 * (uint64_t)no + 4096));
    // (round 2: 2 M literals at most instead of 4 M - a store that runs full reduces early, add_learnt / on_conflict)
    L.learnt_lit_cap = (uint32_t)std::min<uint64_t>(2u << 20, std::max<uint64_t>(1u << 19, 6 * base_lits));
    if (learnt_cap) L.learnt_cap = learnt_cap;
    if (learnt_lit_cap) L.learnt_lit_cap = learnt_lit_cap;
    L.vm_cap = 3 * nv + 256;
    L.assump_cap = assump_cap;
    L.script_cap = script_cap;
    // watch lists: literal t's list holds the clauses currently watching ~t.  Initial slots get
    // 50% + 2 entries of slack; a list that outgrows its slot moves to the top of the bump pool and
    // the device compacts the pool again at every learnt-clause reduction (rebuild_watches).
    std::vector<uint32_t> cap(2 * (size_t)nv, 0);
    for (uint32_t c = 0; c < no; c++) { cap[P.cl_lits[P.cl_hdr[c].start] ^ 1]++; cap[P.cl_lits[P.cl_hdr[c].start + 1] ^ 1]++; }
    uint64_t pool_need = 0;
    std::vector<uint32_t> base(2 * (size_t)nv);
    for (size_t t = 0; t < cap.size(); t++) {
        cap[t] += (cap[t] >> 1) + 2;
        base[t] = (uint32_t)pool_need;
        pool_need += cap[t];
    }
    // room for a dense rebuild with every learnt slot in use, plus 50% for relocations in between
    uint64_t dense_max = 3 * ((uint64_t)no + L.learnt_cap) + 4 * (uint64_t)nv;   // (rebuild_watches: size + size/2 + 2 per list)
    uint64_t pool_cap = dense_max + dense_max / 2 + (1u << 16);
    if (pool_slack) pool_cap = pool_need + pool_slack;
    if (pool_cap > 0xfffffff0ull) throw HipErr{"formula too large (watch pool)"};
    L.pool_cap = (uint32_t)pool_cap;
    size_t off = 0;
    auto place = [&](uint64_t& field, size_t bytes) { field = off; off = align_up(off + bytes, 256); };
    place(L.state, sizeof(MsState));
    place(L.val, 16 * (((size_t)nv + 15) / 16));
    place(L.vrec, sizeof(MsVarRec) * (size_t)nv);
    place(L.vm_pos, 4 * (size_t)nv);
    place(L.best, (size_t)nv);
    place(L.trail, 4 * (size_t)nv);
    place(L.trail_lim, 4 * ((size_t)nv + 1));
    place(L.vm_order, 4 * (size_t)L.vm_cap);
    place(L.wl, sizeof(MsClauseRec) * ((size_t)no + L.learnt_cap));
    place(L.whdr, sizeof(MsWatchHdr) * 2 * (size_t)nv);
    place(L.lc_lbd, 4 * (size_t)L.learnt_cap);
    place(L.learnt_buf, 4 * ((size_t)nv + 1));
    place(L.toclear, 4 * ((size_t)nv + 1));
    place(L.lvl_stamp, 4 * ((size_t)nv + 2));
    place(L.remap, 4 * (size_t)L.learnt_cap);
    place(L.overflow, 4 * 3 * MS_OVERFLOW_CAP);
    place(L.assumps, 4 * (size_t)std::max<uint32_t>(assump_cap, 1));
    place(L.script, 4 * (size_t)std::max<uint32_t>(script_cap, 1));
    place(L.exp, 4 * (size_t)MS_EXPORT_RECS * MS_SHARE_REC);
    // the big, cold-tailed arrays last
    place(L.lc_lits, 4 * (size_t)L.learnt_lit_cap);
    place(L.pool, 16 * (size_t)L.pool_cap);
    L.slab_bytes = align_up(off, 4096);

    // Only the head of the slab (everything before lc_lits) plus the initial watch
    // pool needs initial contents; lc_lits is left as allocated.
    tmpl.assign(L.slab_bytes, 0);
    char* T = tmpl.data();
    MsState* st = (MsState*)(T + L.state);
    st->status = MS_ST_RUNNING;
    st->trail_n = (int32_t)P.units.size();
    st->qhead = P.units_propagated ? st->trail_n : 0;
    st->n_levels = 0;
    st->vm_end = (int32_t)nv;
    st->vm_search = (int32_t)nv - 1;
    st->pool_top = (uint32_t)pool_need;
    s.pool_init = pool_need;
    st->next_reduce = s.opts.reduce_first > 0 ? (uint64_t)s.opts.reduce_first : 2000;
    st->next_rephase = s.rephase_every ? s.rephase_every : 2000;
    st->next_vivify = s.first_vivify ? s.first_vivify : 1500;   // (easy bounds are decided before that: vivification is for the long refutations)
    memset(T + L.best, 255, nv);
    uint8_t* val = (uint8_t*)(T + L.val);        // zero = every variable unassigned
    MsVarRec* vrec = (MsVarRec*)(T + L.vrec);
    int32_t* vm_order = (int32_t*)(T + L.vm_order);
    // initial decision order: the caller's numbering (the search starts at position nv - 1); variables that occur in no
    // clause (replaced by an equivalent literal, eliminated) behind all others
    std::vector<uint8_t> occurs(nv, 0);
    for (const MsClauseHdr& h : P.cl_hdr)      // (cl_lits carries padding behind the last clause)
        for (uint32_t k = 0; k < h.size; k++) occurs[P.cl_lits[h.start + k] >> 1] = 1;
    for (size_t t = 0; t < P.lit_hdr.size(); t++) if (P.lit_hdr[t].bin_n || P.lit_hdr[t].tern_n) occurs[t >> 1] = 1;
    uint32_t pos = nv;
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t e = 0; e < nv; e++) {
            const uint32_t v = P.perm[e];
            if ((occurs[v] != 0) != (pass == 0)) continue;
            pos--;
            vrec[v] = MsVarRec{0, MS_REASON_NONE, 0, 0, /*phase=*/1, /*seen=*/0};
            ((int32_t*)(T + L.vm_pos))[v] = (int32_t)pos;
            vm_order[pos] = (int32_t)v;
        }
    int32_t* trail = (int32_t*)(T + L.trail);
    for (size_t i = 0; i < P.units.size(); i++) {
        int32_t l = P.units[i];
        trail[i] = l;
        val[l >> 1] = (uint8_t)(2u | (uint32_t)(l & 1));
    }
    MsClauseRec* wl = (MsClauseRec*)(T + L.wl);
    MsWatchHdr* whdr = (MsWatchHdr*)(T + L.whdr);
    int4* pool = (int4*)(T + L.pool);
    for (size_t t = 0; t < cap.size(); t++)
        whdr[MS_HIDX(t, nv)] = MsWatchHdr{base[t], 0, cap[t], 0, P.lit_hdr[t].bin_off, P.lit_hdr[t].bin_n, P.lit_hdr[t].tern_off, P.lit_hdr[t].tern_n};
    for (uint32_t c = 0; c < no; c++) {
        int32_t a = P.cl_lits[P.cl_hdr[c].start], b = P.cl_lits[P.cl_hdr[c].start + 1];
        wl[c] = MsClauseRec{a, b, P.cl_hdr[c].start, P.cl_hdr[c].size};
        pool[whdr[MS_HIDX(a ^ 1, nv)].base + whdr[MS_HIDX(a ^ 1, nv)].size++] = make_int4((int)c, b, (int)P.cl_hdr[c].start, (int)P.cl_hdr[c].size);
        pool[whdr[MS_HIDX(b ^ 1, nv)].base + whdr[MS_HIDX(b ^ 1, nv)].size++] = make_int4((int)c, a, (int)P.cl_hdr[c].start, (int)P.cl_hdr[c].size);
    }
}

void set_error(mi355sat* s, const std::string& m) { s->err = m; }

void upload_formula(mi355sat& s, const Prepared& P, uint32_t assump_cap, uint32_t script_cap, uint32_t want_workers,
                    uint32_t initial_workers = 0, uint32_t learnt_cap = 0, uint32_t learnt_lit_cap = 0, int no_room_code = MI355SAT_ERR_HIP,
                    uint32_t pool_slack = 0) {
    HIPCHK(hipSetDevice(s.device));
    std::vector<char> tmpl;
    build_layout_and_template(s, P, assump_cap, script_cap, tmpl, learnt_cap, learnt_lit_cap, pool_slack);
    s.n_vars = P.n_vars;
    s.perm = P.perm;
    s.d_cl_lits.upload(P.cl_lits, s.stream);
    s.d_bin_lits.upload_nonempty(P.bin_lits, s.stream);
    s.d_tern_pairs.upload_nonempty(P.tern_pairs, s.stream);
    s.d_tern_owner.upload_nonempty(P.tern_owner, s.stream);
    s.sh.n_vars = P.n_vars;
    s.sh.n_orig = (uint32_t)P.cl_hdr.size();
    s.sh.cl_lits = s.d_cl_lits.p;
    s.sh.bin_lits = s.d_bin_lits.p;
    s.sh.tern_pairs = s.d_tern_pairs.p;
    s.sh.tern_owner = s.d_tern_owner.p;
    // assignment in LDS (2 bits per variable) when it still leaves room for 12 waves per CU
    // (measured on rect 64x64: 12 waves/CU with the assignment in HBM beat 6 waves/CU with it in LDS)
    s.lds_val_bytes = ((P.n_vars + 15) / 16) * 4 + 5 * ((P.n_vars + 31) / 32) * 4;   // 2-bit assignment + five 1-bit maps (marks, current level, level 0, minimisation: failed, queued)
    s.lds_val = staged_in_lds(s.opts.lds_val, s.lds_val_bytes);
    // worker count limited by free HBM
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += SlabBuf::cached_bytes(s.device);   // a parked slab buffer of an earlier handle is ours to reuse
    uint64_t fit = (uint64_t)((double)free_b * 0.85) / (s.L.slab_bytes * 1ull);
    if (fit < 2) throw HipErr{"not enough device memory for one worker slab", no_room_code};
    uint32_t W = (uint32_t)std::min<uint64_t>(want_workers, fit - 1);
    if (W == 0) W = 1;
    s.n_workers = W;
    s.d_template.alloc(s.L.slab_bytes);
    HIPCHK(hipMemcpyAsync(s.d_template.p, tmpl.data(), s.L.slab_bytes, hipMemcpyHostToDevice, s.stream));
    // Slabs for `initial_workers` only (the ramp-up's first phase) unless a parked buffer already covers all of
    // them: hipMalloc costs ~30 ms per GiB, and an easy instance never needs the rest (grow_workers).
    uint32_t A = W;
    if (initial_workers && initial_workers < W && SlabBuf::cached_bytes(s.device) < (size_t)W * s.L.slab_bytes) A = initial_workers;
    s.n_alloc = A;
    const double t_alloc0 = now_s();
    s.d_slabs.alloc((size_t)A * s.L.slab_bytes, s.device);
    if (s.opts.verbose) fprintf(stderr, "[mi355sat] slab allocation %.1f GiB (%u of %u workers): %.3f s\n", (double)A * s.L.slab_bytes / 1073741824.0, A, W, now_s() - t_alloc0);
    s.d_states.alloc(W);
    s.d_any_done.alloc(1);
    // clause exchange: on unless switched off, whenever there is more than one worker
    s.share_slots = 0;
    if (s.opts.share >= 0 && W > 1 && script_cap == 0) {
        s.share_slots = 1u << 19;   // 64 MiB of records
        while ((uint64_t)s.share_slots < (uint64_t)W * MS_EXPORT_RECS) s.share_slots <<= 1;   // one collection (<= W * MS_EXPORT_RECS
                                                                                              // records) never wraps onto itself
        s.share_hash_n = 1u << 22;
        s.d_share_pool.alloc((size_t)s.share_slots * MS_SHARE_REC);
        s.d_share_n.alloc(1);
        s.d_share_hash.alloc(s.share_hash_n);
        s.d_share_intake.alloc(1);
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    if (s.opts.verbose)
        fprintf(stderr, "[mi355sat] vars=%u long=%u tern=%zu bin=%zu units=%zu slab=%.2f MiB workers=%u lds_val=%d\n", P.n_vars,
                s.sh.n_orig, P.tern_pairs.size() / 3, P.bin_lits.size() / 2, P.units.size(), s.L.slab_bytes / 1048576.0, W, (int)s.lds_val);
}

// Replicate the template into every worker slab (head + initial watch pool only).
void replicate_template(mi355sat& s, uint32_t from, uint32_t to) {   // workers [from, to)
    const MsLayout& L = s.L;
    const size_t head = L.lc_lits;  // everything before the learnt literal store
    if (to <= from) return;
    hipLaunchKernelGGL(ms_replicate_kernel, dim3(64, to - from), dim3(256), 0, s.stream, (const char*)s.d_template.p,
                       s.d_slabs.p + (size_t)from * L.slab_bytes, (uint64_t)L.slab_bytes, (uint64_t)head, (uint64_t)L.pool,
                       (uint64_t)(16 * s.pool_init));
    HIPCHK(hipGetLastError());
}

void reset_workers(mi355sat& s) {
    replicate_template(s, 0, s.n_alloc);
    HIPCHK(hipMemsetAsync(s.d_any_done.p, 0, sizeof(int32_t), s.stream));
    if (s.share_slots) {
        HIPCHK(hipMemsetAsync(s.d_share_n.p, 0, sizeof(unsigned long long), s.stream));
        HIPCHK(hipMemsetAsync(s.d_share_hash.p, 0, sizeof(unsigned long long) * s.share_hash_n, s.stream));
        s.share_slices = 0;
        s.share_export_pos = 0;
    }
}

void customize(mi355sat& s, const std::vector<int32_t>* assump, const std::vector<uint64_t>* assump_off,
               const std::vector<int32_t>* script, const std::vector<uint64_t>* script_off, uint32_t n_instances,
               int32_t park_from = -1) {
    if (assump_off) {
        s.d_assump.upload_nonempty(*assump, s.stream);
        s.d_assump_off.upload(*assump_off, s.stream);
    }
    if (script_off) {
        s.d_script.upload_nonempty(*script, s.stream);
        s.d_script_off.upload(*script_off, s.stream);
    }
    hipLaunchKernelGGL(ms_customize_kernel, dim3(s.n_alloc), dim3(256), 0, s.stream, s.L, s.d_slabs.p,
                       s.n_alloc, assump_off ? s.d_assump.p : nullptr, assump_off ? s.d_assump_off.p : nullptr,
                       script_off ? s.d_script.p : nullptr, script_off ? s.d_script_off.p : nullptr, n_instances,
                       s.opts.seed, park_from, 0u, s.opts.phase_mix);
    HIPCHK(hipGetLastError());
}

// ---- phase hints -------------------------------------------------------------------------------------------------------
// The handle's hints in the device's variables, as ms_phase_kernel reads them (one byte per device variable: 0 none, 1
// TRUE first, 2 FALSE first), uploaded: through the equivalent-literal substitution, which may flip the sign, then the
// device's variable order - the route of the assumptions (map_assumptions).  In increasing caller-variable order, so of
// two hints that meet on one representative the later one wins.  An eliminated variable has no device variable, one
// fixed at level 0 no phase to seed: counted.
void map_phases(mi355sat& s) {
    mi355sat::Phases& ph = s.ph;
    std::vector<uint8_t> bytes(s.n_vars, 0), gone(s.n_vars, 0);
    for (const MsElim& e : s.elims) gone[e.x >> 1] = 1;
    ph.info.dropped_eliminated = ph.info.dropped_fixed = ph.info.mapped = 0;
    for (size_t v = 0; v < ph.hint.size() && v < s.n_vars; v++) {
        if (!ph.hint[v]) continue;
        const int32_t l = device_literal(s, s.perm, ph.hint[v] < 0 ? -(int32_t)(v + 1) : (int32_t)(v + 1), &gone);
        if (l < 0) { ph.info.dropped_eliminated++; continue; }
        const uint32_t dv = (uint32_t)(l >> 1);
        if (dv < ph.dev_fixed.size() && ph.dev_fixed[dv]) { ph.info.dropped_fixed++; continue; }
        bytes[dv] = (uint8_t)(1 + (l & 1));
    }
    for (uint8_t b : bytes) ph.info.mapped += b != 0;
    ph.on_device = ph.info.mapped > 0;
    if (ph.on_device) s.d_phase.upload(bytes, s.stream);
}

// Seeds workers [from, to) with the hints on the device (nothing to do without any), on the stream.
void seed_phases(mi355sat& s, uint32_t from, uint32_t to) {
    if (!s.ph.on_device || to <= from || s.L.n_vars == 0) return;
    for (uint32_t w = from; w < to; w += 32768) {   // (gridDim.y is a 16-bit number)
        const uint32_t n = std::min(to - w, 32768u);
        hipLaunchKernelGGL(ms_phase_kernel, dim3((s.L.n_vars + 255) / 256, n), dim3(256), 0, s.stream, s.L, s.d_slabs.p, w, w + n,
                           (const uint8_t*)s.d_phase.p);
        HIPCHK(hipGetLastError());
        s.ph.info.launches++;
    }
}

// A cold start seeds every worker it created; a warm one the resident workers, and only if a hint changed since they
// were last seeded (they keep the phases they saved otherwise).  The workers stand at level 0 in both cases.
void apply_phases(mi355sat& s, bool warm) {
    mi355sat::Phases& ph = s.ph;
    if (warm && ph.applied == ph.version) return;
    ph.applied = ph.version;
    ph.on_device = false;
    if (!ph.info.hinted) return;     // (a cleared hint takes nothing back: what it seeded is the worker's saved phase now)
    map_phases(s);
    seed_phases(s, 0, s.n_alloc);
    HIPCHK(hipStreamSynchronize(s.stream));
    (warm ? ph.info.applied_warm : ph.info.applied_cold)++;
}

// The search outlived the ramp-up's first phase: give the remaining workers their slabs.  The running workers'
// slabs move into the full-size buffer (device-to-device copy), the new ones start from the template with the
// assumption list of instance w % n_instances, as at the beginning.
void grow_workers(mi355sat& s, uint32_t n_instances, uint32_t target) {
    target = std::min(target, s.n_workers);
    if (s.n_alloc >= target) return;
    const uint32_t old = s.n_alloc;
    const double t0 = now_s();
    if (s.d_slabs.cap >= (size_t)target * s.L.slab_bytes) {
        // the buffer came from the parked one of an earlier handle (or of this handle's probing) and has the room
        // already: no allocation (hipMalloc of 8.7 GiB is 0.25 s - a quarter of the rect 24x24 ladder), no move
        s.d_slabs.n = (size_t)target * s.L.slab_bytes;
    } else {
        SlabBuf big;
        big.alloc((size_t)target * s.L.slab_bytes, s.device);
        HIPCHK(hipMemcpyAsync(big.p, s.d_slabs.p, (size_t)old * s.L.slab_bytes, hipMemcpyDeviceToDevice, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        std::swap(big.p, s.d_slabs.p); std::swap(big.n, s.d_slabs.n); std::swap(big.cap, s.d_slabs.cap); std::swap(big.dev, s.d_slabs.dev);
        big.release();   // the small buffer (parked if nothing larger is)
    }
    s.n_alloc = target;
    replicate_template(s, old, s.n_alloc);
    hipLaunchKernelGGL(ms_customize_kernel, dim3(s.n_alloc - old), dim3(256), 0, s.stream, s.L, s.d_slabs.p, s.n_alloc,
                       s.d_assump.p, s.d_assump_off.p, (const int32_t*)nullptr, (const uint64_t*)nullptr, n_instances, s.opts.seed,
                       -1, old, s.opts.phase_mix);
    HIPCHK(hipGetLastError());
    seed_phases(s, old, s.n_alloc);      // the phase hints, as the workers of the first stage got them
    HIPCHK(hipStreamSynchronize(s.stream));
    if (s.opts.verbose) fprintf(stderr, "[mi355sat] grew from %u to %u worker slabs (%.1f GiB): %.3f s\n", old, s.n_alloc,
                                (double)s.n_alloc * s.L.slab_bytes / 1073741824.0, now_s() - t0);
}

void gather_states(mi355sat& s, std::vector<MsState>& out) {
    out.assign(s.n_workers, MsState{});   // a worker without a slab yet: RUNNING, all counters zero
    hipLaunchKernelGGL(ms_gather_states_kernel, dim3((s.n_alloc + 63) / 64), dim3(64), 0, s.stream, s.L,
                       s.d_slabs.p, s.n_alloc, s.d_states.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out.data(), s.d_states.p, sizeof(MsState) * s.n_alloc, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
}

// ---- formula simplification before search (`simp::Glucose`, crates/repl/src/main.rs:17) --------------------------
// Equivalent-literal substitution: strongly connected components of the binary implication graph (iterative
// Tarjan on the host - a few 10^5 edges), every literal replaced by the smallest literal of its component.
uint64_t els_scc(Formula& F) {
    if (F.unsat) return 0;
    const uint32_t nl2 = 2 * F.nv;
    const size_t nn = F.n_clauses();
    std::vector<uint32_t> off(nl2 + 1, 0);
    for (size_t c = 0; c < nn; c++)
        if (F.no[c + 1] - F.no[c] == 2) { off[(F.nl[F.no[c]] ^ 1) + 1]++; off[(F.nl[F.no[c] + 1] ^ 1) + 1]++; }
    for (uint32_t i = 0; i < nl2; i++) off[i + 1] += off[i];
    std::vector<int32_t> adj(off[nl2]);
    {
        std::vector<uint32_t> fill(off.begin(), off.end() - 1);
        for (size_t c = 0; c < nn; c++)
            if (F.no[c + 1] - F.no[c] == 2) {
                const int32_t a = F.nl[F.no[c]], b = F.nl[F.no[c] + 1];
                adj[fill[a ^ 1]++] = b;
                adj[fill[b ^ 1]++] = a;
            }
    }
    std::vector<int32_t> index(nl2, -1), low(nl2, 0), rep(nl2, -1), stack, work, it(nl2, 0);
    std::vector<uint8_t> on(nl2, 0);
    int32_t counter = 0;
    for (uint32_t root = 0; root < nl2; root++) {
        if (index[root] >= 0 || off[root] == off[root + 1]) continue;
        work.push_back((int32_t)root);
        while (!work.empty()) {
            const int32_t v = work.back();
            if (index[v] < 0) { index[v] = low[v] = counter++; stack.push_back(v); on[v] = 1; it[v] = (int32_t)off[v]; }
            bool descended = false;
            while (it[v] < (int32_t)off[v + 1]) {
                const int32_t u = adj[it[v]++];
                if (index[u] < 0) { work.push_back(u); descended = true; break; }
                if (on[u]) low[v] = std::min(low[v], index[u]);
            }
            if (descended) continue;
            if (low[v] == index[v]) {
                size_t k = stack.size();
                int32_t m = v;
                do { k--; m = std::min(m, stack[k]); } while (stack[k] != v);
                for (size_t j = k; j < stack.size(); j++) { rep[stack[j]] = m; on[stack[j]] = 0; }
                stack.resize(k);
            }
            work.pop_back();
            if (!work.empty()) low[work.back()] = std::min(low[work.back()], low[v]);
        }
    }
    uint64_t n_sub = 0;
    std::vector<int32_t> map(nl2);
    for (uint32_t l = 0; l < nl2; l++) map[l] = (int32_t)l;
    for (uint32_t v = 0; v < F.nv; v++) {
        const int32_t r = rep[2 * v];
        if (r < 0 || r == (int32_t)(2 * v)) continue;
        if (r == (int32_t)(2 * v + 1)) { F.unsat = true; return 0; }      // x and ~x in one component
        if ((r >> 1) > (int32_t)v) continue;                              // (the mirror component decides)
        map[2 * v] = r;
        map[2 * v + 1] = r ^ 1;
        F.subst[v] = r;
        F.lemma({(int32_t)(2 * v + 1), r});
        F.lemma({(int32_t)(2 * v), r ^ 1});
        n_sub++;
    }
    if (!n_sub) return 0;
    F.n_equiv += n_sub;
    std::vector<int32_t> nl2v, tmp;
    std::vector<uint64_t> no2{0};
    nl2v.reserve(F.nl.size());
    for (size_t c = 0; c < nn && !F.unsat; c++) {
        tmp.clear();
        bool changed = false;
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) { tmp.push_back(map[F.nl[k]]); changed = changed || map[F.nl[k]] != F.nl[k]; }
        if (changed) {
            std::vector<int32_t> lem = tmp;
            std::sort(lem.begin(), lem.end());
            lem.erase(std::unique(lem.begin(), lem.end()), lem.end());
            bool taut = false;
            for (size_t i = 0; i + 1 < lem.size(); i++) taut = taut || (lem[i] ^ 1) == lem[i + 1];
            if (!taut) F.lemma(lem);
        }
        if (!normal_clause(F, tmp)) continue;
        nl2v.insert(nl2v.end(), tmp.begin(), tmp.end());
        no2.push_back(nl2v.size());
    }
    F.nl.swap(nl2v);
    F.no.swap(no2);
    return n_sub;
}

void launch_probe(mi355sat& s);   // below (needs launch parameters)
const char* status_text(int st);

// Failed-literal probing on the device (ms_probe_kernel): both polarities of every variable that still occurs.
uint64_t device_probe(mi355sat& s, Formula& F) {
    if (F.unsat || F.n_clauses() == 0) return 0;
    Prepared P;
    build_csr(s, F, /*units_propagated=*/true, P);
    std::vector<uint8_t> occurs(F.nv, 0);
    for (int32_t l : F.nl) occurs[l >> 1] = 1;
    std::vector<uint32_t> cand;
    for (uint32_t v = 0; v < F.nv; v++) if (occurs[v] && !F.val[v]) cand.push_back(v);
    if (cand.empty()) return 0;
    uint32_t W = (uint32_t)std::min<size_t>(1024, cand.size());
    std::vector<std::vector<int32_t>> per;
    std::vector<int32_t> script;
    std::vector<uint64_t> soff;
    uint32_t cap = 0;
    for (;;) {   // as many workers as the device has room for (the script length is part of the slab layout)
        per.assign(W, {});
        for (size_t i = 0; i < cand.size(); i++) {
            const int32_t dl = 2 * (int32_t)P.perm[cand[i]];
            per[i % W].push_back(dl);
            per[i % W].push_back(dl ^ 1);
        }
        script.clear();
        soff.assign(1, 0);
        cap = 0;
        for (auto& v : per) { script.insert(script.end(), v.begin(), v.end()); soff.push_back(script.size()); cap = std::max<uint32_t>(cap, (uint32_t)v.size()); }
        upload_formula(s, P, 0, cap, W);
        if (s.n_workers >= W) break;
        W = s.n_workers;
    }
    reset_workers(s);
    customize(s, nullptr, nullptr, &script, &soff, W);
    launch_probe(s);
    // results
    std::vector<uint32_t> inv(P.perm.size());
    for (uint32_t e = 0; e < P.perm.size(); e++) inv[P.perm[e]] = e;
    auto to_caller = [&](int32_t dl) { return 2 * (int32_t)inv[dl >> 1] | (dl & 1); };
    const size_t fact_cap = 3 * (((size_t)P.n_vars + 1) / 3);
    std::vector<int32_t> res((size_t)W * cap), nfacts(W);
    HIPCHK(hipMemcpy2D(res.data(), 4 * (size_t)cap, s.d_slabs.p + s.L.script, s.L.slab_bytes, 4 * (size_t)cap, W, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(nfacts.data(), 4, s.d_slabs.p + s.L.learnt_buf, s.L.slab_bytes, 4, W, hipMemcpyDeviceToHost));
    // only as many columns of the fact rows as the busiest worker filled (a full row is n_vars ints per worker)
    size_t fact_used = 0;
    for (uint32_t w = 0; w < W; w++) fact_used = std::max(fact_used, 3 * (size_t)std::max(nfacts[w], 0));
    const size_t fact_row = std::min(fact_cap, fact_used);
    std::vector<int32_t> facts((size_t)W * std::max<size_t>(fact_row, 1));
    if (fact_row) HIPCHK(hipMemcpy2D(facts.data(), 4 * fact_row, s.d_slabs.p + s.L.toclear, s.L.slab_bytes, 4 * fact_row, W, hipMemcpyDeviceToHost));
    std::vector<MsState> sts;
    gather_states(s, sts);
    uint64_t n_new = 0;
    for (uint32_t w = 0; w < W && !F.unsat; w++) {
        if (sts[w].status < 0) throw HipErr{std::string("probing: ") + status_text(sts[w].status)};
        if (sts[w].status == MS_ST_UNSAT) { F.unsat = true; break; }       // conflict among the formula's own units
        for (size_t d = 0; d < per[w].size(); d++)
            if (res[(size_t)w * cap + d] == -1) {                          // failed literal: its negation is a fact
                const int32_t a = to_caller(per[w][d]);
                if (F.val[a >> 1] == 0) { F.lemma({a ^ 1}); F.n_failed++; n_new++; }
                if (!F.assign_unit(a ^ 1)) F.unsat = true;
            }
        for (int32_t f = 0; f < nfacts[w] && 3 * ((size_t)f + 1) <= fact_row && !F.unsat; f++) {
            const int32_t* t = facts.data() + (size_t)w * fact_row + 3 * (size_t)f;
            const int32_t m = to_caller(t[1]), a = to_caller(t[2]);
            if (t[0] == 1) {                                               // a -> m and ~a -> m
                if (F.val[m >> 1] == 0) { F.lemma({a ^ 1, m}); F.lemma({a, m}); F.lemma({m}); F.n_necessary++; n_new++; }
                if (!F.assign_unit(m)) F.unsat = true;
            } else if (t[0] == 2 && (m >> 1) != (a >> 1)) {                // a -> m and ~a -> ~m: m == a, as two binary clauses
                std::vector<int32_t> c1{a ^ 1, m}, c2{a, m ^ 1};
                for (auto* c : {&c1, &c2}) {
                    F.lemma(*c);
                    if (normal_clause(F, *c)) { F.nl.insert(F.nl.end(), c->begin(), c->end()); F.no.push_back(F.nl.size()); }
                }
                n_new++;
            }
        }
    }
    return n_new;
}

// Subsumption / self-subsuming resolution on the device (ms_subsume_kernel), applied on the host.
uint64_t device_subsume(mi355sat& s, Formula& F) {
    if (F.unsat || F.n_clauses() == 0) return 0;
    const size_t nn = F.n_clauses();
    std::vector<unsigned long long> sig(nn, 0);
    std::vector<uint32_t> occ_off(2 * (size_t)F.nv + 1, 0);
    for (size_t c = 0; c < nn; c++)
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) {
            sig[c] |= 1ull << (((uint32_t)(F.nl[k] >> 1) * 2654435761u) >> 26);
            occ_off[F.nl[k] + 1]++;
        }
    for (size_t i = 0; i < 2 * (size_t)F.nv; i++) occ_off[i + 1] += occ_off[i];
    std::vector<uint32_t> occ(F.nl.size()), fill(occ_off.begin(), occ_off.end() - 1);
    for (size_t c = 0; c < nn; c++)
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) occ[fill[F.nl[k]]++] = (uint32_t)c;
    DevBuf<int32_t> d_lits, d_drop;
    DevBuf<uint64_t> d_offs;
    DevBuf<unsigned long long> d_sig;
    DevBuf<uint32_t> d_occ_off, d_occ, d_sub;
    d_lits.upload(F.nl, s.stream);
    d_offs.upload(F.no, s.stream);
    d_sig.upload(sig, s.stream);
    d_occ_off.upload(occ_off, s.stream);
    d_occ.upload(occ, s.stream);
    d_sub.alloc(nn);
    d_drop.alloc(nn);
    HIPCHK(hipMemsetAsync(d_sub.p, 0, 4 * nn, s.stream));
    HIPCHK(hipMemsetAsync(d_drop.p, 0xff, 4 * nn, s.stream));
    hipLaunchKernelGGL(ms_subsume_kernel, dim3((uint32_t)((nn + 255) / 256)), dim3(256), 0, s.stream, (uint32_t)nn, d_lits.p, d_offs.p,
                       d_sig.p, d_occ_off.p, d_occ.p, 64u, d_sub.p, d_drop.p);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> sub(nn);
    std::vector<int32_t> drop(nn);
    HIPCHK(hipMemcpyAsync(sub.data(), d_sub.p, 4 * nn, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(drop.data(), d_drop.p, 4 * nn, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    uint64_t n = 0;
    std::vector<int32_t> nl2, tmp;
    std::vector<uint64_t> no2{0};
    nl2.reserve(F.nl.size());
    for (size_t c = 0; c < nn && !F.unsat; c++) {
        if (sub[c]) { F.n_subsumed++; n++; continue; }
        tmp.assign(F.nl.begin() + F.no[c], F.nl.begin() + F.no[c + 1]);
        if (drop[c] >= 0) {
            tmp.erase(std::remove(tmp.begin(), tmp.end(), drop[c]), tmp.end());
            F.lemma(tmp);
            F.n_strengthened++;
            n++;
            if (!normal_clause(F, tmp)) continue;
        }
        nl2.insert(nl2.end(), tmp.begin(), tmp.end());
        no2.push_back(nl2.size());
    }
    F.nl.swap(nl2);
    F.no.swap(no2);
    return n;
}

inline bool bve_enabled(const mi355sat& s) { return s.opts.simp == 2; }

// Bounded variable elimination - `SimpSolver::eliminate` of the reference's backend ([ext] Een & Biere 2005, MiniSat's
// limits: no more clauses than before (grow = 0), no resolvent longer than 20 literals).  A variable x that is not
// frozen (assumptions are) is resolved away: every clause with x against every clause with ~x, tautologies dropped;
// if that does not make the formula larger, the resolvents replace the clauses of x.  The clauses of the smaller side
// are kept aside (F.elims): in reverse elimination order they give x its value in a model of the rest
// (`extendModel`).  Host code: occurrence lists and a cost-ordered queue, a few 10 ms on these formulas; every
// resolvent is a RUP lemma of the proof.
uint64_t bve_eliminate(Formula& F) {
    if (F.unsat || F.n_clauses() == 0) return 0;
    const uint32_t nv = F.nv;
    const int CLAUSE_LIM = 20, OCC_LIM = 400;
    std::vector<uint8_t> frozen(nv, 0), gone(nv, 0);
    for (int32_t l : F.frozen_lits) {
        while (F.subst[l >> 1] != 2 * (l >> 1)) l = F.subst[l >> 1] ^ (l & 1);
        frozen[l >> 1] = 1;
    }
    std::vector<int32_t>& nl = F.nl;
    std::vector<uint64_t>& no = F.no;
    std::vector<uint8_t> alive(F.n_clauses(), 1);
    std::vector<std::vector<uint32_t>> occ(2 * (size_t)nv);
    std::vector<uint32_t> n_occ(2 * (size_t)nv, 0);
    for (size_t c = 0; c < F.n_clauses(); c++)
        for (uint64_t k = no[c]; k < no[c + 1]; k++) { occ[nl[k]].push_back((uint32_t)c); n_occ[nl[k]]++; }
    auto cost = [&](uint32_t v) { return (uint64_t)n_occ[2 * v] * n_occ[2 * v + 1]; };
    typedef std::pair<uint64_t, uint32_t> QE;
    std::priority_queue<QE, std::vector<QE>, std::greater<QE>> heap;
    for (uint32_t v = 0; v < nv; v++)
        if (!frozen[v] && !F.val[v] && (n_occ[2 * v] || n_occ[2 * v + 1])) heap.push({cost(v), v});
    std::vector<uint32_t> stamp(2 * (size_t)nv, 0);
    uint32_t epoch = 0;
    std::vector<uint32_t> P, N;
    std::vector<int32_t> res;
    uint64_t n_elim = 0;
    auto kill = [&](uint32_t c) {
        alive[c] = 0;
        for (uint64_t k = no[c]; k < no[c + 1]; k++) {
            const int32_t l = nl[k];
            n_occ[l]--;
            const uint32_t u = (uint32_t)(l >> 1);
            if (!frozen[u] && !gone[u] && !F.val[u]) heap.push({cost(u), u});
        }
    };
    while (!heap.empty() && !F.unsat) {
        const QE top = heap.top();
        heap.pop();
        const uint32_t v = top.second;
        if (gone[v] || F.val[v] || top.first != cost(v)) continue;     // stale entry (a fresher one is in the queue)
        const int32_t x = 2 * (int32_t)v, nx = x + 1;
        if (n_occ[x] + n_occ[nx] == 0) continue;
        if (n_occ[x] > (uint32_t)OCC_LIM || n_occ[nx] > (uint32_t)OCC_LIM || top.first > 4096) continue;
        P.clear();
        N.clear();
        for (uint32_t c : occ[x]) if (alive[c]) P.push_back(c);
        for (uint32_t c : occ[nx]) if (alive[c]) N.push_back(c);
        occ[x] = P;
        occ[nx] = N;
        // count the non-tautological resolvents
        size_t cnt = 0;
        bool ok = true;
        for (size_t i = 0; i < P.size() && ok; i++) {
            epoch++;
            const uint32_t c = P[i];
            const int clen = (int)(no[c + 1] - no[c]);
            for (uint64_t k = no[c]; k < no[c + 1]; k++) stamp[nl[k]] = epoch;
            for (size_t j = 0; j < N.size() && ok; j++) {
                const uint32_t d = N[j];
                int extra = 0;
                bool taut = false;
                for (uint64_t k = no[d]; k < no[d + 1] && !taut; k++) {
                    const int32_t l = nl[k];
                    if (l == nx) continue;
                    if (stamp[l ^ 1] == epoch) taut = true;
                    else if (stamp[l] != epoch) extra++;
                }
                if (taut) continue;
                if (++cnt > P.size() + N.size() || clen - 1 + extra > CLAUSE_LIM) ok = false;
            }
        }
        if (!ok) continue;
        // eliminate: keep the smaller side for the model, add the resolvents, drop both sides
        {
            const bool pos_side = P.size() <= N.size();
            const std::vector<uint32_t>& side = pos_side ? P : N;
            MsElim e{pos_side ? x : nx, (uint32_t)F.elim_lits.size(), 0};
            for (uint32_t c : side) {
                F.elim_lits.insert(F.elim_lits.end(), nl.begin() + no[c], nl.begin() + no[c + 1]);
                F.elim_lits.push_back(-1);
            }
            e.end = (uint32_t)F.elim_lits.size();
            F.elims.push_back(e);
        }
        gone[v] = 1;
        for (size_t i = 0; i < P.size() && !F.unsat; i++)
            for (size_t j = 0; j < N.size() && !F.unsat; j++) {
                const uint32_t c = P[i], d = N[j];
                res.clear();
                for (uint64_t k = no[c]; k < no[c + 1]; k++) if (nl[k] != x) res.push_back(nl[k]);
                for (uint64_t k = no[d]; k < no[d + 1]; k++) if (nl[k] != nx) res.push_back(nl[k]);
                std::sort(res.begin(), res.end());
                res.erase(std::unique(res.begin(), res.end()), res.end());
                bool taut = false;
                for (size_t q = 0; q + 1 < res.size(); q++) taut = taut || (res[q] ^ 1) == res[q + 1];
                if (taut) continue;
                F.lemma(res);
                if (res.size() <= 1) {
                    if (res.empty() || !F.assign_unit(res[0])) F.unsat = true;
                    continue;
                }
                const uint32_t id = (uint32_t)F.n_clauses();
                nl.insert(nl.end(), res.begin(), res.end());
                no.push_back(nl.size());
                alive.push_back(1);
                for (int32_t l : res) { occ[l].push_back(id); n_occ[l]++; }
            }
        for (uint32_t c : P) kill(c);
        for (uint32_t c : N) kill(c);
        n_elim++;
    }
    if (!n_elim) return 0;
    F.n_eliminated += n_elim;
    std::vector<int32_t> nl2;
    std::vector<uint64_t> no2{0};
    nl2.reserve(nl.size());
    for (size_t c = 0; c < F.n_clauses(); c++) {
        if (!alive[c]) continue;
        nl2.insert(nl2.end(), nl.begin() + no[c], nl.begin() + no[c + 1]);
        no2.push_back(nl2.size());
    }
    F.nl.swap(nl2);
    F.no.swap(no2);
    return n_elim;
}

// The values of the eliminated variables in a model of the remaining formula (MiniSat's extendModel): last eliminated
// first; x is false unless one of its kept clauses has every other literal false.  model: 1 true / -1 false per variable.
void extend_model(const std::vector<MsElim>& elims, const std::vector<int32_t>& elim_lits, std::vector<int8_t>& model) {
    for (size_t i = elims.size(); i-- > 0;) {
        const MsElim& e = elims[i];
        const size_t v = (size_t)(e.x >> 1);
        if (v >= model.size()) continue;
        bool need = false;
        for (uint32_t k = e.begin; k < e.end && !need;) {
            bool others_false = true;
            for (; elim_lits[k] >= 0; k++) {
                const int32_t l = elim_lits[k];
                if (l == e.x || (size_t)(l >> 1) >= model.size()) continue;
                const int8_t m = model[l >> 1];
                if (((l & 1) ? -m : m) > 0) others_false = false;
            }
            k++;
            need = others_false;
        }
        model[v] = (int8_t)(((e.x & 1) != 0) == need ? -1 : 1);
    }
}

// The whole pipeline: units, then rounds of {equivalent literals, probing} while they find something, then
// subsumption, then variable elimination (and subsumption among its resolvents).  Everything it derives is a
// consequence of the caller's formula alone (never of assumptions); the assumptions' variables are not eliminated.
void simplify_formula(mi355sat& s, Formula& F) {
    propagate_units(F);
    if (s.opts.simp < 0 || F.unsat) return;
    const double t0 = now_s();
    const size_t c0 = F.n_clauses(), l0 = F.nl.size(), u0 = F.units.size();
    double t_els = 0, t_probe = 0, t_sub = 0;
    for (int round = 0; round < 3 && !F.unsat; round++) {
        double ta = now_s();
        uint64_t n = els_scc(F);
        propagate_units(F);
        t_els += now_s() - ta;
        ta = now_s();
        n += device_probe(s, F);
        propagate_units(F);
        t_probe += now_s() - ta;
        if (!n) break;
    }
    for (int pass = 0; pass < 3 && !F.unsat; pass++) {
        const double ta = now_s();
        const uint64_t n = device_subsume(s, F);
        propagate_units(F);
        t_sub += now_s() - ta;
        if (!n) break;
    }
    if (s.opts.verbose)
        fprintf(stderr, "[mi355sat] simplification stages: equivalent literals %.3f s, probing %.3f s, subsumption %.3f s\n", t_els, t_probe, t_sub);
    const double t1 = now_s();
    if (bve_enabled(s) && !F.unsat && bve_eliminate(F)) {
        propagate_units(F);
        for (int pass = 0; pass < 2 && !F.unsat; pass++) {
            const uint64_t n = device_subsume(s, F);
            propagate_units(F);
            if (!n) break;
        }
    }
    if (s.opts.verbose && bve_enabled(s))
        fprintf(stderr, "[mi355sat] variable elimination %.3f s: %llu variables\n", now_s() - t1, (unsigned long long)F.n_eliminated);
    if (s.opts.verbose)
        fprintf(stderr, "[mi355sat] simplification %.3f s: clauses %zu -> %zu, literals %zu -> %zu, units +%zu (failed literals %llu, necessary %llu), "
                "equivalent variables %llu, subsumed %llu, strengthened %llu%s\n", now_s() - t0, c0, F.n_clauses(), l0, F.nl.size(),
                F.units.size() - u0, (unsigned long long)F.n_failed, (unsigned long long)F.n_necessary, (unsigned long long)F.n_equiv,
                (unsigned long long)F.n_subsumed, (unsigned long long)F.n_strengthened, F.unsat ? " - UNSAT" : "");
}

// Test hook (mi355sat_debug_keep_simplified): the formula as simplify_formula left it, in the caller's variables - the
// remaining clauses, every level-0 fact as a one-literal clause, both binary clauses of every substitution (the empty
// clause if the simplification refuted the formula); and the clauses kept aside for the eliminated variables.
void keep_simplified_copy(mi355sat& s, const Formula& F) {
    auto dimacs = [](int32_t l) { return (l & 1) ? -((l >> 1) + 1) : ((l >> 1) + 1); };
    for (int k = 0; k < 2; k++) { s.kept[k].clear(); s.kept_n[k] = 0; }
    std::vector<int32_t>& out = s.kept[0];
    for (size_t c = 0; c < F.n_clauses(); c++) {
        for (uint64_t k = F.no[c]; k < F.no[c + 1]; k++) out.push_back(dimacs(F.nl[k]));
        out.push_back(0);
    }
    s.kept_n[0] = F.n_clauses();
    for (int32_t u : F.units) { out.push_back(dimacs(u)); out.push_back(0); s.kept_n[0]++; }
    for (uint32_t v = 0; v < F.nv; v++) {
        const int32_t r = F.subst[v];
        if (r == 2 * (int32_t)v) continue;
        out.insert(out.end(), {-(int32_t)(v + 1), dimacs(r), 0, (int32_t)(v + 1), dimacs(r ^ 1), 0});
        s.kept_n[0] += 2;
    }
    if (F.unsat) { out.push_back(0); s.kept_n[0]++; }
    for (int32_t l : F.elim_lits) {
        s.kept[1].push_back(l < 0 ? 0 : dimacs(l));
        if (l < 0) s.kept_n[1]++;
    }
    s.kept_valid = true;
}

// The members of MsState that are running counters - a worker only ever adds to them, from the template on - as pairs
// (a's, b's): the one list behind summing them over workers and taking a warm solve's share of them.  A counter added to
// MsState goes here.
template <class A, class B, class Op>
void for_each_counter(A& a, B& b, Op op) {
    op(a.n_steps, b.n_steps); op(a.n_redo, b.n_redo);
    op(a.propagations, b.propagations); op(a.decisions, b.decisions); op(a.conflicts, b.conflicts); op(a.restarts, b.restarts);
    op(a.reduce_dbs, b.reduce_dbs); op(a.n_watch, b.n_watch); op(a.n_cl_lit, b.n_cl_lit); op(a.n_move, b.n_move); op(a.n_enq, b.n_enq);
    op(a.n_exported, b.n_exported); op(a.n_imported, b.n_imported); op(a.n_imported_units, b.n_imported_units);
    op(a.slice_cycles, b.slice_cycles); op(a.learnt_total, b.learnt_total); op(a.learnt_lits_total, b.learnt_lits_total);
    op(a.n_vivified, b.n_vivified); op(a.n_viv_lits, b.n_viv_lits); op(a.n_rephase, b.n_rephase);
    op(a.n_import_skipped, b.n_import_skipped); op(a.n_forced_imports, b.n_forced_imports);
    op(a.n_pressure_reduces, b.n_pressure_reduces); op(a.n_pool_rebuilds, b.n_pool_rebuilds); op(a.n_imports_dropped_full, b.n_imports_dropped_full);
    for (int i = 0; i < 16; i++) op(a.prof[i], b.prof[i]);
}

// Adds the workers' counters to the handle's stats.  bcp_times (mi355sat_propagate_batch with `repeat`): sts are the
// counters of one run of that many identical ones, and the BCP traffic counters stand for all of them.
void accumulate_stats(mi355sat& s, const std::vector<MsState>& sts, uint64_t bcp_times = 1) {
    mi355sat_stats_t& o = s.stats;
    MsState t{};                 // the counters summed over the workers
    uint64_t learnts = 0, llits = 0;
    for (auto& st : sts) {
        for_each_counter(t, st, [](auto& sum, const auto& x) { sum += x; });
        learnts += st.n_learnts; llits += st.lc_lits_n;
    }
    o.propagations += t.propagations * bcp_times; o.n_deq += t.propagations * bcp_times; o.n_watch += t.n_watch * bcp_times;
    o.n_cl_lit += t.n_cl_lit * bcp_times; o.n_move += t.n_move * bcp_times; o.n_enq += t.n_enq * bcp_times;
    o.decisions += t.decisions; o.conflicts += t.conflicts; o.restarts += t.restarts; o.reduce_dbs += t.reduce_dbs;
    o.learnts = learnts; o.learnt_literals = llits;
    o.bcp_steps += t.n_steps; o.bcp_requeued += t.n_redo;
    o.shared_exported += t.n_exported; o.shared_imported += t.n_imported; o.shared_imported_units += t.n_imported_units;
    s.heur = mi355sat_heuristics_info{};
    s.heur.n_vivified = t.n_vivified; s.heur.n_viv_lits = t.n_viv_lits; s.heur.n_rephase = t.n_rephase;
    s.heur.import_skipped = t.n_import_skipped; s.heur.forced_imports = t.n_forced_imports;
    s.cap_events[0] = t.n_pressure_reduces; s.cap_events[1] = t.n_pool_rebuilds; s.cap_events[2] = t.n_imports_dropped_full;
    const uint64_t* prof = t.prof;
    const uint64_t cyc = t.slice_cycles;
    if (prof[0] && s.opts.verbose) {
        static const char* nm[] = {"offsets", "binary", "ternary", "long", "close", "analyze", "backjump+learn", "decide", "reduce"};
        fprintf(stderr, "[mi355sat] phase cycle shares of %.3e worker-cycles:", (double)cyc);
        for (int i = 0; i < 9; i++) fprintf(stderr, " %s=%.1f%%", nm[i], 100.0 * (double)prof[i] / (double)cyc);
        const uint64_t confl = t.conflicts;
        fprintf(stderr, "; resolution steps per conflict %.1f, learnt clause %.1f literals", (double)prof[9] / (double)std::max<uint64_t>(1, confl),
                (double)t.learnt_lits_total / (double)std::max<uint64_t>(1, t.learnt_total));
        fprintf(stderr, "; of analyze: recursive minimisation %.1f%%, local %.1f%%; %.1f nodes per call, %.2f calls per conflict\n",
                100.0 * (double)prof[10] / (double)cyc, 100.0 * (double)prof[11] / (double)cyc,
                (double)prof[12] / (double)std::max<uint64_t>(1, prof[13]), (double)prof[13] / (double)std::max<uint64_t>(1, confl));
    }
}


void fetch_model(mi355sat& s, uint32_t worker, std::vector<int8_t>& out, uint64_t n_vars_out) {
    std::vector<uint8_t> asg((size_t)s.n_vars + 1);
    if (s.n_vars)
        HIPCHK(hipMemcpy(asg.data(), s.d_slabs.p + (size_t)worker * s.L.slab_bytes + s.L.val, s.n_vars, hipMemcpyDeviceToHost));
    // the device's values, then the eliminated variables (their kept clauses mention device variables and variables
    // eliminated later only), then the variables replaced by an equivalent literal (representatives have smaller indices)
    std::vector<int8_t> m(s.n_vars, 0);
    for (uint64_t v = 0; v < s.n_vars; v++) m[v] = asg[s.perm[v]] == MS_ASG_TRUE ? 1 : -1;  // (a variable left free would read false)
    extend_model(s.elims, s.elim_lits, m);
    for (uint64_t v = 0; v < s.n_vars; v++) {
        const int32_t r = v < s.subst.size() ? s.subst[v] : 2 * (int32_t)v;
        if (r != 2 * (int32_t)v && (uint64_t)(r >> 1) < v) m[v] = (r & 1) ? (int8_t)-m[r >> 1] : m[r >> 1];
    }
    out.assign(n_vars_out, 0);
    for (uint64_t v = 0; v < n_vars_out && v < s.n_vars; v++) out[v] = m[v];
}

struct SliceResult { float ms; };

// Which build a launch of `active` workers runs, and with how much dynamic LDS: the one place that decides it (launch_slice
// follows it; mi355sat_debug_search_build_rule evaluates it without a launch).  mode 0 = search, else BCP / probing
// (wps 0: those kernels have one build per LDS variant).
//   lds: assignment (2 bits / variable) and analysis marks (1 bit) in LDS when this launch's workers per CU leave room
//        (160 KB per CU, 150 KB of it budgeted; a workgroup's static LDS aside: 5.2 KB, 13.2 KB in the builds with the sort
//        buffer): 16 workers per CU -> 3.4 KB each, one per CU -> up to 64 KB, which covers rect 64x64.  State is written
//        back to HBM at every slice end, so consecutive launches may differ.  The budget is SIGNED: above 25 workers per CU
//        the reserve exceeds the share and nothing is staged.
//   wps: the build compiled for the launch's waves per SIMD: 1 (<= 1024 workers: the SIMD's whole register file, everything
//        inlined), 2 (<= 2048: no spills either), else the full fleet's.
inline mi355sat_search_build choose_build(uint32_t active, uint32_t lds_val_bytes, bool staged, int opt_lds_val, int opt_one_per_simd, int mode) {
    mi355sat_search_build b{};
    b.active = active;
    b.lds_val_bytes = lds_val_bytes;
    bool lds = staged;
    if (mode == 0 && opt_lds_val == 0) {
        const int64_t per_cu = ((int64_t)active + 255) / 256;
        const int64_t budget = std::max<int64_t>(0, std::min<int64_t>(64 * 1024, 150 * 1024 / per_cu - (per_cu <= 8 ? 14 : 6) * 1024));
        lds = (int64_t)lds_val_bytes <= budget;
    }
    b.lds = lds ? 1 : 0;
    b.dyn_lds_bytes = lds ? lds_val_bytes : 0;
    if (mode == 0) {
        int wps = opt_one_per_simd < 0 ? MS_SEARCH_WAVES_PER_SIMD : (active <= 1024 ? 1 : (active <= 2048 ? 2 : MS_SEARCH_WAVES_PER_SIMD));
        if (opt_one_per_simd == 2 || opt_one_per_simd == 4) wps = std::max(wps, opt_one_per_simd == 2 ? 2 : MS_SEARCH_WAVES_PER_SIMD);   // (A/B: a build for more waves)
        b.wps = wps;
    }
    return b;
}

// One timed kernel launch on the stream: `launch` between two events, its error checked, the time between the events added
// to stats.kernel_seconds, stats.kernel_launches counted.  `after` is queued behind the second event and ahead of the wait:
// what it launches is not measured.
template <class Launch, class After>
SliceResult timed_launch(mi355sat& s, Launch launch, After after) {
    HIPCHK(hipEventRecord(s.ev0, s.stream));
    launch();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev1, s.stream));
    after();
    HIPCHK(hipEventSynchronize(s.ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
    s.stats.kernel_seconds += ms * 1e-3;
    s.stats.kernel_launches++;
    return SliceResult{ms};
}

// A flag known at run time as a template argument of a launch: f(std::true_type) or f(std::false_type).
template <class F>
void with_flag(bool flag, F f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

SliceResult launch_slice(mi355sat& s, int mode, bool stop_on_any, bool done_on_refuted = true, uint32_t active = 0, int auto_slice_ms = 20) {
    if (active == 0 || active > s.n_alloc) active = s.n_alloc;   // workers [0, active) run this slice
    MsParams prm{};
    prm.n_workers = active;
    const bool deterministic = s.opts.deterministic > 0;
    prm.slice_conflicts = s.opts.slice_conflicts > 0 ? (uint32_t)s.opts.slice_conflicts : (deterministic ? 200u : 0xffffffffu);
    prm.slice_props = 0;
    // default: time-bounded slices (all workers stop together; no straggler tail), 20 ms
    const int slice_ms = deterministic ? 0 : (s.opts.slice_ms > 0 ? s.opts.slice_ms : (s.opts.slice_conflicts > 0 ? 0 : auto_slice_ms));
    prm.slice_ticks = slice_ms > 0 ? (uint64_t)slice_ms * 100000ull : 0;
    prm.stop_flag = s.stop_flag;
    prm.stop_on_any = stop_on_any && !deterministic ? 1 : 0;
    prm.max_groups = s.opts.max_groups > 0 ? s.opts.max_groups : MS_MAX_GROUPS;
    prm.any_done = s.d_any_done.p;
    prm.done_on_refuted = done_on_refuted ? 1 : 0;
    prm.proof_buf = s.d_proof.p;
    prm.proof_len = s.d_proof_len.p;
    prm.proof_cap = s.proof_cap;
    prm.reduce_first = s.opts.reduce_first > 0 ? (uint32_t)s.opts.reduce_first : 2000u;
    prm.reduce_inc = s.opts.reduce_inc > 0 ? (uint32_t)s.opts.reduce_inc : 300u;
    prm.rephase = s.opts.rephase;
    prm.restart_k_pct = s.opts.restart_k_pct;
    prm.restart_k2_pct = s.opts.restart_k2_pct;
    prm.import_pct = s.opts.import_pct;
    prm.vivify = s.opts.vivify;
    prm.sched = s.vivify_every | (s.rephase_every << 16);
    const bool share = mode == 0 && s.share_slots != 0;
    const uint32_t share_intake_cap = (uint32_t)std::max(16, slice_ms > 0 ? 16 * slice_ms : 256);   // 16 clauses per ms of slice
    if (share) {
        prm.share_pool = s.d_share_pool.p;
        prm.share_n = s.d_share_n.p;
        prm.share_slots = s.share_slots;
        prm.share_max_lbd = s.opts.share_lbd > 0 ? (uint32_t)s.opts.share_lbd : 4u;
        prm.share_max_len = s.opts.share_len > 0 ? (uint32_t)s.opts.share_len : (uint32_t)MS_SHARE_MAXLEN;
        prm.share_interval = s.opts.share_interval > 0 ? (uint32_t)s.opts.share_interval : 0xffffffffu;
    }
    const mi355sat_search_build build = choose_build(active, s.lds_val_bytes, s.lds_val, s.opts.lds_val, s.opts.one_per_simd, mode);
    const bool lds = build.lds != 0;
    const int wps = build.wps;
    return timed_launch(s, [&] {
        if (mode == 0) {
            const uint64_t n_launches = s.last_build.launches;
            const uint32_t seen = s.last_build.builds_seen;
            s.last_build = build;
            s.last_build.launches = n_launches + 1;
            s.last_build.builds_seen = seen | (1u << ((lds ? 3 : 0) + (wps == 1 ? 0 : (wps == 2 ? 1 : 2))));
        }
        with_flag(lds, [&](auto lds_build) {      // (dyn_lds_bytes is 0 in the builds without the assignment in LDS)
            constexpr bool LV = decltype(lds_build)::value;
#define MS_LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(active), dim3(MS_WAVE), build.dyn_lds_bytes, s.stream, s.sh, s.L, s.d_slabs.p, prm)
            if (mode == 2) MS_LAUNCH(ms_probe_kernel<LV>);
            else if (mode != 0) MS_LAUNCH(ms_bcp_kernel<LV>);
            else if (wps == 1) MS_LAUNCH(ms_search_kernel<LV, 1>);
            else if (wps == 2) MS_LAUNCH(ms_search_kernel<LV, 2>);
            else MS_LAUNCH(ms_search_kernel<LV, MS_SEARCH_WAVES_PER_SIMD>);
#undef MS_LAUNCH
        });
    }, [&] {
        if (!share) return;      // the slice's exported clauses into the ring, behind the measured launch
        if ((++s.share_slices & 255) == 0)   // forget old signatures before the set fills up (a clause may then be passed on twice)
            HIPCHK(hipMemsetAsync(s.d_share_hash.p, 0, sizeof(unsigned long long) * s.share_hash_n, s.stream));
        HIPCHK(hipMemsetAsync(s.d_share_intake.p, 0, sizeof(uint32_t), s.stream));
        const bool ordered = s.opts.deterministic > 0;
        hipLaunchKernelGGL(ms_share_collect_kernel, dim3(ordered ? 1 : (s.n_alloc + 63) / 64), dim3(ordered ? 1 : 64), 0, s.stream, s.L, s.d_slabs.p,
                           s.n_alloc, s.d_share_pool.p, s.share_slots, s.d_share_n.p, s.d_share_hash.p, s.share_hash_n - 1,
                           s.d_share_intake.p, share_intake_cap, ordered ? 1 : 0);
        HIPCHK(hipGetLastError());
    });
}

void launch_probe(mi355sat& s) { launch_slice(s, 2, false); }

// DRUP text (DIMACS literals, one lemma per line).  Order: what the simplification derived, then after every
// slice the clauses each worker learnt in it (worker by worker, each in its own derivation order), finally the empty
// clause.  That order makes every line a RUP consequence of the lines before it: a learnt clause depends on its
// worker's earlier clauses and on exchanged clauses, and the exchange only hands on clauses of EARLIER slices.
// A batch or a sweep writes one such file for all its instances: the lemmas of all workers of all instances are one
// derivation from the caller's formula (assumptions are decisions, so a learnt clause follows from the formula alone), and
// behind the lemmas of a slice stands, for every instance that slice decided UNSAT, the clause of its negated core
// (proof_core_lines).
void proof_open(mi355sat& s) {
    if (s.proof_file) fclose(s.proof_file);      // (a sweep begun over a running one)
    s.proof_file = fopen(s.proof_path.c_str(), "w");
    if (!s.proof_file) throw HipErr{"cannot open proof file " + s.proof_path};
    s.proof_empty = false;
    s.proof_log = mi355sat_proof_log_info{};
    bool line_start = true;
    for (int32_t l : s.simp_proof) {   // (caller's numbering already)
        if (l < 0) { fputs("0\n", s.proof_file); s.proof_empty = s.proof_empty || line_start; }
        else fprintf(s.proof_file, "%d ", to_dimacs(l));
        line_start = l < 0;
    }
}
// After a slice: the 2 * W lengths, the overflow rule, then ONE kernel (ms_proof_gather_kernel: a wavefront per non-empty
// log packs its lemma words and its deletion words, rewritten to the caller's literals) and ONE copy; the host only
// formats text.  The order in the file is the order of the packed buffer: worker by worker, lemmas then deletion lines.
void proof_drain(mi355sat& s) {
    if (!s.proof_file || !s.d_proof_len.p) return;
    struct Timed {       // (mi355sat_debug_proof_log: the wall time of the drains, whichever way one ends)
        mi355sat_proof_log_info& info;
        double t0 = now_s();
        ~Timed() { info.drains++; info.drain_seconds += now_s() - t0; }
    } timed{s.proof_log};
    const uint32_t W = (uint32_t)(s.d_proof_len.n / 2);     // per worker: lemma words from word 0 up, deletion words from the top down
    std::vector<uint32_t> len(2 * (size_t)W), jobs;
    HIPCHK(hipMemcpy(len.data(), s.d_proof_len.p, sizeof(uint32_t) * 2 * W, hipMemcpyDeviceToHost));
    uint64_t total = 0;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t n_lem = len[2 * w], n_del = len[2 * w + 1];
        if (!n_lem && !n_del) continue;
        if (n_lem > s.proof_cap || n_del > s.proof_cap - n_lem)
            throw HipErr{"proof buffer overflow (a worker learnt more in one slice than its log holds)", MI355SAT_ERR_OOM};
        jobs.insert(jobs.end(), {w, n_lem, n_del, (uint32_t)total});
        total += (uint64_t)n_lem + n_del;
        if (total > 0xffffffffull) throw HipErr{"proof buffer overflow (one slice's logs exceed 2^32 words)", MI355SAT_ERR_OOM};
    }
    if (jobs.empty()) return;
    if (s.d_proof_jobs.n < jobs.size()) s.d_proof_jobs.alloc(jobs.size() + jobs.size() / 2);
    if (s.d_proof_out.n < total) s.d_proof_out.alloc((size_t)(total + total / 2));
    HIPCHK(hipMemcpyAsync(s.d_proof_jobs.p, jobs.data(), sizeof(uint32_t) * jobs.size(), hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(ms_proof_gather_kernel, dim3((uint32_t)(jobs.size() / 4)), dim3(MS_WAVE), 0, s.stream, (const int32_t*)s.d_proof.p,
                       s.proof_cap, (const uint32_t*)s.d_proof_jobs.p, (const uint32_t*)s.d_proof_inv.p, (uint32_t)s.d_proof_inv.n, s.d_proof_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(s.d_proof_len.p, 0, sizeof(uint32_t) * 2 * W, s.stream));
    std::vector<int32_t> buf((size_t)total);
    HIPCHK(hipMemcpyAsync(buf.data(), s.d_proof_out.p, sizeof(int32_t) * buf.size(), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    std::string text;
    text.reserve(buf.size() * 7);
    char num[16];
    for (int32_t x : buf) {
        if (x == MS_PROOF_BAD) throw HipErr{"device solver internal error (a proof log holds a literal out of range)"};
        if (x == -2) text += "d ";             // deletion line
        else if (x < 0) text += "0\n";
        else { text.append(num, (size_t)snprintf(num, sizeof num, "%d ", to_dimacs(x))); }
    }
    fwrite(text.data(), 1, text.size(), s.proof_file);
    s.proof_log.gathers++;
    s.proof_log.logs += jobs.size() / 4;
    s.proof_log.words += total;
}
// An UNSAT answer ends the proof with the clause of the negated core: under assumptions, what the formula implies about
// them; without any (or when the formula itself is refuted), the empty clause.
void proof_close(mi355sat& s, bool unsat, const std::vector<int32_t>& core = {}) {
    if (!s.proof_file) return;
    if (unsat) {
        for (int32_t l : core) fprintf(s.proof_file, "%d ", -l);
        fputs("0\n", s.proof_file);
    }
    fclose(s.proof_file);
    s.proof_file = nullptr;
}

const char* status_text(int st) {
    switch (st) {
        case MS_ST_ERR_POOL: return "device watch pool exhausted";
        case MS_ST_ERR_LEARNT: return "device learnt-clause store exhausted";
        case MS_ST_ERR_INTERNAL: return "device solver internal error";
        default: return "unknown device status";
    }
}

// A worker's negative status as its call's failure: the text in s.err, the code `internal` (each caller's own) for
// MS_ST_ERR_INTERNAL and MI355SAT_ERR_OOM for a full store.  (warm_begin answers a full store with a cold start: not here.)
int status_error(mi355sat& s, int st, int internal, const char* prefix = "") {
    s.err = std::string(prefix) + status_text(st);
    return st == MS_ST_ERR_INTERNAL ? internal : MI355SAT_ERR_OOM;
}

// The worker whose slab is the model of instance `inst` - it keeps that slab until the caller has read it - or -1.
inline int32_t model_holder(const std::vector<int32_t>& results, const std::vector<int32_t>& winner, uint64_t inst) {
    return results[inst] == MI355SAT_SAT ? winner[inst] : -1;
}

struct Sweep;

// What the host tells workers between two slices, for ms_assign_kernel to apply: a new status, a restart request and a
// new assumption list (the worker's cube) each.  Queued by Sweep::assign / park, which keep the host's side of it.
struct WorkerUpdates {
    std::vector<int32_t> upd, data;
    // The record as ms_assign_kernel reads it, five words: worker, status, restart request, the length of its assumption
    // list and where that starts in the launch's data buffer.
    void add_at(uint32_t w, int32_t status, int32_t restart, size_t n, size_t at) {
        upd.insert(upd.end(), {(int32_t)w, status, restart, (int32_t)n, (int32_t)at});
    }
    void add(uint32_t w, int32_t status, int32_t restart, const std::vector<int32_t>& cube) {   // the list travels in `data`
        add_at(w, status, restart, cube.size(), data.size());
        data.insert(data.end(), cube.begin(), cube.end());
    }
    void send(mi355sat& s, Sweep& sw, const int32_t* resident = nullptr);
};

// Shared driver for solve(), solve_batch() and the stepwise sweep API.
// Worker w starts on instance w % n_instances; workers of decided (or withdrawn) instances move on
// to the open ones (w_inst).  DESIGN.md §5 has the states of an instance and of a worker and who moves them.
struct Sweep {
    uint32_t n_instances = 0;
    std::vector<int32_t> results, winner;
    std::vector<uint8_t> dropped;                // withdrawn by the caller: result stays INTERRUPTED, counts as decided
    std::vector<double> weights;                 // share of the fleet each open instance should get (empty: equal)
    bool weights_dirty = false;
    std::vector<int32_t> base_assump;            // internal literals
    std::vector<uint64_t> base_off;
    uint64_t n_moved = 0;
    float ramp_ms = 0;                           // kernel time of this sweep so far
    uint32_t decided = 0;                        // instances that are not open
    bool formula_unsat = false;                  // a worker refuted the formula itself: whatever is reopened is UNSAT too
    bool stop_at_first = false;
    bool active = false;
    std::vector<MsState> sts;
    uint64_t conflicts = 0;
    // cube scheduler (opts.cube_split): every busy worker owns one cube = its instance's base
    // assumptions + split literals; the cubes of an instance partition its search space
    bool split = false;
    std::vector<int32_t> w_inst;
    std::vector<std::vector<int32_t>> w_cube;   // internal literals
    std::vector<uint8_t> w_busy;
    std::vector<uint64_t> w_conf0;               // worker's conflict count when it got its cube
    std::vector<uint32_t> open;                  // per instance: its busy workers (with splitting: its open cubes)
    uint64_t n_splits = 0, n_closed = 0;
    DevBuf<int32_t> d_upd, d_data;
    // failed-assumption cores (solve(), solve_batch(), and the public sweep API while it logs a proof - without one it
    // launches nothing for them): per instance, one flag per entry of the caller's assumption list
    bool cores = false;
    std::vector<uint32_t> base_src;              // per entry of base_assump: its index in the caller's list of the instance
    std::vector<std::vector<uint8_t>> core_flag;
    // a batch or a sweep that logs a proof (sweep_begin): the caller's lists, and per instance "its core line is written"
    bool log_cores = false;
    std::vector<int32_t> caller_assump;
    std::vector<uint64_t> caller_off;
    std::vector<uint8_t> core_logged;
    std::vector<int32_t> core_of(uint32_t inst) const {      // (log_cores) the caller's literals an UNSAT verdict rests on
        std::vector<int32_t> c;
        for (uint64_t k = 0; k < core_flag[inst].size(); k++)
            if (core_flag[inst][k]) c.push_back(caller_assump[caller_off[inst] + k]);
        return c;
    }
    DevBuf<int32_t> d_fw, d_fok;
    DevBuf<uint32_t> d_fout, d_fscratch;
    DevBuf<int32_t> d_qlits;                     // core minimisation: what ms_core_model_kernel looks up (core_models)
    DevBuf<uint32_t> d_qoff;
    // warm incremental solve: a plain solve() that may leave its workers to the next one (a cold start) or took them over
    // from the one before (a warm start: their counters run on from counters0, conflicts0 = those conflicts summed)
    bool keep_warm = false;
    std::vector<MsState> counters0;
    uint64_t conflicts0 = 0;

    // ---- an instance: open, withdrawn, SAT or UNSAT.  Only pose / decide / withdraw / reopen / reset write results, winner,
    // dropped and decided.
    bool is_open(uint32_t inst) const { return results[inst] == MI355SAT_INTERRUPTED && !dropped[inst]; }
    // Posed (anew): open, no verdict, an empty core over its n_assumps entries of the caller's list.
    void pose(uint32_t inst, uint64_t n_assumps) {
        if (!is_open(inst)) decided--;
        results[inst] = MI355SAT_INTERRUPTED;
        winner[inst] = -1;
        dropped[inst] = 0;
        if (cores) core_flag[inst].assign(n_assumps, 0);
    }
    // An open instance gets its verdict, from `worker` (-1: from no search).
    void decide(uint32_t inst, int32_t verdict, int32_t worker) { results[inst] = verdict; winner[inst] = worker; decided++; }
    // The caller withdraws an instance / takes it up again: true if that changes what there is to search.  Only an open
    // instance is withdrawn, only one withdrawn without a verdict comes back - as UNSAT at once, and counted as before,
    // if the formula itself has fallen meanwhile.
    bool withdraw(uint32_t inst) {
        if (!is_open(inst)) return false;
        dropped[inst] = 1;
        decided++;
        return true;
    }
    bool reopen(uint32_t inst) {
        if (!dropped[inst] || results[inst] != MI355SAT_INTERRUPTED) return false;
        dropped[inst] = 0;
        if (formula_unsat) { results[inst] = MI355SAT_UNSAT; return false; }
        decided--;
        return true;
    }
    // A sweep over n instances begins (assump_off: the caller's lists): nothing decided, no kernel time, no counters
    // taken over.  `cores` is the caller's to set before, `split` and the per-worker arrays (place_workers) follow once
    // the fleet is known.
    void reset(uint32_t n, bool first_only, const std::vector<uint64_t>& assump_off) {
        n_instances = n;
        stop_at_first = first_only;
        decided = 0;
        active = split = formula_unsat = false;
        n_moved = 0;
        ramp_ms = 0;
        counters0.clear();
        conflicts0 = 0;
        results.assign(n, MI355SAT_INTERRUPTED);
        winner.assign(n, -1);
        dropped.assign(n, 0);
        core_flag.assign(cores ? n : 0, {});
        core_logged.assign(log_cores ? n : 0, 0);
        for (uint32_t i = 0; i < n; i++) pose(i, assump_off[i + 1] - assump_off[i]);
    }

    // ---- a worker: busy on a cube of its instance (running, or finished with a status sweep_step has yet to take), or
    // idle (parked on the device, or finished and read).  Only assign / idle / close_cube / park / place_workers write w_inst,
    // w_busy, w_cube, w_conf0 and open.
    std::vector<int32_t> base_cube(uint32_t inst) const {      // the instance's own list: the cube of its whole search space
        return std::vector<int32_t>(base_assump.begin() + base_off[inst], base_assump.begin() + base_off[inst + 1]);
    }
    bool holds_model(uint32_t w) const { return model_holder(results, winner, (uint32_t)w_inst[w]) == (int32_t)w; }
    // Worker w is busy on `cube` of instance inst from now on.  u (null: the device has it already, as at the start)
    // takes the record: the list and MS_ST_RUNNING, with `restart` from level 0 and its conflicts on the cube counted anew.
    void assign(uint32_t w, uint32_t inst, std::vector<int32_t> cube, int32_t restart, WorkerUpdates* u) {
        if (w_busy[w]) open[w_inst[w]]--;
        w_inst[w] = (int32_t)inst;
        w_busy[w] = 1;
        w_cube[w] = std::move(cube);
        open[inst]++;
        if (w < sts.size()) {                    // (not before the first slice: nothing is gathered yet)
            if (restart) w_conf0[w] = sts[w].conflicts;
            sts[w].status = MS_ST_RUNNING;
        }
        if (u) u->add(w, MS_ST_RUNNING, restart, w_cube[w]);
    }
    void idle(uint32_t w) {
        if (w_busy[w]) open[w_inst[w]]--;
        w_busy[w] = 0;
        w_cube[w].clear();
    }
    // Worker w came back MS_ST_REFUTED / MS_ST_UNSAT and sweep_step has read that: its cube is closed.
    void close_cube(uint32_t w) { idle(w); n_closed++; }
    // Worker w gives up its cube; a running one hears MS_ST_PARKED (a finished one keeps its status on the device).
    void park(uint32_t w, WorkerUpdates& u) {
        idle(w);
        if (sts[w].status != MS_ST_RUNNING) return;
        u.add(w, MS_ST_PARKED, 0, {});
        sts[w].status = MS_ST_PARKED;
    }
    // Worker w of W starts on instance w % n_instances, its cube that instance's list; with cube splitting only the first
    // worker of an instance is busy, the others wait for a cube to steal.
    void place_workers(uint32_t W) {
        w_inst.assign(W, 0);
        w_cube.assign(W, {});
        w_busy.assign(W, 0);
        w_conf0.assign(W, 0);
        open.assign(n_instances, 0);
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t inst = w % n_instances;
            if (split && w >= n_instances) w_inst[w] = (int32_t)inst;
            else assign(w, inst, base_cube(inst), 0, nullptr);
        }
    }
};

// Nothing to tell: no upload, no launch.  resident (warm_begin, its one user): the lists are on the device already and
// more follows on the stream - no `data`, no wait.
inline void WorkerUpdates::send(mi355sat& s, Sweep& sw, const int32_t* resident) {
    if (upd.empty()) return;
    // One record per worker: the records of a launch are applied by workgroups in no particular order, so of two for
    // one worker (parked because its instance was decided and handed a stolen cube in the same pass of schedule_cubes;
    // woken and moved on in one pass of rebalance_workers) either could come last.  The later one holds, a restart
    // request of either stays.
    {
        std::vector<int32_t> last;
        std::vector<size_t> at_of;     // worker -> its record in `last`, + 1
        for (size_t r = upd.size() / 5; r-- > 0;) {
            const size_t w = (size_t)upd[5 * r];
            if (w >= at_of.size()) at_of.resize(w + 1, 0);
            if (at_of[w]) { last[at_of[w] - 1 + 2] |= upd[5 * r + 2]; continue; }
            at_of[w] = last.size() + 1;
            last.insert(last.end(), upd.begin() + 5 * r, upd.begin() + 5 * r + 5);
        }
        upd.swap(last);
    }
    const uint32_t n = (uint32_t)(upd.size() / 5);
    sw.d_upd.upload(upd, s.stream);
    if (!resident) sw.d_data.upload_nonempty(data, s.stream);
    hipLaunchKernelGGL(ms_assign_kernel, dim3(n), dim3(64), 0, s.stream, s.L, s.d_slabs.p, n, sw.d_upd.p, resident ? resident : sw.d_data.p);
    HIPCHK(hipGetLastError());
    if (!resident) HIPCHK(hipStreamSynchronize(s.stream));
}

// Caller's assumption lists -> device literals: equivalent-literal substitution, then the device's variable order (perm);
// each literal at most once per instance (a repeated assumption would open a level of its own: a list longer than n_vars
// would overrun trail_lim).  base_src keeps where each one came from in the caller's list of its instance.
void map_assumptions(const mi355sat& s, const std::vector<uint32_t>& perm, uint32_t n_vars, const std::vector<int32_t>& assump,
                     const std::vector<uint64_t>& assump_off, uint32_t n_instances, std::vector<int32_t>& a_int,
                     std::vector<uint64_t>& a_off, std::vector<uint32_t>& base_src) {
    a_int.clear();
    a_off.assign(1, 0);
    base_src.clear();
    std::vector<uint32_t> stamp(2 * (size_t)n_vars, 0);
    for (uint32_t i = 0; i < n_instances; i++) {
        for (uint64_t k = assump_off[i]; k < assump_off[i + 1]; k++) {
            const int32_t d = assump[k];
            if (d == 0 || var_of(d) > n_vars) throw HipErr{"assumption literal out of range"};
            const int32_t l = device_literal(s, perm, d);
            if (stamp[l] == i + 1) continue;
            stamp[l] = i + 1;
            a_int.push_back(l);
            base_src.push_back((uint32_t)(k - assump_off[i]));
        }
        a_off.push_back(a_int.size());
    }
}

inline uint32_t fleet_size(const mi355sat& s) {      // opts.workers, or the default by formula size (sweep_begin)
    return s.opts.workers > 0 ? (uint32_t)s.opts.workers
                              : (s.offs.size() > 100000 ? MS_SEARCH_WAVES_PER_SIMD * 1024u : (s.offs.size() > 20000 ? 1024u : 256u));
}

// Ramp-up: a worker alone on its CU runs ~3x faster than one of 16, and an easy instance is decided by ONE
// worker's few hundred conflicts - so the first 100 ms of kernel time go to one worker per CU, the next
// 300 ms to four, and only a search that is still open after that gets the whole fleet.  (Measured: rect
// 32x32 k=120 0.167 -> 0.088 s; 250 / 1000 ms thresholds gain nothing more at 64x64 - a worker there is bound
// by DRAM latency even when alone - and delay the rect 24x24 ladder by 0.5-1 s.)
// How many of `fleet` workers the next slice runs - and need a slab - a whole number per instance.
uint32_t ramp_target(const mi355sat& s, const Sweep& sw, uint32_t fleet) {
    if (s.opts.ramp < 0 || sw.split || s.opts.deterministic > 0) return fleet;
    const uint32_t n = sw.n_instances, want = sw.ramp_ms < 100.f ? 256u : (sw.ramp_ms < 400.f ? 1024u : fleet);
    return std::min(fleet, std::max(want, n) / n * n);
}

// (a batch or a sweep that logs a proof) One line - the negated core, in the caller's literals - for every instance that
// is UNSAT and has none yet, in instance order: behind the lemmas of the slice that decided them (sweep_step), or behind
// what the simplification derived when that refuted the formula (sweep_begin).  The line is RUP where it stands: the
// deciding worker's clauses are in the file, and its final conflict follows from them under the core by propagation.
// The empty clause - the core of a formula that is refuted itself, by a worker or by the simplification - is written once
// per file; a core that holds a literal and its negation gives a tautology, and nothing is written for it.  An instance
// answered UNSAT "at once" when it is reopened (Sweep::reopen) has the empty core: no line.
void proof_core_lines(mi355sat& s, Sweep& sw) {
    if (!s.proof_file || !sw.log_cores) return;
    auto empty_clause = [&] {
        if (!s.proof_empty) fputs("0\n", s.proof_file);
        s.proof_empty = true;
    };
    if (sw.formula_unsat) empty_clause();        // (also when no instance was open to take the verdict)
    for (uint32_t i = 0; i < sw.n_instances; i++) {
        if (sw.results[i] != MI355SAT_UNSAT || sw.core_logged[i]) continue;
        sw.core_logged[i] = 1;
        std::vector<int32_t> core = sw.core_of(i), sorted;
        if (core.empty()) { empty_clause(); continue; }
        sorted = core;
        std::sort(sorted.begin(), sorted.end(), [](int32_t a, int32_t b) { return var_of(a) != var_of(b) ? var_of(a) < var_of(b) : a < b; });
        bool taut = false;
        for (size_t k = 0; k + 1 < sorted.size(); k++) taut = taut || sorted[k] == -sorted[k + 1];
        if (taut) continue;
        for (int32_t l : core) fprintf(s.proof_file, "%d ", -l);
        fputs("0\n", s.proof_file);
        s.proof_log.core_lines++;
    }
}

// keep (may be null): caller's literals whose variables must survive the simplification besides the assumptions' - lists
// that sweep_repose will pose later; their number is also the room the slabs leave for an assumption list.
int sweep_begin(mi355sat& s, Sweep& sw, const std::vector<int32_t>& assump, const std::vector<uint64_t>& assump_off,
                uint32_t n_instances, bool stop_at_first, const std::vector<int32_t>* keep = nullptr, bool plain_solve = false) {
    Prepared P;
    {
        Formula F;
        normalise(s, F);
        F.log_proof = !s.proof_path.empty();
        auto freeze = [&](const std::vector<int32_t>& list) {
            for (int32_t d : list)
                if (d != 0 && var_of(d) <= F.nv) F.frozen_lits.push_back(to_internal(d));
        };
        freeze(assump);
        if (keep) freeze(*keep);
        simplify_formula(s, F);
        if (s.keep_simplified) keep_simplified_copy(s, F);
        build_csr(s, F, /*units_propagated=*/true, P);
        s.subst = F.subst;
        s.elims.swap(F.elims);
        s.elim_lits.swap(F.elim_lits);
        s.stats.simp_eliminated = F.n_eliminated;
        s.simp_proof.swap(F.proof);
        s.stats.simp_units = F.n_failed + F.n_necessary;
        s.stats.simp_equivalences = F.n_equiv;
        s.stats.simp_clauses_removed = F.n_subsumed + F.n_strengthened;
    }
    if (!s.proof_path.empty()) {
        if (n_instances != 1 && s.opts.cube_split > 0) throw HipErr{"a proof can only be logged for a plain solve()"};
        proof_open(s);
        // (a plain solve ends its file itself, with the core mi355sat_solve reports: proof_close)
        sw.log_cores = sw.cores && !plain_solve;
        if (sw.log_cores) { sw.caller_assump = assump; sw.caller_off = assump_off; }
    }
    sw.reset(n_instances, stop_at_first, assump_off);
    s.ph.on_device = false;              // (the mapping of the hints on the device was the last upload's)
    if (P.unsat) {
        for (uint32_t i = 0; i < n_instances; i++) sw.decide(i, MI355SAT_UNSAT, -1);
        s.trivially_unsat = true;
        proof_core_lines(s, sw);
        return 0;
    }
    // default fleet: the whole GPU (16 waves per CU) for large formulas; mid-size ones measured fastest to a verdict
    // with 1024 workers (rect 24x24 ladder), small ones do not pay for more than one worker per CU
    uint32_t want = fleet_size(s);
    if (want < n_instances) want = n_instances;
    want = want / n_instances * n_instances;
    s.d_proof.release();
    s.d_proof_len.release();
    s.proof_cap = 0;
    sw.split = s.opts.cube_split > 0 && want > n_instances;   // opt-in: see DESIGN.md (measured: not yet a win)
    std::vector<int32_t> a_int;
    std::vector<uint64_t> a_off;
    map_assumptions(s, P.perm, P.n_vars, assump, assump_off, n_instances, a_int, a_off, sw.base_src);
    uint32_t max_assumps = 0;
    for (uint32_t i = 0; i < n_instances; i++)
        max_assumps = std::max<uint32_t>(max_assumps, (uint32_t)(a_off[i + 1] - a_off[i]));
    // (a solve that may be followed by warm ones leaves room for their assumption lists)
    if (keep) max_assumps = std::max<uint32_t>(max_assumps, (uint32_t)keep->size());
    const uint32_t assump_cap = sw.split ? max_assumps + 512 : max_assumps + (sw.keep_warm ? 256u : 0u);
    upload_formula(s, P, assump_cap, 0, want, /*initial_workers=*/ramp_target(s, sw, want), s.want_learnt_cap, s.want_learnt_lit_cap, MI355SAT_ERR_HIP, s.want_pool_slack);
    if (s.n_workers < n_instances) throw HipErr{"not enough device memory for one worker per instance"};
    s.n_workers = s.n_workers / n_instances * n_instances;
    s.n_alloc = std::min(s.n_alloc, s.n_workers);
    if (!s.proof_path.empty()) {   // one log per worker, drained after every slice: a slice's lemmas (~10^4 learnt clauses) plus the
        // deletion lines of one clause-database reduction, which may drop half of a full learnt store at once (lemmas that do
        // not fit fail the solve - the proof would be wrong; deletion lines that do not fit are dropped - they are optional)
        s.proof_cap = (uint32_t)std::min<uint64_t>(1u << 23, (1u << 20) + s.L.learnt_lit_cap / 2 + 2ull * s.L.learnt_cap);
        if (s.want_proof_cap) s.proof_cap = s.want_proof_cap;
        s.d_proof.alloc((size_t)s.n_workers * s.proof_cap);
        s.d_proof_len.alloc(2 * (size_t)s.n_workers);
        HIPCHK(hipMemsetAsync(s.d_proof_len.p, 0, sizeof(uint32_t) * 2 * s.n_workers, s.stream));
        s.d_proof_inv.upload(inverse_order(P.perm), s.stream);      // (what ms_proof_gather_kernel maps a log's literals through)
    }
    s.cap_info = mi355sat_capacity_info{};
    s.cap_info.learnt_cap = s.L.learnt_cap; s.cap_info.learnt_lit_cap = s.L.learnt_lit_cap; s.cap_info.pool_cap = s.L.pool_cap;
    s.cap_info.pool_initial = (uint32_t)s.pool_init; s.cap_info.proof_cap = s.proof_cap; s.cap_info.assump_cap = s.L.assump_cap;
    s.cap_info.vm_cap = s.L.vm_cap;
    s.cap_info_valid = true;
    s.cap_events[0] = s.cap_events[1] = s.cap_events[2] = 0;
    reset_workers(s);
    customize(s, &a_int, &a_off, nullptr, nullptr, n_instances, sw.split ? (int32_t)n_instances : -1);
    s.ph.dev_fixed.assign(P.n_vars, 0);
    for (int32_t l : P.units) s.ph.dev_fixed[l >> 1] = 1;
    apply_phases(s, /*warm=*/false);     // after the customisation: a hint outranks opts.phase_mix
    HIPCHK(hipStreamSynchronize(s.stream));
    s.stats.workers = s.n_workers;
    sw.base_assump = a_int;
    sw.base_off = a_off;
    sw.place_workers(s.n_workers);
    sw.active = true;
    return 0;
}

// Work stealing between two slices: idle workers take over sub-cubes split off the oldest free
// decisions of running workers.  Victim with cube C and decisions d1..dm keeps C,d1..dm; thief j
// gets C,d1..d(j-1),~dj — together they partition C, so an instance is UNSAT exactly when all its
// cubes are closed.
void schedule_cubes(mi355sat& s, Sweep& sw) {
    const uint32_t W = s.n_workers, cap = s.L.assump_cap;
    WorkerUpdates u;
    std::vector<uint32_t> idle, victims;
    for (uint32_t w = 0; w < W; w++) {
        // Its instance was decided by someone else: parked, whatever its own status - nobody wants that any more.  (Here
        // the two parks differ for a reason: rebalance_workers leaves a FINISHED worker its cube, whose verdict sweep_step
        // takes once the instance is open again.  That only this one cleared the cube was an accident: nothing reads it.)
        if (sw.w_busy[w] && sw.results[sw.w_inst[w]] != MI355SAT_INTERRUPTED) sw.park(w, u);
        if (!sw.w_busy[w]) { if (!sw.holds_model(w)) idle.push_back(w); }
        else if (sw.sts[w].status == MS_ST_RUNNING && sw.sts[w].n_split > 0) victims.push_back(w);
    }
    // hardest cubes first: most conflicts spent on the current cube
    std::sort(victims.begin(), victims.end(), [&](uint32_t a, uint32_t b) {
        return sw.sts[a].conflicts - sw.w_conf0[a] > sw.sts[b].conflicts - sw.w_conf0[b];
    });
    std::vector<uint32_t> taken(W, 0);
    size_t next_idle = 0;
    for (uint32_t round = 0; round < MS_SPLIT_MAX && next_idle < idle.size(); round++) {
        bool any = false;
        for (uint32_t v : victims) {
            if (next_idle >= idle.size()) break;
            if (taken[v] != round || (int32_t)round >= sw.sts[v].n_split) continue;
            if (sw.w_cube[v].size() + 1 > cap) continue;
            const int32_t d = sw.sts[v].split[round];
            const uint32_t inst = (uint32_t)sw.w_inst[v];
            std::vector<int32_t> cube = sw.w_cube[v];
            cube.push_back(d ^ 1);
            sw.assign(idle[next_idle++], inst, cube, /*restart=*/1, &u);
            cube.back() = d;
            sw.assign(v, inst, cube, 0, nullptr);     // (its record follows once, with all it has given away)
            sw.n_splits++;
            taken[v] = round + 1;
            any = true;
        }
        if (!any) break;
    }
    for (uint32_t v : victims)
        if (taken[v]) sw.assign(v, (uint32_t)sw.w_inst[v], sw.w_cube[v], 0, &u);
    u.send(s, sw);
}

// Portfolio mode, between two slices: the workers of instances that are decided (or withdrawn) move to
// the open instances with the fewest workers.  They keep their learnt clauses (consequences of the
// formula alone) and only swap their assumption list; the worker holding a SAT instance's model stays.
// all (sweep_repose): every instance was posed anew, so every worker that has a slab moves, whatever it worked on.
void rebalance_workers(mi355sat& s, Sweep& sw, bool all = false) {
    const uint32_t n_instances = sw.n_instances;
    std::vector<uint32_t> cnt(n_instances, 0), movable;
    WorkerUpdates u;
    for (uint32_t w = 0; w < s.n_alloc; w++) {   // (a worker without a slab yet is picked up after grow_workers)
        const uint32_t inst = (uint32_t)sw.w_inst[w];
        const int st = sw.sts[w].status;
        if (!all && sw.is_open(inst)) {
            // parked when its instance was withdrawn (opts.rebalance = -1, or nothing was open), and the instance is open
            // again: back to its own list, from level 0.  Not a migration - it holds with rebalancing off too.  (A worker
            // that FINISHED its withdrawn instance - MS_ST_SAT, MS_ST_REFUTED - stays as it is: sweep_step takes its verdict.)
            if (st == MS_ST_PARKED) sw.assign(w, inst, sw.base_cube(inst), /*restart=*/1, &u);
            if (sw.sts[w].status == MS_ST_RUNNING) cnt[inst]++;
            continue;
        }
        if (!all && sw.holds_model(w)) continue;
        if (st == MS_ST_RUNNING || st == MS_ST_SAT || st == MS_ST_REFUTED || st == MS_ST_PARKED) movable.push_back(w);
    }
    std::vector<uint32_t> open;
    for (uint32_t i = 0; i < n_instances; i++) if (sw.is_open(i)) open.push_back(i);
    if (open.empty() || (s.opts.rebalance < 0 && !all)) {
        for (uint32_t w : movable)      // (only what runs: a finished worker keeps cube and status - see schedule_cubes)
            if (sw.sts[w].status == MS_ST_RUNNING) sw.park(w, u);
    } else {
        // Each open instance's share of the fleet follows its weight (mi355sat_sweep_set_weights; default equal).
        // Workers of instances well above their share (> 25 % and > 2 workers) are taken off them too - highest
        // worker index first, never the last one - so that a caller's change of priorities takes effect.
        double wsum = 0;
        for (uint32_t i : open) wsum += sw.weights.empty() ? 1.0 : std::max(1e-6, sw.weights[i]);
        uint32_t total = (uint32_t)movable.size();
        for (uint32_t i : open) total += cnt[i];
        std::vector<double> target(n_instances, 0);
        for (uint32_t i : open) target[i] = std::max(1.0, total * (sw.weights.empty() ? 1.0 : std::max(1e-6, sw.weights[i])) / wsum);
        if (!sw.weights.empty()) {
            std::vector<uint32_t> surplus(n_instances, 0);
            for (uint32_t i : open)
                if (cnt[i] > target[i] * 1.25 + 2) surplus[i] = cnt[i] - (uint32_t)target[i];
            for (uint32_t w = s.n_alloc; w-- > 0;) {
                const uint32_t inst = (uint32_t)sw.w_inst[w];
                if (!sw.is_open(inst) || !surplus[inst] || sw.sts[w].status != MS_ST_RUNNING || cnt[inst] <= 1) continue;
                surplus[inst]--;
                cnt[inst]--;
                movable.push_back(w);
            }
        }
        // an open instance nobody works on (reopened with every worker busy elsewhere, or its workers' slabs came later)
        // takes one worker from the instance that has the most - weights or not: it would never be decided otherwise
        for (uint32_t i : open) {
            if (cnt[i] > 0 || !movable.empty()) continue;
            uint32_t rich = open[0];
            for (uint32_t j : open) if (cnt[j] > cnt[rich]) rich = j;
            if (cnt[rich] <= 1) break;
            for (uint32_t w = s.n_alloc; w-- > 0;)
                if ((uint32_t)sw.w_inst[w] == rich && sw.sts[w].status == MS_ST_RUNNING) { movable.push_back(w); cnt[rich]--; break; }
        }
        for (uint32_t w : movable) {
            uint32_t best = open[0];
            double best_need = -1e30;
            for (uint32_t i : open) {   // the instance furthest below its share, relative to it
                const double need = (target[i] - cnt[i]) / target[i];
                if (need > best_need) { best_need = need; best = i; }
            }
            cnt[best]++;
            sw.assign(w, best, sw.base_cube(best), /*restart=*/1, &u);
            sw.n_moved++;
        }
    }
    u.send(s, sw);
}

// What ms_final_kernel and ms_core_model_kernel answer with: per wave k of n a row of bits (sw.d_fout, out_words words each:
// one bit per entry of a worker's assumption list) and a flag that the row is sound (sw.d_fok).  Grows the two buffers,
// has the caller launch its kernel on the stream, reads both back and hands over every set bit i of every row k, in
// increasing order; a row that is not sound ends it with MI355SAT_ERR_STATE and the caller's text.
inline uint32_t bit_row_words(const mi355sat& s) { return std::max<uint32_t>(1, (s.L.assump_cap + 31) / 32); }
template <class Launch, class Bit>
int read_bit_rows(mi355sat& s, Sweep& sw, uint32_t n, const char* not_ok, Launch launch, Bit bit) {
    const uint32_t out_words = bit_row_words(s);
    if (sw.d_fout.n < (size_t)n * out_words) sw.d_fout.alloc((size_t)n * out_words);
    if (sw.d_fok.n < n) sw.d_fok.alloc(n);
    launch(out_words);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> out((size_t)n * out_words);
    std::vector<int32_t> ok(n);
    HIPCHK(hipMemcpyAsync(out.data(), sw.d_fout.p, sizeof(uint32_t) * out.size(), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(ok.data(), sw.d_fok.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    for (uint32_t k = 0; k < n; k++) {
        if (!ok[k]) { set_error(&s, not_ok); return MI355SAT_ERR_STATE; }
        for (uint32_t i = 0; i < 32 * out_words; i++)
            if ((out[(size_t)k * out_words + i / 32] >> (i % 32)) & 1u) bit(k, i);
    }
    return 0;
}

// Failed assumptions of the workers in fw, which came back MS_ST_REFUTED from the slice just gathered: ms_final_kernel,
// on the stream ahead of anything that rewrites a slab's assumptions (rebalance_workers, schedule_cubes, customize).  The
// kernel reports indices into the worker's (deduplicated) assumption list: those below its instance's own count map back
// to the caller's list through base_src; split literals (cube_split) drop out - the cubes of an instance are the leaves
// of a complete split tree, so the union of their cores restricted to the instance's assumptions is a core of it.
int final_cores(mi355sat& s, Sweep& sw, const std::vector<int32_t>& fw) {
    const uint32_t n = (uint32_t)fw.size();
    const uint32_t mwords = (s.n_vars + 31) / 32;
    const bool lds = s.opts.lds_val >= 0 && 4ull * mwords <= 48 * 1024;   // the marks in LDS, or a scratch row per workgroup
    sw.d_fw.upload(fw, s.stream);
    return read_bit_rows(s, sw, n, "device solver internal error (final conflict analysis)", [&](uint32_t out_words) {
        if (lds) {
            hipLaunchKernelGGL(ms_final_kernel<true>, dim3(n), dim3(MS_WAVE), 4 * mwords, s.stream, s.sh, s.L, (const char*)s.d_slabs.p,
                               (const int32_t*)sw.d_fw.p, (uint32_t*)nullptr, sw.d_fout.p, out_words, sw.d_fok.p);
        } else {
            if (sw.d_fscratch.n < (size_t)n * std::max<uint32_t>(mwords, 1)) sw.d_fscratch.alloc((size_t)n * std::max<uint32_t>(mwords, 1));
            hipLaunchKernelGGL(ms_final_kernel<false>, dim3(n), dim3(MS_WAVE), 0, s.stream, s.sh, s.L, (const char*)s.d_slabs.p,
                               (const int32_t*)sw.d_fw.p, sw.d_fscratch.p, sw.d_fout.p, out_words, sw.d_fok.p);
        }
    }, [&](uint32_t k, uint32_t i) {
        const uint32_t inst = (uint32_t)sw.w_inst[fw[k]];
        const uint64_t b0 = sw.base_off[inst];
        if (i < sw.base_off[inst + 1] - b0) sw.core_flag[inst][sw.base_src[b0 + i]] = 1;
    });
}

// ---- warm incremental solve ----------------------------------------------------------------------------------------
// Clauses [c0, c1) of inc.lits / inc.offs (on the device already) to workers [from, to): ms_attach_kernel, on the stream.
void attach_clauses(mi355sat& s, uint32_t from, uint32_t to, uint32_t c0, uint32_t c1) {
    if (to <= from) return;
    hipLaunchKernelGGL(ms_attach_kernel, dim3(to - from), dim3(MS_WAVE), 0, s.stream, s.sh, s.L, s.d_slabs.p, from, to,
                       (const int32_t*)s.d_inc_lits.p, (const uint32_t*)s.d_inc_offs.p, c0, c1);
    HIPCHK(hipGetLastError());
    s.inc.info.attach_launches++;
}

// Start a plain solve() on the workers the one before left on the device: nothing is simplified, built, uploaded or reset.
// The clauses added since go through the mapping the upload gave the assumptions (s.subst, then s.perm) and are attached
// to every resident worker; every worker gets the new assumption list and MS_ST_RUNNING (ms_assign_kernel) and keeps its
// learnt clauses, saved phases, decision order, restart averages and its position in the exchange ring.  Returns
// MI355SAT_COLD_NONE with sw ready for sweep_step() (or decided already), or the reason why this solve has to start cold
// (nothing on the device has changed then, except after MI355SAT_COLD_DEVICE_FULL).
int warm_begin(mi355sat& s, Sweep& sw, const std::vector<int32_t>& assump, const std::vector<uint64_t>& assump_off) {
    mi355sat::Incremental& I = s.inc;
    if (!s.proof_path.empty()) return MI355SAT_COLD_PROOF;
    if (s.opts.cube_split > 0) return MI355SAT_COLD_CUBE_SPLIT;
    if (!I.resident) return I.why_not;
    // the caller's literal on the device, or the reason why it has none
    auto map_lit = [&](int32_t d, int32_t& out) -> int {
        if (var_of(d) > s.n_vars) return MI355SAT_COLD_NEW_VAR;
        out = device_literal(s, s.perm, d, &I.eliminated);
        return out < 0 ? MI355SAT_COLD_ELIMINATED : 0;
    };
    int32_t l = 0;
    for (int32_t d : assump) if (int why = map_lit(d, l)) return why;
    std::vector<int32_t> a_int;
    std::vector<uint64_t> a_off;
    std::vector<uint32_t> base_src;
    map_assumptions(s, s.perm, s.n_vars, assump, assump_off, 1, a_int, a_off, base_src);
    if (a_int.size() > s.L.assump_cap) return MI355SAT_COLD_ASSUMP_CAP;
    // the clauses added since the workers last heard of any: sorted, without repeated literals and tautologies
    const size_t nc = s.offs.size() - 1;
    std::vector<int32_t> nl, tmp;
    std::vector<uint32_t> no;
    uint64_t units = 0, pinned = 0, pinned_lits = 0;
    bool empty_clause = false;
    for (size_t c = I.n_clauses; c < nc; c++) {
        tmp.clear();
        for (uint64_t k = s.offs[c]; k < s.offs[c + 1]; k++) {
            if (int why = map_lit(s.lits[k], l)) return why;
            tmp.push_back(l);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        bool taut = false;
        for (size_t i = 0; i + 1 < tmp.size(); i++) if ((tmp[i] ^ 1) == tmp[i + 1]) taut = true;
        if (taut) continue;
        if (tmp.empty()) { empty_clause = true; continue; }
        if (tmp.size() == 1) units++;
        else { pinned++; pinned_lits += (tmp.size() + 3) & ~(size_t)3; }
        nl.insert(nl.end(), tmp.begin(), tmp.end());
        no.push_back((uint32_t)nl.size());
    }
    // attached clauses are never dropped (reduce_db keeps LBD <= 2): they may take a quarter of a worker's learnt store
    if (I.pinned + pinned > s.L.learnt_cap / 4 || I.pinned_lits + pinned_lits > s.L.learnt_lit_cap / 4) return MI355SAT_COLD_PINNED_SHARE;

    // from here on the solve is warm
    const uint32_t c0 = (uint32_t)(I.offs.size() - 1);
    for (uint32_t o : no) I.offs.push_back((uint32_t)I.lits.size() + o);
    I.lits.insert(I.lits.end(), nl.begin(), nl.end());
    const uint32_t c1 = (uint32_t)(I.offs.size() - 1);
    I.pinned += pinned;
    I.pinned_lits += pinned_lits;
    I.n_clauses = nc;
    sw.reset(1, /*first_only=*/true, assump_off);
    sw.base_src = base_src;
    sw.base_assump = a_int;
    sw.base_off = a_off;
    const uint32_t W = s.n_workers;
    sw.place_workers(W);         // (one instance: every worker on it)
    sw.counters0 = I.base;
    sw.counters0.resize(W, MsState{});
    I.info.resident_learnts = 0;
    for (const MsState& st : sw.counters0) { sw.conflicts0 += st.conflicts; I.info.resident_learnts += st.n_learnts; }
    I.info.attached_clauses += pinned;
    I.info.attached_units += units;
    if (empty_clause) {
        I.refuted = true;
        sw.decide(0, MI355SAT_UNSAT, -1);
        return MI355SAT_COLD_NONE;
    }
    // the assumption list: to every resident worker now, and where grow_workers takes it from for the workers it creates
    s.d_assump.upload_nonempty(a_int, s.stream);
    s.d_assump_off.upload(a_off, s.stream);
    WorkerUpdates u;
    for (uint32_t w = 0; w < s.n_alloc; w++) u.add_at(w, MS_ST_RUNNING, 1, a_int.size(), 0);    // (every worker reads s.d_assump)
    u.send(s, sw, s.d_assump.p);
    s.d_inc_lits.upload_nonempty(I.lits, s.stream);
    s.d_inc_offs.upload(I.offs, s.stream);
    attach_clauses(s, 0, s.n_alloc, c0, c1);    // (without new clauses it still takes every worker to level 0)
    HIPCHK(hipMemsetAsync(s.d_any_done.p, 0, sizeof(int32_t), s.stream));
    std::vector<MsState> sts;
    gather_states(s, sts);
    s.stats.workers = W;
    sw.active = true;
    for (const MsState& st : sts) {
        if (st.status == MS_ST_ERR_INTERNAL) throw HipErr{status_text(st.status)};
        if (st.status < 0) { sw.active = false; return MI355SAT_COLD_DEVICE_FULL; }
        if (st.status == MS_ST_UNSAT && sw.is_open(0)) {      // a new clause is false under the level-0 facts
            I.refuted = true;
            sw.decide(0, MI355SAT_UNSAT, -1);
        }
    }
    sw.sts = sts;
    if (sw.decided == 0) apply_phases(s, /*warm=*/true);    // every worker stands at level 0 (attach_clauses)
    return MI355SAT_COLD_NONE;
}

// What the slice just gathered decided: closes the cubes of the workers that came back refuted and gives the open
// instances their verdicts.  fw receives the refuted workers whose failed assumptions are wanted (final_cores).  Returns 0
// or the error of a worker whose stores are full.
int collect_verdicts(mi355sat& s, Sweep& sw, std::vector<int32_t>& fw) {
    int rc = 0;
    uint64_t confl = 0;
    for (uint32_t w = 0; w < s.n_workers; w++) {
        const MsState& st = sw.sts[w];
        confl += st.conflicts;
        if (st.status < 0) rc = status_error(s, st.status, MI355SAT_ERR_STATE);
        if (!sw.w_busy[w]) continue;
        const uint32_t inst = (uint32_t)sw.w_inst[w];
        // A worker that finishes the cube of a WITHDRAWN instance keeps it (busy, its status as it is; a non-running worker
        // is not touched by a slice): the cube is closed, and the verdict taken, at the first step after mi355sat_sweep_reopen.
        if (st.status == MS_ST_UNSAT) sw.formula_unsat = true;
        else if (sw.dropped[inst]) continue;
        if (st.status == MS_ST_REFUTED || st.status == MS_ST_UNSAT) sw.close_cube(w);
        if (st.status == MS_ST_UNSAT) {   // refuted without any decision: the formula itself, whatever the assumptions
            for (uint32_t i = 0; i < sw.n_instances; i++)
                if (sw.is_open(i)) {
                    sw.decide(i, MI355SAT_UNSAT, (int32_t)w);
                    if (sw.cores) std::fill(sw.core_flag[i].begin(), sw.core_flag[i].end(), 0);   // the empty core
                }
            continue;
        }
        if (!sw.is_open(inst)) continue;
        // with splitting every closed cube contributes to its instance's core, without it the deciding worker alone
        if (sw.cores && st.status == MS_ST_REFUTED) fw.push_back((int32_t)w);
        if (st.status == MS_ST_SAT) sw.decide(inst, MI355SAT_SAT, (int32_t)w);
        // (with splitting) the last open cube of the instance closed; without it every worker holds the whole search space
        else if (st.status == MS_ST_REFUTED && (!sw.split || sw.open[inst] == 0)) sw.decide(inst, MI355SAT_UNSAT, (int32_t)w);
    }
    sw.conflicts = confl - sw.conflicts0;
    return rc;
}

void report_slice(const mi355sat& s, const Sweep& sw) {      // opts.verbose
    uint64_t confl = 0, props = 0, nl = 0, busy = 0, viv = 0, vivl = 0;
    for (auto& st : sw.sts) { confl += st.conflicts; props += st.propagations; nl += st.n_learnts; viv += st.n_vivified; vivl += st.n_viv_lits; }
    if (viv) fprintf(stderr, "[mi355sat] vivified %llu clauses, %llu literals removed\n", (unsigned long long)viv, (unsigned long long)vivl);
    for (auto b : sw.w_busy) busy += b;
    fprintf(stderr, "[mi355sat] slice: decided %u/%u conflicts=%llu props=%llu kernel=%.3fs busy=%llu/%u splits=%llu closed=%llu kept=%llu\n",
            sw.decided, sw.n_instances, (unsigned long long)confl, (unsigned long long)props, s.stats.kernel_seconds,
            (unsigned long long)busy, s.n_workers, (unsigned long long)sw.n_splits, (unsigned long long)sw.n_closed,
            (unsigned long long)nl);
}

// What must hold between two slices, whatever the caller did: O(workers + instances), nothing next to a slice and its
// gather_states.  A violation is a slip of the bookkeeping above and would show slices later as a stall or a lost verdict.
int sweep_consistent(mi355sat& s, const Sweep& sw) {
    const char* bad = nullptr;
    uint32_t not_open = 0;
    std::vector<uint32_t> busy(sw.n_instances, 0);
    for (uint32_t i = 0; i < sw.n_instances; i++) {
        not_open += sw.is_open(i) ? 0 : 1;
        const int32_t win = sw.winner[i];
        if (sw.results[i] == MI355SAT_INTERRUPTED ? win != -1 : win < -1 || win >= (int32_t)sw.w_inst.size()) bad = "an instance's winner";
        else if (sw.dropped[i] && sw.results[i] != MI355SAT_INTERRUPTED) bad = "a verdict on a withdrawn instance";
        else if (sw.results[i] == MI355SAT_SAT && (win < 0 || (uint32_t)sw.w_inst[win] != i)) bad = "a model's worker moved on";
    }
    if (sw.decided != not_open) bad = "the count of decided instances";
    for (size_t w = 0; w < sw.w_inst.size() && sw.active; w++) {
        if ((uint32_t)sw.w_inst[w] >= sw.n_instances) { bad = "a worker's instance"; break; }
        if (sw.w_busy[w]) busy[sw.w_inst[w]]++;
        else if (!sw.w_cube[w].empty()) bad = "an idle worker's cube";
    }
    for (uint32_t i = 0; i < sw.n_instances && sw.active && !bad; i++)
        if (sw.open[i] != busy[i]) bad = "an instance's busy workers";
    if (!bad) return 0;
    s.err = std::string("device solver internal error (sweep bookkeeping: ") + bad + ")";
    return MI355SAT_ERR_STATE;
}

// One slice of the search kernel over all workers.  Returns 0 or a negative error.
int sweep_step(mi355sat& s, Sweep& sw) {
    if (!sw.active) return 0;
    const uint32_t n_instances = sw.n_instances;
    // 1. ramp-up: the fleet of this slice, and slabs for it
    const uint32_t active = ramp_target(s, sw, s.n_workers);
    if (active > s.n_alloc) {
        const uint32_t had = s.n_alloc;
        grow_workers(s, n_instances, active);
        // the new workers start on instance w % n_instances - which may be decided or withdrawn by now: move them before the slice
        if (n_instances > 1 && !sw.split && s.n_alloc > had && !sw.sts.empty() && sw.decided > 0) {
            sw.sts.resize(s.n_workers, MsState{});
            rebalance_workers(s, sw);
        }
        // (warm incremental solve) workers fresh from the template know the uploaded formula only: everything attached since
        if (sw.keep_warm && s.n_alloc > had && s.inc.offs.size() > 1) attach_clauses(s, had, s.n_alloc, 0, (uint32_t)(s.inc.offs.size() - 1));
    }
    // 2. launch.  Default slice length: 20 ms while a solve is young (easy bounds are decided within a few), 50 ms after one
    // second and 100 ms after ten of kernel time - the host's share per slice (collecting states, the caller's loop) was a
    // quarter of the wall-clock of the rect 26x26 ladder with 10 ms slices
    const int auto_ms = sw.ramp_ms < 1000.f ? 20 : (sw.ramp_ms < 10000.f ? 50 : 100);
    SliceResult sr = launch_slice(s, 0, /*stop_on_any=*/n_instances == 1 || sw.stop_at_first, /*done_on_refuted=*/!sw.split, active, auto_ms);
    sw.ramp_ms += sr.ms;
    // 3. drain, gather, collect
    proof_drain(s);
    gather_states(s, sw.sts);
    std::vector<int32_t> fw;
    int rc = collect_verdicts(s, sw, fw);
    if (s.opts.verbose) report_slice(s, sw);
    if (rc) return rc;
    // 4. cores - before any slab's assumptions are rewritten below - and who works on what in the next slice
    if (!fw.empty() && (rc = final_cores(s, sw, fw)) != 0) return rc;
    proof_core_lines(s, sw);
    HIPCHK(hipMemsetAsync(s.d_any_done.p, 0, sizeof(int32_t), s.stream));
    if (sw.decided < n_instances && !(sw.stop_at_first && sw.decided > 0)) {
        if (sw.split) schedule_cubes(s, sw);
        else if (n_instances > 1 && (sw.decided > 0 || sw.weights_dirty)) rebalance_workers(s, sw);
        sw.weights_dirty = false;
    }
    return sweep_consistent(s, sw);
}

bool sweep_finished(const mi355sat& s, const Sweep& sw) {
    if (!sw.active) return true;
    if (sw.decided == sw.n_instances || (sw.stop_at_first && sw.decided > 0)) return true;
    if (s.interrupted.load() || *s.stop_flag) return true;
    if (s.opts.conflict_budget > 0 && (int64_t)sw.conflicts >= s.opts.conflict_budget) return true;
    return false;
}

// An interrupt is consumed by the solve it stops (or, if it came before solve(), by the next one, which
// returns INTERRUPTED at once): later solves on the same handle run normally.
void consume_interrupt(mi355sat& s) {
    if (s.interrupted.exchange(0)) __atomic_store_n(s.stop_flag, 0, __ATOMIC_SEQ_CST);
}

void sweep_end(mi355sat& s, Sweep& sw) {
    if (sw.active && !sw.counters0.empty()) {   // a warm solve: the workers' counters ran on from the solve before
        std::vector<MsState> d = sw.sts;
        for (size_t w = 0; w < d.size() && w < sw.counters0.size(); w++)
            for_each_counter(d[w], sw.counters0[w], [](auto& now, const auto& then) { now -= then; });
        accumulate_stats(s, d);
    } else if (sw.active) accumulate_stats(s, sw.sts);
    sw.active = false;
    consume_interrupt(s);
}

// The model of instance inst from the slab of the worker that found it; false if the instance is not SAT.
bool fetch_model_of(mi355sat& s, const std::vector<int32_t>& results, const std::vector<int32_t>& winner, uint64_t inst, std::vector<int8_t>& out) {
    const int32_t w = model_holder(results, winner, inst);
    if (w >= 0) fetch_model(s, (uint32_t)w, out, s.max_var);
    return w >= 0;
}

// After the caller withdrew or reopened instances (changed: that made a difference): the workers of what is no longer
// open move on, parked workers and those of decided instances take up what is open again.  Not with cube splitting,
// where a withdrawn instance's cubes are searched on.
int reschedule_after_caller(mi355sat& s, Sweep& sw, bool changed) {
    if (changed && sw.active && !sw.split) {
        if (sw.sts.size() != s.n_workers) gather_states(s, sw.sts);
        rebalance_workers(s, sw);
    }
    return sweep_consistent(s, sw);
}

// cores (may be null): per instance, the caller's assumptions its UNSAT answer rests on, in the caller's order (empty
// for the other answers)
int run_search(mi355sat& s, const std::vector<int32_t>& assump, const std::vector<uint64_t>& assump_off,
               uint32_t n_instances, std::vector<int32_t>& results, std::vector<int32_t>& winner, bool stop_at_first,
               std::vector<std::vector<int32_t>>* cores = nullptr, bool plain_solve = false) {
    mi355sat::Incremental& I = s.inc;
    const bool incremental = plain_solve && I.on;     // (else solve_batch, or the mode is off: always cold, nothing kept)
    if (incremental && I.refuted && s.proof_path.empty()) {     // the formula only grows: UNSAT with the empty core, no launch
        results.assign(1, MI355SAT_UNSAT);
        winner.assign(1, -1);
        if (cores) cores->assign(1, {});
        consume_interrupt(s);
        I.info.warm_solves++;
        return 0;
    }
    Sweep sw;
    sw.cores = cores != nullptr;
    int rc = 0;
    // 1. warm - on the workers the solve() before left - or cold: simplified, uploaded and replicated anew
    const int why = incremental ? warm_begin(s, sw, assump, assump_off) : MI355SAT_COLD_FIRST;
    const bool warm = incremental && why == MI355SAT_COLD_NONE;
    sw.keep_warm = incremental && s.proof_path.empty() && s.opts.cube_split <= 0;    // (what a warm start takes, too)
    bool uploaded = false;      // a cold start put workers on the device that the next solve() may go on with
    if (warm) I.info.warm_solves++;
    else {
        if (incremental) {
            I.info.cold_solves++;
            I.info.last_cold_reason = why;
        }
        go_cold(s, plain_solve ? MI355SAT_COLD_FIRST : MI355SAT_COLD_OTHER_SEARCH);
        rc = sweep_begin(s, sw, assump, assump_off, n_instances, stop_at_first, nullptr, plain_solve);
        if (sw.keep_warm && !rc && s.trivially_unsat) I.refuted = true;
        uploaded = sw.keep_warm && !rc && !s.trivially_unsat;
        if (uploaded) {     // what these workers know: the formula as it stands, nothing attached
            I.n_clauses = s.offs.size() - 1;
            I.eliminated.assign(s.n_vars, 0);
            for (const MsElim& e : s.elims) I.eliminated[e.x >> 1] = 1;
            I.lits.clear();
            I.offs.assign(1, 0);
            I.pinned = I.pinned_lits = 0;
        }
    }
    // 2. search
    const bool searched = sw.active;
    while (!rc && !sweep_finished(s, sw)) rc = sweep_step(s, sw);
    // 3. what the next solve() finds on the device (an error that leaves by exception: mi355sat_solve goes cold)
    if (sw.keep_warm && rc) go_cold(s, MI355SAT_COLD_FIRST);
    else if (sw.keep_warm) {
        if (uploaded) I.resident = true;
        if (searched) {
            I.base = sw.sts;    // (empty: interrupted before the first slice - the workers are as the template left them)
            I.base.resize(s.n_workers, MsState{});
            for (const MsState& st : sw.sts) if (st.status == MS_ST_UNSAT) I.refuted = true;
        }
    }
    sweep_end(s, sw);
    results = sw.results;
    winner = sw.winner;
    if (cores) {
        cores->assign(n_instances, {});
        for (uint32_t i = 0; i < n_instances && !rc; i++) {
            if (results[i] != MI355SAT_UNSAT) continue;
            for (uint64_t k = 0; k < sw.core_flag[i].size(); k++)
                if (sw.core_flag[i][k]) (*cores)[i].push_back(assump[assump_off[i] + k]);
        }
    }
    return rc;
}


// ---- core minimisation (mi355sat_minimize_core) ------------------------------------------------------------------------
// Deletion-based minimisation of a failed-assumption core as ONE sweep: the formula is simplified, uploaded and replicated
// once, every round poses its candidates - the working core without one chunk each - into the running sweep
// (sweep_repose), and the workers keep their learnt clauses, saved phases, decision order and the exchange ring from
// round to round: all of that follows from the formula alone and holds under every candidate.  DESIGN.md §5.

// Pose `lits` (caller's literals) as instance `inst` of the running sweep in place of what it was: mapped as at the
// beginning (map_assumptions), base_assump / base_off / base_src rewritten, the instance open again with no verdict and
// an empty core.  The workers hear of it through sweep_retarget().
void sweep_repose(mi355sat& s, Sweep& sw, uint32_t inst, const std::vector<int32_t>& lits) {
    std::vector<int32_t> a_int;
    std::vector<uint64_t> a_off;
    std::vector<uint32_t> src;
    map_assumptions(s, s.perm, s.n_vars, lits, {0, (uint64_t)lits.size()}, 1, a_int, a_off, src);
    if (a_int.size() > s.L.assump_cap) throw HipErr{"reposed assumption list does not fit the slabs"};
    const uint64_t b0 = sw.base_off[inst], b1 = sw.base_off[inst + 1];
    sw.base_assump.erase(sw.base_assump.begin() + b0, sw.base_assump.begin() + b1);
    sw.base_assump.insert(sw.base_assump.begin() + b0, a_int.begin(), a_int.end());
    sw.base_src.erase(sw.base_src.begin() + b0, sw.base_src.begin() + b1);
    sw.base_src.insert(sw.base_src.begin() + b0, src.begin(), src.end());
    for (uint32_t i = inst + 1; i <= sw.n_instances; i++) sw.base_off[i] = sw.base_off[i] - (b1 - b0) + a_int.size();
    sw.pose(inst, lits.size());
}

// After the instances of a round are posed: every worker that has a slab moves to one of them (rebalance_workers ->
// ms_assign_kernel: new assumption list, MS_ST_RUNNING, back to level 0); the lists go where grow_workers takes them
// from for the workers the ramp-up creates later.
void sweep_retarget(mi355sat& s, Sweep& sw) {
    s.d_assump.upload_nonempty(sw.base_assump, s.stream);
    s.d_assump_off.upload(sw.base_off, s.stream);
    if (sw.sts.size() != s.n_workers) gather_states(s, sw.sts);
    rebalance_workers(s, sw, /*all=*/true);
    HIPCHK(hipMemsetAsync(s.d_any_done.p, 0, sizeof(int32_t), s.stream));
}

// What the models of SAT candidates say about the literals they did not assume: ms_core_model_kernel, one wave per
// winner, on the stream after the slice and ahead of anything that rewrites a slab's assumptions (a SAT instance's winner
// keeps its slab until sweep_retarget).  chunks[k] = the caller's literals winner k's candidate left out; falsified[k]
// receives, per device literal its model falsifies, the positions in chunks[k] that map to it.
int core_models(mi355sat& s, Sweep& sw, const std::vector<int32_t>& winners, const std::vector<std::vector<int32_t>>& chunks,
                std::vector<std::vector<std::vector<uint32_t>>>& falsified, mi355sat_core_min_info& info) {
    const uint32_t n = (uint32_t)winners.size();
    std::vector<int32_t> lits, q;
    std::vector<uint64_t> off{0}, q_off64;
    std::vector<uint32_t> src;
    for (const auto& c : chunks) { lits.insert(lits.end(), c.begin(), c.end()); off.push_back(lits.size()); }
    map_assumptions(s, s.perm, s.n_vars, lits, off, n, q, q_off64, src);
    std::vector<uint32_t> q_off(q_off64.begin(), q_off64.end());
    for (uint32_t k = 0; k < n; k++)
        if (q_off[k + 1] - q_off[k] > 32u * bit_row_words(s) || (uint32_t)winners[k] >= s.n_alloc) throw HipErr{"core minimisation: list out of range"};
    sw.d_fw.upload(winners, s.stream);
    sw.d_qlits.upload_nonempty(q, s.stream);
    sw.d_qoff.upload(q_off, s.stream);
    falsified.assign(n, {});
    return read_bit_rows(s, sw, n, "device solver internal error (a SAT worker's slab is no model)", [&](uint32_t out_words) {
        hipLaunchKernelGGL(ms_core_model_kernel, dim3(n), dim3(MS_WAVE), 0, s.stream, s.L, (const char*)s.d_slabs.p, (const int32_t*)sw.d_fw.p,
                           (const int32_t*)sw.d_qlits.p, (const uint32_t*)sw.d_qoff.p, sw.d_fout.p, out_words, sw.d_fok.p);
        info.model_launches++;
    }, [&](uint32_t k, uint32_t i) {
        const uint32_t b0 = q_off[k];
        if (i >= q_off[k + 1] - b0) return;
        std::vector<uint32_t> pos;
        for (uint32_t p = src[b0 + i]; p < chunks[k].size(); p++)       // (src: the first position that maps to it)
            if (device_literal(s, s.perm, chunks[k][p]) == q[b0 + i]) pos.push_back(p);
        falsified[k].push_back(pos);
    });
}

// The loop.  K: the working core (caller's literals, in the caller's order), crit[i]: K[i] is proved critical (formula
// AND K without K[i] is SAT - which it stays for every later K, a subset).  Invariant: formula AND K is UNSAT.  A round
// splits the literals not yet critical into chunks and poses K without chunk j as candidate j, at most N = min(64,
// workers) of them.  UNSAT: its final-conflict core F (a subset of K without the chunk) becomes K; crit stays inside F.
// SAT: the model falsifies a non-empty set D inside the chunk; |D| = 1 makes that literal critical.  A round of SAT
// answers without a new critical literal halves the chunk size; at size 1 every SAT answer is a critical literal.  So
// every round shrinks K, grows crit or halves the chunk size: the loop ends, with K = crit (irreducible), or on the
// conflict budget / an interrupt with a K that is still a core.
int minimize_search(mi355sat& s, std::vector<int32_t>& K, int64_t budget, mi355sat_core_min_info& info) {
    uint32_t N = std::min<uint32_t>(64, fleet_size(s));
    if (s.core_min_round) N = std::min(N, s.core_min_round);
    N = (uint32_t)std::min<size_t>(N, K.size());
    const std::vector<int32_t> K0 = K;
    std::vector<uint8_t> crit(K.size(), 0);
    uint64_t c = UINT64_MAX;              // chunk size of the round before (what a halving halves)
    Sweep sw;
    sw.cores = true;
    bool begun = false, stop = false;
    int rc = 0;
    while (!rc) {
        std::vector<uint32_t> open;       // positions in K not yet critical
        for (uint32_t i = 0; i < K.size(); i++) if (!crit[i]) open.push_back(i);
        if (open.empty()) { info.minimal = 1; break; }
        if (stop) break;
        // chunks: the whole of `open` in m even parts if that makes them no larger than c, else its first m * c literals
        const uint32_t m = (uint32_t)std::min<size_t>(N, open.size());
        const uint64_t even = (open.size() + m - 1) / m;
        std::vector<std::vector<uint32_t>> chunk(m);
        if (even <= c) c = even;
        for (uint32_t j = 0; j < m; j++) {
            const size_t a = even <= c ? open.size() * j / m : (size_t)c * j, b = even <= c ? open.size() * (j + 1) / m : (size_t)c * (j + 1);
            chunk[j].assign(open.begin() + a, open.begin() + b);
        }
        std::vector<std::vector<uint32_t>> cand(m);       // positions in K
        std::vector<std::vector<int32_t>> cand_lits(m);
        for (uint32_t j = 0; j < m; j++) {
            std::vector<uint8_t> out(K.size(), 0);
            for (uint32_t i : chunk[j]) out[i] = 1;
            for (uint32_t i = 0; i < K.size(); i++) if (!out[i]) { cand[j].push_back(i); cand_lits[j].push_back(K[i]); }
        }
        if (!begun) {     // (m == N in the first round)
            std::vector<int32_t> assump;
            std::vector<uint64_t> assump_off{0};
            for (uint32_t j = 0; j < m; j++) { assump.insert(assump.end(), cand_lits[j].begin(), cand_lits[j].end()); assump_off.push_back(assump.size()); }
            begun = true;
            rc = sweep_begin(s, sw, assump, assump_off, N, false, &K0);
            if (rc) break;
        } else {
            for (uint32_t j = 0; j < m; j++) sweep_repose(s, sw, j, cand_lits[j]);
            for (uint32_t j = m; j < N; j++) { sw.pose(j, 0); sw.withdraw(j); }     // unused this round
            sweep_retarget(s, sw);
        }
        info.rounds++;
        info.candidates += m;
        // slices until the first UNSAT answer, or all answers
        for (;;) {
            bool any_unsat = false;
            for (uint32_t j = 0; j < m; j++) any_unsat = any_unsat || sw.results[j] == MI355SAT_UNSAT;
            if (any_unsat || sw.decided == N || !sw.active) break;
            if (s.interrupted.load() || *s.stop_flag || (budget > 0 && (int64_t)sw.conflicts >= budget)) { stop = true; break; }
            if ((rc = sweep_step(s, sw)) != 0) break;
        }
        if (rc) break;
        // SAT answers: the chunk's one literal, or what the model falsifies of it
        uint32_t n_sat = 0, new_crit = 0;
        std::vector<int32_t> winners;
        std::vector<uint32_t> wj;
        std::vector<std::vector<int32_t>> wchunks;
        for (uint32_t j = 0; j < m; j++) {
            if (sw.results[j] != MI355SAT_SAT) continue;
            n_sat++;
            if (chunk[j].size() == 1) { crit[chunk[j][0]] = 1; new_crit++; continue; }
            winners.push_back(sw.winner[j]);
            wj.push_back(j);
            wchunks.emplace_back();
            for (uint32_t i : chunk[j]) wchunks.back().push_back(K[i]);
        }
        info.candidates_sat += n_sat;
        if (!winners.empty()) {
            std::vector<std::vector<std::vector<uint32_t>>> falsified;
            if ((rc = core_models(s, sw, winners, wchunks, falsified, info)) != 0) break;
            for (size_t k = 0; k < winners.size(); k++) {
                if (falsified[k].empty()) { set_error(&s, "device solver internal error (a model satisfies a refuted core)"); rc = MI355SAT_ERR_STATE; break; }
                // several of the caller's literals on one device literal (repeats, equivalent literals): none is critical alone
                if (falsified[k].size() != 1 || falsified[k][0].size() != 1) continue;
                crit[chunk[wj[k]][falsified[k][0][0]]] = 1;
                new_crit++;
                info.critical_by_model++;
            }
            if (rc) break;
        }
        // UNSAT answers: the smallest of their cores is the new K
        int best = -1;
        std::vector<uint32_t> F;
        for (uint32_t j = 0; j < m; j++) {
            if (sw.results[j] != MI355SAT_UNSAT) continue;
            info.candidates_unsat++;
            std::vector<uint32_t> f;
            for (size_t k = 0; k < cand[j].size(); k++) if (sw.core_flag[j][k]) f.push_back(cand[j][k]);
            if (best < 0 || f.size() < F.size()) { best = (int)j; F.swap(f); }
        }
        if (best >= 0) {
            std::vector<int32_t> K2;
            std::vector<uint8_t> crit2, in(K.size(), 0);
            for (uint32_t i : F) { in[i] = 1; K2.push_back(K[i]); crit2.push_back(crit[i]); }
            for (uint32_t i = 0; i < K.size(); i++)
                if (crit[i] && !in[i]) { set_error(&s, "device solver internal error (a core without a critical literal)"); rc = MI355SAT_ERR_STATE; }
            if (rc) break;
            K.swap(K2);
            crit.swap(crit2);
        } else if (!stop && new_crit == 0) c = std::max<uint64_t>(1, c / 2);
    }
    info.conflicts = sw.conflicts;
    if (begun) sweep_end(s, sw);
    else consume_interrupt(s);
    return rc;
}

// core: the handle's core to minimise in place.  Returns 0 or a negative error.
int minimize_core_impl(mi355sat* s, Core& core, int64_t conflict_budget, mi355sat_core_min_info* out) {
    mi355sat_core_min_info info{};
    info.size_before = info.size_after = core.lits.size();
    const double t0 = now_s();
    int rc = 0;
    if (s->interrupted.load()) consume_interrupt(*s);                 // stopped at once: the core as it is
    else if (core.minimal || core.lits.empty()) { info.minimal = 1; core.minimal = true; }
    else if (core.lits.size() == 1 && s->sat_clauses == s->offs.size()) { info.minimal = 1; core.minimal = true; }   // the formula alone has a model
    else {
        go_cold(*s, MI355SAT_COLD_OTHER_SEARCH);                      // "another search in between" for the warm mode
        const mi355sat_opts opts = s->opts;
        const mi355sat_stats_t st0 = s->stats;
        std::string proof_path;
        proof_path.swap(s->proof_path);                               // the proof of the solve is closed: nothing is logged
        s->opts.cube_split = 0;                                       // candidates are whole instances, one core each
        std::vector<int32_t> K = core.lits;
        rc = guarded(s, GUARD_TIMED, [&] { return minimize_search(*s, K, conflict_budget, info); });
        s->opts = opts;
        s->proof_path.swap(proof_path);
        keep_last_solve_stats(s->stats, st0);                         // (not this upload's)
        if (!rc) {
            core.lits.swap(K);
            core.minimal = info.minimal != 0;
            info.size_after = core.lits.size();
        }
    }
    info.seconds = now_s() - t0;
    if (out) *out = info;
    return rc;
}


// ---- DRUP proof check (mi355sat_check_proof) --------------------------------------------------------------------------
// Host side of ms_rup_kernel: the proof as lemmas (the target last), validated against the handle's variables before
// anything is uploaded; the formula prepared WITHOUT simplification in the caller's variable order (the trusted base);
// the slab's learnt store sized from the proof; one contiguous segment of the lemma list per worker; launches until every
// worker is done, the interrupt flag polled between them.  DESIGN.md §4.
struct ProofLemmas {
    std::vector<int32_t> lits;         // DIMACS literals of all lemmas, then the target's
    std::vector<uint64_t> offs{0};     // n_lemmas + 2 entries once the target is appended
    uint64_t n_lemmas = 0, n_deletions = 0;
    // with mi355sat_proof_deletions on: the deletion lines (DIMACS literals) and the item each stands in front of
    bool keep_deletions = false;
    std::vector<int32_t> del_lits;
    std::vector<uint64_t> del_offs{0}, del_at;
};

// The clauses a check must derive: target t = lits[offs[t] .. offs[t + 1]), DIMACS literals; valid (may be null) receives
// one verdict per target (mi355sat_check_proof_targets).  mi355sat_check_proof's one target is the case n = 1.
struct ProofTargets {
    const int32_t* lits;
    const uint64_t* offs;
    uint64_t n;
    int32_t* valid;
};

// One check as it passes from stage to stage of check_proof_impl.
struct ProofCheck {
    ProofLemmas& pf;                   // the proof; proof_target appends the targets as items n_lemmas ..
    mi355sat_proof_info& info;
    const ProofTargets& tg;
    uint32_t n_items = 0, n_targets = 0;   // the lemmas and the targets; the targets
    DevBuf<uint8_t> d_tfail;           // per target: a worker found it not RUP
    Prepared P;                        // the caller's clauses: not simplified, in the caller's variable order
    // the proof as the device reads it (proof_device_form)
    std::vector<int32_t> dl;           // device literals item by item, each variable at most once per item
    std::vector<uint32_t> doff{0};
    std::vector<uint8_t> skip;         // per item: it holds x and ~x - true whatever the assignment, never checked
    uint64_t store_lits = 0;           // what the lemmas take in a worker's learnt store, each 16-byte aligned
    // deletion lines honoured (proof_resolve_deletions): per lemma the item it dies in front of, per item "a group here"
    bool del = false;
    std::vector<uint32_t> death;
    std::vector<uint8_t> group;
    uint64_t lock_slack = 0, lock_slack_words = 0;   // room for dead lemmas a worker keeps because they are locked
    DevBuf<uint32_t> d_death;
    // on the device (proof_upload): S segments of the item list, one worker each
    uint32_t S = 0;
    DevBuf<int32_t> d_lits;
    DevBuf<uint32_t> d_offs;
    DevBuf<uint8_t> d_skip;
    DevBuf<unsigned long long> d_mins; // complements of the first failed lemma and of the point of refutation
    bool interrupted = false;          // proof_launches stopped at the interrupt flag
};

// proof: flat words (mi355sat.h).  Returns 0 or MI355SAT_ERR_ARG with a text.
int parse_proof_words(mi355sat& s, const int32_t* proof, uint64_t n_words, ProofLemmas& out) {
    uint64_t i = 0;
    while (i < n_words) {
        const bool del = proof[i] == INT32_MIN;
        if (del) i++;
        const uint64_t st = i;
        while (i < n_words && proof[i] != 0) {
            if (proof[i] == INT32_MIN) { s.err = "proof: a deletion marker inside a clause"; return MI355SAT_ERR_ARG; }
            if (var_of(proof[i]) > s.max_var) { s.err = "proof: a variable the handle does not have"; return MI355SAT_ERR_ARG; }
            i++;
        }
        if (i == n_words) { s.err = "proof: the last clause is not terminated"; return MI355SAT_ERR_ARG; }
        if (del) {
            out.n_deletions++;
            if (out.keep_deletions) {
                out.del_lits.insert(out.del_lits.end(), proof + st, proof + i);
                out.del_offs.push_back(out.del_lits.size());
                out.del_at.push_back(out.n_lemmas);
            }
        } else {
            out.lits.insert(out.lits.end(), proof + st, proof + i);
            out.offs.push_back(out.lits.size());
            out.n_lemmas++;
        }
        i++;   // the 0
    }
    return 0;
}

// DRUP text -> flat words as dimacs.read_drup makes them.
int read_proof_file(mi355sat& s, const char* path, std::vector<int32_t>& words) {
    FILE* f = fopen(path, "r");
    if (!f) { s.err = std::string("cannot open proof file ") + path; return MI355SAT_ERR_ARG; }
    std::string text;
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    const char* p = text.c_str();
    bool line_start = true, open_clause = false;
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\r') p++;
        if (*p == '\n') { p++; line_start = true; continue; }
        if (!*p) break;
        if (*p == 'd' && line_start && !open_clause) { words.push_back(INT32_MIN); p++; line_start = false; open_clause = true; continue; }
        char* end = nullptr;
        const long long v = strtoll(p, &end, 10);
        if (end == p || v <= INT32_MIN || v > INT32_MAX) { s.err = std::string("malformed proof file ") + path; return MI355SAT_ERR_ARG; }
        words.push_back((int32_t)v);
        open_clause = v != 0;
        line_start = false;
        p = end;
    }
    return 0;
}

// One launch of the checker over all segments; mt.log set: the tracing build (a trim).
SliceResult launch_rup(mi355sat& s, const ProofCheck& C, const MsTrace& mt) {
    const uint32_t active = C.S, chunk = s.proof_chunk;
    MsParams prm{};
    prm.n_workers = active;
    prm.max_groups = s.opts.max_groups > 0 ? s.opts.max_groups : MS_MAX_GROUPS;
    prm.slice_conflicts = chunk ? chunk : 0xffffffffu;         // lemmas per worker and launch
    prm.slice_ticks = chunk ? 0 : 20ull * 100000ull;           // ... or 20 ms
    prm.stop_flag = s.stop_flag;
    const mi355sat_search_build build = choose_build(active, s.lds_val_bytes, s.lds_val, s.opts.lds_val, s.opts.one_per_simd, 1);
    return timed_launch(s, [&] {
        with_flag(build.lds != 0, [&](auto lds_build) {
            with_flag(mt.log != nullptr, [&](auto traced) {
                with_flag(C.del, [&](auto deleting) {
                    hipLaunchKernelGGL((ms_rup_kernel<decltype(lds_build)::value, decltype(traced)::value, decltype(deleting)::value>), dim3(active),
                                       dim3(MS_WAVE), build.dyn_lds_bytes, s.stream, s.sh, s.L, s.d_slabs.p, prm, (const int32_t*)C.d_lits.p,
                                       (const uint32_t*)C.d_offs.p, (const uint8_t*)C.d_skip.p, C.n_items, C.d_mins.p, mt,
                                       (const uint32_t*)C.d_death.p, C.n_items - C.n_targets, C.d_tfail.p);
                });
            });
        });
    }, [] {});
}

// ---- trimming a checked proof (mi355sat_trim_proof) -----------------------------------------------------------------------
// The traced check's host side: the device names what a check rested on by what the worker holds - a long clause's index,
// the literals of a binary or ternary clause, a unit's literal, a lemma's index; here those become the caller's clause
// indices and lemma indices, one list per checked item in the order a checker has to propagate them (the trail positions).
// normalise / build_csr drop tautologies and duplicates: a clause that occurs twice is named by its lowest index.
struct TrimRun {
    uint32_t flags = 0;
    mi355sat_trim_info* out = nullptr;
    uint64_t n_clauses = 0;
    // device identity -> caller clause index (identity_order: a device literal is the caller's, 2 * (var - 1) + neg)
    std::vector<uint64_t> long_idx;
    std::map<std::array<int32_t, 3>, uint64_t> short_idx;       // sorted literals; a binary clause's third is INT32_MAX
    std::unordered_map<int32_t, uint64_t> unit_idx;
    // what the device reported: ids (caller clause i: i; lemma j: n_clauses + j) in hint order
    std::vector<std::vector<uint64_t>> deps;
    std::vector<uint8_t> have;
    struct Refutation { std::vector<uint64_t> ids; std::vector<int32_t> implied; };   // implied: the literal each clause gave, -1: the conflict
    std::map<uint64_t, Refutation> refuted;                       // by the item the worker stood in front of
    DevBuf<uint32_t> d_log, d_used;
    uint32_t words = 0;
    MsTrace mt{};                      // what the tracing build of ms_rup_kernel gets (trim_begin)
};

static std::array<int32_t, 3> short_key(int32_t a, int32_t b, int32_t c) {
    std::array<int32_t, 3> k{a, b, c};
    std::sort(k.begin(), k.end());
    return k;
}

// The reverse maps, clause by clause as normalise sees them.  Returns where normalise stops (an empty clause, or a
// unit against an earlier unit), the clause or the pair that is - the whole core when the formula falls before any launch.
std::vector<uint64_t> trim_maps(const mi355sat& s, TrimRun& T) {
    std::vector<uint64_t> unsat_core;
    std::vector<int32_t> tmp;
    T.n_clauses = s.offs.size() - 1;
    for (uint64_t c = 0; c < T.n_clauses; c++) {
        tmp.clear();
        for (uint64_t k = s.offs[c]; k < s.offs[c + 1]; k++) tmp.push_back(to_internal(s.lits[k]));
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        bool taut = false;
        for (size_t i = 0; i + 1 < tmp.size(); i++) taut = taut || (tmp[i] ^ 1) == tmp[i + 1];
        if (taut) continue;
        if (tmp.empty()) { if (unsat_core.empty()) unsat_core = {c}; }
        else if (tmp.size() == 1) {
            auto other = T.unit_idx.find(tmp[0] ^ 1);
            if (other != T.unit_idx.end() && unsat_core.empty()) unsat_core = {other->second, c};
            T.unit_idx.emplace(tmp[0], c);
        } else if (tmp.size() == 2) T.short_idx.emplace(short_key(tmp[0], tmp[1], INT32_MAX), c);
        else if (tmp.size() == 3) T.short_idx.emplace(short_key(tmp[0], tmp[1], tmp[2]), c);
        else T.long_idx.push_back(c);
    }
    return unsat_core;
}

int trim_fail(mi355sat& s, const char* what) {
    s.err = std::string("proof trim: ") + what;
    return MI355SAT_ERR_HIP;
}

// The dependency log's words per worker: the test hook's or the rule's, never below two items of the largest size - a worker
// ends its launch when its region has less room than that.
uint32_t trim_log_words(const mi355sat& s, uint32_t n_vars, uint32_t S) {
    const uint64_t floor_words = 2 * MS_TR_ITEM_WORDS(n_vars);
    const uint64_t rule = std::min<uint64_t>(1u << 18, (1u << 26) / S);
    return (uint32_t)std::max<uint64_t>(floor_words, s.trim_log_words ? s.trim_log_words : rule);
}

// The trim before the launch: the reverse maps and the dependency log.
void trim_begin(mi355sat& s, TrimRun& T, const ProofCheck& C) {
    trim_maps(s, T);
    T.words = trim_log_words(s, C.P.n_vars, C.S);
    T.out->log_words_per_worker = T.words;
    T.d_log.alloc((size_t)C.S * T.words);
    T.d_used.upload(std::vector<uint32_t>(C.S, 0u), s.stream);
    T.deps.assign(C.n_items, {});
    T.have.assign(C.n_items, 0);
    T.mt = MsTrace{T.d_log.p, T.d_used.p, T.words, 0};
}

// After every launch: each worker's region of the dependency log parsed and mapped, the cursors reset.
int trim_drain(mi355sat& s, TrimRun& T, uint32_t S, uint32_t n_items) {
    std::vector<uint32_t> used(S), buf;
    HIPCHK(hipMemcpy(used.data(), T.d_used.p, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool any = false;
    std::vector<std::array<int64_t, 3>> recs;        // pos, id, implied
    for (uint32_t w = 0; w < S; w++) {
        if (!used[w]) continue;
        any = true;
        if (used[w] > T.words || used[w] % MS_TR_REC) return trim_fail(s, "a log cursor out of range");
        buf.resize(used[w]);
        HIPCHK(hipMemcpy(buf.data(), T.d_log.p + (size_t)w * T.words, (size_t)used[w] * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < buf.size();) {
            const uint32_t item = buf[i] & ~MS_TR_REFUTED, n = buf[i + 1];
            const bool refuted = (buf[i] & MS_TR_REFUTED) != 0;
            if (item >= n_items + (refuted ? 1u : 0u) || (uint64_t)n > (uint64_t)s.L.n_vars + 2 || i + MS_TR_REC * ((size_t)n + 1) > buf.size())
                return trim_fail(s, "a malformed log item");
            recs.clear();
            for (uint32_t r = 0; r < n; r++) {
                const int32_t* x = (const int32_t*)&buf[i + MS_TR_REC * ((size_t)r + 1)];
                const uint32_t tag = (uint32_t)x[0] >> 28;
                const int64_t pos = x[0] & 0x0fffffff;
                int64_t id = -1, implied = -1;
                if (tag == MS_TR_LONG) { if ((uint32_t)x[1] < T.long_idx.size()) id = (int64_t)T.long_idx[x[1]]; implied = x[3]; }
                else if (tag == MS_TR_BIN || tag == MS_TR_TERN) {
                    auto it = T.short_idx.find(short_key(x[1], x[2], tag == MS_TR_BIN ? INT32_MAX : x[3]));
                    if (it != T.short_idx.end()) id = (int64_t)it->second;
                    implied = x[1];
                } else if (tag == MS_TR_UNIT) {
                    auto it = T.unit_idx.find(x[1]);
                    if (it != T.unit_idx.end()) id = (int64_t)it->second;
                    implied = x[1];
                } else if (tag == MS_TR_LEMMA || tag == MS_TR_UNIT_LEMMA) {
                    if ((uint32_t)x[1] < item) id = (int64_t)(T.n_clauses + (uint32_t)x[1]);
                    implied = x[3];
                }
                if (id < 0) return trim_fail(s, "a record names no clause of the caller and no earlier lemma");
                recs.push_back({pos, id, implied});
            }
            std::sort(recs.begin(), recs.end());
            std::vector<uint64_t> ids;
            for (auto& r : recs) ids.push_back((uint64_t)r[1]);
            if (refuted) {
                TrimRun::Refutation& R = T.refuted[item];
                R.ids.swap(ids);
                R.implied.clear();
                for (size_t k = 0; k < recs.size(); k++) R.implied.push_back(k + 1 == recs.size() ? -1 : (int32_t)recs[k][2]);
            } else {
                T.deps[item].swap(ids);
                T.have[item] = 1;
            }
            T.out->dep_records += n;
            i += MS_TR_REC * ((size_t)n + 1);
        }
    }
    if (any) {
        T.out->log_drains++;
        HIPCHK(hipMemsetAsync(T.d_used.p, 0, S * sizeof(uint32_t), s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
    }
    return 0;
}

// The one way a trim result reaches the handle: the core, the needed lemmas (ascending), and as lines those lemmas and the
// target, each (with hints) with the ids it rests on as LRAT numbers - a lemma's as traced, the target's given.
void trim_publish(mi355sat& s, TrimRun& T, const ProofLemmas& pf, std::vector<uint64_t> core, std::vector<uint64_t> lemmas,
                  const std::vector<uint64_t>& target_ids, bool no_lines) {
    mi355sat::Trim& R = s.trim;
    R.drop();
    R.no_lines = no_lines;
    R.n_clauses = T.n_clauses;
    R.n_lemmas = pf.n_lemmas;
    R.hints = (T.flags & MI355SAT_TRIM_HINTS) != 0;
    std::sort(core.begin(), core.end());
    R.core.swap(core);
    R.lemmas.swap(lemmas);
    auto line = [&](uint64_t j, const std::vector<uint64_t>& ids) {
        R.lits.insert(R.lits.end(), pf.lits.begin() + pf.offs[j], pf.lits.begin() + pf.offs[j + 1]);
        R.offs.push_back(R.lits.size());
        if (!R.hints) return;
        R.hint.emplace_back();
        for (uint64_t id : ids) R.hint.back().push_back(id + 1);
    };
    for (uint64_t j : R.lemmas) line(j, T.deps[j]);
    line(pf.n_lemmas, target_ids);
    R.valid = true;
    T.out->core_clauses = R.core.size();
    T.out->lemmas_needed = R.lemmas.size();
}

// From the target backwards: a needed item's clauses enter the core, its lemmas become needed.  (The target's device
// literals decide which hints of a level-0 refutation a non-empty target keeps.)
int trim_reach(mi355sat& s, TrimRun& T, const ProofCheck& C) {
    const uint64_t nl = C.pf.n_lemmas, nc = T.n_clauses, refuted_at = C.info.refuted_at;
    const bool taut = C.skip[nl] != 0;           // a tautological target: nothing to derive, no lines
    std::vector<uint8_t> needed(nl, 0), core(nc, 0);
    std::vector<uint64_t> target_ids;
    if (!taut && refuted_at != UINT64_MAX) {
        auto it = T.refuted.find(refuted_at);
        if (it == T.refuted.end()) return trim_fail(s, "no worker traced the refutation");
        // under the negated target a clause whose literal the target assumes is satisfied, and one that gives a literal of
        // the target ends the derivation
        std::unordered_map<int32_t, int> tl;
        for (uint32_t k = C.doff[nl]; k < C.doff[nl + 1]; k++) tl[C.dl[k]] = 1;
        for (size_t k = 0; k < it->second.ids.size(); k++) {
            const int32_t x = it->second.implied[k];
            if (x >= 0 && tl.count(x ^ 1)) continue;
            target_ids.push_back(it->second.ids[k]);
            if (x >= 0 && tl.count(x)) break;
        }
    } else if (!taut) {
        if (!T.have[nl]) return trim_fail(s, "the target's check was not traced");
        target_ids = T.deps[nl];
    }
    const uint64_t upper = std::min(nl, refuted_at);
    auto use = [&](const std::vector<uint64_t>& ids, uint64_t below) {
        for (uint64_t id : ids) {
            if (id < nc) core[id] = 1;
            else if (id - nc < below) needed[id - nc] = 1;
            else return false;
        }
        return true;
    };
    if (!use(target_ids, upper)) return trim_fail(s, "the target rests on a lemma behind the refutation");
    for (uint64_t j = upper; j-- > 0;) {
        if (!needed[j]) continue;
        if (!T.have[j]) return trim_fail(s, "a needed lemma's check was not traced");
        if (!use(T.deps[j], j)) return trim_fail(s, "a lemma rests on a later one");
    }
    std::vector<uint64_t> core_ids, lemma_ids;
    for (uint64_t c = 0; c < nc; c++) if (core[c]) core_ids.push_back(c);
    for (uint64_t j = 0; j < nl; j++) if (needed[j]) lemma_ids.push_back(j);
    trim_publish(s, T, C.pf, core_ids, lemma_ids, target_ids, taut);
    return 0;
}

// The trim after a verdict "valid": the reach - or, where the caller's clauses fell before any launch (an empty clause,
// contradictory units), that clause or that pair as the core and as the hints of the one line, the target's.
int trim_finish(mi355sat& s, TrimRun& T, const ProofCheck& C) {
    if (!C.P.unsat) return trim_reach(s, T, C);
    const std::vector<uint64_t> unsat_core = trim_maps(s, T);
    if (unsat_core.empty()) return trim_fail(s, "the refuting clauses were not found");
    trim_publish(s, T, C.pf, unsat_core, {}, unsat_core, false);
    return 0;
}

// ---- the stages of a check (check_proof_impl runs them in this order) ----------------------------------------------------------
// 1. The target: validated, appended as the last item; the sizes a worker's clause store can index.
int proof_target(mi355sat& s, ProofCheck& C) {
    ProofLemmas& pf = C.pf;
    const ProofTargets& tg = C.tg;
    const int32_t* target = tg.lits + (tg.n ? tg.offs[0] : 0);
    const uint64_t n_target = tg.offs[tg.n] - tg.offs[0];
    for (uint64_t t = 0; t < tg.n; t++)
        if (tg.offs[t + 1] < tg.offs[t]) { s.err = "proof target: offsets not monotone"; return MI355SAT_ERR_ARG; }
    for (uint64_t i = 0; i < n_target; i++) {
        if (target[i] == 0 || target[i] == INT32_MIN) { s.err = "proof target: literal 0 inside a clause"; return MI355SAT_ERR_ARG; }
        if (var_of(target[i]) > s.max_var) { s.err = "proof target: a variable the handle does not have"; return MI355SAT_ERR_ARG; }
    }
    if (pf.n_lemmas + tg.n + 1 > 0x7fffffffull || pf.lits.size() + n_target + 5 * (pf.n_lemmas + tg.n + 1) > 0x7ffffff0ull) {
        s.err = "proof too large for a worker's clause store";
        return MI355SAT_ERR_OOM;
    }
    pf.lits.insert(pf.lits.end(), target, target + n_target);
    for (uint64_t t = 0; t < tg.n; t++) pf.offs.push_back(pf.offs[pf.n_lemmas] + (tg.offs[t + 1] - tg.offs[0]));
    C.n_targets = (uint32_t)tg.n;
    C.n_items = (uint32_t)(pf.n_lemmas + tg.n);  // target t is item number n_lemmas + t
    C.info.n_lemmas = pf.n_lemmas;
    C.info.n_deletions_ignored = pf.n_deletions;
    C.info.first_failed = C.info.refuted_at = UINT64_MAX;
    return 0;
}

// 1b. (mi355sat_proof_deletions) The deletion lines resolved as include/mi355sat.h defines it: which lemma each one names,
// hence per lemma the item it dies in front of and per item whether a group stands there; the counts and the peak of Live,
// which are functions of the proof alone; the room for locked clauses.  Clauses compare as literal sets: sorted by
// variable, repeats dropped.  Lemmas are found through a hash of that form - per hash the live lemma lines, latest last -
// and compared literal by literal; the caller's clauses get their table only when a line finds no lemma.
void proof_resolve_deletions(mi355sat& s, ProofCheck& C) {
    const ProofLemmas& pf = C.pf;
    mi355sat_proof_del_info& D = s.proof_del_info;
    D = mi355sat_proof_del_info{};
    s.proof_del_have = true;
    C.del = true;
    const uint64_t nl = pf.n_lemmas;
    C.death.assign(C.n_items, UINT32_MAX);
    C.group.assign(C.n_items, 0);
    std::vector<int32_t> a, b;
    auto canon = [](const int32_t* p, const int32_t* e, std::vector<int32_t>& out) {     // returns: x and ~x
        out.assign(p, e);
        std::sort(out.begin(), out.end(), [](int32_t x, int32_t y) { return std::abs(x) != std::abs(y) ? std::abs(x) < std::abs(y) : x < y; });
        out.erase(std::unique(out.begin(), out.end()), out.end());
        bool taut = false;
        for (size_t i = 0; i + 1 < out.size(); i++) taut = taut || out[i] == -out[i + 1];
        return taut;
    };
    auto hash = [](const std::vector<int32_t>& v) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (int32_t x : v) h = (h ^ (uint32_t)x) * 0x100000001b3ull;
        return h;
    };
    std::vector<uint32_t> words(nl, 0);           // per lemma: its room in the store
    std::vector<uint8_t> joins(nl, 0);            // ... and whether it ever is in Live (a tautology is not)
    std::unordered_map<uint64_t, std::vector<uint32_t>> live;
    std::unordered_map<uint64_t, std::vector<uint64_t>> orig;
    bool have_orig = false;
    std::vector<uint32_t> dead_words;
    uint64_t n_live = 0, w_live = 0, di = 0;
    const uint64_t nd = pf.del_at.size();
    for (uint64_t j = 0; j <= nl; j++) {
        if (di < nd && pf.del_at[di] == j) D.groups++;
        for (; di < nd && pf.del_at[di] == j; di++) {
            canon(pf.del_lits.data() + pf.del_offs[di], pf.del_lits.data() + pf.del_offs[di + 1], a);
            const uint64_t h = hash(a);
            auto it = live.find(h);
            bool found = false;
            if (it != live.end())
                for (size_t k = it->second.size(); k-- > 0 && !found;) {
                    const uint32_t i = it->second[k];
                    canon(pf.lits.data() + pf.offs[i], pf.lits.data() + pf.offs[i + 1], b);
                    if (a != b) continue;
                    found = true;
                    it->second.erase(it->second.begin() + k);
                    D.honoured++;
                    if (!joins[i]) continue;          // a tautology: never attached
                    C.death[i] = (uint32_t)j;
                    C.group[j] = 1;
                    n_live--;
                    w_live -= words[i];
                    dead_words.push_back(words[i]);
                }
            if (found) continue;
            if (!have_orig) {
                have_orig = true;
                for (uint64_t c = 0; c + 1 < s.offs.size(); c++) {
                    canon(s.lits.data() + s.offs[c], s.lits.data() + s.offs[c + 1], b);
                    orig[hash(b)].push_back(c);
                }
            }
            auto io = orig.find(h);
            if (io != orig.end())
                for (uint64_t c : io->second) {
                    canon(s.lits.data() + s.offs[c], s.lits.data() + s.offs[c + 1], b);
                    if (a == b) { found = true; break; }
                }
            if (found) D.ignored_original++;
            else D.ignored_unmatched++;
        }
        if (j == nl) break;                           // the target never joins
        const bool taut = canon(pf.lits.data() + pf.offs[j], pf.lits.data() + pf.offs[j + 1], a);
        live[hash(a)].push_back((uint32_t)j);
        if (taut) continue;
        joins[j] = 1;
        words[j] = (uint32_t)((a.size() + 3) & ~(size_t)3);
        n_live++;
        w_live += words[j];
        D.peak_live_lemmas = std::max(D.peak_live_lemmas, n_live);
        D.peak_live_words = std::max(D.peak_live_words, w_live);
    }
    // a worker keeps a dead lemma that is the reason of a level-0 fact: one per variable at most, the longest at worst
    C.lock_slack = std::min<uint64_t>((uint64_t)s.max_var + 1, dead_words.size());
    std::sort(dead_words.begin(), dead_words.end(), std::greater<uint32_t>());
    for (uint64_t k = 0; k < C.lock_slack; k++) C.lock_slack_words += dead_words[k];
    C.info.n_deletions_ignored = D.ignored_original + D.ignored_unmatched;
}

// 2. The answers that need no launch (an interrupt is consumed before the slabs are given up).  true: info.valid has one.
bool proof_without_launch(mi355sat& s, ProofCheck& C) {
    if (s.interrupted.load()) {      // as a solve: an interrupt that came before the call stops it at once
        consume_interrupt(s);
        C.info.valid = -1;           // (check_proof_impl returns MI355SAT_INTERRUPTED for it)
        return true;
    }
    go_cold(s, MI355SAT_COLD_OTHER_SEARCH);      // (the slabs become this check's)
    s.ph.on_device = false;
    prepare(s, /*simplify=*/false, C.P, /*identity_order=*/true);
    if (C.P.unsat) {             // an empty clause or contradictory units among the caller's clauses
        C.info.refuted_at = 0;
        C.info.valid = 1;
    } else if (C.P.n_vars == 0) {    // no variable, no clause: only empty lemmas are possible, and none is RUP
        C.info.first_failed = 0;
        C.info.valid = 0;
    } else return false;
    return true;
}

// 3. The proof as the device reads it.  An item's own literal order is kept - a solver writes the asserting literal first,
// and the first two free literals become the watches: sorted, the lists of the lowest variables would hold most of the proof.
void proof_device_form(ProofCheck& C) {
    const ProofLemmas& pf = C.pf;
    C.skip.assign(C.n_items, 0);
    C.dl.reserve(pf.lits.size() + 4);
    std::vector<int32_t> tmp;
    std::vector<uint32_t> stamp(C.P.n_vars, 0);     // per variable: 2 * (j + 1) | sign of its literal in lemma j
    for (uint32_t j = 0; j < C.n_items; j++) {
        tmp.clear();
        for (uint64_t k = pf.offs[j]; k < pf.offs[j + 1]; k++) {
            const int32_t l = to_device(C.P.perm, pf.lits[k]);
            uint32_t& st = stamp[l >> 1];
            if ((st >> 1) != j + 1) { st = 2 * (j + 1) | (uint32_t)(l & 1); tmp.push_back(l); }
            else if ((st & 1u) != (uint32_t)(l & 1)) C.skip[j] = 1;
        }
        if (C.skip[j]) tmp.clear();
        C.dl.insert(C.dl.end(), tmp.begin(), tmp.end());
        C.doff.push_back((uint32_t)C.dl.size());
        if (j < C.n_items - C.n_targets) C.store_lits += (tmp.size() + 3) & ~(size_t)3;     // (a target takes no room)
    }
    for (int k = 0; k < 4; k++) C.dl.push_back(0);
}

// 4. The formula to the device with a learnt store that holds every lemma (each 16-byte aligned; add_learnt wants 8 words
// of headroom), one worker per segment with its script - cursor, a, b, pad, checked (64 bit), attached (64 bit) - and
// the proof behind it.  With deletion lines honoured the stores hold the peak of the live lemmas and the locked ones
// (proof_resolve_deletions) instead of every lemma, the script has words [8] / [9] for the pass counters, and death[] goes
// along.
void proof_upload(mi355sat& s, ProofCheck& C, uint32_t segments) {
    mi355sat_proof_del_info& D = s.proof_del_info;
    const uint32_t learnt_cap = C.del ? (uint32_t)std::max<uint64_t>(1, D.peak_live_lemmas + C.lock_slack) : (uint32_t)C.pf.n_lemmas + 1;
    const uint32_t learnt_lit_cap = (uint32_t)((C.del ? D.peak_live_words + C.lock_slack_words : C.store_lits) + 16);
    const uint32_t script_words = C.del ? 12 : 8;
    uint32_t S = std::min(segments ? segments : fleet_size(s), C.n_items);
    upload_formula(s, C.P, 0, script_words, S, 0, learnt_cap, learnt_lit_cap, MI355SAT_ERR_OOM);
    if (C.del) {
        D.learnt_cap = s.L.learnt_cap; D.learnt_lit_cap = s.L.learnt_lit_cap; D.pool_cap = s.L.pool_cap;
        C.d_death.upload(C.death, s.stream);
    }
    S = std::min(S, s.n_workers);                // (what device memory holds)
    s.n_workers = s.n_alloc = S;
    C.S = C.info.segments = C.info.workers = S;
    std::vector<int32_t> script;
    std::vector<uint64_t> soff{0};
    for (uint32_t w = 0; w < S; w++) {
        const int32_t a = (int32_t)((uint64_t)C.n_items * w / S), b = (int32_t)((uint64_t)C.n_items * (w + 1) / S);
        script.insert(script.end(), {0, a, b, 0, 0, 0, 0, 0});
        script.resize(script.size() + (script_words - 8), 0);
        soff.push_back(script.size());
    }
    reset_workers(s);
    customize(s, nullptr, nullptr, &script, &soff, S);
    C.d_lits.upload(C.dl, s.stream);
    C.d_offs.upload(C.doff, s.stream);
    std::vector<uint8_t> flags = C.skip;         // per item, bit 0: skip; bit 1 (the DEL builds): a group in front of it
    if (C.del) for (uint32_t j = 0; j < C.n_items; j++) if (C.group[j]) flags[j] |= 2;
    C.d_skip.upload(flags, s.stream);
    C.d_mins.upload(std::vector<unsigned long long>{0ull, 0ull}, s.stream);      // complements of "none"
    C.d_tfail.upload(std::vector<uint8_t>(C.n_targets, 0), s.stream);
}

// 5. Launches until no worker is running, the interrupt flag polled between them; a traced check's log drained after each.
int proof_launches(mi355sat& s, ProofCheck& C, TrimRun* T) {
    const double k0 = s.stats.kernel_seconds;
    std::vector<MsState> sts;
    for (;;) {
        if (s.interrupted.load()) { C.interrupted = true; break; }
        launch_rup(s, C, T ? T->mt : MsTrace{});
        C.info.launches++;
        gather_states(s, sts);
        if (T) if (int rc = trim_drain(s, *T, C.S, C.n_items)) return rc;
        bool running = false;
        for (uint32_t w = 0; w < C.S; w++) {
            if (sts[w].status < 0) return status_error(s, sts[w].status, MI355SAT_ERR_HIP, "proof check: ");
            running = running || sts[w].status == MS_ST_RUNNING;
        }
        if (!running) break;
    }
    C.info.kernel_seconds = s.stats.kernel_seconds - k0;
    for (const MsState& st : sts) C.info.propagations += st.propagations;
    return 0;
}

// 6. The workers' counters, and unless an interrupt ended the check (valid = -1) the verdict.
int proof_verdict(mi355sat& s, ProofCheck& C) {
    mi355sat_proof_info& info = C.info;
    if (info.launches) {
        const size_t sw = C.del ? 12 : 8;
        std::vector<int32_t> sc((size_t)C.S * sw);
        HIPCHK(hipMemcpy2D(sc.data(), 4 * sw, s.d_slabs.p + s.L.script, s.L.slab_bytes, 4 * sw, C.S, hipMemcpyDeviceToHost));
        for (uint32_t w = 0; w < C.S; w++) {
            uint64_t c[2];
            memcpy(c, &sc[(size_t)w * sw + 4], sizeof c);
            info.lemmas_checked += c[0];
            info.lemmas_attached += c[1];
            if (C.del) { s.proof_del_info.skipped_locked += (uint32_t)sc[w * sw + 8]; s.proof_del_info.compactions += (uint32_t)sc[w * sw + 9]; }
        }
    }
    if (C.interrupted) {
        consume_interrupt(s);
        info.valid = -1;
        return 0;
    }
    unsigned long long mins[2];
    HIPCHK(hipMemcpy(mins, C.d_mins.p, sizeof mins, hipMemcpyDeviceToHost));
    info.first_failed = ~mins[0];
    info.refuted_at = ~mins[1];
    // (a lemma behind the point of refutation is RUP whatever a worker that had not seen the refuting lemmas yet made of it:
    // a worker checks lemma j against ALL lemmas before j, so there is no such worker - kept as a cross-check)
    if (info.first_failed != UINT64_MAX && info.refuted_at <= info.first_failed) {
        s.err = "proof check: a lemma failed behind the point of refutation";
        return MI355SAT_ERR_HIP;
    }
    info.valid = info.first_failed == UINT64_MAX ? 1 : 0;
    if (C.tg.valid) {
        std::vector<uint8_t> fail(C.n_targets);
        HIPCHK(hipMemcpy(fail.data(), C.d_tfail.p, fail.size(), hipMemcpyDeviceToHost));
        for (uint32_t t = 0; t < C.n_targets; t++) C.tg.valid[t] = fail[t] ? 0 : 1;
    }
    return 0;
}

// T (may be null): mi355sat_trim_proof's traced check, which attaches before the launch (trim_begin), after each launch
// (trim_drain, in proof_launches) and after a verdict "valid" (trim_finish).
int check_proof_impl(mi355sat& s, ProofLemmas& pf, const ProofTargets& tg, uint32_t segments, mi355sat_proof_info& info, TrimRun* T) {
    ProofCheck C{pf, info, tg};
    if (tg.valid) std::fill(tg.valid, tg.valid + tg.n, -1);      // (what an interrupt leaves)
    if (int rc = proof_target(s, C)) return rc;
    if (s.proof_del) proof_resolve_deletions(s, C);
    if (proof_without_launch(s, C)) {      // refuted caller's clauses: every target holds; no variable: none does
        if (tg.valid && info.valid >= 0) std::fill(tg.valid, tg.valid + tg.n, info.valid);
    } else {
        proof_device_form(C);
        proof_upload(s, C, segments);
        if (T) trim_begin(s, *T, C);
        HIPCHK(hipStreamSynchronize(s.stream));
        if (int rc = proof_launches(s, C, T)) return rc;
        if (int rc = proof_verdict(s, C)) return rc;
    }
    if (info.valid < 0) return MI355SAT_INTERRUPTED;     // before the call or between two launches
    return T && info.valid == 1 ? trim_finish(s, *T, C) : 0;
}

// The one body of mi355sat_check_proof, _trim_proof and their _file variants (name: the entry's in its messages).  The words
// come from memory or, with a path, from a DRUP text file; trim (may be null): the traced check, whose result stays on the
// handle, instead of the plain one that fills `out`.
int proof_entry(mi355sat* s, const char* name, const int32_t* words, uint64_t n_words, const char* path, const ProofTargets& tg,
                uint32_t segments, mi355sat_proof_info* out, mi355sat_trim_info* trim = nullptr, uint32_t flags = 0) {
    if (s->sweep) { s->err = std::string(name) + "() called during a sweep"; return MI355SAT_ERR_STATE; }
    if (!s->pending.empty()) { s->err = std::string(name) + "() called inside an unterminated clause"; return MI355SAT_ERR_STATE; }
    ProofLemmas pf;
    pf.keep_deletions = s->proof_del;
    if (int rc = guarded(s, GUARD_HOST, [&] {
            std::vector<int32_t> text;
            if (!path) return parse_proof_words(*s, words, n_words, pf);
            if (int e = read_proof_file(*s, path, text)) return e;
            return parse_proof_words(*s, text.data(), text.size(), pf);
        })) return rc;
    // (every refusal above leaves an earlier trim_proof's result on the handle; a bad target is refused below, after the drop)
    mi355sat_proof_info info{};
    const double t0 = now_s();
    s->trim.drop();
    TrimRun T{flags, trim};          // (used by a trim only)
    if (trim) *trim = mi355sat_trim_info{};
    const int rc = guarded(s, GUARD_TIMED, [&] { return check_proof_impl(*s, pf, tg, segments, info, trim ? &T : nullptr); });
    if (rc < 0 || info.valid != 1) s->trim.drop();
    info.seconds = now_s() - t0;
    if (rc < 0) go_cold(*s, MI355SAT_COLD_FIRST);
    *(trim ? &trim->check : out) = info;
    return rc;
}

// ---- strict LRAT check (mi355sat_check_lrat) ------------------------------------------------------------------------------
// Host side of ms_lrat_kernel.  The file is parsed and validated before anything is uploaded; what is not LRAT at all is
// MI355SAT_ERR_ARG.  The database is the caller's clauses as they were added (no simplification, the caller's variables)
// with the file's lines behind them; every hint id is rewritten to a clause index of that database by binary search over
// the increasing line ids - an id that names neither an original nor an EARLIER line becomes MS_LRAT_NONE, which the device
// reports when the hint's turn comes.  The first line whose id is not above its predecessor's (the originals' for the
// first) ends what is uploaded: it is the first rejected line unless an earlier one is.  Lines go to the device in file
// order, in chunks; the first chunk with a rejection ends the call.  The call owns its device buffers and leaves the worker
// slabs, and with them everything a solve, a trim or the IPASIR state keeps, alone.  DESIGN.md §4.
struct LratFile {
    std::vector<uint64_t> ids;             // per line, as written
    std::vector<int32_t> lits;             // DIMACS literals line by line
    std::vector<uint64_t> loffs{0};
    std::vector<uint64_t> hints;           // ids as written, all > 0
    std::vector<uint64_t> hoffs{0};
};

// lines: flat words `id, literals, 0, hints, 0` (W = int32_t: the caller's array; int64_t: a text file's numbers).
template <class W>
int parse_lrat_words(mi355sat& s, const W* w, uint64_t n, LratFile& F) {
    uint64_t i = 0;
    while (i < n) {
        const int64_t id = (int64_t)w[i++];
        if (id <= 0) { s.err = id == INT32_MIN ? "lrat: a deletion marker" : "lrat: a line's id is not positive"; return MI355SAT_ERR_ARG; }
        for (; i < n && w[i] != 0; i++) {
            const int64_t l = (int64_t)w[i];
            if (l <= INT32_MIN || l > INT32_MAX) { s.err = "lrat: a literal out of range"; return MI355SAT_ERR_ARG; }
            if (var_of((int32_t)l) > s.max_var) { s.err = "lrat: a variable the handle does not have"; return MI355SAT_ERR_ARG; }
            F.lits.push_back((int32_t)l);
        }
        if (i == n) { s.err = "lrat: a line's clause is not terminated"; return MI355SAT_ERR_ARG; }
        i++;
        for (; i < n && w[i] != 0; i++) {
            if ((int64_t)w[i] < 0) { s.err = "lrat: a negative hint"; return MI355SAT_ERR_ARG; }
            F.hints.push_back((uint64_t)w[i]);
        }
        if (i == n) { s.err = "lrat: the last line's hints are not terminated"; return MI355SAT_ERR_ARG; }
        i++;
        F.ids.push_back((uint64_t)id);
        F.loffs.push_back(F.lits.size());
        F.hoffs.push_back(F.hints.size());
    }
    return 0;
}

// LRAT text, one line per clause -> the flat words.  A line must be whole: integers only (so `id d ...` is refused), the
// clause's 0, hints without a 0 among them, the closing 0.
int read_lrat_file(mi355sat& s, const char* path, std::vector<int64_t>& words) {
    FILE* f = fopen(path, "r");
    if (!f) { s.err = std::string("cannot open LRAT file ") + path; return MI355SAT_ERR_ARG; }
    std::string text;
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    const char* p = text.c_str();
    const char* const end_text = p + text.size();
    uint64_t line_no = 0;
    while (p < end_text) {
        line_no++;
        const size_t first = words.size();
        size_t zeros = 0;
        for (;;) {
            while (*p == ' ' || *p == '\t' || *p == '\r') p++;
            if (*p == '\n' || p >= end_text) break;
            char* end = nullptr;
            const long long v = strtoll(p, &end, 10);
            const bool whole = end != p && (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n' || end >= end_text);
            if (!whole || v < -(1ll << 62) || v > (1ll << 62)) {
                s.err = "lrat: line " + std::to_string(line_no) + (*p == 'd' ? " is a deletion line" : " is not a line of integers");
                return MI355SAT_ERR_ARG;
            }
            words.push_back(v);
            zeros += v == 0;
            p = end;
        }
        if (p < end_text) p++;      // the '\n'
        const size_t n = words.size() - first;
        if (n == 0) continue;
        // id, literals, 0, hints, 0: the first 0 behind the id ends the clause, the only other one ends the line
        if (words[first] <= 0) { s.err = "lrat: line " + std::to_string(line_no) + " has no positive id"; return MI355SAT_ERR_ARG; }
        if (n < 3 || words.back() != 0 || zeros != 2) {
            s.err = "lrat: line " + std::to_string(line_no) + (zeros > 2 ? " has a 0 among its hints" : " is not terminated");
            return MI355SAT_ERR_ARG;
        }
    }
    return 0;
}

inline bool same_literal_set(std::vector<int32_t> a, std::vector<int32_t> b) {
    std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end());
    std::sort(b.begin(), b.end()); b.erase(std::unique(b.begin(), b.end()), b.end());
    return a == b;
}

// Which build of ms_lrat_kernel runs: the assignment map in LDS (2 bits per variable, one wavefront per workgroup) when
// opts.lds_val forces it and a workgroup may have that much (64 KB), or on auto when 16 workgroups per CU fit the 150 KB the
// search builds budget; else one word per variable and wave in HBM.
inline uint32_t lrat_map_bytes(uint32_t n_vars) { return (uint32_t)align_up((size_t)((n_vars + 15) / 16) * 4, 16); }
inline bool lrat_in_lds(int opt_lds_val, uint32_t map_bytes) {
    if (opt_lds_val < 0) return false;
    return map_bytes <= (opt_lds_val > 0 ? 64u * 1024 : 150u * 1024 / 16);
}

int check_lrat_impl(mi355sat& s, const LratFile& F, const int32_t* target, uint64_t n_target, mi355sat_lrat_info& info) {
    for (uint64_t i = 0; i < n_target; i++) {
        if (target[i] == 0 || target[i] == INT32_MIN) { s.err = "lrat target: literal 0 inside a clause"; return MI355SAT_ERR_ARG; }
        if (var_of(target[i]) > s.max_var) { s.err = "lrat target: a variable the handle does not have"; return MI355SAT_ERR_ARG; }
    }
    const uint64_t n_orig = s.offs.size() - 1, n_lines = F.ids.size();
    info.n_lines = n_lines;
    info.n_hints = F.hints.size();
    // the target: a tautology needs no line; else the last line must be it
    const std::vector<int32_t> tg(target, target + n_target);
    bool taut = false;
    for (int32_t l : tg) taut = taut || std::find(tg.begin(), tg.end(), -l) != tg.end();
    if (taut) info.derives_target = 1;
    else if (n_lines) info.derives_target = same_literal_set(tg, std::vector<int32_t>(F.lits.begin() + F.loffs[n_lines - 1], F.lits.end())) ? 1 : 0;
    // the lines whose ids are in order: [0, n_up)
    uint64_t n_up = 0;
    for (uint64_t last = n_orig; n_up < n_lines && F.ids[n_up] > last; n_up++) last = F.ids[n_up];
    const uint64_t n_db_lits = s.lits.size() + F.loffs[n_up];
    // (the kernel forms `offset + lane` in 32 bits: the last offset stays a wavefront and more below 2^32)
    if (n_orig + n_up + 2 > 0xffffff00ull || n_up + 2 > (1ull << 30) || n_db_lits > 0xffffff00ull || F.hoffs[n_up] > 0xffffff00ull) {
        s.err = "lrat: the file is too large for the device's 32-bit indices";
        return MI355SAT_ERR_OOM;
    }
    const uint32_t n_vars = (uint32_t)std::max<uint64_t>(1, s.max_var);
    const uint32_t map_bytes = lrat_map_bytes(n_vars);
    const bool lds = lrat_in_lds(s.opts.lds_val, map_bytes);
    info.lds = lds ? 1 : 0;
    info.dyn_lds_bytes = lds ? map_bytes : 0;
    // the database: originals, then the lines; the hints as clause indices
    std::vector<int32_t> dl;
    std::vector<uint32_t> doff{0};
    dl.reserve(n_db_lits);
    doff.reserve(n_orig + n_up + 1);
    for (uint64_t c = 0; c < n_orig; c++) {
        for (uint64_t k = s.offs[c]; k < s.offs[c + 1]; k++) dl.push_back(to_internal(s.lits[k]));
        doff.push_back((uint32_t)dl.size());
        info.longest_clause = std::max<uint64_t>(info.longest_clause, s.offs[c + 1] - s.offs[c]);
    }
    for (uint64_t i = 0; i < n_up; i++) {
        for (uint64_t k = F.loffs[i]; k < F.loffs[i + 1]; k++) dl.push_back(to_internal(F.lits[k]));
        doff.push_back((uint32_t)dl.size());
        info.longest_clause = std::max<uint64_t>(info.longest_clause, F.loffs[i + 1] - F.loffs[i]);
    }
    std::vector<uint32_t> dh(F.hoffs[n_up]), dhoff(n_up + 1);
    for (uint64_t i = 0; i < n_up; i++) {
        dhoff[i] = (uint32_t)F.hoffs[i];
        for (uint64_t k = F.hoffs[i]; k < F.hoffs[i + 1]; k++) {
            const uint64_t h = F.hints[k];
            uint32_t idx = MS_LRAT_NONE;
            if (h <= n_orig) idx = (uint32_t)(h - 1);
            else {      // an earlier line (ids[0, i) increase strictly, and all are below this line's own)
                const auto it = std::lower_bound(F.ids.begin(), F.ids.begin() + i, h);
                if (it != F.ids.begin() + i && *it == h) idx = (uint32_t)(n_orig + (uint64_t)(it - F.ids.begin()));
            }
            dh[k] = idx;
        }
    }
    dhoff[n_up] = (uint32_t)F.hoffs[n_up];
    uint64_t rej_line = UINT64_MAX;
    uint32_t rej_reason = 0, rej_hint = MS_LRAT_NONE;
    // an interrupt that came before the call stops it here, whatever the file holds - also one that needs no launch
    bool interrupted = s.interrupted.load() != 0;
    DevBuf<uint32_t> d_used;
    const size_t used_words = std::max<size_t>(1, (n_orig + 31) / 32);
    if (n_up && !interrupted) {
        // one word per variable and wave holds the HBM build's map: at most 1 GiB of it
        const uint32_t grid_cap = lds ? 4096u : (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(64, (1ull << 28) / n_vars));
        DevBuf<int32_t> d_lits;
        DevBuf<uint32_t> d_offs, d_hints, d_hoffs, d_rec, d_map;
        d_lits.upload_nonempty(dl, s.stream);
        d_offs.upload(doff, s.stream);
        d_hints.upload_nonempty(dh, s.stream);
        d_hoffs.upload(dhoff, s.stream);
        d_used.alloc(used_words);
        HIPCHK(hipMemsetAsync(d_used.p, 0, used_words * 4, s.stream));
        d_rec.alloc((size_t)grid_cap * 4);
        HIPCHK(hipMemsetAsync(d_rec.p, 0xff, (size_t)grid_cap * 16, s.stream));
        if (!lds) {
            const size_t map_words = (size_t)std::min<uint64_t>(grid_cap, n_up) * n_vars;
            d_map.alloc(map_words);
            HIPCHK(hipMemsetAsync(d_map.p, 0, map_words * 4, s.stream));
        }
        HIPCHK(hipStreamSynchronize(s.stream));
        MsLrat A{};
        A.lits = d_lits.p; A.offs = d_offs.p; A.hints = d_hints.p; A.hoffs = d_hoffs.p;
        A.used = d_used.p; A.rec = d_rec.p; A.map = d_map.p;
        A.n_orig = (uint32_t)n_orig; A.n_vars = n_vars;
        const double k0 = s.stats.kernel_seconds;
        std::vector<uint32_t> rec;
        for (uint64_t a = 0; a < n_up && rej_line == UINT64_MAX;) {
            if (s.interrupted.load()) { interrupted = true; break; }
            // a launch: lrat_chunk lines (the test hook), else lines until they hold 2^24 hints - about 20 ms at the 7e8
            // hints a second measured on the rect 24 file
            uint64_t b = a + 1;
            if (s.lrat_chunk) b = std::min<uint64_t>(n_up, a + s.lrat_chunk);
            else while (b < n_up && F.hoffs[b] - F.hoffs[a] < (1ull << 24)) b++;
            const uint32_t grid = (uint32_t)std::min<uint64_t>(b - a, grid_cap);
            A.line0 = (uint32_t)a; A.line1 = (uint32_t)b;
            timed_launch(s, [&] {
                with_flag(lds, [&](auto lds_build) {
                    hipLaunchKernelGGL((ms_lrat_kernel<decltype(lds_build)::value>), dim3(grid), dim3(MS_WAVE), info.dyn_lds_bytes, s.stream, A);
                });
            }, [] {});
            info.launches++;
            info.waves = std::max<uint64_t>(info.waves, grid);
            rec.resize((size_t)grid * 4);
            HIPCHK(hipMemcpy(rec.data(), d_rec.p, rec.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t w = 0; w < grid; w++)
                if (rec[4 * w] != MS_LRAT_NONE && rec[4 * w] < rej_line) { rej_line = rec[4 * w]; rej_reason = rec[4 * w + 1]; rej_hint = rec[4 * w + 2]; }
            a = b;
        }
        info.kernel_seconds = s.stats.kernel_seconds - k0;
        if (rej_line != UINT64_MAX && (rej_line >= n_up || rej_reason < MS_LRAT_TAUTOLOGY || rej_reason > MS_LRAT_LAST_NOT_FALSIFIED)) {
            s.err = "lrat check: the device reported a line it was not given";
            return MI355SAT_ERR_HIP;
        }
    }
    if (interrupted) {
        consume_interrupt(s);
        info.accepted = -1;
        return MI355SAT_INTERRUPTED;
    }
    if (rej_line == UINT64_MAX && n_up < n_lines) { rej_line = n_up; rej_reason = MS_LRAT_ID_ORDER; }
    if (rej_line != UINT64_MAX) {
        info.first_rejected = rej_line;
        info.first_rejected_id = F.ids[rej_line];
        info.reason = (int32_t)rej_reason;
        info.reject_hint = rej_hint == MS_LRAT_NONE ? UINT64_MAX : rej_hint;
        return 0;
    }
    info.accepted = 1;
    info.valid = info.derives_target;
    if (n_up) {
        std::vector<uint32_t> bits(used_words);
        HIPCHK(hipMemcpy(bits.data(), d_used.p, used_words * 4, hipMemcpyDeviceToHost));
        for (uint64_t c = 0; c < n_orig; c++) if (bits[c >> 5] >> (c & 31) & 1) s.lrat.used.push_back(c);
    }
    s.lrat.valid = true;
    info.used_originals = s.lrat.used.size();
    return 0;
}

// The one body of mi355sat_check_lrat and _check_lrat_file.
int lrat_entry(mi355sat* s, const int32_t* words, uint64_t n_words, const char* path, const int32_t* target, uint64_t n_target,
               mi355sat_lrat_info* out) {
    mi355sat_lrat_info info{};
    info.first_rejected = info.reject_hint = UINT64_MAX;
    *out = info;                        // (every refusal below leaves it so)
    s->lrat = mi355sat::Lrat();         // the result of the check before ends here, also when this one is refused
    if (s->sweep) { s->err = "check_lrat() called during a sweep"; return MI355SAT_ERR_STATE; }
    if (!s->pending.empty()) { s->err = "check_lrat() called inside an unterminated clause"; return MI355SAT_ERR_STATE; }
    LratFile F;
    const double t0 = now_s();          // (info.seconds is the whole call: reading and parsing the text is most of it)
    if (int rc = guarded(s, GUARD_HOST, [&] {
            std::vector<int64_t> text;
            if (!path) return parse_lrat_words(*s, words, n_words, F);
            if (int e = read_lrat_file(*s, path, text)) return e;
            return parse_lrat_words(*s, text.data(), text.size(), F);
        })) return rc;
    const int rc = guarded(s, GUARD_TIMED, [&] { return check_lrat_impl(*s, F, target, n_target, info); });
    if (rc < 0) s->lrat = mi355sat::Lrat();
    info.seconds = now_s() - t0;
    *out = info;
    return rc;
}

}  // namespace

struct SweepHolder { Sweep sw; mi355sat_stats_t base; };

// =============================================================================== C ABI
extern "C" {

uint64_t mi355sat_abi_sizes(uint64_t* stats_size) {
    if (stats_size) *stats_size = sizeof(mi355sat_stats_t);
    return sizeof(mi355sat_opts);
}

void mi355sat_release_cached_memory(void) {
    std::lock_guard<std::mutex> g(g_slab_cache.mu);
    for (int d = 0; d < 64; d++)
        if (g_slab_cache.p[d]) {
            if (hipSetDevice(d) == hipSuccess) (void)hipFree(g_slab_cache.p[d]);
            g_slab_cache.p[d] = nullptr;
            g_slab_cache.bytes[d] = 0;
        }
}

const char* mi355sat_signature(void) { return "mi355sat 0.1 (HIP/gfx950 wave-parallel CDCL)"; }

const char* mi355sat_last_error(const mi355sat* s) {
    if (s) return s->err.c_str();
    std::lock_guard<std::mutex> g(g_new_error_mu);
    return g_new_error.c_str();
}

mi355sat* mi355sat_new(const mi355sat_opts* opts) {
    auto fail = [](const std::string& m) -> mi355sat* {
        std::lock_guard<std::mutex> g(g_new_error_mu);
        g_new_error = m;
        return nullptr;
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(std::string("no usable HIP device (mi355sat has no CPU fallback): ") +
                    (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    mi355sat* s = new (std::nothrow) mi355sat;
    if (!s) return fail("out of host memory");
    if (opts) s->opts = *opts;
    int dev = 0;
    if (opts && opts->device >= 0) dev = opts->device;
    else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= n) { delete s; return fail("device ordinal out of range"); }
    s->device = dev;
    try {
        HIPCHK(hipSetDevice(dev));
        HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&s->ev0));
        HIPCHK(hipEventCreate(&s->ev1));
        HIPCHK(hipHostMalloc((void**)&s->stop_flag, sizeof(int32_t), hipHostMallocMapped));
        *s->stop_flag = 0;
    } catch (HipErr& he) {
        std::string m = he.msg;
        delete s;
        return fail(m);
    }
    return s;
}

void mi355sat_free(mi355sat* s) {
    if (!s) return;
    // The order: the handle's device selected and its stream idle before anything goes; the sweep and the proof file are
    // not the handle's members, so by hand; then `delete s`, whose members' destructors return every device buffer (the
    // slabs: parked for the next handle) while that device is still the current one; the pinned flag, the events and the
    // stream are plain handles the destructor does not know about, and the stream outlives the buffers that were used on it.
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s->sweep;
    if (s->proof_file) fclose(s->proof_file);
    int32_t* const stop_flag = s->stop_flag;
    const hipEvent_t ev0 = s->ev0, ev1 = s->ev1;
    const hipStream_t stream = s->stream;
    delete s;
    if (stop_flag) (void)hipHostFree(stop_flag);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
}

int mi355sat_reserve(mi355sat* s, uint64_t n_vars) {
    if (!s) return MI355SAT_ERR_ARG;
    if (n_vars > s->max_var) s->max_var = n_vars;
    s->stats.max_var = s->max_var;
    return 0;
}

static int add_clause_impl(mi355sat* s, const int32_t* l, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        int32_t d = l[i];
        if (d == 0 || d == INT32_MIN) { s->err = "literal 0 inside a clause"; return MI355SAT_ERR_ARG; }
        if (var_of(d) > MS_MAX_VARS) { s->err = "variable index too large"; return MI355SAT_ERR_ARG; }
        if (var_of(d) > s->max_var) s->max_var = var_of(d);
    }
    s->lits.insert(s->lits.end(), l, l + n);
    s->offs.push_back(s->lits.size());
    s->core.valid = false;     // IPASIR: adding leaves the UNSAT state
    s->trim.drop();            // (clause indices mean something else now)
    s->lrat = mi355sat::Lrat();
    s->stats.n_clauses++;
    s->stats.max_var = s->max_var;
    s->stats.avg_clause_len = (double)s->lits.size() / (double)s->stats.n_clauses;
    return 0;
}

int mi355sat_add_cnf(mi355sat* s, const int32_t* lits, const uint64_t* offsets, uint64_t n_clauses) {
    if (!s || (n_clauses && (!offsets || (!lits && offsets[n_clauses] > offsets[0])))) return MI355SAT_ERR_ARG;
    return guarded(s, GUARD_HOST, [&] {
        for (uint64_t c = 0; c < n_clauses; c++) {
            if (offsets[c + 1] < offsets[c]) { s->err = "offsets not monotone"; return MI355SAT_ERR_ARG; }
            int rc = add_clause_impl(s, lits + offsets[c], offsets[c + 1] - offsets[c]);
            if (rc) return rc;
        }
        return 0;
    });
}

int mi355sat_add(mi355sat* s, int32_t lit_or_0) {
    if (!s) return MI355SAT_ERR_ARG;
    return guarded(s, GUARD_HOST, [&] {
        if (lit_or_0 != 0) { s->pending.push_back(lit_or_0); return 0; }
        int rc = add_clause_impl(s, s->pending.data(), s->pending.size());
        s->pending.clear();
        return rc;
    });
}

void mi355sat_interrupt(mi355sat* s) {
    if (!s) return;
    s->interrupted.store(1);
    if (s->stop_flag) __atomic_store_n(s->stop_flag, 1, __ATOMIC_SEQ_CST);
}

int mi355sat_assume(mi355sat* s, int32_t lit) {
    if (!s) return MI355SAT_ERR_ARG;
    const uint64_t v = var_of(lit);
    if (lit == 0 || v > MS_MAX_VARS) { s->err = "assumption literal out of range"; return MI355SAT_ERR_ARG; }
    if (int rc = guarded(s, GUARD_HOST, [&] { s->assumps.push_back(lit); return 0; })) return rc;
    if (v > s->max_var) { s->max_var = v; s->stats.max_var = v; }   // as mi355sat_reserve
    s->core.valid = false;
    return 0;
}

int mi355sat_failed(mi355sat* s, int32_t lit) {
    if (!s) return MI355SAT_ERR_ARG;
    if (!s->core.valid) { s->err = "no failed assumptions: the last solve() did not return UNSAT"; return MI355SAT_ERR_STATE; }
    return std::find(s->core.lits.begin(), s->core.lits.end(), lit) != s->core.lits.end() ? 1 : 0;
}

// A model (one byte per caller variable) into a caller's buffer of n_vars entries: 0 behind the model's end.
static void copy_model(const std::vector<int8_t>& m, int8_t* out, uint64_t n_vars) {
    for (uint64_t v = 0; v < n_vars; v++) out[v] = v < m.size() ? m[v] : 0;
}

static int copy_core(mi355sat* s, const Core& core, int32_t* out, uint64_t cap, uint64_t* n) {
    if (n) *n = core.lits.size();
    if (!out) return 0;
    if (cap < core.lits.size()) { s->err = "core buffer too small"; return MI355SAT_ERR_ARG; }
    std::copy(core.lits.begin(), core.lits.end(), out);
    return 0;
}

// The core of instance `instance` of the last solve_batch() into *core, or why there is none (`what`: how the message
// begins): MI355SAT_ERR_ARG for an index beyond that batch, MI355SAT_ERR_STATE where there was no batch or the instance
// was not UNSAT - or the core is not to be touched now (blocked).
static int find_batch_core(mi355sat* s, uint64_t instance, const char* what, Core** core, bool blocked = false) {
    const size_t n = s->batch_cores.size();
    if (instance < n && s->batch_cores[instance].valid && !blocked) { *core = &s->batch_cores[instance]; return 0; }
    s->err = std::string(what) + ": instance out of range or not UNSAT in the last solve_batch()";
    return instance >= n && n ? MI355SAT_ERR_ARG : MI355SAT_ERR_STATE;
}

int mi355sat_core(mi355sat* s, int32_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    if (!s->core.valid) { s->err = "no core: the last solve() did not return UNSAT"; return MI355SAT_ERR_STATE; }
    return copy_core(s, s->core, out, cap, n);
}

int mi355sat_core_of(mi355sat* s, uint64_t instance, int32_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    Core* core = nullptr;
    if (int rc = find_batch_core(s, instance, "no core", &core)) return rc;
    return copy_core(s, *core, out, cap, n);
}

int mi355sat_minimize_core(mi355sat* s, int64_t conflict_budget, mi355sat_core_min_info* out) {
    if (!s || conflict_budget < 0) return MI355SAT_ERR_ARG;
    if (!s->core.valid || s->sweep) { s->err = "no core to minimise: the last solve() did not return UNSAT"; return MI355SAT_ERR_STATE; }
    return minimize_core_impl(s, s->core, conflict_budget, out);
}

int mi355sat_minimize_core_of(mi355sat* s, uint64_t instance, int64_t conflict_budget, mi355sat_core_min_info* out) {
    if (!s || conflict_budget < 0) return MI355SAT_ERR_ARG;
    Core* core = nullptr;
    if (int rc = find_batch_core(s, instance, "no core to minimise", &core, /*blocked=*/s->sweep != nullptr)) return rc;
    return minimize_core_impl(s, *core, conflict_budget, out);
}

int mi355sat_debug_core_min_round(mi355sat* s, uint32_t max_candidates) {
    if (!s) return MI355SAT_ERR_ARG;
    s->core_min_round = max_candidates;
    return 0;
}

// ---- phase hints: kept in the caller's variables; the next cold start (or a warm one, if they changed) applies them
static int set_hint(mi355sat* s, uint64_t v, int8_t h) {      // v 1-based
    mi355sat::Phases& ph = s->ph;
    if (v > ph.hint.size()) {
        if (!h) return 0;
        ph.hint.resize(v, 0);
    }
    int8_t& cur = ph.hint[v - 1];
    if (cur == h) return 0;
    ph.info.hinted += (h != 0) - (cur != 0);
    cur = h;
    ph.version++;
    return 0;
}

int mi355sat_phase(mi355sat* s, int32_t lit) {
    if (!s) return MI355SAT_ERR_ARG;
    const uint64_t v = var_of(lit);
    if (lit == 0 || v > MS_MAX_VARS) { s->err = "phase literal out of range"; return MI355SAT_ERR_ARG; }
    if (int rc = guarded(s, GUARD_HOST, [&] { return set_hint(s, v, lit > 0 ? 1 : -1); })) return rc;
    if (v > s->max_var) { s->max_var = v; s->stats.max_var = v; }   // as mi355sat_reserve
    return 0;
}

int mi355sat_unphase(mi355sat* s, int32_t var) {
    if (!s) return MI355SAT_ERR_ARG;
    if (var <= 0 || (uint64_t)var > MS_MAX_VARS) { s->err = "variable out of range"; return MI355SAT_ERR_ARG; }
    return set_hint(s, (uint64_t)var, 0);
}

int mi355sat_set_phases(mi355sat* s, const int8_t* phases, uint64_t n_vars) {
    if (!s || (n_vars && !phases)) return MI355SAT_ERR_ARG;
    if (n_vars > MS_MAX_VARS) { s->err = "variable index too large"; return MI355SAT_ERR_ARG; }
    return guarded(s, GUARD_HOST, [&] {
        uint64_t top = 0;
        for (uint64_t v = 1; v <= n_vars; v++) {
            set_hint(s, v, phases[v - 1] > 0 ? 1 : (phases[v - 1] < 0 ? -1 : 0));
            if (phases[v - 1]) top = v;
        }
        if (top > s->max_var) { s->max_var = top; s->stats.max_var = top; }
        return 0;
    });
}

int mi355sat_debug_phases(const mi355sat* s, mi355sat_phase_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    *out = s->ph.info;
    return 0;
}

int mi355sat_set_proof_path(mi355sat* s, const char* path) {
    if (!s) return MI355SAT_ERR_ARG;
    s->proof_path = path ? path : "";
    return 0;
}

int mi355sat_debug_proof_log(const mi355sat* s, mi355sat_proof_log_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    *out = s->proof_log;
    return 0;
}

int mi355sat_check_proof(mi355sat* s, const int32_t* proof, uint64_t n_words, const int32_t* target, uint64_t n_target,
                         uint32_t segments, mi355sat_proof_info* out) {
    if (!s || !out || (n_words && !proof) || (n_target && !target)) return MI355SAT_ERR_ARG;
    const uint64_t toff[2] = {0, n_target};
    return proof_entry(s, "check_proof", proof, n_words, nullptr, ProofTargets{target, toff, 1, nullptr}, segments, out);
}

int mi355sat_check_proof_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target, uint32_t segments,
                              mi355sat_proof_info* out) {
    if (!s || !out || !path || (n_target && !target)) return MI355SAT_ERR_ARG;
    const uint64_t toff[2] = {0, n_target};
    return proof_entry(s, "check_proof", nullptr, 0, path, ProofTargets{target, toff, 1, nullptr}, segments, out);
}

// (target_offsets[0] need not be 0; a target may be empty, so `targets` may be NULL when every one is)
static bool bad_target_lists(const int32_t* targets, const uint64_t* target_offsets, uint64_t n_targets, const int32_t* target_valid) {
    return !target_offsets || !target_valid || n_targets == 0 || (!targets && target_offsets[n_targets] > target_offsets[0]);
}

int mi355sat_check_proof_targets(mi355sat* s, const int32_t* proof, uint64_t n_words, const int32_t* targets,
                                 const uint64_t* target_offsets, uint64_t n_targets, uint32_t segments, int32_t* target_valid,
                                 mi355sat_proof_info* out) {
    if (!s || !out || (n_words && !proof)) return MI355SAT_ERR_ARG;
    if (bad_target_lists(targets, target_offsets, n_targets, target_valid)) { s->err = "check_proof_targets: no targets"; return MI355SAT_ERR_ARG; }
    return proof_entry(s, "check_proof_targets", proof, n_words, nullptr, ProofTargets{targets, target_offsets, n_targets, target_valid}, segments, out);
}

int mi355sat_check_proof_targets_file(mi355sat* s, const char* path, const int32_t* targets, const uint64_t* target_offsets,
                                      uint64_t n_targets, uint32_t segments, int32_t* target_valid, mi355sat_proof_info* out) {
    if (!s || !out || !path) return MI355SAT_ERR_ARG;
    if (bad_target_lists(targets, target_offsets, n_targets, target_valid)) { s->err = "check_proof_targets: no targets"; return MI355SAT_ERR_ARG; }
    return proof_entry(s, "check_proof_targets", nullptr, 0, path, ProofTargets{targets, target_offsets, n_targets, target_valid}, segments, out);
}

int mi355sat_debug_proof_check_chunk(mi355sat* s, uint32_t max_lemmas_per_launch) {
    if (!s) return MI355SAT_ERR_ARG;
    s->proof_chunk = max_lemmas_per_launch;
    return 0;
}

int mi355sat_proof_deletions(mi355sat* s, int on) {
    if (!s) return MI355SAT_ERR_ARG;
    s->proof_del = on != 0;
    return 0;
}

int mi355sat_debug_proof_deletions(const mi355sat* s, mi355sat_proof_del_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    if (!s->proof_del_have) return MI355SAT_ERR_STATE;      // (const handle: no error text)
    *out = s->proof_del_info;
    return 0;
}

int mi355sat_trim_proof(mi355sat* s, const int32_t* proof, uint64_t n_words, const int32_t* target, uint64_t n_target,
                        uint32_t segments, uint32_t flags, mi355sat_trim_info* out) {
    if (!s || !out || (n_words && !proof) || (n_target && !target) || (flags & ~MI355SAT_TRIM_HINTS)) return MI355SAT_ERR_ARG;
    const uint64_t toff[2] = {0, n_target};
    return proof_entry(s, "trim_proof", proof, n_words, nullptr, ProofTargets{target, toff, 1, nullptr}, segments, nullptr, out, flags);
}

int mi355sat_trim_proof_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target, uint32_t segments,
                             uint32_t flags, mi355sat_trim_info* out) {
    if (!s || !out || !path || (n_target && !target) || (flags & ~MI355SAT_TRIM_HINTS)) return MI355SAT_ERR_ARG;
    const uint64_t toff[2] = {0, n_target};
    return proof_entry(s, "trim_proof", nullptr, 0, path, ProofTargets{target, toff, 1, nullptr}, segments, nullptr, out, flags);
}

static int trim_result(mi355sat* s) {
    if (s->trim.valid) return 0;
    s->err = "no trimmed proof: the last call was not a mi355sat_trim_proof() that found the proof valid";
    return MI355SAT_ERR_STATE;
}

static int copy_indices(mi355sat* s, const std::vector<uint64_t>& v, uint64_t* out, uint64_t cap, uint64_t* n) {
    if (n) *n = v.size();
    if (!out) return 0;
    if (cap < v.size()) { s->err = "index buffer too small"; return MI355SAT_ERR_ARG; }
    std::copy(v.begin(), v.end(), out);
    return 0;
}

int mi355sat_trim_core(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    if (int rc = trim_result(s)) return rc;
    return copy_indices(s, s->trim.core, out, cap, n);
}

int mi355sat_trim_lemmas(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    if (int rc = trim_result(s)) return rc;
    return copy_indices(s, s->trim.lemmas, out, cap, n);
}

// One clause per line: (LRAT) its id first, the literals, 0, (LRAT) the hints and another 0.
static int write_trimmed(mi355sat* s, const char* path, bool lrat) {
    if (!s || !path) return MI355SAT_ERR_ARG;
    if (int rc = trim_result(s)) return rc;
    const mi355sat::Trim& R = s->trim;
    if (lrat && !R.hints) { s->err = "trim_write_lrat(): the proof was trimmed without MI355SAT_TRIM_HINTS"; return MI355SAT_ERR_STATE; }
    return guarded(s, GUARD_HOST, [&] {
        FILE* f = fopen(path, "w");
        if (!f) { s->err = std::string("cannot open ") + path; return MI355SAT_ERR_ARG; }
        const size_t n_lines = R.no_lines && lrat ? 0 : R.offs.size() - 1;
        for (size_t i = 0; i < n_lines; i++) {
            const bool is_target = i + 1 == R.offs.size() - 1;
            if (lrat) fprintf(f, "%llu ", (unsigned long long)(R.n_clauses + 1 + (is_target ? R.n_lemmas : R.lemmas[i])));
            for (uint64_t k = R.offs[i]; k < R.offs[i + 1]; k++) fprintf(f, "%d ", R.lits[k]);
            fputs("0", f);
            if (lrat) {
                for (uint64_t h : R.hint[i]) fprintf(f, " %llu", (unsigned long long)h);
                fputs(" 0", f);
            }
            fputs("\n", f);
        }
        const bool bad = ferror(f) != 0;
        if (fclose(f) != 0 || bad) { s->err = std::string("cannot write ") + path; return MI355SAT_ERR_ARG; }
        return 0;
    });
}

int mi355sat_trim_write_drup(mi355sat* s, const char* path) { return write_trimmed(s, path, false); }
int mi355sat_trim_write_lrat(mi355sat* s, const char* path) { return write_trimmed(s, path, true); }

int mi355sat_debug_trim_log(mi355sat* s, uint32_t words_per_worker) {
    if (!s) return MI355SAT_ERR_ARG;
    s->trim_log_words = words_per_worker;
    return 0;
}

int mi355sat_check_lrat(mi355sat* s, const int32_t* lines, uint64_t n_words, const int32_t* target, uint64_t n_target,
                        mi355sat_lrat_info* out) {
    if (!s || !out || (n_words && !lines) || (n_target && !target)) return MI355SAT_ERR_ARG;
    return lrat_entry(s, lines, n_words, nullptr, target, n_target, out);
}

int mi355sat_check_lrat_file(mi355sat* s, const char* path, const int32_t* target, uint64_t n_target, mi355sat_lrat_info* out) {
    if (!s || !out || !path || (n_target && !target)) return MI355SAT_ERR_ARG;
    return lrat_entry(s, nullptr, 0, path, target, n_target, out);
}

int mi355sat_lrat_used(mi355sat* s, uint64_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    if (!s->lrat.valid) {
        s->err = "no checked LRAT file: the last call was not a mi355sat_check_lrat() that accepted every line";
        return MI355SAT_ERR_STATE;
    }
    return copy_indices(s, s->lrat.used, out, cap, n);
}

int mi355sat_debug_lrat_chunk(mi355sat* s, uint32_t max_lines_per_launch) {
    if (!s) return MI355SAT_ERR_ARG;
    s->lrat_chunk = max_lines_per_launch;
    return 0;
}

int mi355sat_set_incremental(mi355sat* s, int on) {
    if (!s) return MI355SAT_ERR_ARG;
    s->inc.on = on != 0;
    if (!s->inc.on) go_cold(*s, MI355SAT_COLD_FIRST);
    return 0;
}

int mi355sat_debug_incremental(const mi355sat* s, mi355sat_incremental_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    *out = s->inc.info;
    out->enabled = s->inc.on ? 1 : 0;
    return 0;
}

int mi355sat_debug_heuristics(const mi355sat* s, mi355sat_heuristics_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    *out = s->heur;
    return 0;
}

int mi355sat_debug_set_capacities(mi355sat* s, uint32_t learnt_cap, uint32_t learnt_lit_cap, uint32_t pool_slack, uint32_t proof_cap) {
    if (!s) return MI355SAT_ERR_ARG;
    // floors: conflict-clause minimisation keeps two node lists of learnt_cap / 2 entries in `remap`; add_learnt wants a
    // clause plus 8 words; a proof log holds at least one short lemma.  Ceilings: the rule's own maxima.
    if ((learnt_cap && (learnt_cap < 4 || learnt_cap > (1u << 17))) || (learnt_lit_cap && (learnt_lit_cap < 64 || learnt_lit_cap > (2u << 20))) ||
        pool_slack > (1u << 30) || (proof_cap && (proof_cap < 8 || proof_cap > (1u << 23)))) {
        s->err = "debug_set_capacities: a capacity outside its range";
        return MI355SAT_ERR_ARG;
    }
    s->want_learnt_cap = learnt_cap; s->want_learnt_lit_cap = learnt_lit_cap; s->want_pool_slack = pool_slack; s->want_proof_cap = proof_cap;
    return 0;
}

int mi355sat_debug_capacities(const mi355sat* s, mi355sat_capacity_info* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    if (!s->cap_info_valid) return MI355SAT_ERR_STATE;
    *out = s->cap_info;
    out->pressure_reduces = s->cap_events[0]; out->pool_rebuilds = s->cap_events[1]; out->imports_dropped_full = s->cap_events[2];
    return 0;
}

int mi355sat_debug_set_schedule(mi355sat* s, uint32_t first_vivify, uint32_t vivify_every, uint32_t rephase_every) {
    if (!s || vivify_every > 0xffffu || rephase_every > 0xffffu) return MI355SAT_ERR_ARG;
    s->first_vivify = first_vivify; s->vivify_every = vivify_every; s->rephase_every = rephase_every;
    go_cold(*s, MI355SAT_COLD_FIRST);      // next_vivify / next_rephase are part of a worker's state
    return 0;
}

int mi355sat_solve(mi355sat* s) {
    if (!s) return MI355SAT_ERR_ARG;
    std::vector<int32_t> assump;
    assump.swap(s->assumps);     // IPASIR: the assumptions hold for this solve only, whatever it returns
    s->core = Core{};
    if (!s->pending.empty()) { s->err = "solve() called inside an unterminated clause"; return MI355SAT_ERR_STATE; }
    const int rc = guarded(s, GUARD_TIMED, [&] {
        std::vector<uint64_t> aoff{0, (uint64_t)assump.size()};
        std::vector<int32_t> results, winner;
        std::vector<std::vector<int32_t>> cores;
        if (int err = run_search(*s, assump, aoff, 1, results, winner, true, &cores, /*plain_solve=*/true)) return err;
        const int result = results[0];
        if (result == MI355SAT_UNSAT) { s->core.lits = cores[0]; s->core.valid = true; }
        proof_close(*s, result == MI355SAT_UNSAT, s->core.lits);
        s->model.clear();
        if (result == MI355SAT_SAT) fetch_model(*s, (uint32_t)winner[0], s->model, s->max_var);
        tally_answer(*s, result);
        return result;
    });
    if (rc < 0) {      // a failed solve: its truncated proof file is closed, not leaked, and the next solve() starts cold
        proof_close(*s, false);
        go_cold(*s, MI355SAT_COLD_FIRST);
    }
    return rc;
}

int mi355sat_solve_batch(mi355sat* s, const int32_t* assumps, const uint64_t* assump_offsets, uint64_t n_instances,
                         int32_t* results_out, int stop_at_first) {
    if (!s || !assump_offsets || !results_out || n_instances == 0) return MI355SAT_ERR_ARG;
    const int rc = guarded(s, GUARD_TIMED, [&] {
        std::vector<int32_t> assump, results, winner;
        std::vector<uint64_t> aoff;
        copy_lists(assumps, assump_offsets, n_instances, assump, aoff);
        s->batch_cores.clear();
        std::vector<std::vector<int32_t>> cores;
        if (int err = run_search(*s, assump, aoff, (uint32_t)n_instances, results, winner, stop_at_first != 0, &cores)) return err;
        s->batch_models.assign(n_instances, {});
        s->batch_cores.assign(n_instances, Core{});
        for (uint64_t i = 0; i < n_instances; i++) {
            results_out[i] = results[i];
            s->batch_cores[i].lits.swap(cores[i]);
            s->batch_cores[i].valid = results[i] == MI355SAT_UNSAT;
            fetch_model_of(*s, results, winner, i, s->batch_models[i]);
            tally_answer(*s, results[i]);
        }
        return 0;
    });
    proof_close(*s, false);      // (the core lines are in it: proof_core_lines; after an error it ends where the error came)
    return rc;
}

int mi355sat_propagate_batch(mi355sat* s, const int32_t* decisions, const uint64_t* decision_offsets,
                             uint64_t n_instances, int8_t* out_values, uint64_t n_vars, int32_t* out_conflict,
                             int32_t* out_trail_len, int32_t repeat) {
    if (!s || !decision_offsets || n_instances == 0) return MI355SAT_ERR_ARG;
    return guarded(s, GUARD_TIMED, [&] {
        go_cold(*s, MI355SAT_COLD_OTHER_SEARCH);     // (the slabs become this batch's)
        s->ph.on_device = false;     // scripted BCP decides nothing: no phase hints
        Prepared P;
        prepare(*s, /*simplify=*/false, P);
        if (P.unsat) {  // contradictory unit clauses: every instance conflicts before any decision
            for (uint64_t i = 0; i < n_instances; i++) {
                if (out_conflict) out_conflict[i] = 1;
                if (out_trail_len) out_trail_len[i] = 0;
            }
            if (out_values) memset(out_values, 0, n_instances * n_vars);
            return 0;
        }
        std::vector<int32_t> script;
        std::vector<uint64_t> soff;
        copy_lists(decisions, decision_offsets, n_instances, script, soff);
        uint32_t max_script = 0;
        for (uint64_t i = 0; i < n_instances; i++) max_script = std::max<uint32_t>(max_script, (uint32_t)(soff[i + 1] - soff[i]));
        for (int32_t& d : script) {
            if (d == 0 || var_of(d) > P.n_vars) throw HipErr{"decision literal out of range"};
            d = to_device(P.perm, d);
        }
        upload_formula(*s, P, 0, max_script, (uint32_t)n_instances);
        if (s->n_workers < n_instances) throw HipErr{"not enough device memory for the batch"};
        std::vector<MsState> sts;
        if (repeat < 1) repeat = 1;
        for (int r = 0; r < repeat; r++) {
            reset_workers(*s);
            customize(*s, nullptr, nullptr, &script, &soff, (uint32_t)n_instances);
            launch_slice(*s, 1, false);
        }
        gather_states(*s, sts);
        for (uint64_t i = 0; i < n_instances; i++) {
            if (sts[i].status < 0) return status_error(*s, sts[i].status, MI355SAT_ERR_OOM);
            if (out_conflict) out_conflict[i] = sts[i].status == MS_ST_UNSAT ? 1 : 0;
            if (out_trail_len) out_trail_len[i] = sts[i].trail_n;
        }
        accumulate_stats(*s, sts, (uint64_t)repeat);     // counters of the last repeat only, scaled
        if (out_values) {
            const size_t nw = P.n_vars;
            std::vector<uint8_t> raw(n_instances * nw + 1);
            if (P.n_vars)
                HIPCHK(hipMemcpy2D(raw.data(), nw, s->d_slabs.p + s->L.val, s->L.slab_bytes, nw,
                                   n_instances, hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < n_instances; i++)
                for (uint64_t v = 0; v < n_vars; v++) {
                    uint8_t x = v < P.n_vars ? raw[i * nw + P.perm[v]] : MS_ASG_UNDEF;
                    out_values[i * n_vars + v] = x == MS_ASG_TRUE ? 1 : (x == MS_ASG_FALSE ? -1 : 0);
                }
        }
        return 0;
    });
}

int mi355sat_sweep_begin(mi355sat* s, const int32_t* assumps, const uint64_t* assump_offsets, uint64_t n_instances) {
    if (!s || !assump_offsets || n_instances == 0) return MI355SAT_ERR_ARG;
    const int rc = guarded(s, GUARD_DEVICE, [&] {
        std::vector<int32_t> assump;
        std::vector<uint64_t> aoff;
        copy_lists(assumps, assump_offsets, n_instances, assump, aoff);
        proof_close(*s, false);                          // (of a sweep this one replaces)
        delete s->sweep;
        s->sweep = new SweepHolder;
        s->sweep->base = s->stats;
        s->trim.drop();
        go_cold(*s, MI355SAT_COLD_OTHER_SEARCH);
        s->sweep->sw.cores = !s->proof_path.empty();     // final-conflict cores only while a proof is logged: its core lines
        return sweep_begin(*s, s->sweep->sw, assump, aoff, (uint32_t)n_instances, false);
    });
    if (rc < 0) proof_close(*s, false);
    return rc;
}

int mi355sat_sweep_step(mi355sat* s, int32_t* results_out, uint64_t* n_decided) {
    if (!s || !s->sweep) return MI355SAT_ERR_STATE;
    const int step_rc = guarded(s, GUARD_TIMED, [&] {
        Sweep& sw = s->sweep->sw;
        int rc = sweep_step(*s, sw);
        if (results_out) for (uint32_t i = 0; i < sw.n_instances; i++) results_out[i] = sw.results[i];
        if (n_decided) *n_decided = sw.decided;
        // running totals so that stats() is meaningful between steps: what they were when the sweep began, this sweep's
        // times, and the workers' counters as they stand
        const mi355sat_stats_t keep = s->stats;
        s->stats = s->sweep->base;
        s->stats.kernel_seconds = keep.kernel_seconds;
        s->stats.kernel_launches = keep.kernel_launches;
        s->stats.solve_seconds = keep.solve_seconds;
        keep_last_solve_stats(s->stats, keep);
        accumulate_stats(*s, sw.sts);
        return rc;
    });
    if (step_rc < 0) proof_close(*s, false);     // the file ends where the error came, as a failed solve()'s
    return step_rc;
}

int mi355sat_sweep_drop(mi355sat* s, const uint64_t* instances, uint64_t n) {
    if (!s || !s->sweep || (n && !instances)) return MI355SAT_ERR_STATE;
    return guarded(s, GUARD_DEVICE, [&] {
        Sweep& sw = s->sweep->sw;
        bool any = false;
        for (uint64_t j = 0; j < n; j++) {
            if (instances[j] >= sw.n_instances) { s->err = "instance out of range"; return MI355SAT_ERR_ARG; }
            any |= sw.withdraw((uint32_t)instances[j]);
        }
        return reschedule_after_caller(*s, sw, any && sw.decided < sw.n_instances);     // (nothing left open: nobody moves)
    });
}

int mi355sat_sweep_set_weights(mi355sat* s, const double* weights, uint64_t n) {
    if (!s || !s->sweep || !weights) return MI355SAT_ERR_STATE;
    Sweep& sw = s->sweep->sw;
    if (n != sw.n_instances) { s->err = "one weight per instance"; return MI355SAT_ERR_ARG; }
    std::vector<double> w(weights, weights + n);
    for (double x : w) if (!(x >= 0)) { s->err = "weights must be >= 0"; return MI355SAT_ERR_ARG; }
    if (w != sw.weights) { sw.weights.swap(w); sw.weights_dirty = true; }
    return 0;
}

int mi355sat_sweep_reopen(mi355sat* s, const uint64_t* instances, uint64_t n) {
    if (!s || !s->sweep || (n && !instances)) return MI355SAT_ERR_STATE;
    return guarded(s, GUARD_DEVICE, [&] {
        Sweep& sw = s->sweep->sw;
        bool any = false;
        for (uint64_t j = 0; j < n; j++) {
            if (instances[j] >= sw.n_instances) { s->err = "instance out of range"; return MI355SAT_ERR_ARG; }
            any |= sw.reopen((uint32_t)instances[j]);
        }
        return reschedule_after_caller(*s, sw, any);
    });
}

int mi355sat_sweep_model_of(mi355sat* s, uint64_t instance, int8_t* out, uint64_t n_vars) {
    if (!s || !s->sweep || !out) return MI355SAT_ERR_STATE;
    return guarded(s, GUARD_DEVICE, [&] {
        Sweep& sw = s->sweep->sw;
        std::vector<int8_t> m;
        if (instance >= sw.n_instances || !fetch_model_of(*s, sw.results, sw.winner, instance, m)) {
            s->err = "no model for that instance";
            return MI355SAT_ERR_STATE;
        }
        copy_model(m, out, n_vars);
        return 0;
    });
}

int mi355sat_sweep_core_of(mi355sat* s, uint64_t instance, int32_t* out, uint64_t cap, uint64_t* n) {
    if (!s) return MI355SAT_ERR_ARG;
    if (!s->sweep || !s->sweep->sw.log_cores) { s->err = "no core: no sweep that logs a proof is running"; return MI355SAT_ERR_STATE; }
    const Sweep& sw = s->sweep->sw;
    if (instance >= sw.n_instances || sw.results[instance] != MI355SAT_UNSAT) {
        s->err = "no core: instance out of range or not UNSAT in this sweep";
        return instance >= sw.n_instances ? MI355SAT_ERR_ARG : MI355SAT_ERR_STATE;
    }
    return guarded(s, GUARD_HOST, [&] {
        Core core;
        core.lits = sw.core_of((uint32_t)instance);
        return copy_core(s, core, out, cap, n);
    });
}

int mi355sat_sweep_end(mi355sat* s) {
    if (!s || !s->sweep) return MI355SAT_ERR_STATE;
    proof_close(*s, false);
    return guarded(s, GUARD_DEVICE, [&] {
        Sweep& sw = s->sweep->sw;
        s->batch_models.assign(sw.n_instances, {});
        for (uint32_t i = 0; i < sw.n_instances; i++) fetch_model_of(*s, sw.results, sw.winner, i, s->batch_models[i]);
        consume_interrupt(*s);
        delete s->sweep;
        s->sweep = nullptr;
        return 0;
    });
}

int32_t mi355sat_val(mi355sat* s, int32_t lit) {
    if (!s || lit == 0) return 0;
    const uint64_t v = var_of(lit);
    if (v > s->model.size()) return 0;
    int8_t m = s->model[v - 1];
    if (m == 0) return 0;
    bool is_true = (lit > 0) == (m > 0);
    return is_true ? lit : -lit;
}

int mi355sat_model(mi355sat* s, int8_t* out, uint64_t n_vars) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    if (s->model.empty() && s->max_var) { s->err = "no model (last result was not SAT)"; return MI355SAT_ERR_STATE; }
    copy_model(s->model, out, n_vars);
    return 0;
}

int mi355sat_model_of(mi355sat* s, uint64_t instance, int8_t* out, uint64_t n_vars) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    if (instance >= s->batch_models.size() || s->batch_models[instance].empty()) {
        s->err = "no model for that instance";
        return MI355SAT_ERR_STATE;
    }
    copy_model(s->batch_models[instance], out, n_vars);
    return 0;
}

int mi355sat_debug_share_ring(mi355sat* s, int32_t* out, uint64_t cap_words, uint64_t* n_records) {
    if (!s || !n_records) return MI355SAT_ERR_ARG;
    *n_records = 0;
    if (!s->share_slots || !s->d_share_pool.p) return 0;
    return guarded(s, GUARD_DEVICE, [&] {
        HIPCHK(hipStreamSynchronize(s->stream));
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, s->d_share_n.p, sizeof n, hipMemcpyDeviceToHost));
        const uint64_t live = std::min<uint64_t>(n, s->share_slots);
        std::vector<int32_t> ring((size_t)live * MS_SHARE_REC);
        if (live) HIPCHK(hipMemcpy(ring.data(), s->d_share_pool.p, ring.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        const std::vector<uint32_t> inv = inverse_order(s->perm);
        uint64_t w = 0;
        for (uint64_t r = 0; r < live; r++) {
            const int32_t* rec = ring.data() + r * MS_SHARE_REC;
            const int sz = rec[0] & 63;
            if (sz < 1 || sz > MS_SHARE_MAXLEN) { s->err = "malformed record in the exchange ring"; return MI355SAT_ERR_STATE; }
            if (out && w + (uint64_t)sz + 1 <= cap_words) {
                for (int j = 1; j <= sz; j++) {
                    if (rec[j] < 0 || (uint32_t)(rec[j] >> 1) >= inv.size()) { s->err = "literal out of range in the exchange ring"; return MI355SAT_ERR_STATE; }
                    out[w + j - 1] = to_dimacs(inv, rec[j]);
                }
                out[w + sz] = 0;
            }
            w += (uint64_t)sz + 1;
            (*n_records)++;
        }
        return w <= cap_words || !out ? 0 : MI355SAT_ERR_ARG;
    });
}

int mi355sat_debug_keep_simplified(mi355sat* s, int on) {
    if (!s) return MI355SAT_ERR_ARG;
    s->keep_simplified = on != 0;
    if (!on) { for (int k = 0; k < 2; k++) { std::vector<int32_t>().swap(s->kept[k]); s->kept_n[k] = 0; } s->kept_valid = false; }
    return 0;
}

int mi355sat_debug_simplified(mi355sat* s, int which, int32_t* out, uint64_t cap_words, uint64_t* n_words, uint64_t* n_clauses) {
    if (!s || !n_words || !n_clauses || which < 0 || which > 1) return MI355SAT_ERR_ARG;
    *n_words = *n_clauses = 0;
    if (!s->kept_valid) { s->err = "no simplified formula kept: arm mi355sat_debug_keep_simplified() before the solve"; return MI355SAT_ERR_STATE; }
    const std::vector<int32_t>& k = s->kept[which];
    *n_words = k.size();
    *n_clauses = s->kept_n[which];
    if (!out) return 0;
    if (cap_words < k.size()) return MI355SAT_ERR_ARG;
    std::copy(k.begin(), k.end(), out);
    return 0;
}

int mi355sat_debug_last_search_build(const mi355sat* s, mi355sat_search_build* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    if (s->last_build.launches == 0) return MI355SAT_ERR_STATE;
    *out = s->last_build;
    return 0;
}

int mi355sat_debug_search_build_rule(uint32_t active, uint32_t lds_val_bytes, int32_t staged, int32_t lds_val, int32_t one_per_simd,
                                     int32_t mode, mi355sat_search_build* out) {
    if (!out || active == 0) return MI355SAT_ERR_ARG;
    *out = choose_build(active, lds_val_bytes, staged < 0 ? staged_in_lds(lds_val, lds_val_bytes) : staged != 0, lds_val, one_per_simd, mode);
    return 0;
}

// ---- clause exchange between handles (GPUs) working on the SAME formula ------------------------------------------------
// Records travel as [lbd, DIMACS literals ..., 0] in the CALLER's variables: a ring record is a consequence of the
// simplified formula this handle searches, hence of the caller's formula (simplification only derives consequences,
// substituted variables are written as their representatives), so another handle - whose own simplification may have
// come out differently - can map it into its own variables and attach it.  The import normalises what the mapping leaves:
// a record that names both members of an equivalence class of THIS handle arrives as one device literal twice, or as a
// literal and its negation - and a clause in a worker's store holds every variable at most once (conflict analysis marks
// and counts the variables of a reason one lane each: a variable presented by two lanes is counted twice, the walk runs
// off the trail, MS_ST_ERR_INTERNAL).  So the mapped record is sorted, a repeated literal kept once, and a record with a
// literal and its negation (true whatever the assignment) dropped and not counted, exactly as warm_begin treats a clause
// the caller adds.
#define MS_FOREIGN_PRODUCER 0x3ffffu    // producer id of records that came from another handle: never handed out again
int mi355sat_share_export(mi355sat* s, int32_t* out, uint64_t cap_words, uint64_t* n_words, uint64_t* n_records) {
    if (!s || !n_words || !n_records) return MI355SAT_ERR_ARG;
    *n_words = 0; *n_records = 0;
    if (!s->share_slots || !s->d_share_pool.p || !s->sweep) return 0;
    return guarded(s, GUARD_DEVICE, [&] {
        HIPCHK(hipStreamSynchronize(s->stream));
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, s->d_share_n.p, sizeof n, hipMemcpyDeviceToHost));
        uint64_t from = s->share_export_pos;
        if (n - from > s->share_slots) from = n - s->share_slots;     // overwritten before anybody asked
        if (n == from) return 0;
        std::vector<int32_t> recs((size_t)(n - from) * MS_SHARE_REC);
        for (uint64_t r = from; r < n;) {      // at most two pieces (the ring wraps)
            const uint64_t slot = r % s->share_slots, cnt = std::min<uint64_t>(n - r, s->share_slots - slot);
            HIPCHK(hipMemcpy(recs.data() + (r - from) * MS_SHARE_REC, s->d_share_pool.p + slot * MS_SHARE_REC,
                             cnt * MS_SHARE_REC * sizeof(int32_t), hipMemcpyDeviceToHost));
            r += cnt;
        }
        const std::vector<uint32_t> inv = inverse_order(s->perm);
        uint64_t w = 0, consumed = from;
        for (uint64_t r = from; r < n; r++) {
            const int32_t* rec = recs.data() + (r - from) * MS_SHARE_REC;
            const uint32_t hdr = (uint32_t)rec[0];
            const int sz = (int)(hdr & 63u);
            if ((hdr >> 14) == MS_FOREIGN_PRODUCER || sz < 1 || sz > MS_SHARE_MAXLEN) { consumed = r + 1; continue; }
            if (out && w + (uint64_t)sz + 2 > cap_words) break;        // the rest waits for the next call
            if (out) {
                out[w] = (int32_t)std::max<uint32_t>(1u, (hdr >> 6) & 255u);
                for (int j = 1; j <= sz; j++) {
                    if (rec[j] < 0 || (uint32_t)(rec[j] >> 1) >= inv.size()) { s->err = "literal out of range in the exchange ring"; return MI355SAT_ERR_STATE; }
                    out[w + j] = to_dimacs(inv, rec[j]);
                }
                out[w + sz + 1] = 0;
            }
            w += (uint64_t)sz + 2;
            (*n_records)++;
            consumed = r + 1;
        }
        if (out) s->share_export_pos = consumed;     // (out == NULL only sizes the buffer)
        *n_words = w;
        return 0;
    });
}

int mi355sat_share_import(mi355sat* s, const int32_t* clauses, uint64_t n_words, uint64_t* n_records) {
    if (!s || (!clauses && n_words)) return MI355SAT_ERR_ARG;
    if (n_records) *n_records = 0;
    if (!n_words || !s->share_slots || !s->d_share_pool.p || !s->sweep) return 0;
    if (s->proof_file) return 0;                       // a foreign clause has no derivation in the proof being logged
    return guarded(s, GUARD_DEVICE, [&] {
        std::vector<uint8_t> gone(s->n_vars, 0);       // variables this handle's simplification resolved away
        for (const MsElim& e : s->elims) if ((uint32_t)(e.x >> 1) < gone.size()) gone[e.x >> 1] = 1;
        std::vector<int32_t> recs;
        uint64_t n_new = 0;
        for (uint64_t i = 0; i < n_words;) {
            const int32_t lbd = clauses[i++];
            int32_t rec[MS_SHARE_REC];
            int sz = 0;
            bool ok = lbd >= 1;
            while (i < n_words && clauses[i] != 0) {
                const int32_t d = clauses[i++];
                if (var_of(d) > s->n_vars || sz >= MS_SHARE_MAXLEN) { ok = false; continue; }
                const int32_t l = device_literal(*s, s->perm, d, &gone);     // (bounded by subst.size() there)
                if (l < 0) { ok = false; continue; }
                rec[1 + sz++] = l;
            }
            if (i >= n_words) { s->err = "share_import: clause without terminator"; return MI355SAT_ERR_ARG; }
            i++;   // the terminator
            if (!ok || sz < 1) continue;
            // as warm_begin does for an added clause: sorted, a repeated device literal once, a tautology not at all
            std::sort(rec + 1, rec + 1 + sz);
            sz = (int)(std::unique(rec + 1, rec + 1 + sz) - (rec + 1));
            bool taut = false;
            for (int j = 1; j < sz; j++) taut = taut || (rec[j] ^ 1) == rec[j + 1];
            if (taut) continue;
            rec[0] = (int32_t)((uint32_t)sz | ((uint32_t)std::min<int32_t>(lbd, 255) << 6) | (MS_FOREIGN_PRODUCER << 14));
            for (int j = sz + 1; j < MS_SHARE_REC; j++) rec[j] = 0;
            recs.insert(recs.end(), rec, rec + MS_SHARE_REC);
            n_new++;
        }
        if (!n_new) return 0;
        if (n_new > s->share_slots) { s->err = "share_import: more records than the ring holds"; return MI355SAT_ERR_ARG; }
        HIPCHK(hipStreamSynchronize(s->stream));
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, s->d_share_n.p, sizeof n, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < n_new;) {
            const uint64_t slot = (n + r) % s->share_slots, cnt = std::min<uint64_t>(n_new - r, s->share_slots - slot);
            HIPCHK(hipMemcpy(s->d_share_pool.p + slot * MS_SHARE_REC, recs.data() + r * MS_SHARE_REC,
                             cnt * MS_SHARE_REC * sizeof(int32_t), hipMemcpyHostToDevice));
            r += cnt;
        }
        n += n_new;
        HIPCHK(hipMemcpy(s->d_share_n.p, &n, sizeof n, hipMemcpyHostToDevice));
        if (n_records) *n_records = n_new;
        return 0;
    });
}

int mi355sat_stats(const mi355sat* s, mi355sat_stats_t* out) {
    if (!s || !out) return MI355SAT_ERR_ARG;
    *out = s->stats;
    return 0;
}

}  // extern "C"
