// The host-side arithmetic of a model query (imputation, marginal likelihoods, site and window conditionals): the scratch budget, the order in
// which instances are dealt out, and how many instances one launch takes.  Pure functions in plain C++17, no HIP and no environment:
// free device memory and the MPST_IMPUTE_CHUNK_GB / MPST_IMP_NO_ORDER switches come in as arguments, which the caller reads.
// tests/test_query_plan.py compiles it alone; mpst_internal.h includes it for everything else.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace mpst {

constexpr int SITECOND_TILE = 16;       // instances per workgroup of the site conditionals' walk

// Bytes of per-instance scratch a query may keep on the device at a time: half of the free memory, at most 48 GB; chunk_gb (the text
// of MPST_IMPUTE_CHUNK_GB, or null) replaces it, with a floor of 0.001 GB.  The 27 GB of environments of configs[4] (8192 instances
// x 100 missing sites x 32 KB) are one block on a 288 GB device, 512 workgroups of the batched sweep instead of seven launches of 82.
inline double query_budget(size_t free_b, const char* chunk_gb) {
    if (chunk_gb) return std::max(0.001, atof(chunk_gb)) * (double)(1ull << 30);
    return std::min(48.0 * (double)(1ull << 30), 0.5 * (double)free_b);
}

// cdf points stored per missing site: the grid indices 0, stride, 2 stride, ... and always ngrid - 1 (0: no cdfs asked for)
inline int64_t cdf_points(int32_t ngrid, int32_t stride) { return stride > 0 ? (int64_t)(ngrid - 2) / stride + 2 : 0; }

// Instances are dealt out to workgroups in the order of where their missing sites begin (in the direction of the sweep):
// workgroups that are resident together then walk the chain in step and find the site tensor the first of them fetched
// still in the L2 (a 262 KB tensor per site at configs[4], re-read by every instance).  The key of an instance with nothing
// missing is T; ties keep the caller's order, and so does everything with keep_caller_order (MPST_IMP_NO_ORDER).  Results do
// not depend on the order.
inline std::vector<int32_t> impute_plan_order(const uint8_t* missing, int64_t N, int64_t T, bool backwards, bool keep_caller_order) {
    std::vector<int32_t> order((size_t)N), key((size_t)N, (int32_t)T);
    for (int64_t i = 0; i < N; ++i) {
        order[i] = (int32_t)i;
        for (int64_t j = 0; j < T; ++j)
            if (missing[i * T + (backwards ? T - 1 - j : j)]) { key[i] = (int32_t)j; break; }
    }
    if (!keep_caller_order) std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    return order;
}

// what the block of an imputation call is cut from
struct ImputeSizes {
    int64_t N, K;               // instances; trajectories per instance
    int32_t T, cap, zw, esz;    // sites; largest bond dimension; 2 for complex models; bytes of a chain element (4 or 8)
    int32_t maxm, ngrid;        // most missing sites of an instance; grid values
    int64_t welems;             // scratch elements per instance of the large-chi environment kernel (mpst_impute.hip: impute_work_elems)
    int64_t cdf_inst;           // doubles of cdf rows per instance
    int32_t nq, u_trials;       // levels; uniform numbers per (chain, site) the caller hands over (0: none, or drawn on the device)
    int64_t site_grid_doubles;  // doubles of a per-site grid table, 0 for the one shared table
    bool dist;                  // a *_dist call
};
struct ImputeBlock {
    int64_t chunk, per_bytes;   // instances per launch; scratch bytes of one instance
    bool nomem;                 // a *_dist call of which not even one instance fits: chunk is not set
};
// Per instance: its environments once, p_k and S_k for each of its K chains, its cdf rows (staged with its block, copied out and
// scattered after its sweep).  A block is a run of whole instances, i.e. of chunk * K chains.  What lives for the whole call comes
// off the budget, never below one instance: the outputs and uniform numbers of the extra trajectories, the levels' q_out [N][T][nq],
// a per-site table (T times the shared one - 128 MB at configs[4]).
inline ImputeBlock impute_plan_block(const ImputeSizes& s, size_t free_b, const char* chunk_gb) {
    const int64_t N = s.N, K = s.K;
    const double dbl = (double)sizeof(double);
    ImputeBlock b{0, 0, false};
    b.per_bytes = ((int64_t)s.maxm * s.cap * s.cap * s.zw + s.welems) * (int64_t)s.esz + 2ll * K * s.ngrid * (int64_t)sizeof(double) +
                  s.cdf_inst * (int64_t)sizeof(double);
    const double per = (double)b.per_bytes;
    double budget = query_budget(free_b, chunk_gb);
    if (K > 1) budget = std::max(budget - (double)(N * (K - 1) * s.T) * dbl * (2.0 + (double)s.u_trials), per);
    if (s.nq > 0) budget = std::max(budget - (double)(N * s.T * s.nq) * dbl, per);
    if (s.site_grid_doubles > 0) budget = std::max(budget - (double)s.site_grid_doubles * dbl, per);
    if (s.dist && per > 0.9 * (double)free_b) {         // (the calls without distribution outputs are left as they were)
        b.nomem = true;
        return b;
    }
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(budget / per)));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(1ll << 30) / K));      // the sweep's grid counts chains in 32 bits
    if (chunk < N && chunk > 4096) chunk &= ~(int64_t)4095;      // whole rounds of 16-instance workgroups on 256 CUs
    b.chunk = chunk;
    return b;
}

// Marginal likelihoods keep no environments: a block is all N instances (at most 2^30) unless the kernel works in global scratch
// (welems > 0, mpst_impute.hip: marginal_work_elems), which is cut from half of the free memory, at most 48 GB.  MPST_IMPUTE_CHUNK_GB
// has never applied to this call, and still does not.
inline int64_t marginal_plan_block(int64_t N, int64_t welems, int32_t esz, size_t free_b) {
    int64_t chunk = std::min<int64_t>(N, (int64_t)1 << 30);
    if (welems) chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(query_budget(free_b, nullptr) / ((double)welems * (double)esz))));
    return chunk;
}

// workgroups of the site conditionals' grid phase (each owns ngrid doubles of pbuf and sbuf), an (instance, site) pair at a time
inline int64_t sitecond_grid_workgroups(int64_t pairs) { return std::max<int64_t>(1, std::min<int64_t>(pairs, 4096)); }

struct SitecondBlock {
    int64_t chunk, tiles, grid_wgs;     // instances per launch; workgroups of its walk; workgroups of its grid phase
};
// Site conditionals: the walk's left rows ([T][16][chi] per workgroup of sixteen instances) and the amplitudes are the scratch of a
// block; a block smaller than N is whole workgroups of the walk, at least one.
inline SitecondBlock sitecond_plan_block(int64_t N, int32_t T, int32_t cap, int32_t d, int32_t zw, size_t free_b, const char* chunk_gb) {
    const double per_bytes = (double)T * (cap + d + 1) * zw * sizeof(double);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(query_budget(free_b, chunk_gb) / per_bytes)));
    chunk = std::min<int64_t>(chunk, ((int64_t)1 << 30) / T);                                           // (instance, site) pairs in 32 bits
    if (chunk < N) chunk = std::max<int64_t>(SITECOND_TILE, chunk / SITECOND_TILE * SITECOND_TILE);
    return {chunk, (chunk + SITECOND_TILE - 1) / SITECOND_TILE, sitecond_grid_workgroups(chunk * T)};
}

// ---- window conditionals (mpst_window.inl: k_win_walk, k_win) ----
constexpr int WINDOW_BIG_MATS = 4;              // chi x chi matrices of global scratch per workgroup of k_win beyond the LDS limit
constexpr int WINDOW_MAX_WORKGROUPS = 4096;     // of k_win, a (instance, start) pair at a time
constexpr int WINDOW_MAX_BIG_WORKGROUPS = 1024; // ... where each owns global scratch

struct WindowBlock {
    int64_t chunk, tiles, win_wgs;      // instances per launch; workgroups of its walk; workgroups of its window kernel
};
// Window conditionals.  With budget = query_budget(free_b, chunk_gb), in bytes:
//     per instance    T * (2 * cap * zw + max_width) * 8      the left and the right rows of every site, and the block's nll
//     per workgroup   WINDOW_BIG_MATS * cap * cap * zw * 8    of k_win, on the big route only (big_route: the matrix step in global scratch)
//     chunk   = floor((big_route ? 3/4 : 1) * budget / per instance), at least 1, at most N and at most floor(2^30 / T)
//               ((instance, start) pairs in 32 bits); a chunk smaller than N is whole tiles of SITECOND_TILE instances, at least one
//     tiles   = ceil(chunk / SITECOND_TILE)
//     win_wgs = min(chunk * T, WINDOW_MAX_WORKGROUPS); on the big route also at most WINDOW_MAX_BIG_WORKGROUPS and at most
//               floor(budget / 4 / per workgroup), never below 1
// The shares of the big route are fixed, so both results are monotone in the budget.
inline WindowBlock window_plan_block(int64_t N, int32_t T, int32_t cap, int32_t zw, int32_t max_width, bool big_route, size_t free_b,
                                     const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const double per_bytes = (double)T * (2.0 * cap * zw + max_width) * sizeof(double);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)((big_route ? 0.75 : 1.0) * budget / per_bytes)));
    chunk = std::min<int64_t>(chunk, ((int64_t)1 << 30) / T);
    if (chunk < N) chunk = std::max<int64_t>(SITECOND_TILE, chunk / SITECOND_TILE * SITECOND_TILE);
    int64_t wgs = std::min<int64_t>(chunk * T, WINDOW_MAX_WORKGROUPS);
    if (big_route) {
        const double wg_bytes = (double)WINDOW_BIG_MATS * cap * cap * zw * sizeof(double);
        wgs = std::min<int64_t>(std::min<int64_t>(wgs, WINDOW_MAX_BIG_WORKGROUPS), (int64_t)(0.25 * budget / wg_bytes));
    }
    return {chunk, (chunk + SITECOND_TILE - 1) / SITECOND_TILE, std::max<int64_t>(1, wgs)};
}

// ---- pair analysis (mpst_analysis.hip: k_an_pair) ----
// A chain (class, i) carries d (d + 1) / 2 blocks E^{ss'}, s <= s', each ld x ld with ld = chi_max rounded up to the k-step of the
// MFMA (4) and a row stride of ld + 4 (LDS banks).  E and the E' of the next site live in LDS while both fit beside the kernel's
// static LDS; beyond that in global scratch, one region per workgroup.
constexpr int64_t PAIR_LDS_BYTES = 156 * 1024;         // dynamic LDS of k_an_pair (160 KB less its static part)
constexpr int PAIR_MAX_WORKGROUPS = 512;

inline int pair_blocks(int d) { return d * (d + 1) / 2; }
inline int pair_ld(int cap) { return (cap + 3) & ~3; }
inline int pair_stride(int cap) { return pair_ld(cap) + 4; }
inline int pair_tiles(int cap) { return (cap + 15) / 16; }       // 16-column tiles of a block
inline int64_t pair_state_bytes(int d, int cap) { return 2ll * pair_blocks(d) * pair_ld(cap) * pair_stride(cap) * (int64_t)sizeof(double); }
inline bool pair_state_in_lds(int d, int cap) { return pair_state_bytes(d, cap) <= PAIR_LDS_BYTES; }
// global scratch of one workgroup: the Frobenius partials of a step, [block][column tile][t'][t], and the state where LDS does not hold it
inline int64_t pair_workgroup_bytes(int d, int cap) {
    return (int64_t)pair_blocks(d) * pair_tiles(cap) * d * d * (int64_t)sizeof(double) + (pair_state_in_lds(d, cap) ? 0 : pair_state_bytes(d, cap));
}

struct PairPlan {
    bool lds;                       // the carried state lives in LDS
    int64_t workgroups;             // of k_an_pair, persistent over the C T chains
    int64_t rho_bytes;              // of the stored rho_ij of the largest block (0 without mutual information)
    std::vector<int32_t> row0;      // block b is the rows i in [row0[b], row0[b + 1]) of every class: whole rows, at least one
};
// The stored rho_ij (d^4 doubles per pair, C (T - 1 - i) pairs in row i) are cut into blocks of whole rows under block_bytes and under
// an eighth of the query budget; the rest of the budget caps the workgroups through their scratch, never below one.  The model itself
// (its padded copy included) is not counted, as in the other queries.
inline PairPlan pair_plan(int C, int T, int d, int cap, bool store_rho, int64_t block_bytes, size_t free_b, const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    PairPlan p{pair_state_in_lds(d, cap), 1, 0, {0}};
    if (store_rho) {
        const double lim = std::min((double)block_bytes, budget / 8.0);
        const double pair_b = (double)d * d * d * d * sizeof(double);
        double acc = 0.0, worst = 0.0;
        for (int i = 0; i < T; ++i) {
            const double row = (double)C * (T - 1 - i) * pair_b;
            if (i > p.row0.back() && acc + row > lim) {
                p.row0.push_back(i);
                acc = 0.0;
            }
            acc += row;
            worst = std::max(worst, acc);
        }
        p.rho_bytes = (int64_t)worst;
    }
    p.row0.push_back(T);
    const double left = store_rho ? budget * (7.0 / 8.0) : budget;      // a fixed share: the cap is monotone in the budget
    const int64_t chains = (int64_t)C * T;
    p.workgroups = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chains, PAIR_MAX_WORKGROUPS), (int64_t)(left / (double)pair_workgroup_bytes(d, cap))));
    return p;
}

// ---- marginal site conditionals (mpst_margcond.inl: k_mc_walk, k_mc_grid) ----
constexpr int MARGCOND_BIG_MATS = 5;            // chi x chi matrices of global scratch per workgroup of k_mc_walk beyond the LDS limit
constexpr int MARGCOND_MAX_GRID_WORKGROUPS = 4096;      // of k_mc_grid, an (instance, site) pair at a time

struct MargcondBlock {
    int64_t chunk, grid_wgs;            // instances per launch (= workgroups of its walk); workgroups of its grid phase
    int64_t per_bytes;                  // scratch bytes of one instance
};
// Marginal site conditionals.  With budget = query_budget(free_b, chunk_gb), in bytes:
//     per instance    T * (cap * cap * zw + d * d * zw + outputs) * 8     the kept densities of every site, rho_t of every site and the
//                                                                         block's own outputs (`outputs` doubles per (instance, site):
//                                                                         one for each of nll, pit, med, err, mean asked for, and nq)
//                   + MARGCOND_BIG_MATS * cap * cap * zw * 8              on the big route only: the walk is a workgroup per instance
//     chunk    = floor(budget / per instance), at least 1, at most N and at most floor((2^30 - 1) / T), so that chunk * T < 2^30
//                ((instance, site) pairs in 32 bits); whole instances, no rounding: a workgroup of the walk is one instance
//     grid_wgs = min(chunk * T, MARGCOND_MAX_GRID_WORKGROUPS)
// x and the mask ([N][T], 9 bytes per pair) and the 2 * ngrid doubles of every grid workgroup live for the whole call and are not
// counted, as in the site conditionals.
inline MargcondBlock margcond_plan_block(int64_t N, int32_t T, int32_t cap, int32_t d, int32_t zw, int32_t outputs, bool big_route, size_t free_b,
                                         const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const double mat = (double)cap * cap * zw;
    const double per = ((double)T * (mat + (double)d * d * zw + outputs) + (big_route ? MARGCOND_BIG_MATS * mat : 0.0)) * sizeof(double);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(budget / per)));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (((int64_t)1 << 30) - 1) / T));
    return {chunk, std::max<int64_t>(1, std::min<int64_t>(chunk * T, MARGCOND_MAX_GRID_WORKGROUPS)), (int64_t)per};
}

// the blocks [i0, i0 + count) of N instances, `chunk` at a time; stops at the first non-zero result of f and returns it
template <typename F>
inline int for_each_block(int64_t N, int64_t chunk, F&& f) {
    for (int64_t i0 = 0; i0 < N; i0 += chunk)
        if (int rc = f(i0, std::min(chunk, N - i0))) return rc;
    return 0;
}

}  // namespace mpst
