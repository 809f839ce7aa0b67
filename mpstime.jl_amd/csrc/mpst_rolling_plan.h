// The host-side arithmetic of the rolling-origin forecasts (mpst_rolling.inl: k_roll_rows, k_prefix_env, k_roll_tables, k_roll_score,
// k_roll_grid): the bytes of what lives for the whole call, how many targets one block of tables holds, and how many series one block
// takes.  Pure functions in plain C++17, no HIP and no environment; the query budget is mpst_query_plan.h's.
// tests/test_rolling_plan.py compiles it alone.
#pragma once
#include "mpst_prefix_plan.h"

namespace mpst {

constexpr int ROLLING_TILE = SITECOND_TILE;             // series per workgroup of k_roll_rows and k_roll_score
constexpr int ROLLING_MAX_TABLE_WORKGROUPS = 1024;      // of k_roll_tables, a (target, class, pair s <= s') chain at a time; each owns one matrix of scratch
constexpr int ROLLING_MAX_GRID_WORKGROUPS = 4096;       // of k_roll_grid, a (series, origin, horizon) triple at a time

inline int rolling_pairs(int d) { return d * (d + 1) / 2; }
// the pair s <= s' among them, row by row of the upper triangle (the kernels use the same formula)
inline int rolling_pair_index(int s, int sp, int d) { return s * d - s * (s - 1) / 2 + (sp - s); }
// matrices a target u keeps: K_c^{t,u}[s,s'] for t = u .. u-H+1, every class and every pair.  Slot ((ul * H + (u - t)) * C + c) * pairs + pair,
// ul the target's index in its block.
inline int64_t rolling_target_mats(int32_t H, int32_t C, int32_t d) { return (int64_t)H * C * rolling_pairs(d); }

struct RollingPlan {
    int64_t fixed_bytes;        // what lives for the whole call
    int64_t target_bytes;       // table bytes of one target
    int64_t per_bytes;          // scratch and result bytes of one series
    int64_t table_wgs;          // workgroups of k_roll_tables (and matrices of its scratch)
    int64_t tblock;             // targets per block of tables
    int64_t chunk;              // series per block
    int64_t grid_wgs;           // workgroups of k_roll_grid for a full block
    bool nomem;                 // G / lnG and the scratch do not fit the budget: the blocks are not set
};
// Rolling forecasts.  With budget = query_budget(free_b, chunk_gb), mat = cap * cap * zw * 8 and pairs = d (d + 1) / 2, in bytes:
//     fixed        prefix_table_mats(T, C, label_site) * mat + (T + 1) * C * 8      G and lnG of k_prefix_env
//                  (+ C * PREFIX_ENV_BIG_MATS * mat on the big route: its scratch)
//                  + table_wgs * mat,  table_wgs = min(ROLLING_MAX_TABLE_WORKGROUPS, T * C * pairs)      the scratch of k_roll_tables
//                  Never cut: beyond the budget is `nomem`.
//     per target   H * C * pairs * mat         its chains; a target's matrices are used by H origins and dropped with its block
//     per series   T * C * (cap * zw + 1) * 8  the normalised row of every origin and class, and its log
//                + T * H * d * d * zw * 8      rho of every triple
//                + T * H * outputs * 8         the block's own results (`outputs` doubles per triple: one for each of nll, pit, med, err,
//                                              mean asked for, and nq)
//     tblock   = floor((budget - fixed) / 2 / per target), at least 1 and at most T: the tables take at most half of what is left unless
//                a single target is larger
//     chunk    = floor((budget - fixed - tblock * per target) / per series), at least 1, at most N and at most
//                floor((2^30 - 1) / (T * H)) (triples of a block in 30 bits); a chunk smaller than N is whole tiles of ROLLING_TILE
//                series, at least one
//     grid_wgs = min(chunk * T * H, ROLLING_MAX_GRID_WORKGROUPS)
inline RollingPlan rolling_plan(int64_t N, int32_t T, int32_t C, int32_t label_site, int32_t cap, int32_t d, int32_t zw, int32_t H, int32_t outputs,
                                bool big_route, size_t free_b, const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const int64_t mat = (int64_t)cap * cap * zw * (int64_t)sizeof(double), dbl = (int64_t)sizeof(double);
    RollingPlan p{};
    p.table_wgs = std::min<int64_t>(ROLLING_MAX_TABLE_WORKGROUPS, (int64_t)T * C * rolling_pairs(d));
    p.fixed_bytes = prefix_table_mats(T, C, label_site) * mat + (int64_t)(T + 1) * C * dbl + (big_route ? (int64_t)C * PREFIX_ENV_BIG_MATS * mat : 0) +
                    p.table_wgs * mat;
    p.target_bytes = rolling_target_mats(H, C, d) * mat;
    p.per_bytes = ((int64_t)T * C * ((int64_t)cap * zw + 1) + (int64_t)T * H * ((int64_t)d * d * zw + outputs)) * dbl;
    if ((double)p.fixed_bytes > budget) {
        p.nomem = true;
        return p;
    }
    const double left = budget - (double)p.fixed_bytes;
    p.tblock = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)(0.5 * left / (double)p.target_bytes)));
    int64_t chunk = (int64_t)((left - (double)(p.tblock * p.target_bytes)) / (double)p.per_bytes);
    chunk = std::max<int64_t>(1, std::min<int64_t>(N, chunk));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (((int64_t)1 << 30) - 1) / ((int64_t)T * H)));
    if (chunk < N) chunk = std::max<int64_t>(ROLLING_TILE, chunk / ROLLING_TILE * ROLLING_TILE);
    p.chunk = chunk;
    p.grid_wgs = std::max<int64_t>(1, std::min<int64_t>(chunk * T * H, ROLLING_MAX_GRID_WORKGROUPS));
    return p;
}

}  // namespace mpst
