// The host-side arithmetic of the prefix marginals (mpst_prefix.inl: k_prefix_env, k_prefix_score): the bytes of the model-only G
// tables, whether they fit, and how many series one launch of the walk takes.  Pure functions in plain C++17, no HIP and no
// environment; the query budget is mpst_query_plan.h's.  tests/test_prefix_host.py compiles it alone.
#pragma once
#include "mpst_query_plan.h"

namespace mpst {

constexpr int PREFIX_TILE = SITECOND_TILE;      // series per workgroup of k_prefix_score
constexpr int PREFIX_ENV_BIG_MATS = 3;          // chi x chi matrices of global scratch per workgroup of k_prefix_env beyond the LDS limit

// G^t lives on the bond left of site t, t = 0 .. T.  For t <= label_site the recursion from the right end has passed the label site:
// one matrix per class; for t > label_site one matrix shared by all classes.
inline int64_t prefix_table_mats(int32_t T, int32_t C, int32_t label_site) { return (int64_t)(label_site + 1) * C + (T - label_site); }
// the slot of G_c^t among them (the kernels index the table with the same formula)
inline int64_t prefix_table_slot(int32_t t, int32_t c, int32_t C, int32_t label_site) {
    return t <= label_site ? (int64_t)t * C + c : (int64_t)(label_site + 1) * C + (t - label_site - 1);
}

struct PrefixPlan {
    int64_t mats;               // G matrices, each cap * cap * zw doubles
    int64_t table_bytes;        // what lives for the whole call: the matrices, ln tr [T + 1][C], and on the big route the recursion's scratch
    int64_t per_bytes;          // scratch bytes of one series
    int64_t chunk, tiles;       // series per launch of the walk; its workgroups
    bool nomem;                 // the tables do not fit the budget: chunk and tiles are not set
};
// Prefix marginals.  With budget = query_budget(free_b, chunk_gb), in bytes:
//     tables       mats * cap * cap * zw * 8 + (T + 1) * C * 8  (+ C * PREFIX_ENV_BIG_MATS * cap * cap * zw * 8 on the big route: a
//                  workgroup of k_prefix_env per class).  They are never cut over t: tables beyond the budget are `nomem`.
//     per series   (C + 1) * cap * zw * 8      the row of every class past the label site and the shared row they start from
//                + (T + 1) * C * 8             the block's own results
//     chunk  = floor((budget - tables) / per series), at most N and at most floor((2^30 - 1) / (T + 1)); a chunk smaller than N is whole
//              tiles of PREFIX_TILE series, at least one
//     tiles  = ceil(chunk / PREFIX_TILE)
inline PrefixPlan prefix_plan(int64_t N, int32_t T, int32_t C, int32_t label_site, int32_t cap, int32_t zw, bool big_route, size_t free_b,
                              const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const int64_t mat = (int64_t)cap * cap * zw * (int64_t)sizeof(double);
    PrefixPlan p{prefix_table_mats(T, C, label_site), 0, 0, 0, 0, false};
    p.table_bytes = p.mats * mat + (int64_t)(T + 1) * C * (int64_t)sizeof(double) + (big_route ? (int64_t)C * PREFIX_ENV_BIG_MATS * mat : 0);
    p.per_bytes = ((int64_t)(C + 1) * cap * zw + (int64_t)(T + 1) * C) * (int64_t)sizeof(double);
    if ((double)p.table_bytes > budget) {
        p.nomem = true;
        return p;
    }
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)((budget - (double)p.table_bytes) / (double)p.per_bytes)));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (((int64_t)1 << 30) - 1) / (T + 1)));
    if (chunk < N) chunk = std::max<int64_t>(PREFIX_TILE, chunk / PREFIX_TILE * PREFIX_TILE);
    p.chunk = chunk;
    p.tiles = (chunk + PREFIX_TILE - 1) / PREFIX_TILE;
    return p;
}

}  // namespace mpst
