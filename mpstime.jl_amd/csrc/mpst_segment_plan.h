// The host-side arithmetic of the segment marginals (mpst_segment.inl: k_segment_left, k_prefix_env, k_segment_walk): the bytes of the
// model-only L and G tables, whether they fit, how many workgroups the walk keeps resident and how many series one launch of it takes.
// Pure functions in plain C++17, no HIP and no environment; the query budget is mpst_query_plan.h's.  tests/test_segment_host.py
// compiles it alone.
#pragma once
#include "mpst_prefix_plan.h"

namespace mpst {

constexpr int SEGMENT_TILE = SITECOND_TILE;     // a block of series smaller than N is a whole number of these
constexpr int SEGMENT_BIG_MATS = 5;             // chi x chi matrices of global scratch per workgroup of k_segment_walk beyond the LDS limit
constexpr int SEGMENT_WGS_PER_CU = 4;           // resident workgroups of k_segment_walk per compute unit ...
constexpr int SEGMENT_BIG_WGS_PER_CU = 2;       // ... and where each owns global scratch

// L^t lives on the bond left of site t, t = 0 .. T, as G^t does.  For t <= label_site the recursion from the left end has not met the
// label site: one matrix shared by all classes; for t > label_site one matrix per class.  With the G tables (prefix_table_mats) that
// is (T + 1)(C + 1) matrices whatever the label site.
inline int64_t segment_left_mats(int32_t T, int32_t C, int32_t label_site) { return (int64_t)(label_site + 1) + (int64_t)(T - label_site) * C; }
// the slot of L_c^t among them (the kernels index the table with the same formula)
inline int64_t segment_left_slot(int32_t t, int32_t c, int32_t C, int32_t label_site) {
    return t <= label_site ? (int64_t)t : (int64_t)(label_site + 1) + (int64_t)(t - label_site - 1) * C + c;
}
// the persistent workgroups of the walk, a (series, start) item at a time: a fixed number per compute unit, never more than the items
// of the largest launch
inline int64_t segment_walk_workgroups(int32_t cus, bool big_route, int64_t items) {
    const int64_t per_cu = big_route ? SEGMENT_BIG_WGS_PER_CU : SEGMENT_WGS_PER_CU;
    return std::max<int64_t>(1, std::min<int64_t>(items, per_cu * std::max<int32_t>(1, cus)));
}

struct SegmentPlan {
    int64_t mats;               // L and G matrices, each cap * cap * zw doubles
    int64_t walk_wgs;           // workgroups of k_segment_walk, whatever the block
    int64_t table_bytes;        // what lives for the whole call: the matrices, lnL and lnG [T + 1][C], and on the big route the scratch
    int64_t per_bytes;          // result bytes of one series
    int64_t chunk;              // series per launch of the walk
    bool nomem;                 // the tables do not fit the budget: chunk is not set
};
// Segment marginals.  With budget = query_budget(free_b, chunk_gb), in bytes:
//     tables       (T + 1)(C + 1) * cap * cap * zw * 8 + 2 * (T + 1) * C * 8, and on the big route
//                  (2 * C * PREFIX_ENV_BIG_MATS + walk_wgs * SEGMENT_BIG_MATS) * cap * cap * zw * 8: a workgroup per class of each table
//                  kernel, and the walk's scratch per RESIDENT workgroup, not per item.  They are never cut: tables beyond the budget
//                  are `nomem`.
//     per series   T * max_width * C * 8       the block's own results
//     walk_wgs = segment_walk_workgroups(cus, big_route, N * T)
//     chunk    = floor((budget - tables) / per series), at most N and at most floor((2^30 - 1) / (T * max_width)) (entries of a
//                block and class in 30 bits); a chunk smaller than N is whole tiles of SEGMENT_TILE series, at least one
inline SegmentPlan segment_plan(int64_t N, int32_t T, int32_t C, int32_t label_site, int32_t cap, int32_t zw, int32_t max_width, bool big_route,
                                int32_t cus, size_t free_b, const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const int64_t mat = (int64_t)cap * cap * zw * (int64_t)sizeof(double);
    SegmentPlan p{prefix_table_mats(T, C, label_site) + segment_left_mats(T, C, label_site), 0, 0, 0, 0, false};
    p.walk_wgs = segment_walk_workgroups(cus, big_route, N * T);
    p.table_bytes = p.mats * mat + 2 * (int64_t)(T + 1) * C * (int64_t)sizeof(double) +
                    (big_route ? (2 * (int64_t)C * PREFIX_ENV_BIG_MATS + p.walk_wgs * SEGMENT_BIG_MATS) * mat : 0);
    p.per_bytes = (int64_t)T * max_width * C * (int64_t)sizeof(double);
    if ((double)p.table_bytes > budget) {
        p.nomem = true;
        return p;
    }
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)((budget - (double)p.table_bytes) / (double)p.per_bytes)));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (((int64_t)1 << 30) - 1) / ((int64_t)T * max_width)));
    if (chunk < N) chunk = std::max<int64_t>(SEGMENT_TILE, chunk / SEGMENT_TILE * SEGMENT_TILE);
    p.chunk = chunk;
    return p;
}

}  // namespace mpst
