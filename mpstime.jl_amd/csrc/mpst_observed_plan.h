// The host-side arithmetic of the observed conditionals (mpst_observed.inl: k_obs_operator, k_obs_walk, k_obs_grid): how many series one
// block takes.  Pure functions in plain C++17, no HIP and no environment; the query budget is mpst_query_plan.h's.
// tests/test_observed_plan.py compiles it alone.
#pragma once
#include "mpst_query_plan.h"

namespace mpst {

constexpr int OBSERVED_MAX_GRID_WORKGROUPS = MARGCOND_MAX_GRID_WORKGROUPS;      // of k_obs_operator and k_obs_grid, an (instance, site) pair at a time

struct ObservedBlock {
    int64_t chunk, grid_wgs;            // instances per launch (= workgroups of its walk); workgroups of its operator kernel and its grid phase
    int64_t per_bytes;                  // scratch bytes of one instance
};
// Observed conditionals.  With budget = query_budget(free_b, chunk_gb), in bytes:
//     per instance    T * (cap * cap * zw + d * d * zw + outputs) * 8     what margcond_plan_block counts: the kept densities, rho_t and the
//                                                                         block's own per-site outputs (`outputs` doubles per (instance,
//                                                                         site): one for each of nll_obs, pit and the med, err, mean of
//                                                                         either group asked for, nq for each q asked for)
//                   + T * d * d * zw * 8                                  the operator of every site
//                   + 8                                                   logev
//                   + MARGCOND_BIG_MATS * cap * cap * zw * 8              on the big route only: the walk is a workgroup per instance
//     chunk    = floor(budget / per instance), at least 1, at most N and at most floor((2^30 - 1) / T); whole instances
//     grid_wgs = min(chunk * T, OBSERVED_MAX_GRID_WORKGROUPS)
// kind, a, b and x ([N][T], 25 bytes per pair) and the 2 * ngrid doubles of every grid workgroup live for the whole call and are not
// counted, as in the marginal conditionals.
inline ObservedBlock observed_plan_block(int64_t N, int32_t T, int32_t cap, int32_t d, int32_t zw, int32_t outputs, bool big_route, size_t free_b,
                                         const char* chunk_gb) {
    const double budget = query_budget(free_b, chunk_gb);
    const double mat = (double)cap * cap * zw, op = (double)d * d * zw;
    const double per = ((double)T * (mat + 2.0 * op + outputs) + 1.0 + (big_route ? MARGCOND_BIG_MATS * mat : 0.0)) * sizeof(double);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(budget / per)));
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (((int64_t)1 << 30) - 1) / T));
    return {chunk, std::max<int64_t>(1, std::min<int64_t>(chunk * T, OBSERVED_MAX_GRID_WORKGROUPS)), (int64_t)per};
}

}  // namespace mpst
