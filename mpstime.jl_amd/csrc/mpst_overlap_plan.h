// The host-side arithmetic of the model overlaps (mpst_overlap.hip: k_overlap): the padded sizes of a pair's state, where it lives, what
// a pair costs, the order in which the pairs are dealt out and how many one launch takes.  Pure functions in plain C++17, no HIP and no
// environment; the query budget is mpst_query_plan.h's.  tests/test_overlap_plan.py compiles it alone.
#pragma once
#include <math.h>
#include <numeric>
#include "mpst_query_plan.h"

namespace mpst {

// A pair (a, b) carries the environment E (rows: the bond of a, columns: the bond of b), the E' of the next site, the environment of
// the other end, and X = E M_b, d times as wide.  Bonds are padded to the 16 x 16 tile of the fp64 MFMA; E has a row stride of two more
// (LDS banks: sixteen rows a wave reads together fall on different ones).  Complex models keep a real and an imaginary plane of each.
constexpr int64_t OVERLAP_LDS_BYTES = 156 * 1024;       // dynamic LDS of k_overlap (160 KB less its static part)
constexpr int64_t OVERLAP_MAX_BLOCK = 1 << 20;          // pairs of one launch

inline int overlap_pad(int chi) { return (chi + 15) & ~15; }
inline int overlap_ld(int cap) { return overlap_pad(cap) + 2; }
inline int64_t overlap_env_doubles(int cap) { return (int64_t)overlap_pad(cap) * overlap_ld(cap); }
inline int64_t overlap_x_doubles(int d, int cap) { return (int64_t)overlap_pad(cap) * d * overlap_pad(cap); }
// cap: the largest bond dimension of any model of the call (every workgroup's state has the same shape); planes: 2 for complex models
inline int64_t overlap_state_bytes(int d, int cap, int planes) {
    return (int64_t)planes * (3 * overlap_env_doubles(cap) + overlap_x_doubles(d, cap)) * (int64_t)sizeof(double);
}
inline bool overlap_state_in_lds(int d, int cap, int planes) { return overlap_state_bytes(d, cap, planes) <= OVERLAP_LDS_BYTES; }
// device bytes a pair holds for the length of its block: its results (g, the exponent), its two indices, and the state where LDS does not hold it
inline int64_t overlap_pair_bytes(int d, int cap, int planes, int cmax) {
    return (int64_t)cmax * cmax * planes * (int64_t)sizeof(double) + (int64_t)sizeof(int64_t) + 2 * (int64_t)sizeof(int32_t) +
           (overlap_state_in_lds(d, cap, planes) ? 0 : overlap_state_bytes(d, cap, planes));
}

// Multiply-adds of the two GEMMs of every site of the walk for the pair of chains with bonds chia[T + 1], chib[T + 1], as padded; the
// label site (p) counts as a site of each class of b.  Real arithmetic: a complex pair costs four times this, which orders nothing.
inline double overlap_pair_cost(const int32_t* chia, const int32_t* chib, int T, int d, int p, int cb) {
    double cost = 0.0;
    for (int j = 0; j < T; ++j) {
        const double al = overlap_pad(chia[j]), ar = overlap_pad(chia[j + 1]), bl = overlap_pad(chib[j]), br = overlap_pad(chib[j + 1]);
        const double in_a = j <= p ? al : ar, out_a = j <= p ? ar : al, in_b = j <= p ? bl : br, out_b = j <= p ? br : bl;
        cost += (in_a * in_b * d * out_b + out_a * in_a * d * out_b) * (j == p ? cb : 1);
    }
    return cost;
}

// the pairs most expensive first; ties keep the caller's order.  Results do not depend on the order.
inline std::vector<int32_t> overlap_pair_order(const std::vector<double>& cost) {
    std::vector<int32_t> order(cost.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
    return order;
}

// pairs per launch: what the query budget holds of them, at least one
inline int64_t overlap_block_pairs(int64_t P, int64_t pair_bytes, size_t free_b, const char* chunk_gb) {
    const int64_t fit = (int64_t)std::min(query_budget(free_b, chunk_gb) / (double)pair_bytes, (double)OVERLAP_MAX_BLOCK);
    return std::max<int64_t>(1, std::min<int64_t>(P, fit));
}

}  // namespace mpst
