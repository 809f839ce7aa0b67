// How mpst_sweep_batch_multi deals its contexts into groups: plain C++17 without HIP, so that it is tested on the host
// (tests/batch_groups_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mpst {

struct BatchGroups {
    std::vector<int32_t> keys;              // the distinct keys, in order of first appearance
    std::vector<std::vector<int>> index;    // per group: its members' positions in the call, ascending
};

// Groups the K members by key[k].  Returns -1, or the first group (in order of appearance) that holds more than max_group
// members: the call is then to be rejected; *out is complete either way.
inline int plan_batch_groups(const int32_t* key, int K, size_t max_group, BatchGroups* out) {
    out->keys.clear();
    out->index.clear();
    for (int k = 0; k < K; ++k) {
        size_t g = 0;
        while (g < out->keys.size() && out->keys[g] != key[k]) ++g;
        if (g == out->keys.size()) {
            out->keys.push_back(key[k]);
            out->index.emplace_back();
        }
        out->index[g].push_back(k);
    }
    for (size_t g = 0; g < out->index.size(); ++g)
        if (out->index[g].size() > max_group) return (int)g;
    return -1;
}

}  // namespace mpst
