// Prints the observed-conditional plan (csrc/mpst_observed_plan.h: observed_plan_block) of every case on the command line as one JSON
// document.  tests/test_observed_plan.py compiles this file alone, with the host compiler and its sanitizers.  A case is
//     o:<N>:<T>:<cap>:<d>:<zw>:<outputs>:<big route>:<free bytes>:<override>
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_observed_plan.h"

using namespace mpst;

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> f;
    for (size_t i = 0; i <= s.size();) {
        size_t j = s.find(sep, i);
        if (j == std::string::npos) j = s.size();
        f.push_back(s.substr(i, j - i));
        i = j + 1;
    }
    return f;
}

int main(int argc, char** argv) {
    printf("{\"MARGCOND_BIG_MATS\":%d,\"OBSERVED_MAX_GRID_WORKGROUPS\":%d,\"cases\":[\n", MARGCOND_BIG_MATS, OBSERVED_MAX_GRID_WORKGROUPS);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        if (f[0] != "o" || f.size() != 10) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        const int64_t N = num(1);
        const ObservedBlock b = observed_plan_block(N, (int32_t)num(2), (int32_t)num(3), (int32_t)num(4), (int32_t)num(5), (int32_t)num(6), num(7) != 0,
                                                    (size_t)num(8), f[9] == "-" ? nullptr : f[9].c_str());
        int64_t nblocks = 0, covered = 0, largest = 0;
        for_each_block(N, b.chunk, [&](int64_t i0, int64_t count) {
            if (i0 != covered) return 1;
            ++nblocks;
            covered += count;
            if (count > largest) largest = count;
            return 0;
        });
        printf("{\"case\":\"%s\",\"chunk\":%lld,\"grid_wgs\":%lld,\"per_bytes\":%lld,\"nblocks\":%lld,\"covered\":%lld,\"largest\":%lld}%s\n", argv[a],
               (long long)b.chunk, (long long)b.grid_wgs, (long long)b.per_bytes, (long long)nblocks, (long long)covered, (long long)largest,
               a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
