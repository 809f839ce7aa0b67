// Prints the rolling-forecast plan (csrc/mpst_rolling_plan.h: rolling_plan) of every case on the command line as one JSON document.
// tests/test_rolling_plan.py compiles this file alone, with the host compiler and its sanitizers.  A case is
//     r:<N>:<T>:<C>:<label site>:<cap>:<d>:<zw>:<max horizon>:<outputs>:<big route>:<free bytes>:<override>
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_rolling_plan.h"

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
    printf("{\"ROLLING_TILE\":%d,\"ROLLING_MAX_TABLE_WORKGROUPS\":%d,\"ROLLING_MAX_GRID_WORKGROUPS\":%d,\"cases\":[\n", ROLLING_TILE,
           ROLLING_MAX_TABLE_WORKGROUPS, ROLLING_MAX_GRID_WORKGROUPS);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        if (f[0] != "r" || f.size() != 13) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        const int64_t N = num(1);
        const int32_t T = (int32_t)num(2), C = (int32_t)num(3), d = (int32_t)num(6), H = (int32_t)num(8);
        const RollingPlan p = rolling_plan(N, T, C, (int32_t)num(4), (int32_t)num(5), d, (int32_t)num(7), H, (int32_t)num(9), num(10) != 0,
                                           (size_t)num(11), f[12] == "-" ? nullptr : f[12].c_str());
        // every pair s <= s' names a slot below the number of pairs, every slot once
        std::vector<int> hits((size_t)rolling_pairs(d), 0);
        bool pairs_ok = rolling_target_mats(H, C, d) == (int64_t)H * C * rolling_pairs(d);
        for (int s = 0; s < d; ++s)
            for (int sp = s; sp < d; ++sp) {
                const int k = rolling_pair_index(s, sp, d);
                if (k < 0 || k >= rolling_pairs(d)) pairs_ok = false;
                else ++hits[(size_t)k];
            }
        for (int h : hits) pairs_ok = pairs_ok && h == 1;
        int64_t nblocks = 0, covered = 0, largest = 0, ragged = 0, tblocks = 0, tcovered = 0;
        if (!p.nomem) {
            for_each_block(N, p.chunk, [&](int64_t i0, int64_t count) {
                if (i0 != covered) return 1;
                ++nblocks;
                covered += count;
                if (count > largest) largest = count;
                if (i0 + count < N && count % ROLLING_TILE) ++ragged;
                return 0;
            });
            for_each_block(T, p.tblock, [&](int64_t u0, int64_t count) {
                if (u0 != tcovered) return 1;
                ++tblocks;
                tcovered += count;
                return 0;
            });
        }
        printf("{\"case\":\"%s\",\"fixed_bytes\":%lld,\"target_bytes\":%lld,\"per_bytes\":%lld,\"table_wgs\":%lld,\"nomem\":%d,\"tblock\":%lld,"
               "\"chunk\":%lld,\"grid_wgs\":%lld,\"pairs_ok\":%d,\"nblocks\":%lld,\"covered\":%lld,\"largest\":%lld,\"ragged\":%lld,\"tblocks\":%lld,"
               "\"tcovered\":%lld}%s\n", argv[a], (long long)p.fixed_bytes, (long long)p.target_bytes, (long long)p.per_bytes, (long long)p.table_wgs,
               p.nomem ? 1 : 0, (long long)p.tblock, (long long)p.chunk, (long long)p.grid_wgs, pairs_ok ? 1 : 0, (long long)nblocks,
               (long long)covered, (long long)largest, (long long)ragged, (long long)tblocks, (long long)tcovered, a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
