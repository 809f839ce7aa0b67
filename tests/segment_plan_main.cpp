// Prints the segment-marginal plan (csrc/mpst_segment_plan.h: segment_plan) of every case on the command line as one JSON document.
// tests/test_segment_host.py compiles this file alone, with the host compiler and its sanitizers.  A case is
//     s:<N>:<T>:<C>:<label site>:<cap>:<zw>:<max width>:<big route>:<compute units>:<free bytes>:<override>
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_segment_plan.h"

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
    printf("{\"SEGMENT_TILE\":%d,\"SEGMENT_BIG_MATS\":%d,\"SEGMENT_WGS_PER_CU\":%d,\"SEGMENT_BIG_WGS_PER_CU\":%d,\"cases\":[\n", SEGMENT_TILE,
           SEGMENT_BIG_MATS, SEGMENT_WGS_PER_CU, SEGMENT_BIG_WGS_PER_CU);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        if (f[0] != "s" || f.size() != 12) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        const int64_t N = num(1);
        const int32_t T = (int32_t)num(2), C = (int32_t)num(3), ls = (int32_t)num(4);
        const SegmentPlan p = segment_plan(N, T, C, ls, (int32_t)num(5), (int32_t)num(6), (int32_t)num(7), num(8) != 0, (int32_t)num(9), (size_t)num(10),
                                           f[11] == "-" ? nullptr : f[11].c_str());
        // every (t, class) names a slot of the left table below its size; the classes share a slot exactly where t <= label site; every
        // slot is named once
        const int64_t left = segment_left_mats(T, C, ls);
        std::vector<int> hits((size_t)left, 0);
        bool slots_ok = left + prefix_table_mats(T, C, ls) == p.mats;
        for (int32_t t = 0; t <= T; ++t)
            for (int32_t c = 0; c < C; ++c) {
                const int64_t s = segment_left_slot(t, c, C, ls);
                if (s < 0 || s >= left || (t <= ls && s != segment_left_slot(t, 0, C, ls))) slots_ok = false;
                else if (t > ls || c == 0) ++hits[(size_t)s];
            }
        for (int h : hits) slots_ok = slots_ok && h == 1;
        int64_t nblocks = 0, covered = 0, largest = 0, ragged = 0;
        if (!p.nomem)
            for_each_block(N, p.chunk, [&](int64_t i0, int64_t count) {
                if (i0 != covered) return 1;
                ++nblocks;
                covered += count;
                if (count > largest) largest = count;
                if (i0 + count < N && count % SEGMENT_TILE) ++ragged;
                return 0;
            });
        printf("{\"case\":\"%s\",\"mats\":%lld,\"walk_wgs\":%lld,\"table_bytes\":%lld,\"per_bytes\":%lld,\"nomem\":%d,\"chunk\":%lld,\"slots_ok\":%d,"
               "\"nblocks\":%lld,\"covered\":%lld,\"largest\":%lld,\"ragged\":%lld}%s\n", argv[a], (long long)p.mats, (long long)p.walk_wgs,
               (long long)p.table_bytes, (long long)p.per_bytes, p.nomem ? 1 : 0, (long long)p.chunk, slots_ok ? 1 : 0, (long long)nblocks,
               (long long)covered, (long long)largest, (long long)ragged, a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
