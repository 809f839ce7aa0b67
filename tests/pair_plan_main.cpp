// Prints the pair analysis plan (csrc/mpst_query_plan.h: pair_plan and the limit functions beside it) of every case on the command
// line as one JSON document.  tests/pair_plan.py compiles this file alone with the host compiler.  A case is
//     p:<C>:<T>:<d>:<cap>:<store rho>:<block bytes>:<free bytes>:<override>
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_query_plan.h"

using namespace mpst;

int main(int argc, char** argv) {
    printf("{\"PAIR_LDS_BYTES\":%lld,\"PAIR_MAX_WORKGROUPS\":%d,\"cases\":[\n", (long long)PAIR_LDS_BYTES, PAIR_MAX_WORKGROUPS);
    for (int a = 1; a < argc; ++a) {
        std::vector<std::string> f;
        const std::string s = argv[a];
        for (size_t i = 0; i <= s.size();) {
            size_t j = s.find(':', i);
            if (j == std::string::npos) j = s.size();
            f.push_back(s.substr(i, j - i));
            i = j + 1;
        }
        if (f.size() != 9 || f[0] != "p") {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        const int C = (int)num(1), T = (int)num(2), d = (int)num(3), cap = (int)num(4);
        const PairPlan p = pair_plan(C, T, d, cap, num(5) != 0, num(6), (size_t)num(7), f[8] == "-" ? nullptr : f[8].c_str());
        printf("{\"case\":\"%s\",\"lds\":%d,\"workgroups\":%lld,\"rho_bytes\":%lld,\"state_bytes\":%lld,\"workgroup_bytes\":%lld,\"ld\":%d,\"stride\":%d,"
               "\"tiles\":%d,\"row0\":[",
               argv[a], p.lds ? 1 : 0, (long long)p.workgroups, (long long)p.rho_bytes, (long long)pair_state_bytes(d, cap),
               (long long)pair_workgroup_bytes(d, cap), pair_ld(cap), pair_stride(cap), pair_tiles(cap));
        for (size_t i = 0; i < p.row0.size(); ++i) printf("%s%d", i ? "," : "", p.row0[i]);
        printf("]}%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
