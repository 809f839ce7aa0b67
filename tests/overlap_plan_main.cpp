// Prints the model overlaps plan (csrc/mpst_overlap_plan.h) of every case on the command line as one JSON document.
// tests/test_overlap_plan.py compiles this file alone with the host compiler.  A case is
//     v:<d>:<cap>:<planes>:<cmax>:<P>:<free bytes>:<override>        sizes, route and pairs per launch
//     o:<T>:<d>:<p>:<chi of model 0>/<chi of model 1>/...:<C,C,...>  cost and order of every pair a <= b; a chi is T + 1 numbers joined by ,
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_overlap_plan.h"

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
    printf("{\"OVERLAP_LDS_BYTES\":%lld,\"OVERLAP_MAX_BLOCK\":%lld,\"cases\":[\n", (long long)OVERLAP_LDS_BYTES, (long long)OVERLAP_MAX_BLOCK);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        if (f.size() == 8 && f[0] == "v") {
            const int d = (int)num(1), cap = (int)num(2), planes = (int)num(3), cmax = (int)num(4);
            const int64_t P = num(5), pair_bytes = overlap_pair_bytes(d, cap, planes, cmax);
            const int64_t block = overlap_block_pairs(P, pair_bytes, (size_t)num(6), f[7] == "-" ? nullptr : f[7].c_str());
            printf("{\"case\":\"%s\",\"pad\":%d,\"ld\":%d,\"env\":%lld,\"x\":%lld,\"state_bytes\":%lld,\"lds\":%d,\"pair_bytes\":%lld,\"block\":%lld}", argv[a],
                   overlap_pad(cap), overlap_ld(cap), (long long)overlap_env_doubles(cap), (long long)overlap_x_doubles(d, cap),
                   (long long)overlap_state_bytes(d, cap, planes), overlap_state_in_lds(d, cap, planes) ? 1 : 0, (long long)pair_bytes, (long long)block);
        } else if (f.size() == 6 && f[0] == "o") {
            const int T = (int)num(1), d = (int)num(2), p = (int)num(3);
            std::vector<std::vector<int32_t>> chi;
            for (const std::string& m : split(f[4], '/')) {
                chi.emplace_back();
                for (const std::string& x : split(m, ',')) chi.back().push_back(atoi(x.c_str()));
                if ((int)chi.back().size() != T + 1) {
                    fprintf(stderr, "bad chi in %s\n", argv[a]);
                    return 2;
                }
            }
            std::vector<int> ncls;
            for (const std::string& x : split(f[5], ',')) ncls.push_back(atoi(x.c_str()));
            if (ncls.size() != chi.size()) {
                fprintf(stderr, "bad classes in %s\n", argv[a]);
                return 2;
            }
            std::vector<double> cost;
            for (size_t x = 0; x < chi.size(); ++x)
                for (size_t y = x; y < chi.size(); ++y) cost.push_back(overlap_pair_cost(chi[x].data(), chi[y].data(), T, d, p, ncls[y]));
            const std::vector<int32_t> order = overlap_pair_order(cost);
            printf("{\"case\":\"%s\",\"cost\":[", argv[a]);
            for (size_t i = 0; i < cost.size(); ++i) printf("%s%.17g", i ? "," : "", cost[i]);
            printf("],\"order\":[");
            for (size_t i = 0; i < order.size(); ++i) printf("%s%d", i ? "," : "", order[i]);
            printf("]}");
        } else {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        printf("%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
