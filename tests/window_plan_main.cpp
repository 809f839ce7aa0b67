// Prints the window-conditional plan (csrc/mpst_query_plan.h: window_plan_block) of every case on the command line as one JSON document.
// tests/test_window_plan.py compiles this file alone, with the host compiler and its sanitizers.  A case is
//     w:<N>:<T>:<cap>:<zw>:<max_width>:<big route>:<free bytes>:<override>
// where <override> is the text of MPST_IMPUTE_CHUNK_GB or - for none.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mpst_query_plan.h"

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
    printf("{\"SITECOND_TILE\":%d,\"WINDOW_BIG_MATS\":%d,\"WINDOW_MAX_WORKGROUPS\":%d,\"WINDOW_MAX_BIG_WORKGROUPS\":%d,\"cases\":[\n", SITECOND_TILE,
           WINDOW_BIG_MATS, WINDOW_MAX_WORKGROUPS, WINDOW_MAX_BIG_WORKGROUPS);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        if (f[0] != "w" || f.size() != 9) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        const int64_t N = num(1);
        const WindowBlock b = window_plan_block(N, (int32_t)num(2), (int32_t)num(3), (int32_t)num(4), (int32_t)num(5), num(6) != 0, (size_t)num(7),
                                                f[8] == "-" ? nullptr : f[8].c_str());
        printf("{\"case\":\"%s\",\"chunk\":%lld,\"tiles\":%lld,\"win_wgs\":%lld,\"blocks\":[", argv[a], (long long)b.chunk, (long long)b.tiles,
               (long long)b.win_wgs);
        for_each_block(N, b.chunk, [&](int64_t i0, int64_t count) {
            printf("%s[%lld,%lld]", i0 ? "," : "", (long long)i0, (long long)count);
            return 0;
        });
        printf("]}%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
