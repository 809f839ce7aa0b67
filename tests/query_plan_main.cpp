// Prints the query plan (csrc/mpst_query_plan.h) of every case on the command line as one JSON document.
// tests/test_query_plan.py compiles this file alone, with the host compiler and its sanitizers, and compares the output with
// tests/golden/query_plan.json.  A case is one of
//     i:<N>:<K>:<T>:<cap>:<zw>:<esz>:<maxm>:<ngrid>:<welems>:<cdf_inst>:<nq>:<u_trials>:<site_grid_doubles>:<dist>:<free bytes>:<override>
//     s:<N>:<T>:<cap>:<d>:<zw>:<free bytes>:<override>          site conditionals
//     m:<N>:<welems>:<esz>:<free bytes>                         marginal likelihoods
//     o:<T>:<backwards>:<keep caller order>:<rows>              the order; rows: comma separated strings of 0 / 1, one per instance
//     c:<ngrid>:<stride>                                        cdf points per site
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

static void blocks(int64_t N, int64_t chunk) {
    printf(",\"blocks\":[");
    for_each_block(N, chunk, [&](int64_t i0, int64_t count) {
        printf("%s[%lld,%lld]", i0 ? "," : "", (long long)i0, (long long)count);
        return 0;
    });
    printf("]");
}

int main(int argc, char** argv) {
    printf("{\"SITECOND_TILE\":%d,\"cases\":[\n", SITECOND_TILE);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split(argv[a], ':');
        auto num = [&](size_t k) { return atoll(f[k].c_str()); };
        auto text = [&](size_t k) { return f[k] == "-" ? nullptr : f[k].c_str(); };
        printf("{\"case\":\"%s\"", argv[a]);
        if (f[0] == "i" && f.size() == 17) {
            ImputeSizes s{};
            s.N = num(1), s.K = num(2), s.T = (int32_t)num(3), s.cap = (int32_t)num(4), s.zw = (int32_t)num(5), s.esz = (int32_t)num(6);
            s.maxm = (int32_t)num(7), s.ngrid = (int32_t)num(8), s.welems = num(9), s.cdf_inst = num(10), s.nq = (int32_t)num(11);
            s.u_trials = (int32_t)num(12), s.site_grid_doubles = num(13), s.dist = num(14) != 0;
            const ImputeBlock b = impute_plan_block(s, (size_t)num(15), text(16));
            printf(",\"per_bytes\":%lld,\"nomem\":%d", (long long)b.per_bytes, b.nomem ? 1 : 0);
            if (!b.nomem) {
                printf(",\"chunk\":%lld", (long long)b.chunk);
                blocks(s.N, b.chunk);
            }
        } else if (f[0] == "s" && f.size() == 8) {
            const SitecondBlock b = sitecond_plan_block(num(1), (int32_t)num(2), (int32_t)num(3), (int32_t)num(4), (int32_t)num(5), (size_t)num(6), text(7));
            printf(",\"chunk\":%lld,\"tiles\":%lld,\"grid_wgs\":%lld", (long long)b.chunk, (long long)b.tiles, (long long)b.grid_wgs);
            blocks(num(1), b.chunk);
        } else if (f[0] == "m" && f.size() == 5) {
            const int64_t chunk = marginal_plan_block(num(1), num(2), (int32_t)num(3), (size_t)num(4));
            printf(",\"chunk\":%lld", (long long)chunk);
            blocks(num(1), chunk);
        } else if (f[0] == "o" && f.size() == 5) {
            const int64_t T = num(1);
            const std::vector<std::string> rows = split(f[4], ',');
            std::vector<uint8_t> missing;
            for (const std::string& r : rows) {
                if ((int64_t)r.size() != T) { fprintf(stderr, "bad row in %s\n", argv[a]); return 2; }
                for (char ch : r) missing.push_back(ch == '1');
            }
            const std::vector<int32_t> order = impute_plan_order(missing.data(), (int64_t)rows.size(), T, num(2) != 0, num(3) != 0);
            printf(",\"order\":[");
            for (size_t i = 0; i < order.size(); ++i) printf("%s%d", i ? "," : "", order[i]);
            printf("]");
        } else if (f[0] == "c" && f.size() == 3) {
            printf(",\"points\":%lld", (long long)cdf_points((int32_t)num(1), (int32_t)num(2)));
        } else {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        printf("}%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
