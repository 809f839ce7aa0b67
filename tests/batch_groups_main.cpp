// Stand-alone driver of csrc/mpst_batch_groups.h for tests/test_batch_groups.py: includes nothing of the library but that header.
// Each argument is one case, "max_group:k0,k1,...": printed as one JSON object {"keys": [...], "index": [[...], ...], "rejected": g}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "mpst_batch_groups.h"

int main(int argc, char** argv) {
    printf("[");
    for (int a = 1; a < argc; ++a) {
        char* p = argv[a];
        const long max_group = strtol(p, &p, 10);
        if (*p != ':') return 2;
        std::vector<int32_t> key;
        do {
            ++p;
            key.push_back((int32_t)strtol(p, &p, 10));
        } while (*p == ',');
        if (*p) return 2;
        mpst::BatchGroups g;
        const int bad = mpst::plan_batch_groups(key.data(), (int)key.size(), (size_t)max_group, &g);
        printf("%s{\"keys\": [", a > 1 ? ",\n" : "");
        for (size_t i = 0; i < g.keys.size(); ++i) printf("%s%d", i ? ", " : "", (int)g.keys[i]);
        printf("], \"index\": [");
        for (size_t i = 0; i < g.index.size(); ++i) {
            printf("%s[", i ? ", " : "");
            for (size_t j = 0; j < g.index[i].size(); ++j) printf("%s%d", j ? ", " : "", g.index[i][j]);
            printf("]");
        }
        printf("], \"rejected\": %d}", bad);
    }
    printf("]\n");
    return 0;
}
