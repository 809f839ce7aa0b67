// Stand-alone driver of csrc/mpst_bond_plan.h for tests/test_bond_plan.py: includes nothing of the library but that header.
// Each argument is one case and prints one line of integers (null: a null pointer):
//   slot:T,k       "slot T k  lid going_left next_lid chains_into_next  site left_side prev_site prev_bond out_bond out_site" (the bond's step)
//   env:T,site,left "env T site left  site left_side prev_site prev_bond out_bond out_site"
//   row:site,stride,esz "row site stride esz  <byte offset of env_row<double>> <byte offset of env_row_e>"
//   yhat:d,cap,v1  "yhat d cap v1  row"          grad:d,nw  "grad d nw  row"
//   lists          "yhat_list n  LM D4 V2 ..." and "grad_list n  AW2 D2 FS KC NW threads ..." on two lines, from the X-macros
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mpst_bond_plan.h"

static void print_step(const mpst::EnvStep& e) { printf(" %d %d %d %d %d %d\n", e.site, e.left_side, e.prev_site, e.prev_bond, e.out_bond, e.out_site); }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        char* p = strchr(argv[a], ':');
        const std::string what(argv[a], p ? (size_t)(p - argv[a]) : strlen(argv[a]));
        std::vector<long> x;
        while (p && *p) x.push_back(strtol(p + 1, &p, 10));
        if (what == "slot" && x.size() == 2) {
            const int T = (int)x[0], k = (int)x[1];
            const mpst::BondSlot b = mpst::bond_slot(k, T - 1);
            printf("slot %d %d %d %d %d %d", T, k, b.lid, b.going_left, b.next_lid, (int)b.chains_into_next);
            print_step(mpst::env_step_of_bond(b.lid, b.going_left, T));
        } else if (what == "env" && x.size() == 3) {
            printf("env %ld %ld %ld", x[0], x[1], x[2]);
            print_step(mpst::env_step((int)x[1], (int)x[2], (int)x[0]));
        } else if (what == "row" && x.size() == 3) {
            const int site = (int)x[0];
            const int64_t stride = x[1];
            const size_t esz = (size_t)x[2];
            std::vector<double> rows((size_t)(site < 0 ? 1 : site + 1) * stride * (esz / sizeof(double) + 1));      // holds row `site` either way
            double* r = mpst::env_row(rows.data(), site, stride);
            char* e = (char*)mpst::env_row_e(rows.data(), site, stride, esz);
            printf("row %d %ld %ld ", site, (long)stride, (long)esz);
            if (r) { *r = 1.0; printf("%ld ", (long)((char*)r - (char*)rows.data())); } else printf("null ");
            if (e) { *e = 1; printf("%ld\n", (long)(e - (char*)rows.data())); } else printf("null\n");
        } else if (what == "yhat" && x.size() == 3) {
            printf("yhat %ld %ld %ld %d\n", x[0], x[1], x[2], mpst::yhat_s_variant((int)x[0], (int)x[1], x[2] != 0));
        } else if (what == "grad" && x.size() == 2) {
            printf("grad %ld %ld %d\n", x[0], x[1], mpst::grad_s_variant((int)x[0], (int)x[1]));
        } else if (what == "lists") {
#define X(LM, D4, V2) +1
            int n = 0 YHAT_S_LIST(X);
#undef X
            printf("yhat_list %d", n);
#define X(LM, D4, V2) printf(" %d %d %d", LM, (int)D4, (int)V2);
            YHAT_S_LIST(X)
#undef X
#define X(AW2, D2, FS, KC, NW, THREADS) +1
            n = 0 GRAD_S_LIST(X);
#undef X
            printf("\ngrad_list %d", n);
#define X(AW2, D2, FS, KC, NW, THREADS) printf(" %d %d %d %d %d %d", AW2, D2, FS, KC, NW, THREADS);
            GRAD_S_LIST(X)
#undef X
            printf("\n");
        } else
            return 2;
    }
    return 0;
}
