// Prints the data set plan (csrc/mpst_dataset_plan.h) of every case on the command line as one JSON document.
// tests/test_dataset_plan.py compiles this file alone, with the host compiler and its sanitizers, and compares the output with
// tests/golden/dataset_plan.json.  A case is
//     c:<counts>:<global counts or ->:<parts target override, 0 = none>     labels 0..C-1 expanded from the per-class counts
//     l:<C>:<labels>                                                        the labels as given (rejections)
// with comma separated lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mpst_dataset_plan.h"

using namespace mpst;

static std::vector<int64_t> csv(const std::string& s) {
    std::vector<int64_t> v;
    for (size_t i = 0; i < s.size();) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        v.push_back(atoll(s.substr(i, j - i).c_str()));
        i = j + 1;
    }
    return v;
}

static std::vector<std::string> fields(const std::string& s) {
    std::vector<std::string> f;
    for (size_t i = 0; i <= s.size();) {
        size_t j = s.find(':', i);
        if (j == std::string::npos) j = s.size();
        f.push_back(s.substr(i, j - i));
        i = j + 1;
    }
    return f;
}

template <typename V>
static void list(const V& v) {
    printf("[");
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}
template <typename V>
static void ints(const char* name, const V& v) {
    printf("\"%s\":", name);
    list(v);
    printf(",");
}
static void spans(const char* name, const std::vector<Span>& v) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s[%d,%d,%d,%d]", i ? "," : "", v[i].start, v[i].count, v[i].cls, v[i].pad);
    printf("],");
}
static void parts(const std::vector<Part>& v) {
    printf("[");
    for (size_t i = 0; i < v.size(); ++i)
        printf("%s[%d,%d,%d,%d,%d,%d,%d,%d]", i ? "," : "", v[i].start, v[i].count, v[i].own, v[i].cls, v[i].first_of_cls, v[i].pad0, v[i].pad1, v[i].pad2);
    printf("]");
}

int main(int argc, char** argv) {
    printf("{\"TILE_S\":%d,\"CHUNK_S\":%d,\"PARTS_TARGET\":%d,\"cases\":[\n", TILE_S, CHUNK_S, PARTS_TARGET);
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = fields(argv[a]);
        std::vector<int32_t> labels;
        std::vector<int64_t> gc;
        int C = 0, target = 0;
        if (f.size() == 4 && f[0] == "c") {
            const std::vector<int64_t> counts = csv(f[1]);
            C = (int)counts.size();
            for (int k = 0; k < C; ++k) labels.insert(labels.end(), (size_t)counts[k], (int32_t)k);
            if (f[2] != "-") gc = csv(f[2]);
            target = atoi(f[3].c_str());
        } else if (f.size() == 3 && f[0] == "l") {
            C = atoi(f[1].c_str());
            for (int64_t l : csv(f[2])) labels.push_back((int32_t)l);
        } else {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        DataSetPlan p;
        const LabelVerdict v = plan_dataset(labels.data(), (int64_t)labels.size(), C, gc.empty() ? nullptr : gc.data(), target, &p);
        printf("{\"case\":\"%s\",\"verdict\":[%d,%lld,%d]", argv[a], (int)v.what, (long long)v.index, (int)v.label);
        if (v.what == LabelVerdict::OK) {
            printf(",\"plan\":{");
            ints("counts", p.counts); ints("gcounts", p.gcounts);
            printf("\"Nglobal\":%lld,", (long long)p.Nglobal);
            spans("tiles", p.tiles); spans("chunks", p.chunks);
            ints("cls_chunk_off", p.cls_chunk_off); ints("cls_off", p.cls_off);
            printf("\"parts\":["); parts(p.parts[0]); printf(","); parts(p.parts[1]); printf("],");
            printf("\"part_off\":["); list(p.part_off[0]); printf(","); list(p.part_off[1]); printf("],");
            printf("\"inv_count\":[");
            for (size_t i = 0; i < p.inv_count.size(); ++i) printf("%s%.17g", i ? "," : "", p.inv_count[i]);
            printf("]}");
        }
        printf("}%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
