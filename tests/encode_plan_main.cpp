// Prints the verdict of encode_basis_validate and, where it accepts, the tables of encode_tables (csrc/mpst_encode_plan.h) for every case
// on the command line as one JSON document.  tests/test_encode_plan.py compiles this file alone, with the host compiler and its
// sanitizers.  A case is colon separated; every table is a comma separated list given as name=list and becomes a heap array of exactly
// that many entries, a name that is left out a NULL pointer, a trailing "null" field a NULL options struct:
//     closed:<basis>:<d>
//     split:<T>:<d>:<aux_basis>:<aux_dim>:<nbins>:<per_site>[:bins=..]
//     kde:<T>:<d>:<npoints>:<per_site>[:lo=..][:step=..][:coef=..][:minx=..][:scale=..][:cvecs=..]
//     proj:<T>:<d>:<basis>:<max_order>[:orders=..][:inv=..]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "mpst_encode_plan.h"

using namespace mpst;

static std::vector<std::string> split_at(const std::string& s, char sep) {
    std::vector<std::string> f;
    for (size_t i = 0; i <= s.size();) {
        size_t j = s.find(sep, i);
        if (j == std::string::npos) j = s.size();
        f.push_back(s.substr(i, j - i));
        i = j + 1;
    }
    return f;
}

// the tables of one case, each in an allocation of its exact length
struct Tables {
    std::map<std::string, std::unique_ptr<double[]>> f64;
    std::unique_ptr<int32_t[]> orders;
    Tables(const std::vector<std::string>& f, size_t first) {
        for (size_t k = first; k < f.size(); ++k) {
            const size_t eq = f[k].find('=');
            if (eq == std::string::npos) continue;
            const std::string name = f[k].substr(0, eq), list = f[k].substr(eq + 1);
            const std::vector<std::string> v = list.empty() ? std::vector<std::string>() : split_at(list, ',');
            if (name == "orders") {
                orders.reset(new int32_t[v.size()]);
                for (size_t i = 0; i < v.size(); ++i) orders[i] = (int32_t)atol(v[i].c_str());
            } else {
                f64[name].reset(new double[v.size()]);
                for (size_t i = 0; i < v.size(); ++i) f64[name][i] = strtod(v[i].c_str(), nullptr);
            }
        }
    }
    const double* get(const char* name) const {
        auto it = f64.find(name);
        return it == f64.end() ? nullptr : it->second.get();
    }
};

static void number(double v) {
    if (std::isnan(v)) printf("NaN");
    else if (std::isinf(v)) printf(v > 0 ? "Infinity" : "-Infinity");
    else printf("%.17g", v);
}

static void span(const char* name, const EncodeSpan& s) { printf("\"%s\":[%lld,%lld],", name, (long long)s.off, (long long)s.n); }

static std::string escaped(const std::string& s) {
    std::string o;
    for (char ch : s) {
        if (ch == '"' || ch == '\\') o += '\\';
        o += ch;
    }
    return o;
}

int main(int argc, char** argv) {
    printf("{\"cases\":[\n");
    for (int a = 1; a < argc; ++a) {
        const std::vector<std::string> f = split_at(argv[a], ':');
        const bool null_struct = f.back() == "null";
        auto num = [&](size_t k) { return k < f.size() ? atoi(f[k].c_str()) : 0; };
        if (f.size() < 3) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        const int32_t T = f[0] == "closed" ? 1 : num(1), d = num(2);
        const Tables tab(f, 3);
        mpst_encode_opts eo{};
        mpst_split_opts sp{};
        mpst_kde_opts kd{};
        mpst_proj_opts pj{};
        EncodeBasis b;
        if (f[0] == "closed") {
            eo.basis = num(1);
            b = EncodeBasis::closed(&eo);
        } else if (f[0] == "split") {
            sp.aux_basis = num(3), sp.aux_dim = num(4), sp.nbins = num(5), sp.per_site = num(6), sp.bins = tab.get("bins");
            b = EncodeBasis::split(null_struct ? nullptr : &sp);
        } else if (f[0] == "kde") {
            kd.npoints = num(3), kd.per_site = num(4);
            kd.lo = tab.get("lo"), kd.step = tab.get("step"), kd.coef = tab.get("coef"), kd.minx = tab.get("minx"), kd.scale = tab.get("scale"),
            kd.cvecs = tab.get("cvecs");
            b = EncodeBasis::kde(null_struct ? nullptr : &kd);
        } else if (f[0] == "proj") {
            pj.basis = num(3), pj.max_order = num(4), pj.orders = tab.orders.get(), pj.inv_norm = tab.get("inv");
            b = EncodeBasis::proj(null_struct ? nullptr : &pj);
        } else {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        const EncodeReject r = encode_basis_validate(b, T, d);
        printf("{\"case\":\"%s\",\"code\":%d,\"text\":\"%s\"", argv[a], r.code, escaped(r.text).c_str());
        if (r.code == 0) {
            const EncodeTables t = encode_tables(b, T, d);
            printf(",\"family\":%d,\"is_complex\":%d,\"aux_dim\":%d,\"bin_stride\":%lld,\"spans\":{", b.family(), (int)b.is_complex(), (int)b.aux_dim(d),
                   (long long)t.bin_stride);
            span("bins", t.bins), span("kde_lo", t.kde_lo), span("kde_step", t.kde_step), span("kde_minx", t.kde_minx), span("kde_scale", t.kde_scale);
            span("kde_coef", t.kde_coef), span("kde_cvecs", t.kde_cvecs), span("kde_zero", t.kde_zero), span("proj_tab", t.proj_tab);
            printf("\"proj_inv\":[%lld,%lld]},\"f64\":[", (long long)t.proj_inv.off, (long long)t.proj_inv.n);
            for (size_t i = 0; i < t.f64.size(); ++i) {
                if (i) printf(",");
                number(t.f64[i]);
            }
            printf("],\"i32\":[");
            for (size_t i = 0; i < t.i32.size(); ++i) printf("%s%d", i ? "," : "", (int)t.i32[i]);
            printf("]");
        }
        printf("}%s\n", a + 1 < argc ? "," : "");
    }
    printf("]}\n");
    return 0;
}
