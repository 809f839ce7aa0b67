// The host-side plan of a device-side encoding: which kind of basis a request names (EncodeBasis), every check that can reject it
// (encode_basis_validate) and the host images of the tables its kernel indexes (encode_tables).  These are the only guard between the
// caller's tables and a device read, so they are pure functions in plain C++17, no HIP: tests/test_encode_plan.py compiles this file
// alone under the host sanitizers; mpst_internal.h includes it for everything else.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/mpstime_hip.h"

namespace mpst {

constexpr int32_t SPLIT_MAX_BINS = 512, KDE_MAX_D = 16;
constexpr int32_t PROJ_MAX_D = 16, PROJ_MAX_LEGENDRE = 7 * PROJ_MAX_D, PROJ_MAX_FOURIER = 5 * PROJ_MAX_D;

inline bool basis_is_complex(int basis) { return basis == MPST_BASIS_FOURIER || basis == MPST_BASIS_STOUDENMIRE || basis == MPST_BASIS_SAHAND; }

// What a request encodes with: the entry point's kind and the one options struct that belongs to it (null: that entry point's error).
//   CLOSED  mpst_encode_opts   a closed-form basis, eo->basis
//   SPLIT   mpst_split_opts    bins over the auxiliary closed-form basis sp->aux_basis
//   KDE     mpst_kde_opts      a Sahand-Legendre basis: fitted tables, real states
//   PROJ    mpst_proj_opts     the listed members of a Legendre / Fourier family
struct EncodeBasis {
    enum Kind { CLOSED, SPLIT, KDE, PROJ } kind = CLOSED;
    const void* opts = nullptr;
    static EncodeBasis closed(const mpst_encode_opts* eo) { return {CLOSED, eo}; }
    static EncodeBasis split(const mpst_split_opts* sp) { return {SPLIT, sp}; }
    static EncodeBasis kde(const mpst_kde_opts* kd) { return {KDE, kd}; }
    static EncodeBasis proj(const mpst_proj_opts* pj) { return {PROJ, pj}; }
    const mpst_encode_opts* eo() const { return kind == CLOSED ? (const mpst_encode_opts*)opts : nullptr; }
    const mpst_split_opts* sp() const { return kind == SPLIT ? (const mpst_split_opts*)opts : nullptr; }
    const mpst_kde_opts* kd() const { return kind == KDE ? (const mpst_kde_opts*)opts : nullptr; }
    const mpst_proj_opts* pj() const { return kind == PROJ ? (const mpst_proj_opts*)opts : nullptr; }
    // the closed-form basis the kernel evaluates (KDE: none - a real one stands in wherever only real / complex matters).  Of a
    // validated request: opts is not null
    int family() const { return kind == SPLIT ? sp()->aux_basis : kind == PROJ ? pj()->basis : kind == KDE ? MPST_BASIS_LEGENDRE_NO_NORM : eo()->basis; }
    bool is_complex() const { return basis_is_complex(family()); }
    // the closed-form basis' own dimension within the d states of a site
    int32_t aux_dim(int32_t d) const { return kind == SPLIT ? sp()->aux_dim : d; }
};

struct EncodeReject {
    int code = 0;           // 0: accepted
    std::string text;
};
__attribute__((format(printf, 2, 3))) inline EncodeReject encode_reject(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return {code, buf};
}

inline bool kde_site_is_zero(const mpst_kde_opts* kd, int64_t site, int32_t d) {
    for (int64_t q = 0; q < (int64_t)d * d; ++q)
        if (kd->cvecs[site * d * d + q] != 0.0) return false;
    return true;
}

// a closed-form basis of dimension d: on its own (mpst_encode_dataset / _values) or as the auxiliary basis of a split one
inline EncodeReject closed_basis_validate(int basis, int d, bool split) {
    if (basis < MPST_BASIS_LEGENDRE || basis > MPST_BASIS_UNIFORM)
        return encode_reject(MPST_ERR_UNSUPPORTED, "%s", split ? "split bases are implemented over the closed-form bases (Legendre, Fourier, Stoudenmire, Sahand, Uniform)"
                                                             : "device-side encoding implements the closed-form bases (Legendre, Fourier, Stoudenmire, Sahand, Uniform)");
    const int odd = split ? MPST_ERR_UNSUPPORTED : MPST_ERR_INVALID;
    if (basis == MPST_BASIS_STOUDENMIRE && d != 2) return encode_reject(odd, "Stoudenmire Angle encoding only supports d = 2!");
    if (basis == MPST_BASIS_SAHAND && d % 2) return encode_reject(odd, "Sahand encoding only supports even dimension");
    return {};
}

inline EncodeReject split_validate(const mpst_split_opts* sp, int32_t T, int32_t d) {
    if (!sp || !sp->bins) return encode_reject(MPST_ERR_INVALID, "NULL split options or bin edges");
    if (sp->nbins < 1 || sp->nbins > SPLIT_MAX_BINS)
        return encode_reject(MPST_ERR_INVALID, "nbins must lie in 1 .. %d (got %d)", (int)SPLIT_MAX_BINS, (int)sp->nbins);
    if (sp->aux_dim < 1 || (int64_t)sp->nbins * sp->aux_dim != d)
        return encode_reject(MPST_ERR_INVALID, "The auxilliary basis dimension (%d) must evenly divide the total feature dimension (%d): d = nbins * aux_dim, nbins = %d",
                             (int)sp->aux_dim, (int)d, (int)sp->nbins);       // get_nbins_safely, splitbases.jl:2-9
    if (sp->per_site != 0 && sp->per_site != 1) return encode_reject(MPST_ERR_INVALID, "per_site must be 0 or 1");
    if (EncodeReject r = closed_basis_validate(sp->aux_basis, sp->aux_dim, true); r.code) return r;
    const int64_t nsite = sp->per_site ? T : 1, ne = sp->nbins + 1;
    for (int64_t t = 0; t < nsite; ++t)
        for (int64_t k = 0; k + 1 < ne; ++k)
            if (!(sp->bins[t * ne + k] <= sp->bins[t * ne + k + 1]))
                return encode_reject(MPST_ERR_INVALID, "bin edges must be non-decreasing (site %lld, edges %lld and %lld: %g, %g)", (long long)t, (long long)k,
                                     (long long)(k + 1), sp->bins[t * ne + k], sp->bins[t * ne + k + 1]);
    return {};
}

// the tables of a site whose coefficients are all zero are not read, by this check or by the kernel
inline EncodeReject kde_validate(const mpst_kde_opts* kd, int32_t T, int32_t d) {
    if (!kd || !kd->lo || !kd->step || !kd->coef || !kd->minx || !kd->scale || !kd->cvecs)
        return encode_reject(MPST_ERR_INVALID, "NULL density-estimate options or table");
    if (kd->npoints < 3) return encode_reject(MPST_ERR_INVALID, "a density estimate has at least 3 grid points (got %d)", (int)kd->npoints);
    if (kd->per_site != 0 && kd->per_site != 1) return encode_reject(MPST_ERR_INVALID, "per_site must be 0 or 1");
    if (d < 1 || d > KDE_MAX_D) return encode_reject(MPST_ERR_INVALID, "the Sahand-Legendre bases are encoded for d = 1 .. %d (got %d)", (int)KDE_MAX_D, (int)d);
    const int64_t nsite = kd->per_site ? T : 1;
    auto bad = [](double v) { return !(v > 0.0) || !std::isfinite(v); };
    for (int64_t t = 0; t < nsite; ++t) {
        if (kde_site_is_zero(kd, t, d)) continue;
        if (bad(kd->step[t]) || bad(kd->scale[t]) || bad(kd->minx[t]))
            return encode_reject(MPST_ERR_INVALID, "site %lld: step, scale and minx must be positive and finite (got %g, %g, %g)", (long long)t, kd->step[t],
                                 kd->scale[t], kd->minx[t]);
    }
    return {};
}

// every entry the kernel turns into a trip count or an index
inline EncodeReject proj_validate(const mpst_proj_opts* pj, int32_t T, int32_t d) {
    if (!pj || !pj->orders) return encode_reject(MPST_ERR_INVALID, "NULL projected-basis options or order table");
    const bool fourier = pj->basis == MPST_BASIS_FOURIER;
    if (!fourier && pj->basis != MPST_BASIS_LEGENDRE && pj->basis != MPST_BASIS_LEGENDRE_NO_NORM)
        return encode_reject(MPST_ERR_INVALID, "a projected basis is Legendre, Legendre without norm or Fourier (got basis %d)", (int)pj->basis);
    if (d < 1 || d > PROJ_MAX_D) return encode_reject(MPST_ERR_INVALID, "the projected bases are encoded for d = 1 .. %d (got %d)", (int)PROJ_MAX_D, (int)d);
    const int32_t cap = fourier ? PROJ_MAX_FOURIER : PROJ_MAX_LEGENDRE;
    if (pj->max_order < 0 || pj->max_order > cap)
        return encode_reject(MPST_ERR_INVALID, "max_order must be within 0 .. %d (got %d)", (int)cap, (int)pj->max_order);
    for (int64_t q = 0; q < (int64_t)T * d; ++q) {
        const int32_t o = pj->orders[q];
        if ((o < 0 && !fourier) || o > pj->max_order || o < -pj->max_order)
            return encode_reject(MPST_ERR_INVALID, "site %lld, slot %lld: order %d outside %s%d .. %d", (long long)(q / d), (long long)(q % d), (int)o,
                                 fourier ? "-" : "", fourier ? (int)pj->max_order : 0, (int)pj->max_order);
    }
    if (pj->basis == MPST_BASIS_LEGENDRE) {
        if (!pj->inv_norm) return encode_reject(MPST_ERR_INVALID, "NULL inv_norm for the normalised projected Legendre basis");
        for (int32_t t = 0; t < T; ++t)
            if (!(pj->inv_norm[t] > 0.0) || !std::isfinite(pj->inv_norm[t]))
                return encode_reject(MPST_ERR_INVALID, "site %d: inv_norm must be positive and finite (got %g)", (int)t, pj->inv_norm[t]);
    }
    return {};
}

// The checks of a request of T sites and d states per site (include/mpstime_hip.h), in the order the entry points report them.
inline EncodeReject encode_basis_validate(const EncodeBasis& b, int32_t T, int32_t d) {
    if (b.kind == EncodeBasis::CLOSED) return b.eo() ? closed_basis_validate(b.eo()->basis, d, false) : encode_reject(MPST_ERR_INVALID, "NULL encode options");
    if (T < 1) return encode_reject(MPST_ERR_INVALID, "bad dimensions");
    return b.kind == EncodeBasis::SPLIT ? split_validate(b.sp(), T, d) : b.kind == EncodeBasis::KDE ? kde_validate(b.kd(), T, d) : proj_validate(b.pj(), T, d);
}

// Where a table lies in EncodeTables::f64 / ::i32: `n` entries from `off`; off < 0: the request has no such table
struct EncodeSpan {
    int64_t off = -1, n = 0;
};
// The host images of everything the kernels index, one vector per element type: each is one upload.
struct EncodeTables {
    std::vector<double> f64;
    std::vector<int32_t> i32;
    // SPLIT: [T][nbins + 1] edges (bin_stride = nbins + 1) or [nbins + 1] shared by all sites (bin_stride = 0)
    EncodeSpan bins;
    int64_t bin_stride = 0;
    // KDE, S = T or 1 sites: lo | step | minx | scale [S] | coef [S][npoints + 2] | cvecs [S][d][d] (f64); zero [S] (i32): 1 where the
    // site's cvecs are all zero
    EncodeSpan kde_lo, kde_step, kde_minx, kde_scale, kde_coef, kde_cvecs, kde_zero;
    // PROJ: tab [T][2 d] (i32): per site the d orders in ascending order, then the slot of each; inv [T] (f64): MPST_BASIS_LEGENDRE only
    EncodeSpan proj_tab, proj_inv;
};

// The tables of a request that encode_basis_validate accepted.
inline EncodeTables encode_tables(const EncodeBasis& b, int32_t T, int32_t d) {
    EncodeTables o;
    auto put = [&o](const double* p, int64_t n) {
        const EncodeSpan s{(int64_t)o.f64.size(), n};
        o.f64.insert(o.f64.end(), p, p + n);
        return s;
    };
    if (const mpst_split_opts* sp = b.sp()) {
        o.bins = put(sp->bins, (int64_t)(sp->per_site ? T : 1) * (sp->nbins + 1));
        o.bin_stride = sp->per_site ? sp->nbins + 1 : 0;
    }
    if (const mpst_kde_opts* kd = b.kd()) {
        const int64_t ks = kd->per_site ? T : 1;
        o.i32.resize((size_t)ks);
        for (int64_t t = 0; t < ks; ++t) o.i32[(size_t)t] = kde_site_is_zero(kd, t, d);
        o.kde_zero = {0, ks};
        o.f64.reserve((size_t)(ks * (4 + kd->npoints + 2 + (int64_t)d * d)));
        o.kde_lo = put(kd->lo, ks), o.kde_step = put(kd->step, ks), o.kde_minx = put(kd->minx, ks), o.kde_scale = put(kd->scale, ks);
        o.kde_coef = put(kd->coef, ks * ((int64_t)kd->npoints + 2));
        o.kde_cvecs = put(kd->cvecs, ks * d * d);
    }
    if (const mpst_proj_opts* pj = b.pj()) {
        // the sort (stable, so equal orders keep their slots' order) turns the site's list into what k_encode_proj walks once
        o.i32.resize((size_t)T * 2 * d);
        for (int32_t t = 0; t < T; ++t) {
            int32_t* ord = o.i32.data() + (size_t)t * 2 * d;
            int32_t* slot = ord + d;
            const int32_t* src = pj->orders + (size_t)t * d;
            for (int32_t j = 0; j < d; ++j) slot[j] = j;
            std::stable_sort(slot, slot + d, [&](int32_t a, int32_t c) { return src[a] < src[c]; });
            for (int32_t j = 0; j < d; ++j) ord[j] = src[slot[j]];
        }
        o.proj_tab = {0, (int64_t)T * 2 * d};
        if (pj->basis == MPST_BASIS_LEGENDRE) o.proj_inv = put(pj->inv_norm, T);
    }
    return o;
}

}  // namespace mpst
