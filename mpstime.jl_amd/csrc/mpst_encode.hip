// mpst_encode.hip - device-side preprocessing + encoding: the closed-form bases, the split bases over them, the fitted
// Sahand-Legendre bases and the projected bases.
//
// Replaces, for the real bases the array sweep can train on, the host pipeline
//   transform_train_data / transform_test_data  (src/utils.jl:161-275)
//   legendre / legendre_no_norm                  (src/Encodings/bases.jl:70-108)
//   the per-value encode loop of encode_dataset  (src/Encodings/encodings.jl:120-150)
// so that a fit uploads the N x T raw matrix instead of the d times larger product states.  The order
// statistics of the RobustSigmoid fit (median and quartiles of the training set, utils.jl:171-176) come from a
// device radix sort of the N T values (hipCUB - a plain library sort, not a hot kernel) when asked for.
// Every formula keeps the reference's order of operations; FMA contraction is off in this file so the
// Bonnet recursion rounds like the host restatement (differences come from exp() only, ~1 ulp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "mpst_internal.h"

#pragma clang fp contract(off)

namespace mpst {

__device__ __forceinline__ double enc_stage1(const EncDev& e, double x) {
    if (e.sigmoid) x = 1.0 / (1.0 + exp(-(x - e.med) / e.s));
    return x;
}
// value after sigmoid, min-max and data_bounds (what the test path inspects per series)
__device__ __forceinline__ double enc_stage2(const EncDev& e, double x) {
    x = enc_stage1(e, x);
    if (e.minmax) {
        const double lo = e.lohi[0], hi = e.lohi[1];
        x = (x - lo) / (hi - lo);
        x = x * (e.ub - e.lb) + e.lb;
    }
    return x;
}

// min / max of the sigmoid-transformed training data: per-block partials, then one block
__global__ __launch_bounds__(256) void k_enc_range(EncDev e, const double* __restrict__ X, double* __restrict__ part) {
    __shared__ double smin[4], smax[4];
    const int64_t total = e.N * e.T;
    double mn = 1e300, mx = -1e300;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const double y = enc_stage1(e, X[i]);
        mn = fmin(mn, y);
        mx = fmax(mx, y);
    }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
        part[2 * blockIdx.x + 1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    }
}
__global__ __launch_bounds__(64) void k_enc_range_final(const double* __restrict__ part, int nblocks, double* __restrict__ lohi) {
    double mn = 1e300, mx = -1e300;
    for (int i = threadIdx.x; i < nblocks; i += 64) {
        mn = fmin(mn, part[2 * i]);
        mx = fmax(mx, part[2 * i + 1]);
    }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if (threadIdx.x == 0) {
        lohi[0] = mn;
        lohi[1] = mx;
    }
}

// test data: per-series out-of-bounds rescale (utils.jl:243-266): shift by the minimum if it is
// negative, then divide by the maximum if it exceeds 1.  One wave per series.
__global__ __launch_bounds__(256) void k_enc_series_fix(EncDev e, const double* __restrict__ X, double* __restrict__ fix) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= e.N) return;
    double mn = 1e300, mx = -1e300;
    for (int t = lane; t < e.T; t += 64) {
        const double u = enc_stage2(e, X[i * e.T + t]);
        mn = fmin(mn, u);
        mx = fmax(mx, u);
    }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    const double shift = mn < 0.0 ? mn : 0.0;
    const double hi = mx - shift;             // maximum after the shift (same subtraction the elements get)
    const double scale = hi > 1.0 ? hi : 1.0;
    if (lane == 0) {
        fix[2 * i] = shift;
        fix[2 * i + 1] = scale;
    }
}

// ---- the closed-form bases (src/Encodings/bases.jl), one helper each: k_encode writes the states as they are, k_encode_split
// (SCALE) writes w times the state - w is rect's 1 or 0.5, so the product is exact ----------------------------------------------
template <bool SCALE> __device__ __forceinline__ double enc_w(double v, double w) {
    if constexpr (SCALE) return v * w;
    else return v;
}
// angle_encode (bases.jl:7-21, periods = 1/4): cispi(3x/2) cospi(x/2), cispi(-3x/2) sinpi(x/2)
template <bool SCALE> __device__ __forceinline__ void enc_stoudenmire(double x, double w, double* outc) {
    double s3, c3, sh, ch;
    sincospi(1.5 * x, &s3, &c3);
    sincospi(0.5 * x, &sh, &ch);
    outc[0] = enc_w<SCALE>(c3 * ch, w);
    outc[1] = enc_w<SCALE>(s3 * ch, w);
    outc[2] = enc_w<SCALE>(c3 * sh, w);
    outc[3] = enc_w<SCALE>(-s3 * sh, w);
}
// sahand_encode (bases.jl:45-68): d/2 intervals of width 2/d, two states each, zero outside their interval
template <bool SCALE> __device__ __forceinline__ void enc_sahand(double x, int d, double w, double* outc) {
    const double dxs = 2.0 / d;
    for (int k = 0; k < d; ++k) {
        const int interval = k / 2 + 1;
        const double startx = (interval - 1) * dxs;
        const bool inside = startx <= x && x <= interval * dxs;
        double s3, c3, sh, ch;
        sincospi(1.5 * x / dxs, &s3, &c3);
        sincospi(0.5 * (x - startx) / dxs, &sh, &ch);
        const bool odd = (k & 1) == 0;
        outc[2 * k] = inside ? enc_w<SCALE>(odd ? c3 * ch : c3 * sh, w) : 0.0;
        outc[2 * k + 1] = inside ? enc_w<SCALE>(odd ? s3 * ch : -s3 * sh, w) : 0.0;
    }
}
// uniform_encode (bases.jl:2-4)
template <bool SCALE> __device__ __forceinline__ void enc_uniform(int d, double w, double* outu) {
    for (int k = 0; k < d; ++k) outu[k] = enc_w<SCALE>(1.0 / d, w);
}
// fourier_encode (bases.jl:23-42): cispi(f x) / sqrt(d) with f = 0, 1, -1, 2, -2, ...
template <bool SCALE> __device__ __forceinline__ void enc_fourier(double x, int d, double w, double* outc) {
    const double inv = 1.0 / sqrt((double)d);
    for (int k = 0; k < d; ++k) {
        const int f = (k + 1) / 2 * ((k & 1) ? 1 : -1);
        double sn, cs;
        sincospi((double)f * x, &sn, &cs);
        outc[2 * k] = enc_w<SCALE>(cs * inv, w);
        outc[2 * k + 1] = enc_w<SCALE>(sn * inv, w);
    }
}
// P_k(x) by Bonnet's recursion from p1 = P_{k-1}(x) and p0 = P_{k-2}(x), which move on by one order
__device__ __forceinline__ double bonnet_step(int k, double x, double& p0, double& p1) {
    if (k == 0) return 1.0;
    if (k == 1) return x;
    const int m = k - 1;
    const double p = ((2 * m + 1) * x * p1 - m * p0) / (m + 1);
    p0 = p1;
    p1 = p;
    return p;
}
// Bonnet recursion, then sqrt((2k+1)/2) (normalised Legendre), then the optional 1/nrm (bases.jl:77-92)
template <bool SCALE> __device__ __forceinline__ void enc_legendre(double x, int d, bool norm, double nrm, double w, double* out) {
    double p0 = 1.0, p1 = x;
    for (int k = 0; k < d; ++k) {
        double v = bonnet_step(k, x, p0, p1) * sqrt((2.0 * k + 1.0) / 2.0);
        if (norm) v = v / nrm;
        out[k] = enc_w<SCALE>(v, w);
    }
}
// d states of basis `basis` at x: d doubles (real bases) or d (re, im) pairs
template <bool SCALE> __device__ __forceinline__ void enc_basis(int basis, double x, int d, double nrm, double w, double* out) {
    if (basis == MPST_BASIS_STOUDENMIRE) enc_stoudenmire<SCALE>(x, w, out);
    else if (basis == MPST_BASIS_SAHAND) enc_sahand<SCALE>(x, d, w, out);
    else if (basis == MPST_BASIS_UNIFORM) enc_uniform<SCALE>(d, w, out);
    else if (basis == MPST_BASIS_FOURIER) enc_fourier<SCALE>(x, d, w, out);
    else enc_legendre<SCALE>(x, d, basis == MPST_BASIS_LEGENDRE, nrm, w, out);
}

// the value of (site t, series i) in the encoding's range: stage 2, the per-series out-of-bounds fix, the range map
__device__ __forceinline__ double enc_value(const EncDev& e, const double* __restrict__ X, int64_t t, int64_t i) {
    double x = enc_stage2(e, X[i * e.T + t]);
    if (e.fix) {
        const double shift = e.fix[2 * i], scale = e.fix[2 * i + 1];
        if (shift != 0.0) x -= shift;
        if (scale != 1.0) x /= scale;
    }
    return (e.b - e.a) * x + e.a;
}

// The front end of the four encoding kernels: one thread per (site t, series i), idx = t N + i; consecutive threads = consecutive
// series, so the values every thread writes are contiguous across the wave ([T][N][d] site-major, the sweep's layout).  x = enc_value
// of (t, i).  Not live: the thread has nothing to evaluate - it lies past the last value or, KIND = KDE, at a site whose coefficients
// are all zero: its d zeros are written here and none of the site's tables, its value included, is read
struct EncAt {
    int64_t idx, t, i;
    double x;
    bool live;
};
template <int KIND> __device__ __forceinline__ EncAt enc_at(const EncDev& e, const double* __restrict__ X, double* __restrict__ phi) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= e.N * e.T) return {idx, 0, 0, 0.0, false};
    const int64_t t = idx / e.N, i = idx - t * e.N;
    if constexpr (KIND == EncodeBasis::KDE) {
        if (e.kde_zero[e.kde_per_site ? t : 0]) {
            for (int n = 0; n < e.d; ++n) phi[idx * e.d + n] = 0.0;
            return {idx, t, i, 0.0, false};
        }
    }
    return {idx, t, i, enc_value(e, X, t, i), true};
}

__global__ __launch_bounds__(256) void k_encode(EncDev e, const double* __restrict__ X, double* __restrict__ phi) {
    const auto [idx, t, i, x, live] = enc_at<EncodeBasis::CLOSED>(e, X, phi);
    if (!live) return;
    enc_basis<false>(e.basis, x, e.d, e.nrm, 1.0, phi + idx * e.d * (e.fourier ? 2 : 1));
}

// Split bases (src/Encodings/splitbases.jl): the same thread mapping and front end; the thread walks its site's edge list
// (e.bins + t * e.bin_stride, nbins + 1 edges; consecutive threads share it - it stays in the cache) and restates
// project_onto_bins (:113-132) bin by bin: rect (:96-108) of x_prop / scale - 0.5 selects the bin - or, exactly on an interior
// edge, both neighbours at 0.5 -, the auxiliary basis is evaluated at a + x_prop in selected bins only, the others are zeroed.
// An empty bin (dx = 0) gives x_prop = +-inf or NaN, which every comparison rejects, as on the host.
__global__ __launch_bounds__(256) void k_encode_split(EncDev e, const double* __restrict__ X, double* __restrict__ phi) {
    const auto [idx, t, i, x, live] = enc_at<EncodeBasis::SPLIT>(e, X, phi);
    if (!live) return;
    const double* __restrict__ bins = e.bins + t * e.bin_stride;
    const int nb = e.nbins, w = e.aux_dim * (e.fourier ? 2 : 1);       // doubles per bin
    double* out = phi + idx * nb * w;
    const double a = bins[0], scale = bins[nb] - a;
    for (int k = 0; k < nb; ++k) {
        const double dx = bins[k + 1] - bins[k];
        const double x_prop = scale * (x - bins[k]) / dx;
        const double r = x_prop / scale - 0.5;
        const double lbound = k == 0 ? 1.0 : 0.5, rbound = k == nb - 1 ? 1.0 : 0.5;
        const double select = r == -0.5 ? lbound : (r == 0.5 ? rbound : ((-0.5 <= r && r <= 0.5) ? 1.0 : 0.0));
        double* o = out + k * w;
        if (select == 0.0) {
            for (int q = 0; q < w; ++q) o[q] = 0.0;
        } else {
            enc_basis<true>(e.basis, a + x_prop, e.aux_dim, e.nrm, select, o);
        }
    }
}

// Sahand-Legendre bases (bases.jl:111-129): the same thread mapping and front end.  The thread reads its site's density estimate -
// three neighbouring coefficients of the quadratic B-spline through the K grid values (consecutive threads share the site: the table
// stays in the cache) -, takes f0 = max(sqrt(max(pdf, 0)), minx) and writes f0 / scale * sum_i cvecs[n][i] x^i for the d functions.
// The spline index is clamped to 1 .. K, so the three reads stay inside the K + 2 coefficients whatever x is.  A site whose
// coefficients are all zero (nothing to fit there) writes zeros and reads none of its tables.
__global__ __launch_bounds__(256) void k_encode_kde(EncDev e, const double* __restrict__ X, double* __restrict__ phi) {
    const auto [idx, t, i, x, live] = enc_at<EncodeBasis::KDE>(e, X, phi);
    if (!live) return;
    const int64_t s = e.kde_per_site ? t : 0;
    const int d = e.d;
    double* out = phi + idx * d;
    const int K = e.kde_npoints;
    const double lo = e.kde_lo[s], step = e.kde_step[s];
    double p = 0.0;
    if (!(x < lo || x > lo + (K - 1) * step)) {
        const double u = (x - lo) / step + 1.0;
        const double r = fmin(fmax(rint(u), 1.0), (double)K);          // round half to even, as the host's rint
        const double f = u - r;
        const double* __restrict__ c = e.kde_coef + s * (K + 2) + (int64_t)r;
        p = c[-1] * (0.5 * ((f - 0.5) * (f - 0.5))) + c[0] * (0.75 - f * f) + c[1] * (0.5 * ((f + 0.5) * (f + 0.5)));
    }
    const double f0 = fmax(sqrt(fmax(p, 0.0)), e.kde_minx[s]);
    const double scale = e.kde_scale[s];
    const double* __restrict__ cv = e.kde_cvecs + s * d * d;
    for (int n = 0; n < d; ++n) {
        double acc = 0.0, xp = 1.0;
        for (int q = 0; q < d; ++q) {
            acc += cv[n * d + q] * xp;
            xp *= x;
        }
        out[n] = acc * f0 / scale;
    }
}

// Projected bases (bases.jl:94-107; DESIGN.md, "Projected bases"): the same thread mapping and front end.  Site t evaluates its own
// d members of the Legendre / Fourier family.  Its table (e.proj_tab + 2 d t; consecutive threads share the site, so it comes from
// the cache) holds the d orders in ascending order and, behind them, the slot each one is written to - the host sorted the site's
// list, so an unsorted list or a repeated order costs nothing here and every slot is written exactly once.
// Legendre: the Bonnet recursion of enc_legendre runs up to the site's largest order and stops at every listed one.
// Fourier: sincospi(f x) / sqrt(d) as enc_fourier, f signed.
// Bounds: q runs over 0 .. d-1, so the reads stay inside the site's 2 d entries; the slots are a permutation of 0 .. d-1 and the
// orders are within 0 .. 7 * 16 (the host built and checked both); x enters no index, so a NaN value only gives NaN states.
__global__ __launch_bounds__(256) void k_encode_proj(EncDev e, const double* __restrict__ X, double* __restrict__ phi) {
    const auto [idx, t, i, x, live] = enc_at<EncodeBasis::PROJ>(e, X, phi);
    if (!live) return;
    const int d = e.d;
    const int32_t* __restrict__ ord = e.proj_tab + t * 2 * d;
    const int32_t* __restrict__ slot = ord + d;
    if (e.fourier) {
        double* out = phi + idx * d * 2;
        const double inv = 1.0 / sqrt((double)d);
        for (int q = 0; q < d; ++q) {
            double sn, cs;
            sincospi((double)ord[q] * x, &sn, &cs);
            out[2 * slot[q]] = cs * inv;
            out[2 * slot[q] + 1] = sn * inv;
        }
        return;
    }
    double* out = phi + idx * d;
    const double inv = e.proj_inv ? e.proj_inv[t] : 1.0;
    const int last = ord[d - 1];
    double p0 = 1.0, p1 = x;
    int q = 0;
    for (int k = 0; k <= last; ++k) {
        const double pk = bonnet_step(k, x, p0, p1);
        if (ord[q] != k) continue;
        double v = pk * sqrt((2.0 * k + 1.0) / 2.0);
        if (e.proj_inv) v = v * inv;
        for (; q < d && ord[q] == k; ++q) out[slot[q]] = v;
        if (q == d) break;
    }
}

// ---- RobustSigmoid fit: median and inter-quartile range of all training values ---------------------------------
// type-7 quantiles (Julia's / NumPy's default) of the sorted values; the interpolation is written as NumPy's _lerp so that
// the host restatement and this kernel agree to the bit (Julia's a + g (b - a) differs from it by at most one ulp)
__global__ void k_enc_quantiles(const double* __restrict__ xs, int64_t n, double* __restrict__ out /* median, q25, q75 */) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    auto lerp = [](double a, double b, double t) {
        const double dba = b - a;
        return t >= 0.5 ? b - dba * (1.0 - t) : a + dba * t;
    };
    auto quant = [&](double q) {
        const double pos = q * (double)(n - 1);
        const int64_t lo = (int64_t)floor(pos);
        const int64_t hi = lo + 1 < n ? lo + 1 : n - 1;
        return lerp(xs[lo], xs[hi], pos - (double)lo);
    };
    out[0] = (n & 1) ? xs[n / 2] : 0.5 * (xs[n / 2 - 1] + xs[n / 2]);       // np.median / Statistics.median: mean of the middle pair
    out[1] = quant(0.25);
    out[2] = quant(0.75);
}
size_t order_stats_temp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, (const double*)nullptr, (double*)nullptr, (int)n);
    return bytes;
}
hipError_t launch_order_stats(const double* X, double* sorted, void* temp, size_t temp_bytes, int64_t n, double* out3, hipStream_t s) {
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, X, sorted, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_enc_quantiles, dim3(1), dim3(1), 0, s, (const double*)sorted, n, out3);
    return hipGetLastError();
}

void launch_encode(const EncDev& e, const double* X, double* phi, double* part, double* lohi, double* fix, int fit_range,
                   hipStream_t s) {
    if (fit_range) {
        const int nb = 256;
        hipLaunchKernelGGL(k_enc_range, dim3(nb), dim3(256), 0, s, e, X, part);
        hipLaunchKernelGGL(k_enc_range_final, dim3(1), dim3(64), 0, s, (const double*)part, nb, lohi);
    }
    if (fix) hipLaunchKernelGGL(k_enc_series_fix, dim3((unsigned)((e.N + 3) / 4)), dim3(256), 0, s, e, X, fix);
    const dim3 grid((unsigned)((e.N * e.T + 255) / 256));
    switch (e.kind) {
        case EncodeBasis::PROJ: hipLaunchKernelGGL(k_encode_proj, grid, dim3(256), 0, s, e, X, phi); break;
        case EncodeBasis::KDE: hipLaunchKernelGGL(k_encode_kde, grid, dim3(256), 0, s, e, X, phi); break;
        case EncodeBasis::SPLIT: hipLaunchKernelGGL(k_encode_split, grid, dim3(256), 0, s, e, X, phi); break;
        default: hipLaunchKernelGGL(k_encode, grid, dim3(256), 0, s, e, X, phi);
    }
}

}  // namespace mpst
