// Model overlaps: the inner products G_ab[c, c'] = <psi_{a,c} | psi_{b,c'}> of the class states of K models, no
// counterpart in the reference beyond the class overlap matrix of get_training_summary (src/summary.jl:247-251).
//
// One workgroup per pair (a, b), the pairs most expensive first.  With the label at site p, the left environment walks sites 0..p-1,
//     X = L M_B           [chi_a_l x chi_b_l] [chi_b_l x d chi_b_r]
//     L' = A_mat^H X_mat  [chi_a_r x chi_a_l d] [chi_a_l d x chi_b_r]      (the reshape between the two is free),
// and the right environment walks sites T-1..p+1 with the same two products: the host stores those tensors mirrored, (r, s, l), so
// one step serves both ends.  At the label site, per class c' of b, Y = B_p^{c'} R^T and Z = L Y on the same pipe; the accumulators of Z
// meet conj(A_p^c) of every class c of a as they lie, so Z is never stored.  Every product runs on v_mfma_f64_16x16x4_f64; bonds are
// padded to 16 with zeros on the host, so no tile and no k-step is predicated.  Complex models keep a real and an imaginary plane of
// every operand and take four real MFMAs per k-step.
// After every site the environment is divided by the power of two of its largest magnitude (ldexp: nothing is rounded) and the integer
// exponent is summed per pair, so ln|G| = ln|g| + exponent ln 2 holds at any chain length.  An environment that is exactly zero ends the
// pair with a status word (no trap, no assert).  Sums have one fixed order per shape: no atomics, and a pair's bits depend neither on
// which pairs travel along nor on where it runs.  The state (three environments and X) lives in LDS up to 156 KB, in per-workgroup global
// scratch beyond (mpst_overlap_plan.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "mpst_internal.h"
#include "mpst_overlap_plan.h"

namespace mpst {
namespace {

constexpr int OV_THREADS = 256, OV_WAVES = OV_THREADS / 64;
constexpr int64_t OV_ZERO = std::numeric_limits<int64_t>::min();       // exponent of a pair whose environment vanished

struct OvArgs {
    const double* W;            // the models: site j of model k at W + off[k T + j]
    const int64_t* off;         // [K][T]
    const int32_t* chi;         // [K][T + 1]
    const int32_t* ncls;        // [K]
    const int32_t* pairs;       // [count][2] of this launch
    double* g;                  // [count][Cmax][Cmax] (pairs: complex), zero on entry
    int64_t* ex;                // [count]
    double* gws;                // scratch, state doubles per workgroup, or null: LDS
    int64_t env, xsz;           // doubles of one plane of an environment and of X
    int T, d, p, Cmax, ldE;
};

struct P2 { double re, im; };

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// C (M x N) = op(A) (M x K) B (K x N) by the workgroup, M, N and K multiples of 16: a wave owns (16 rows, NB tiles of 16 columns) at
// a time, fa(row, k) / fb(k, col) fetch an element, fs(row, col, re, im) takes a result.  kConjA: op(A) = conj(A) (fa transposes itself).
template <bool CX, bool kConjA, int NB, class FA, class FB, class FS>
__device__ __forceinline__ void ov_gemm_nb(int mt, int ng, int K, FA fa, FB fb, FS fs) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i16 = lane & 15, kq = lane >> 4;
    for (int item = wv; item < mt * ng; item += OV_WAVES) {
        const int m0 = (item / ng) * 16, n0 = (item % ng) * (16 * NB);
        d4 cr[NB], ci[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) cr[u] = ci[u] = d4{0.0, 0.0, 0.0, 0.0};
        // K is a multiple of 16 (every bond is padded to 16): the operands of four k-steps are fetched before their MFMAs are issued
        for (int k0 = 0; k0 < K; k0 += 16) {
            P2 a[4], b[4][NB];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = fa(m0 + i16, k0 + 4 * q + kq);
#pragma unroll
                for (int u = 0; u < NB; ++u) b[q][u] = fb(k0 + 4 * q + kq, n0 + 16 * u + i16);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    cr[u] = mfma_f64(a[q].re, b[q][u].re, cr[u]);
                    if (CX) {
                        cr[u] = mfma_f64(kConjA ? a[q].im : -a[q].im, b[q][u].im, cr[u]);
                        ci[u] = mfma_f64(a[q].re, b[q][u].im, ci[u]);
                        ci[u] = mfma_f64(kConjA ? -a[q].im : a[q].im, b[q][u].re, ci[u]);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) fs(m0 + kq + 4 * r, n0 + 16 * u + i16, cr[u][r], CX ? ci[u][r] : 0.0);
    }
}

// the widest column blocking that divides the tiles and still gives every wave an item (a function of the shape alone); complex
// operands stop at two tiles, which are four accumulators: four would spill
template <bool CX, bool kConjA, class FA, class FB, class FS>
__device__ __forceinline__ void ov_gemm(int M, int N, int K, FA fa, FB fb, FS fs) {
    const int mt = M / 16, nt = N / 16;
    if (!CX && nt % 4 == 0 && mt * (nt / 4) >= OV_WAVES) ov_gemm_nb<CX, kConjA, 4>(mt, nt / 4, K, fa, fb, fs);
    else if (nt % 2 == 0 && mt * (nt / 2) >= OV_WAVES) ov_gemm_nb<CX, kConjA, 2>(mt, nt / 2, K, fa, fb, fs);
    else ov_gemm_nb<CX, kConjA, 1>(mt, nt, K, fa, fb, fs);
}

// E = [1], padded to one tile
template <bool CX>
__device__ void ov_unit(double* E, int64_t env, int ldE) {
    for (int e = threadIdx.x; e < 16 * 16; e += OV_THREADS) {
        const int i = (e / 16) * ldE + e % 16;
        E[i] = e == 0 ? 1.0 : 0.0;
        if (CX) E[env + i] = 0.0;
    }
    __syncthreads();
}

// One site of a walk: En = A^H (E B) over the bonds (ai x bi) -> (ao x bo), all padded; At / Bt: the site tensors, element (in, s, out) at
// (in d + s) out_dim + out.  En is divided by 2^e, e the exponent of its largest magnitude, and e is added to *ex; false when En is zero.
template <bool CX>
__device__ bool ov_step(const double* At, const double* Bt, int ai, int ao, int bi, int bo, int d, const double* E, double* X, double* En,
                        const OvArgs& g, double* red, int64_t* ex) {
    const int ldE = g.ldE, nx = d * bo;
    const int64_t env = g.env, xsz = g.xsz, sza = (int64_t)ai * d * ao, szb = (int64_t)bi * d * bo;
    ov_gemm<CX, false>(
        ai, nx, bi, [&](int row, int k) { return P2{E[row * ldE + k], CX ? E[env + row * ldE + k] : 0.0}; },
        [&](int k, int col) { return P2{Bt[(int64_t)k * nx + col], CX ? Bt[szb + (int64_t)k * nx + col] : 0.0}; },
        [&](int row, int col, double re, double im) {
            X[(int64_t)row * nx + col] = re;
            if (CX) X[xsz + (int64_t)row * nx + col] = im;
        });
    __syncthreads();
    double mx = 0.0;
    ov_gemm<CX, true>(
        ao, bo, ai * d, [&](int row, int k) { return P2{At[(int64_t)k * ao + row], CX ? At[sza + (int64_t)k * ao + row] : 0.0}; },
        [&](int k, int col) { return P2{X[(int64_t)k * bo + col], CX ? X[xsz + (int64_t)k * bo + col] : 0.0}; },
        [&](int row, int col, double re, double im) {
            En[row * ldE + col] = re;
            mx = fmax(mx, fabs(re));
            if (CX) {
                En[env + row * ldE + col] = im;
                mx = fmax(mx, fabs(im));
            }
        });
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = 0.0;
    for (int w = 0; w < OV_WAVES; ++w) mx = fmax(mx, red[w]);
    if (!(mx > 0.0)) return false;
    const int e = ilogb(mx);
    for (int q = threadIdx.x; q < ao * bo; q += OV_THREADS) {
        const int i = (q / bo) * ldE + q % bo;
        En[i] = ldexp(En[i], -e);
        if (CX) En[env + i] = ldexp(En[env + i], -e);
    }
    *ex += e;
    __syncthreads();
    return true;
}

template <bool CX, bool kLds>
__global__ __launch_bounds__(OV_THREADS, 2) void k_overlap(OvArgs g) {
    extern __shared__ double smem[];
    __shared__ double red[OV_WAVES];
    __shared__ double part[OV_WAVES][32];
    constexpr int PL = CX ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = g.T, d = g.d, p = g.p, ldE = g.ldE;
    const int64_t env = g.env, xsz = g.xsz;
    double* base = kLds ? smem : g.gws + (int64_t)blockIdx.x * PL * (3 * env + xsz);
    double* Eb[3] = {base, base + PL * env, base + 2 * PL * env};
    double* X = base + 3 * PL * env;
    const int a = g.pairs[2 * blockIdx.x], b = g.pairs[2 * blockIdx.x + 1];
    const int32_t *cha = g.chi + (int64_t)a * (T + 1), *chb = g.chi + (int64_t)b * (T + 1);
    const int64_t *offa = g.off + (int64_t)a * T, *offb = g.off + (int64_t)b * T;
    auto pad = [](int c) { return (c + 15) & ~15; };
    int64_t ex = 0;
    bool live = true;
    // the left environment: sites 0 .. p-1
    int cur = 0;
    ov_unit<CX>(Eb[0], env, ldE);
    for (int j = 0; j < p && live; ++j) {
        live = ov_step<CX>(g.W + offa[j], g.W + offb[j], pad(cha[j]), pad(cha[j + 1]), pad(chb[j]), pad(chb[j + 1]), d, Eb[cur], X, Eb[cur ^ 1], g, red, &ex);
        cur ^= 1;
    }
    const double* L = Eb[cur];
    // the right environment: sites T-1 .. p+1, stored mirrored
    double* Rb[2] = {Eb[cur ^ 1], Eb[2]};
    int rc = 0;
    if (live) ov_unit<CX>(Rb[0], env, ldE);
    for (int j = T - 1; j > p && live; --j) {
        live = ov_step<CX>(g.W + offa[j], g.W + offb[j], pad(cha[j + 1]), pad(cha[j]), pad(chb[j + 1]), pad(chb[j]), d, Rb[rc], X, Rb[rc ^ 1], g, red, &ex);
        rc ^= 1;
    }
    if (!live) {
        if (tid == 0) g.ex[blockIdx.x] = OV_ZERO;
        return;
    }
    const double* R = Rb[rc];
    // the label site: G[c][c'] = <A_p^c, L (B_p^c' R^T)>
    const int al = pad(cha[p]), ar = pad(cha[p + 1]), bl = pad(chb[p]), br = pad(chb[p + 1]), Ca = g.ncls[a], Cb = g.ncls[b], nz = d * ar;
    const int64_t sza = (int64_t)al * d * ar, szb = (int64_t)bl * d * br;
    const double* Ap = g.W + offa[p];
    double* gout = g.g + (int64_t)blockIdx.x * g.Cmax * g.Cmax * PL;
    for (int cp = 0; cp < Cb; ++cp) {
        const double* Bt = g.W + offb[p] + (int64_t)cp * PL * szb;
        ov_gemm<CX, false>(
            bl * d, ar, br, [&](int row, int k) { return P2{Bt[(int64_t)row * br + k], CX ? Bt[szb + (int64_t)row * br + k] : 0.0}; },
            [&](int k, int col) { return P2{R[col * ldE + k], CX ? R[env + col * ldE + k] : 0.0}; },
            [&](int row, int col, double re, double im) {
                X[(int64_t)row * ar + col] = re;
                if (CX) X[xsz + (int64_t)row * ar + col] = im;
            });
        __syncthreads();
        // the classes of a four at a time (Z is formed again for every four: one site of the chain, and C <= 4 forms it once)
        for (int c0 = 0; c0 < Ca; c0 += 4) {
            double gr[4] = {0.0, 0.0, 0.0, 0.0}, gi[4] = {0.0, 0.0, 0.0, 0.0};
            ov_gemm<CX, false>(
                al, nz, bl, [&](int row, int k) { return P2{L[row * ldE + k], CX ? L[env + row * ldE + k] : 0.0}; },
                [&](int k, int col) { return P2{X[(int64_t)k * nz + col], CX ? X[xsz + (int64_t)k * nz + col] : 0.0}; },
                [&](int row, int col, double re, double im) {
                    const double* ap = Ap + (int64_t)c0 * PL * sza + (int64_t)row * nz + col;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c0 + c < Ca) {
                            const double xr = ap[(int64_t)c * PL * sza];
                            gr[c] = fma(xr, re, gr[c]);
                            if (CX) {
                                const double xi = ap[(int64_t)c * PL * sza + sza];
                                gr[c] = fma(xi, im, gr[c]);
                                gi[c] = fma(xr, im, gi[c]);
                                gi[c] = fma(-xi, re, gi[c]);
                            }
                        }
                });
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double vr = wave_sum(gr[c]), vi = CX ? wave_sum(gi[c]) : 0.0;
                if (lane == 0) {
                    part[wv][2 * (c0 + c)] = vr;
                    part[wv][2 * (c0 + c) + 1] = vi;
                }
            }
        }
        __syncthreads();
        if (tid < Ca * PL) {
            const int c = tid / PL, z = tid % PL;
            double v = 0.0;
            for (int w = 0; w < OV_WAVES; ++w) v += part[w][2 * c + z];
            gout[((int64_t)c * g.Cmax + cp) * PL + z] = v;
        }
        __syncthreads();
    }
    if (tid == 0) g.ex[blockIdx.x] = ex;
}

hipError_t launch_overlap(bool cx, bool lds, const OvArgs& g, int count, size_t lds_bytes, hipStream_t s) {
    if (lds) {
        const void* f = cx ? (const void*)k_overlap<true, true> : (const void*)k_overlap<false, true>;
        if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OVERLAP_LDS_BYTES); e != hipSuccess) return e;
    }
    if (cx) {
        if (lds) hipLaunchKernelGGL((k_overlap<true, true>), dim3(count), dim3(OV_THREADS), lds_bytes, s, g);
        else hipLaunchKernelGGL((k_overlap<true, false>), dim3(count), dim3(OV_THREADS), 0, s, g);
    } else {
        if (lds) hipLaunchKernelGGL((k_overlap<false, true>), dim3(count), dim3(OV_THREADS), lds_bytes, s, g);
        else hipLaunchKernelGGL((k_overlap<false, false>), dim3(count), dim3(OV_THREADS), 0, s, g);
    }
    return hipGetLastError();
}

#define OV_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

}  // namespace

// validated by the caller (mpst_api.hip): the models agree in T, d, label site and element type, every pair index lies in [0, K)
hipError_t model_overlaps(const OverlapHost& h, size_t free_b, const char* chunk_gb, hipStream_t s, double* g_out, double* lg_out, double* seconds) {
    const int K = h.K, T = h.T, d = h.d, p = h.label_site, PL = h.cx ? 2 : 1;
    const int64_t P = (int64_t)h.pairs.size() / 2;
    int cap = 1, cmax = 1;
    for (int k = 0; k < K; ++k) {
        cmax = std::max(cmax, (int)h.ncls[k]);
        for (int j = 0; j <= T; ++j) cap = std::max(cap, (int)h.chi[k][j]);
    }
    std::fill(g_out, g_out + P * cmax * cmax * PL, 0.0);
    if (P == 0) {
        if (seconds) *seconds = 0.0;
        return hipSuccess;
    }
    // the models in the device layout: (in, s, out) with the bonds padded to 16, `in` the left bond up to the label site and the right
    // bond beyond it; the classes of the label site one after the other; the imaginary plane behind the real one
    std::vector<int64_t> off((size_t)K * T);
    std::vector<int32_t> chi((size_t)K * (T + 1));
    int64_t total = 0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < T; ++j) {
            off[(size_t)k * T + j] = total;
            total += (int64_t)PL * overlap_pad(h.chi[k][j]) * d * overlap_pad(h.chi[k][j + 1]) * (j == p ? h.ncls[k] : 1);
        }
    std::vector<double> hw((size_t)total, 0.0);
    for (int k = 0; k < K; ++k) {
        std::memcpy(&chi[(size_t)k * (T + 1)], h.chi[k], (size_t)(T + 1) * sizeof(int32_t));
        for (int j = 0; j < T; ++j) {
            const int Dl = h.chi[k][j], Dr = h.chi[k][j + 1], lp = overlap_pad(Dl), rp = overlap_pad(Dr);
            const int64_t sz = (int64_t)lp * d * rp;
            const double* src = (const double*)h.site[k][j];
            for (int c = 0; c < (j == p ? h.ncls[k] : 1); ++c) {
                double* dst = &hw[(size_t)(off[(size_t)k * T + j] + (int64_t)c * PL * sz)];
                for (int r = 0; r < Dr; ++r)
                    for (int l = 0; l < Dl; ++l)
                        for (int q = 0; q < d; ++q) {
                            const size_t e = q + (size_t)d * (l + (size_t)Dl * (r + (size_t)Dr * c));
                            const int64_t o = j <= p ? ((int64_t)l * d + q) * rp + r : ((int64_t)r * d + q) * lp + l;
                            dst[o] = src[e * PL];
                            if (h.cx) dst[sz + o] = src[e * PL + 1];
                        }
            }
        }
    }
    // the pairs, most expensive first, cut into blocks under the query budget
    std::vector<double> cost((size_t)P);
    for (int64_t q = 0; q < P; ++q) cost[q] = overlap_pair_cost(h.chi[h.pairs[2 * q]], h.chi[h.pairs[2 * q + 1]], T, d, p, h.ncls[h.pairs[2 * q + 1]]);
    const std::vector<int32_t> order = overlap_pair_order(cost);
    std::vector<int32_t> hp((size_t)2 * P);
    for (int64_t q = 0; q < P; ++q) {
        hp[2 * q] = h.pairs[2 * order[q]];
        hp[2 * q + 1] = h.pairs[2 * order[q] + 1];
    }
    const bool lds = overlap_state_in_lds(d, cap, PL);
    const int64_t state = overlap_state_bytes(d, cap, PL) / 8, gsz = (int64_t)cmax * cmax * PL;
    const int64_t block = overlap_block_pairs(P, overlap_pair_bytes(d, cap, PL, cmax), free_b, chunk_gb);
    Bufs bufs;
    double *dW, *dg, *gws = nullptr;
    int64_t *doff, *dex;
    int32_t *dchi, *dncls, *dpairs;
    OV_TRY(bufs.get(&dW, total));
    OV_TRY(bufs.get(&doff, (int64_t)off.size()));
    OV_TRY(bufs.get(&dchi, (int64_t)chi.size()));
    OV_TRY(bufs.get(&dncls, K));
    OV_TRY(bufs.get(&dpairs, 2 * P));
    OV_TRY(bufs.get(&dg, P * gsz));
    OV_TRY(bufs.get(&dex, P));
    if (!lds) OV_TRY(bufs.get(&gws, block * state));
    OV_TRY(hipMemcpyAsync(dW, hw.data(), (size_t)total * sizeof(double), hipMemcpyHostToDevice, s));
    OV_TRY(hipMemcpyAsync(doff, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    OV_TRY(hipMemcpyAsync(dchi, chi.data(), chi.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    OV_TRY(hipMemcpyAsync(dncls, h.ncls.data(), (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, s));
    OV_TRY(hipMemcpyAsync(dpairs, hp.data(), hp.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    OV_TRY(hipMemsetAsync(dg, 0, (size_t)(P * gsz) * sizeof(double), s));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t* e; ~Ev() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    OV_TRY(hipEventCreate(&ev[0]));
    OV_TRY(hipEventCreate(&ev[1]));
    OvArgs g{dW, doff, dchi, dncls, dpairs, dg, dex, gws, overlap_env_doubles(cap), overlap_x_doubles(d, cap), T, d, p, cmax, overlap_ld(cap)};
    OV_TRY(hipEventRecord(ev[0], s));
    for (int64_t q0 = 0; q0 < P; q0 += block) {
        const int count = (int)std::min(block, P - q0);
        g.pairs = dpairs + 2 * q0;
        g.g = dg + q0 * gsz;
        g.ex = dex + q0;
        OV_TRY(launch_overlap(h.cx, lds, g, count, (size_t)state * sizeof(double), s));
    }
    OV_TRY(hipEventRecord(ev[1], s));
    std::vector<double> hg((size_t)(P * gsz));
    std::vector<int64_t> hex((size_t)P);
    OV_TRY(hipMemcpyAsync(hg.data(), dg, hg.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    OV_TRY(hipMemcpyAsync(hex.data(), dex, hex.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    OV_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    OV_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (seconds) *seconds = ms * 1e-3;
    // g of a pair is brought to a largest magnitude in [1, 2) by one more power of two, which joins the exponent
    for (int64_t q = 0; q < P; ++q) {
        const double* src = &hg[(size_t)(q * gsz)];
        double* dst = g_out + (int64_t)order[q] * gsz;
        double mx = 0.0;
        for (int64_t e = 0; e < gsz; ++e) mx = std::max(mx, std::fabs(src[e]));
        if (hex[q] == OV_ZERO || !(mx > 0.0)) {
            lg_out[order[q]] = -INFINITY;
            continue;
        }
        const int eg = std::ilogb(mx);
        for (int64_t e = 0; e < gsz; ++e) dst[e] = std::ldexp(src[e], -eg);
        lg_out[order[q]] = (double)(hex[q] + eg) * 0.6931471805599453094;
    }
    return hipSuccess;
}

}  // namespace mpst
