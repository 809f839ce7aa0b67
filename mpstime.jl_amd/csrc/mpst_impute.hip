// Imputation engine: src/Imputation/MPS_methods.jl:42-330 + sampling_utils.jl:98-275 of the
// reference, batched over test instances - the reference works one instance at a time (and farms instances out with
// @distributed, hyperopt_utils.jl:201).
//
// The reference conditions the class MPS on the known values (precondition, :42-99), moves the orthogonality centre to
// the first missing site (orthogonalize!, :115) and then walks the missing sites: reduced density matrix rho = A A'
// of the centre tensor, "probability" of every grid value x_k (20 001 of them), cumulative trapezoid, median / mode /
// inverse-transform sample, projection onto the chosen state, next site (impute_at!, :103-177).  Canonical forms are a
// gauge choice: the same rho (up to a positive scale that cancels everywhere) is
//     rho = (L W_j) R_{j+1} (L W_j)^T,
// with L the left environment VECTOR of the known / already imputed sites and R_{j+1} the right environment MATRIX in
// which known sites are projected and missing sites are traced out.  That turns one instance into two sweeps over the
// chain with chi x chi state, and the batch into two launches:
//   k_imp_right : a workgroup per instance.  R_T = 1, R_j = M_j R_{j+1} M_j^T (known, M_j = sum_s phi_s W_j[s]) or
//                 sum_s W_j[s] R_{j+1} W_j[s]^T (missing); R_{j+1} is stored for every missing j.  Rescaled by its trace at
//                 every site.  While the pass has met known sites only, R = r r^H: a vector recursion r <- M_j r.
//   k_imp_leftb : sixteen instances per workgroup (mpst_impute_batched.inl) where the densities are closed-form (TRIG below)
//                 and the panels fit the LDS; the closed-form density (ImpDens) and the formation of its coefficients are written
//                 once for both sweeps, in mpst_impute_density.inl; the same steps as
//   k_imp_left  : a workgroup per instance.  L_0 = 1; known site: L <- L M_j; missing site: rho, p_k = |rho phi_k|^2 over the grid (the value the
//                 reference computes: rdm is a plain Matrix there, so get_conditional_probability(state, rdm) takes the
//                 (state, A::Matrix) method, sampling_utils.jl:19-41, and returns |state' * rdm|^2, not state' rdm state), block-wide prefix sums, selection,
//                 weighted median absolute deviation, L <- phi* (L W_j).
// Both imputation orders of the reference (impute_order = :forwards / :backwards, MPS_methods.jl:107-121): backwards is
// the mirror image - the matrices come from the left, the vector from the right - and runs through the same kernels with
// the two bond indices of every site tensor swapped (`rev`).
// Element types.  The model (site tensors, encoded known values, grid states) is real or complex (the reference's
// Fourier / Sahand bases give complex MPSs, trained through its legacy ITensor path); the chain contractions - site
// tensors, environment matrices, the vector L - run in fp64 or in fp32 (MFMA f32 16x16x4, half the LDS and HBM bytes),
// while the density on the grid, its prefix sums and every selection are always fp64.  Complex matrices live in LDS as
// separate real and imaginary planes so that a complex product is four real MFMA chains.
// Limits: d <= 16, chi <= 128.  The environment pass keeps two padded chi x chi matrices (+ a 16-row block) in LDS up to
// chi = 64 (complex fp64: 48); beyond that k_imp_right_big works out of global scratch.
#include "mpst_internal.h"
#include "mpst_prefix_plan.h"
#include "mpst_segment_plan.h"
#include "mpst_rolling_plan.h"
#include <cstdlib>
#include <type_traits>

namespace mpst {

constexpr int IMP_T = 256;
constexpr int IMP_MAXD = 16;

// element e of an array of R (real) or of interleaved (re, im) pairs of R (complex)
template <typename R, bool CX> __device__ __forceinline__ void zload(const R* __restrict__ p, int64_t e, R& re, R& im) {
    if constexpr (CX) {
        const typename Mx<R>::vec2 t = reinterpret_cast<const typename Mx<R>::vec2*>(p)[e];
        re = t.x;
        im = t.y;
    } else {
        re = p[e];
        im = R(0);
    }
}
template <typename R, bool CX> __device__ __forceinline__ void zstore(R* __restrict__ p, int64_t e, R re, R im) {
    if constexpr (CX) {
        typename Mx<R>::vec2 t;
        t.x = re;
        t.y = im;
        reinterpret_cast<typename Mx<R>::vec2*>(p)[e] = t;
    } else {
        p[e] = re;
    }
}

__device__ __forceinline__ double blk_sum(double x, double* red) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double blk_max(double x, double* red) {
    x = wave_max(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// A site as seen by a pass that enters through bond `in` and leaves through bond `out`: element (i, s, o) of the class
// MPS of class `cls` ([a][s][b] with live dimensions; the label site holds one such block per class).  Forwards the
// left pass enters from the left (in = left bond), backwards from the right; the matrix pass is the opposite.
template <typename R> struct SiteView {
    const R* W;
    int Din, Dout;
    int64_t si, ss, so;      // strides of the (in, s, out) indices, in elements
};
template <typename R, bool CX> __device__ __forceinline__ SiteView<R> site_view(const ImpModel& v, int j, int cls, bool in_is_left) {
    const int Dl = v.chi[j], Dr = v.chi[j + 1];
    int64_t off = (int64_t)j * v.site_stride;
    if (j == *v.label_site) off += (int64_t)cls * Dl * v.d * Dr;
    SiteView<R> sv;
    sv.W = (const R*)v.sites + (CX ? 2 : 1) * off;
    sv.ss = Dr;
    if (in_is_left) {
        sv.Din = Dl; sv.Dout = Dr; sv.si = (int64_t)v.d * Dr; sv.so = 1;
    } else {
        sv.Din = Dr; sv.Dout = Dl; sv.si = 1; sv.so = (int64_t)v.d * Dr;
    }
    return sv;
}

// ---- right environments ------------------------------------------------------------------------------------------------
// Matrices in LDS are (real plane, imaginary plane) pairs, zero-padded to multiples of 16 rows / columns.
template <typename R> struct Plane {
    R *r, *i;
};

// The environment of the sites beyond a missing site, R' = sum_s Ms R Ms^H with Ms = W_j[s] (missing site) or
// sum_q conj(phi_q) W_j[q] (known site).  LDS holds R, the site matrix and the whole product T1 = Ms R: one workgroup per CU,
// a wave per 16 x 16 tile (16 waves at chi = 64), 3 barriers per site matrix, and W_j[s + 1] is on its way into registers while
// W_j[s] is used.  (Round 3's kernel kept one 16-row block of T1 and two workgroups of 4 waves per CU: 8 x 4 x 2 phases of
// 64 MFMAs per site with a barrier after each - 482 ms at configs[4] for 175 ms of matrix time; this one 313 ms.)  Both products read their operands ALONG rows: T1 = Ms R = Ms (R)^H because R is Hermitian, R' += T1 Ms^H;
// the MFMA does not care which k goes with which (k-quarter, step) slot as long as A and B agree, so lane (row, kq) takes
// k = kq * ks + u: consecutive steps are consecutive addresses, one ds_read_b128 feeds 4 (fp32) or 2 (fp64) steps.
template <int NW> __device__ __forceinline__ double blk_sum_n(double x, double* red) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += red[w];
    return t;
}
// C (+)= A[a_row0 .. +15][:] * B[n0 .. +15][:]^H over k = 0 .. 4 ks - 1; ks a multiple of 16 / sizeof(R), rows 16-byte aligned
template <typename R, bool CX>
__device__ __forceinline__ void lds_tile_rows(typename Mx<R>::acc_t& cr, typename Mx<R>::acc_t& ci, Plane<R> A, int a_row0, Plane<R> B, int n0,
                                              int ks, int ld) {
    constexpr int VEC = 16 / (int)sizeof(R);
    typedef R vec_t __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63, i16 = lane & 15, kq = lane >> 4;
    const int ia = (a_row0 + i16) * ld + kq * ks, ib = (n0 + i16) * ld + kq * ks;
    const vec_t* Ar = reinterpret_cast<const vec_t*>(A.r + ia);
    const vec_t* Br = reinterpret_cast<const vec_t*>(B.r + ib);
    const vec_t* Ai = reinterpret_cast<const vec_t*>(A.i + ia);
    const vec_t* Bi = reinterpret_cast<const vec_t*>(B.i + ib);
    const int ng = ks / VEC;
    for (int g = 0; g < ng; ++g) {
        const vec_t ar = Ar[g], br = Br[g];
        if constexpr (CX) {
            const vec_t ai = Ai[g], bi = Bi[g];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                cr = Mx<R>::mma(ar[e], br[e], cr);
                ci = Mx<R>::mma(ai[e], br[e], ci);
                cr = Mx<R>::mma(ai[e], bi[e], cr);
                ci = Mx<R>::mma(-ar[e], bi[e], ci);
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) cr = Mx<R>::mma(ar[e], br[e], cr);
        }
    }
}
// The same tile for complex operands with THREE real products per k-step instead of four (the 3M form of (a + ib)(c - id)):
//   K1 += (a + b) c,  K2 += a (-d - c),  K3 += b (c - d);   re = K1 - K3,  im = K1 + K2.
// The derived operands are formed in registers from the planes (three vector adds per 128-bit read); the three accumulators stay
// separate across k-loops and site matrices (the combination is linear) and are combined once.  Normwise as accurate as the
// four-product form; a quarter of the matrix-pipe time gone.
template <typename R>
__device__ __forceinline__ void lds_tile_rows3(typename Mx<R>::acc_t& k1, typename Mx<R>::acc_t& k2, typename Mx<R>::acc_t& k3, Plane<R> A, int a_row0,
                                               Plane<R> B, int n0, int ks, int ld) {
    constexpr int VEC = 16 / (int)sizeof(R);
    typedef R vec_t __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63, i16 = lane & 15, kq = lane >> 4;
    const int ia = (a_row0 + i16) * ld + kq * ks, ib = (n0 + i16) * ld + kq * ks;
    const vec_t* Ar = reinterpret_cast<const vec_t*>(A.r + ia);
    const vec_t* Br = reinterpret_cast<const vec_t*>(B.r + ib);
    const vec_t* Ai = reinterpret_cast<const vec_t*>(A.i + ia);
    const vec_t* Bi = reinterpret_cast<const vec_t*>(B.i + ib);
    const int ng = ks / VEC;
    for (int g = 0; g < ng; ++g) {
        const vec_t ar = Ar[g], br = Br[g], ai = Ai[g], bi = Bi[g];
        const vec_t as = ar + ai, bd = -bi - br, bs = br - bi;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            k1 = Mx<R>::mma(as[e], br[e], k1);
            k2 = Mx<R>::mma(ar[e], bd[e], k2);
            k3 = Mx<R>::mma(ai[e], bs[e], k3);
        }
    }
}
template <typename R, bool CX, int IMR_T>
__global__ __launch_bounds__(IMR_T) void k_imp_right(ImpModel v, const uint8_t* __restrict__ missing, R* __restrict__ Rbuf,
                                                      int max_missing, const int32_t* __restrict__ ord, int rev) {
    using acc_t = typename Mx<R>::acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    R* smem = reinterpret_cast<R*>(smem_raw);
    __shared__ double red[IMR_T / 64];
    constexpr int NW = IMR_T / 64, NQ = IMR_T == 512 ? 5 : 4;      // waves; site-matrix elements per thread (the host picks IMR_T)
    constexpr int NTW = IMR_T == 512 ? 2 : 1;                      // tiles per wave: 16 on 16 waves, 9 on 8, <= 4 on 4
    constexpr int ZW = CX ? 2 : 1;
    const int64_t i = ord[blockIdx.x];          // instance; scratch buffers are indexed by blockIdx.x (chunk-local)
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const uint8_t* mi = missing + i * T;
    int nm = 0;
    for (int j = 0; j < T; ++j) nm += mi[j] ? 1 : 0;
    if (nm == 0) return;
    const int cls = v.label[i];
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 16 / (int)sizeof(R);       // rows 16-byte aligned and 4 banks apart: conflict-free 128-bit operand reads
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const Plane<R> Rc{smem, smem + (ZW - 1) * msz};
    const Plane<R> Ms0{smem + ZW * msz, smem + ZW * msz + (ZW - 1) * msz};              // the site matrix, double-buffered
    const Plane<R> Ms1{smem + 3 * ZW * msz, smem + 3 * ZW * msz + (ZW - 1) * msz};
    const Plane<R> T1{smem + 2 * ZW * msz, smem + 2 * ZW * msz + (ZW - 1) * msz};
    for (int e = tid; e < 4 * ZW * msz; e += IMR_T) smem[e] = R(0);
    __syncthreads();
    if (tid == 0) Rc.r[0] = R(1);
    __syncthreads();
    // this wave's tiles of the tpr x tpr grid: wave (and wave + NW: only 9 tiles on 8 waves)
    const bool h0 = wave < ntile, h1 = NTW > 1 && wave + NW < ntile;
    const int rbA = h0 ? wave / tpr : 0, wcA = h0 ? wave % tpr : 0;
    const int rbB = h1 ? (wave + NW) / tpr : rbA, wcB = h1 ? (wave + NW) % tpr : wcA;
    int slot = 0;
    // ---- the known sites the pass meets before its first missing one: R = r r^H stays an outer product ----------------------------
    // r <- M_j r (M_j = sum_q conj(phi_q) W_j[q]) is one matrix-vector product against the site tensor where the matrix recursion
    // forms M_j from d site matrices and multiplies twice (15 us a site, a third of the sites of a 50 % block in mid-chain).
    // r and the partial sums live in the T1 planes.
    int step0 = 0;
    while (step0 < T && mi[rev ? step0 : T - 1 - step0] == 0) ++step0;        // (nm > 0: there is one)
    if (step0 > 0) {
        R* vr = T1.r;                       // r: [cp]; partial sums behind it: [IMR_T]
        R* vi = T1.i;
        R* pr_ = T1.r + cp;
        R* pi_ = T1.i + cp;
        if (tid < cp) {
            vr[tid] = tid == 0 ? R(1) : R(0);
            if constexpr (CX) vi[tid] = R(0);
        }
        __syncthreads();
        int Dlast = 1;
        for (int step = 0; step < step0; ++step) {
            const int j = rev ? step : T - 1 - step;
            const SiteView<R> sv = site_view<R, CX>(v, j, cls, rev != 0);
            const int Di = sv.Din, Do = sv.Dout;
            const R* ph = (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
            // lanes along the index that is contiguous in memory: the input bond (this pass enters through the tensor's fast bond:
            // a wave per output value, a wave-wide sum) or the output bond (a wave per input value, partial vectors summed in LDS)
            constexpr int VB = 4;          // states per batch of loads (eight: registers - a workgroup per CU less in the smaller forms - for 1 %)
            R nr = R(0), ni = R(0);
            if (sv.si == 1) {
                const R xr = lane < Di ? vr[lane] : R(0), xi = (CX && lane < Di) ? vi[lane] : R(0);
                for (int o0 = wave; o0 < Do; o0 += 2 * NW) {
                    const int o1 = o0 + NW;
                    R a0r = R(0), a0i = R(0), a1r = R(0), a1i = R(0);
                    for (int q0 = 0; q0 < d; q0 += VB) {
                        R w0r[VB], w0i[VB], w1r[VB], w1i[VB], fr_[VB], fi_[VB];
#pragma unroll
                        for (int u = 0; u < VB; ++u) {
                            w0r[u] = w0i[u] = w1r[u] = w1i[u] = fr_[u] = fi_[u] = R(0);
                            if (q0 + u < d) {
                                zload<R, CX>(ph, q0 + u, fr_[u], fi_[u]);
                                if (lane < Di) {
                                    zload<R, CX>(sv.W, (int64_t)lane + (int64_t)(q0 + u) * sv.ss + (int64_t)o0 * sv.so, w0r[u], w0i[u]);
                                    if (o1 < Do) zload<R, CX>(sv.W, (int64_t)lane + (int64_t)(q0 + u) * sv.ss + (int64_t)o1 * sv.so, w1r[u], w1i[u]);
                                }
                            }
                        }
#pragma unroll
                        for (int u = 0; u < VB; ++u) {           // += conj(phi_q) W(i, q, o)
                            a0r = fma(fr_[u], w0r[u], a0r);
                            a1r = fma(fr_[u], w1r[u], a1r);
                            if constexpr (CX) {
                                a0r = fma(fi_[u], w0i[u], a0r);
                                a0i = fma(fr_[u], w0i[u], a0i);
                                a0i = fma(-fi_[u], w0r[u], a0i);
                                a1r = fma(fi_[u], w1i[u], a1r);
                                a1i = fma(fr_[u], w1i[u], a1i);
                                a1i = fma(-fi_[u], w1r[u], a1i);
                            }
                        }
                    }
                    // times r_i, summed over the lanes
                    const double s0r = wave_sum((double)(CX ? fma(a0r, xr, -a0i * xi) : a0r * xr));
                    const double s1r = wave_sum((double)(CX ? fma(a1r, xr, -a1i * xi) : a1r * xr));
                    double s0i = 0.0, s1i = 0.0;
                    if constexpr (CX) {
                        s0i = wave_sum((double)fma(a0r, xi, a0i * xr));
                        s1i = wave_sum((double)fma(a1r, xi, a1i * xr));
                    }
                    if (lane == 0) {
                        pr_[o0] = (R)s0r;
                        if constexpr (CX) pi_[o0] = (R)s0i;
                        if (o1 < Do) {
                            pr_[o1] = (R)s1r;
                            if constexpr (CX) pi_[o1] = (R)s1i;
                        }
                    }
                }
                __syncthreads();
                if (tid < Do) {
                    nr = pr_[tid];
                    if constexpr (CX) ni = pi_[tid];
                }
            } else {
                // (so == 1) a wave per input value i, lanes along o; VB states in flight
                R ar = R(0), ai = R(0);
                for (int i_ = wave; i_ < Di; i_ += NW) {
                    const R xr = vr[i_], xi = CX ? vi[i_] : R(0);
                    for (int q0 = 0; q0 < d; q0 += VB) {
                        R wr[VB], wi[VB], fr_[VB], fi_[VB];
#pragma unroll
                        for (int u = 0; u < VB; ++u) {
                            wr[u] = wi[u] = fr_[u] = fi_[u] = R(0);
                            if (q0 + u < d) {
                                zload<R, CX>(ph, q0 + u, fr_[u], fi_[u]);
                                if (lane < Do) zload<R, CX>(sv.W, (int64_t)i_ * sv.si + (int64_t)(q0 + u) * sv.ss + (int64_t)lane * sv.so, wr[u], wi[u]);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < VB; ++u) {
                            // conj(phi_q) r_i
                            const R cr = CX ? fma(fr_[u], xr, fi_[u] * xi) : fr_[u] * xr;
                            const R ci = CX ? fma(fr_[u], xi, -fi_[u] * xr) : R(0);
                            ar = fma(cr, wr[u], ar);
                            if constexpr (CX) {
                                ar = fma(-ci, wi[u], ar);
                                ai = fma(cr, wi[u], ai);
                                ai = fma(ci, wr[u], ai);
                            }
                        }
                    }
                }
                if (lane < Do) {
                    pr_[wave * Do + lane] = ar;
                    if constexpr (CX) pi_[wave * Do + lane] = ai;
                }
                __syncthreads();
                if (tid < Do) {
                    for (int w = 0; w < NW; ++w) {
                        nr += pr_[w * Do + tid];
                        if constexpr (CX) ni += pi_[w * Do + tid];
                    }
                }
            }
            __syncthreads();
            if (tid < cp) {
                vr[tid] = tid < Do ? nr : R(0);
                if constexpr (CX) vi[tid] = tid < Do ? ni : R(0);
            }
            // |r| = 1 (the trace of r r^H): every quantity downstream is scale-free
            const double n2 = blk_sum_n<NW>(tid < Do ? (double)nr * (double)nr + (double)ni * (double)ni : 0.0, red);
            const R sc = n2 > 0.0 ? (R)(1.0 / sqrt(n2)) : R(1);
            if (tid < cp) {
                vr[tid] *= sc;
                if constexpr (CX) vi[tid] *= sc;
            }
            __syncthreads();
            Dlast = Do;
        }
        for (int e = tid; e < cp * cp; e += IMR_T) {
            const int a_ = e / cp, b2 = e - a_ * cp;
            const bool live = a_ < Dlast && b2 < Dlast;
            const R xr = vr[a_], yr = vr[b2];
            if constexpr (CX) {
                const R xi = vi[a_], yi = vi[b2];                       // r_a conj(r_b)
                Rc.r[a_ * ld + b2] = live ? fma(xr, yr, xi * yi) : R(0);
                Rc.i[a_ * ld + b2] = live ? fma(xi, yr, -xr * yi) : R(0);
            } else {
                Rc.r[a_ * ld + b2] = live ? xr * yr : R(0);
            }
        }
        __syncthreads();
    }
    for (int step = step0; step < T; ++step) {
        const int j = rev ? step : T - 1 - step;
        const SiteView<R> sv = site_view<R, CX>(v, j, cls, rev != 0);
        const int Di = sv.Din, Do = sv.Dout;
        const bool miss = mi[j] != 0;
        const R* ph = (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
        const int ns = miss ? d : 1;
        const bool in_fast = sv.si == 1;
        const int Df = in_fast ? Di : Do;
        const int tmo = (Do + 15) >> 4, tni = (Di + 15) >> 4;
        // the site after this one (the pass stops at the first missing site of the sweep, so there is one)
        const int jn = rev ? j + 1 : j - 1;
        const bool has_next = step + 1 < T;
        const SiteView<R> svn = site_view<R, CX>(v, has_next ? jn : j, cls, rev != 0);
        // the (at most NQ) elements of the site matrix this thread carries
        int64_t off[NQ];
        int dst[NQ];
        R fr[NQ], fi[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int e = tid + q * IMR_T;
            const int slow = e / Df, fast = e - slow * Df;
            const int ii = in_fast ? fast : slow, oo = in_fast ? slow : fast;
            off[q] = (int64_t)ii * sv.si + (int64_t)oo * sv.so;
            dst[q] = e < Di * Do ? oo * ld + ii : -1;
        }
        auto fetch = [&](int s_) {          // Ms = W_j[s_] (missing) or sum_q conj(phi_q) W_j[q] (known)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                fr[q] = R(0);
                fi[q] = R(0);
            }
            if (miss) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (dst[q] >= 0) zload<R, CX>(sv.W, off[q] + (int64_t)s_ * sv.ss, fr[q], fi[q]);
            } else {
                // complex models: two states per round trip to the L2 (four spill at 128 registers; real models lose a workgroup
                // per CU to the extra registers and more than they gain: one)
                constexpr int KB = CX ? 2 : 1;
                for (int q0 = 0; q0 < d; q0 += KB) {
                    R pr[KB], pi[KB], wr[KB][NQ], wi[KB][NQ];
#pragma unroll
                    for (int u = 0; u < KB; ++u) {
                        pr[u] = pi[u] = R(0);
                        const bool lq = q0 + u < d;
                        if (lq) zload<R, CX>(ph, q0 + u, pr[u], pi[u]);
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            wr[u][q] = R(0);
                            wi[u][q] = R(0);
                            if (lq && dst[q] >= 0) zload<R, CX>(sv.W, off[q] + (int64_t)(q0 + u) * sv.ss, wr[u][q], wi[u][q]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < KB; ++u) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            fr[q] = fma(pr[u], wr[u][q], fr[q]);
                            if constexpr (CX) {
                                fr[q] = fma(pi[u], wi[u][q], fr[q]);
                                fi[q] = fma(pr[u], wi[u][q], fi[q]);
                                fi[q] = fma(-pi[u], wr[u][q], fi[q]);
                            }
                        }
                    }
                }
            }
        };
        acc_t rnr[NTW], rni[NTW], rn3[NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            rnr[t] = acc_t{0, 0, 0, 0};
            rni[t] = acc_t{0, 0, 0, 0};
            rn3[t] = acc_t{0, 0, 0, 0};
        }
        auto put = [&](const Plane<R>& M) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (dst[q] >= 0) {
                    M.r[dst[q]] = fr[q];
                    if constexpr (CX) M.i[dst[q]] = fi[q];
                }
        };
        // a missing site: its environment goes to memory first - behind the request for the first site matrix, whose round trip
        // the stores cover; the pass ends at the last missing site
        const bool last = miss && slot + 1 == nm;
        if (!last) fetch(0);
        if (miss) {
            R* out = Rbuf + ((int64_t)blockIdx.x * max_missing + slot) * cm * cm * ZW;
            for (int e = tid; e < Di * Di; e += IMR_T) {
                const int at = (e / Di) * ld + (e % Di);
                zstore<R, CX>(out, e, Rc.r[at], CX ? Rc.i[at] : R(0));
            }
            ++slot;
            if (last) break;
        }
        put(Ms0);
        __syncthreads();
        if (ns > 1) fetch(1);                       // in flight during the first product
        for (int s = 0; s < ns; ++s) {
            // (by value, pointer by pointer: a ternary between the two Plane lvalues selects an address and parks both in scratch)
            const Plane<R> Ms{(s & 1) ? Ms1.r : Ms0.r, (s & 1) ? Ms1.i : Ms0.i};
            // T1 = Ms R^H (Do x Di)
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                const int rb = t == 0 ? rbA : rbB, wc = t == 0 ? wcA : wcB;
                if ((t == 0 ? h0 : h1) && rb < tmo && wc < tni) {
                    acc_t ar = {0, 0, 0, 0}, ai = {0, 0, 0, 0};
                    if constexpr (CX) {
                        acc_t k3 = {0, 0, 0, 0};
                        lds_tile_rows3<R>(ar, ai, k3, Ms, 16 * rb, Rc, 16 * wc, ks, ld);     // ar = K1, ai = K2
                        ai = ar + ai;
                        ar = ar - k3;
                    } else {
                        lds_tile_rows<R, CX>(ar, ai, Ms, 16 * rb, Rc, 16 * wc, ks, ld);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int at = (16 * rb + Mx<R>::row(kq, r)) * ld + 16 * wc + i16;
                        T1.r[at] = ar[r];
                        if constexpr (CX) T1.i[at] = ai[r];
                    }
                }
            }
            // the next site matrix goes into the other buffer (last read before the previous step's closing barrier): its
            // load had a whole product to arrive, and the step needs two barriers instead of three
            if (s + 1 < ns) put(Plane<R>{(s & 1) ? Ms0.r : Ms1.r, (s & 1) ? Ms0.i : Ms1.i});
            __syncthreads();
            if (s + 2 < ns) fetch(s + 2);
            // R' += T1 Ms^H (Do x Do)
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                const int rb = t == 0 ? rbA : rbB, wc = t == 0 ? wcA : wcB;
                if ((t == 0 ? h0 : h1) && rb < tmo && wc < tmo) {
                    if constexpr (CX) lds_tile_rows3<R>(rnr[t], rni[t], rn3[t], T1, 16 * rb, Ms, 16 * wc, ks, ld);      // K1, K2, K3
                    else lds_tile_rows<R, CX>(rnr[t], rni[t], T1, 16 * rb, Ms, 16 * wc, ks, ld);
                }
            }
            lds_barrier();
        }
        // the new environment replaces the old one, rescaled by its trace (taken from the accumulators: the diagonal tiles' lanes
        // with row == column); rows / columns beyond Do are zero for the next site
        double tr = 0.0;
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const bool have = t == 0 ? h0 : h1;
            const int rb = t == 0 ? rbA : rbB, wc = t == 0 ? wcA : wcB;
            if constexpr (CX) {                      // re = K1 - K3, im = K1 + K2
                rni[t] = rnr[t] + rni[t];
                rnr[t] = rnr[t] - rn3[t];
            }
            if (have && rb == wc) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (Mx<R>::row(kq, r) == i16 && 16 * rb + i16 < Do) tr += (double)rnr[t][r];
            }
        }
        tr = blk_sum_n<NW>(tr, red);
        const R sc = tr > 0.0 ? (R)(1.0 / tr) : R(1);
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const bool have = t == 0 ? h0 : h1;
            const int rb = t == 0 ? rbA : rbB, wc = t == 0 ? wcA : wcB;
            if (!have) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rb + Mx<R>::row(kq, r), col = 16 * wc + i16;
                const bool live = row < Do && col < Do;
                Rc.r[row * ld + col] = live ? rnr[t][r] * sc : R(0);
                if constexpr (CX) Rc.i[row * ld + col] = live ? rni[t][r] * sc : R(0);
            }
        }
        // The site-matrix buffers keep their zeros outside the live block as long as the matrices do not shrink (`put` writes live
        // elements only; T1 needs none: its stale rows / columns meet zeros of the site matrix or rows of R' that are masked above)
        if (has_next && (svn.Dout < Do || svn.Din < Di)) {
            for (int e = tid; e < cp * cp; e += IMR_T) {
                const int a_ = e / cp, b2 = e - a_ * cp;
                Ms0.r[a_ * ld + b2] = R(0);
                Ms1.r[a_ * ld + b2] = R(0);
                if constexpr (CX) {
                    Ms0.i[a_ * ld + b2] = R(0);
                    Ms1.i[a_ * ld + b2] = R(0);
                }
            }
        }
        __syncthreads();
    }
}

// ---- right environments beyond the LDS limit ---------------------------------------------------------------------------
// chi up to CAP_LIMIT (128): the four chi x chi matrices of an instance live in global scratch (L2-resident: 4 x 128 KB
// per workgroup) and the MFMA operands are read straight from there, 8 k-steps of loads in flight per wave.  A missing
// site's W_j[s] is not even copied: the A / B operands walk the stored tensor with its own strides.  Slower per flop than
// the LDS kernel (it costs speed, not capability).
#ifndef GM_KU
#define GM_KU 4
#endif
template <typename R> struct GMat {        // element (r, c) = p[(r * sr + c * sc) * ZW (+ 1)], rows x cols live
    const R* p;
    int64_t sr, sc;
    int rows, cols;
};
template <typename R, bool CX> __device__ __forceinline__ void gload(const GMat<R>& m, int r, int c, R& re, R& im) {
    re = R(0);
    im = R(0);
    if (r < m.rows && c < m.cols) zload<R, CX>(m.p, (int64_t)r * m.sr + (int64_t)c * m.sc, re, im);
}
// C (M x N row-major, leading dimension ldc) (+)= A * B  or  A * B^H (TB: B is the N x K operand); one unit = a 16-row
// block times NTE column tiles, nothing in the k-loop predicated on the tile count (see lds_mm_unit)
template <typename R, bool CX, int NTE, bool TB>
__device__ __forceinline__ void gmem_mm_unit(R* __restrict__ Cm, int ldc, const GMat<R>& A, const GMat<R>& B, int M, int N, int K, int m0, int nb,
                                             bool accumulate) {
    using acc_t = typename Mx<R>::acc_t;
    const int lane = threadIdx.x & 63, i16 = lane & 15, kq = lane >> 4;
    constexpr int KU = GM_KU;                 // k-steps per batch of loads
    acc_t accr[NTE], acci[NTE];
#pragma unroll
    for (int t = 0; t < NTE; ++t) {
        accr[t] = acc_t{0, 0, 0, 0};
        acci[t] = acc_t{0, 0, 0, 0};
        if (accumulate) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = m0 + Mx<R>::row(kq, r), cc = (nb + t) * 16 + i16;
                if (rr < M && cc < N) {
                    R x, y;
                    zload<R, CX>(Cm, (int64_t)rr * ldc + cc, x, y);
                    accr[t][r] = x;
                    acci[t][r] = y;
                }
            }
        }
    }
    for (int k0 = 0; k0 < K; k0 += 4 * KU) {
        R ar[KU], ai[KU], br[NTE][KU], bi[NTE][KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int k = k0 + 4 * u + kq;
            gload<R, CX>(A, m0 + i16, k < K ? k : A.cols, ar[u], ai[u]);
#pragma unroll
            for (int t = 0; t < NTE; ++t) {
                const int n = (nb + t) * 16 + i16;
                if (TB) gload<R, CX>(B, n, k < K ? k : B.cols, br[t][u], bi[t][u]);
                else gload<R, CX>(B, k < K ? k : B.rows, n, br[t][u], bi[t][u]);
            }
        }
        // k-steps beyond K multiply zeros (gload returns 0 out of range): no test needed
#pragma unroll
        for (int u = 0; u < KU; ++u) {
#pragma unroll
            for (int t = 0; t < NTE; ++t) {
                accr[t] = Mx<R>::mma(ar[u], br[t][u], accr[t]);
                if constexpr (CX) {
                    accr[t] = Mx<R>::mma(TB ? ai[u] : -ai[u], bi[t][u], accr[t]);
                    acci[t] = Mx<R>::mma(ai[u], br[t][u], acci[t]);
                    acci[t] = Mx<R>::mma(TB ? -ar[u] : ar[u], bi[t][u], acci[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NTE; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = m0 + Mx<R>::row(kq, r), cc = (nb + t) * 16 + i16;
            if (rr < M && cc < N) zstore<R, CX>(Cm, (int64_t)rr * ldc + cc, accr[t][r], acci[t][r]);
        }
    }
}
template <typename R, bool CX>
__device__ __forceinline__ void gmem_mm(R* __restrict__ Cm, int ldc, GMat<R> A, GMat<R> B, int M, int N, int K, bool tb, bool accumulate) {
    const int wave = threadIdx.x >> 6;
    const int tm = (M + 15) >> 4, tn = (N + 15) >> 4;
    constexpr int NT = 2;                     // column tiles per unit
    const int ngrp = (tn + NT - 1) / NT;
    for (int unit = wave; unit < tm * ngrp; unit += 4) {
        const int m0 = (unit / ngrp) * 16, nb = (unit % ngrp) * NT;
        const bool two = nb + 1 < tn;
        if (tb) {
            if (two) gmem_mm_unit<R, CX, 2, true>(Cm, ldc, A, B, M, N, K, m0, nb, accumulate);
            else gmem_mm_unit<R, CX, 1, true>(Cm, ldc, A, B, M, N, K, m0, nb, accumulate);
        } else {
            if (two) gmem_mm_unit<R, CX, 2, false>(Cm, ldc, A, B, M, N, K, m0, nb, accumulate);
            else gmem_mm_unit<R, CX, 1, false>(Cm, ldc, A, B, M, N, K, m0, nb, accumulate);
        }
    }
}

template <typename R, bool CX>
__global__ __launch_bounds__(IMP_T) void k_imp_right_big(ImpModel v, const uint8_t* __restrict__ missing, R* __restrict__ Rbuf,
                                                         R* __restrict__ work /* [chunk][4][cap*cap] */, int max_missing, const int32_t* __restrict__ ord, int rev) {
    __shared__ double red[4];
    constexpr int ZW = CX ? 2 : 1;
    const int64_t i = ord[blockIdx.x];          // instance; scratch buffers are indexed by blockIdx.x (chunk-local)
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x;
    const uint8_t* mi = missing + i * T;
    int nm = 0;
    for (int j = 0; j < T; ++j) nm += mi[j] ? 1 : 0;
    if (nm == 0) return;
    const int cls = v.label[i];
    const int64_t msz = (int64_t)cm * cm * ZW;
    R* base = work + (int64_t)blockIdx.x * 4 * msz;
    R* Rc = base;                  // current environment, compact [Di][Di]
    R* Rn = base + msz;            // next one, compact [Do][Do]
    R* Mb = base + 2 * msz;        // M_j of a known site, [Do][Di]
    R* T1 = base + 3 * msz;        // [Do][Di]
    if (tid == 0) zstore<R, CX>(Rc, 0, R(1), R(0));
    __syncthreads();
    int slot = 0;
    for (int step = 0; step < T; ++step) {
        const int j = rev ? step : T - 1 - step;
        const SiteView<R> sv = site_view<R, CX>(v, j, cls, rev != 0);
        const int Di = sv.Din, Do = sv.Dout;
        const bool miss = mi[j] != 0;
        if (miss) {
            R* out = Rbuf + ((int64_t)blockIdx.x * max_missing + slot) * cm * cm * ZW;
            for (int e = tid; e < Di * Di * ZW; e += IMP_T) out[e] = Rc[e];
            ++slot;
            if (slot == nm) break;
        }
        const GMat<R> Rm{Rc, Di, 1, Di, Di};
        if (miss) {
            for (int s_ = 0; s_ < d; ++s_) {
                // W_j[s] as the (out x in) matrix of this pass, read in place
                const GMat<R> Ws{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};
                gmem_mm<R, CX>(T1, Di, Ws, Rm, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<R, CX>(Rn, Do, GMat<R>{T1, Di, 1, Do, Di}, Ws, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            }
        } else {
            const R* ph = (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
            const bool in_fast = sv.si == 1;
            const int Df = in_fast ? Di : Do;
            for (int e0 = tid; e0 < Di * Do; e0 += 8 * IMP_T) {
                R accr[8], acci[8];
                int64_t off[8];
                int dst[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int e = e0 + q * IMP_T;
                    const int slow = e / Df, fast = e - slow * Df;
                    const int ii = in_fast ? fast : slow, oo = in_fast ? slow : fast;
                    off[q] = (int64_t)ii * sv.si + (int64_t)oo * sv.so;
                    dst[q] = oo * Di + ii;
                    accr[q] = R(0);
                    acci[q] = R(0);
                }
                for (int qq = 0; qq < d; ++qq) {
                    R pr, pi;
                    zload<R, CX>(ph, qq, pr, pi);
                    R wr[8], wi[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        wr[q] = R(0);
                        wi[q] = R(0);
                        if (e0 + q * IMP_T < Di * Do) zload<R, CX>(sv.W, off[q] + (int64_t)qq * sv.ss, wr[q], wi[q]);
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        accr[q] = fma(pr, wr[q], accr[q]);
                        if constexpr (CX) {
                            accr[q] = fma(pi, wi[q], accr[q]);
                            acci[q] = fma(pr, wi[q], acci[q]);
                            acci[q] = fma(-pi, wr[q], acci[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (e0 + q * IMP_T < Di * Do) zstore<R, CX>(Mb, dst[q], accr[q], acci[q]);
            }
            __syncthreads();
            const GMat<R> Mm{Mb, Di, 1, Do, Di};
            gmem_mm<R, CX>(T1, Di, Mm, Rm, Do, Di, Di, false, false);
            __syncthreads();
            gmem_mm<R, CX>(Rn, Do, GMat<R>{T1, Di, 1, Do, Di}, Mm, Do, Do, Di, true, false);
            __syncthreads();
        }
        double tr = 0.0;
        for (int a_ = tid; a_ < Do; a_ += IMP_T) tr += (double)Rn[((int64_t)a_ * Do + a_) * ZW];
        tr = blk_sum(tr, red);
        const R sc = tr > 0.0 ? (R)(1.0 / tr) : R(1);
        for (int e = tid; e < Do * Do * ZW; e += IMP_T) Rn[e] *= sc;
        __syncthreads();
        R* tmp = Rc;
        Rc = Rn;
        Rn = tmp;
    }
}

// ---- the sweep with the imputation itself ---------------------------------------------------------------------------------
constexpr int IMP_MAXQ = 16;    // levels per call
// what a chain reads through its instance and what it addresses by itself
struct ImpChain {
    int64_t inst;               // instance: missing, phi, label
    int64_t rslot;              // chunk-local slot of the instance's environments in Rbuf
    int64_t row;                // inst * ntraj + trajectory: the row of u, x_out, err_out
    int traj;
};
__device__ __forceinline__ ImpChain imp_chain(const ImpArgs& g, int64_t c) {
    ImpChain ch;
    ch.rslot = g.ntraj == 1 ? c : c / g.ntraj;
    ch.inst = g.ord[ch.rslot];
    ch.traj = (int)(c - ch.rslot * g.ntraj);
    ch.row = ch.inst * g.ntraj + ch.traj;
    return ch;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a counter-based generator,
// ten rounds of two 32 x 32 -> 64 bit multiplications on a 128-bit counter under a 64-bit key that is bumped by the Weyl constants
// after every round.  No state: the draw of (row id, trajectory, site, trial) under a seed is a pure function of the five.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// counter = (row id low word, row id high word, trajectory, site | trial << 20), key = (seed low word, seed high word); the
// uniform number in [0, 1) takes the top 27 bits of output word 0 and the top 26 bits of word 1: 53 bits, every value exact
constexpr int IMP_SEED_SITE_BITS = 20;
static_assert((1 << IMP_SEED_SITE_BITS) == IMPUTE_SEED_MAX_SITES && (1 << (32 - IMP_SEED_SITE_BITS)) == IMPUTE_SEED_MAX_TRIALS, "counter word 3");
__device__ __forceinline__ double philox_uniform(unsigned long long seed, int64_t row, int traj, int site, int trial) {
    uint32_t c[4] = {(uint32_t)(uint64_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)traj,
                     (uint32_t)site | ((uint32_t)trial << IMP_SEED_SITE_BITS)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (double)(((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6)) * (1.0 / 9007199254740992.0);
}
// trial t of chain `ch` at site j
__device__ __forceinline__ double imp_uniform(const ImpArgs& g, const ImpChain& ch, int T, int j, int t) {
    if (g.use_seed) return philox_uniform(g.seed, g.row_id ? g.row_id[ch.inst] : ch.inst, ch.traj, j, t);
    return g.u[(ch.row * T + j) * g.ntrial + t];
}
enum { IMP_MEDIAN = 0, IMP_MODE = 1, IMP_QUANTILE = 2, IMP_MEAN = 3, IMP_ITS_REJECT = 4 };
enum { IMP_BASIS_LEGENDRE = 0, IMP_BASIS_LEGENDRE_NO_NORM = 1, IMP_BASIS_FOURIER = 2, IMP_BASIS_STOUDENMIRE = 3, IMP_BASIS_SAHAND = 4,
       IMP_BASIS_UNIFORM = 5 };

// ---- a density on the grid: prefix sums, cumulative trapezoid, selections ----------------------------------------------------------
// What k_imp_left does with the density of a missing site and k_sc_grid (mpst_sitecond.inl) with a leave-one-out conditional, written
// once.  Everything here is called by all IMP_T threads of a workgroup; where a prefix sum or a cdf value comes from (the table S_k or
// a closed form) is the caller's `Sabs` / `cdf_at`.
//
// Prefix sums of p[0 .. n): each wave scans a contiguous quarter of the grid, 64 values per row: coalesced loads eight rows ahead, a
// DPP inclusive scan per row, a wave-uniform carry.  S holds the sums relative to the start of the quarter; the
// four quarter totals go to wtot and GridSums::at adds the right ones.  No barrier inside the pass.  (The first
// version gave every thread a contiguous segment: four passes of uncoalesced, latency-bound loads, 64 us per
// imputed site whatever chi and d - 70 % of the kernel at chi = 32.)
__device__ __forceinline__ void grid_prefix_sums(const double* p, double* S, int n, int nrow, int rpw, double* wtot) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = wave * rpw, row1 = min(nrow, row0 + rpw);
    constexpr int PF = 8;
    double buf[PF], cur[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) {
        const int k = (row0 + q) * 64 + lane;
        buf[q] = (row0 + q < row1 && k < n) ? p[k] : 0.0;
    }
    double carry = 0.0;
    for (int rr = row0; rr < row1; rr += PF) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            cur[q] = buf[q];
            const int k = (rr + PF + q) * 64 + lane;
            buf[q] = (rr + PF + q < row1 && k < n) ? p[k] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            if (rr + q < row1) {
                const double x = wave_incl_scan(cur[q]) + carry;
                const int k = (rr + q) * 64 + lane;
                if (k < n) S[k] = x;
                carry = readlane_f64(x, 63);
            }
        }
    }
    if (lane == 0) wtot[wave] = carry;
}
// the inclusive prefix sum S_k from the table grid_prefix_sums left
struct GridSums {
    const double* S;
    int quarter;
    double w1, w2, w3;          // the totals of the quarters before the second, third and fourth
    __device__ __forceinline__ double at(int k) const {
        const int qd = k / quarter;
        return S[k] + (qd == 0 ? 0.0 : (qd == 1 ? w1 : (qd == 2 ? w2 : w3)));
    }
};
// cumulative trapezoid at grid index k (cumul_integrate(x, p, TrapezoidalEvenFast()))
template <typename SF> __device__ __forceinline__ double grid_cdf_at(int k, double dx, double p0, SF Sabs) {
    if (k == 0) return 0.0;
    return 0.5 * dx * ((Sabs(k - 1) + Sabs(k)) - p0);
}
// first index of the block-wide maximum of p (mode; also the weighted median's "one weight above half" rule) from every thread's
// own first maximum (pmax, kmax)
__device__ __forceinline__ int grid_arg_pmax(double pmax, int kmax, int n, double* red, int* isel, double& gmax) {
    const int tid = threadIdx.x;
    gmax = blk_max(pmax, red);
    int cand = (pmax == gmax) ? kmax : n;
    cand = -(int)wave_max((double)(-cand));
    __syncthreads();
    if ((tid & 63) == 0) isel[tid >> 6] = cand;
    __syncthreads();
    const int km = min(min(isel[0], isel[1]), min(isel[2], isel[3]));
    __syncthreads();
    return km;
}
// number of leading rows of 64 whose LAST element satisfies a monotone predicate (true ... true false ... false
// along the grid): every thread tests the ends of its rows (two gathers in flight), one barrier
template <typename PF> __device__ __forceinline__ int grid_rows_passing(int n, int nrow, int* isel, PF pred_at) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int c = 0;
    for (int r = tid; r < nrow; r += IMP_T) c += pred_at(min(n - 1, 64 * r + 63)) ? 1 : 0;
    int w = 0;
    for (int it = 0; it < (nrow + IMP_T - 1) / IMP_T; ++it) w += __popcll(__ballot(c > it));
    __syncthreads();
    if (lane == 0) isel[wave] = w;
    __syncthreads();
    const int tot = isel[0] + isel[1] + isel[2] + isel[3];
    __syncthreads();
    return tot;
}
// argmin_k |cdf_k / Z - target|: the cdf is non-decreasing, so the minimiser sits at the crossing.  The points
// with cdf_k <= target * Z form a prefix: first the row of 64 that holds its end (row ends only), then the
// position inside that row (one coalesced row, every wave for itself) - two memory round trips instead of a pass
// over the grid - and finally the reference's own expression |cdf_k / Z - target| on the handful of
// neighbours, first minimum wins (argmin).
template <typename CF> __device__ __forceinline__ int grid_quantile(double target, double Z, int n, int nrow, int* isel, CF cdf_at) {
    const int lane = threadIdx.x & 63;
    const double tz = target * Z;
    const int rc = grid_rows_passing(n, nrow, isel, [&](int k) { return cdf_at(k) <= tz; });
    int klo = n - 1;
    if (rc < nrow) {
        const int k = 64 * rc + lane;
        const bool le = k < n && cdf_at(k) <= tz;
        klo = 64 * rc + __popcll(__ballot(le)) - 1;
    }
    if (klo < 0) klo = 0;
    // (the six candidates on six lanes, then the first minimum in lane order = in grid order)
    const int kfirst = max(0, klo - 2), klast = min(n - 1, klo + 3);
    const int kk = kfirst + lane;
    double a = 1e300;
    if (lane < 6 && kk <= klast) a = fabs(cdf_at(kk) / Z - target);
    int ks = klo;
    double best = 1e300;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        const double al = readlane_f64(a, l);
        if (al < best) {
            best = al;
            ks = kfirst + l;
        }
    }
    return ks;
}
// StatsBase.median(|x - x_c|, pweights(p / Z)): the deviations grow with the distance from kc on the uniform
// grid; the cumulative weight of the window [kc - jj, kc + jj] comes from the prefix sums and grows with jj: the
// same two-level search for the first half-width whose window outweighs half the total.  `heaviest(mid, km)`: whether one grid
// value alone outweighs half the total (then km is its index): the caller knows how to find the maximum of its density.
// jhit: the half-width at which the window tipped the balance (-1: one value outweighed half the total, or no window did).
template <typename SF, typename HF>
__device__ __forceinline__ double grid_wmad(int kc, const double* grid_x, double Stot, double Z, int n, int nrow, int* isel, SF Sabs, HF heaviest,
                                            int& jtip) {
    const int lane = threadIdx.x & 63;
    const double xc = grid_x[kc];
    const double mid = 0.5 * (Stot / Z);
    int km = 0;
    jtip = -1;
    if (heaviest(mid, km)) return fabs(grid_x[km] - xc);
    auto light = [&](int jj) {          // the window of half-width jj does NOT yet outweigh half the total
        const int hi = min(n - 1, kc + jj), lo = kc - jj - 1;
        const double shi = Sabs(hi), slo = lo >= 0 ? Sabs(lo) : 0.0;
        return !((shi - slo) / Z > mid);
    };
    const int rc = grid_rows_passing(n, nrow, isel, light);
    int jhit = n;
    if (rc < nrow) {
        const int jj = 64 * rc + lane;
        const unsigned long long bal = __ballot(jj < n && !light(jj));
        if (bal) jhit = 64 * rc + (__ffsll((long long)bal) - 1);
    }
    if (jhit >= n) return 0.0;
    jtip = jhit;
    // the element that tips the balance is one of the two at distance jhit (whichever exists)
    const int lo = kc - jhit, hi = kc + jhit;
    return (lo >= 0) ? fabs(grid_x[lo] - xc) : fabs(grid_x[min(hi, n - 1)] - xc);
}

#include "mpst_impute_density.inl"

// The conditioning state of the mean (get_mean_from_rdm): the encoding of E[x] = ex itself, which is not a grid value.  Legendre with
// the encoder's arithmetic (k_encode; bases.jl:77-92,108), Fourier (bases.jl:23-42: cispi(f x) / sqrt(d), f = 0, 1, -1, 2, -2, ...) or
// one of the other closed forms; one thread, store(k, re, im) per state.
// (Not the enc_* of mpst_encode.hip: the Fourier encoder multiplies by 1 / sqrt(d) where this divides by sqrt(d) - the last bit differs.)
template <typename SF> __device__ __forceinline__ void imp_mean_state(int basis, double ex, int d, SF store) {
    if (basis == IMP_BASIS_FOURIER) {
        for (int k = 0; k < d; ++k) {
            const int f = (k + 1) / 2 * ((k & 1) ? 1 : -1);
            double sn, cs;
            sincospi((double)f * ex, &sn, &cs);
            store(k, cs / sqrt((double)d), sn / sqrt((double)d));
        }
    } else if (basis == IMP_BASIS_STOUDENMIRE) {
        // angle_encode (bases.jl:7-21, periods = 1/4): cispi(3x/2) cos(pi x/2), cispi(-3x/2) sin(pi x/2)
        double s3, c3, sh, ch;
        sincospi(1.5 * ex, &s3, &c3);
        sincospi(0.5 * ex, &sh, &ch);
        store(0, c3 * ch, s3 * ch);
        store(1, c3 * sh, -s3 * sh);
    } else if (basis == IMP_BASIS_SAHAND) {
        // sahand_encode (bases.jl:45-68): d/2 intervals of width 2/d, two states each, zero outside their interval
        const double dxs = 2.0 / d;
        for (int k = 0; k < d; ++k) {
            const int interval = k / 2 + 1;
            const double startx = (interval - 1) * dxs;
            const bool inside = startx <= ex && ex <= interval * dxs;
            double s3, c3, sh, ch;
            sincospi(1.5 * ex / dxs, &s3, &c3);
            sincospi(0.5 * (ex - startx) / dxs, &sh, &ch);
            const bool odd = (k & 1) == 0;                  // i = k + 1 odd
            store(k, inside ? (odd ? c3 * ch : c3 * sh) : 0.0, inside ? (odd ? s3 * ch : -s3 * sh) : 0.0);
        }
    } else if (basis == IMP_BASIS_UNIFORM) {
        for (int k = 0; k < d; ++k) store(k, 1.0 / d, 0.0);
    } else {
        const double nrm = sqrt(sqrt((2 * d + 1) / 2.0) * d);
        double q0 = 1.0, q1 = ex;
        for (int k = 0; k < d; ++k) {
            double pk;
            if (k == 0) pk = 1.0;
            else if (k == 1) pk = ex;
            else {
                const int m = k - 1;
                pk = ((2 * m + 1) * ex * q1 - m * q0) / (m + 1);
                q0 = q1;
                q1 = pk;
            }
            double val = pk * sqrt((2.0 * k + 1.0) / 2.0);
            if (basis == IMP_BASIS_LEGENDRE) val = val / nrm;
            store(k, val, 0.0);
        }
    }
}

// ---- the steps of k_imp_left at one site (all called by the IMP_T threads of the chain's workgroup) ---------------------------------
// normalise rho by its trace (p scales with the square, every quantity below is scale-free)
template <bool CX> __device__ __forceinline__ void imp_rdm_normalise(double* rho, double* rhoi, int d) {
    double tr = 0.0;
    for (int s_ = 0; s_ < d; ++s_) tr += rho[s_ * IMP_MAXD + s_];
    const double sc = tr > 0.0 ? 1.0 / tr : 1.0;
    __syncthreads();
    for (int e = threadIdx.x; e < d * d; e += IMP_T) {
        rho[(e / d) * IMP_MAXD + (e % d)] *= sc;
        if constexpr (CX) rhoi[(e / d) * IMP_MAXD + (e % d)] *= sc;
    }
    __syncthreads();
}
// The coefficient block of ImpDens from rho, dealt out over the workgroup: M = rho^H rho / rho^T rho an entry per thread, then
// complex: a thread per harmonic;  real: c_l = sum_ss' M_ss' A[l][s][s'] with eight threads per l, their partial sums combined as a tree.
// tmr / tmi: M (complex: rows IMP_MAXD apart; real: dense [d][d], as the table Atab); lpart: the partial sums.
template <bool CX>
__device__ __forceinline__ void imp_dens_coeffs(const double* rho, const double* rhoi, double* tmr, double* tmi, double* lpart, const double* Atab,
                                                double* co, int d, double x0, double dxu) {
    const int tid = threadIdx.x, ldm = CX ? IMP_MAXD : d;
    for (int e = tid; e < d * d; e += IMP_T) {
        const int a = e / d, bx = e - a * d;
        double mr = 0.0, mi = 0.0;
        for (int s_ = 0; s_ < d; ++s_) {
            if constexpr (CX) {
                const double ar = rho[s_ * IMP_MAXD + a], ai = rhoi[s_ * IMP_MAXD + a];
                const double br = rho[s_ * IMP_MAXD + bx], bi = rhoi[s_ * IMP_MAXD + bx];
                mr = fma(ar, br, fma(ai, bi, mr));
                mi = fma(ar, bi, fma(-ai, br, mi));
            } else {
                mr = fma(rho[s_ * IMP_MAXD + a], rho[s_ * IMP_MAXD + bx], mr);
            }
        }
        tmr[a * ldm + bx] = mr;
        if constexpr (CX) tmi[a * ldm + bx] = mi;
    }
    __syncthreads();
    if constexpr (CX) {
        // harmonic m: c_m sums the entries whose frequencies differ by m, B_m = c_m i e^{i pi (m x0 - m dx / 2)} / (2 sin(pi m dx / 2))
        if (tid < d) {
            const int m = tid;
            double cr = 0.0, ci = 0.0;
            for (int a = 0; a < d; ++a) {
                const int fa = (a + 1) / 2 * ((a & 1) ? 1 : -1), fb = fa + m;
                const int bx = fb == 0 ? 0 : (fb > 0 ? 2 * fb - 1 : -2 * fb);        // the state of frequency fb
                if (bx >= d) continue;
                cr += tmr[a * ldm + bx];
                ci += tmi[a * ldm + bx];
            }
            const double sc = (m == 0 ? 1.0 : 2.0) / (double)d;
            cr *= sc;
            ci = m == 0 ? 0.0 : ci * sc;
            co[m] = cr;
            co[IMP_MAXD + m] = ci;
            double br_ = 0.0, bi_ = 0.0;
            if (m > 0) {
                double sa, ca, sn, cs;
                sincospi(0.5 * m * dxu, &sa, &ca);
                sincospi((double)m * x0 - 0.5 * m * dxu, &sn, &cs);
                const double er = -sn / (2.0 * sa), ei = cs / (2.0 * sa);               // i e^{i pi (m x0 - m dx / 2)} / (2 sin)
                br_ = cr * er - ci * ei;
                bi_ = cr * ei + ci * er;
            }
            co[2 * IMP_MAXD + m] = br_;
            co[3 * IMP_MAXD + m] = bi_;
        }
    } else {
        const int l = tid >> 3, part = tid & 7;
        if (l < 2 * d - 1) {
            const double* Al = Atab + l * d * d;
            double a = 0.0;
            for (int e = part; e < d * d; e += 8) a = fma(tmr[e], Al[e], a);
            lpart[l * 8 + part] = a;
        }
        __syncthreads();
        if (tid < 2 * d - 1) {
            const double* q = lpart + tid * 8;
            co[tid] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
        }
    }
    __syncthreads();
}
// Ln <- sum_s conj(state_s) (L W)[s]: a known site's encoded value (condition_until_next!: class_mps[i] * dag(timeseries_enc[i])) or
// the chosen state of a missing one (Am = ms' * A, MPS_methods.jl:161); state(s, re, im) loads component s
template <typename R, bool CX, typename LF> __device__ __forceinline__ void imp_project(Plane<R> LW, Plane<R> Ln, int d, int Do, int cm, LF state) {
    for (int o = threadIdx.x; o < Do; o += IMP_T) {
        R tr = R(0), ti = R(0);
        for (int q = 0; q < d; ++q) {
            R pr, pi;
            state(q, pr, pi);
            tr = fma(pr, LW.r[q * cm + o], tr);
            if constexpr (CX) {
                tr = fma(pi, LW.i[q * cm + o], tr);
                ti = fma(pr, LW.i[q * cm + o], ti);
                ti = fma(-pi, LW.r[q * cm + o], ti);
            }
        }
        Ln.r[o] = tr;
        if constexpr (CX) Ln.i[o] = ti;
    }
}
// L <- Ln rescaled by its largest magnitude
template <typename R, bool CX> __device__ __forceinline__ void imp_rescale(Plane<R> L, Plane<R> Ln, int Do, double* red) {
    const int tid = threadIdx.x;
    double mx = 0.0;
    for (int o = tid; o < Do; o += IMP_T) {
        mx = fmax(mx, fabs((double)Ln.r[o]));
        if constexpr (CX) mx = fmax(mx, fabs((double)Ln.i[o]));
    }
    mx = blk_max(mx, red);
    const R sc = mx > 0.0 ? (R)(1.0 / mx) : R(1);
    for (int o = tid; o < Do; o += IMP_T) {
        L.r[o] = Ln.r[o] * sc;
        if constexpr (CX) L.i[o] = Ln.i[o] * sc;
    }
    __syncthreads();
}

// OCC = workgroups per CU the kernel is compiled for.  Two (256 VGPRs) for real models and for complex ones with d <= 5: the
// latency-bound loops gain more from the second resident workgroup than the ~300 B of spills cost (45 -> 32 ms at
// chi = 32); complex models with larger d keep the whole register file (their density loop spills too much at 256).
//
// TRIG = densities in closed form (ImpDens, mpst_impute_density.inl), for grid states the host recognised from the tables themselves:
// * complex models, the Fourier basis cispi(f_s x) / sqrt(d) on a uniform grid: p(x) = |rho phi(x)|^2 = sum_ss' conj(phi_s)
//   (rho^H rho)_ss' phi_s' is a trigonometric polynomial with the d harmonics m = f_s' - f_s >= 0, and the prefix sums of the
//   reference's cumulative trapezoid over the grid are geometric series:
//     p(x) = c_0 + sum_m Re(c_m e^{i pi m x}),   S_K = sum_{k<=K} p(x_k) = c_0 (K + 1) + sum_m Re(B_m (1 - w_m^{K+1})),
//     w_m = e^{i pi m dx},  B_m = c_m e^{i pi m x_0} / (1 - w_m) = c_m i e^{i pi (m x_0 - m dx / 2)} / (2 sin(pi m dx / 2)).
// * real models, the Legendre bases kappa_s P_s(x) (bases.jl:70-108, with or without the norm) on a uniform grid in [-1, 1]:
//   p(x) = sum_ss' (rho^T rho)_ss' phi_s phi_s' = sum_{l <= 2d-2} c_l P_l(x) through the linearisation P_s P_s' = sum_l a(s,s',l) P_l
//   (table from the host, Gauss-Legendre quadrature), and the prefix sums follow from the Euler-Maclaurin formula, which a
//   polynomial of degree 2d - 2 <= 30 on a grid of step 1e-4 satisfies to rounding with two correction terms:
//     S_K = (F(x_K) - F(x_0)) / h + (p(x_0) + p(x_K)) / 2 + h/12 (p1(x_K) - p1(x_0)) - h^3/720 (p3(x_K) - p3(x_0)),
//   F = the antiderivative sum_l c_l (P_{l+1} - P_{l-1}) / (2l + 1), p1 / p3 the first / third derivative; P_l and its
//   derivatives by their three-term recurrences.
// Neither the 20 001 x d table of grid states nor p_k and S_k ever exist: the median, the quantiles and the WMAD evaluate S at the
// O(log n) indices their searches visit, the mode and the mean evaluate p at every grid value from 2 d coefficients in LDS.
//
// DIST = the distribution outputs of mpst_impute_dist next to the median (get_cdfs, src/Imputation/imputation.jl:581-622;
// impute_med_and_get_cdf!, MPS_methods.jl:350-466; get_cdf, sampling_utils.jl:205-241): more levels through the median's own
// quantile() and the normalised cdf from the median's own cumulative trapezoid (cdf_at: ImpDens::cdf in closed form, grid_cdf_at on
// the table).  A template flag, not a branch: the instantiations without it compile exactly as before (the table kernels are at
// their register limit).
//
// Per site: contract (LW), then a known site projects onto its encoded value; a missing site forms U, rho and the density, selects by
// g.method with this kernel's block-wide searches, projects onto the chosen state; rescale.  (The method switch stands in the kernel:
// as a function over an object of the searches, for k_imp_leftb to share, it cost k_imp_leftb 0.8 % of the default benchmark pass and
// this kernel 3.5 % of a complex fp64 call with levels, profiles/impute_sweep_refactor.txt.)
template <typename R, bool CX, int OCC, bool TRIG = false, bool DIST = false> __global__ __launch_bounds__(IMP_T, OCC) void k_imp_left(ImpModel v, ImpArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    R* smem = reinterpret_cast<R*>(smem_raw);
    __shared__ double red[4];
    __shared__ double rho[IMP_MAXD * IMP_MAXD];           // real part
    __shared__ double rhoi[CX ? IMP_MAXD * IMP_MAXD : 1]; // imaginary part
    __shared__ double wtot[4];                              // totals of the four quarters of the grid (prefix sums)
    __shared__ int isel[4];
    __shared__ double lev[DIST ? IMP_MAXQ : 1];             // DIST: the levels
    __shared__ double dco[TRIG ? ImpDens<CX>::NCO : 1];     // TRIG: the coefficient block of the density
    __shared__ double tmr[TRIG ? IMP_MAXD * IMP_MAXD : 1], tmi[TRIG ? IMP_MAXD * IMP_MAXD : 1];      // rho^H rho
    __shared__ double lpart[(TRIG && !CX) ? 2 * IMP_MAXD * 8 : 1];       // Legendre: partial sums of c_l
    constexpr int ZW = CX ? 2 : 1;
    const ImpChain ch = imp_chain(g, blockIdx.x);        // this workgroup's chain; p / S scratch is the chain's own (blockIdx.x)
    const int64_t i = ch.inst;
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x;
    const uint8_t* mi = g.missing + i * T;
    int nm = 0;
    for (int j = 0; j < T; ++j) nm += mi[j] ? 1 : 0;
    if (nm == 0) return;
    const int cls = v.label[i];
    // vectors and d x chi panels as (real plane, imaginary plane) pairs
    const int vsz = cm, psz = IMP_MAXD * cm;
    const Plane<R> L{smem, smem + (ZW - 1) * vsz};
    const Plane<R> Ln{smem + ZW * vsz, smem + ZW * vsz + (ZW - 1) * vsz};
    R* pan = smem + 2 * ZW * vsz;
    const Plane<R> LW{pan, pan + (ZW - 1) * psz};                               // [d][cm]
    const Plane<R> U{pan + ZW * psz, pan + ZW * psz + (ZW - 1) * psz};          // [d][cm]
    R* msp = pan + 2 * ZW * psz;
    const Plane<R> ms{msp, msp + (ZW - 1) * IMP_MAXD};                          // [d] chosen state
    double* Atab = reinterpret_cast<double*>(msp + ZW * IMP_MAXD);               // TRIG, real: [2d-1][d][d] linearisation table
    if constexpr (TRIG && !CX) {
        for (int e = threadIdx.x; e < (2 * v.d - 1) * v.d * v.d; e += IMP_T) Atab[e] = g.lin[e];
    }
    double* p = g.pbuf + (int64_t)blockIdx.x * g.ngrid;
    double* S = g.sbuf + (int64_t)blockIdx.x * g.ngrid;
    const int n = g.ngrid;
    const double dx = g.grid_x[1] - g.grid_x[0];
    if constexpr (DIST) {
        if (tid < g.nq) lev[tid] = g.levels[tid];
    }
    if (tid == 0) {
        L.r[0] = R(1);
        if constexpr (CX) L.i[0] = R(0);
    }
    __syncthreads();
    int seen = 0;
    for (int step = 0; step < T; ++step) {
        const int j = g.rev ? T - 1 - step : step;
        const SiteView<R> sv = site_view<R, CX>(v, j, cls, g.rev == 0);
        const int Di = sv.Din, Do = sv.Dout;
        // LW[s][o] = sum_i L[i] W(i, s, o) for both kinds of site; a known site then contracts s with its encoded value.
        // Forwards consecutive threads are consecutive o (contiguous in memory), backwards the loads of a thread are.  Two
        // outputs x 16 bond values = 32 loads in flight per thread: the loop is a chain of round trips to the L2 / memory-side
        // cache (the 262 KB site tensor of configs[4] is re-read by every instance), so their number is what counts.
        // (This panel, the U panel and the table density stay lambdas of the kernel: as functions of their own, inlined, the same
        // text costs the complex table kernels 870 B and the complex closed-form kernels at OCC 3 / 4 240-300 B more scratch per lane,
        // profiles/impute_sweep_refactor.txt.)
        {
            const int nout = d * Do;
            auto lw_pass = [&](auto NOc) {
                constexpr int NO = decltype(NOc)::value, LQ = TRIG ? 16 : 8;    // (the table kernels are at their register limit: 8 as before)
                for (int e0 = tid; e0 < nout; e0 += NO * IMP_T) {
                    const int e1 = e0 + IMP_T;
                    const bool v1 = NO == 2 && e1 < nout;
                    const int s0 = e0 / Do, o0 = e0 - s0 * Do, s1 = v1 ? e1 / Do : s0, o1 = v1 ? e1 - s1 * Do : o0;
                    const int64_t w0 = (int64_t)s0 * sv.ss + (int64_t)o0 * sv.so, w1 = (int64_t)s1 * sv.ss + (int64_t)o1 * sv.so;
                    R tr0 = R(0), ti0 = R(0), tr1 = R(0), ti1 = R(0);
                    for (int a0 = 0; a0 < Di; a0 += LQ) {
                        R wr0[LQ], wi0[LQ], wr1[NO == 2 ? LQ : 1], wi1[NO == 2 ? LQ : 1];
#pragma unroll
                        for (int q = 0; q < LQ; ++q) {
                            wr0[q] = wi0[q] = R(0);
                            if constexpr (NO == 2) wr1[q] = wi1[q] = R(0);
                            if (a0 + q < Di) {
                                zload<R, CX>(sv.W, w0 + (int64_t)(a0 + q) * sv.si, wr0[q], wi0[q]);
                                if constexpr (NO == 2)
                                    if (v1) zload<R, CX>(sv.W, w1 + (int64_t)(a0 + q) * sv.si, wr1[q], wi1[q]);
                            }
                        }
#pragma unroll
                        for (int q = 0; q < LQ; ++q)
                            if (a0 + q < Di) {
                                const R lr = L.r[a0 + q];
                                tr0 = fma(lr, wr0[q], tr0);
                                if constexpr (NO == 2) tr1 = fma(lr, wr1[q], tr1);
                                if constexpr (CX) {
                                    const R li = L.i[a0 + q];
                                    tr0 = fma(-li, wi0[q], tr0);
                                    ti0 = fma(lr, wi0[q], ti0);
                                    ti0 = fma(li, wr0[q], ti0);
                                    if constexpr (NO == 2) {
                                        tr1 = fma(-li, wi1[q], tr1);
                                        ti1 = fma(lr, wi1[q], ti1);
                                        ti1 = fma(li, wr1[q], ti1);
                                    }
                                }
                            }
                    }
                    LW.r[s0 * cm + o0] = tr0;
                    if constexpr (CX) LW.i[s0 * cm + o0] = ti0;
                    if (v1) {
                        LW.r[s1 * cm + o1] = tr1;
                        if constexpr (CX) LW.i[s1 * cm + o1] = ti1;
                    }
                }
            };
            if (nout > IMP_T) lw_pass(std::integral_constant<int, 2>{});
            else lw_pass(std::integral_constant<int, 1>{});
        }
        __syncthreads();
        if (mi[j] == 0) {
            const R* ph = (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
            imp_project<R, CX>(LW, Ln, d, Do, cm, [&](int q, R& pr, R& pi) { zload<R, CX>(ph, q, pr, pi); });
        } else {
            const R* Rm = (const R*)g.Rbuf + (ch.rslot * g.max_missing + (nm - 1 - seen)) * cm * cm * ZW;      // the instance's environment of the site
            ++seen;
            // U = LW R   (R: this instance's environment of the site, [Do][Do] compact, read once from memory - same load pattern)
            {
                const int nout = d * Do;
                auto u_pass = [&](auto NOc) {
                    constexpr int NO = decltype(NOc)::value, LQ = TRIG ? 16 : 8;    // (the table kernels are at their register limit: 8 as before)
                    for (int e0 = tid; e0 < nout; e0 += NO * IMP_T) {
                        const int e1 = e0 + IMP_T;
                        const bool v1 = NO == 2 && e1 < nout;
                        const int s0 = e0 / Do, o0 = e0 - s0 * Do, s1 = v1 ? e1 / Do : s0, o1 = v1 ? e1 - s1 * Do : o0;
                        const bool share = o1 == o0;      // (the usual case: the two outputs share the column of R)
                        R tr0 = R(0), ti0 = R(0), tr1 = R(0), ti1 = R(0);
                        for (int q0 = 0; q0 < Do; q0 += LQ) {
                            R r0[LQ], j0[LQ], r1[NO == 2 ? LQ : 1], j1[NO == 2 ? LQ : 1];
#pragma unroll
                            for (int q = 0; q < LQ; ++q) {
                                r0[q] = j0[q] = R(0);
                                if constexpr (NO == 2) r1[q] = j1[q] = R(0);
                                if (q0 + q < Do) {
                                    zload<R, CX>(Rm, (int64_t)(q0 + q) * Do + o0, r0[q], j0[q]);
                                    if constexpr (NO == 2)
                                        if (v1 && !share) zload<R, CX>(Rm, (int64_t)(q0 + q) * Do + o1, r1[q], j1[q]);
                                }
                            }
#pragma unroll
                            for (int q = 0; q < LQ; ++q)
                                if (q0 + q < Do) {
                                    const R a0r = LW.r[s0 * cm + q0 + q];
                                    tr0 = fma(a0r, r0[q], tr0);
                                    if constexpr (CX) {
                                        const R a0i = LW.i[s0 * cm + q0 + q];
                                        tr0 = fma(-a0i, j0[q], tr0);
                                        ti0 = fma(a0r, j0[q], ti0);
                                        ti0 = fma(a0i, r0[q], ti0);
                                    }
                                    if constexpr (NO == 2) {
                                        const R x1 = share ? r0[q] : r1[q], y1 = share ? j0[q] : j1[q];
                                        const R a1r = LW.r[s1 * cm + q0 + q];
                                        tr1 = fma(a1r, x1, tr1);
                                        if constexpr (CX) {
                                            const R a1i = LW.i[s1 * cm + q0 + q];
                                            tr1 = fma(-a1i, y1, tr1);
                                            ti1 = fma(a1r, y1, ti1);
                                            ti1 = fma(a1i, x1, ti1);
                                        }
                                    }
                                }
                        }
                        U.r[s0 * cm + o0] = tr0;
                        if constexpr (CX) U.i[s0 * cm + o0] = ti0;
                        if (v1) {
                            U.r[s1 * cm + o1] = tr1;
                            if constexpr (CX) U.i[s1 * cm + o1] = ti1;
                        }
                    }
                };
                if (nout > IMP_T) u_pass(std::integral_constant<int, 2>{});
                else u_pass(std::integral_constant<int, 1>{});
            }
            __syncthreads();
            // rho = U LW^H, rows IMP_MAXD apart: four threads per entry (a quad: every fourth bond value each, summed over the quad with DPP).
            // (In the kernel body: as a function of its own it cost the table kernels up to 0.9 %, profiles/impute_sweep_refactor.txt.)
            for (int e4 = tid; e4 < ((4 * d * d + 63) & ~63); e4 += IMP_T) {
                const int e = e4 >> 2, part = e4 & 3;
                const bool live = e < d * d;
                const int s_ = live ? e / d : 0, s2 = live ? e - s_ * d : 0;
                R tr = R(0), ti = R(0);
                for (int k = part; k < Do; k += 4) {
                    const R ur = U.r[s_ * cm + k], br = LW.r[s2 * cm + k];
                    tr = fma(ur, br, tr);
                    if constexpr (CX) {
                        const R ui_ = U.i[s_ * cm + k], bi = LW.i[s2 * cm + k];
                        tr = fma(ui_, bi, tr);
                        ti = fma(ui_, br, ti);
                        ti = fma(-ur, bi, ti);
                    }
                }
                double dr = (double)tr, di = (double)ti;
                dr += dpp_mov<0xB1>(dr);               // quad_perm [1, 0, 3, 2]
                di += dpp_mov<0xB1>(di);
                dr += dpp_mov<0x4E>(dr);               // quad_perm [2, 3, 0, 1]
                di += dpp_mov<0x4E>(di);
                if (live && part == 0) {
                    rho[s_ * IMP_MAXD + s2] = dr;
                    if constexpr (CX) rhoi[s_ * IMP_MAXD + s2] = di;
                }
            }
            __syncthreads();
            imp_rdm_normalise<CX>(rho, rhoi, d);
            // ---- the density: closed form (TRIG), or p_k and its prefix sums S_k as tables in the chain's scratch ------------------
            double pmax = -1.0;       // every thread's own first maximum of p (TRIG: only once a method asks, see arg_pmax)
            int kmax = 0;
            const int nrow = (n + 63) >> 6, rpw = (nrow + 3) >> 2, quarter = rpw * 64;
            ImpDens<CX> den;
            if constexpr (TRIG) {
                den.co = dco;
                den.d = d;
                den.x0 = g.x0;
                den.dxu = g.dxu;
                den.dx = dx;
                imp_dens_coeffs<CX>(rho, rhoi, tmr, tmi, lpart, Atab, dco, d, g.x0, g.dxu);
                den.close();
            } else {
            // p_k = |rho phi_k|^2: grid values interleaved over the threads (consecutive lanes read consecutive encoded
            // states: coalesced), and every thread's own first maximum (pmax, kmax); then every thread sums its CONTIGUOUS segment
            // for the block-wide scan (grid_prefix_sums)
            if constexpr (CX) {
                // rho stays in LDS (every lane reads the same entry: broadcast), two grid values per round trip
                const double2* gp = reinterpret_cast<const double2*>(g.grid_phi + (int64_t)j * g.grid_site_stride);      // site j's table (stride 0: the shared one)
                auto evalc = [&](auto DD) {
                    constexpr int D = decltype(DD)::value;
                    for (int kb = tid; kb < n; kb += 2 * IMP_T) {
                        double2 f[2][D];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int k = kb + q * IMP_T;
                            const double2* ph = gp + (int64_t)(k < n ? k : 0) * D;
#pragma unroll
                            for (int s2 = 0; s2 < D; ++s2) f[q][s2] = ph[s2];
                        }
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int k = kb + q * IMP_T;
                            if (k < n) {
                                double pk = 0.0;
#pragma unroll
                                for (int s_ = 0; s_ < D; ++s_) {
                                    double qr = 0.0, qi = 0.0;
#pragma unroll
                                    for (int s2 = 0; s2 < D; ++s2) {
                                        const double ar = rho[s_ * IMP_MAXD + s2], ai = rhoi[s_ * IMP_MAXD + s2];
                                        qr = fma(ar, f[q][s2].x, qr);
                                        qr = fma(-ai, f[q][s2].y, qr);
                                        qi = fma(ar, f[q][s2].y, qi);
                                        qi = fma(ai, f[q][s2].x, qi);
                                    }
                                    pk = fma(qr, qr, pk);
                                    pk = fma(qi, qi, pk);
                                }
                                p[k] = pk;
                                if (pk > pmax) {
                                    pmax = pk;
                                    kmax = k;
                                }
                            }
                        }
                    }
                };
                switch (d) {
                    case 2: evalc(std::integral_constant<int, 2>{}); break;
                    case 3: evalc(std::integral_constant<int, 3>{}); break;
                    case 4: evalc(std::integral_constant<int, 4>{}); break;
                    case 5: evalc(std::integral_constant<int, 5>{}); break;
                    case 6: evalc(std::integral_constant<int, 6>{}); break;
                    case 7: evalc(std::integral_constant<int, 7>{}); break;
                    case 8: evalc(std::integral_constant<int, 8>{}); break;
                    case 10: evalc(std::integral_constant<int, 10>{}); break;
                    case 12: evalc(std::integral_constant<int, 12>{}); break;
                    case 14: evalc(std::integral_constant<int, 14>{}); break;
                    case 16: evalc(std::integral_constant<int, 16>{}); break;
                    default:
                        for (int k = tid; k < n; k += IMP_T) {
                            const double2* ph = gp + (int64_t)k * d;
                            double pk = 0.0;
                            for (int s_ = 0; s_ < d; ++s_) {
                                double qr = 0.0, qi = 0.0;
                                for (int s2 = 0; s2 < d; ++s2) {
                                    const double ar = rho[s_ * IMP_MAXD + s2], ai = rhoi[s_ * IMP_MAXD + s2];
                                    const double2 fv = ph[s2];
                                    qr = fma(ar, fv.x, qr);
                                    qr = fma(-ai, fv.y, qr);
                                    qi = fma(ar, fv.y, qi);
                                    qi = fma(ai, fv.x, qi);
                                }
                                pk = fma(qr, qr, pk);
                                pk = fma(qi, qi, pk);
                            }
                            p[k] = pk;
                            if (pk > pmax) {
                                pmax = pk;
                                kmax = k;
                            }
                        }
                }
            } else {
                auto eval = [&](auto DD) {
                    constexpr int D = decltype(DD)::value;
                    constexpr int Q = D <= 4 ? 4 : (D <= 8 ? 2 : 1);       // grid values per batch of loads (d > 8: one - the batch is 2 d registers)
                    constexpr int DR = D <= 4 ? D : 1;                     // rho in registers for d <= 4, else read from LDS
                    double rr[DR * DR];                                    // (every lane reads the same entry: a broadcast)
#pragma unroll
                    for (int e = 0; e < DR * DR; ++e) rr[e] = rho[(e / DR) * IMP_MAXD + (e % DR)];
                    double fa[Q][D], fb[Q][D];                             // two batches: one in flight while the other is consumed
                    const double* gphi = g.grid_phi + (int64_t)j * g.grid_site_stride;      // site j's table (stride 0: the shared one)
                    auto loadf = [&](double (&f)[Q][D], int kb) {
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            const int k = kb + q * IMP_T;
                            const double* ph = gphi + (int64_t)(k < n ? k : 0) * D;
#pragma unroll
                            for (int s2 = 0; s2 < D; ++s2) f[q][s2] = ph[s2];
                        }
                    };
                    auto consume = [&](const double (&f)[Q][D], int kb) {
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            const int k = kb + q * IMP_T;
                            if (k < n) {
                                double pk = 0.0;
#pragma unroll
                                for (int s_ = 0; s_ < D; ++s_) {
                                    double qq = 0.0;
#pragma unroll
                                    for (int s2 = 0; s2 < D; ++s2) qq = fma(D <= 4 ? rr[(s_ * DR + s2) % (DR * DR)] : rho[s_ * IMP_MAXD + s2], f[q][s2], qq);
                                    pk = fma(qq, qq, pk);
                                }
                                p[k] = pk;
                                if (pk > pmax) {      // strictly greater: within a thread k increases, so this keeps the first maximum
                                    pmax = pk;
                                    kmax = k;
                                }
                            }
                        }
                    };
                    loadf(fa, tid);
                    for (int kb = tid; kb < n; kb += 2 * Q * IMP_T) {
                        loadf(fb, kb + Q * IMP_T);
                        consume(fa, kb);
                        loadf(fa, kb + 2 * Q * IMP_T);
                        consume(fb, kb + Q * IMP_T);
                    }
                };
                switch (d) {
                    case 2: eval(std::integral_constant<int, 2>{}); break;
                    case 3: eval(std::integral_constant<int, 3>{}); break;
                    case 4: eval(std::integral_constant<int, 4>{}); break;
                    case 5: eval(std::integral_constant<int, 5>{}); break;
                    case 6: eval(std::integral_constant<int, 6>{}); break;
                    case 7: eval(std::integral_constant<int, 7>{}); break;
                    case 8: eval(std::integral_constant<int, 8>{}); break;
                    // (the reference's imputation examples use Legendre d = 10 ... 12: the generic loop below is 10-100x slower)
                    case 9: eval(std::integral_constant<int, 9>{}); break;
                    case 10: eval(std::integral_constant<int, 10>{}); break;
                    case 11: eval(std::integral_constant<int, 11>{}); break;
                    case 12: eval(std::integral_constant<int, 12>{}); break;
                    case 13: eval(std::integral_constant<int, 13>{}); break;
                    case 14: eval(std::integral_constant<int, 14>{}); break;
                    case 15: eval(std::integral_constant<int, 15>{}); break;
                    case 16: eval(std::integral_constant<int, 16>{}); break;
                    default:
                        for (int k = tid; k < n; k += IMP_T) {
                            const double* ph = g.grid_phi + (int64_t)j * g.grid_site_stride + (int64_t)k * d;
                            double pk = 0.0;
                            for (int s_ = 0; s_ < d; ++s_) {
                                double q = 0.0;
                                for (int s2 = 0; s2 < d; ++s2) q = fma(rho[s_ * IMP_MAXD + s2], ph[s2], q);
                                pk = fma(q, q, pk);
                            }
                            p[k] = pk;
                            if (pk > pmax) {
                                pmax = pk;
                                kmax = k;
                            }
                        }
                }
            }
            __threadfence_block();
            __syncthreads();
            grid_prefix_sums(p, S, n, nrow, rpw, wtot);
            __threadfence_block();
            __syncthreads();
            }
            const double woff1 = wtot[0], woff2 = woff1 + wtot[1], woff3 = woff2 + wtot[2];
            const GridSums tab{S, quarter, woff1, woff2, woff3};
            auto Sabs = [&](int k) {
                if constexpr (TRIG) return den.S(k);
                else return tab.at(k);
            };
            auto Pat = [&](int k) {
                if constexpr (TRIG) return den.P(g.grid_x[k]);
                else return p[k];
            };
            double Stot;
            if constexpr (TRIG) Stot = den.S(n - 1);
            else Stot = woff3 + wtot[3];
            const double p0 = Pat(0);
            if constexpr (TRIG) den.p0 = p0;
            auto cdf_at = [&](int k) {                                               // cumulative trapezoid
                if constexpr (TRIG) return den.cdf(k);
                else return grid_cdf_at(k, dx, p0, Sabs);
            };
            const double Z = cdf_at(n - 1);
            // ---- this kernel's searches: block-wide, written once for this kernel and k_sc_grid (grid_* above) ----
            auto arg_pmax = [&](double& gmax) {
                // TRIG: the maximum over the grid, only where a method needs it (mode; the WMAD's one-weight-above-half rule)
                if constexpr (TRIG)
                    for (int k = tid; k < n; k += IMP_T) {
                        const double pk = den.P(g.grid_x[k]);
                        if (pk > pmax) {
                            pmax = pk;
                            kmax = k;
                        }
                    }
                return grid_arg_pmax(pmax, kmax, n, red, isel, gmax);
            };
            auto quantile = [&](double target) { return grid_quantile(target, Z, n, nrow, isel, cdf_at); };
            int jtip_unused;
            auto wmad = [&](int kc) {
                return grid_wmad(kc, g.grid_x, Stot, Z, n, nrow, isel, Sabs, [&](double mid, int& km) {
                    // (TRIG: no grid value can outweigh half the total unless the bound c_0 + sum |c_m| does - never on a fine grid)
                    if constexpr (TRIG)
                        if (!(den.tbound / Z > mid)) return false;
                    double gm;
                    km = arg_pmax(gm);
                    return gm / Z > mid;
                }, jtip_unused);
            };
            // the two grid moments of the mean, eight grid values per thread in flight
            auto sum_xp = [&]() {
                double a = 0.0;
                for (int kb = tid; kb < n; kb += 8 * IMP_T) {
                    double t[8], xx[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int k = kb + q * IMP_T;
                        t[q] = k < n ? Pat(k) : 0.0;
                        xx[q] = k < n ? g.grid_x[k] : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) a = fma(xx[q], t[q], a);
                }
                a = blk_sum(a, red);
                __syncthreads();
                return a;
            };
            auto sum_dev2p = [&](double ex) {
                double b2 = 0.0;
                for (int kb = tid; kb < n; kb += 8 * IMP_T) {
                    double t[8], xx[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int k = kb + q * IMP_T;
                        t[q] = k < n ? Pat(k) : 0.0;
                        xx[q] = k < n ? g.grid_x[k] : ex;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) b2 = fma((xx[q] - ex) * (xx[q] - ex), t[q], b2);
                }
                b2 = blk_sum(b2, red);
                __syncthreads();
                return b2;
            };
            auto set_state = [&](int k, double re, double im) {
                ms.r[k] = (R)re;
                if constexpr (CX) ms.i[k] = (R)im;
            };
            // ---- select by g.method ------------------------------------------------------------------------------------------------
            int ksel = 0;
            double xsel = 0.0, err = 0.0;
            bool state_from_grid = true;
            if (g.method == IMP_MODE) {
                double gm;
                ksel = arg_pmax(gm);                                         // get_mode_from_rdm, sampling_utils.jl:98-143
            } else if (g.method == IMP_MEDIAN) {
                ksel = quantile(0.5);                                        // get_median_from_rdm, :159-196
                if (g.get_wmad) err = wmad(ksel);
                if constexpr (DIST) {
                    // the levels: the median's search once more per level on the density that is already there; the chain is
                    // conditioned on the median alone
                    for (int l = 0; l < g.nq; ++l) {
                        const int kl = quantile(lev[l]);
                        if (tid == 0) g.q_out[(ch.row * T + j) * g.nq + l] = g.grid_x[kl];
                    }
                    // the cdf (cdf /= cdf[end], sampling_utils.jl:205-241) at every cdf_stride-th grid index and the last one, one pass,
                    // consecutive threads store consecutive doubles.  Row = the site's rank among the instance's missing sites in
                    // ascending order (cdfs[i] by position, MPS_methods.jl:413), whatever the direction of the sweep.
                    if (g.cdf_stride > 0) {
                        const int row = g.rev ? nm - seen : seen - 1;
                        double* co_ = g.cdf_out + ((int64_t)ch.rslot * g.cdf_rows + row) * g.ncdf;       // (staged per block: the chain's slot)
                        for (int m = tid; m < g.ncdf; m += IMP_T) {
                            const int k = m == g.ncdf - 1 ? n - 1 : m * g.cdf_stride;
                            co_[m] = cdf_at(k) / Z;
                        }
                    }
                }
            } else if (g.method == IMP_QUANTILE) {
                ksel = quantile(imp_uniform(g, ch, T, j, 0));               // get_sample_from_rdm without rejection, :262-270
            } else if (g.method == IMP_ITS_REJECT) {
                // get_sample_from_rdm with a rejection threshold (:271-290): median and WMAD first, then up to max_trials
                // inverse-transform samples, the first within threshold * WMAD of the median is kept (else the last drawn)
                const int kmed = quantile(0.5);
                const double w = wmad(kmed);
                const double xm = g.grid_x[kmed];
                ksel = kmed;
                for (int t = 0; t < g.ntrial; ++t) {
                    ksel = quantile(imp_uniform(g, ch, T, j, t));
                    if (fabs(g.grid_x[ksel] - xm) < g.reject_thr * w) break;
                }
                err = w;
            } else {
                // get_mean_from_rdm (:60-96): E[x] = sum x p dx / Z, std from the same sums; the conditioning state is the
                // encoding of E[x] itself, which is not a grid value
                const double dxm = (g.grid_x[n - 1] - g.grid_x[0]) / (double)(n - 1);
                const double ex = sum_xp() * dxm / Z;
                if (g.get_wmad) err = sqrt(sum_dev2p(ex) * dxm / Z);
                xsel = ex;
                state_from_grid = false;
                if (tid == 0) imp_mean_state(g.mean_basis, ex, d, set_state);
            }
            if (state_from_grid) {
                xsel = g.grid_x[ksel];
                if (tid < d) {
                    const double* gsel = g.grid_phi + (int64_t)j * g.grid_site_stride;      // site j's table (stride 0: the shared one)
                    const int64_t e = ((int64_t)ksel * d + tid) * ZW;
                    set_state(tid, gsel[e], CX ? gsel[e + 1] : 0.0);
                }
            }
            if (tid == 0) {
                g.x_out[ch.row * T + j] = xsel;
                g.err_out[ch.row * T + j] = err;
            }
            __syncthreads();
            imp_project<R, CX>(LW, Ln, d, Do, cm, [&](int q, R& pr, R& pi) {
                pr = ms.r[q];
                pi = CX ? ms.i[q] : R(0);
            });
            if (seen == nm) break;             // nothing beyond the last missing site is needed
        }
        __syncthreads();
        imp_rescale<R, CX>(L, Ln, Do, red);
    }
}

#include "mpst_impute_batched.inl"
#include "mpst_marginal.inl"
#include "mpst_sitecond.inl"
#include "mpst_window.inl"
#include "mpst_margcond.inl"
#include "mpst_observed.inl"
#include "mpst_prefix.inl"
#include "mpst_segment.inl"
#include "mpst_rolling.inl"

static size_t right_lds_bytes(int cap, bool cx, bool f32) {
    const int cp = (cap + 15) & ~15;
    return (size_t)(cx ? 2 : 1) * 4 * cp * (cp + (f32 ? 4 : 2)) * (f32 ? 4 : 8);
}
static size_t left_lds_bytes(int cap, bool cx, bool f32) {
    return (size_t)(2 * cap + 2 * IMP_MAXD * cap + IMP_MAXD) * (cx ? 2 : 1) * (f32 ? 4 : 8);
}
// the LDS kernel's limit; beyond it (or everywhere with MPST_IMPUTE_BIG=1, a test hook): k_imp_right_big
static int impute_lds_chi_limit(bool cx, bool f32) {
    static const bool force = getenv("MPST_IMPUTE_BIG") != nullptr;
    return force ? 0 : ((cx && !f32) ? 48 : 64);     // complex fp64 above 48: one workgroup per CU in LDS loses to the global-scratch kernel (measured)
}
int impute_chi_limit(bool, bool) { return CAP_LIMIT; }
int64_t impute_work_elems(int cap, bool cx, bool f32) { return cap > impute_lds_chi_limit(cx, f32) ? 4ll * cap * cap * (cx ? 2 : 1) : 0; }
int64_t marginal_work_elems(int cap, bool cx, bool f32) { return cap > impute_lds_chi_limit(cx, f32) ? (int64_t)MRG_BIG_MATS * cap * cap * (cx ? 2 : 1) : 0; }
// window conditionals keep three of the environment pass's four matrices in LDS (E, the site matrix, T1)
static size_t window_lds_bytes(int cap, bool cx) { return right_lds_bytes(cap, cx, false) / 4 * 3; }
bool window_big_route(int cap, bool cx) { return cap > impute_lds_chi_limit(cx, false); }
// marginal site conditionals keep the environment pass's four matrices in LDS (L, the site matrix, K_s, R)
bool margcond_big_route(int cap, bool cx) { return cap > impute_lds_chi_limit(cx, false); }
// the prefix marginals' recursion keeps three of them (E, the site matrix, T1)
static size_t prefix_env_lds_bytes(int cap, bool cx) { return right_lds_bytes(cap, cx, false) / 4 * 3; }
bool prefix_big_route(int cap, bool cx) { return cap > impute_lds_chi_limit(cx, false); }

// ---- the route of a call: which kernels, at which block size / occupancy / dynamic LDS -----------------------------------
struct ImputeSwitches {
    int force_occ;              // MPST_IMP_OCC=1|2|4 (read once, a lab switch): the occupancy of the plain one-chain kernels, no batched sweep
    bool no_batch;              // MPST_IMP_NO_BATCH=1 (every call, a test hook): the one-chain kernel where the batched sweep would run
    bool cdf_batch;             // MPST_IMP_DIST_CDF_BATCH=1 (every call): a call with a cdf stays in the batched sweep
};
static ImputeSwitches impute_switches() {
    static const int force_occ = [] { const char* e = getenv("MPST_IMP_OCC"); return e ? atoi(e) : 0; }();
    return ImputeSwitches{force_occ, getenv("MPST_IMP_NO_BATCH") != nullptr, getenv("MPST_IMP_DIST_CDF_BATCH") != nullptr};
}
struct ImputeRoute {
    bool env_big;               // environment pass: k_imp_right_big (global scratch), else k_imp_right in LDS
    int env_threads;            // ... with that many threads
    size_t env_lds;
    bool batched, emb;          // sweep: k_imp_leftb<EMB>, sixteen chains per workgroup, else k_imp_left, a workgroup per chain
    int occ;                    // ... built for that many workgroups per CU
    bool trig, dist;            // k_imp_left<TRIG, DIST>, k_imp_leftb<DIST> (which only runs on closed-form grids)
    size_t lds;                 // dynamic LDS of the sweep kernel
};
static ImputeRoute impute_route(const ImpModel& v, const ImputeParams& q, const ImputeSwitches& sw) {
    const bool CX = v.is_complex != 0, F32 = v.compute_f32 != 0;
    ImputeRoute r{};
    r.env_big = v.cap > impute_lds_chi_limit(CX, F32);
    // a wave per 16 x 16 tile: 16, 9 (on 8 waves), 4 or 1 tiles
    const int tpr = (v.cap + 15) >> 4;
    r.env_threads = tpr >= 4 ? 1024 : (tpr == 3 ? 512 : 256);
    r.env_lds = r.env_big ? 0 : right_lds_bytes(v.cap, CX, F32);
    r.trig = q.trig != 0;
    const bool mean_ok = q.g.method != IMP_MEAN || (CX ? q.g.mean_basis == IMP_BASIS_FOURIER
                                                       : (q.g.mean_basis == IMP_BASIS_LEGENDRE || q.g.mean_basis == IMP_BASIS_LEGENDRE_NO_NORM ||
                                                          q.g.mean_basis == IMP_BASIS_UNIFORM));
    // the distribution outputs (mpst_impute_dist with levels or a cdf): the DIST instantiations, on the routes the plain median takes.
    // A call with a cdf leaves the batched sweep - there a wave's 20 001-point store would hold up the fifteen other chains of its
    // workgroup (A/B in DESIGN 16; MPST_IMP_DIST_CDF_BATCH=1 keeps it there, the losing variant of that A/B)
    r.dist = q.g.nq > 0 || q.g.cdf_stride > 0;
    const bool batch_ok = !r.dist || q.g.cdf_stride == 0 || sw.cdf_batch;
    // closed-form densities: sixteen instances per workgroup
    if (r.trig && !sw.no_batch && sw.force_occ == 0 && mean_ok && batch_ok && imb_fits(v.cap, v.d, CX, F32)) {
        r.batched = true;
        r.emb = CX && v.d <= 8;
        r.lds = imb_layout(v.cap, v.d, CX, F32).bytes;
        return r;
    }
    // Legendre states on a uniform grid (closed form, real models): the linearisation table rides in LDS behind the panels
    r.lds = left_lds_bytes(v.cap, CX, F32) + ((r.trig && !CX) ? (size_t)(2 * v.d - 1) * v.d * v.d * sizeof(double) : 0);
    // (the distribution kernels run at the occupancy their route has by default; MPST_IMP_OCC is a lab switch of the plain kernels)
    const int forced = r.dist ? 0 : sw.force_occ;
    if (r.trig) {
        // closed-form densities: no density loop, so no reason to keep the whole register file for one workgroup
        // complex models, three workgroups per CU (170 VGPRs): same-box A/B at configs[4] with 16 / 8 loads per output in flight:
        // OCC 2: 83.5 / 148 ms, OCC 3: 76.2 / 97 ms, OCC 4 (spilling): 121 / 102 ms
        // (real models, three workgroups per CU: d = 4, chi = 32: 15.9 / 14.6 / 13.3 ms at 1 / 2 / 3; d = 12, chi = 40: 27.5 / 27.6 / 26.6)
        r.occ = (forced == 1 || forced == 2 || (forced == 4 && CX)) ? forced : 3;
        return r;
    }
    // two workgroups per CU (128 VGPRs each, 70-183 of them spilled) against one (256 VGPRs, no spill): the spilling
    // build wins where the density loop is latency-bound - real models and complex ones with d <= 5 - because a second
    // workgroup hides more than the scratch traffic costs (same-box A/B: profiles/r03_impute_occupancy_ab.txt;
    // MPST_IMP_OCC=1|2 forces either)
    // (real models with d > 8 - the reference's imputation examples use Legendre d = 10 ... 12 - likewise: d = 12, chi = 40: 147 ms with
    // two spilling workgroups per CU, 44 ms with one; 774 ms before the density loop had unrolled forms beyond d = 8)
    r.occ = (forced == 1 || forced == 2) ? forced : (((CX && v.d > 5) || (!CX && v.d > 8)) ? 1 : 2);
    return r;
}

// ---- from the route to the launch ------------------------------------------------------------------------------------------------
// Every instantiation a route can name stands in one of the three lists below, once.  imp_raise_lds expands them to raise each
// entry's dynamic-LDS limit to the most it can be launched with, imp_env / imp_sweep expand them to launch the entry the route
// names - so what can be launched cannot lack its attribute.
// WHEN is the compile-time condition on the model's type (the complex-only variants are not built for real models).
#define IMP_RIGHT_LIST(X) X(256) X(512) X(1024)
#define IMP_LEFT_LIST(X) /* WHEN, OCC, TRIG, DIST */                                                                               \
    X(true, 1, false, false) X(true, 2, false, false) X(true, 1, false, true) X(true, 2, false, true)                               \
    X(true, 1, true, false) X(true, 2, true, false) X(true, 3, true, false) X(CX, 4, true, false) X(true, 3, true, true)
#define IMP_LEFTB_LIST(X) /* WHEN, EMB, DIST */ X(true, false, false) X(CX, true, false) X(true, false, true) X(CX, true, true)

template <typename R, bool CX>
static hipError_t imp_raise_lds() {
    constexpr bool F32 = std::is_same<R, float>::value;
    const size_t right_max = right_lds_bytes(impute_lds_chi_limit(CX, F32), CX, F32), left_max = left_lds_bytes(CAP_LIMIT, CX, F32);
    const size_t table_max = CX ? 0 : (2 * IMP_MAXD - 1) * IMP_MAXD * IMP_MAXD * sizeof(double);
#define RAISE(KERNEL, BYTES)                                                                                                        \
    if (hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES)); e != hipSuccess) return e;
#define X(BS) RAISE((k_imp_right<R, CX, BS>), right_max)
    IMP_RIGHT_LIST(X)
#undef X
#define X(WHEN, OCC, TRIG, DIST) if constexpr (WHEN) { RAISE((k_imp_left<R, CX, OCC, TRIG, DIST>), left_max + (TRIG ? table_max : 0)) }
    IMP_LEFT_LIST(X)
#undef X
#define X(WHEN, EMB, DIST) if constexpr (WHEN) { RAISE((k_imp_leftb<R, CX, EMB, DIST>), IMB_LDS_MAX) }
    IMP_LEFTB_LIST(X)
#undef X
    RAISE((k_marginal<R, CX, false>), right_max)      // the environment pass's matrices and limit
#undef RAISE
    return hipSuccess;
}

hipError_t impute_init_attrs(int device) {
    static std::atomic<unsigned long long> done{0};
    if (device >= 0 && device < 64 && (done.load(std::memory_order_acquire) >> device) & 1ull) return hipSuccess;
    for (hipError_t e : {imp_raise_lds<double, false>(), imp_raise_lds<double, true>(), imp_raise_lds<float, false>(), imp_raise_lds<float, true>()})
        if (e != hipSuccess) return e;
    for (hipError_t e : {hipFuncSetAttribute((const void*)k_win<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)window_lds_bytes(impute_lds_chi_limit(false, false), false)),
                         hipFuncSetAttribute((const void*)k_win<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)window_lds_bytes(impute_lds_chi_limit(true, false), true))})
        if (e != hipSuccess) return e;
    for (hipError_t e : {hipFuncSetAttribute((const void*)k_mc_walk<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(false, false), false, false)),
                         hipFuncSetAttribute((const void*)k_mc_walk<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(true, false), true, false))})
        if (e != hipSuccess) return e;
    for (hipError_t e : {hipFuncSetAttribute((const void*)k_obs_walk<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(false, false), false, false)),
                         hipFuncSetAttribute((const void*)k_obs_walk<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(true, false), true, false))})
        if (e != hipSuccess) return e;
    for (hipError_t e : {hipFuncSetAttribute((const void*)k_prefix_env<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)prefix_env_lds_bytes(impute_lds_chi_limit(false, false), false)),
                         hipFuncSetAttribute((const void*)k_prefix_env<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)prefix_env_lds_bytes(impute_lds_chi_limit(true, false), true))})
        if (e != hipSuccess) return e;
    // segment marginals: the left table keeps the prefix recursion's three matrices, the walk the environment pass's four
    for (hipError_t e : {hipFuncSetAttribute((const void*)k_segment_left<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)prefix_env_lds_bytes(impute_lds_chi_limit(false, false), false)),
                         hipFuncSetAttribute((const void*)k_segment_left<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)prefix_env_lds_bytes(impute_lds_chi_limit(true, false), true)),
                         hipFuncSetAttribute((const void*)k_segment_walk<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(false, false), false, false)),
                         hipFuncSetAttribute((const void*)k_segment_walk<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)right_lds_bytes(impute_lds_chi_limit(true, false), true, false))})
        if (e != hipSuccess) return e;
    if (device >= 0 && device < 64) done.fetch_or(1ull << device, std::memory_order_release);
    return hipSuccess;
}

// the instances order[i0 .. i0 + count) on a stream, an event between the two kernels
struct ImputeChunk { int64_t i0, count; hipStream_t s; hipEvent_t mid; };

template <typename R, bool CX>
static hipError_t imp_env(const ImputeRoute& rt, const ImpModel& v, const ImputeParams& q, const ImputeChunk& ch) {
    const dim3 grid((unsigned)ch.count);
    if (rt.env_big) {
        hipLaunchKernelGGL((k_imp_right_big<R, CX>), grid, dim3(IMP_T), 0, ch.s, v, q.g.missing, (R*)q.g.Rbuf, (R*)q.work, q.g.max_missing,
                           q.order + ch.i0, q.g.rev);
        return hipSuccess;
    }
#define X(BS)                                                                                                                       \
    if (rt.env_threads == BS) {                                                                                                     \
        hipLaunchKernelGGL((k_imp_right<R, CX, BS>), grid, dim3(BS), rt.env_lds, ch.s, v, q.g.missing, (R*)q.g.Rbuf, q.g.max_missing, \
                           q.order + ch.i0, q.g.rev);                                                                               \
        return hipSuccess;                                                                                                          \
    }
    IMP_RIGHT_LIST(X)
#undef X
    return hipErrorInvalidValue;
}

template <typename R, bool CX>
static hipError_t imp_sweep(const ImputeRoute& rt, const ImpModel& v, const ImpArgs& g, const ImputeChunk& ch) {
    // the environment pass ran once per instance; the sweep runs once per chain (ntraj adjacent chains per instance)
    const int64_t nchain = ch.count * g.ntraj;
#define X(WHEN, OCC, TRIG, DIST)                                                                                                    \
    if constexpr (WHEN) {                                                                                                           \
        if (!rt.batched && rt.occ == OCC && rt.trig == TRIG && rt.dist == DIST) {                                                   \
            hipLaunchKernelGGL((k_imp_left<R, CX, OCC, TRIG, DIST>), dim3((unsigned)nchain), dim3(IMP_T), rt.lds, ch.s, v, g);     \
            return hipSuccess;                                                                                                      \
        }                                                                                                                           \
    }
    IMP_LEFT_LIST(X)
#undef X
#define X(WHEN, EMB, DIST)                                                                                                          \
    if constexpr (WHEN) {                                                                                                           \
        if (rt.batched && rt.emb == EMB && rt.dist == DIST) {                                                                       \
            hipLaunchKernelGGL((k_imp_leftb<R, CX, EMB, DIST>), dim3((unsigned)((nchain + IMB_B - 1) / IMB_B)), dim3(IMB_T), rt.lds, ch.s, \
                               v, g, (int)nchain);                                                                                  \
            return hipSuccess;                                                                                                      \
        }                                                                                                                           \
    }
    IMP_LEFTB_LIST(X)
#undef X
    return hipErrorInvalidValue;
}

// both kernels of a chunk
template <typename R, bool CX>
static hipError_t imp_run(const ImputeRoute& rt, const ImpModel& v, const ImputeParams& q, const ImputeChunk& ch) {
    if (hipError_t e = imp_env<R, CX>(rt, v, q, ch); e != hipSuccess) return e;
    if (ch.mid) (void)hipEventRecord(ch.mid, ch.s);
    ImpArgs g = q.g;
    g.ord = q.order + ch.i0;
#ifdef MPST_LAB
    // lab builds only (make EXTRA=-DMPST_LAB): MPST_IMB_DBG switches parts of k_imp_leftb off for timing - results are then
    // WRONG by construction, so the shipped library never reads the variable
    static const int imb_dbg = [] { const char* e = getenv("MPST_IMB_DBG"); return e ? atoi(e) : 0; }();
    g.dbg = imb_dbg;
#endif
    return imp_sweep<R, CX>(rt, v, g, ch);
}

int launch_impute(const ImpModel& v, const ImputeParams& q, int64_t i0, int64_t count, hipStream_t s, hipEvent_t mid) {
    const ImputeRoute rt = impute_route(v, q, impute_switches());
    const ImputeChunk ch{i0, count, s, mid};
    const hipError_t e = v.is_complex ? (v.compute_f32 ? imp_run<float, true>(rt, v, q, ch) : imp_run<double, true>(rt, v, q, ch))
                                      : (v.compute_f32 ? imp_run<float, false>(rt, v, q, ch) : imp_run<double, false>(rt, v, q, ch));
    return e == hipSuccess ? (rt.batched ? 1 : 0) : -1;
}

// the marginal likelihoods of the instances order[i0 .. i0 + count): the environment pass's route (LDS or global scratch), one kernel
template <typename R, bool CX>
static hipError_t marg_run(const ImputeRoute& rt, const ImpModel& v, const ImputeParams& q, const ImputeChunk& ch) {
    ImpArgs g = q.g;
    g.ord = q.order + ch.i0;
    const dim3 grid((unsigned)ch.count);
    if (rt.env_big) hipLaunchKernelGGL((k_marginal<R, CX, true>), grid, dim3(IMP_T), 0, ch.s, v, g, q.nclass, (R*)q.work);
    else hipLaunchKernelGGL((k_marginal<R, CX, false>), grid, dim3(IMP_T), rt.env_lds, ch.s, v, g, q.nclass, (R*)nullptr);
    return hipGetLastError();
}

int launch_marginal(const ImpModel& v, const ImputeParams& q, int64_t i0, int64_t count, hipStream_t s) {
    const ImputeRoute rt = impute_route(v, q, impute_switches());
    const ImputeChunk ch{i0, count, s, nullptr};
    const hipError_t e = v.is_complex ? (v.compute_f32 ? marg_run<float, true>(rt, v, q, ch) : marg_run<double, true>(rt, v, q, ch))
                                      : (v.compute_f32 ? marg_run<float, false>(rt, v, q, ch) : marg_run<double, false>(rt, v, q, ch));
    return e == hipSuccess ? 0 : -1;
}
// leave-one-out site conditionals of a chunk: the walk, sixteen instances per workgroup, then the grid phase, a workgroup per
// (instance, site) pair at a time
int launch_sitecond(const ImpModel& v, const ScArgs& g, hipStream_t s, hipEvent_t mid) {
    const dim3 wgrid((unsigned)((g.count + SC_B - 1) / SC_B)), ggrid((unsigned)sitecond_grid_workgroups(g.count * v.T));
    if (v.is_complex) hipLaunchKernelGGL((k_sc_walk<true>), wgrid, dim3(SC_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_sc_walk<false>), wgrid, dim3(SC_T), 0, s, v, g);
    if (hipGetLastError() != hipSuccess) return -1;
    if (mid) (void)hipEventRecord(mid, s);
    if (v.is_complex) hipLaunchKernelGGL((k_sc_grid<true>), ggrid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_sc_grid<false>), ggrid, dim3(IMP_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// window conditionals of a chunk: the walk that keeps both rows, sixteen instances per workgroup, then the window kernel, a workgroup
// per (instance, start) pair at a time
int launch_window(const ImpModel& v, const WinArgs& g, int64_t walk_wgs, int64_t win_wgs, hipStream_t s, hipEvent_t mid) {
    const dim3 wgrid((unsigned)walk_wgs), kgrid((unsigned)win_wgs);
    if (v.is_complex) hipLaunchKernelGGL((k_win_walk<true>), wgrid, dim3(SC_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_win_walk<false>), wgrid, dim3(SC_T), 0, s, v, g);
    if (hipGetLastError() != hipSuccess) return -1;
    if (mid) (void)hipEventRecord(mid, s);
    const bool big = window_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : window_lds_bytes(v.cap, v.is_complex != 0);
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_win<true, true>), kgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_win<true, false>), kgrid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_win<false, true>), kgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_win<false, false>), kgrid, dim3(IMP_T), lds, s, v, g);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// marginal site conditionals of a chunk: the walk, a workgroup per instance, then the grid phase, a workgroup per (instance, site) pair
// at a time
int launch_margcond(const ImpModel& v, const McArgs& g, int64_t grid_wgs, hipStream_t s, hipEvent_t mid) {
    const dim3 wgrid((unsigned)g.count), ggrid((unsigned)grid_wgs);
    const bool big = margcond_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : right_lds_bytes(v.cap, v.is_complex != 0, false);
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_mc_walk<true, true>), wgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_mc_walk<true, false>), wgrid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_mc_walk<false, true>), wgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_mc_walk<false, false>), wgrid, dim3(IMP_T), lds, s, v, g);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    if (mid) (void)hipEventRecord(mid, s);
    if (v.is_complex) hipLaunchKernelGGL((k_mc_grid<true>), ggrid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_mc_grid<false>), ggrid, dim3(IMP_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// observed conditionals of a chunk: the operators of its soft sites, the walk (a workgroup per instance), an event, and - with `grid` -
// the grid phase, a workgroup per (instance, site) pair at a time
int launch_observed(const ImpModel& v, const ObsArgs& g, int64_t grid_wgs, bool grid, hipStream_t s, hipEvent_t mid) {
    const dim3 wgrid((unsigned)g.count), ggrid((unsigned)grid_wgs);
    const bool big = margcond_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : right_lds_bytes(v.cap, v.is_complex != 0, false);
    if (v.is_complex) hipLaunchKernelGGL((k_obs_operator<true>), ggrid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_obs_operator<false>), ggrid, dim3(IMP_T), 0, s, v, g);
    if (hipGetLastError() != hipSuccess) return -1;
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_obs_walk<true, true>), wgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_obs_walk<true, false>), wgrid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_obs_walk<false, true>), wgrid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_obs_walk<false, false>), wgrid, dim3(IMP_T), lds, s, v, g);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    if (mid) (void)hipEventRecord(mid, s);
    if (!grid) return 0;
    if (v.is_complex) hipLaunchKernelGGL((k_obs_grid<true>), ggrid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_obs_grid<false>), ggrid, dim3(IMP_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// prefix marginals: the tables of the model, a workgroup per class
int launch_prefix_env(const ImpModel& v, const PrefixArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)g.C);
    const bool big = prefix_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : prefix_env_lds_bytes(v.cap, v.is_complex != 0);
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_prefix_env<true, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_prefix_env<true, false>), grid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_prefix_env<false, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_prefix_env<false, false>), grid, dim3(IMP_T), lds, s, v, g);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ... and the walk of a chunk with its scores, sixteen instances per workgroup
int launch_prefix_score(const ImpModel& v, const PrefixArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)((g.count + SC_B - 1) / SC_B));
    if (v.is_complex) hipLaunchKernelGGL((k_prefix_score<true>), grid, dim3(SC_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_prefix_score<false>), grid, dim3(SC_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// segment marginals: the left table (k_segment_left) and the right one (k_prefix_env as it is, on a PrefixArgs of this call), a
// workgroup per class each
int launch_segment_tables(const ImpModel& v, const SegmentArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)g.C);
    const bool big = prefix_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : prefix_env_lds_bytes(v.cap, v.is_complex != 0);
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_segment_left<true, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_segment_left<true, false>), grid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_segment_left<false, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_segment_left<false, false>), grid, dim3(IMP_T), lds, s, v, g);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    PrefixArgs p{};
    p.G = g.G, p.lnG = g.lnG, p.work = g.work_right, p.C = g.C;
    return launch_prefix_env(v, p, s);
}
// ... and the walk of a chunk, a (series, start) item at a time on persistent workgroups
int launch_segment_walk(const ImpModel& v, const SegmentArgs& g, int64_t walk_wgs, hipStream_t s) {
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(walk_wgs, g.count * v.T)));
    const bool big = prefix_big_route(v.cap, v.is_complex != 0);
    const size_t lds = big ? 0 : right_lds_bytes(v.cap, v.is_complex != 0, false);
    if (v.is_complex) {
        if (big) hipLaunchKernelGGL((k_segment_walk<true, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_segment_walk<true, false>), grid, dim3(IMP_T), lds, s, v, g);
    } else {
        if (big) hipLaunchKernelGGL((k_segment_walk<false, true>), grid, dim3(IMP_T), 0, s, v, g);
        else hipLaunchKernelGGL((k_segment_walk<false, false>), grid, dim3(IMP_T), lds, s, v, g);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// rolling-origin forecasts: the rows of a chunk, sixteen series per workgroup
int launch_rolling_rows(const ImpModel& v, const RollingArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)((g.count + SC_B - 1) / SC_B));
    if (v.is_complex) hipLaunchKernelGGL((k_roll_rows<true>), grid, dim3(SC_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_roll_rows<false>), grid, dim3(SC_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ... the chains of a block of targets, then the score of every (tile, origin) against them
int launch_rolling_tables(const ImpModel& v, const RollingArgs& g, int64_t table_wgs, hipStream_t s) {
    const int64_t items = (int64_t)(g.u1 - g.u0) * g.C * rolling_pairs(v.d);
    const dim3 tgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>(table_wgs, items)));
    const dim3 sgrid((unsigned)(((g.count + SC_B - 1) / SC_B) * v.T));
    if (v.is_complex) hipLaunchKernelGGL((k_roll_tables<true>), tgrid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_roll_tables<false>), tgrid, dim3(IMP_T), 0, s, v, g);
    if (hipGetLastError() != hipSuccess) return -1;
    if (v.is_complex) hipLaunchKernelGGL((k_roll_score<true>), sgrid, dim3(SC_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_roll_score<false>), sgrid, dim3(SC_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// ... and the grid phase of a chunk, a (series, origin, horizon) triple at a time
int launch_rolling_grid(const ImpModel& v, const RollingArgs& g, int64_t grid_wgs, hipStream_t s) {
    const dim3 grid((unsigned)grid_wgs);
    if (v.is_complex) hipLaunchKernelGGL((k_roll_grid<true>), grid, dim3(IMP_T), 0, s, v, g);
    else hipLaunchKernelGGL((k_roll_grid<false>), grid, dim3(IMP_T), 0, s, v, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace mpst
