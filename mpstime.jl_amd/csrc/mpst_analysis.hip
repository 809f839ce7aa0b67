// Entanglement analysis of a trained model (src/Analysis/analyse.jl): the bipartite entanglement entropy at every bond
// (bipartite_spectrum, :20-64), the single-site entropy at every site (single_site_spectrum, :69-138) and its variation
// when the first k sites are measured at an instance's values (see_variation, :168-194).
//
// Reformulation.  The reference orthogonalises and SVDs once per bond, and rebuilds, renormalises and
// re-orthogonalises a conditioned MPS for every (instance, k).  Here:
//   1. k_an_canon  brings each class MPS (label slice folded in) to right-canonical form ONCE: Householder LQ per site,
//                  right to left; the last factor's norm is dropped, so ||psi|| = 1.  Bonds may shrink to min(chi_l, d chi_r).
//   2. k_an_bvec   the measured boundary vector of every (instance, k): v_k = v_{k-1} sum_s phi_{k-1}(s) B_{k-1}^s,
//                  normalised at every step (a zero vector becomes NaN, as normalize! of a zero MPS does).
//   3. k_an_walk   with the block right of k right-orthonormal, row k of see_variation is the left density walk
//                      L_k = v_k v_k^T,  X^s = L_j B_j^s,  rho_j(s, s') = <B_j^s, X^s'>_F,  L_{j+1} = sum_s B_j^sT X^s
//                  over j = k..T-1; row 0 (v_0 = [1]) is single_site_spectrum.  One workgroup per chain, persistent over
//                  the chains, longest first.  The k = 0 walk of the entanglement call also keeps every L_j.
//   4. k_an_see    one thread per rho: cyclic Jacobi (eigenvalues only), rho_correct (:69-91), -sum lambda log lambda.
//   5. k_an_bee    eigenvalues of L_j (the Schmidt weights across bond j in this gauge: no SVD), one workgroup per bond,
//                  parallel-ordered Jacobi, -sum p log p over p > 1e-12 (:37-43).
// Real fp64 only, chi <= 128, d <= 16.  No trap or abort on the device: a DomainError of rho_correct is reported through a
// status word (the smallest failing flat index, atomicMin) and the offending value stored in place of the entropy.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "mpst_internal.h"

namespace mpst {
namespace {

constexpr int AN_THREADS = 256;
constexpr int AN_LDS_LD = 48;                  // leading dimension up to which the walk keeps L, X, L' in LDS (3 ld^2 doubles)
constexpr double AN_EIGTOL = 1.4901161193847656e-8;     // sqrt(eps()), rho_correct's default
constexpr int64_t AN_BLOCK_BYTES = 512ll << 20;         // densities + boundary vectors of one block of instances

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Site tensor j of class c at sites + (c T + j) S, element (l, s, r) at (l d + s) chi_r + r: row l of the chi_l x (d chi_r)
// matrix M_j is contiguous, and so is column l of A = M_j^T, which the Householder QR below factors in place.
__global__ __launch_bounds__(AN_THREADS) void k_an_canon(double* sites, int32_t* chi, int T, int d, int64_t S, double* work) {
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t* ch = chi + (int64_t)c * (T + 1);
    double* Qb = work + (int64_t)c * 2 * S;
    double* Fb = Qb + S;
    __shared__ double tau[128];
    __shared__ double red[AN_THREADS / 64];
    for (int j = T - 1; j >= 1; --j) {
        double* A = sites + ((int64_t)c * T + j) * S;
        const int n = ch[j], m = d * ch[j + 1], np = min(m, n);
        // A (m x n) = Q R; reflector l: v = [1, x(l+1:) * scal], H = I - t v v^T.  Every wave forms it (same data, same order:
        // same bits), applies it to its share of the trailing columns, and the column itself is overwritten after a barrier.
        for (int l = 0; l < np; ++l) {
            double* x = A + (int64_t)l * m;
            double ss = 0.0;
            for (int i = l + 1 + lane; i < m; i += 64) ss += x[i] * x[i];
            ss = wave_sum(ss);
            const double alpha = x[l];
            double beta = alpha, t = 0.0, scal = 0.0;
            if (ss > 0.0) {
                beta = -copysign(sqrt(alpha * alpha + ss), alpha);
                t = (beta - alpha) / beta;
                scal = 1.0 / (alpha - beta);
            }
            for (int cc = l + 1 + wv; cc < n; cc += AN_THREADS / 64) {
                double* y = A + (int64_t)cc * m;
                double p = 0.0;
                for (int i = l + 1 + lane; i < m; i += 64) p += x[i] * y[i];
                const double w = t * (y[l] + scal * wave_sum(p));
                const double ws = w * scal;
                for (int i = l + 1 + lane; i < m; i += 64) y[i] -= ws * x[i];
                if (lane == 0) y[l] -= w;
            }
            __syncthreads();
            for (int i = l + 1 + tid; i < m; i += AN_THREADS) x[i] *= scal;
            if (tid == 0) { x[l] = beta; tau[l] = t; }
            __syncthreads();
        }
        // Q (m x np, column-major) = H_0 ... H_{np-1} I, accumulated backwards
        for (int64_t e = tid; e < (int64_t)m * np; e += AN_THREADS) Qb[e] = (e % m == e / m) ? 1.0 : 0.0;
        __syncthreads();
        for (int l = np - 1; l >= 0; --l) {
            const double* v = A + (int64_t)l * m;
            const double t = tau[l];
            for (int cc = l + wv; cc < np; cc += AN_THREADS / 64) {
                double* y = Qb + (int64_t)cc * m;
                double p = 0.0;
                for (int i = l + 1 + lane; i < m; i += 64) p += v[i] * y[i];
                const double w = t * (y[l] + wave_sum(p));
                for (int i = l + 1 + lane; i < m; i += 64) y[i] -= w * v[i];
                if (lane == 0) y[l] -= w;
            }
            __syncthreads();
        }
        // fold R^T (n x np) into site j-1: M_{j-1}[l][s][r'] = sum_{r >= r'} M_{j-1}[l][s][r] R(r', r), R(r', r) = A(r', r)
        double* P = sites + ((int64_t)c * T + j - 1) * S;
        const int nl = ch[j - 1];
        for (int64_t e = tid; e < (int64_t)nl * d * np; e += AN_THREADS) {
            const int rp = (int)(e % np);
            const double* row = P + (e / np) * n;
            double acc = 0.0;
            for (int r = rp; r < n; ++r) acc += row[r] * A[(int64_t)r * m + rp];
            Fb[e] = acc;
        }
        __syncthreads();
        for (int64_t e = tid; e < (int64_t)nl * d * np; e += AN_THREADS) P[e] = Fb[e];
        for (int64_t e = tid; e < (int64_t)m * np; e += AN_THREADS) A[e] = Qb[e];    // new M_j (np x m) = Q^T
        if (tid == 0) ch[j] = np;
        __syncthreads();
    }
    // site 0 (chi_l = 1): its norm is the state's norm; dropping it normalises the state (a zero state becomes NaN)
    double* A0 = sites + (int64_t)c * T * S;
    const int m0 = d * ch[1];
    double ss = 0.0;
    for (int i = tid; i < m0; i += AN_THREADS) ss += A0[i] * A0[i];
    ss = wave_sum(ss);
    if (lane == 0) red[wv] = ss;
    __syncthreads();
    ss = 0.0;
    for (int w = 0; w < AN_THREADS / 64; ++w) ss += red[w];
    const double inv = 1.0 / sqrt(ss);
    for (int i = tid; i < m0; i += AN_THREADS) A0[i] *= inv;
}

// V[b][k][0..ld): the normalised measured boundary vector of instance i0 + b before site k (V[b][0] = e_0); zero padded.
__global__ __launch_bounds__(AN_THREADS) void k_an_bvec(const double* sites, const int32_t* chi, int T, int d, int64_t S, int ld,
                                                        const double* phi, int64_t i0, double* V) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i = i0 + b;
    __shared__ double v[128], ph[16], red[AN_THREADS / 64];
    double* out = V + (int64_t)b * T * ld;
    for (int r = tid; r < ld; r += AN_THREADS) out[r] = (r == 0) ? 1.0 : 0.0;
    if (tid < 128) v[tid] = (tid == 0) ? 1.0 : 0.0;
    for (int k = 1; k < T; ++k) {
        const int cl = chi[k - 1], cr = chi[k];
        const double* B = sites + (int64_t)(k - 1) * S;
        if (tid < d) ph[tid] = phi[(i * T + (k - 1)) * d + tid];
        __syncthreads();
        double w = 0.0;
        if (tid < cr)
            for (int l = 0; l < cl; ++l) {
                double a = 0.0;
                for (int s = 0; s < d; ++s) a += ph[s] * B[((int64_t)l * d + s) * cr + tid];
                w += v[l] * a;
            }
        double ss = wave_sum(w * w);
        if (lane == 0) red[wv] = ss;
        __syncthreads();
        ss = 0.0;
        for (int q = 0; q < AN_THREADS / 64; ++q) ss += red[q];
        w /= sqrt(ss);
        if (tid < 128) v[tid] = (tid < cr) ? w : 0.0;
        for (int r = tid; r < ld; r += AN_THREADS) out[(int64_t)k * ld + r] = (r < cr) ? w : 0.0;
        __syncthreads();
    }
}

// One workgroup per chain (b, k), chains q = k nb + b dealt out longest first.  rho[((b nk + k) T + j) d d + s d + s'];
// Lout (k = 0 walk of the entanglement call): L_j for j = 1..T-1 at Lout + j ld ld.  Matrices have leading dimension ld
// (even, >= every bond); 2x2 register tiles, whose padding rows / columns stay zero because the operands' do.
template <bool kLds>
__global__ __launch_bounds__(AN_THREADS) void k_an_walk(const double* sites, const int32_t* chi, int T, int d, int64_t S, int ld,
                                                        const double* V, int nb, int nk, double* rho, double* Lout, double* gws) {
    extern __shared__ double smem[];
    __shared__ double rpart[AN_THREADS / 64][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t mm = (int64_t)ld * ld;
    double* L = kLds ? smem : gws + (int64_t)blockIdx.x * 3 * mm;
    double* X = L + mm;
    double* Ln = X + mm;
    for (int64_t q = blockIdx.x; q < (int64_t)nb * nk; q += gridDim.x) {
        const int k = (int)(q / nb), b = (int)(q % nb);
        const double* v = V + ((int64_t)b * T + k) * ld;
        for (int64_t e = tid; e < mm; e += AN_THREADS) L[e] = v[e / ld] * v[e % ld];
        __syncthreads();
        for (int j = k; j < T; ++j) {
            const int cl = chi[j], cr = chi[j + 1];
            const int tr = (cl + 1) >> 1, tc = (cr + 1) >> 1;
            const double* B = sites + (int64_t)j * S;
            for (int sp = 0; sp < d; ++sp) {
                double racc[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) racc[s] = 0.0;
                // X = L B^sp, and the partial Frobenius products <B^s, X> of this thread's tiles
                for (int t = tid; t < tr * tc; t += AN_THREADS) {
                    const int r0 = 2 * (t / tc), c0 = 2 * (t % tc);
                    const bool c1ok = c0 + 1 < cr, r1ok = r0 + 1 < cl;
                    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
                    for (int a = 0; a < cl; ++a) {
                        const double l0 = L[(int64_t)r0 * ld + a], l1 = L[(int64_t)(r0 + 1) * ld + a];
                        const double* br = B + ((int64_t)a * d + sp) * cr + c0;
                        const double b0 = br[0], b1 = c1ok ? br[1] : 0.0;
                        a00 += l0 * b0; a01 += l0 * b1; a10 += l1 * b0; a11 += l1 * b1;
                    }
                    X[(int64_t)r0 * ld + c0] = a00; X[(int64_t)r0 * ld + c0 + 1] = a01;
                    X[(int64_t)(r0 + 1) * ld + c0] = a10; X[(int64_t)(r0 + 1) * ld + c0 + 1] = a11;
#pragma unroll
                    for (int s = 0; s < 16; ++s)
                        if (s < d) {
                            const double* b0r = B + ((int64_t)r0 * d + s) * cr + c0;
                            double acc = b0r[0] * a00 + (c1ok ? b0r[1] * a01 : 0.0);
                            if (r1ok) {
                                const double* b1r = B + ((int64_t)(r0 + 1) * d + s) * cr + c0;
                                acc += b1r[0] * a10 + (c1ok ? b1r[1] * a11 : 0.0);
                            }
                            racc[s] += acc;
                        }
                }
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    if (s < d) {
                        const double r = wave_sum(racc[s]);
                        if (lane == 0) rpart[wv][s * d + sp] = r;
                    }
                __syncthreads();
                // L' (+)= B^spT X
                for (int t = tid; t < tc * tc; t += AN_THREADS) {
                    const int r0 = 2 * (t / tc), c0 = 2 * (t % tc);
                    const bool r1ok = r0 + 1 < cr;
                    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
                    for (int a = 0; a < cl; ++a) {
                        const double* br = B + ((int64_t)a * d + sp) * cr + r0;
                        const double b0 = br[0], b1 = r1ok ? br[1] : 0.0;
                        const double x0 = X[(int64_t)a * ld + c0], x1 = X[(int64_t)a * ld + c0 + 1];
                        a00 += b0 * x0; a01 += b0 * x1; a10 += b1 * x0; a11 += b1 * x1;
                    }
                    double* o0 = Ln + (int64_t)r0 * ld + c0;
                    double* o1 = o0 + ld;
                    if (sp == 0) { o0[0] = a00; o0[1] = a01; o1[0] = a10; o1[1] = a11; }
                    else { o0[0] += a00; o0[1] += a01; o1[0] += a10; o1[1] += a11; }
                }
                __syncthreads();
            }
            double* rout = rho + (((int64_t)b * nk + k) * T + j) * d * d;
            for (int e = tid; e < d * d; e += AN_THREADS) {
                double r = 0.0;
                for (int w = 0; w < AN_THREADS / 64; ++w) r += rpart[w][e];
                rout[e] = r;
            }
            if (Lout && j + 1 < T)
                for (int64_t e = tid; e < mm; e += AN_THREADS) Lout[(int64_t)(j + 1) * mm + e] = Ln[e];
            double* tmp = L; L = Ln; Ln = tmp;
            __syncthreads();
        }
    }
}

// rho_correct (analyse.jl:69-91) + -tr(rho log rho) on the eigenvalues; out[e] for e = (b nk + k) T + j, 0 where j < k.
template <int D>
__device__ void see_one(const double* rp, double* out, int64_t e, unsigned long long* status) {
    double a[D][D];
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
        for (int q = 0; q < D; ++q) a[p][q] = 0.5 * (rp[p * D + q] + rp[q * D + p]);
    for (int sweep = 0; sweep < 50; ++sweep) {
        bool rot = false;
#pragma unroll
        for (int p = 0; p < D - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < D; ++q) {
                const double apq = a[p][q];
                if (!(fabs(apq) > 1e-300)) continue;
                rot = true;
                const double th = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r)
                    if (r != p && r != q) {
                        const double arp = a[r][p], arq = a[r][q];
                        a[r][p] = a[p][r] = c * arp - s * arq;
                        a[r][q] = a[q][r] = s * arp + c * arq;
                    }
            }
        if (!rot) break;
    }
    double lam[D];
    bool neg = false;
    int bad = -1;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        lam[p] = a[p][p];
        neg |= lam[p] < 0.0;
        if (lam[p] < -AN_EIGTOL && (bad < 0 || lam[p] < lam[bad])) bad = p;
    }
    if (bad >= 0) {
        out[e] = lam[bad];
        atomicMin(status, (unsigned long long)e * 4 + 1);
        return;
    }
    if (neg) {
        double tr = 0.0;
#pragma unroll
        for (int p = 0; p < D; ++p) { lam[p] = fmax(lam[p], AN_EIGTOL); tr += lam[p]; }
        if (!(fabs(tr - 1.0) <= 0.01)) {
            out[e] = tr;
            atomicMin(status, (unsigned long long)e * 4 + 2);
            return;
        }
    }
    double h = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p)
        if (lam[p] > 0.0) h -= lam[p] * log(lam[p]);
        else if (lam[p] != 0.0) h = lam[p];     // NaN
    out[e] = h;
}

template <int D>
__global__ __launch_bounds__(AN_THREADS) void k_an_see(const double* rho, int64_t n, int T, int nk, double* out, unsigned long long* status) {
    const int64_t e = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x;
    if (e >= n) return;
    const int j = (int)(e % T), k = (int)((e / T) % nk);
    if (j < k) { out[e] = 0.0; return; }
    see_one<D>(rho + e * D * D, out, e, status);
}

// eig(L_j), j = 1 + blockIdx.x, by parallel-ordered (round-robin) Jacobi in place; bee[j - 1] = -sum_{p > 1e-12} p log p.
__global__ __launch_bounds__(AN_THREADS) void k_an_bee(double* Lall, const int32_t* chi, int ld, double* bee) {
    const int j = 1 + blockIdx.x, tid = threadIdx.x;
    const int n = chi[j], n2 = n + (n & 1), np = n2 / 2;
    double* A = Lall + (int64_t)j * ld * ld;
    __shared__ double cs[64][2];
    __shared__ int pq[64][2];
    __shared__ int any;
    for (int sweep = 0; sweep < 60 && n > 1; ++sweep) {
        if (tid == 0) any = 0;
        __syncthreads();
        for (int r = 0; r < n2 - 1; ++r) {
            if (tid < np) {
                int p, q;
                if (tid == 0) { p = r; q = n2 - 1; }
                else { p = (r + tid) % (n2 - 1); q = (r - tid + n2 - 1) % (n2 - 1); }
                if (p > q) { const int t = p; p = q; q = t; }
                double c = 1.0, s = 0.0;
                if (q < n) {
                    const double apq = A[(int64_t)p * ld + q];
                    if (fabs(apq) > 1e-300) {
                        const double th = (A[(int64_t)q * ld + q] - A[(int64_t)p * ld + p]) / (2.0 * apq);
                        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        any = 1;
                    }
                }
                pq[tid][0] = p; pq[tid][1] = q; cs[tid][0] = c; cs[tid][1] = s;
            }
            __syncthreads();
            for (int e = tid; e < np * n; e += AN_THREADS) {        // columns: A <- A J
                const int i = e / n, row = e % n, p = pq[i][0], q = pq[i][1];
                if (q >= n || cs[i][1] == 0.0) continue;
                const double c = cs[i][0], s = cs[i][1];
                const double x = A[(int64_t)row * ld + p], y = A[(int64_t)row * ld + q];
                A[(int64_t)row * ld + p] = c * x - s * y;
                A[(int64_t)row * ld + q] = s * x + c * y;
            }
            __syncthreads();
            for (int e = tid; e < np * n; e += AN_THREADS) {        // rows: A <- J^T A
                const int i = e / n, col = e % n, p = pq[i][0], q = pq[i][1];
                if (q >= n || cs[i][1] == 0.0) continue;
                const double c = cs[i][0], s = cs[i][1];
                const double x = A[(int64_t)p * ld + col], y = A[(int64_t)q * ld + col];
                A[(int64_t)p * ld + col] = c * x - s * y;
                A[(int64_t)q * ld + col] = s * x + c * y;
            }
            __syncthreads();
            if (tid < np && pq[tid][1] < n && cs[tid][1] != 0.0) {
                A[(int64_t)pq[tid][0] * ld + pq[tid][1]] = 0.0;
                A[(int64_t)pq[tid][1] * ld + pq[tid][0]] = 0.0;
            }
            __syncthreads();
        }
        const bool more = any != 0;
        __syncthreads();
        if (!more) break;
    }
    if (tid == 0) {
        double h = 0.0;
        for (int i = 0; i < n; ++i) {
            const double p = A[(int64_t)i * ld + i];
            if (p > 1e-12) h -= p * log(p);
            else if (p != p) h = p;
        }
        bee[j - 1] = h;
    }
}

template <int D>
void launch_see_d(const double* rho, int64_t n, int T, int nk, double* out, unsigned long long* st, hipStream_t s) {
    hipLaunchKernelGGL(k_an_see<D>, dim3((unsigned)((n + AN_THREADS - 1) / AN_THREADS)), dim3(AN_THREADS), 0, s, rho, n, T, nk, out, st);
}

void launch_see(int d, const double* rho, int64_t n, int T, int nk, double* out, unsigned long long* st, hipStream_t s) {
    switch (d) {
        case 1: launch_see_d<1>(rho, n, T, nk, out, st, s); break;
        case 2: launch_see_d<2>(rho, n, T, nk, out, st, s); break;
        case 3: launch_see_d<3>(rho, n, T, nk, out, st, s); break;
        case 4: launch_see_d<4>(rho, n, T, nk, out, st, s); break;
        case 5: launch_see_d<5>(rho, n, T, nk, out, st, s); break;
        case 6: launch_see_d<6>(rho, n, T, nk, out, st, s); break;
        case 7: launch_see_d<7>(rho, n, T, nk, out, st, s); break;
        case 8: launch_see_d<8>(rho, n, T, nk, out, st, s); break;
        case 9: launch_see_d<9>(rho, n, T, nk, out, st, s); break;
        case 10: launch_see_d<10>(rho, n, T, nk, out, st, s); break;
        case 11: launch_see_d<11>(rho, n, T, nk, out, st, s); break;
        case 12: launch_see_d<12>(rho, n, T, nk, out, st, s); break;
        case 13: launch_see_d<13>(rho, n, T, nk, out, st, s); break;
        case 14: launch_see_d<14>(rho, n, T, nk, out, st, s); break;
        case 15: launch_see_d<15>(rho, n, T, nk, out, st, s); break;
        default: launch_see_d<16>(rho, n, T, nk, out, st, s); break;
    }
}

void launch_walk(const double* sites, const int32_t* chi, int T, int d, int64_t S, int ld, const double* V, int nb, int nk, double* rho,
                 double* Lout, double* gws, int grid, hipStream_t s) {
    if (ld <= AN_LDS_LD)
        hipLaunchKernelGGL(k_an_walk<true>, dim3(grid), dim3(AN_THREADS), (size_t)3 * ld * ld * sizeof(double), s, sites, chi, T, d, S, ld, V,
                           nb, nk, rho, Lout, gws);
    else
        hipLaunchKernelGGL(k_an_walk<false>, dim3(grid), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, ld, V, nb, nk, rho, Lout, gws);
}

int walk_grid(int ld, int64_t nchains) { return (int)std::min<int64_t>(nchains, ld <= AN_LDS_LD ? 1024 : 512); }

// device buffers of one call, freed on every exit
struct Bufs {
    std::vector<void*> p;
    template <typename T>
    hipError_t get(T** out, int64_t n) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, (size_t)std::max<int64_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
    ~Bufs() { for (void* q : p) (void)hipFree(q); }
};

#define AN_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// classes [c0, c0 + nc) of the host model, label slice folded in, to the device layout; chi per class
hipError_t upload_model(const AnalysisHost& h, int c0, int nc, int64_t S, Bufs& bufs, double** dsites, int32_t** dchi, hipStream_t s) {
    const int T = h.T, d = h.d;
    std::vector<double> hs((size_t)nc * T * S, 0.0);
    std::vector<int32_t> hc((size_t)nc * (T + 1));
    for (int c = 0; c < nc; ++c) {
        for (int j = 0; j <= T; ++j) hc[(size_t)c * (T + 1) + j] = h.chi[j];
        for (int j = 0; j < T; ++j) {
            const int Dl = h.chi[j], Dr = h.chi[j + 1], cc = (j == h.label_site) ? c0 + c : 0;
            const double* src = h.site[j];
            double* dst = &hs[((size_t)c * T + j) * S];
            for (int l = 0; l < Dl; ++l)
                for (int sidx = 0; sidx < d; ++sidx)
                    for (int r = 0; r < Dr; ++r)
                        dst[((size_t)l * d + sidx) * Dr + r] = src[sidx + (size_t)d * (l + (size_t)Dl * (r + (size_t)Dr * cc))];
        }
    }
    AN_TRY(bufs.get(dsites, (int64_t)hs.size()));
    AN_TRY(bufs.get(dchi, (int64_t)hc.size()));
    AN_TRY(hipMemcpyAsync(*dsites, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, s));
    AN_TRY(hipMemcpyAsync(*dchi, hc.data(), hc.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return hipSuccess;
}

void decode_status(unsigned long long st, const double* out, int T, int nk, int cls, int64_t i0, AnalysisDomain* dom) {
    const int64_t e = (int64_t)(st / 4);
    dom->kind = (int)(st % 4);
    dom->cls = cls;
    dom->site = (int)(e % T);
    dom->k = (int)((e / T) % nk);
    dom->inst = nk > 1 ? i0 + e / ((int64_t)T * nk) : -1;
    dom->value = out[e];
}

}  // namespace

int analysis_lds_ld() { return AN_LDS_LD; }

hipError_t analysis_entanglement(const AnalysisHost& h, hipStream_t s, double* bee, double* see, AnalysisDomain* dom) {
    const int T = h.T, d = h.d, C = h.C;
    int cap = 1;
    for (int j = 0; j <= T; ++j) cap = std::max(cap, (int)h.chi[j]);
    const int ld = cap + (cap & 1);
    const int64_t S = (int64_t)cap * d * cap, mm = (int64_t)ld * ld;
    dom->kind = 0;
    Bufs bufs;
    double *sites, *work, *V, *rho, *Lall, *sout, *bout, *gws = nullptr;
    int32_t* chi;
    unsigned long long* st;
    AN_TRY(upload_model(h, 0, C, S, bufs, &sites, &chi, s));
    AN_TRY(bufs.get(&work, (int64_t)C * 2 * S));
    AN_TRY(bufs.get(&V, (int64_t)T * ld));
    AN_TRY(bufs.get(&rho, (int64_t)C * T * d * d));
    AN_TRY(bufs.get(&Lall, (int64_t)C * T * mm));
    AN_TRY(bufs.get(&sout, (int64_t)C * T));
    AN_TRY(bufs.get(&bout, (int64_t)C * T));
    AN_TRY(bufs.get(&st, 1));
    if (ld > AN_LDS_LD) AN_TRY(bufs.get(&gws, 3 * mm));
    std::vector<double> e0(ld, 0.0);
    e0[0] = 1.0;
    AN_TRY(hipMemcpyAsync(V, e0.data(), ld * sizeof(double), hipMemcpyHostToDevice, s));
    AN_TRY(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), s));
    AN_TRY(hipMemsetAsync(bout, 0, C * T * sizeof(double), s));
    hipLaunchKernelGGL(k_an_canon, dim3(C), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, work);
    for (int c = 0; c < C; ++c) {
        const double* cs = sites + (int64_t)c * T * S;
        const int32_t* cc = chi + (int64_t)c * (T + 1);
        launch_walk(cs, cc, T, d, S, ld, V, 1, 1, rho + (int64_t)c * T * d * d, Lall + (int64_t)c * T * mm, gws, 1, s);
        if (T > 1) hipLaunchKernelGGL(k_an_bee, dim3(T - 1), dim3(AN_THREADS), 0, s, Lall + (int64_t)c * T * mm, cc, ld, bout + (int64_t)c * T);
    }
    launch_see(d, rho, (int64_t)C * T, T, 1, sout, st, s);
    AN_TRY(hipGetLastError());
    std::vector<double> hs((size_t)C * T), hb((size_t)C * T);
    unsigned long long hst = 0;
    AN_TRY(hipMemcpyAsync(hs.data(), sout, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    AN_TRY(hipMemcpyAsync(hb.data(), bout, hb.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    AN_TRY(hipMemcpyAsync(&hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
    AN_TRY(hipStreamSynchronize(s));
    if (hst != ~0ull) {
        const int64_t e = (int64_t)(hst / 4);
        decode_status(hst, hs.data(), T, 1, (int)(e / T), 0, dom);
        return hipSuccess;
    }
    for (int c = 0; c < C; ++c) {
        if (T > 1) hb[(size_t)c * T + T - 1] = hb[(size_t)c * T + T - 2];     // entropy[N] cuts bond N-1 again (analyse.jl:30-32)
        if (bee) std::memcpy(bee + (size_t)c * T, &hb[(size_t)c * T], T * sizeof(double));
        if (see) std::memcpy(see + (size_t)c * T, &hs[(size_t)c * T], T * sizeof(double));
    }
    return hipSuccess;
}

hipError_t analysis_see_variation(const AnalysisHost& h, int cls, const double* phi, int64_t N, hipStream_t s, double* out, double* seconds,
                                  AnalysisDomain* dom) {
    const int T = h.T, d = h.d;
    int cap = 1;
    for (int j = 0; j <= T; ++j) cap = std::max(cap, (int)h.chi[j]);
    const int ld = cap + (cap & 1);
    const int64_t S = (int64_t)cap * d * cap, mm = (int64_t)ld * ld;
    const int64_t per = (int64_t)T * T * (d * d + 1) + (int64_t)T * ld;     // doubles per instance in a block
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(N, AN_BLOCK_BYTES / 8 / per));
    dom->kind = 0;
    Bufs bufs;
    double *sites, *work, *dphi, *V, *rho, *dout, *gws = nullptr;
    int32_t* chi;
    unsigned long long* st;
    AN_TRY(upload_model(h, cls, 1, S, bufs, &sites, &chi, s));
    AN_TRY(bufs.get(&work, 2 * S));
    AN_TRY(bufs.get(&dphi, N * T * d));
    AN_TRY(bufs.get(&V, (int64_t)nb * T * ld));
    AN_TRY(bufs.get(&rho, (int64_t)nb * T * T * d * d));
    AN_TRY(bufs.get(&dout, (int64_t)nb * T * T));
    AN_TRY(bufs.get(&st, 1));
    const int grid = walk_grid(ld, (int64_t)nb * T);
    if (ld > AN_LDS_LD) AN_TRY(bufs.get(&gws, (int64_t)grid * 3 * mm));
    AN_TRY(hipMemcpyAsync(dphi, phi, (size_t)N * T * d * sizeof(double), hipMemcpyHostToDevice, s));
    AN_TRY(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), s));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t* e; ~Ev() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    AN_TRY(hipEventCreate(&ev[0]));
    AN_TRY(hipEventCreate(&ev[1]));
    double total = 0.0;
    AN_TRY(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(k_an_canon, dim3(1), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, work);
    for (int64_t i0 = 0; i0 < N; i0 += nb) {
        const int n = (int)std::min<int64_t>(nb, N - i0);
        hipLaunchKernelGGL(k_an_bvec, dim3(n), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, ld, dphi, i0, V);
        launch_walk(sites, chi, T, d, S, ld, V, n, T, rho, nullptr, gws, walk_grid(ld, (int64_t)n * T), s);
        launch_see(d, rho, (int64_t)n * T * T, T, T, dout, st, s);
        AN_TRY(hipGetLastError());
        AN_TRY(hipEventRecord(ev[1], s));
        unsigned long long hst = 0;
        AN_TRY(hipMemcpyAsync(out + i0 * T * T, dout, (size_t)n * T * T * sizeof(double), hipMemcpyDeviceToHost, s));
        AN_TRY(hipMemcpyAsync(&hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
        AN_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        AN_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        total += ms * 1e-3;
        if (hst != ~0ull) {
            decode_status(hst, out + i0 * T * T, T, T, cls, i0, dom);
            break;
        }
        AN_TRY(hipEventRecord(ev[0], s));
    }
    if (seconds) *seconds = total;
    return hipSuccess;
}

}  // namespace mpst
