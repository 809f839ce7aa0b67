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
//   6. k_an_pair   pair analysis, no counterpart in the reference: from the canonical tensors and the L_j of the k = 0
//                  walk, the two-site reduced density matrix of every pair of sites on the fp64 matrix pipe, its moments under an
//                  observable as they appear, and (k_an_pair_ent, on the Jacobi sweep k_an_bee uses) its entropy.
// Real fp64 only, chi <= 128, d <= 16.  No trap or abort on the device: a DomainError of rho_correct is reported through a
// status word (the smallest failing flat index, atomicMin) and the offending value stored in place of the entropy.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "mpst_internal.h"

namespace mpst {
namespace {

constexpr int AN_THREADS = 256;
// k_an_pair: eight waves up to four column tiles (two waves per SIMD, 256 registers each: no scratch), four beyond
constexpr int pair_threads(int nt) { return nt <= 4 ? 512 : AN_THREADS; }
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

// Parallel-ordered (round-robin) Jacobi of the symmetric n x n matrix A (leading dimension ld, n <= 128) in place, by the whole
// workgroup; the eigenvalues are left on the diagonal.
__device__ void jacobi_diag(double* A, int n, int ld, double (*cs)[2], int (*pq)[2], int* any) {
    const int tid = threadIdx.x, n2 = n + (n & 1), np = n2 / 2;
    for (int sweep = 0; sweep < 60 && n > 1; ++sweep) {
        if (tid == 0) *any = 0;
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
                        *any = 1;
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
        const bool more = *any != 0;
        __syncthreads();
        if (!more) break;
    }
}

// eig(L_j), j = 1 + blockIdx.x, in place; bee[j - 1] = -sum_{p > 1e-12} p log p.
__global__ __launch_bounds__(AN_THREADS) void k_an_bee(double* Lall, const int32_t* chi, int ld, double* bee) {
    const int j = 1 + blockIdx.x, tid = threadIdx.x;
    const int n = chi[j];
    double* A = Lall + (int64_t)j * ld * ld;
    __shared__ double cs[64][2];
    __shared__ int pq[64][2];
    __shared__ int any;
    jacobi_diag(A, n, ld, cs, pq, &any);
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

// ---- pair analysis: the two-site reduced density matrix of every pair of sites -------------------------------------
// S of the n x n matrices at M + m n n (m = blockIdx.x; overwritten): (rho + rho^T) / 2, Jacobi, -sum over lam > 0 of lam ln lam.
// No rho_correct and no threshold: x ln x is continuous at 0.  A NaN eigenvalue gives NaN.
__global__ __launch_bounds__(AN_THREADS) void k_an_pair_ent(double* M, int n, double* S) {
    const int tid = threadIdx.x;
    double* A = M + (int64_t)blockIdx.x * n * n;
    __shared__ double cs[64][2];
    __shared__ int pq[64][2];
    __shared__ int any;
    for (int e = tid; e < n * n; e += AN_THREADS) {
        const int r = e / n, c = e % n;
        if (r < c) {
            const double v = 0.5 * (A[r * n + c] + A[c * n + r]);
            A[r * n + c] = v;
            A[c * n + r] = v;
        }
    }
    __syncthreads();
    jacobi_diag(A, n, n, cs, pq, &any);
    if (tid == 0) {
        double h = 0.0;
        for (int i = 0; i < n; ++i) {
            const double p = A[(int64_t)i * n + i];
            if (p > 0.0) h -= p * log(p);
            else if (p != p) h = p;
        }
        S[blockIdx.x] = h;
    }
}

// Bp[c][j][s] (ldp x ldp, row l, column r): site tensor j of class c after k_an_canon, zero beyond its bonds
__global__ __launch_bounds__(AN_THREADS) void k_an_pair_pack(const double* sites, const int32_t* chi, int T, int d, int64_t S, int ldp, double* Bp) {
    const int j = blockIdx.x, c = blockIdx.y;
    const int32_t* ch = chi + (int64_t)c * (T + 1);
    const int cl = ch[j], cr = ch[j + 1];
    const double* src = sites + ((int64_t)c * T + j) * S;
    double* dst = Bp + ((int64_t)c * T + j) * d * ldp * ldp;
    for (int e = threadIdx.x; e < d * ldp * ldp; e += AN_THREADS) {
        const int s = e / (ldp * ldp), l = (e / ldp) % ldp, r = e % ldp;
        dst[e] = (l < cl && r < cr) ? src[((int64_t)l * d + s) * cr + r] : 0.0;
    }
}

// pairs (i', j) of one class in the rows [i_lo, i) of a chain of T sites
__host__ __device__ inline int64_t pair_rows_before(int T, int i_lo, int i) {
    return (int64_t)(i - i_lo) * (T - 1) - ((int64_t)i * (i - 1) / 2 - (int64_t)i_lo * (i_lo - 1) / 2);
}

struct PairArgs {
    const double* Bp;           // [C][T][d][ldp][ldp]
    const int32_t* chi;         // [C][T + 1], as k_an_canon left it
    const double* Lall;         // [C][T][ldL][ldL]: L_j for j >= 1 (k_an_walk's Lout)
    const double* obs;          // [T][d][d] or null
    double* rho;                // [C rows_before(i) + c (T - 1 - i) + j - i - 1][d d][d d] of this block, or null
    double* craw;               // [C][T][T]: tr(rho_ij O_i (x) O_j), or null
    double* gws;                // scratch, wg_doubles per workgroup
    int64_t wg_doubles;
    int C, T, d, ldL, ld, lde, i_lo, i_hi;
};

// One chain per (class c, first site i): E^{ss'} = B_i^sT L_i B_i^s' for s <= s', then for j = i + 1 .. T - 1 and every kept block
// and t':  Y = E^{ss'} B_j^t',  rho_ij[(s,t),(s',t')] = <B_j^t, Y>_F for every t,  E'^{ss'} += B_j^t'T Y.  A wave owns (block, 16
// columns of Y): the NT row tiles of Y stay in its accumulators, which are the B operand of the second product as they lie (lane l
// owns rows (l >> 4) + 4 r, the k index of the instruction), so Y is never stored.  The partial Frobenius products of a column tile go
// to the workgroup's scratch and are added over the tiles in a fixed order: no atomics, and nothing depends on where a chain runs.
// Blocks are ld x ld (ld a multiple of 4) with row stride lde; rows and columns beyond a bond are exact zeros, because Bp's are.
template <int NT, bool kLds>
__global__ __launch_bounds__(pair_threads(NT)) void k_an_pair(PairArgs g) {
    extern __shared__ double smem[];
    constexpr int ldp = 16 * NT, PT = pair_threads(NT);
    __shared__ double red[PT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i16 = lane & 15, kq = lane >> 4;
    const int T = g.T, d = g.d, ld = g.ld, lde = g.lde, ldL = g.ldL, np = d * (d + 1) / 2, dd = d * d;
    const int64_t bs = (int64_t)ld * lde, tsz = (int64_t)ldp * ldp;
    double* ws = g.gws + (int64_t)blockIdx.x * g.wg_doubles;
    double* fro = ws;                                           // [np][NT][t'][t]
    double* E = kLds ? smem : ws + (int64_t)np * NT * dd;
    double* En = E + np * bs;
    const int64_t nchains = (int64_t)(g.i_hi - g.i_lo) * g.C;
    for (int64_t q = blockIdx.x; q < nchains; q += gridDim.x) {
        const int i = g.i_lo + (int)(q / g.C), c = (int)(q % g.C);
        const int32_t* ch = g.chi + (int64_t)c * (T + 1);
        const double* Bc = g.Bp + (int64_t)c * T * d * tsz;
        {   // E^{ss'} of site i (scalar: once per chain)
            const double* Bi = Bc + (int64_t)i * d * tsz;
            const int cl = ch[i], cr = ch[i + 1];
            const double* L = g.Lall + ((int64_t)c * T + i) * ldL * ldL;
            double* X = En;                                     // X = L_i B_i^s' (cl x cr)
            for (int sp = 0; sp < d; ++sp) {
                const double* Bs = Bi + sp * tsz;
                for (int e = tid; e < cl * cr; e += PT) {
                    const int a = e / cr, b = e % cr;
                    double acc = 0.0;
                    if (i == 0) acc = Bs[b];                    // L_0 = [1]
                    else
                        for (int l = 0; l < cl; ++l) acc += L[a * ldL + l] * Bs[l * ldp + b];
                    X[a * lde + b] = acc;
                }
                __syncthreads();
                for (int s = 0; s <= sp; ++s) {
                    const double* Bt = Bi + s * tsz;
                    double* Ep = E + (sp * (sp + 1) / 2 + s) * bs;
                    for (int e = tid; e < ld * ld; e += PT) {
                        const int a = e / ld, b = e % ld;
                        double acc = 0.0;
                        if (a < cr && b < cr)
                            for (int l = 0; l < cl; ++l) acc += Bt[l * ldp + a] * X[l * lde + b];
                        Ep[a * lde + b] = acc;
                    }
                }
                __syncthreads();
            }
        }
        const int64_t pair0 = (int64_t)g.C * pair_rows_before(T, g.i_lo, i) + (int64_t)c * (T - 1 - i);
        for (int j = i + 1; j < T; ++j) {
            const double* Bj = Bc + (int64_t)j * d * tsz;
            const bool carry = j + 1 < T;
            for (int item = wv; item < np * NT; item += PT / 64) {
                const int p = item / NT, bb = item % NT, col = bb * 16 + i16;
                const double* Ep = E + p * bs;
                d4 en[NT];
#pragma unroll
                for (int u = 0; u < NT; ++u) en[u] = d4{0.0, 0.0, 0.0, 0.0};
                for (int tp = 0; tp < d; ++tp) {
                    const double* Bt = Bj + tp * tsz;
                    d4 y[NT];
#pragma unroll
                    for (int lt = 0; lt < NT; ++lt) {
                        const int row = lt * 16 + i16;
                        const bool rok = row < ld;
                        d4 acc = {0.0, 0.0, 0.0, 0.0};
                        for (int k0 = 0; k0 < ld; k0 += 4) {
                            const double a = rok ? Ep[row * lde + k0 + kq] : 0.0;
                            acc = mfma_f64(a, Bt[(k0 + kq) * ldp + col], acc);
                        }
                        y[lt] = acc;
                    }
                    for (int t = 0; t < d; ++t) {
                        const double* Bq = Bj + t * tsz;
                        double f = 0.0;
#pragma unroll
                        for (int lt = 0; lt < NT; ++lt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) f = fma(Bq[(lt * 16 + kq + 4 * r) * ldp + col], y[lt][r], f);
                        f = wave_sum(f);
                        if (lane == 0) fro[((int64_t)item * d + tp) * d + t] = f;
                    }
                    if (carry) {
#pragma unroll
                        for (int at = 0; at < NT; ++at)
#pragma unroll
                            for (int lt = 0; lt < NT; ++lt)
#pragma unroll
                                for (int r = 0; r < 4; ++r) en[at] = mfma_f64(Bt[(lt * 16 + kq + 4 * r) * ldp + at * 16 + i16], y[lt][r], en[at]);
                    }
                }
                if (carry) {
                    double* Eo = En + p * bs;
#pragma unroll
                    for (int at = 0; at < NT; ++at)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = at * 16 + kq + 4 * r;
                            if (row < ld && col < ld) Eo[row * lde + col] = en[at][r];
                        }
                }
            }
            __threadfence_block();
            __syncthreads();
            // rho_ij and its moment: the column tiles in order; the s > s' entries are the transposed block's
            double* rout = g.rho ? g.rho + (pair0 + (j - i - 1)) * dd * dd : nullptr;
            const double* Oi = g.obs ? g.obs + (int64_t)i * dd : nullptr;
            const double* Oj = g.obs ? g.obs + (int64_t)j * dd : nullptr;
            double mom = 0.0;
            for (int e = tid; e < np * dd; e += PT) {
                const int p = e / dd, tp = (e / d) % d, t = e % d;
                double v = 0.0;
                for (int bb = 0; bb < NT; ++bb) v += fro[(((int64_t)p * NT + bb) * d + tp) * d + t];
                int sp = 0;
                while ((sp + 1) * (sp + 2) / 2 <= p) ++sp;
                const int s = p - sp * (sp + 1) / 2;
                if (rout) {
                    rout[(int64_t)(s * d + t) * dd + sp * d + tp] = v;
                    if (s != sp) rout[(int64_t)(sp * d + tp) * dd + s * d + t] = v;
                }
                if (Oi) mom += (s == sp ? 1.0 : 2.0) * Oi[s * d + sp] * Oj[t * d + tp] * v;
            }
            if (Oi) {
                mom = wave_sum(mom);
                if (lane == 0) red[wv] = mom;
                __syncthreads();
                if (tid == 0) {
                    double m = 0.0;
                    for (int w = 0; w < PT / 64; ++w) m += red[w];
                    g.craw[((int64_t)c * T + i) * T + j] = m;
                    g.craw[((int64_t)c * T + j) * T + i] = m;
                }
            }
            double* tmp = E; E = En; En = tmp;
            __syncthreads();
        }
    }
}

template <int NT>
hipError_t launch_pair_nt(const PairArgs& g, bool lds, int grid, size_t lds_bytes, hipStream_t s) {
    if (lds) {
        if (hipError_t e = hipFuncSetAttribute((const void*)k_an_pair<NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAIR_LDS_BYTES);
            e != hipSuccess)
            return e;
        hipLaunchKernelGGL((k_an_pair<NT, true>), dim3(grid), dim3(pair_threads(NT)), lds_bytes, s, g);
    } else {
        hipLaunchKernelGGL((k_an_pair<NT, false>), dim3(grid), dim3(pair_threads(NT)), 0, s, g);
    }
    return hipSuccess;
}

hipError_t launch_pair(int nt, const PairArgs& g, bool lds, int grid, size_t lds_bytes, hipStream_t s) {
    switch (nt) {
        case 1: return launch_pair_nt<1>(g, lds, grid, lds_bytes, s);
        case 2: return launch_pair_nt<2>(g, lds, grid, lds_bytes, s);
        case 3: return launch_pair_nt<3>(g, lds, grid, lds_bytes, s);
        case 4: return launch_pair_nt<4>(g, lds, grid, lds_bytes, s);
        case 5: return launch_pair_nt<5>(g, lds, grid, lds_bytes, s);
        case 6: return launch_pair_nt<6>(g, lds, grid, lds_bytes, s);
        case 7: return launch_pair_nt<7>(g, lds, grid, lds_bytes, s);
        default: return launch_pair_nt<8>(g, lds, grid, lds_bytes, s);
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

hipError_t analysis_pairs(const AnalysisHost& h, const double* obs, bool obs_per_site, size_t free_b, const char* chunk_gb, hipStream_t s,
                          double* mi, double* mean, double* cov, double* seconds, double* phases) {
    const int T = h.T, d = h.d, C = h.C, dd = d * d;
    int cap = 1;
    for (int j = 0; j <= T; ++j) cap = std::max(cap, (int)h.chi[j]);
    const int ldL = cap + (cap & 1), nt = pair_tiles(cap), ldp = 16 * nt;
    const int64_t S = (int64_t)cap * d * cap, mmL = (int64_t)ldL * ldL, npc = (int64_t)T * (T - 1) / 2;     // pairs per class
    const bool want_mi = mi != nullptr, want_mom = mean || cov;
    const PairPlan plan = pair_plan(C, T, d, cap, want_mi, AN_BLOCK_BYTES, free_b, chunk_gb);
    const int nblocks = (int)plan.row0.size() - 1;
    Bufs bufs;
    double *sites, *work, *V, *rho1, *Lall, *Bp, *gws, *gwsw = nullptr, *rho = nullptr, *sij = nullptr, *s1 = nullptr, *craw = nullptr, *dobs = nullptr;
    int32_t* chi;
    AN_TRY(upload_model(h, 0, C, S, bufs, &sites, &chi, s));
    AN_TRY(bufs.get(&work, (int64_t)C * 2 * S));
    AN_TRY(bufs.get(&V, (int64_t)T * ldL));
    AN_TRY(bufs.get(&rho1, (int64_t)C * T * dd));
    AN_TRY(bufs.get(&Lall, (int64_t)C * T * mmL));
    AN_TRY(bufs.get(&Bp, (int64_t)C * T * d * ldp * ldp));
    AN_TRY(bufs.get(&gws, plan.workgroups * (pair_workgroup_bytes(d, cap) / 8)));
    if (ldL > AN_LDS_LD) AN_TRY(bufs.get(&gwsw, 3 * mmL));
    if (want_mi) {
        AN_TRY(bufs.get(&rho, plan.rho_bytes / 8));
        AN_TRY(bufs.get(&sij, C * npc));
        AN_TRY(bufs.get(&s1, (int64_t)C * T));
    }
    if (want_mom) {
        std::vector<double> ho((size_t)T * dd);
        for (int j = 0; j < T; ++j) std::memcpy(&ho[(size_t)j * dd], obs + (obs_per_site ? (size_t)j * dd : 0), dd * sizeof(double));
        AN_TRY(bufs.get(&dobs, (int64_t)T * dd));
        AN_TRY(bufs.get(&craw, (int64_t)C * T * T));
        AN_TRY(hipMemcpyAsync(dobs, ho.data(), ho.size() * sizeof(double), hipMemcpyHostToDevice, s));
        AN_TRY(hipStreamSynchronize(s));        // ho leaves scope
    }
    std::vector<double> e0(ldL, 0.0);
    e0[0] = 1.0;
    AN_TRY(hipMemcpyAsync(V, e0.data(), ldL * sizeof(double), hipMemcpyHostToDevice, s));
    // events: the call's begin and end, and (begin, middle, end) of every block
    struct Evs {
        std::vector<hipEvent_t> e;
        ~Evs() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
    } evs;
    for (int k = 0; k < 2 + 3 * nblocks; ++k) {
        hipEvent_t x;
        AN_TRY(hipEventCreate(&x));
        evs.e.push_back(x);
    }
    AN_TRY(hipEventRecord(evs.e[0], s));
    hipLaunchKernelGGL(k_an_canon, dim3(C), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, work);
    for (int c = 0; c < C; ++c)
        launch_walk(sites + (int64_t)c * T * S, chi + (int64_t)c * (T + 1), T, d, S, ldL, V, 1, 1, rho1 + (int64_t)c * T * dd, Lall + (int64_t)c * T * mmL,
                    gwsw, 1, s);
    hipLaunchKernelGGL(k_an_pair_pack, dim3(T, C), dim3(AN_THREADS), 0, s, sites, chi, T, d, S, ldp, Bp);
    AN_TRY(hipGetLastError());
    std::vector<double> hr1((size_t)C * T * dd);
    AN_TRY(hipMemcpyAsync(hr1.data(), rho1, hr1.size() * sizeof(double), hipMemcpyDeviceToHost, s));     // before the entropy kernel diagonalises it in place
    PairArgs g{Bp, chi, Lall, dobs, rho, craw, gws, pair_workgroup_bytes(d, cap) / 8, C, T, d, ldL, pair_ld(cap), pair_stride(cap), 0, 0};
    int64_t off = 0;
    for (int b = 0; b < nblocks; ++b) {
        g.i_lo = plan.row0[b];
        g.i_hi = plan.row0[b + 1];
        const int64_t np_b = (int64_t)C * pair_rows_before(T, g.i_lo, g.i_hi), chains = (int64_t)C * (g.i_hi - g.i_lo);
        AN_TRY(hipEventRecord(evs.e[2 + 3 * b], s));
        if (T > 1) AN_TRY(launch_pair(nt, g, plan.lds, (int)std::min<int64_t>(plan.workgroups, chains), (size_t)pair_state_bytes(d, cap), s));
        AN_TRY(hipEventRecord(evs.e[3 + 3 * b], s));
        if (want_mi) {
            if (np_b > 0) hipLaunchKernelGGL(k_an_pair_ent, dim3((unsigned)np_b), dim3(AN_THREADS), 0, s, rho, dd, sij + off);
            if (b == 0) hipLaunchKernelGGL(k_an_pair_ent, dim3(C * T), dim3(AN_THREADS), 0, s, rho1, d, s1);
        }
        AN_TRY(hipGetLastError());
        AN_TRY(hipEventRecord(evs.e[4 + 3 * b], s));
        off += np_b;
    }
    AN_TRY(hipEventRecord(evs.e[1], s));
    std::vector<double> hsij((size_t)(want_mi ? C * npc : 0)), hs1((size_t)(want_mi ? C * T : 0)), hcr((size_t)(want_mom ? (int64_t)C * T * T : 0));
    if (want_mi) {
        if (!hsij.empty()) AN_TRY(hipMemcpyAsync(hsij.data(), sij, hsij.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        AN_TRY(hipMemcpyAsync(hs1.data(), s1, hs1.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (want_mom) AN_TRY(hipMemcpyAsync(hcr.data(), craw, hcr.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    AN_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    AN_TRY(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
    if (seconds) *seconds = ms * 1e-3;
    phases[0] = phases[1] = 0.0;
    for (int b = 0; b < nblocks; ++b) {
        AN_TRY(hipEventElapsedTime(&ms, evs.e[2 + 3 * b], evs.e[3 + 3 * b]));
        phases[0] += ms * 1e-3;
        AN_TRY(hipEventElapsedTime(&ms, evs.e[3 + 3 * b], evs.e[4 + 3 * b]));
        phases[1] += ms * 1e-3;
    }
    // the one-site moments and the assembly of the symmetric outputs (C T^2 values) on the host
    std::vector<double> mu((size_t)T);
    for (int c = 0; c < C; ++c) {
        if (want_mi) {
            double* mo = mi + (size_t)c * T * T;
            const double* sc = &hs1[(size_t)c * T];
            int64_t o = 0;
            for (int b = 0; b < nblocks; ++b) {
                const int lo = plan.row0[b], hi = plan.row0[b + 1];
                for (int i = lo; i < hi; ++i) {
                    const double* row = hsij.data() + o + (int64_t)C * pair_rows_before(T, lo, i) + (int64_t)c * (T - 1 - i);
                    for (int j = i + 1; j < T; ++j) mo[(size_t)i * T + j] = mo[(size_t)j * T + i] = sc[i] + sc[j] - row[j - i - 1];
                }
                o += (int64_t)C * pair_rows_before(T, lo, hi);
            }
            for (int i = 0; i < T; ++i) mo[(size_t)i * T + i] = sc[i];
        }
        if (want_mom) {
            for (int i = 0; i < T; ++i) {
                const double* r = &hr1[((size_t)c * T + i) * dd];
                const double* O = obs + (obs_per_site ? (size_t)i * dd : 0);
                double m1 = 0.0, m2 = 0.0;
                for (int a = 0; a < d; ++a)
                    for (int bq = 0; bq < d; ++bq) {
                        double oo = 0.0;
                        for (int k = 0; k < d; ++k) oo += O[a * d + k] * O[k * d + bq];
                        const double ra = 0.5 * (r[a * d + bq] + r[bq * d + a]);
                        m1 += ra * O[a * d + bq];
                        m2 += ra * oo;
                    }
                mu[i] = m1;
                if (mean) mean[(size_t)c * T + i] = m1;
                if (cov) cov[((size_t)c * T + i) * T + i] = m2 - m1 * m1;
            }
            if (cov)
                for (int i = 0; i < T; ++i)
                    for (int j = i + 1; j < T; ++j)
                        cov[((size_t)c * T + i) * T + j] = cov[((size_t)c * T + j) * T + i] = hcr[((size_t)c * T + i) * T + j] - mu[i] * mu[j];
        }
    }
    return hipSuccess;
}

}  // namespace mpst
