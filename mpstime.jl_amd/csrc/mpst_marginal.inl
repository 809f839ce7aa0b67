// Marginal likelihoods (included by mpst_impute.hip): ln l_c(i) of the known values of instance i under the label slice W_c
// of every class c, the missing sites summed over their physical index -
//     l_c(i) = sum over s_j, j missing, of | < (x)_{j known} phi[i][j] (x)_{j missing} e_{s_j} | W_c > |^2,
// the squared norm of what precondition (src/Imputation/MPS_methods.jl:42-99) leaves behind, for the label slice as stored (not
// renormalised per class).  With A_j = W_j[s_j] (missing) or M_j = sum_q conj(phi_q) W_j[q] (known) the amplitude is the matrix
// product A_1 ... A_T, and the sum of its squared moduli over the missing indices is the density recursion of k_imp_right,
//     E' = sum_s A_j[s] E A_j[s]^H          (one term at a known site),
// run towards the label site from BOTH ends: every class shares every tensor but the label site's, so the two half chains are
// walked once per instance, not once per class -
//     R over the right bond of the label site, from the sites behind it (entered through their right bond),
//     L over its left bond, from the sites before it (entered through their left bond),
// and the C label blocks close the chain: l_c = sum_ab (sum_s A_c[s]^T L conj(A_c[s]))_ab R_ab - tr(L m_c R m_c^H) at a known
// label site, sum_s tr(L W_s^c R (W_s^c)^H) at a missing one.
// * While a half chain has met known sites only its density is an outer product x x^H and the recursion is the vector
//   recursion x <- M_j x; complete series never form a matrix: l_c = |L m_c R|^2 with two vectors.
// * Every site rescales the state to trace one (the vector: to norm one) and adds ln(trace) to an fp64 accumulator, on the
//   fp32 compute path too: ln l loses about 0.9 per known site of a random model, so an unscaled fp32 chain underflows near
//   T = 100 and an fp64 chain near T = 900.  A trace that is not a positive finite number ends the instance with -inf in every
//   class (the half chains are shared); a label block whose closing sum is not positive gives -inf for its class.  Never NaN.
// * phi is read at known sites only.
// One workgroup of 256 threads per instance.  Up to the LDS limit of k_imp_right the matrices E, A_j[s], T1 = A E and the kept R
// live in LDS as zero-padded (re, im) planes and are multiplied by lds_tile_rows, a wave per 16 x 16 tile (up to four tiles per
// wave); beyond it (chi <= 128) they live in global scratch, five chi x chi matrices per workgroup, multiplied by gmem_mm as in
// k_imp_right_big.  One lane stores the C results of its instance.
constexpr int MRG_NTW = 4;          // tiles per wave: 16 tiles at chi = 64 on 4 waves
constexpr int MRG_BIG_MATS = 5;     // matrices of global scratch per workgroup beyond the LDS limit
constexpr int MRG_MAXC = 16;

// a matrix of the recursion: (re, im) planes `pl` elements apart with leading dimension ld in LDS, interleaved pairs in global scratch
template <typename R, bool CX, bool BIG> struct MrgMat {
    R* p;
    int ld, pl;
    __device__ __forceinline__ void get(int r, int c, R& re, R& im) const {
        if constexpr (BIG) {
            zload<R, CX>(p, (int64_t)r * ld + c, re, im);
        } else {
            re = p[r * ld + c];
            im = R(0);
            if constexpr (CX) im = p[pl + r * ld + c];
        }
    }
    __device__ __forceinline__ void set(int r, int c, R re, R im) const {
        if constexpr (BIG) {
            zstore<R, CX>(p, (int64_t)r * ld + c, re, im);
        } else {
            p[r * ld + c] = re;
            if constexpr (CX) p[pl + r * ld + c] = im;
        }
    }
};

// M[o][i] = W_j[s](i, o) (ph == null) or sum_q conj(ph_q) W_j[q](i, o); consecutive threads along the index that is contiguous in
// memory.  `pad`: the rest of the cp x cp LDS block is zeroed (operands of lds_tile_rows).
template <typename R, bool CX, bool BIG>
__device__ __forceinline__ void mrg_site_matrix(const MrgMat<R, CX, BIG>& M, int cp, const SiteView<R>& sv, const R* __restrict__ ph, int s, int d,
                                                bool pad) {
    const int Di = sv.Din, Do = sv.Dout, tid = threadIdx.x;
    const bool in_fast = sv.si == 1;
    const int Df = in_fast ? Di : Do;
    for (int e = tid; e < Di * Do; e += IMP_T) {
        const int slow = e / Df, fast = e - slow * Df;
        const int ii = in_fast ? fast : slow, oo = in_fast ? slow : fast;
        const int64_t off = (int64_t)ii * sv.si + (int64_t)oo * sv.so;
        R ar = R(0), ai = R(0);
        if (ph) {
#pragma unroll 4
            for (int q = 0; q < d; ++q) {
                R pr, pi, wr, wi;
                zload<R, CX>(ph, q, pr, pi);
                zload<R, CX>(sv.W, off + (int64_t)q * sv.ss, wr, wi);
                ar = fma(pr, wr, ar);
                if constexpr (CX) {
                    ar = fma(pi, wi, ar);
                    ai = fma(pr, wi, ai);
                    ai = fma(-pi, wr, ai);
                }
            }
        } else {
            zload<R, CX>(sv.W, off + (int64_t)s * sv.ss, ar, ai);
        }
        M.set(oo, ii, ar, ai);
    }
    if constexpr (!BIG) {
        if (pad) {
            for (int e = tid; e < cp * cp; e += IMP_T) {
                const int r = e / cp, c = e - r * cp;
                if (r >= Do || c >= Di) M.set(r, c, R(0), R(0));
            }
        }
    }
}

// y = M x (Do x Di): two threads per output value (Do <= 128)
template <typename R, bool CX, bool BIG>
__device__ __forceinline__ void mrg_matvec(const MrgMat<R, CX, BIG>& M, int Do, int Di, const R* xr, const R* xi, R* yr, R* yi) {
    const int o = threadIdx.x >> 1, h = threadIdx.x & 1;
    R ar = R(0), ai = R(0);
    if (o < Do) {
        for (int k = h; k < Di; k += 2) {
            R mr, mi_;
            M.get(o, k, mr, mi_);
            ar = fma(mr, xr[k], ar);
            if constexpr (CX) {
                ar = fma(-mi_, xi[k], ar);
                ai = fma(mr, xi[k], ai);
                ai = fma(mi_, xr[k], ai);
            }
        }
    }
    ar += __shfl_xor(ar, 1);
    if constexpr (CX) ai += __shfl_xor(ai, 1);
    if (h == 0 && o < Do) {
        yr[o] = ar;
        if constexpr (CX) yi[o] = ai;
    }
}

// E = x x^H (D x D; in LDS zero-padded to cp x cp)
template <typename R, bool CX, bool BIG>
__device__ __forceinline__ void mrg_outer(const MrgMat<R, CX, BIG>& M, int cp, int D, const R* xr, const R* xi) {
    const int dim = BIG ? D : cp;
    for (int e = threadIdx.x; e < dim * dim; e += IMP_T) {
        const int a_ = e / dim, b_ = e - a_ * dim;
        const bool live = a_ < D && b_ < D;
        R re = R(0), im = R(0);
        if (live) {
            re = xr[a_] * xr[b_];
            if constexpr (CX) {
                re = fma(xi[a_], xi[b_], re);
                im = fma(xi[a_], xr[b_], -xr[a_] * xi[b_]);
            }
        }
        M.set(a_, b_, re, im);
    }
}

template <typename R, bool CX, bool BIG>
__global__ __launch_bounds__(IMP_T) void k_marginal(ImpModel v, ImpArgs g, int C, R* __restrict__ work) {
    using acc_t = typename Mx<R>::acc_t;
    using Mat = MrgMat<R, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    __shared__ double lres[MRG_MAXC];
    __shared__ R xs[2][2][CAP_LIMIT];           // the vector of the running half chain: [current / next][re / im]
    __shared__ R us[2][CAP_LIMIT];              // the right half chain's, kept for the closing
    constexpr int ZW = CX ? 2 : 1;
    const int64_t i = g.ord[blockIdx.x];        // instance; the global scratch is indexed by blockIdx.x (chunk-local)
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const uint8_t* mi = g.missing ? g.missing + i * T : nullptr;
    const int ls = *v.label_site;
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 16 / (int)sizeof(R);    // as in k_imp_right: rows 16-byte aligned and 4 banks apart
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    R *pRc, *pRn = nullptr, *pMs, *pT1, *pSv;   // E, (global scratch) E', the site matrix, T1 = A E, the kept R
    if constexpr (BIG) {
        const int64_t bsz = (int64_t)cm * cm * ZW;
        R* base = work + (int64_t)blockIdx.x * MRG_BIG_MATS * bsz;
        pRc = base;
        pRn = base + bsz;
        pMs = base + 2 * bsz;
        pT1 = base + 3 * bsz;
        pSv = base + 4 * bsz;
    } else {
        R* smem = reinterpret_cast<R*>(smem_raw);
        pRc = smem;
        pMs = smem + ZW * msz;
        pT1 = smem + 2 * ZW * msz;
        pSv = smem + 3 * ZW * msz;
        for (int e = tid; e < 4 * ZW * msz; e += IMP_T) smem[e] = R(0);
        __syncthreads();
    }
    auto mat = [&](R* p, int cols) { return Mat{p, BIG ? cols : ld, BIG ? 0 : msz}; };
    auto plane = [&](R* p) { return Plane<R>{p, p + (ZW - 1) * msz}; };
    // the state of the running half chain (uniform over the workgroup)
    int cur = 0, D = 1;
    bool isvec = true, dead = false;
    double lg = 0.0;

    // x <- M_j x at a known site; false: the state vanished
    auto vec_step = [&](const SiteView<R>& sv, const R* ph) -> bool {
        const int Di = sv.Din, Do = sv.Dout;
        const Mat M = mat(pMs, Di);
        mrg_site_matrix<R, CX, BIG>(M, cp, sv, ph, 0, d, false);
        __syncthreads();
        mrg_matvec<R, CX, BIG>(M, Do, Di, xs[cur][0], xs[cur][1], xs[cur ^ 1][0], xs[cur ^ 1][1]);
        __syncthreads();
        R nr = R(0), ni = R(0);
        if (tid < Do) {
            nr = xs[cur ^ 1][0][tid];
            if constexpr (CX) ni = xs[cur ^ 1][1][tid];
        }
        const double n2 = blk_sum((double)nr * (double)nr + (double)ni * (double)ni, red);
        if (!(n2 > 0.0 && n2 < INFINITY)) return false;
        lg += log(n2);
        const double sc = 1.0 / sqrt(n2);
        if (tid < Do) {
            xs[cur ^ 1][0][tid] = (R)((double)nr * sc);
            if constexpr (CX) xs[cur ^ 1][1][tid] = (R)((double)ni * sc);
        }
        cur ^= 1;
        D = Do;
        __syncthreads();
        return true;
    };

    // E' = sum_s A[s] E A[s]^H through the site `sv` (one term, M_j, at a known site).  closing == false: E <- E' / tr E', returns the
    // trace (E is left alone unless the trace is a positive finite number); closing == true: returns sum_ab E'_ab R_ab, E stays.
    auto mat_step = [&](const SiteView<R>& sv, const R* ph, bool miss, bool closing) -> double {
        const int Di = sv.Din, Do = sv.Dout, ns = miss ? d : 1;
        double out = 0.0;
        if constexpr (BIG) {
            const GMat<R> Rm{pRc, Di, 1, Di, Di};
            for (int s_ = 0; s_ < ns; ++s_) {
                GMat<R> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};       // a missing site's W_j[s], read in place
                if (!miss) {
                    mrg_site_matrix<R, CX, BIG>(mat(pMs, Di), cp, sv, ph, 0, d, false);
                    __syncthreads();
                    A = GMat<R>{pMs, Di, 1, Do, Di};
                }
                gmem_mm<R, CX>(pT1, Di, A, Rm, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<R, CX>(pRn, Do, GMat<R>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            }
            if (closing) {
                for (int e = tid; e < Do * Do; e += IMP_T) {
                    R er, ei, sr, si_;
                    zload<R, CX>(pRn, e, er, ei);
                    zload<R, CX>(pSv, e, sr, si_);
                    out += (double)er * (double)sr - (double)ei * (double)si_;
                }
                return blk_sum(out, red);
            }
            for (int a_ = tid; a_ < Do; a_ += IMP_T) out += (double)pRn[((int64_t)a_ * Do + a_) * ZW];
            out = blk_sum(out, red);
            if (!(out > 0.0 && out < INFINITY)) return out;
            const double sc = 1.0 / out;
            for (int e = tid; e < Do * Do * ZW; e += IMP_T) pRn[e] = (R)((double)pRn[e] * sc);
            __syncthreads();
            R* tmp = pRc;
            pRc = pRn;
            pRn = tmp;
            return out;
        } else {
            const Plane<R> Rcp = plane(pRc), Msp = plane(pMs), T1p = plane(pT1), Svp = plane(pSv);
            const int tmo = (Do + 15) >> 4, tni = (Di + 15) >> 4;
            acc_t accr[MRG_NTW], acci[MRG_NTW];
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                accr[t] = acc_t{0, 0, 0, 0};
                acci[t] = acc_t{0, 0, 0, 0};
            }
            for (int s_ = 0; s_ < ns; ++s_) {
                mrg_site_matrix<R, CX, BIG>(mat(pMs, Di), cp, sv, miss ? nullptr : ph, s_, d, true);
                __syncthreads();
                // T1 = A E^H = A E (Do x Di); the tiles beyond it are zeroed
#pragma unroll
                for (int t = 0; t < MRG_NTW; ++t) {
                    const int tile = wave + 4 * t;
                    if (tile < ntile) {
                        const int rb = tile / tpr, wc = tile - rb * tpr;
                        acc_t ar = {0, 0, 0, 0}, ai = {0, 0, 0, 0};
                        if (rb < tmo && wc < tni) lds_tile_rows<R, CX>(ar, ai, Msp, 16 * rb, Rcp, 16 * wc, ks, ld);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int at = (16 * rb + Mx<R>::row(kq, r)) * ld + 16 * wc + i16;
                            T1p.r[at] = ar[r];
                            if constexpr (CX) T1p.i[at] = ai[r];
                        }
                    }
                }
                __syncthreads();
                // E' += T1 A^H (Do x Do)
#pragma unroll
                for (int t = 0; t < MRG_NTW; ++t) {
                    const int tile = wave + 4 * t;
                    if (tile < ntile) {
                        const int rb = tile / tpr, wc = tile - rb * tpr;
                        if (rb < tmo && wc < tmo) lds_tile_rows<R, CX>(accr[t], acci[t], T1p, 16 * rb, Msp, 16 * wc, ks, ld);
                    }
                }
                __syncthreads();
            }
            // the trace (the diagonal tiles' lanes with row == column) or the closing sum against R, from the accumulators
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                const int tile = wave + 4 * t;
                if (tile >= ntile) continue;
                const int rb = tile / tpr, wc = tile - rb * tpr;
                if (rb >= tmo || wc >= tmo) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + Mx<R>::row(kq, r), col = 16 * wc + i16;
                    if (row >= Do || col >= Do) continue;
                    if (closing) {
                        out += (double)accr[t][r] * (double)Svp.r[row * ld + col];
                        if constexpr (CX) out -= (double)acci[t][r] * (double)Svp.i[row * ld + col];
                    } else if (row == col) {
                        out += (double)accr[t][r];
                    }
                }
            }
            out = blk_sum(out, red);
            if (closing || !(out > 0.0 && out < INFINITY)) return out;
            const double sc = 1.0 / out;
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                const int tile = wave + 4 * t;
                if (tile >= ntile) continue;
                const int rb = tile / tpr, wc = tile - rb * tpr;
                const bool have = rb < tmo && wc < tmo;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + Mx<R>::row(kq, r), col = 16 * wc + i16;
                    const bool live = have && row < Do && col < Do;
                    Rcp.r[row * ld + col] = live ? (R)((double)accr[t][r] * sc) : R(0);
                    if constexpr (CX) Rcp.i[row * ld + col] = live ? (R)((double)acci[t][r] * sc) : R(0);
                }
            }
            __syncthreads();
            return out;
        }
    };

    // the n sites j0, j0 + dj, ... from the unit boundary towards the label site
    auto half_chain = [&](int j0, int dj, int n, bool in_is_left) {
        if (tid == 0) {
            xs[0][0][0] = R(1);
            xs[0][1][0] = R(0);
        }
        cur = 0;
        D = 1;
        isvec = true;
        lg = 0.0;
        __syncthreads();
        for (int st = 0; st < n && !dead; ++st) {
            const int j = j0 + dj * st;
            const bool miss = mi && mi[j] != 0;
            const SiteView<R> sv = site_view<R, CX>(v, j, 0, in_is_left);
            const R* ph = (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
            if (isvec && !miss) {
                if (!vec_step(sv, ph)) dead = true;
                continue;
            }
            if (isvec) {
                mrg_outer<R, CX, BIG>(mat(pRc, D), cp, D, xs[cur][0], xs[cur][1]);
                __syncthreads();
                isvec = false;
            }
            const double tr = mat_step(sv, ph, miss, false);
            if (!(tr > 0.0 && tr < INFINITY)) dead = true;
            else lg += log(tr);
            D = sv.Dout;
        }
    };

    // R: sites T-1 ... ls+1, kept in us (vector) or pSv (matrix)
    half_chain(T - 1, -1, T - 1 - ls, false);
    const bool rvec = isvec;
    const int DR = D;
    const double lgR = lg;
    if (!dead) {
        if (rvec) {
            if (tid < DR) {
                us[0][tid] = xs[cur][0][tid];
                if constexpr (CX) us[1][tid] = xs[cur][1][tid];
            }
        } else {
            const int n = BIG ? DR * DR * ZW : ZW * msz;
            for (int e = tid; e < n; e += IMP_T) pSv[e] = pRc[e];
        }
        __syncthreads();
        // L: sites 0 ... ls-1
        half_chain(0, 1, ls, true);
    }
    if (dead) {
        if (tid == 0)
            for (int c = 0; c < C; ++c) g.x_out[i * C + c] = -INFINITY;
        return;
    }
    const double lgs = lg + lgR;
    const bool lmiss = mi && mi[ls] != 0;
    const R* phl = (const R*)v.phi + ((int64_t)ls * v.N + i) * d * ZW;
    const bool allvec = isvec && rvec && !lmiss;
    if (!allvec) {
        if (isvec) mrg_outer<R, CX, BIG>(mat(pRc, D), cp, D, xs[cur][0], xs[cur][1]);
        if (rvec) mrg_outer<R, CX, BIG>(mat(pSv, DR), cp, DR, us[0], us[1]);
        __syncthreads();
    }
    for (int c = 0; c < C; ++c) {
        const SiteView<R> sv = site_view<R, CX>(v, ls, c, true);
        double l;
        if (allvec) {
            // l_c = |L m_c R|^2
            const Mat M = mat(pMs, sv.Din);
            mrg_site_matrix<R, CX, BIG>(M, cp, sv, phl, 0, d, false);
            __syncthreads();
            mrg_matvec<R, CX, BIG>(M, sv.Dout, sv.Din, xs[cur][0], xs[cur][1], xs[cur ^ 1][0], xs[cur ^ 1][1]);
            __syncthreads();
            double ar = 0.0, ai = 0.0;
            if (tid < sv.Dout) {
                const double yr = (double)xs[cur ^ 1][0][tid], ur = (double)us[0][tid];
                ar = yr * ur;
                if constexpr (CX) {
                    const double yi = (double)xs[cur ^ 1][1][tid], ui = (double)us[1][tid];
                    ar -= yi * ui;
                    ai = yr * ui + yi * ur;
                }
            }
            ar = blk_sum(ar, red);
            if constexpr (CX) ai = blk_sum(ai, red);
            l = ar * ar + ai * ai;
        } else {
            l = mat_step(sv, phl, lmiss, true);
        }
        if (tid == 0) lres[c] = (l > 0.0 && l < INFINITY) ? log(l) + lgs : -INFINITY;
    }
    __syncthreads();
    if (tid == 0)
        for (int c = 0; c < C; ++c) g.x_out[i * C + c] = lres[c];
}
