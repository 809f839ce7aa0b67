// Segment marginals (included by mpst_impute.hip): for every series i, every class c, every start a and every width w <= max_width with
// a + w <= T the likelihood of the values of the sites a .. a+w-1 alone, every other site summed out (the Born rule of
// mpst_marginal_model on the complement mask of the segment),
//     l_c(i; a, w) = Re sum_ab E[a,b] G_c^{a+w}[a,b],
//     L_c^t     the density recursion of k_marginal from the left end through the sites 0 .. t-1, all of them missing,
//               E' = sum_s W_j[:, s, :]^T E conj(W_j[:, s, :]); the same for every class until it has passed the label site,
//     G_c^t     the table of k_prefix_env (mpst_prefix.inl): the same recursion from the right end through the sites T-1 .. t,
//     E         the walk from E = L^a through the known sites a .. a+w-1, E <- M_j^T E conj(M_j) with M_j = sum_q conj(phi_q) W_j[:, q, :].
// Both tables depend on the model only; what depends on the data is a walk of w known-site steps between two table entries, and the
// width w + 1 is one more step of the walk the width w ended with: N T max_width steps of 2 * 2 chi^3 flops, whatever T - w is.
//
// k_segment_left: the mirror image of k_prefix_env.  A workgroup per class walks the recursion from L^0 = 1 up to L^T and stores every L
// at trace one in the table (slot: mpst_segment_plan.h, segment_left_slot; row-major with leading dimension chi_t, (re, im) pairs for
// complex models) with the running sum of ln(trace) in lnL[t][c].  For t <= label_site the chains of all classes hold the same bits and
// class 0 stores them.  The matrix step and its two routes are k_prefix_env's.  A trace that is not a positive finite number ends the
// chain: lnL = -inf and a zero matrix from there on.  The right table is k_prefix_env itself, launched on a PrefixArgs of this call.
//
// k_segment_walk: a work item is a (series, start) pair; a fixed number of persistent workgroups of 256 threads take the items
// blockIdx.x, blockIdx.x + gridDim.x, ... in that order.  The step is k_marginal's known-site mat_step: up to the LDS limit of the
// environment pass E, M_j and T1 = M_j E live in LDS as zero-padded planes and are multiplied by lds_tile_rows, beyond it in the
// workgroup's global scratch by gmem_mm.  Every step rescales E to trace one and adds ln(trace) to an fp64 accumulator.  Left of the
// label site there is one E for all classes: after every step it is scored against the C tables G_c, each closing a chi^2 elementwise
// dot - a thread's stride of elements, the wave, the four waves, always in that order.  At the label site the workgroup keeps the
// shared E (a fourth matrix in LDS, a fifth in the scratch) and finishes the remaining widths class after class from the copy; a start
// beyond the label site begins every class from its own L_c^a.  (A workgroup per (series, start, class) would repeat the shared part
// of the walk C times.)  One lane stores each entry with a plain store: an item sees neither its neighbours nor the block cut.
// A trace that is not a positive finite number gives -inf for that width and the wider ones of the start - left of the label site for
// every class, from it on for the class at hand; a closing form that is not gives -inf for its class from that width on.  Entries with
// a + w > T are NaN.  Never NaN inside the triangle.
constexpr int SEG_MAXC = 16;
__device__ __forceinline__ int64_t seg_left_slot(int t, int c, int C, int ls) { return t <= ls ? (int64_t)t : (int64_t)(ls + 1) + (int64_t)(t - ls - 1) * C + c; }

template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_segment_left(ImpModel v, SegmentArgs g) {
    using R = double;
    using acc_t = typename Mx<R>::acc_t;
    using Mat = MrgMat<R, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    constexpr int ZW = CX ? 2 : 1;
    const int c = blockIdx.x, C = g.C, T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int ls = *v.label_site;
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 16 / (int)sizeof(R);
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const int64_t gsz = (int64_t)cm * cm * ZW;
    R *pRc, *pRn = nullptr, *pMs = nullptr, *pT1;       // E, (global scratch) E', (LDS) the site matrix, T1 = A E
    if constexpr (BIG) {
        R* base = g.work_left + (int64_t)c * PREFIX_ENV_BIG_MATS * gsz;
        pRc = base;
        pRn = base + gsz;
        pT1 = base + 2 * gsz;
        if (tid == 0) {
            pRc[0] = R(1);
            if constexpr (CX) pRc[1] = R(0);
        }
    } else {
        R* smem = reinterpret_cast<R*>(smem_raw);
        pRc = smem;
        pMs = smem + ZW * msz;
        pT1 = smem + 2 * ZW * msz;
        for (int e = tid; e < 3 * ZW * msz; e += IMP_T) smem[e] = R(0);
        __syncthreads();
        if (tid == 0) pRc[0] = R(1);
    }
    auto mat = [&](R* p, int cols) { return Mat{p, BIG ? cols : ld, BIG ? 0 : msz}; };
    auto plane = [&](R* p) { return Plane<R>{p, p + (ZW - 1) * msz}; };
    // L^0 is the 1 x 1 unit
    if (tid == 0) {
        if (c == 0) zstore<R, CX>(g.L + seg_left_slot(0, 0, C, ls) * gsz, 0, R(1), R(0));
        g.lnL[c] = 0.0;
    }
    __syncthreads();
    double lg = 0.0;
    for (int j = 0; j < T; ++j) {
        const SiteView<R> sv = site_view<R, CX>(v, j, c, true);
        const int Di = sv.Din, Do = sv.Dout;
        const bool keep = j >= ls || c == 0;                // L^{j+1} is this class's own once the chain has passed the label site
        R* dst = g.L + seg_left_slot(j + 1, c, C, ls) * gsz;
        double tr = 0.0;
        if constexpr (BIG) {
            const GMat<R> Rm{pRc, Di, 1, Di, Di};
            for (int s_ = 0; s_ < d; ++s_) {
                const GMat<R> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};     // W_j[s]^T, read in place
                gmem_mm<R, CX>(pT1, Di, A, Rm, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<R, CX>(pRn, Do, GMat<R>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            }
            for (int a_ = tid; a_ < Do; a_ += IMP_T) tr += (double)pRn[((int64_t)a_ * Do + a_) * ZW];
            tr = blk_sum(tr, red);
            if (tr > 0.0 && tr < INFINITY) {
                const double sc = 1.0 / tr;
                for (int e = tid; e < Do * Do * ZW; e += IMP_T) {
                    const R x = pRn[e] * sc;
                    pRn[e] = x;
                    if (keep) dst[e] = x;
                }
                __syncthreads();
                R* tmp = pRc;
                pRc = pRn;
                pRn = tmp;
            }
        } else {
            const Plane<R> Rcp = plane(pRc), Msp = plane(pMs), T1p = plane(pT1);
            const int tmo = (Do + 15) >> 4, tni = (Di + 15) >> 4;
            acc_t accr[MRG_NTW], acci[MRG_NTW];
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                accr[t] = acc_t{0, 0, 0, 0};
                acci[t] = acc_t{0, 0, 0, 0};
            }
            for (int s_ = 0; s_ < d; ++s_) {
                mrg_site_matrix<R, CX, BIG>(mat(pMs, Di), cp, sv, nullptr, s_, d, true);
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
            // the trace: the diagonal tiles' lanes with row == column
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                const int tile = wave + 4 * t;
                if (tile >= ntile) continue;
                const int rb = tile / tpr, wc = tile - rb * tpr;
                if (rb >= tmo || wc != rb) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + Mx<R>::row(kq, r), col = 16 * wc + i16;
                    if (row == col && row < Do) tr += (double)accr[t][r];
                }
            }
            tr = blk_sum(tr, red);
            if (tr > 0.0 && tr < INFINITY) {
                const double sc = 1.0 / tr;
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
                        const R xr = live ? accr[t][r] * sc : R(0), xi = (CX && live) ? acci[t][r] * sc : R(0);
                        Rcp.r[row * ld + col] = xr;
                        if constexpr (CX) Rcp.i[row * ld + col] = xi;
                        if (live && keep) zstore<R, CX>(dst, (int64_t)row * Do + col, xr, xi);
                    }
                }
                __syncthreads();
            }
        }
        if (!(tr > 0.0 && tr < INFINITY)) {
            // the state vanished (or is not finite) from here on: every segment that starts behind this site is -inf
            for (int jj = j + 1; jj <= T; ++jj) {
                if (tid == 0) g.lnL[(int64_t)jj * C + c] = -INFINITY;
                if (jj > ls || c == 0) {
                    R* z = g.L + seg_left_slot(jj, c, C, ls) * gsz;
                    const int Dj = v.chi[jj];
                    for (int e = tid; e < Dj * Dj * ZW; e += IMP_T) z[e] = R(0);
                }
            }
            return;
        }
        lg += log(tr);
        if (tid == 0) g.lnL[(int64_t)(j + 1) * C + c] = lg;
    }
}

template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_segment_walk(ImpModel v, SegmentArgs g) {
    using R = double;
    using acc_t = typename Mx<R>::acc_t;
    using Mat = MrgMat<R, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    __shared__ double redc[4 * SEG_MAXC];       // the waves' parts of the closings, [class][wave]
    constexpr int ZW = CX ? 2 : 1;
    const int C = g.C, T = v.T, d = v.d, cm = v.cap, mw = g.max_width, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int ls = *v.label_site;
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 16 / (int)sizeof(R);    // as in k_marginal: rows 16-byte aligned and 4 banks apart
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const int64_t gsz = (int64_t)cm * cm * ZW;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    R *pRc, *pRn = nullptr, *pMs, *pT1, *pSv;   // E, (global scratch) E', the site matrix, T1 = M E, the kept shared E
    if constexpr (BIG) {
        R* base = g.work + (int64_t)blockIdx.x * SEGMENT_BIG_MATS * gsz;
        pRc = base;
        pRn = base + gsz;
        pMs = base + 2 * gsz;
        pT1 = base + 3 * gsz;
        pSv = base + 4 * gsz;
    } else {
        R* smem = reinterpret_cast<R*>(smem_raw);
        pRc = smem;
        pMs = smem + ZW * msz;
        pT1 = smem + 2 * ZW * msz;
        pSv = smem + 3 * ZW * msz;
        for (int e = tid; e < 4 * ZW * msz; e += IMP_T) smem[e] = R(0);
    }
    auto mat = [&](R* p, int cols) { return Mat{p, BIG ? cols : ld, BIG ? 0 : msz}; };
    auto plane = [&](R* p) { return Plane<R>{p, p + (ZW - 1) * msz}; };

    // E <- M E M^H / trace through the known site `sv`, M = (sum_q conj(ph_q) W_j[q])^T: k_marginal's mat_step with its one term.
    // Returns the trace; E is left alone unless it is a positive finite number.
    auto mat_step = [&](const SiteView<R>& sv, const R* ph) -> double {
        const int Di = sv.Din, Do = sv.Dout;
        double out = 0.0;
        if constexpr (BIG) {
            mrg_site_matrix<R, CX, BIG>(mat(pMs, Di), cp, sv, ph, 0, d, false);
            __syncthreads();
            const GMat<R> Rm{pRc, Di, 1, Di, Di}, A{pMs, Di, 1, Do, Di};
            gmem_mm<R, CX>(pT1, Di, A, Rm, Do, Di, Di, false, false);
            __syncthreads();
            gmem_mm<R, CX>(pRn, Do, GMat<R>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, false);
            __syncthreads();
            for (int a_ = tid; a_ < Do; a_ += IMP_T) out += (double)pRn[((int64_t)a_ * Do + a_) * ZW];
            out = blk_sum(out, red);
            if (!(out > 0.0 && out < INFINITY)) return out;
            const double sc = 1.0 / out;
            for (int e = tid; e < Do * Do * ZW; e += IMP_T) pRn[e] *= sc;
            __syncthreads();
            R* tmp = pRc;
            pRc = pRn;
            pRn = tmp;
            return out;
        } else {
            const Plane<R> Rcp = plane(pRc), Msp = plane(pMs), T1p = plane(pT1);
            const int tmo = (Do + 15) >> 4, tni = (Di + 15) >> 4;
            acc_t accr[MRG_NTW], acci[MRG_NTW];
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                accr[t] = acc_t{0, 0, 0, 0};
                acci[t] = acc_t{0, 0, 0, 0};
            }
            mrg_site_matrix<R, CX, BIG>(mat(pMs, Di), cp, sv, ph, 0, d, true);
            __syncthreads();
            // T1 = M E^H = M E (Do x Di); the tiles beyond it are zeroed
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
            // E' = T1 M^H (Do x Do)
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                const int tile = wave + 4 * t;
                if (tile < ntile) {
                    const int rb = tile / tpr, wc = tile - rb * tpr;
                    if (rb < tmo && wc < tmo) lds_tile_rows<R, CX>(accr[t], acci[t], T1p, 16 * rb, Msp, 16 * wc, ks, ld);
                }
            }
            // the trace: the diagonal tiles' lanes with row == column
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                const int tile = wave + 4 * t;
                if (tile >= ntile) continue;
                const int rb = tile / tpr, wc = tile - rb * tpr;
                if (rb >= tmo || wc != rb) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + Mx<R>::row(kq, r), col = 16 * wc + i16;
                    if (row == col && row < Do) out += (double)accr[t][r];
                }
            }
            out = blk_sum(out, red);            // (its barriers: every wave is done with E and T1)
            if (!(out > 0.0 && out < INFINITY)) return out;
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
                    Rcp.r[row * ld + col] = live ? accr[t][r] * sc : R(0);
                    if constexpr (CX) Rcp.i[row * ld + col] = live ? acci[t][r] * sc : R(0);
                }
            }
            __syncthreads();
            return out;
        }
    };
    // E = the D x D table entry `src` (in LDS zero-padded to cp x cp)
    auto load_E = [&](const R* __restrict__ src, int D) {
        if constexpr (BIG) {
            for (int e = tid; e < D * D * ZW; e += IMP_T) pRc[e] = src[e];
        } else {
            const Mat E = mat(pRc, D);
            for (int e = tid; e < cp * cp; e += IMP_T) {
                const int r = e / cp, c_ = e - r * cp;
                R xr = R(0), xi = R(0);
                if (r < D && c_ < D) zload<R, CX>(src, (int64_t)r * D + c_, xr, xi);
                E.set(r, c_, xr, xi);
            }
        }
        __syncthreads();
    };
    // the shared E (D x D) to the kept copy, and back
    auto copy_E = [&](R* __restrict__ dst, const R* __restrict__ src, int D) {
        const int n = BIG ? D * D * ZW : ZW * msz;
        for (int e = tid; e < n; e += IMP_T) dst[e] = src[e];
        __syncthreads();
    };

    const int64_t nitem = g.count * T;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t il = item / T, i = g.first + il;
        const int a = (int)(item - il * T);
        const int nw = min(mw, T - a), jend = a + nw;
        double* out = g.logp + (il * T + a) * (int64_t)mw * C;
        __syncthreads();                        // the previous item is done with the matrices and the closings' parts
        // every entry of the item: -inf inside the triangle until its closing has succeeded, NaN beyond the end of the chain
        for (int e = tid; e < mw * C; e += IMP_T) out[e] = e / C < nw ? -INFINITY : qnan;
        bool cdead = false;                     // (thread c:) a closing of class c was not a positive finite number
        const double lnLa = tid < C ? g.lnL[(int64_t)a * C + tid] : 0.0;
        // ln l_c of the segment that ends ahead of site t, for the classes c0 .. c0 + nc - 1, from the E at hand; lg: the sum of ln(trace)
        // over its steps.  Barriers: the caller has synchronised E; one inside.
        auto close = [&](int t, int c0, int nc, double lg) {
            const int D = v.chi[t];
            for (int c = c0; c < c0 + nc; ++c) {
                const R* __restrict__ Gc = g.G + pfx_slot(t, c, C, ls) * gsz;
                double q = 0.0;
                for (int e = tid; e < D * D; e += IMP_T) {
                    R er, ei, gr, gi;
                    if constexpr (BIG) {
                        zload<R, CX>(pRc, e, er, ei);
                    } else {
                        const int r = e / D;
                        mat(pRc, D).get(r, e - r * D, er, ei);
                    }
                    zload<R, CX>(Gc, e, gr, gi);
                    q = fma(er, gr, q);
                    if constexpr (CX) q = fma(-ei, gi, q);
                }
                q = wave_sum(q);
                if (lane == 0) redc[c * 4 + wave] = q;
            }
            __syncthreads();
            if (tid >= c0 && tid < c0 + nc) {
                const double q = (redc[tid * 4] + redc[tid * 4 + 1]) + (redc[tid * 4 + 2] + redc[tid * 4 + 3]);
                if (!(q > 0.0 && q < INFINITY)) cdead = true;
                if (!cdead) {
                    const double lp = ((lnLa + lg) + log(q)) + g.lnG[(int64_t)t * C + tid];
                    out[(int64_t)(t - a - 1) * C + tid] = lp == lp ? lp : -INFINITY;
                }
            }
        };
        int j = a;
        double lg = 0.0;
        if (a <= ls) {
            // one E for all classes up to the label site
            load_E(g.L + seg_left_slot(a, 0, C, ls) * gsz, v.chi[a]);
            bool dead = false;
            for (; j < jend && j < ls; ++j) {
                const double tr = mat_step(site_view<R, CX>(v, j, 0, true), (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW);
                if (!(tr > 0.0 && tr < INFINITY)) {
                    dead = true;
                    break;
                }
                lg += log(tr);
                close(j + 1, 0, C, lg);
            }
            if (dead || j >= jend) continue;
            if (C > 1) copy_E(pSv, pRc, v.chi[ls]);
        }
        // from the label site on (or from a start beyond it): class after class
        const int j0 = j;
        const double lg0 = lg;
        for (int c = 0; c < C; ++c) {
            if (a > ls) load_E(g.L + seg_left_slot(a, c, C, ls) * gsz, v.chi[a]);
            else if (c > 0) copy_E(pRc, pSv, v.chi[ls]);
            lg = lg0;
            for (j = j0; j < jend; ++j) {
                const double tr = mat_step(site_view<R, CX>(v, j, c, true), (const R*)v.phi + ((int64_t)j * v.N + i) * d * ZW);
                if (!(tr > 0.0 && tr < INFINITY)) break;
                lg += log(tr);
                close(j + 1, c, 1, lg);
            }
        }
    }
}
