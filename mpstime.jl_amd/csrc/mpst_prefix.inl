// Prefix marginals (included by mpst_impute.hip): for every series i, every prefix length t = 0 .. T and every class c the likelihood of
// the first t values with the sites t .. T-1 summed out (the Born rule of mpst_marginal_model on the suffix mask of t),
//     l_c(i; t) = x_t G_c^t x_t^H,
//     x_t       the row walk through the known sites 0 .. t-1, x <- x M_j with M_j = sum_q conj(phi_q) W_j[:, q, :]; the same for every
//               class until the walk has passed the label site,
//     G_c^t     the density recursion of k_marginal from the right end through the sites T-1 .. t, all of them missing,
//               E' = sum_s W_j[:, s, :] E W_j[:, s, :]^H, which depends on the model only.
// One walk per series gives all T + 1 prefixes: N T (d + C) chi^2 multiply-adds instead of the N T^2 d chi^3 of T + 1 suffix-masked
// replicas through k_marginal.
//
// k_prefix_env: a workgroup per class walks the recursion from G^T = 1 down to G^0 and stores every G at trace one in the table
// (slot: mpst_prefix_plan.h, prefix_table_slot; row-major with leading dimension chi_t, (re, im) pairs for complex models) with the
// running sum of ln(trace) in lnG[t][c].  For t > label_site the chains of all classes hold the same bits and class 0 stores them.  The
// matrix step is k_marginal's: up to the LDS limit of the environment pass E, W_j[s] and T1 = W_j[s] E live in LDS as zero-padded planes
// and are multiplied by lds_tile_rows, beyond it in global scratch by gmem_mm.  A trace that is not a positive finite number ends the
// chain: lnG = -inf and a zero matrix from there on, so every prefix that needs them is -inf.
//
// k_prefix_score: sixteen series per workgroup, four waves, the row step of sc_walk: for every s the product X (16 x Din) . W_j[:, s, :]
// on v_mfma_f64_16x16x4_f64, then sum_s conj(phi_s) (.) row by row.  Ahead of every site and after the last one Y = X . G_c^t on the same
// pipe and the row dots Re(y . conj(x)), the waves' parts summed in a fixed order.  Every site rescales every row to norm one and adds
// ln(norm^2) to the row's fp64 accumulator.  Past the label site a row is a (series, class) pair: the rows of class c live in slot c of
// the workgroup's global scratch (slot C: the shared row they all start from) and come to LDS for their step.  A row does not see its
// neighbours.  A quadratic form that is not a positive finite number gives -inf for that entry; a row whose norm is not is zeroed, so
// that every later prefix of it is -inf.  Never NaN.
constexpr int PFX_MAXC = 16;
__device__ __forceinline__ int64_t pfx_slot(int t, int c, int C, int ls) { return t <= ls ? (int64_t)t * C + c : (int64_t)(ls + 1) * C + (t - ls - 1); }

template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_prefix_env(ImpModel v, PrefixArgs g) {
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
        R* base = g.work + (int64_t)c * PREFIX_ENV_BIG_MATS * gsz;
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
    // G^T is the 1 x 1 unit
    if (tid == 0) {
        if (c == 0) zstore<R, CX>(g.G + pfx_slot(T, 0, C, ls) * gsz, 0, R(1), R(0));
        g.lnG[(int64_t)T * C + c] = 0.0;
    }
    __syncthreads();
    double lg = 0.0;
    for (int j = T - 1; j >= 0; --j) {
        const SiteView<R> sv = site_view<R, CX>(v, j, c, false);
        const int Di = sv.Din, Do = sv.Dout;
        const bool keep = j <= ls || c == 0;
        R* dst = g.G + pfx_slot(j, c, C, ls) * gsz;
        double tr = 0.0;
        if constexpr (BIG) {
            const GMat<R> Rm{pRc, Di, 1, Di, Di};
            for (int s_ = 0; s_ < d; ++s_) {
                const GMat<R> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};     // W_j[s], read in place
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
            // the class state vanished (or is not finite) from here on: every prefix that needs these tables is -inf
            for (int jj = j; jj >= 0; --jj) {
                if (tid == 0) g.lnG[(int64_t)jj * C + c] = -INFINITY;
                if (jj <= ls || c == 0) {
                    R* z = g.G + pfx_slot(jj, c, C, ls) * gsz;
                    const int Dj = v.chi[jj];
                    for (int e = tid; e < Dj * Dj * ZW; e += IMP_T) z[e] = R(0);
                }
            }
            return;
        }
        lg += log(tr);
        if (tid == 0) g.lnG[(int64_t)j * C + c] = lg;
    }
}

template <bool CX> __global__ __launch_bounds__(SC_T) void k_prefix_score(ImpModel v, PrefixArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double Xr[SC_B * SC_LD], Xi[CX ? SC_B * SC_LD : 1];
    __shared__ double phr[SC_B * SC_PS], phi_[CX ? SC_B * SC_PS : 1];
    __shared__ double wd[4 * SC_B];                     // the waves' parts of the row dots
    __shared__ double lgs[(PFX_MAXC + 1) * SC_B];       // ln(norm^2) summed over the sites: [0] the shared rows, [1 + c] the rows of class c
    const int T = v.T, d = v.d, cm = v.cap, C = g.C, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t start = (int64_t)blockIdx.x * SC_B;               // chunk-local
    const int count = (int)min((int64_t)SC_B, g.count - start);
    const int64_t inst0 = g.first + start;
    const int ls = *v.label_site;
    const int64_t gsz = (int64_t)cm * cm * ZW;
    double* crows = g.crows + (int64_t)blockIdx.x * (C + 1) * SC_B * cm * ZW;
    const int orow = tid >> 4, osub = tid & 15;                     // sixteen threads per row outside the products

    auto load_phi = [&](int j) {
        for (int e = tid; e < SC_B * d; e += SC_T) {
            const int row = e / d, s = e - row * d;
            double pr = 0.0, pi = 0.0;
            if (row < count) zload<double, CX>((const double*)v.phi, ((int64_t)j * v.N + inst0 + row) * d + s, pr, pi);
            phr[row * SC_PS + s] = pr;
            if constexpr (CX) phi_[row * SC_PS + s] = pi;
        }
    };
    // V = X . B for this wave's column tiles, B(k, col) = B[off + k * sk + col * sc] (pairs: complex), Din x Dout live
    auto xmul = [&](const double* __restrict__ B, int64_t off, int64_t sk, int64_t sc, int Din, int Dout, d4 (&vr)[SC_NTW], d4 (&vi)[SC_NTW]) {
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            vr[u] = d4{0.0, 0.0, 0.0, 0.0};
            vi[u] = d4{0.0, 0.0, 0.0, 0.0};
            if ((wave + 4 * u) * 16 >= Dout) continue;              // (wave-uniform)
            const int col = (wave + 4 * u) * 16 + i16;
            const bool cv = col < Dout;
            const int64_t wb = off + (int64_t)col * sc;
            for (int k0 = 0; k0 < Din; k0 += 4 * SC_KU) {           // SC_KU k-steps of the operand in flight, then their products
                double wr[SC_KU], wi[SC_KU];
#pragma unroll
                for (int q = 0; q < SC_KU; ++q) {
                    const int k = k0 + 4 * q + kq;
                    wr[q] = wi[q] = 0.0;
                    if (cv && k < Din) zload<double, CX>(B, wb + (int64_t)k * sk, wr[q], wi[q]);
                }
#pragma unroll
                for (int q = 0; q < SC_KU; ++q) {
                    if (k0 + 4 * q >= Din) break;
                    const int k = k0 + 4 * q + kq;                  // (k < Din + 3: inside the row, times a zero of the operand)
                    const double xr = Xr[i16 * SC_LD + k];
                    vr[u] = mfma_f64(xr, wr[q], vr[u]);
                    if constexpr (CX) {
                        const double xi = Xi[i16 * SC_LD + k];
                        vr[u] = mfma_f64(-xi, wi[q], vr[u]);
                        vi[u] = mfma_f64(xr, wi[q], vi[u]);
                        vi[u] = mfma_f64(xi, wr[q], vi[u]);
                    }
                }
            }
        }
    };
    // one site: the rows become sum_s conj(phi_s) (.) (X W_j[:, s, :]) for the class block `cls` of the label site.  Barriers: the caller has
    // synchronised X and the site vectors; the rows are in place after the caller's next barrier.
    auto step = [&](int j, int cls) -> int {
        const SiteView<double> sv = site_view<double, CX>(v, j, cls, true);
        d4 outr[SC_NTW], outi[SC_NTW];
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            outr[u] = d4{0.0, 0.0, 0.0, 0.0};
            outi[u] = d4{0.0, 0.0, 0.0, 0.0};
        }
        for (int s = 0; s < d; ++s) {
            d4 vr[SC_NTW], vi[SC_NTW];
            xmul(sv.W, (int64_t)s * sv.ss, sv.si, sv.so, sv.Din, sv.Dout, vr, vi);
#pragma unroll
            for (int u = 0; u < SC_NTW; ++u) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = kq + 4 * r;
                    const double pr = phr[row * SC_PS + s];
                    outr[u][r] = fma(pr, vr[u][r], outr[u][r]);
                    if constexpr (CX) {
                        const double pi = phi_[row * SC_PS + s];
                        outr[u][r] = fma(pi, vi[u][r], outr[u][r]);
                        outi[u][r] = fma(pr, vi[u][r], outi[u][r]);
                        outi[u][r] = fma(-pi, vr[u][r], outi[u][r]);
                    }
                }
            }
        }
        __syncthreads();                    // every wave is done with the rows
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            if ((wave + 4 * u) * 16 >= sv.Dout) continue;
            const int col = (wave + 4 * u) * 16 + i16;                  // (columns beyond Dout: exact zeros)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xr[(kq + 4 * r) * SC_LD + col] = outr[u][r];
                if constexpr (CX) Xi[(kq + 4 * r) * SC_LD + col] = outi[u][r];
            }
        }
        return sv.Dout;
    };
    // the rows in LDS to norm one, ln(norm^2) to the accumulators of slot `to` (which start from those of slot `from`); a row whose norm is
    // not a positive finite number is zeroed: all its later prefixes are -inf
    auto rescale = [&](int D, int from, int to) {
        double n2 = 0.0;
        for (int cc = osub; cc < D; cc += 16) {
            const double xr = Xr[orow * SC_LD + cc];
            n2 = fma(xr, xr, n2);
            if constexpr (CX) {
                const double xi = Xi[orow * SC_LD + cc];
                n2 = fma(xi, xi, n2);
            }
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) n2 += __shfl_xor(n2, o);
        const bool ok = n2 > 0.0 && n2 < INFINITY;
        const double sc = ok ? 1.0 / sqrt(n2) : 0.0;
        for (int cc = osub; cc < SC_LD; cc += 16) {
            const bool live = ok && cc < D;
            Xr[orow * SC_LD + cc] = live ? Xr[orow * SC_LD + cc] * sc : 0.0;
            if constexpr (CX) Xi[orow * SC_LD + cc] = live ? Xi[orow * SC_LD + cc] * sc : 0.0;
        }
        if (osub == 0) lgs[to * SC_B + orow] = ok ? lgs[from * SC_B + orow] + log(n2) : 0.0;
    };
    // ln l_c(.; t) of the rows in LDS (bond t, accumulators of slot `slot`) into the block's results.  Barriers: the caller has synchronised X.
    auto score = [&](int t, int c, int slot) {
        const int D = v.chi[t];
        d4 yr[SC_NTW], yi[SC_NTW];
        xmul(g.G + pfx_slot(t, c, C, ls) * gsz, 0, D, 1, D, D, yr, yi);
        double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            const int col = (wave + 4 * u) * 16 + i16;
            if (col >= D) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = fma(yr[u][r], Xr[(kq + 4 * r) * SC_LD + col], p[r]);
                if constexpr (CX) p[r] = fma(yi[u][r], Xi[(kq + 4 * r) * SC_LD + col], p[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double x = sum16(p[r]);
            if (i16 == 0) wd[wave * SC_B + kq + 4 * r] = x;
        }
        __syncthreads();
        if (tid < count) {
            const double q = (wd[0 * SC_B + tid] + wd[1 * SC_B + tid]) + (wd[2 * SC_B + tid] + wd[3 * SC_B + tid]);
            const double lp = (q > 0.0 && q < INFINITY) ? log(q) + lgs[slot * SC_B + tid] + g.lnG[(int64_t)t * C + c] : -INFINITY;
            g.logp[((start + tid) * (int64_t)(T + 1) + t) * C + c] = lp == lp ? lp : -INFINITY;
        }
        __syncthreads();
    };
    // the rows between LDS and slot `slot` of the workgroup's scratch (D live columns; the rest of an LDS row is zeroed)
    auto store_rows = [&](int slot, int D) {
        for (int cc = osub; cc < D; cc += 16) {
            double xi = 0.0;
            if constexpr (CX) xi = Xi[orow * SC_LD + cc];
            zstore<double, CX>(crows, ((int64_t)slot * SC_B + orow) * cm + cc, Xr[orow * SC_LD + cc], xi);
        }
    };
    auto load_rows = [&](int slot, int D) {
        for (int cc = osub; cc < SC_LD; cc += 16) {
            double xr = 0.0, xi = 0.0;
            if (cc < D) zload<double, CX>(crows, ((int64_t)slot * SC_B + orow) * cm + cc, xr, xi);
            Xr[orow * SC_LD + cc] = xr;
            if constexpr (CX) Xi[orow * SC_LD + cc] = xi;
        }
    };

    for (int e = tid; e < SC_B * SC_LD; e += SC_T) {
        Xr[e] = (e % SC_LD) == 0 ? 1.0 : 0.0;
        if constexpr (CX) Xi[e] = 0.0;
    }
    if (tid < SC_B) lgs[tid] = 0.0;
    __syncthreads();
    for (int j = 0; j < T; ++j) {
        // prefix j while the rows are shared: every class has its own G
        if (j <= ls)
            for (int c = 0; c < C; ++c) score(j, c, 0);
        load_phi(j);
        __syncthreads();
        if (j < ls) {
            const int Dout = step(j, 0);
            __syncthreads();
            rescale(Dout, 0, 0);
            __syncthreads();
            continue;
        }
        // from the label site on: a row per (series, class); prefix j + 1 right after the step of class c
        const int Din = v.chi[j];
        if (j == ls) {
            store_rows(C, Din);
            __threadfence_block();
            __syncthreads();
        }
        for (int c = 0; c < C; ++c) {
            load_rows(j == ls ? C : c, Din);
            __syncthreads();
            const int Dout = step(j, c);
            __syncthreads();
            rescale(Dout, j == ls ? 0 : 1 + c, 1 + c);
            __syncthreads();
            score(j + 1, c, 1 + c);
            store_rows(c, Dout);
            __threadfence_block();
            __syncthreads();
        }
    }
}
