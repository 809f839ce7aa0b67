// Window conditionals (included by mpst_impute.hip): for a COMPLETE series i of class c_i, a start t and every width w <= max_width with
// t + w <= T, the negative log Born probability of the window's values given all the others,
//     nll[i][t][w-1] = ln l_c(i; {t, ..., t+w-1}) - ln l_c(i; {}),
// l_c(i; M) the marginal likelihood of mpst_marginal.inl with the sites in M summed over their physical index.  With the rows of the
// leave-one-out walk (mpst_sitecond.inl) in hand - l_{t-1} before the window, r_{t+w} behind it - only the window itself is
// marginalised, and the width w + 1 is one more step of the recursion the width w ended with:
//     x_0 = l_{t-1},          x_k = x_{k-1} M_{t+k-1}                                        (the known values: a vector)
//     E_0 = x_0 x_0^H,        E_k = sum_s W_{t+k-1}[:, s, :]^T E_{k-1} conj(W_{t+k-1}[:, s, :])   (the values summed out: a density)
//     nll[i][t][k-1] = ln(r_{t+k}^T E_k conj(r_{t+k})) - ln |x_k . r_{t+k}|^2.
// One pass of max_width steps per start gives every width: N T max_width d chi^3 against the N T^2 max_width d chi^3 of one marginal
// chain per window.  x is rescaled to norm one and E to trace one at every step, their logarithms accumulated in fp64; the scales of
// the walk's rows l~, r~ (each divided by its largest magnitude) are the same in both terms and cancel.
//
// k_win_walk: sc_walk with KEEP_R - both rows of every site of every series to global scratch ([2 T][16][chi] per workgroup).
// k_win: a workgroup of 256 threads per (series, start) pair at a time, the grid capped and strided over the pairs.  The vector step is
// k_marginal's (mrg_site_matrix + mrg_matvec).  The matrix step, up to the LDS limit of the environment pass: E, the site matrix and
// T1 = A E in LDS as zero-padded (re, im) planes, two lds_tile_rows products per physical index, a wave per 16 x 16 tile; beyond it
// (BIG): gmem_mm in WINDOW_BIG_MATS chi x chi matrices of global scratch per workgroup, W_j[s] read in place.  The closing is a
// quadratic form with a vector, so no R is kept.  At the label site the tensor is the block of the series' class.  One lane stores
// each width with a plain store; every reduction has one order, and a pair does not see what travels with it.
// Degenerate cases: |x_k . r|^2 = 0 gives +inf; a trace or a closing form that is not a positive finite number gives NaN for that width
// and the wider ones of the same start, and so does a row l~_{t-1} without a norm; entries with t + w > T are NaN.
template <bool CX> __global__ __launch_bounds__(SC_T) void k_win_walk(ImpModel v, WinArgs g) {
    sc_walk<CX, true>(v, g);
}

template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_win(ImpModel v, WinArgs g) {
    using acc_t = typename Mx<double>::acc_t;
    using Mat = MrgMat<double, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    __shared__ double xs[2][2][CAP_LIMIT];      // the vector: [current / next][re / im]
    __shared__ double rs[2][CAP_LIMIT];         // the right row that closes the current width
    constexpr int ZW = CX ? 2 : 1;
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int ls = *v.label_site, mw = g.max_width;
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 2;                      // as in k_marginal: rows 16-byte aligned and 4 banks apart
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double *pRc, *pRn = nullptr, *pMs, *pT1;    // E, (global scratch) E', the site matrix, T1 = A E
    if constexpr (BIG) {
        const int64_t bsz = (int64_t)cm * cm * ZW;
        double* base = g.work + (int64_t)blockIdx.x * WINDOW_BIG_MATS * bsz;
        pRc = base;
        pRn = base + bsz;
        pMs = base + 2 * bsz;
        pT1 = base + 3 * bsz;
    } else {
        double* smem = reinterpret_cast<double*>(smem_raw);
        pRc = smem;
        pMs = smem + ZW * msz;
        pT1 = smem + 2 * ZW * msz;
        for (int e = tid; e < 3 * ZW * msz; e += IMP_T) smem[e] = 0.0;
    }
    auto mat = [&](double* p, int cols) { return Mat{p, BIG ? cols : ld, BIG ? 0 : msz}; };
    auto plane = [&](double* p) { return Plane<double>{p, p + (ZW - 1) * msz}; };

    // E <- sum_s A[s] E A[s]^H / trace through the site `sv`, A[s] = W_j[s]^T; returns the trace (E is left alone unless it is a positive
    // finite number)
    auto mat_step = [&](const SiteView<double>& sv) -> double {
        const int Di = sv.Din, Do = sv.Dout;
        double out = 0.0;
        if constexpr (BIG) {
            const GMat<double> Rm{pRc, Di, 1, Di, Di};
            for (int s_ = 0; s_ < d; ++s_) {
                const GMat<double> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};
                gmem_mm<double, CX>(pT1, Di, A, Rm, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<double, CX>(pRn, Do, GMat<double>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            }
            for (int a_ = tid; a_ < Do; a_ += IMP_T) out += pRn[((int64_t)a_ * Do + a_) * ZW];
            out = blk_sum(out, red);
            if (!(out > 0.0 && out < INFINITY)) return out;
            const double sc = 1.0 / out;
            for (int e = tid; e < Do * Do * ZW; e += IMP_T) pRn[e] *= sc;
            __syncthreads();
            double* tmp = pRc;
            pRc = pRn;
            pRn = tmp;
            return out;
        } else {
            const Plane<double> Rcp = plane(pRc), Msp = plane(pMs), T1p = plane(pT1);
            const int tmo = (Do + 15) >> 4, tni = (Di + 15) >> 4;
            acc_t accr[MRG_NTW], acci[MRG_NTW];
#pragma unroll
            for (int t = 0; t < MRG_NTW; ++t) {
                accr[t] = acc_t{0, 0, 0, 0};
                acci[t] = acc_t{0, 0, 0, 0};
            }
            for (int s_ = 0; s_ < d; ++s_) {
                mrg_site_matrix<double, CX, BIG>(mat(pMs, Di), cp, sv, nullptr, s_, d, true);
                __syncthreads();
                // T1 = A E^H = A E (Do x Di); the tiles beyond it are zeroed
#pragma unroll
                for (int t = 0; t < MRG_NTW; ++t) {
                    const int tile = wave + 4 * t;
                    if (tile < ntile) {
                        const int rb = tile / tpr, wc = tile - rb * tpr;
                        acc_t ar = {0, 0, 0, 0}, ai = {0, 0, 0, 0};
                        if (rb < tmo && wc < tni) lds_tile_rows<double, CX>(ar, ai, Msp, 16 * rb, Rcp, 16 * wc, ks, ld);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int at = (16 * rb + Mx<double>::row(kq, r)) * ld + 16 * wc + i16;
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
                        if (rb < tmo && wc < tmo) lds_tile_rows<double, CX>(accr[t], acci[t], T1p, 16 * rb, Msp, 16 * wc, ks, ld);
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
                if (rb != wc || rb >= tmo) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rb + Mx<double>::row(kq, r), col = 16 * wc + i16;
                    if (row == col && row < Do) out += accr[t][r];
                }
            }
            out = blk_sum(out, red);
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
                    const int row = 16 * rb + Mx<double>::row(kq, r), col = 16 * wc + i16;
                    const bool live = have && row < Do && col < Do;
                    Rcp.r[row * ld + col] = live ? accr[t][r] * sc : 0.0;
                    if constexpr (CX) Rcp.i[row * ld + col] = live ? acci[t][r] * sc : 0.0;
                }
            }
            __syncthreads();
            return out;
        }
    };

    const int64_t npair = g.count * T;
    for (int64_t pair = blockIdx.x; pair < npair; pair += gridDim.x) {
        const int64_t il = pair / T, i = g.first + il;
        const int t = (int)(pair - il * T);
        const int64_t tile = il / SC_B;
        const int row = (int)(il - tile * SC_B);
        const int cls = v.label[i];
        const int nw = min(mw, T - t);
        double* out = g.nll + (il * T + t) * (int64_t)mw;
        __syncthreads();                        // the previous pair is done with the vectors and the matrices
        // x_0 = l~_{t-1} at norm one, E_0 = x_0 x_0^H
        int D = v.chi[t], cur = 0, k = 0;
        {
            double xr = 0.0, xi = 0.0;
            if (tid < D) zload<double, CX>(g.lrows, ((2 * tile * T + t) * SC_B + row) * cm + tid, xr, xi);
            const double n2 = blk_sum(xr * xr + xi * xi, red);
            if (n2 > 0.0 && n2 < INFINITY) {
                const double sc = 1.0 / sqrt(n2);
                if (tid < D) {
                    xs[0][0][tid] = xr * sc;
                    xs[0][1][tid] = xi * sc;
                }
                __syncthreads();
                mrg_outer<double, CX, BIG>(mat(pRc, D), cp, D, xs[0][0], xs[0][1]);
                __syncthreads();
                k = 1;
            }
        }
        double lgx = 0.0, lgE = 0.0;
        bool xzero = false, xbad = false;       // the vector vanished (every wider window: +inf) / lost its norm (NaN)
        for (; k >= 1 && k <= nw; ++k) {
            const int j = t + k - 1;
            const SiteView<double> sv = site_view<double, CX>(v, j, j == ls ? cls : 0, true);
            const double* ph = (const double*)v.phi + ((int64_t)j * v.N + i) * d * ZW;
            const int Di = sv.Din, Do = sv.Dout;
            if (tid < Do) {
                double rr, ri;
                zload<double, CX>(g.lrows, (((2 * tile + 1) * T + j) * SC_B + row) * cm + tid, rr, ri);
                rs[0][tid] = rr;
                rs[1][tid] = ri;
            }
            if (!xzero && !xbad) {              // x <- x M_j
                const Mat M = mat(pMs, Di);
                mrg_site_matrix<double, CX, BIG>(M, cp, sv, ph, 0, d, false);
                __syncthreads();
                mrg_matvec<double, CX, BIG>(M, Do, Di, xs[cur][0], xs[cur][1], xs[cur ^ 1][0], xs[cur ^ 1][1]);
                __syncthreads();
                double nr = 0.0, ni = 0.0;
                if (tid < Do) {
                    nr = xs[cur ^ 1][0][tid];
                    if constexpr (CX) ni = xs[cur ^ 1][1][tid];
                }
                const double n2 = blk_sum(nr * nr + ni * ni, red);
                if (n2 == 0.0) xzero = true;
                else if (!(n2 > 0.0 && n2 < INFINITY)) xbad = true;
                else {
                    lgx += log(n2);
                    const double sc = 1.0 / sqrt(n2);
                    if (tid < Do) {
                        xs[cur ^ 1][0][tid] = nr * sc;
                        if constexpr (CX) xs[cur ^ 1][1][tid] = ni * sc;
                    }
                    cur ^= 1;
                }
                __syncthreads();
            }
            const double tr = mat_step(sv);
            if (!(tr > 0.0 && tr < INFINITY)) break;
            lgE += log(tr);
            // r^T E conj(r) (real: E is Hermitian) and x . r
            const Mat E = mat(pRc, Do);
            double q = 0.0, ar = 0.0, ai = 0.0;
            for (int e = tid; e < Do * Do; e += IMP_T) {
                const int a_ = e / Do, b_ = e - a_ * Do;
                double er, ei;
                E.get(a_, b_, er, ei);
                const double zr = CX ? fma(rs[1][a_], rs[1][b_], rs[0][a_] * rs[0][b_]) : rs[0][a_] * rs[0][b_];
                q = fma(zr, er, q);
                if constexpr (CX) q = fma(-fma(rs[1][a_], rs[0][b_], -rs[0][a_] * rs[1][b_]), ei, q);
            }
            if (tid < Do) {
                const double yr = xs[cur][0][tid], ur = rs[0][tid];
                ar = yr * ur;
                if constexpr (CX) {
                    const double yi = xs[cur][1][tid], ui = rs[1][tid];
                    ar -= yi * ui;
                    ai = yr * ui + yi * ur;
                }
            }
            q = blk_sum(q, red);
            ar = blk_sum(ar, red);
            if constexpr (CX) ai = blk_sum(ai, red);
            if (!(q > 0.0 && q < INFINITY)) break;
            const double den = xzero ? 0.0 : ar * ar + ai * ai;
            if (tid == 0) out[k - 1] = xbad ? qnan : (den == 0.0 ? INFINITY : (log(q) + lgE) - (log(den) + lgx));
        }
        // the widths a degenerate step ended, and those beyond the end of the chain
        if (tid == 0)
            for (int w = max(k, 1); w <= mw; ++w) out[w - 1] = qnan;
    }
}
