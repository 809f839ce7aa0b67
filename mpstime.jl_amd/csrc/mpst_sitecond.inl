// Leave-one-out site conditionals (included by mpst_impute.hip): for a COMPLETE series i and every site t the distribution of x_t
// given all the other values, p(x_t | x_{!=t}), under the label slice c_i of the model.  With every other site known the conditioned
// state is pure: with M_j = sum_q conj(phi[i][j][q]) W_j[:, q, :] (the projection of precondition, MPS_methods.jl:42-99)
//     l_{-1} = 1, l_j = l_{j-1} M_j;   r_T = 1, r_j = M_j r_{j+1};   a_t[s] = sum_ab l_{t-1}[a] W_t[a, s, b] r_{t+1}[b],
// and p_k = |sum_s conj(g_k[s]) a_t[s]|^2 on the grid states g_k of site t is what k_imp_left forms for an instance whose only
// missing site is t, up to a constant factor: for rho = a a^H the reference's |rho phi|^2 and the Born value phi^H rho phi differ by
// |a|^2, which cancels in everything normalised.  Two vector walks per series (N T d chi^2) replace T environment passes (N T^2 d chi^2).
//
// k_sc_walk: sixteen instances per workgroup, four waves.  A chain step is, for every physical index s, the product
//     v_s (16 x Dout) = X (16 x Din) . W_j[:, s, :] (Din x Dout)          on v_mfma_f64_16x16x4_f64,
// X the sixteen environment rows (LDS), a wave per 16-column tile of the output (two tiles per wave up to chi = 128), and
// out = sum_s conj(phi_s) (.) v_s row by row: the Khatri-Rao product of k_score_walk_b with the sum over s taken after the matrix
// product instead of inside it - the same d chi / 4 MFMAs per tile, and no 16 x d chi tile in LDS.  The B operand is read where the
// tensor lies (L2), with the strides of the walk's direction, as gmem_mm does beyond the LDS limit of the environment pass: one
// route for every chi <= 128.  The left rows l_{t-1} of every site go to global scratch ([T][16][chi] per workgroup); the right walk
// then runs on the fly: its v_s = W_t[:, s, :] r_{t+1} gives a_t[s] (dot with l_{t-1}, 16 lanes, then the tiles in a fixed order) and
// r_t (the sum over s) from one product.  At the label site the step runs once per class present in the tile and a row keeps the
// result of its own class block.  Every site rescales every row by its largest magnitude; a row does not see its neighbours, so a
// series gives the same bits whichever rows travel with it.
//
// k_sc_grid: a workgroup per (series, site) pair at a time: the amplitudes on the grid (the site's own table where there is one per
// site), then k_imp_left's table-path routines - grid_prefix_sums, grid_quantile, grid_wmad, grid_cdf_at - for the median, the
// levels, the WMAD (and which of the two grid values at its distance weighted_median names) and the cdf at the observed value; nll at the exact encoded state.  A site whose Z is not a positive finite
// number gives NaN in its outputs.
constexpr int SC_B = 16;                    // instances per workgroup
constexpr int SC_T = 256;                   // four waves
constexpr int SC_LD = CAP_LIMIT + 2;        // row stride of the environment rows in LDS
constexpr int SC_NTW = CAP_LIMIT / 64;      // column tiles per wave
constexpr int SC_PS = IMP_MAXD + 1;         // row stride of the site vectors / the partial dots
constexpr int SC_KU = 8;                    // k-steps per batch of loads of the site tensor

// The walk of both callers, Args = ScArgs or WinArgs (first, count, lrows).  KEEP_R (window conditionals, mpst_window.inl): lrows has
// 2 T slots per workgroup, the right walk stores its rescaled rows as the left walk does - slot T + j holds r~_{j+1}, what closes a
// window that ends at site j - and forms no amplitudes.
template <bool CX, bool KEEP_R, typename Args> __device__ __forceinline__ void sc_walk(const ImpModel& v, const Args& g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double Xr[SC_B * SC_LD], Xi[CX ? SC_B * SC_LD : 1];
    __shared__ double phr[SC_B * SC_PS], phi_[CX ? SC_B * SC_PS : 1];
    __shared__ double wdr[4 * SC_B * SC_PS], wdi[CX ? 4 * SC_B * SC_PS : 1];
    __shared__ int lab[SC_B];
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t start = (int64_t)blockIdx.x * SC_B;               // chunk-local
    const int count = (int)min((int64_t)SC_B, g.count - start);
    const int64_t inst0 = g.first + start;
    const int ls = *v.label_site;
    double* lrows = g.lrows + (int64_t)blockIdx.x * (KEEP_R ? 2 : 1) * T * SC_B * cm * ZW;
    if (tid < SC_B) lab[tid] = tid < count ? v.label[inst0 + tid] : -1;
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
    auto unit_rows = [&]() {
        for (int e = tid; e < SC_B * SC_LD; e += SC_T) {
            Xr[e] = (e % SC_LD) == 0 ? 1.0 : 0.0;
            if constexpr (CX) Xi[e] = 0.0;
        }
    };
    // the rows in LDS, each divided by its largest magnitude (a row of zeros, or one that is not finite, stays); `keep`: slot of lrows
    auto rescale = [&](int Dout, int keep) {
        double mx = 0.0;
        for (int c = osub; c < Dout; c += 16) {
            mx = fmax(mx, fabs(Xr[orow * SC_LD + c]));
            if constexpr (CX) mx = fmax(mx, fabs(Xi[orow * SC_LD + c]));
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        const double sc = (mx > 0.0 && mx < INFINITY) ? 1.0 / mx : 1.0;
        for (int c = osub; c < Dout; c += 16) {
            double xr = Xr[orow * SC_LD + c] * sc, xi = 0.0;
            if constexpr (CX) xi = Xi[orow * SC_LD + c] * sc;
            Xr[orow * SC_LD + c] = xr;
            if constexpr (CX) Xi[orow * SC_LD + c] = xi;
            if (keep >= 0) zstore<double, CX>(lrows, ((int64_t)keep * SC_B + orow) * cm + c, xr, xi);
        }
    };
    // one site: out = sum_s conj(phi_s) (.) (X W_j[:, s, :]) into the rows; the right walk (t >= 0) also leaves the partial dots of
    // v_s with l_{t-1} in wd.  Barriers: the caller has synchronised X and the site vectors.
    auto step = [&](int j, bool left, int t) {
        d4 outr[SC_NTW], outi[SC_NTW];
        double lr[SC_NTW][4], li[SC_NTW][4];
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            outr[u] = d4{0.0, 0.0, 0.0, 0.0};
            outi[u] = d4{0.0, 0.0, 0.0, 0.0};
        }
        const int Dl = v.chi[j], Dr = v.chi[j + 1];
        const int Din = left ? Dl : Dr, Dout = left ? Dr : Dl;
        if (t >= 0) {
#pragma unroll
            for (int u = 0; u < SC_NTW; ++u) {
                const int col = (wave + 4 * u) * 16 + i16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    lr[u][r] = li[u][r] = 0.0;
                    if (col < Dout) zload<double, CX>(lrows, ((int64_t)t * SC_B + kq + 4 * r) * cm + col, lr[u][r], li[u][r]);
                }
            }
        }
        const int ncls = j == ls ? 1 << 30 : 1;
        for (int c = 0; c < ncls; ++c) {
            if (j == ls) {
                // the classes present in the tile, in ascending order (uniform over the workgroup)
                int nx = 1 << 30;
                for (int r = 0; r < SC_B; ++r)
                    if (lab[r] >= c && lab[r] < nx) nx = lab[r];
                if (nx == (1 << 30)) break;
                c = nx;
            }
            const SiteView<double> sv = site_view<double, CX>(v, j, c, left);
            bool mine[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[r] = j != ls || lab[kq + 4 * r] == c;
            for (int s = 0; s < d; ++s) {
                double par[4] = {0.0, 0.0, 0.0, 0.0}, pai[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int u = 0; u < SC_NTW; ++u) {
                    const int col = (wave + 4 * u) * 16 + i16;
                    if ((wave + 4 * u) * 16 >= Dout) continue;          // (wave-uniform)
                    const bool cv = col < Dout;
                    d4 vr = {0.0, 0.0, 0.0, 0.0}, vi = {0.0, 0.0, 0.0, 0.0};
                    const int64_t wb = (int64_t)s * sv.ss + (int64_t)col * sv.so;
                    for (int k0 = 0; k0 < Din; k0 += 4 * SC_KU) {           // SC_KU k-steps of the tensor in flight, then their products
                        double wr[SC_KU], wi[SC_KU];
#pragma unroll
                        for (int q = 0; q < SC_KU; ++q) {
                            const int k = k0 + 4 * q + kq;
                            wr[q] = wi[q] = 0.0;
                            if (cv && k < Din) zload<double, CX>(sv.W, wb + (int64_t)k * sv.si, wr[q], wi[q]);
                        }
#pragma unroll
                        for (int q = 0; q < SC_KU; ++q) {
                            if (k0 + 4 * q >= Din) break;
                            const int k = k0 + 4 * q + kq;                  // (k < Din + 3: inside the row, times a zero of the tensor)
                            const double xr = Xr[i16 * SC_LD + k];
                            vr = mfma_f64(xr, wr[q], vr);
                            if constexpr (CX) {
                                const double xi = Xi[i16 * SC_LD + k];
                                vr = mfma_f64(-xi, wi[q], vr);
                                vi = mfma_f64(xr, wi[q], vi);
                                vi = mfma_f64(xi, wr[q], vi);
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = kq + 4 * r;
                        const double pr = phr[row * SC_PS + s];
                        if (mine[r]) {
                            outr[u][r] = fma(pr, vr[r], outr[u][r]);
                            if constexpr (CX) {
                                const double pi = phi_[row * SC_PS + s];
                                outr[u][r] = fma(pi, vi[r], outr[u][r]);
                                outi[u][r] = fma(pr, vi[r], outi[u][r]);
                                outi[u][r] = fma(-pi, vr[r], outi[u][r]);
                            }
                        }
                        if (t >= 0) {
                            par[r] = fma(lr[u][r], vr[r], par[r]);
                            if constexpr (CX) {
                                par[r] = fma(-li[u][r], vi[r], par[r]);
                                pai[r] = fma(lr[u][r], vi[r], pai[r]);
                                pai[r] = fma(li[u][r], vr[r], pai[r]);
                            }
                        }
                    }
                }
                if (t >= 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double xr = sum16(par[r]), xi = CX ? sum16(pai[r]) : 0.0;
                        if (i16 == 0 && mine[r]) {
                            wdr[(wave * SC_B + kq + 4 * r) * SC_PS + s] = xr;
                            if constexpr (CX) wdi[(wave * SC_B + kq + 4 * r) * SC_PS + s] = xi;
                        }
                    }
                }
            }
        }
        __syncthreads();                    // every wave is done with the rows
#pragma unroll
        for (int u = 0; u < SC_NTW; ++u) {
            if ((wave + 4 * u) * 16 >= Dout) continue;
            const int col = (wave + 4 * u) * 16 + i16;                  // (columns beyond Dout: exact zeros)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xr[(kq + 4 * r) * SC_LD + col] = outr[u][r];
                if constexpr (CX) Xi[(kq + 4 * r) * SC_LD + col] = outi[u][r];
            }
        }
        return Dout;
    };

    // ---- left walk: l_{j-1} into slot j, j = 0 .. T-1 ----
    unit_rows();
    __syncthreads();
    rescale(1, 0);
    for (int j = 0; j + 1 < T; ++j) {
        load_phi(j);
        __syncthreads();
        const int Dout = step(j, true, -1);
        __syncthreads();
        rescale(Dout, j + 1);
    }
    __threadfence_block();
    __syncthreads();
    if constexpr (KEEP_R) {
        // ---- right walk, kept: r_{t+1} into slot T + t, t = T-1 .. 0 ----
        unit_rows();
        __syncthreads();
        rescale(1, 2 * T - 1);
        for (int t = T - 1; t >= 1; --t) {
            load_phi(t);
            __syncthreads();
            const int Dout = step(t, false, -1);
            __syncthreads();
            rescale(Dout, T + t - 1);
            __syncthreads();
        }
    } else {
        // ---- right walk: a_t and r_t from one product, t = T-1 .. 0 ----
        unit_rows();
        for (int t = T - 1; t >= 0; --t) {
            load_phi(t);
            __syncthreads();
            const int Dout = step(t, false, t);
            // a_t[s]: the four waves' partial dots in a fixed order; conj(phi_t) . a_t over the sixteen lanes of the row
            {
                const int s = osub;
                double ar = 0.0, ai = 0.0;
                if (s < d) {
                    ar = (wdr[(0 * SC_B + orow) * SC_PS + s] + wdr[(1 * SC_B + orow) * SC_PS + s]) +
                         (wdr[(2 * SC_B + orow) * SC_PS + s] + wdr[(3 * SC_B + orow) * SC_PS + s]);
                    if constexpr (CX)
                        ai = (wdi[(0 * SC_B + orow) * SC_PS + s] + wdi[(1 * SC_B + orow) * SC_PS + s]) +
                             (wdi[(2 * SC_B + orow) * SC_PS + s] + wdi[(3 * SC_B + orow) * SC_PS + s]);
                }
                double pr = s < d ? phr[orow * SC_PS + s] : 0.0, pi = 0.0;
                if constexpr (CX) pi = s < d ? phi_[orow * SC_PS + s] : 0.0;
                double yr = pr * ar + pi * ai, yi = pr * ai - pi * ar;
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) {
                    yr += __shfl_xor(yr, o);
                    yi += __shfl_xor(yi, o);
                }
                if (orow < count) {
                    double* am = g.amp + ((start + orow) * T + t) * (int64_t)(d + 1) * ZW;
                    if (s < d) zstore<double, CX>(am, s, ar, ai);
                    if (s == 0) zstore<double, CX>(am, d, yr, yi);
                }
            }
            __syncthreads();
            rescale(Dout, -1);
            __syncthreads();
        }
    }
}
template <bool CX> __global__ __launch_bounds__(SC_T) void k_sc_walk(ImpModel v, ScArgs g) { sc_walk<CX, false>(v, g); }

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_sc_grid(ImpModel v, ScArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double red[4], wtot[4];
    __shared__ int isel[4];
    __shared__ double sar[IMP_MAXD + 1], sai[IMP_MAXD + 1];
    __shared__ double lev[IMP_MAXQ];
    const int T = v.T, d = v.d, tid = threadIdx.x, n = g.ngrid;
    double* p = g.pbuf + (int64_t)blockIdx.x * n;
    double* S = g.sbuf + (int64_t)blockIdx.x * n;
    const int nrow = (n + 63) >> 6, rpw = (nrow + 3) >> 2, quarter = rpw * 64;
    const double dx = g.grid_x[1] - g.grid_x[0];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid < g.nq) lev[tid] = g.levels[tid];
    for (int64_t pair = blockIdx.x; pair < g.count * T; pair += gridDim.x) {
        const int64_t il = pair / T, i = g.first + il;
        const int t = (int)(pair - il * T);
        __syncthreads();                    // the previous pair is done with p, S and the shared values
        if (tid <= d) {
            double ar, ai;
            zload<double, CX>(g.amp + pair * (d + 1) * ZW, tid, ar, ai);
            sar[tid] = ar;
            sai[tid] = ai;
        }
        __syncthreads();
        // the amplitudes at their largest magnitude one: p, Z and the numerator scale alike
        double amax = 0.0;
        for (int s = 0; s < d; ++s) amax = fmax(amax, fmax(fabs(sar[s]), fabs(sai[s])));
        const double asc = (amax > 0.0 && amax < INFINITY) ? 1.0 / amax : 1.0;
        double pmax = -1.0;
        int kmax = 0;
        {
            const double* gp = g.grid_phi + (int64_t)t * g.grid_site_stride;
            double ar[IMP_MAXD], ai[IMP_MAXD];
#pragma unroll
            for (int s = 0; s < IMP_MAXD; ++s) {
                ar[s] = s < d ? sar[s] * asc : 0.0;
                ai[s] = (CX && s < d) ? sai[s] * asc : 0.0;
            }
            for (int k = tid; k < n; k += IMP_T) {
                double qr = 0.0, qi = 0.0;
#pragma unroll
                for (int s = 0; s < IMP_MAXD; ++s) {
                    if (s < d) {
                        double fr, fi;
                        zload<double, CX>(gp, (int64_t)k * d + s, fr, fi);
                        qr = fma(fr, ar[s], qr);                // conj(g) a
                        if constexpr (CX) {
                            qr = fma(fi, ai[s], qr);
                            qi = fma(fr, ai[s], qi);
                            qi = fma(-fi, ar[s], qi);
                        }
                    }
                }
                const double pk = fma(qr, qr, qi * qi);
                p[k] = pk;
                if (pk > pmax) {
                    pmax = pk;
                    kmax = k;
                }
            }
        }
        __threadfence_block();
        __syncthreads();
        grid_prefix_sums(p, S, n, nrow, rpw, wtot);
        __threadfence_block();
        __syncthreads();
        const GridSums tab{S, quarter, wtot[0], wtot[0] + wtot[1], (wtot[0] + wtot[1]) + wtot[2]};
        const double Stot = tab.w3 + wtot[3], p0 = p[0];
        auto Sabs = [&](int k) { return tab.at(k); };
        auto cdf_at = [&](int k) { return grid_cdf_at(k, dx, p0, Sabs); };
        const double Z = cdf_at(n - 1);
        const int64_t o = i * T + t;
        if (!(Z > 0.0 && Z < INFINITY)) {           // (uniform over the workgroup)
            if (tid == 0) {
                if (g.nll) g.nll[o] = qnan;
                if (g.pit) g.pit[o] = qnan;
                if (g.med) g.med[o] = qnan;
                if (g.err) g.err[o] = qnan;
                for (int l = 0; l < g.nq; ++l) g.q[o * g.nq + l] = qnan;
            }
            continue;
        }
        if (g.med || g.err) {
            const int kmed = grid_quantile(0.5, Z, n, nrow, isel, cdf_at);
            double err = 0.0;
            if (g.err && g.get_err) {
                int jt;
                err = grid_wmad(kmed, g.grid_x, Stot, Z, n, nrow, isel, Sabs, [&](double mid, int& km) {
                    double gm;
                    km = grid_arg_pmax(pmax, kmax, n, red, isel, gm);
                    return gm / Z > mid;
                }, jt);
                // Which of the two grid values at the tipping distance: grid_wmad names the lower one, whose deviation from the
                // median equals the upper one's in exact arithmetic.  On a grid that is not made of exact doubles the two
                // deviations are doubles a few 1e-16 apart, and this call's contract is weighted_median itself: the stable sort
                // takes the smaller deviation first (the lower index on a tie), and the result is the one of the pair at which the
                // cumulative weight passes half the total.
                const int lo = kmed - jt, hi = kmed + jt;
                if (jt >= 1 && lo >= 0 && hi <= n - 1) {
                    const double xc = g.grid_x[kmed], vlo = fabs(g.grid_x[lo] - xc), vhi = fabs(g.grid_x[hi] - xc);
                    const bool lo_first = vlo <= vhi;
                    const double before = Sabs(hi - 1) - Sabs(lo), mid = 0.5 * (Stot / Z);
                    const bool first_tips = (before + p[lo_first ? lo : hi]) / Z > mid;
                    err = (first_tips == lo_first) ? vlo : vhi;
                }
            }
            if (tid == 0) {
                if (g.med) g.med[o] = g.grid_x[kmed];
                if (g.err) g.err[o] = err;
            }
        }
        for (int l = 0; l < g.nq; ++l) {
            const int kl = grid_quantile(lev[l], Z, n, nrow, isel, cdf_at);
            if (tid == 0) g.q[o * g.nq + l] = g.grid_x[kl];
        }
        if (tid == 0) {
            if (g.nll) {
                const double yr = sar[d] * asc, yi = sai[d] * asc;
                g.nll[o] = -log(fma(yr, yr, yi * yi) / Z);
            }
            if (g.pit) {
                // F at the observed value, linear between its two neighbours on the grid
                const double x = g.x[o], x0 = g.grid_x[0], x1 = g.grid_x[n - 1];
                double F;
                if (!(x > x0)) F = x == x0 || x < x0 ? 0.0 : qnan;
                else if (!(x < x1)) F = 1.0;
                else {
                    int k = (int)((x - x0) / dx);
                    k = max(0, min(n - 2, k));
                    while (k > 0 && g.grid_x[k] > x) --k;
                    while (k < n - 2 && g.grid_x[k + 1] <= x) ++k;
                    const double xa = g.grid_x[k], xb = g.grid_x[k + 1], Fa = cdf_at(k) / Z, Fb = cdf_at(k + 1) / Z;
                    F = Fa + (Fb - Fa) * ((x - xa) / (xb - xa));
                }
                g.pit[o] = F;
            }
        }
    }
}
