// Rolling-origin forecasts (included by mpst_impute.hip): for every series i, every origin t = 0 .. T-1 and every horizon h = 1 .. H with
// u = t + h - 1 < T the distribution of x_u given x_0 .. x_{t-1} only, the sites t .. T-1 but u summed out (the Born rule of
// mpst_marginal_conditionals on the suffix mask of t, read at site u),
//     rho_c[s, s'] = x_t^c K_c^{t,u}[s, s'] (x_t^c)^H,
//     x_t^c        the row walk of k_prefix_score through the known sites 0 .. t-1 of the label slice c,
//     K_c^{u,u}[s, s'] = W_u[:, s, :] G_c^{u+1} W_u[:, s', :]^H                    (G: the table of k_prefix_env)
//     K_c^{t,u}[s, s'] = sum_q W_t[:, q, :] K_c^{t+1,u}[s, s'] W_t[:, q, :]^H     (site t summed out),
// which depends on the model only.  sum_s K^{t,u}[s, s] = G^t for every u, so every step of a chain is divided by the model-only factor
// exp(lnG[t] - lnG[t+1]) of k_prefix_env and the log scale of K_c^{t,.} is lnG[t][c], whatever u: no chain talks to another.
//
// k_roll_rows: sixteen series per workgroup, the row step of k_prefix_score (X . W_j[:, s, :] on v_mfma_f64_16x16x4_f64, then sum_s
// conj(phi_s) (.) row by row, every row rescaled to norm one at every site with an fp64 log accumulator).  The tile is walked once per
// class that one of its rows asks for (its label, or every class for a mixture row): the normalised x_t^c of every origin and its log go
// to scratch, [chunk][T][C][cap] and [chunk][T][C].  A row whose norm is not a positive finite number is zeroed and its log is -inf from
// there on.
// k_roll_tables: a workgroup per (target u, class, pair s <= s') chain at a time pushes its matrix back H - 1 sites.  The matrix is not
// Hermitian for s != s': the step is the plain order A (K A^H), both products by gmem_mm with W_t[q] and the previous matrix read where
// they lie and one matrix of global scratch per workgroup.  K^{t,u}[s', s] is the conjugate transpose and is not formed.
// k_roll_score: a workgroup per (tile of sixteen series, origin): Y = X K[s, s'] on the matrix pipe with the table read where it lies,
// the row dots against conj(X) with the waves' parts summed in a fixed order, the other triangle as the conjugate.  A labelled row keeps
// the rho of its class (whose scale cancels); a mixture row adds the classes in ascending order, class c at the weight
// exp(a_c - max a), a_c = the row's log at t + lnG[t][c] - the pieces of mpst_prefix_marginals.  A class whose row or table vanished
// weighs nothing.  rho[chunk][T][H][d * d] goes to scratch.
// k_roll_grid: the body of k_mc_grid on a (series, origin, horizon) triple at a time, the grid table, the value and the encoded state
// those of the target u; NaN in every output where u >= T.
// No floating-point atomics, one reduction order: a triple's bits depend neither on its neighbours nor on how the series and the targets
// are cut into blocks.
__device__ __forceinline__ int roll_pair_index(int s, int sp, int d) { return s * d - s * (s - 1) / 2 + (sp - s); }

template <bool CX> __global__ __launch_bounds__(SC_T) void k_roll_rows(ImpModel v, RollingArgs g) {
    __shared__ double Xr[SC_B * SC_LD], Xi[CX ? SC_B * SC_LD : 1];
    __shared__ double phr[SC_B * SC_PS], phi_[CX ? SC_B * SC_PS : 1];
    __shared__ double lgs[SC_B];                        // ln(norm^2) summed over the sites
    __shared__ int labs[SC_B];
    const int T = v.T, d = v.d, cm = v.cap, C = g.C, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t start = (int64_t)blockIdx.x * SC_B;               // chunk-local
    const int count = (int)min((int64_t)SC_B, g.count - start);
    const int64_t inst0 = g.first + start;
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
            for (int k0 = 0; k0 < Din; k0 += 4 * SC_KU) {
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
    // the rows in LDS to norm one, ln(norm^2) to the accumulators; a row whose norm is not a positive finite number is zeroed and its
    // accumulator is -inf: it weighs nothing in a mixture and gives NaN on its own
    auto rescale = [&](int D) {
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
        if (osub == 0) lgs[orow] = ok ? lgs[orow] + log(n2) : -INFINITY;
    };
    // the rows of origin t and class c, and their logs, to the block's scratch
    auto keep = [&](int t, int c) {
        if (orow >= count) return;
        const int D = v.chi[t];
        const int64_t at = ((start + orow) * (int64_t)T + t) * C + c;
        for (int cc = osub; cc < D; cc += 16) {
            double xi = 0.0;
            if constexpr (CX) xi = Xi[orow * SC_LD + cc];
            zstore<double, CX>(g.rows, at * cm + cc, Xr[orow * SC_LD + cc], xi);
        }
        if (osub == 0) g.lrow[at] = lgs[orow];
    };

    if (tid < SC_B) labs[tid] = tid < count ? v.label[inst0 + tid] : -2;
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        bool want = false;
        for (int r = 0; r < SC_B; ++r) want = want || labs[r] == c || labs[r] == -1;
        if (!want) continue;                // (uniform over the workgroup)
        __syncthreads();                    // the walk before is done with the rows
        for (int e = tid; e < SC_B * SC_LD; e += SC_T) {
            Xr[e] = (e % SC_LD) == 0 ? 1.0 : 0.0;
            if constexpr (CX) Xi[e] = 0.0;
        }
        if (tid < SC_B) lgs[tid] = 0.0;
        __syncthreads();
        for (int j = 0; j < T; ++j) {
            keep(j, c);
            load_phi(j);
            __syncthreads();
            const int Dout = step(j, c);
            __syncthreads();
            rescale(Dout);
            __syncthreads();
        }
    }
}

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_roll_tables(ImpModel v, RollingArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    const int d = v.d, cm = v.cap, C = g.C, H = g.H, tid = threadIdx.x;
    const int ls = *v.label_site;
    const int pairs = d * (d + 1) / 2;
    const int64_t gsz = (int64_t)cm * cm * ZW;
    const int64_t items = (int64_t)(g.u1 - g.u0) * C * pairs;
    double* T1 = g.work + (int64_t)blockIdx.x * gsz;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int ul = (int)(it / (C * pairs)), rem = (int)(it - (int64_t)ul * C * pairs);
        const int c = rem / pairs, pair = rem - c * pairs, u = g.u0 + ul;
        int s = 0;
        while (roll_pair_index(s + 1, s + 1, d) <= pair && s + 1 < d) ++s;
        const int sp = s + (pair - roll_pair_index(s, s, d));
        auto slot = [&](int hp) { return g.K + ((((int64_t)ul * H + hp) * C + c) * pairs + pair) * gsz; };
        // 1 / exp(lnG[t] - lnG[t+1]); zero where the factor is not a positive finite number: the chain of the class vanished
        auto scale_of = [&](int t) {
            const double f = exp(g.lnG[(int64_t)t * C + c] - g.lnG[(int64_t)(t + 1) * C + c]);
            return (f > 0.0 && f < INFINITY) ? 1.0 / f : 0.0;
        };
        __syncthreads();                    // the chain before is done with T1
        {
            const SiteView<double> sv = site_view<double, CX>(v, u, c, false);
            const int Di = sv.Din, Do = sv.Dout;
            const GMat<double> As{sv.W + (int64_t)s * sv.ss * ZW, sv.so, sv.si, Do, Di}, Asp{sv.W + (int64_t)sp * sv.ss * ZW, sv.so, sv.si, Do, Di};
            double* Kn = slot(0);
            gmem_mm<double, CX>(T1, Do, GMat<double>{g.G + pfx_slot(u + 1, c, C, ls) * gsz, Di, 1, Di, Di}, Asp, Di, Do, Di, true, false);   // G A_s'^H
            __threadfence_block();
            __syncthreads();
            gmem_mm<double, CX>(Kn, Do, As, GMat<double>{T1, Do, 1, Di, Do}, Do, Do, Di, false, false);                                      // A_s (G A_s'^H)
            __threadfence_block();
            __syncthreads();
            const double sc = scale_of(u);
            for (int e = tid; e < Do * Do * ZW; e += IMP_T) Kn[e] = sc != 0.0 ? Kn[e] * sc : 0.0;
            __threadfence_block();
            __syncthreads();
        }
        for (int hp = 1; hp < H && u - hp >= 0; ++hp) {
            const int t = u - hp;
            const SiteView<double> sv = site_view<double, CX>(v, t, c, false);
            const int Di = sv.Din, Do = sv.Dout;
            const GMat<double> Kp{slot(hp - 1), Di, 1, Di, Di};
            double* Kn = slot(hp);
            for (int q = 0; q < d; ++q) {
                const GMat<double> A{sv.W + (int64_t)q * sv.ss * ZW, sv.so, sv.si, Do, Di};     // W_t[q], read in place
                gmem_mm<double, CX>(T1, Do, Kp, A, Di, Do, Di, true, false);                    // K A^H
                __threadfence_block();
                __syncthreads();
                gmem_mm<double, CX>(Kn, Do, A, GMat<double>{T1, Do, 1, Di, Do}, Do, Do, Di, false, q > 0);       // += A (K A^H)
                __threadfence_block();
                __syncthreads();
            }
            const double sc = scale_of(t);
            for (int e = tid; e < Do * Do * ZW; e += IMP_T) Kn[e] = sc != 0.0 ? Kn[e] * sc : 0.0;
            __threadfence_block();
            __syncthreads();
        }
    }
}

template <bool CX> __global__ __launch_bounds__(SC_T) void k_roll_score(ImpModel v, RollingArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double Xr[SC_B * SC_LD], Xi[CX ? SC_B * SC_LD : 1];
    __shared__ double wd[2][4 * SC_B];                  // the waves' parts of the row dots, re / im
    __shared__ double wgt[SC_B];
    __shared__ int labs[SC_B];
    const int T = v.T, d = v.d, cm = v.cap, C = g.C, H = g.H, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t tile = blockIdx.x / T;
    const int t = (int)(blockIdx.x - tile * T);
    const int64_t start = tile * SC_B;                              // chunk-local
    const int count = (int)min((int64_t)SC_B, g.count - start);
    const int64_t inst0 = g.first + start;
    const int hlo = max(0, g.u0 - t), hhi = min(H, min(T, g.u1) - t);       // the horizons whose target lies in this block of tables
    if (hlo >= hhi) return;
    const int D = v.chi[t], pairs = d * (d + 1) / 2;
    const int64_t gsz = (int64_t)cm * cm * ZW;
    const int orow = tid >> 4, osub = tid & 15;

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
            for (int k0 = 0; k0 < Din; k0 += 4 * SC_KU) {
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

    if (tid < SC_B) labs[tid] = tid < count ? v.label[inst0 + tid] : -2;
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        bool want = false;
        for (int r = 0; r < SC_B; ++r) want = want || labs[r] == c || labs[r] == -1;
        if (!want) continue;                // (uniform over the workgroup)
        __syncthreads();                    // the class before is done with the rows and the weights
        for (int cc = osub; cc < SC_LD; cc += 16) {
            double xr = 0.0, xi = 0.0;
            if (orow < count && cc < D) zload<double, CX>(g.rows, (((start + orow) * (int64_t)T + t) * C + c) * cm + cc, xr, xi);
            Xr[orow * SC_LD + cc] = xr;
            if constexpr (CX) Xi[orow * SC_LD + cc] = xi;
        }
        if (tid < SC_B) {
            double w = 0.0;
            if (labs[tid] == c) w = 1.0;
            else if (labs[tid] == -1) {
                const int64_t at = ((start + tid) * (int64_t)T + t) * C;
                double amax = -INFINITY;
                for (int cc = 0; cc < C; ++cc) amax = fmax(amax, g.lrow[at + cc] + g.lnG[(int64_t)t * C + cc]);
                const double a = g.lrow[at + c] + g.lnG[(int64_t)t * C + c];
                w = (a > -INFINITY && a < INFINITY) ? exp(a - amax) : 0.0;
            }
            wgt[tid] = w;
        }
        __syncthreads();
        for (int hp = hlo; hp < hhi; ++hp) {
            const int ul = t + hp - g.u0;
            for (int s = 0; s < d; ++s)
                for (int sp = s; sp < d; ++sp) {
                    const double* Km = g.K + ((((int64_t)ul * H + hp) * C + c) * pairs + roll_pair_index(s, sp, d)) * gsz;
                    d4 yr[SC_NTW], yi[SC_NTW];
                    xmul(Km, 0, D, 1, D, D, yr, yi);
                    double pr[4] = {0.0, 0.0, 0.0, 0.0}, pi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int u = 0; u < SC_NTW; ++u) {
                        const int col = (wave + 4 * u) * 16 + i16;
                        if (col >= D) continue;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double xr = Xr[(kq + 4 * r) * SC_LD + col];
                            pr[r] = fma(yr[u][r], xr, pr[r]);
                            if constexpr (CX) {
                                const double xi = Xi[(kq + 4 * r) * SC_LD + col];
                                pr[r] = fma(yi[u][r], xi, pr[r]);
                                pi[r] = fma(yi[u][r], xr, pi[r]);
                                pi[r] = fma(-yr[u][r], xi, pi[r]);
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double a = sum16(pr[r]);
                        double b = 0.0;
                        if constexpr (CX) b = sum16(pi[r]);
                        if (i16 == 0) {
                            wd[0][wave * SC_B + kq + 4 * r] = a;
                            wd[1][wave * SC_B + kq + 4 * r] = b;
                        }
                    }
                    __syncthreads();
                    if (tid < count && (labs[tid] == c || labs[tid] == -1)) {
                        double re = (wd[0][0 * SC_B + tid] + wd[0][1 * SC_B + tid]) + (wd[0][2 * SC_B + tid] + wd[0][3 * SC_B + tid]);
                        double im = (wd[1][0 * SC_B + tid] + wd[1][1 * SC_B + tid]) + (wd[1][2 * SC_B + tid] + wd[1][3 * SC_B + tid]);
                        double* rho = g.rho + (((start + tid) * (int64_t)T + t) * H + hp) * (int64_t)(d * d * ZW);
                        if (labs[tid] == -1) {
                            const double w = wgt[tid];          // a class that weighs nothing adds an exact zero
                            re = w != 0.0 ? re * w : 0.0;
                            im = w != 0.0 ? im * w : 0.0;
                            if (c > 0) {                        // the classes in ascending order, by the thread that wrote the ones before
                                double r0, i0;
                                zload<double, CX>(rho, s * d + sp, r0, i0);
                                re += r0;
                                im += i0;
                            }
                        }
                        zstore<double, CX>(rho, s * d + sp, re, im);
                        if (sp != s) zstore<double, CX>(rho, sp * d + s, re, -im);
                    }
                    __syncthreads();
                }
        }
    }
}

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_roll_grid(ImpModel v, RollingArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double red[4], wtot[4];
    __shared__ int isel[4];
    __shared__ double srr[IMP_MAXD * IMP_MAXD], sri[IMP_MAXD * IMP_MAXD];
    __shared__ double lev[IMP_MAXQ];
    const int T = v.T, d = v.d, H = g.H, tid = threadIdx.x, n = g.ngrid;
    double* p = g.pbuf + (int64_t)blockIdx.x * n;
    double* S = g.sbuf + (int64_t)blockIdx.x * n;
    const int nrow = (n + 63) >> 6, rpw = (nrow + 3) >> 2, quarter = rpw * 64;
    const double dx = g.grid_x[1] - g.grid_x[0];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid < g.nq) lev[tid] = g.levels[tid];
    for (int64_t tr = blockIdx.x; tr < g.count * T * H; tr += gridDim.x) {
        const int64_t il = tr / ((int64_t)T * H), i = g.first + il;
        const int rem = (int)(tr - il * T * H), t = rem / H, u = t + (rem - t * H);      // the origin and the target
        const int64_t o = tr;               // the outputs are the block's own: [chunk][T][H]
        __syncthreads();                    // the previous triple is done with p, S and the shared values
        if (u >= T) {                       // beyond the chain (uniform over the workgroup)
            if (tid == 0) {
                if (g.nll) g.nll[o] = qnan;
                if (g.pit) g.pit[o] = qnan;
                if (g.med) g.med[o] = qnan;
                if (g.err) g.err[o] = qnan;
                if (g.mean) g.mean[o] = qnan;
                for (int l = 0; l < g.nq; ++l) g.q[o * g.nq + l] = qnan;
            }
            continue;
        }
        for (int e = tid; e < d * d; e += IMP_T) {
            double rr, ri;
            zload<double, CX>(g.rho + tr * (d * d * ZW), e, rr, ri);
            srr[e] = rr;
            sri[e] = ri;
        }
        __syncthreads();
        // rho at its largest magnitude one: p, Z and the numerator scale alike
        double amax = 0.0;
        for (int e = 0; e < d * d; ++e) amax = fmax(amax, fmax(fabs(srr[e]), fabs(sri[e])));
        const double asc = (amax > 0.0 && amax < INFINITY) ? 1.0 / amax : 1.0;
        double pmax = -1.0, m1 = 0.0;
        int kmax = 0;
        {
            const double* gp = g.grid_phi + (int64_t)u * g.grid_site_stride;
            for (int k = tid; k < n; k += IMP_T) {
                double fr[IMP_MAXD], fi[IMP_MAXD];
#pragma unroll
                for (int s = 0; s < IMP_MAXD; ++s) {
                    fr[s] = fi[s] = 0.0;
                    if (s < d) zload<double, CX>(gp, (int64_t)k * d + s, fr[s], fi[s]);
                }
                // Re(sum_s conj(g_s) u_s), u_s = sum_s' rho[s, s'] g_s'
                double q = 0.0;
#pragma unroll
                for (int s = 0; s < IMP_MAXD; ++s) {
                    if (s < d) {
                        double ur = 0.0, ui = 0.0;
#pragma unroll
                        for (int sp = 0; sp < IMP_MAXD; ++sp) {
                            if (sp < d) {
                                const double rr = srr[s * d + sp];
                                ur = fma(rr, fr[sp], ur);
                                if constexpr (CX) {
                                    const double ri = sri[s * d + sp];
                                    ur = fma(-ri, fi[sp], ur);
                                    ui = fma(rr, fi[sp], ui);
                                    ui = fma(ri, fr[sp], ui);
                                }
                            }
                        }
                        q = fma(fr[s], ur, q);
                        if constexpr (CX) q = fma(fi[s], ui, q);
                    }
                }
                const double pk = fmax(q * asc, 0.0);
                p[k] = pk;
                m1 = fma(g.grid_x[k], pk, m1);
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
        if (!(Z > 0.0 && Z < INFINITY)) {           // (uniform over the workgroup)
            if (tid == 0) {
                if (g.nll) g.nll[o] = qnan;
                if (g.pit) g.pit[o] = qnan;
                if (g.med) g.med[o] = qnan;
                if (g.err) g.err[o] = qnan;
                if (g.mean) g.mean[o] = qnan;
                for (int l = 0; l < g.nq; ++l) g.q[o * g.nq + l] = qnan;
            }
            continue;
        }
        if (g.mean) {                               // trapezoid(grid_x p) / Z
            const double tot = blk_sum(m1, red);
            if (tid == 0) g.mean[o] = dx * (tot - 0.5 * (g.grid_x[0] * p0 + g.grid_x[n - 1] * p[n - 1])) / Z;
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
                // which of the two grid values at the tipping distance: the rule of k_sc_grid (weighted_median's stable sort)
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
            const double x = g.x ? g.x[i * T + u] : qnan;
            const bool scored = g.x ? (x - x == 0.0) : true;        // the series are complete: without x the nll only
            if (g.nll) {
                double out = qnan;
                if (scored) {
                    // phi_u^H rho phi_u at the exact encoded state
                    const double* ph = (const double*)v.phi + ((int64_t)u * v.N + i) * d * ZW;
                    double num = 0.0;
                    for (int s = 0; s < d; ++s) {
                        double ar, ai, ur = 0.0, ui = 0.0;
                        zload<double, CX>(ph, s, ar, ai);
                        for (int sp = 0; sp < d; ++sp) {
                            double br, bi;
                            zload<double, CX>(ph, sp, br, bi);
                            const double rr = srr[s * d + sp], ri = sri[s * d + sp];
                            ur = fma(rr, br, ur);
                            if constexpr (CX) {
                                ur = fma(-ri, bi, ur);
                                ui = fma(rr, bi, ui);
                                ui = fma(ri, br, ui);
                            }
                        }
                        num = fma(ar, ur, num);
                        if constexpr (CX) num = fma(ai, ui, num);
                    }
                    num *= asc;
                    out = num > 0.0 ? -log(num / Z) : INFINITY;
                }
                g.nll[o] = out;
            }
            if (g.pit) {
                // F at the value, linear between its two neighbours on the grid
                const double x0 = g.grid_x[0], x1 = g.grid_x[n - 1];
                double F = qnan;
                if (scored) {
                    if (!(x > x0)) F = 0.0;
                    else if (!(x < x1)) F = 1.0;
                    else {
                        int k = (int)((x - x0) / dx);
                        k = max(0, min(n - 2, k));
                        while (k > 0 && g.grid_x[k] > x) --k;
                        while (k < n - 2 && g.grid_x[k + 1] <= x) ++k;
                        const double xa = g.grid_x[k], xb = g.grid_x[k + 1], Fa = cdf_at(k) / Z, Fb = cdf_at(k + 1) / Z;
                        F = Fa + (Fb - Fa) * ((x - xa) / (xb - xa));
                    }
                }
                g.pit[o] = F;
            }
        }
    }
}
