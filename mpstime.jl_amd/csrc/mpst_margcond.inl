// Marginal site conditionals (included by mpst_impute.hip): for a series i of class c_i with the known sites K_i and EVERY site t, known
// or missing, the distribution of x_t given the known values of the other sites, p(x_t | x_j, j in K_i \ {t}), under the label slice
// c_i of the model as stored.  The convention is the Born rule - that of mpst_marginal_model, the window conditionals and pair
// analysis: with A_j[s] = W_j[:, s, :] at a missing site, M_j = sum_q conj(phi[i][j][q]) W_j[:, q, :] at a known one and the density
// recursion of mpst_marginal.inl, E' = sum_s A_j[s]^T E conj(A_j[s]) (one term, M_j, at a known site),
//     L_{t-1}  the density over the left bond of site t from the sites 0 .. t-1 (L_{-1} = 1),
//     R_{t+1}  the density over its right bond from the sites t+1 .. T-1 (R_T = 1),
//     rho_t[s, s'] = sum_{a a' b b'} L_{t-1}[a, a'] W_t[a, s, b] conj(W_t[a', s', b']) R_{t+1}[b, b'],
// and the density on the grid states g_k of site t is p_k = max(Re(g_k^H rho_t g_k), 0).  Site t itself is never conditioned on.  At a
// complete series rho_t = a_t a_t^H with the a_t of mpst_sitecond.inl.  L and R are rescaled to trace one at every site; no scale is
// kept, everything returned is normalised.
//
// k_mc_walk: a workgroup of 256 threads per series.  The right walk first: R_{t+1} of every site to global scratch ([T][cap][cap] per
// series, slot t with leading dimension chi_{t+1}).  Then the left walk on the fly: at site t, for every physical index s,
//     K_s = L A_s^H            (A_s = W_t[:, s, :]^T, chi_{t+1} x chi_t; K_s = (A_s L)^H)
//     Y_s = K_s R^T            (chi_t x chi_{t+1})
//     rho_t[s, s'] = conj(sum_{a b} Y_s[a, b] W_t[a, s', b])        (d Frobenius forms per s, the tensor read where it lies)
// and then the step L <- sum_s A_s L A_s^H / trace.  Up to the LDS limit of the environment pass the matrices L, the site matrix,
// K_s and R (Y_s takes the site matrix's place) live in LDS as zero-padded (re, im) planes and every product is C = A B^H on
// lds_tile_rows, a wave per 16 x 16 tile; R is loaded conjugated, so that K_s conj(R)^H = K_s R^T.  The step writes the new density
// into the plane R leaves free and the two swap.  No product takes a density for Hermitian: the step is A (E A^H), the first product
// stored as its conjugate transpose so that the second reads it along rows.  (k_marginal's T1 = A E^H, the same in exact arithmetic,
// turns the rounding of a nearly rank-one density from an error of its two factors into a generic one: at T = 1000 the cdf was
// 1.2e-12 off an extended-precision evaluation where this order is 1.5e-13 off.)  Beyond the limit (BIG, chi <= 128): gmem_mm in
// MARGCOND_BIG_MATS matrices of global scratch per workgroup, W_t[s] and R read in place.  The step forms its own product L A_s^H
// (stored transposed; K_s is needed as it is, and the site matrix has made way for Y_s by then), so a missing site costs 4 d
// products where 3 d would do.  The vector shortcut of k_marginal (a half chain that has met known sites only is an outer product)
// is NOT taken: both walks carry matrices from the first site on, which keeps one code path and one reduction order whatever the
// mask.  At the label site the tensor is the block of the series' class.  The Frobenius forms: every wave sums its lanes, the four
// waves are added in a fixed order by one lane per s'.  A series does not see what travels with it.  A trace that is not a positive
// finite number ends its walk: the sites that would have read it get NaN in rho and so in every output.
//
// k_mc_grid: a workgroup per (series, site) pair at a time: the quadratic form g_k^H rho_t g_k on the grid (d^2 per grid value, where
// k_sc_grid has d), then k_imp_left's table-path routines - grid_prefix_sums, grid_quantile, grid_wmad, grid_cdf_at - with the tie
// rules of k_sc_grid, the first moment for the mean (only its total is needed: a block sum in one order), nll at the exact encoded
// state and the cdf at the value wherever x[i][t] is finite - at a known site the leave-one-out score with the missing sites summed
// out, at a missing site the held-out score of the value the caller supplied; NaN elsewhere.
template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_mc_walk(ImpModel v, McArgs g) {
    using acc_t = typename Mx<double>::acc_t;
    using Mat = MrgMat<double, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    __shared__ double part[4][IMP_MAXD][2];     // the Frobenius forms of one s: [wave][s'][re / im]
    constexpr int ZW = CX ? 2 : 1;
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t il = blockIdx.x, i = g.first + il;
    const uint8_t* mi = g.missing ? g.missing + i * T : nullptr;
    const int ls = *v.label_site, cls = v.label[i];
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 2;                      // as in k_marginal: rows 16-byte aligned and 4 banks apart
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t bsz = (int64_t)cm * cm * ZW;
    double* slots = g.dens + il * T * bsz;
    double *pE, *pN, *pMs, *pT1, *pY;           // the density, the other density plane (LDS: R of the site, then E'), the site matrix, K_s / T1, Y_s
    if constexpr (BIG) {
        double* base = g.work + il * MARGCOND_BIG_MATS * bsz;
        pE = base;
        pN = base + bsz;
        pMs = base + 2 * bsz;
        pT1 = base + 3 * bsz;
        pY = base + 4 * bsz;
    } else {
        double* smem = reinterpret_cast<double*>(smem_raw);
        pE = smem;
        pMs = smem + ZW * msz;
        pT1 = smem + 2 * ZW * msz;
        pN = smem + 3 * ZW * msz;
        pY = pMs;
        for (int e = tid; e < 4 * ZW * msz; e += IMP_T) smem[e] = 0.0;
        __syncthreads();
    }
    auto mat = [&](double* p, int cols) { return Mat{p, BIG ? cols : ld, BIG ? 0 : msz}; };
    auto plane = [&](double* p) { return Plane<double>{p, p + (ZW - 1) * msz}; };

    // LDS: C (M x Nn, zeros beyond, the whole cp x cp plane written) (+)= A B^H over the padded planes; `herm`: C^H is stored instead
    auto lds_mm = [&](double* pC, double* pA, double* pB, int M, int Nn, bool accumulate, bool herm) {
        const Plane<double> Ap = plane(pA), Bp = plane(pB), Cp = plane(pC);
        const int tm = (M + 15) >> 4, tn = (Nn + 15) >> 4;
        for (int tile = wave; tile < ntile; tile += 4) {
            const int rb = tile / tpr, wc = tile - rb * tpr;
            acc_t ar = {0, 0, 0, 0}, ai = {0, 0, 0, 0};
            if (accumulate) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int at = (16 * rb + Mx<double>::row(kq, r)) * ld + 16 * wc + i16;
                    ar[r] = Cp.r[at];
                    if constexpr (CX) ai[r] = Cp.i[at];
                }
            }
            if (rb < tm && wc < tn) lds_tile_rows<double, CX>(ar, ai, Ap, 16 * rb, Bp, 16 * wc, ks, ld);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rb + Mx<double>::row(kq, r), col = 16 * wc + i16;
                const bool live = row < M && col < Nn;
                const int at = herm ? col * ld + row : row * ld + col;
                Cp.r[at] = live ? ar[r] : 0.0;
                if constexpr (CX) Cp.i[at] = live ? (herm ? -ai[r] : ai[r]) : 0.0;
            }
        }
    };
    // the density is the 1 x 1 matrix [1]
    auto unit = [&]() {
        if constexpr (BIG) {
            if (tid == 0) zstore<double, CX>(pE, 0, 1.0, 0.0);
        } else {
            for (int e = tid; e < ZW * msz; e += IMP_T) pE[e] = e == 0 ? 1.0 : 0.0;
        }
        __syncthreads();
    };
    // E <- sum_s A[s] E A[s]^H / trace through the site `sv` (one term, M_j, at a known site); returns the trace, and E is left alone
    // unless that is a positive finite number
    auto step = [&](const SiteView<double>& sv, const double* ph, bool miss) -> double {
        const int Di = sv.Din, Do = sv.Dout, ns = miss ? d : 1;
        double out = 0.0;
        for (int s_ = 0; s_ < ns; ++s_) {
            if constexpr (BIG) {
                GMat<double> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};      // a missing site's W_j[s], read in place
                if (!miss) {
                    mrg_site_matrix<double, CX, BIG>(mat(pMs, Di), cp, sv, ph, 0, d, false);
                    __syncthreads();
                    A = GMat<double>{pMs, Di, 1, Do, Di};
                }
                gmem_mm<double, CX>(pT1, Di, A, GMat<double>{pE, Di, 1, Di, Di}, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<double, CX>(pN, Do, GMat<double>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            } else {
                mrg_site_matrix<double, CX, BIG>(mat(pMs, Di), cp, sv, miss ? nullptr : ph, s_, d, true);
                __syncthreads();
                lds_mm(pT1, pE, pMs, Di, Do, false, true);          // (E A^H)^H, stored as the Do x Di matrix it is
                __syncthreads();
                lds_mm(pN, pMs, pT1, Do, Do, s_ > 0, false);        // E' += A (E A^H)
                __syncthreads();
            }
        }
        const Mat En = mat(pN, Do);
        for (int a_ = tid; a_ < Do; a_ += IMP_T) {
            double er, ei;
            En.get(a_, a_, er, ei);
            out += er;
        }
        out = blk_sum(out, red);
        if (!(out > 0.0 && out < INFINITY)) return out;
        const double sc = 1.0 / out;
        const int n = BIG ? Do * Do * ZW : ZW * msz;
        for (int e = tid; e < n; e += IMP_T) pN[e] *= sc;
        __syncthreads();
        double* tmp = pE;
        pE = pN;
        pN = tmp;
        return out;
    };
    auto site_of = [&](int j, bool in_is_left) { return site_view<double, CX>(v, j, j == ls ? cls : 0, in_is_left); };
    auto phi_of = [&](int j) { return (const double*)v.phi + ((int64_t)j * v.N + i) * d * ZW; };
    // the density (D x D) to a slot of the kept walk, leading dimension D
    auto keep = [&](int slot, int D) {
        double* dst = slots + (int64_t)slot * bsz;
        const Mat E = mat(pE, D);
        for (int e = tid; e < D * D; e += IMP_T) {
            const int a_ = e / D, b_ = e - a_ * D;
            double er, ei;
            E.get(a_, b_, er, ei);
            zstore<double, CX>(dst, e, er, ei);
        }
    };

    // ---- right walk, kept: R_{t+1} into slot t, t = T-1 .. 0 ----
    unit();
    keep(T - 1, 1);
    for (int t = T - 1; t >= 1; --t) {
        const SiteView<double> sv = site_of(t, false);
        const double tr = step(sv, phi_of(t), mi && mi[t] != 0);
        if (!(tr > 0.0 && tr < INFINITY)) {
            for (int64_t e = tid; e < (int64_t)t * bsz; e += IMP_T) slots[e] = qnan;
            break;
        }
        keep(t - 1, sv.Dout);
    }
    __threadfence_block();
    __syncthreads();

    // ---- left walk on the fly: rho_t, then the step through site t ----
    unit();
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const SiteView<double> sv = site_of(t, true);
        const int Da = sv.Din, Db = sv.Dout;
        double* rho = g.rho + (il * T + t) * (int64_t)(d * d * ZW);
        if (dead) {
            for (int e = tid; e < d * d * ZW; e += IMP_T) rho[e] = qnan;
            continue;
        }
        const double* Rt = slots + (int64_t)t * bsz;
        if constexpr (!BIG) {
            // conj(R_{t+1}), zero-padded, into the free density plane
            const Mat Rc = mat(pN, Db);
            for (int e = tid; e < cp * cp; e += IMP_T) {
                const int r = e / cp, c_ = e - r * cp;
                double rr = 0.0, ri = 0.0;
                if (r < Db && c_ < Db) zload<double, CX>(Rt, (int64_t)r * Db + c_, rr, ri);
                Rc.set(r, c_, rr, -ri);
            }
        }
        for (int s_ = 0; s_ < d; ++s_) {
            if constexpr (BIG) {
                const GMat<double> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Db, Da};
                gmem_mm<double, CX>(pT1, Db, GMat<double>{pE, Da, 1, Da, Da}, A, Da, Db, Da, true, false);             // K_s = L A_s^H
                __syncthreads();
                gmem_mm<double, CX>(pY, Db, GMat<double>{pT1, Db, 1, Da, Db}, GMat<double>{Rt, 1, Db, Db, Db}, Da, Db, Db, false, false);   // Y_s = K_s R^T
                __syncthreads();
            } else {
                mrg_site_matrix<double, CX, BIG>(mat(pMs, Da), cp, sv, nullptr, s_, d, true);
                __syncthreads();
                lds_mm(pT1, pE, pMs, Da, Db, false, false);         // K_s = L A_s^H
                __syncthreads();
                lds_mm(pY, pT1, pN, Da, Db, false, false);          // Y_s = K_s conj(R)^H = K_s R^T, over the site matrix
                __syncthreads();
            }
            const Mat Y = mat(pY, Db);
            for (int sp = 0; sp < d; ++sp) {
                double fr = 0.0, fi = 0.0;
                for (int e = tid; e < Da * Db; e += IMP_T) {
                    const int a_ = e / Db, b_ = e - a_ * Db;
                    double yr, yi, wr, wi;
                    Y.get(a_, b_, yr, yi);
                    zload<double, CX>(sv.W, (int64_t)a_ * sv.si + (int64_t)sp * sv.ss + (int64_t)b_ * sv.so, wr, wi);
                    fr = fma(yr, wr, fr);
                    if constexpr (CX) {
                        fr = fma(-yi, wi, fr);
                        fi = fma(yr, wi, fi);
                        fi = fma(yi, wr, fi);
                    }
                }
                fr = wave_sum(fr);
                if constexpr (CX) fi = wave_sum(fi);
                if (lane == 0) {
                    part[wave][sp][0] = fr;
                    part[wave][sp][1] = fi;
                }
            }
            __syncthreads();
            if (tid < d) {
                const double fr = (part[0][tid][0] + part[1][tid][0]) + (part[2][tid][0] + part[3][tid][0]);
                const double fi = (part[0][tid][1] + part[1][tid][1]) + (part[2][tid][1] + part[3][tid][1]);
                zstore<double, CX>(rho, s_ * d + tid, fr, -fi);
            }
            __syncthreads();
        }
        if (t + 1 < T) {
            const double tr = step(sv, phi_of(t), mi && mi[t] != 0);
            if (!(tr > 0.0 && tr < INFINITY)) dead = true;
        }
    }
}

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_mc_grid(ImpModel v, McArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double red[4], wtot[4];
    __shared__ int isel[4];
    __shared__ double srr[IMP_MAXD * IMP_MAXD], sri[IMP_MAXD * IMP_MAXD];
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
        for (int e = tid; e < d * d; e += IMP_T) {
            double rr, ri;
            zload<double, CX>(g.rho + pair * (d * d * ZW), e, rr, ri);
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
            const double* gp = g.grid_phi + (int64_t)t * g.grid_site_stride;
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
        const int64_t o = pair;             // the outputs are the block's own: [chunk][T]
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
            const bool miss = g.missing && g.missing[i * T + t] != 0;
            const double x = g.x ? g.x[i * T + t] : qnan;
            const bool scored = g.x ? (x - x == 0.0) : !miss;       // a finite value (without x: a known site, nll only)
            if (g.nll) {
                double out = qnan;
                if (scored) {
                    // phi_t^H rho_t phi_t at the exact encoded state
                    const double* ph = (const double*)v.phi + ((int64_t)t * v.N + i) * d * ZW;
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
