// Observed conditionals (included by mpst_impute.hip): the marginal site conditionals of mpst_margcond.inl with a MEASUREMENT at every
// site in place of "known exactly" / "missing".  A site (i, t) has a kind and two parameters a, b in the encoding's domain:
//     OBS_EXACT    the value is x[i][t] with the state phi[i][t]             E = phi phi^H   (never formed by the walk)
//     OBS_MISSING  nothing observed                                          E = 1           (never formed by the walk)
//     OBS_GAUSS    y = a with noise sd b:  k_k = exp(-(x_k - a)^2 / (2 b^2)) / (b sqrt(2 pi))
//     OBS_INTERVAL a <= x <= b:            k_k = 1 inside, 0 outside
//                                                                            E[s, s'] = sum_k w_k k_k g_k[s] conj(g_k[s'])
//     OBS_OPERATOR the caller's Hermitian d x d matrix                       E = E_user[i][t]
// with w_k the trapezoid weights of the grid (dx / 2 at the two ends, dx inside) and g_k the grid states of site t.  The density walk
// steps through a site with operator E as
//     L' = sum_{s'} B_{s'}^T L conj(A_{s'}),   B_{s'} = sum_s conj(E[s, s']) A_s,   A_s = W_t[:, s, :]
// which is M^T L conj(M) at an exact site and sum_s A_s^T L conj(A_s) at a missing one, and the same from the right.  rho_t is that of
// mpst_margcond.inl - site t's own observation never enters it - and tr(E_t rho_t) is the likelihood of the observation given the others.
//
// k_obs_operator: a workgroup per (series, site) pair at a time writes E of every site but the OPERATOR ones (which the host has copied
// in) to the block's [chunk][T][d][d] array.  The quadrature of a GAUSS / INTERVAL site, for each s: every thread sums its grid values
// k = tid, tid + 256, ... for all s' at once, every wave sums its lanes, one lane per s' adds the four waves in a fixed order.  No atomics.
//
// k_obs_walk: k_mc_walk - the same planes, the same products in the same order, the same two routes - with the site-matrix loader of a
// soft site: obs_site_matrix stages B~_{s'} = sum_s conj(E[s, s']) A~_s (A~_s = A_s^T, as k_mc_walk keeps it), the d slice loads of an
// element issued together, eight at a time, before the first multiply.  On the LDS route a soft site stages A~_{s'}, forms
// (L A~_{s'}^H)^H, stages B~_{s'} over it and adds B~_{s'} (L A~_{s'}^H): two products per s', what a missing site costs.  Beyond the
// LDS limit B~_{s'} goes to the site-matrix slot of the global scratch, A~_{s'} is read in place: (B~_{s'} L) A~_{s'}^H.  The logs of
// the left walk's traces are summed in fp64; with ln tr(E_{T-1} rho_{T-1}) of the last site's density as it stands they are logev, the
// log of the un-normalised chain value.  A walk that ends early (a trace that is not a positive finite number) gives -inf.
//
// k_obs_grid: k_mc_grid's body, twice: on p_k (the predictive group) and on k_k p_k (the posterior group), the likelihood evaluated on
// the fly; each pass only if one of its outputs is asked for.  nll_obs = -ln(tr(E_t rho_t) / Z).
constexpr int OBS_EXACT = 0, OBS_MISSING = 1, OBS_GAUSS = 2, OBS_INTERVAL = 3, OBS_OPERATOR = 4;

// k_k of a GAUSS / INTERVAL site at the grid value x
__device__ __forceinline__ double obs_likelihood(int kind, double a, double b, double x) {
    if (kind == OBS_GAUSS) {
        const double r = x - a;
        return exp(-(r * r) / (2.0 * b * b)) / (b * 2.5066282746310002);      // sqrt(2 pi)
    }
    return (a <= x && x <= b) ? 1.0 : 0.0;
}

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_obs_operator(ImpModel v, ObsArgs g) {
    constexpr int ZW = CX ? 2 : 1;
    __shared__ double part[4][IMP_MAXD][2];
    const int T = v.T, d = v.d, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = g.ngrid;
    const double dx = g.grid_x[1] - g.grid_x[0];
    for (int64_t pair = blockIdx.x; pair < g.count * T; pair += gridDim.x) {
        const int64_t il = pair / T, i = g.first + il;
        const int t = (int)(pair - il * T);
        const int kind = g.kind ? g.kind[i * T + t] : OBS_EXACT;
        double* E = g.E + pair * (int64_t)(d * d * ZW);
        if (kind == OBS_OPERATOR) continue;
        if (kind == OBS_MISSING) {
            for (int e = tid; e < d * d; e += IMP_T) zstore<double, CX>(E, e, (e / d == e % d) ? 1.0 : 0.0, 0.0);
            continue;
        }
        if (kind == OBS_EXACT) {
            const double* ph = (const double*)v.phi + ((int64_t)t * v.N + i) * d * ZW;
            for (int e = tid; e < d * d; e += IMP_T) {
                double ar, ai, br, bi;
                zload<double, CX>(ph, e / d, ar, ai);
                zload<double, CX>(ph, e % d, br, bi);
                zstore<double, CX>(E, e, CX ? fma(ai, bi, ar * br) : ar * br, CX ? fma(ai, br, -(ar * bi)) : 0.0);
            }
            continue;
        }
        const double a = g.a[i * T + t], b = g.b[i * T + t];
        const double* gp = g.grid_phi + (int64_t)t * g.grid_site_stride;
        for (int s = 0; s < d; ++s) {
            double accr[IMP_MAXD], acci[IMP_MAXD];
#pragma unroll
            for (int sp = 0; sp < IMP_MAXD; ++sp) accr[sp] = acci[sp] = 0.0;
            for (int k = tid; k < n; k += IMP_T) {
                const double wk = ((k == 0 || k == n - 1) ? 0.5 * dx : dx) * obs_likelihood(kind, a, b, g.grid_x[k]);
                double sr, si;
                zload<double, CX>(gp, (int64_t)k * d + s, sr, si);
                const double cr = wk * sr, ci = wk * si;
#pragma unroll
                for (int sp = 0; sp < IMP_MAXD; ++sp) {
                    if (sp < d) {
                        double qr, qi;
                        zload<double, CX>(gp, (int64_t)k * d + sp, qr, qi);
                        // (cr + i ci) (qr - i qi)
                        accr[sp] = fma(cr, qr, accr[sp]);
                        if constexpr (CX) {
                            accr[sp] = fma(ci, qi, accr[sp]);
                            acci[sp] = fma(ci, qr, acci[sp]);
                            acci[sp] = fma(-cr, qi, acci[sp]);
                        }
                    }
                }
            }
#pragma unroll
            for (int sp = 0; sp < IMP_MAXD; ++sp) {
                if (sp < d) {
                    const double fr = wave_sum(accr[sp]);
                    double fi = 0.0;
                    if constexpr (CX) fi = wave_sum(acci[sp]);
                    if (lane == 0) {
                        part[wave][sp][0] = fr;
                        part[wave][sp][1] = fi;
                    }
                }
            }
            __syncthreads();
            if (tid < d) {
                const double fr = (part[0][tid][0] + part[1][tid][0]) + (part[2][tid][0] + part[3][tid][0]);
                const double fi = (part[0][tid][1] + part[1][tid][1]) + (part[2][tid][1] + part[3][tid][1]);
                zstore<double, CX>(E, s * d + tid, fr, fi);
            }
            __syncthreads();
        }
    }
}

// M[o][i] = sum_s conj(E[s, sp]) W_j[s](i, o): mrg_site_matrix with a column of conj(E) where it has conj(phi).  `ec`: the column in
// LDS, (re, im) of E[s, sp] at ec[2 s], ec[2 s + 1].  The slice loads of an element go out eight at a time ahead of their multiplies.
template <bool CX, bool BIG>
__device__ __forceinline__ void obs_site_matrix(const MrgMat<double, CX, BIG>& M, int cp, const SiteView<double>& sv, const double* ec, int d, bool pad) {
    const int Di = sv.Din, Do = sv.Dout, tid = threadIdx.x;
    const bool in_fast = sv.si == 1;
    const int Df = in_fast ? Di : Do;
    constexpr int NB = 8;
    for (int e = tid; e < Di * Do; e += IMP_T) {
        const int slow = e / Df, fast = e - slow * Df;
        const int ii = in_fast ? fast : slow, oo = in_fast ? slow : fast;
        const int64_t off = (int64_t)ii * sv.si + (int64_t)oo * sv.so;
        double ar = 0.0, ai = 0.0;
        for (int q0 = 0; q0 < d; q0 += NB) {
            double wr[NB], wi[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                wr[u] = wi[u] = 0.0;
                if (q0 + u < d) zload<double, CX>(sv.W, off + (int64_t)(q0 + u) * sv.ss, wr[u], wi[u]);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if (q0 + u < d) {
                    const double er = ec[2 * (q0 + u)], ei = ec[2 * (q0 + u) + 1];
                    // (er - i ei) (wr + i wi)
                    ar = fma(er, wr[u], ar);
                    if constexpr (CX) {
                        ar = fma(ei, wi[u], ar);
                        ai = fma(er, wi[u], ai);
                        ai = fma(-ei, wr[u], ai);
                    }
                }
            }
        }
        M.set(oo, ii, ar, ai);
    }
    if constexpr (!BIG) {
        if (pad) {
            for (int e = tid; e < cp * cp; e += IMP_T) {
                const int r = e / cp, c = e - r * cp;
                if (r >= Do || c >= Di) M.set(r, c, 0.0, 0.0);
            }
        }
    }
}

template <bool CX, bool BIG> __global__ __launch_bounds__(IMP_T) void k_obs_walk(ImpModel v, ObsArgs g) {
    using acc_t = typename Mx<double>::acc_t;
    using Mat = MrgMat<double, CX, BIG>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red[4];
    __shared__ double part[4][IMP_MAXD][2];     // the Frobenius forms of one s: [wave][s'][re / im]
    __shared__ double ecol[2 * IMP_MAXD];       // a column of E: (re, im) of E[s, s'] for every s
    constexpr int ZW = CX ? 2 : 1;
    const int T = v.T, d = v.d, cm = v.cap, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    const int64_t il = blockIdx.x, i = g.first + il;
    const uint8_t* ki = g.kind ? g.kind + i * T : nullptr;
    const int ls = *v.label_site, cls = v.label[i];
    const int cp = (cm + 15) & ~15;
    const int ld = cp + 2;                      // as in k_marginal: rows 16-byte aligned and 4 banks apart
    const int msz = cp * ld;
    const int tpr = cp >> 4, ntile = tpr * tpr, ks = cp >> 2;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t bsz = (int64_t)cm * cm * ZW;
    double* slots = g.dens + il * T * bsz;
    const double* Es = g.E + il * T * (int64_t)(d * d * ZW);
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
    // E <- (the step through the site `sv` of kind `kind`) / trace; returns the trace, and E is left alone unless that is a positive
    // finite number.  EXACT and MISSING: k_mc_walk's step.  Otherwise, with `Et` the site's operator: sum_s' B~_s' E A~_s'^H
    auto step = [&](const SiteView<double>& sv, const double* ph, int kind, const double* Et) -> double {
        const int Di = sv.Din, Do = sv.Dout;
        const bool miss = kind == OBS_MISSING, soft = kind >= OBS_GAUSS;
        const int ns = (miss || soft) ? d : 1;
        double out = 0.0;
        for (int s_ = 0; s_ < ns; ++s_) {
            if (soft) {
                __syncthreads();                // the previous column has been read
                if (tid < d) {
                    double er, ei;
                    zload<double, CX>(Et, tid * d + s_, er, ei);
                    ecol[2 * tid] = er;
                    ecol[2 * tid + 1] = ei;
                }
                __syncthreads();
            }
            if constexpr (BIG) {
                GMat<double> A{sv.W + (int64_t)s_ * sv.ss * ZW, sv.so, sv.si, Do, Di};      // W_j[s], read in place
                GMat<double> B = A;
                if (soft) {
                    obs_site_matrix<CX, BIG>(mat(pMs, Di), cp, sv, ecol, d, false);
                    __syncthreads();
                    B = GMat<double>{pMs, Di, 1, Do, Di};
                } else if (!miss) {
                    mrg_site_matrix<double, CX, BIG>(mat(pMs, Di), cp, sv, ph, 0, d, false);
                    __syncthreads();
                    A = B = GMat<double>{pMs, Di, 1, Do, Di};
                }
                gmem_mm<double, CX>(pT1, Di, B, GMat<double>{pE, Di, 1, Di, Di}, Do, Di, Di, false, false);
                __syncthreads();
                gmem_mm<double, CX>(pN, Do, GMat<double>{pT1, Di, 1, Do, Di}, A, Do, Do, Di, true, s_ > 0);
                __syncthreads();
            } else {
                mrg_site_matrix<double, CX, BIG>(mat(pMs, Di), cp, sv, (miss || soft) ? nullptr : ph, s_, d, true);
                __syncthreads();
                lds_mm(pT1, pE, pMs, Di, Do, false, true);          // (E A^H)^H, stored as the Do x Di matrix it is
                __syncthreads();
                if (soft) {
                    obs_site_matrix<CX, BIG>(mat(pMs, Di), cp, sv, ecol, d, true);
                    __syncthreads();
                }
                lds_mm(pN, pMs, pT1, Do, Do, s_ > 0, false);        // E' += A (E A^H), B~ (E A^H) at a soft site
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
    auto kind_of = [&](int j) { return ki ? (int)ki[j] : OBS_EXACT; };
    auto op_of = [&](int j) { return Es + (int64_t)j * (d * d * ZW); };
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
        const double tr = step(sv, phi_of(t), kind_of(t), op_of(t));
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
    double lg = 0.0;                            // ln of the traces the left walk divided by (uniform over the workgroup)
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
            const double tr = step(sv, phi_of(t), kind_of(t), op_of(t));
            if (!(tr > 0.0 && tr < INFINITY)) dead = true;
            else lg += log(tr);
        }
    }
    // logev = the logs of the left walk's traces + ln tr(E_{T-1} rho_{T-1}), rho_{T-1} as the walk left it; one lane reads it back
    if (g.logev) {
        __threadfence_block();
        __syncthreads();
        if (tid == 0) {
            double out = -INFINITY;
            if (!dead) {
                const double* rho = g.rho + (il * T + (T - 1)) * (int64_t)(d * d * ZW);
                const double* Et = op_of(T - 1);
                double tr = 0.0;                // Re sum_{s s'} E[s', s] rho[s, s']
                for (int s = 0; s < d; ++s) {
                    for (int sp = 0; sp < d; ++sp) {
                        double er, ei, rr, ri;
                        zload<double, CX>(Et, sp * d + s, er, ei);
                        zload<double, CX>(rho, s * d + sp, rr, ri);
                        tr = fma(er, rr, tr);
                        if constexpr (CX) tr = fma(-ei, ri, tr);
                    }
                }
                if (tr > 0.0 && tr < INFINITY) out = lg + log(tr);
            }
            g.logev[il] = out;
        }
    }
}

template <bool CX> __global__ __launch_bounds__(IMP_T) void k_obs_grid(ImpModel v, ObsArgs g) {
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
    const bool want_pred = g.pred_med || g.pred_err || g.pred_mean || (g.nq > 0 && g.pred_q);
    const bool want_post = g.post_med || g.post_err || g.post_mean || (g.nq > 0 && g.post_q);
    if (tid < g.nq) lev[tid] = g.levels[tid];
    for (int64_t pair = blockIdx.x; pair < g.count * T; pair += gridDim.x) {
        const int64_t il = pair / T, i = g.first + il;
        const int t = (int)(pair - il * T);
        const int kind = g.kind ? g.kind[i * T + t] : OBS_EXACT;
        const bool lik = kind == OBS_GAUSS || kind == OBS_INTERVAL;
        const double oa = lik ? g.a[i * T + t] : 0.0, ob = lik ? g.b[i * T + t] : 0.0;
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
        const int64_t o = pair;             // the outputs are the block's own: [chunk][T]
        double Zpred = qnan;
        // the group of outputs read from the density in p (with this thread's m1, pmax, kmax); returns trapz(p)
        auto group = [&](bool want, double* gmed, double* gerr, double* gmean, double* gq) -> double {
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
            if (!want) return Z;
            if (!(Z > 0.0 && Z < INFINITY)) {           // (uniform over the workgroup)
                if (tid == 0) {
                    if (gmed) gmed[o] = qnan;
                    if (gerr) gerr[o] = qnan;
                    if (gmean) gmean[o] = qnan;
                    if (gq) for (int l = 0; l < g.nq; ++l) gq[o * g.nq + l] = qnan;
                }
                return Z;
            }
            if (gmean) {                                // trapezoid(grid_x p) / Z
                const double tot = blk_sum(m1, red);
                if (tid == 0) gmean[o] = dx * (tot - 0.5 * (g.grid_x[0] * p0 + g.grid_x[n - 1] * p[n - 1])) / Z;
            }
            if (gmed || gerr) {
                const int kmed = grid_quantile(0.5, Z, n, nrow, isel, cdf_at);
                double err = 0.0;
                if (gerr && g.get_err) {
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
                    if (gmed) gmed[o] = g.grid_x[kmed];
                    if (gerr) gerr[o] = err;
                }
            }
            if (gq) {
                for (int l = 0; l < g.nq; ++l) {
                    const int kl = grid_quantile(lev[l], Z, n, nrow, isel, cdf_at);
                    if (tid == 0) gq[o * g.nq + l] = g.grid_x[kl];
                }
            }
            return Z;
        };
        // ---- the predictive group, and what is read at the observation ----
        Zpred = group(want_pred, g.pred_med, g.pred_err, g.pred_mean, g.nq > 0 ? g.pred_q : nullptr);
        const bool zok = Zpred > 0.0 && Zpred < INFINITY;
        if (tid == 0 && (g.nll || g.pit)) {
            const double x = g.x ? g.x[i * T + t] : qnan;
            // EXACT and MISSING: a finite value (without x: an exact site, nll only), as k_mc_grid has it
            const bool scored = kind <= OBS_MISSING && (g.x ? (x - x == 0.0) : kind == OBS_EXACT);
            if (g.nll) {
                double out = qnan;
                if (zok && (scored || kind >= OBS_GAUSS)) {
                    double num = 0.0;
                    if (kind <= OBS_MISSING) {
                        // phi_t^H rho_t phi_t at the exact encoded state
                        const double* ph = (const double*)v.phi + ((int64_t)t * v.N + i) * d * ZW;
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
                    } else {
                        // tr(E_t rho_t) = Re sum_{s s'} E[s', s] rho[s, s']
                        const double* Et = g.E + pair * (int64_t)(d * d * ZW);
                        for (int s = 0; s < d; ++s) {
                            for (int sp = 0; sp < d; ++sp) {
                                double er, ei;
                                zload<double, CX>(Et, sp * d + s, er, ei);
                                num = fma(er, srr[s * d + sp], num);
                                if constexpr (CX) num = fma(-ei, sri[s * d + sp], num);
                            }
                        }
                    }
                    num *= asc;
                    out = num > 0.0 ? -log(num / Zpred) : INFINITY;
                }
                g.nll[o] = out;
            }
            if (g.pit) {
                // F at the value, linear between its two neighbours on the grid (p and S still hold the predictive density)
                const double x0 = g.grid_x[0], x1 = g.grid_x[n - 1];
                double F = qnan;
                if (zok && scored) {
                    const GridSums tab{S, quarter, wtot[0], wtot[0] + wtot[1], (wtot[0] + wtot[1]) + wtot[2]};
                    const double p0 = p[0];
                    auto Sabs = [&](int k) { return tab.at(k); };
                    auto cdf_at = [&](int k) { return grid_cdf_at(k, dx, p0, Sabs); };
                    if (!(x > x0)) F = 0.0;
                    else if (!(x < x1)) F = 1.0;
                    else {
                        int k = (int)((x - x0) / dx);
                        k = max(0, min(n - 2, k));
                        while (k > 0 && g.grid_x[k] > x) --k;
                        while (k < n - 2 && g.grid_x[k + 1] <= x) ++k;
                        const double xa = g.grid_x[k], xb = g.grid_x[k + 1], Fa = cdf_at(k) / Zpred, Fb = cdf_at(k + 1) / Zpred;
                        F = Fa + (Fb - Fa) * ((x - xa) / (xb - xa));
                    }
                }
                g.pit[o] = F;
            }
        }
        // ---- the posterior group: k_k p_k; the predictive density itself at a missing site, NaN at an exact or operator site ----
        if (!want_post) continue;
        if (kind == OBS_EXACT || kind == OBS_OPERATOR) {
            if (tid == 0) {
                if (g.post_med) g.post_med[o] = qnan;
                if (g.post_err) g.post_err[o] = qnan;
                if (g.post_mean) g.post_mean[o] = qnan;
                if (g.nq > 0 && g.post_q) for (int l = 0; l < g.nq; ++l) g.post_q[o * g.nq + l] = qnan;
            }
            continue;
        }
        __syncthreads();                    // lane 0 is done with the predictive p and S
        if (lik) {
            pmax = -1.0, m1 = 0.0, kmax = 0;
            for (int k = tid; k < n; k += IMP_T) {
                const double pk = p[k] * obs_likelihood(kind, oa, ob, g.grid_x[k]);
                p[k] = pk;
                m1 = fma(g.grid_x[k], pk, m1);
                if (pk > pmax) {
                    pmax = pk;
                    kmax = k;
                }
            }
        }
        group(true, g.post_med, g.post_err, g.post_mean, g.nq > 0 ? g.post_q : nullptr);
    }
}
