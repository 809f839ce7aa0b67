// Batched one-launch scoring (mpst_classify_batch): the overlaps of K models with their own data sets in ONE kernel launch, the
// losses and confusion matrices in a second one (summary.jl:4-136; the scoring step of hyperparameters/tuning.jl and
// hyperopt_utils.jl:152-231, where every candidate x fold is scored on a validation set of tens to a few hundred series).
//
// mpst_eval / mpst_classify walk the chain with one k_env launch per site (T + 2 launches per model, each launch-bound on such a set).
// The environments of different series never meet, so here a workgroup takes 16 series of one fit (blockIdx.z) and walks ALL sites
// with them: the left environment rows up to the label site, the right ones down to it, then the label site itself, contracted
// last like k_eval_final does.  Nothing per site goes to memory - the rows live in LDS - and the training caches LE / RE of the
// context are not touched.
//
//  * a step is out_i = Z_i M (k_env's product): Z_i the Khatri-Rao row prev_i (x) phi_i of a series (LDS, 16 x d chi), M the site
//    tensor.  Four waves, one 16-column tile of the output each (chi <= 64 where d chi <= 128), v_mfma_f64_16x16x4_f64 over the
//    contraction in two independent chains (even / odd k-steps, added at the end);
//  * the site tensors stream through LDS: while a step multiplies, every thread holds its 32-entry share of the NEXT site tensor in
//    flight from memory (coalesced: the tensor is read front to back) and parks it in LDS behind the step - in the order the step
//    wants it (the right-hand walk reads the tensor transposed), row stride odd, so that the B operand reads are conflict-free;
//  * LDS: site tensor 128 x 65, Khatri-Rao tile 16 x 130, two sets of environment rows 16 x 66, site vectors 2 x 16 x 17, bond
//    dimensions: 66.6 + 16.6 + 16.9 + 4.4 + 4.1 KB = 109 KB, one workgroup per CU (a scoring call has a few hundred workgroups);
//  * registers: 64 for the share in flight, 8 accumulators, addresses: no scratch.
#include "mpst_internal.h"

namespace mpst {

constexpr int SW_T = 256;            // 4 waves: one 16-column tile of a step's output each
constexpr int SW_BS = 65;            // row stride of the site tensor in LDS (odd)
constexpr int SW_ZS = 130;           // row stride of the Khatri-Rao tile
constexpr int SW_PS = 66;            // row stride of the environment rows
constexpr int SW_NST = 32;           // entries of a site tensor a thread carries: 128 x 64 / 256
constexpr int SW_TMAX = 1023;        // longest chain (the bond dimensions are staged in LDS)

struct ScoreSmem {
    double Bs[MAX_DIM * SW_BS];
    double Zt[16 * SW_ZS];
    double env[2][16 * SW_PS];       // [0] the walk at hand, [1] the finished left-hand rows
    double phs[2][16 * 17];
    double yc[16 * (MAX_C + 1)];
    double wd[4 * 16];               // the row dots of the four column tiles
    int chis[SW_TMAX + 2];
};

__global__ __launch_bounds__(SW_T) void k_score_walk_b(const ScoreJob* __restrict__ jobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    ScoreSmem& S = *reinterpret_cast<ScoreSmem*>(smem_raw);
    const ScoreJob& jb = jobs[blockIdx.z];
    const int64_t N = jb.N;
    const int start = (int)blockIdx.x * 16;
    if (start >= N) return;                  // the grid is sized for the largest set of the batch
    const int count = (int)min((int64_t)16, N - start);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, kq = lane >> 4;
    const int d = jb.d, T = jb.T, C = jb.C;
    for (int i = tid; i <= T; i += SW_T) S.chis[i] = jb.chi[i];
    const int p = *jb.label_site;
    __syncthreads();
    const int col = wave * 16 + i16;

    // share of a tensor of n entries that starts at M, front to back
    double stg[SW_NST];
    auto fetch = [&](const double* __restrict__ M, int n) {
#pragma unroll
        for (int u = 0; u < SW_NST; ++u) {
            const int idx = tid + SW_T * u;
            stg[u] = idx < n ? M[idx] : 0.0;
        }
    };
    // ... parked as B[z][k]: plain, M[z * ncol + k] (left-hand walk, label site), or transposed, M[k * nz + z] (right-hand walk)
    auto park = [&](int n, int ncol, int nz, bool transposed) {
#pragma unroll
        for (int u = 0; u < SW_NST; ++u) {
            const int idx = tid + SW_T * u;
            if (idx < n) {
                if (transposed) {
                    const int k = idx / nz, z = idx - k * nz;
                    S.Bs[z * SW_BS + k] = stg[u];
                } else {
                    const int z = idx / ncol, k = idx - z * ncol;
                    S.Bs[z * SW_BS + k] = stg[u];
                }
            }
        }
    };
    const int prow = tid / d, ps = tid - prow * d;          // threads < 16 d: one entry of the tile's site vectors
    auto fetch_phi = [&](int site) -> double {
        return (prow < 16 && prow < count) ? jb.phi[((int64_t)site * N + start + prow) * d + ps] : 0.0;
    };
    // one step: out_i[k] = sum_z Z_i[z] B[z][k] for the 16 series, k < Dout; Z_i[z] = prev_i[a] phi_i[s], z = a d + s (left) or s Dp + a
    auto khatri_rao = [&](const double* prev /* null: boundary */, int Dp, const double* ph, bool left) {
        const int Z = Dp * d, ZP = (Z + 3) & ~3;
        const int row = tid >> 4;
        for (int a = tid & 15; a < Dp; a += 16) {
            const double pa = row < count ? (prev ? prev[row * SW_PS + a] : 1.0) : 0.0;
            for (int s = 0; s < d; ++s) S.Zt[row * SW_ZS + (left ? a * d + s : s * Dp + a)] = pa * ph[row * 17 + s];
        }
        for (int z = Z + (tid & 15); z < ZP; z += 16) S.Zt[row * SW_ZS + z] = 0.0;
    };
    auto multiply = [&](int Z, int Dout) -> d4 {
        d4 a0 = {0.0, 0.0, 0.0, 0.0}, a1 = {0.0, 0.0, 0.0, 0.0};
        if (wave * 16 < Dout) {
            const int nsteps = (Z + 3) >> 2;
            const bool cv = col < Dout;
            const double* zr = S.Zt + i16 * SW_ZS + kq;
            const double* br = S.Bs + kq * SW_BS + col;
            for (int u = 0; u < nsteps; u += 2) {
                const int z0 = 4 * u + kq, z1 = z0 + 4;
                const double b0 = (cv && z0 < Z) ? br[4 * u * SW_BS] : 0.0;
                const double b1 = (cv && z1 < Z) ? br[(4 * u + 4) * SW_BS] : 0.0;
                a0 = mfma_f64(zr[4 * u], b0, a0);
                if (u + 1 < nsteps) a1 = mfma_f64(zr[4 * u + 4], b1, a1);
            }
        }
        return a0 + a1;
    };

    // ---- the two walks: side 0 the left-hand rows (sites 0 .. p-1), side 1 the right-hand ones (sites T-1 .. p+1) ----
    for (int side = 0; side < 2; ++side) {
        const bool left = side == 0;
        const int nstep = left ? p : T - 1 - p;
        if (nstep <= 0) continue;
        auto site_of = [&](int st) { return left ? st : T - 1 - st; };
        auto tensor_of = [&](int st) { return jb.sites + (int64_t)site_of(st) * jb.site_stride; };
        auto size_of = [&](int st) { const int j = site_of(st); return S.chis[j] * d * S.chis[j + 1]; };
        fetch(tensor_of(0), size_of(0));
        double phq = fetch_phi(site_of(0));
        __syncthreads();                      // (the other walk is done with Bs and phs)
        {
            const int j = site_of(0);
            park(size_of(0), S.chis[j + 1], d * S.chis[j + 1], !left);
            if (prow < 16) S.phs[0][prow * 17 + ps] = phq;
        }
        double* rows = S.env[0];
        for (int st = 0; st < nstep; ++st) {
            const int j = site_of(st);
            const int Dp = st == 0 ? 1 : (left ? S.chis[j] : S.chis[j + 1]);
            const int Dout = left ? S.chis[j + 1] : S.chis[j];
            __syncthreads();                  // this step's tensor and site vectors are parked, the previous step's rows written
            khatri_rao(st == 0 ? nullptr : rows, Dp, S.phs[st & 1], left);
            const bool more = st + 1 < nstep;
            if (more) {                       // the next site flies during the product
                fetch(tensor_of(st + 1), size_of(st + 1));
                phq = fetch_phi(site_of(st + 1));
            }
            __syncthreads();
            const d4 acc = multiply(Dp * d, Dout);
            if (wave * 16 < Dout) {
#pragma unroll
                for (int r = 0; r < 4; ++r) rows[(kq + 4 * r) * SW_PS + col] = acc[r];     // (columns beyond Dout: exact zeros, never read)
            }
            __syncthreads();                  // every wave is done with Bs
            if (more) {
                const int jn = site_of(st + 1);
                park(size_of(st + 1), S.chis[jn + 1], d * S.chis[jn + 1], !left);
                if (prow < 16) S.phs[(st + 1) & 1][prow * 17 + ps] = phq;
            }
        }
        if (left) {                           // keep the left-hand rows aside
            __syncthreads();
            for (int i = tid; i < 16 * SW_PS; i += SW_T) S.env[1][i] = S.env[0][i];
        }
    }
    // ---- the label site, last: yhat_i[c] = sum_b (sum_{a,s} L_i[a] phi_i[s] W_c[a][s][b]) R_i[b] ----
    const int Dl = S.chis[p], Dr = S.chis[p + 1];
    const double* Lrows = p > 0 ? S.env[1] : nullptr;
    const double* Rrows = p < T - 1 ? S.env[0] : nullptr;
    const int nW = Dl * d * Dr;
    const double* Wp = jb.sites + (int64_t)p * jb.site_stride;
    {
        const double phq = fetch_phi(p);
        __syncthreads();
        if (prow < 16) S.phs[0][prow * 17 + ps] = phq;
        __syncthreads();
        khatri_rao(Lrows, Dl, S.phs[0], true);
    }
    fetch(Wp, nW);
    for (int c = 0; c < C; ++c) {
        __syncthreads();                      // Zt is built; the previous class is done with Bs
        park(nW, Dr, 0, false);
        if (c + 1 < C) fetch(Wp + (int64_t)(c + 1) * nW, nW);
        __syncthreads();
        const d4 acc = multiply(Dl * d, Dr);
        // the row dots with the right-hand rows: 16 lanes, then the four column tiles, in a fixed order
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = kq + 4 * r;
            const double x = sum16((wave * 16 < Dr && col < Dr) ? acc[r] * (Rrows ? Rrows[i * SW_PS + col] : 1.0) : 0.0);
            if (i16 == 0) S.wd[wave * 16 + i] = x;
        }
        __syncthreads();
        if (tid < 16) S.yc[tid * (MAX_C + 1) + c] = (S.wd[tid] + S.wd[16 + tid]) + (S.wd[32 + tid] + S.wd[48 + tid]);
    }
    __syncthreads();
    // classify (summary.jl:116-136): the first largest |yhat|, as k_eval_reduce picks it
    if (tid < count) {
        double best = -1.0;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            const double y = S.yc[tid * (MAX_C + 1) + c];
            jb.yhat[(int64_t)(start + tid) * C + c] = y;
            if (fabs(y) > best) {
                best = fabs(y);
                arg = c;
            }
        }
        jb.pred[start + tid] = arg;
    }
}

// MSE_loss_acc_iter (summary.jl:33-58) for every fit of the batch: k_eval_reduce's sums (one workgroup per fit, fixed order).
// out3 = {sum mse, sum kld, correct}; conf[truth][pred]
__global__ __launch_bounds__(1024) void k_score_reduce_b(const ScoreJob* __restrict__ jobs) {
    __shared__ double red[3][16];
    __shared__ int cm[MAX_C * MAX_C];
    const ScoreJob& jb = jobs[blockIdx.z];
    const int C = jb.C, tid = threadIdx.x;
    for (int i = tid; i < C * C; i += 1024) cm[i] = 0;
    __syncthreads();
    double mse = 0.0, kld = 0.0, acc = 0.0;
    for (int64_t i = tid; i < jb.N; i += 1024) {
        const double* y = jb.yhat + i * C;
        const int lab = jb.label[i];
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
            const double t = y[c] - (c == lab ? 1.0 : 0.0);
            s += t * t;
        }
        const int arg = jb.pred[i];
        mse += 0.5 * s;
        kld += -log(y[lab] * y[lab]);
        acc += (arg == lab) ? 1.0 : 0.0;
        atomicAdd(&cm[lab * C + arg], 1);
    }
    mse = wave_sum(mse);
    kld = wave_sum(kld);
    acc = wave_sum(acc);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = mse;
        red[1][tid >> 6] = kld;
        red[2][tid >> 6] = acc;
    }
    __syncthreads();
    if (tid < 3) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[tid][w];
        jb.out3[tid] = t;
    }
    for (int i = tid; i < C * C; i += 1024) jb.conf[i] = cm[i];
}

bool score_walk_supported(int T, int d, int cap, int C) { return d >= 1 && d <= 16 && cap <= 64 && d * cap <= MAX_DIM && T >= 1 && T <= SW_TMAX && C <= MAX_C; }
hipError_t score_init_attrs() { return hipFuncSetAttribute((const void*)k_score_walk_b, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ScoreSmem)); }
void launch_score_b(const ScoreJob* jobs, int K, int64_t maxN, hipStream_t s) {
    hipLaunchKernelGGL(k_score_walk_b, dim3((unsigned)((maxN + 15) / 16), 1, K), dim3(SW_T), sizeof(ScoreSmem), s, jobs);
    hipLaunchKernelGGL(k_score_reduce_b, dim3(1, 1, K), dim3(1024), 0, s, jobs);
}

}  // namespace mpst
