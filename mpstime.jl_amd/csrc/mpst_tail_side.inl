// What k_bond_tail (mpst_fused.hip) and the side workgroups of k_eig_trivec (mpst_eig.hip) share: the part of a bond's tail that needs
// none of the eigensolver's output - the dense S tile and the overlap product P = O bt_new of every 16-series tile - is formed by extra
// workgroups of the eigensolver's launch, on CUs that launch leaves empty, and read back by the tail.  The library is built without
// relocatable device code: both translation units include this file.

#pragma once
#include "mpst_internal.h"

namespace mpst {

constexpr int BT_ELS = 37, BT_PLS = 21;      // LDS row strides of the staged factors (odd: the 16 rows a wave reads hit 16 bank pairs): 32 bond
                                             // entries / 16 site states and zeros behind them (the padded K extent reads up to 4 beyond the live ones)
constexpr int BT_FAC = 16 * (BT_ELS + BT_PLS);

// class-pure tile t of the data set from the tables in the kernel arguments (no dependent global load)
__device__ __forceinline__ Span tile_span_k(const View& v, int t) {
    int c = 0;
#pragma unroll 1
    for (int k = 1; k < v.C; ++k) c += (t >= v.kcls_tile[k]) ? 1 : 0;
    Span s;
    s.cls = c;
    s.start = v.kcls_off[c] + TILE_S * (t - v.kcls_tile[c]);
    s.count = t < v.ntiles ? min(TILE_S, v.kcls_off[c + 1] - s.start) : 0;
    s.pad = 0;
    return s;
}

// One side's Khatri-Rao vectors of a 16-series tile, kept as their FACTORS in LDS (environment row, site vector); entry z of row i
// is formed where it is wanted: left  z = a d + s: prev_i[a] phi_i[s];  right  z = s Dp + b: phi_i[s] prev_i[b]
// (the one product stage16 forms: the same bits).  Division by d / Dp with a multiply (z < 1024).
struct KrSide {
    const double* env;      // [16][BT_ELS]
    const double* ph;       // [16][BT_PLS]
    unsigned magic, div;
    bool left;
};
__device__ __forceinline__ KrSide kr_side(const double* fac, int Dp, int d, bool left) {
    KrSide k;
    k.env = fac;
    k.ph = fac + 16 * BT_ELS;
    k.div = (unsigned)(left ? d : Dp);
    k.magic = (65536u + k.div - 1u) / k.div;
    k.left = left;
    return k;
}
__device__ __forceinline__ double kr_at(const KrSide& k, int row, unsigned z) {
    const unsigned q = (z * k.magic) >> 16, r = z - q * k.div;
    // (entries the padded extent of a product asks for beyond the live ones: on the right the site index reaches 21 at d = 11 .. 16 with a
    // bond of 3 and 31 with a bond of 1 - tests/fuzz_chain4.py found the first; it is clamped onto the row's zero pad, as is the bond index on the left)
    const unsigned ie = min(k.left ? q : r, (unsigned)(BT_ELS - 1)), ip = min(k.left ? r : q, (unsigned)(BT_PLS - 1));
    return k.env[row * BT_ELS + ie] * k.ph[row * BT_PLS + ip];
}

// The factors of one side of a tile, as the 256 loader threads of that side see them: 16 threads per series row (lrow), two bond entries
// and one site state each (lj).  Whole rows are requested (the capacity is a kernel argument) ...
struct FacRegs {
    double fe0, fe1, fp;
};
__device__ __forceinline__ FacRegs tail_fac_request(const double* prev, const double* ph, const Span& tl, int lrow, int lj, int cap, int d) {
    const bool valid = lrow < tl.count;
    const int64_t smp = tl.count > 0 ? tl.start + (valid ? lrow : 0) : 0;
    // (unconditional loads from clamped addresses: see tail_chain_request; a tile beyond the data set has count 0 and start 0)
    const double x0 = prev ? prev[smp * cap + min(lj, cap - 1)] : 1.0;
    const double x1 = prev ? prev[smp * cap + min(lj + 16, cap - 1)] : 1.0;
    const double xp = ph[smp * d + min(lj, d - 1)];
    FacRegs f;
    f.fe0 = (valid && lj < cap) ? x0 : 0.0;
    f.fe1 = (valid && lj + 16 < cap) ? x1 : 0.0;
    f.fp = (valid && lj < d) ? xp : 0.0;
    return f;
}
// ... what lies beyond the live bond Dp is dropped once the dimensions are known (bnd: chain end, the one live entry is 1), and the rows go
// to LDS with the zero pads kr_at clamps onto
__device__ __forceinline__ void tail_fac_store(double* fac, FacRegs f, int lrow, int lj, int Dp, bool bnd) {
    f.fe0 = lj < Dp ? f.fe0 : 0.0;
    f.fe1 = (lj + 16 < Dp && !bnd) ? f.fe1 : 0.0;
    fac[lrow * BT_ELS + lj] = f.fe0;
    fac[lrow * BT_ELS + lj + 16] = f.fe1;
    if (lj < BT_ELS - 32) fac[lrow * BT_ELS + 32 + lj] = 0.0;
    fac[16 * BT_ELS + lrow * BT_PLS + lj] = f.fp;
    if (lj < BT_PLS - 16) fac[16 * BT_ELS + lrow * BT_PLS + 16 + lj] = 0.0;
}

// this wave's 16 columns of bt_new, every k-step: no predicates (sixteen exec-masked loads in a row keep the memory pipeline from
// ever holding a tile's worth of requests).  Rows beyond the live ones meet zeros of the O side, columns beyond them zeros of z:
// their (finite) values are read from clamped addresses and do not matter.  M: the tile's class of bt_new as [k = O index][n = S index].
struct BmSource {
    const double* __restrict__ M;
    unsigned col, NS;
    int kq, KO;
    __device__ __forceinline__ double at(int u) const { return M[(unsigned)min(4 * u + kq, KO - 1) * NS + col]; }
};
__device__ __forceinline__ BmSource tail_bm_source(const double* __restrict__ M, int wave, int i16, int kq, int KO, int NS) {
    return BmSource{M, (unsigned)min(16 * wave + i16, NS - 1), (unsigned)NS, kq, KO};
}
__device__ __forceinline__ void tail_bm_request(const BmSource& src, double (&bm)[32]) {
#pragma unroll
    for (int u = 0; u < 32; ++u) bm[u] = src.at(u);
}

// P = O bt_new, this wave's 16 columns.  A wave issues one MFMA per 64 cycles whatever their dependencies (profiles/ubench/
// mfma_rate.hip), so what a product costs is 64 cycles per MFMA PLUS every operand latency the wave waits out in between:
// operands are fetched a batch of 8 k-steps ahead (left to itself the compiler reads, waits, multiplies, reads ...).
// Whole batches: beyond the live extent the O side is zero.  Two accumulators fed alternately: the tail adds them, (pacc0 + pacc1).
// D4: d == 4 (the headline shapes): on the left side a = u, s = kq are immediates
// LATE: bt_new's entries are not in bm yet (tail_bm_request) but requested a batch ahead of their MFMAs like the other operand - the
// side workgroups, which have 128 registers per lane and all the time in the world; the same values into the same MFMAs
template <bool D4, bool LATE>
__device__ __forceinline__ void tail_overlap_product(const KrSide& ko, int KP, int i16, int kq, double (&bm)[32], const BmSource& src, d4& pacc0, d4& pacc1) {
    double ab[4][8];
    auto fetch = [&](int bt) {
        if (LATE) {
#pragma unroll
            for (int u = 0; u < 8; ++u) bm[8 * bt + u] = src.at(8 * bt + u);
        }
        if (D4 && ko.left) {
            const double* er = ko.env + i16 * BT_ELS + 8 * bt;
#pragma unroll
            for (int u = 0; u < 8; ++u) ab[bt][u] = er[u];
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) ab[bt][u] = kr_at(ko, i16, 4u * (8 * bt + u) + kq);
        }
    };
    const double phf = (D4 && ko.left) ? ko.ph[i16 * BT_PLS + kq] : 1.0;
    fetch(0);
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
        if (bt < 3) fetch(bt + 1);
        asm volatile("" ::: "memory");
        if (32 * bt < KP) {
#pragma unroll
            for (int u = 0; u < 8; u += 2) {
                pacc0 = mfma_f64(ab[bt][u] * phf, bm[8 * bt + u], pacc0);
                pacc1 = mfma_f64(ab[bt][u + 1] * phf, bm[8 * bt + u + 1], pacc1);
            }
        }
    }
}

// ---- one environment step of a 16-series tile: what k_env_walk (mpst_fused.hip) does T - 1 times in a row and a side workgroup of
// k_eig_trivec once per launch (the rebuild job of TailSide).  512 threads, 8 waves = (column tile nt, quarter q of the contraction).
// The product of k_env, bit for bit: the Khatri-Rao tile Zt[i][z] = prev_i[a] phi_i[s] (left z = a d + s, right z = s Dp + a), four MFMA
// chains over env_ks4(nsteps) k-steps each, added as (q0 + q1) + (q2 + q3).  Both callers run this one body: the same products, the
// same sums, the same row.
constexpr int EW_T = 512;
constexpr int EW_ZS = 130;                   // row stride of the dense Khatri-Rao tile
constexpr int EW_PS = 34;                    // row stride of the kept environment rows
constexpr int EW_PHS = 17;                   // row stride of a site's staged vectors
constexpr int EW_STEP_LDS = 16 * EW_ZS + 8 * 256;      // Zt, then the eight partial tiles

// this wave's share of site tensor M as the B operand of its quarter: M[z][col], z = 4 (q ks4 + u) + kq
// left: M[(a,s)][k], row stride Dout;  right: M[k][(s,b)] read transposed, column stride d * Dp (Dp, Dout: the bond dimensions from memory)
__device__ __forceinline__ void env_step_load_b(const double* M, bool left_side, int Dp, int Dout, int d, double (&bv)[8]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kq = lane >> 4, col = (wave & 1) * 16 + (lane & 15), q = wave >> 1;
    const int Z = Dp * d, nsteps = ((Z + 3) & ~3) >> 2, ks4 = env_ks4(nsteps);
    const int64_t sz = left_side ? Dout : 1, sk = left_side ? 1 : (int64_t)d * Dp;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int z = 4 * (q * ks4 + u) + kq;
        bv[u] = (col < Dout && u < ks4 && z < Z) ? M[(int64_t)z * sz + (int64_t)col * sk] : 0.0;
    }
}

// ph: the site's vectors [16][EW_PHS]; prevs: [16][EW_PS], the previous row on entry (first: chain end, 1 is taken instead), this step's on
// return; both written by the caller before the call (the first barrier is in here).  out: the row of the tile's first series (stride
// cap); WT: write-through stores (the side workgroups).  ahead(): what the caller requests while the step computes.
template <bool WT, class Ahead>
__device__ __forceinline__ void env_step_tile(double* __restrict__ Zt, double* __restrict__ part, const double* __restrict__ ph, double* __restrict__ prevs,
                                              const bool first, const bool left_side, const int Dp, const int Dout, const int d, const int count,
                                              const double (&bv)[8], double* __restrict__ out, const int cap, Ahead&& ahead) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, kq = lane >> 4;
    const int nt = wave & 1, q = wave >> 1;
    const int Z = Dp * d, ZP = (Z + 3) & ~3, nsteps = ZP >> 2, ks4 = env_ks4(nsteps);
    // (LDS-only barriers: __syncthreads() would also wait for the acknowledgement of the last step's stores and for the operands
    // requested two steps ahead - the very round trips the walk is built to hide)
    lds_barrier();                              // (also: the previous step's rows are in prevs, its Zt is consumed)
    // ---- the Khatri-Rao tile of this step: Zt[i][z] = prev_i[a] phi_i[s], left z = a d + s, right z = s Dp + a ----
    {
        const int row = tid >> 5, a = tid & 31;  // 16 rows x 32 bond entries
        const double pa = (a < Dp && row < count) ? (first ? 1.0 : prevs[row * EW_PS + a]) : 0.0;
        if (a < Dp) {
            for (int s = 0; s < d; ++s) Zt[row * EW_ZS + (left_side ? a * d + s : s * Dp + a)] = pa * ph[row * EW_PHS + s];
        }
        for (int z = Z + a; z < ZP; z += 32) Zt[row * EW_ZS + z] = 0.0;
    }
    lds_barrier();
    ahead();
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (nt * 16 < Dout) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int step = q * ks4 + u;
            acc = mfma_f64(Zt[i16 * EW_ZS + 4 * min(step, nsteps - 1) + kq], bv[u], acc);      // (bv is zero beyond the contraction)
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(q * 2 + nt) * 256 + r * 64 + lane] = acc[r];
    lds_barrier();
    {
        const int tnt = tid >> 8, e = tid & 255;
        const double sum = (part[tnt * 256 + e] + part[(2 + tnt) * 256 + e]) + (part[(4 + tnt) * 256 + e] + part[(6 + tnt) * 256 + e]);
        const int i = ((e >> 4) & 3) + 4 * (e >> 6), c = tnt * 16 + (e & 15);
        if (i < count && c < Dout) {
            if (WT) __hip_atomic_store(out + (int64_t)i * cap + c, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else out[(int64_t)i * cap + c] = sum;
        }
        prevs[i * EW_PS + c] = sum;
    }
}

}  // namespace mpst
