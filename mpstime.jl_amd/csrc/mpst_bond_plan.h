// What the per-bond launch chain decides on the host from plain integers: the bond order of a sweep, the environment step of a site,
// and which instantiation of the headline kernels a shape gets.  Plain C++17 without HIP, so that it is tested on the host
// (tests/bond_plan_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpst {

// ---- bond order of one sweep (RealRealHighDimension.jl:731, :776) -------------------------------------------------------
// Slot k of a sweep over nb = T - 1 bonds: nb - 1 .. 0 going left, then 0 .. nb - 1 going right.  next_lid: the bond of slot
// k + 1, whose tensor this bond's last launch may assemble (-1: none, or the caller took it away - `unchained`: the tensor is
// rescaled first, or the caches are rebuilt in between); chains_into_next: that bond is the neighbour in the direction of travel
// (everywhere but at the turning point, where the same bond comes again) - the fused chains hand a tensor on only then.
struct BondSlot {
    int lid, going_left, next_lid;
    bool chains_into_next;
    BondSlot unchained() const { return {lid, going_left, -1, false}; }
};
inline BondSlot bond_slot(int k, int nb) {
    auto at = [nb](int q) { return q < nb ? nb - 1 - q : q - nb; };
    BondSlot b{at(k), k < nb, k + 1 < 2 * nb ? at(k + 1) : -1, false};
    b.chains_into_next = b.next_lid >= 0 && b.next_lid == (b.going_left ? b.lid - 1 : b.lid + 1);
    return b;
}
// have_bt of the slot after `prev` (the caller's: it knows where it started and what it took away): the tensor is there iff the
// launches enqueued for `prev`, in this call, were told to assemble it
inline bool assembles_next(const BondSlot& prev, bool fused) { return fused ? prev.chains_into_next : prev.next_lid >= 0; }

// ---- the environment step (update_caches!, construct_caches) --------------------------------------------------------------
// Row out_site of LE (left_side) or RE from row prev_site of the same side (-1: the chain end, no row) and the tensor of `site`;
// prev_bond / out_bond: the bonds whose dimensions the two rows have.
struct EnvStep { int site, left_side, prev_site, prev_bond, out_bond, out_site; };
inline EnvStep env_step(int site, int left_side, int T) {
    if (left_side) return {site, 1, site > 0 ? site - 1 : -1, site, site + 1, site};
    return {site, 0, site < T - 1 ? site + 1 : -1, site + 1, site, site};
}
// the step that follows bond (lid, lid + 1): going left the right site's RE row, going right the left site's LE row
inline EnvStep env_step_of_bond(int lid, int going_left, int T) { return going_left ? env_step(lid + 1, 0, T) : env_step(lid, 1, T); }
// row `site` of [T][stride] rows (stride = N * cap), null for site -1; env_row_e: elements of esz bytes
template <typename R> inline R* env_row(R* base, int site, int64_t stride) { return site < 0 ? nullptr : base + site * stride; }
inline void* env_row_e(void* base, int site, int64_t stride, size_t esz) { return site < 0 ? nullptr : (char*)base + (size_t)(site * stride) * esz; }

// ---- the instantiations of the headline kernels, once: the launchers and b2_init_attrs (mpst_fused.hip) expand these lists, the
// choosers below return a row of them ----
#define YHAT_S_LIST(X) /* LM, D4, V2 */ X(2, true, true) X(2, true, false) X(2, false, false) X(4, false, false)
#define GRAD_S_LIST(X) /* AW2, D2, FS, KC, NW, threads */                                                                         \
    X(2, 1, 0, 256, 8, 512) X(1, 2, 0, 256, 8, 512) X(1, 1, 25, 256, 4, 256) X(1, 1, 25, 256, 8, 512) X(1, 1, 0, 256, 8, 512)

// k_yhat_s: row 0 loads its rows 16 bytes at a time (d = 4, even capacity; v1_forced: MPST_YS_V1 takes it away)
inline int yhat_s_variant(int d, int cap, bool v1_forced) {
    if (d == 4 && cap <= 32 && !(cap & 1) && !v1_forced) return 0;
    if (cap <= 32 && d == 4) return 1;
    if (cap <= 32) return 2;
    return 3;
}
// k_grad_s: row 0 d = 2, 3 (more than 8 left indices per block), row 1 d = 9..16, rows 2 and 3 d = 4 with 4 or 8 waves
inline int grad_s_variant(int d, int b2_nw) {
    const int aw = 32 / d > 1 ? 32 / d : 1;
    if (aw > 8) return 0;
    if (d > 8) return 1;
    if (d == 4 && b2_nw == 4) return 2;
    if (d == 4) return 3;
    return 4;
}

}  // namespace mpst
