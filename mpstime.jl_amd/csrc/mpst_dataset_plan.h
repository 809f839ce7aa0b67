// The host-side plan of a data set: what mpst_set_dataset / mpst_encode_dataset derive from the class labels before a byte is
// uploaded - class counts, class-pure tiles and chunks, the parts of the fused gradient kernel.  A pure function of the labels in
// plain C++17, no HIP: tests/test_dataset_plan.py compiles it alone; mpst_internal.h includes it for everything else.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace mpst {

// A class-pure run of consecutive series (<= 16 for tiles, <= 64 for chunks).
struct Span {
    int32_t start, count, cls, pad;
};

// A part = the series one persistent workgroup of k_bond_fused walks: a class-pure run [start, start+count) of class
// `own`, contracted with the bond tensor of class `cls` (KLD: cls == own; MSE: every class).  Parts are ordered by
// `cls`, so the partial gradients of one class are consecutive.
struct Part {
    int32_t start, count, own, cls;
    int32_t first_of_cls, pad0, pad1, pad2;
};
constexpr int PARTS_TARGET = 128;   // persistent workgroups of the fused gradient kernel (256 for >= 512 tiles of 16 series)
constexpr int TILE_S = 16;    // series per yhat/env tile (one MFMA M-tile)
constexpr int CHUNK_S = 64;   // series per gradient chunk (the GEMM K extent of one partial)
inline int64_t tiles_of(int64_t series) { return (series + TILE_S - 1) / TILE_S; }

struct DataSetPlan {
    std::vector<int64_t> counts, gcounts;   // per-class series counts: local, and over all shards
    int64_t Nglobal = 0;
    std::vector<Span> tiles, chunks;        // class-pure, <= TILE_S / CHUNK_S series each
    std::vector<int32_t> cls_chunk_off;     // [C+1] first chunk of each class
    std::vector<int32_t> cls_off;           // [C+1] first series of each class
    std::vector<Part> parts[2];             // [0] KLD, [1] MSE
    std::vector<int32_t> part_off[2];       // [C+1] first part of each bond-tensor class
    std::vector<double> inv_count;          // [C] 1 / (global series count of the class)
};

struct LabelVerdict {      // what is wrong with label_idx[index] = label, if anything
    enum { OK = 0, OUT_OF_RANGE, UNSORTED } what;
    int64_t index;
    int32_t label;
};

// Fills *p from the labels of N series in C classes, sorted by class (RealRealHighDimension.jl:624), and returns the verdict on them:
// *p is complete only when that is OK.  n_global_per_class: the class counts over all shards, or null (the local ones).
// parts_target_override > 0 replaces the number of parts aimed at (the MPST_PARTS switch, which the caller reads).
inline LabelVerdict plan_dataset(const int32_t* label_idx, int64_t N, int C, const int64_t* n_global_per_class, int parts_target_override,
                                 DataSetPlan* p) {
    *p = DataSetPlan();
    p->counts.assign(C, 0);
    for (int64_t i = 0; i < N; ++i) {
        const int32_t l = label_idx[i];
        if (l < 0 || l >= C) return {LabelVerdict::OUT_OF_RANGE, i, l};
        if (i && l < label_idx[i - 1]) return {LabelVerdict::UNSORTED, i, l};
        p->counts[l]++;
    }
    const std::vector<int64_t>& counts = p->counts;
    p->gcounts = n_global_per_class ? std::vector<int64_t>(n_global_per_class, n_global_per_class + C) : counts;
    p->inv_count.assign(C, 0.0), p->cls_off.assign(C + 1, 0), p->cls_chunk_off.assign(C + 1, 0);
    int64_t tiles_total = 0;
    for (int k = 0; k < C; ++k) {
        const int64_t start = p->cls_off[k];
        for (int64_t o = 0; o < counts[k]; o += TILE_S) p->tiles.push_back({(int32_t)(start + o), (int32_t)std::min<int64_t>(TILE_S, counts[k] - o), k, 0});
        for (int64_t o = 0; o < counts[k]; o += CHUNK_S) p->chunks.push_back({(int32_t)(start + o), (int32_t)std::min<int64_t>(CHUNK_S, counts[k] - o), k, 0});
        p->cls_off[k + 1] = (int32_t)(start + counts[k]);
        p->cls_chunk_off[k + 1] = (int32_t)p->chunks.size();
        tiles_total += tiles_of(counts[k]);
        p->Nglobal += p->gcounts[k];
        if (p->gcounts[k] > 0) p->inv_count[k] = 1.0 / (double)p->gcounts[k];
    }
    // parts of the fused gradient kernel: class-pure runs of whole 16-series tiles, about PARTS_TARGET of them
    int target = tiles_total >= 4 * PARTS_TARGET ? 2 * PARTS_TARGET : PARTS_TARGET;
    if (parts_target_override > 0) target = parts_target_override;
    for (int pk = 0; pk < 2; ++pk) {
        const int tgt = pk ? std::max(1, target / C) : target;      // MSE: every run is walked once per class
        std::vector<Part> runs;
        for (int k = 0; k < C; ++k) {
            const int64_t tk = tiles_of(counts[k]), st = p->cls_off[k];
            if (tk == 0) continue;
            int64_t nk = (tgt * tk + tiles_total / 2) / tiles_total;     // the class' share of the runs: at least one, at most one per tile
            nk = std::max<int64_t>(1, std::min(nk, tk));
            for (int64_t q = 0; q < nk; ++q) {
                const int64_t a = st + tk * q / nk * TILE_S, bnd = std::min(st + tk * (q + 1) / nk * TILE_S, st + counts[k]);
                runs.push_back({(int32_t)a, (int32_t)(bnd - a), k, k, 0, 0, 0, 0});
            }
        }
        p->part_off[pk].assign(C + 1, 0);
        for (int cc = 0; cc < C; ++cc) {
            p->part_off[pk][cc] = (int32_t)p->parts[pk].size();
            for (const Part& r : runs) {
                if (!pk && r.own != cc) continue;
                p->parts[pk].push_back({r.start, r.count, r.own, cc, p->part_off[pk][cc] == (int32_t)p->parts[pk].size() ? 1 : 0, 0, 0, 0});
            }
        }
        p->part_off[pk][C] = (int32_t)p->parts[pk].size();
    }
    return {LabelVerdict::OK, 0, 0};
}

}  // namespace mpst
