// edge_scores.hip -- additive (GAT-style) attention scores on the CSR pattern of the selected hops, and their backward:
//
//     forward    pre[e]      = l[i*ldl + s] + r[j*ldr + s]                     for every stored entry e = (i, j) of selected hop s
//                score[s][e] = pre > 0 ? pre : pre * slope
//     backward   t[e]        = pre > 0 ? g[s][e] : g[s][e] * slope              (pre recomputed; NaN takes the slope branch)
//                dl[i*lddl + s] = sum of t[e] over row i of A_k                 (the ROW side: forward rowptr / colidx only)
//                dr[j*lddr + s] = sum of t[e] over column j of A_k              (the COLUMN side: row j of A_k^T through perm)
//
// -- the first link of the attention chain (scores -> row_softmax.hip -> hop SpMM with values -> sddmm.hip) and the link that
// takes its gradient back to the nodes.  fp32 only.  A translation unit of its own: no existing kernel is compiled differently.
//
// Mapping (gfx950, wave64; streaming kernels: no atomics, no scratch, 16 bytes of LDS on the backward's long path only):
//   * the pattern walk of pattern_walk.hip.h: a wave owns rows_per_wave consecutive rows;
//   * forward (no reduction): the entries of these rows in one hop are ONE contiguous range, streamed 64 entries at a time, each
//     lane finding the row of its entry by bisection among the wave's row pointers;
//   * backward: per hop the wave walks its rows FOUR at a time, lane group gi (16 lanes) standing for row i0 + gi:
//       - all four segments <= 16 entries: one 16-lane group per segment, one colidx load instruction for the four (consecutive
//         rows of one hop are consecutive in memory);
//       - all four <= 64: one entry per lane and segment, the loads of the four going out before the first reduction;
//       - otherwise one segment after the other on the whole wave, 256 entries (four per lane) per iteration;
//   * segments of the plan's long-segment list belong to workgroups of their own: forward -- thread t takes the entries = t
//     (mod 256); backward -- wave w takes the 64-entry chunks = w (mod 4), four per lane in flight, and the four wave totals
//     cross through LDS.
//   The column side is THE SAME device function on the plan's adjoint operand: t_rowptr / t_colidx give (j, i), perm[e'] the
//   forward entry whose g is read; nothing of size nnz is materialised.  Its long list is the adjoint launch's: one entry per
//   row that is long in ANY selected hop, and the workgroup serves every selected hop of that row.
//   Loads of colidx, perm, g (row side) and stores of score are lane-contiguous; r[j], l[i] and g[perm] are 4-byte gathers.
//
// Arithmetic of the backward (documented in include/h2gcn_hip.h): the row softmax's tree, written once in segment_ops.hip.h -- the
// 16-lane group, the wave and the workgroup give the same bits, and an empty segment gives +0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "segment_ops.hip.h"

namespace h2gcn {
namespace edge_scores {

using namespace pattern;
struct Params {
    Geom geom;                              // of the walked operand: A_k (forward, row side) or A_k^T (column side)
    const int32_t* idx[H2GCN_MAX_HOPS];     // its colidx: the OTHER node of every walked entry   (the selected hops, packed)
    const uint32_t* perm[H2GCN_MAX_HOPS];   // column side: the forward entry behind every walked entry
    const float* g[H2GCN_MAX_HOPS];         // backward: dscores, in forward entry order
    float* score[H2GCN_MAX_HOPS];           // forward: scores
    const float* self;                      // the walked rows' operand: l (forward, row side) / r (column side) ...
    const float* other;                     // ... and the gathered one
    float* out;                             // backward: dl (row side) / dr (column side)
    int64_t ld_self, ld_other, ld_out;
    float slope;
};

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(kBlock) void edge_scores_hops_kernel(const Params p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        const float self = p.self[row * p.ld_self + s];
        const int32_t* idx = p.idx[s];
        float* score = p.score[s];
        for (int64_t e = beg + threadIdx.x; e < end; e += kBlock) score[e] = leaky(self + p.other[(int64_t)idx[e] * p.ld_other + s], p.slope);
        return;
    }
    // ---- the tile walk.  The entries of a wave's rows in one hop are ONE contiguous range: the wave streams it 64 entries at a
    // time and every lane finds the row of its entry by bisection among the wave's row pointers (the last row i whose pointer is
    // <= e; the pointers of rows beyond n_rows equal the end of the range, so they are never chosen).
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int rpw = p.geom.rows_per_wave;
    int top = 1;
    while (2 * top < rpw) top *= 2;
    for (s = 0; s < p.geom.n_sel; ++s) {
        const int32_t* __restrict__ idx = p.idx[s];
        float* __restrict__ score = p.score[s];
        const int l0 = rp_lane(p.geom, s, 0);
        const int64_t first = readlane64(rp, l0), last = readlane64(rp, l0 + rpw);
        for (int64_t e0 = first; e0 < last; e0 += kWave) {   // (wave-uniform: bpermute needs every lane)
            const int64_t e = e0 + lane;
            int i = 0;
            for (int step = top; step > 0; step >>= 1) {
                const int c = i + step < rpw ? i + step : rpw;
                if (bpermute64(rp, l0 + c) <= e) i = c;      // (c = rpw: `last`, <= e only in a lane beyond the range)
            }
            const int64_t lo = bpermute64(rp, l0 + i), hi = bpermute64(rp, l0 + (i < rpw ? i + 1 : rpw));   // the segment of e
            if (e < last && hi - lo < p.geom.long_threshold)   // (a long segment: a workgroup of its own)
                score[e] = leaky(p.self[(row0 + i) * p.ld_self + s] + p.other[(int64_t)idx[e] * p.ld_other + s], p.slope);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward
// t of walked entry e of selected hop s.  T: the column side -- e is an entry of A_k^T, g sits at the forward entry perm[e].
template <bool T>
__device__ __forceinline__ float term(const Params& p, int s, float self, int64_t e) {
    const int64_t o = p.idx[s][e];
    const float g = p.g[s][T ? (int64_t)p.perm[s][e] : e];
    const float oth = p.other[o * p.ld_other + s];
    const float pre = T ? oth + self : self + oth;   // l[i] + r[j]
    return pre > 0.f ? g : g * p.slope;
}

template <bool T>
__global__ __launch_bounds__(kBlock) void edge_scores_backward_kernel(const Params p) {
    __shared__ float lds[kWavesPerBlock];   // long segments: the wave totals
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x < p.geom.n_long) {
        // ---- a long segment (row side) / every selected hop of a long row (column side): 64-entry chunks over the 4 waves ----
        const int64_t e = p.geom.long_list[blockIdx.x];
        const int64_t row = T ? e : e >> 4;
        const int s0 = T ? 0 : (int)(e & 15), s1 = T ? p.geom.n_sel : s0 + 1;
        for (int s = s0; s < s1; ++s) {
            const int64_t beg = p.geom.rowptr[s][row], end = p.geom.rowptr[s][row + 1];
            const float self = p.self[row * p.ld_self + s];
            const float total = segment_sum<kWavesPerBlock>([&](int64_t m) { return term<T>(p, s, self, beg + m); }, end - beg, lane, wave, lds);
            if (threadIdx.x == 0) p.out[row * p.ld_out + s] = total;
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows, four at a time ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int rpw = p.geom.rows_per_wave;
    for (int s = 0; s < p.geom.n_sel; ++s)
        for (int i0 = 0; i0 < rpw; i0 += 4) {
            int64_t beg, n;
            group_segment<T>(p.geom, s, i0, row0, rp, lane, &beg, &n);
            if (__ballot(n >= 0) == 0ull) continue;
            if (__ballot(n > kGroup) == 0ull) {
                // one 16-lane group per segment: P[q] = +0 + t, the partials 16 .. 255 are +0
                const int q = lane & (kGroup - 1);
                const int64_t row = row0 + i0 + (lane >> 4);
                float t = 0.f;
                if (q < n) t = term<T>(p, s, p.self[row * p.ld_self + s], beg + q);
                const float total = bfly16<Add>(0.f + t);
                if (q == 0 && n >= 0) p.out[row * p.ld_out + s] = total;   // (an empty segment: +0)
                continue;
            }
            if (__ballot(n > kWave) == 0ull) {
                // one entry per lane and segment: the four segments' loads go out before the first butterfly.  P[lane] = +0 + t,
                // the partials 64 .. 255 are +0
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t bk = readlane64(beg, k * kGroup), nk = readlane64(n, k * kGroup);
                    t[k] = 0.f;
                    if (lane < nk) t[k] = term<T>(p, s, p.self[(row0 + i0 + k) * p.ld_self + s], bk + lane);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (readlane64(n, k * kGroup) < 0) continue;   // (wave-uniform)
                    const float total = bfly64<Add>(0.f + t[k]);
                    if (lane == 0) p.out[(row0 + i0 + k) * p.ld_out + s] = total;
                }
                continue;
            }
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t bk = readlane64(beg, k * kGroup), nk = readlane64(n, k * kGroup);
                if (nk < 0) continue;   // (wave-uniform)
                const int64_t row = row0 + i0 + k;
                const float self = p.self[row * p.ld_self + s];
                const float total = segment_sum<1>([&](int64_t m) { return term<T>(p, s, self, bk + m); }, nk, lane, 0, nullptr);
                if (lane == 0) p.out[row * p.ld_out + s] = total;
            }
        }
}

}  // namespace edge_scores
}  // namespace h2gcn

extern "C" {

int h2gcn_edge_scores_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                               int64_t ldr, float negative_slope, float* const* scores_dev, void* stream) {
    using namespace h2gcn::edge_scores;
    return scores_forward<Params, false>(edge_scores_hops_kernel, plan, hop_mask, l_dev, ldl, r_dev, ldr, 1, negative_slope, scores_dev, stream);
}

int h2gcn_edge_scores_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                        const float* r_dev, int64_t ldr, float negative_slope, const float* const* dscores_dev,
                                        float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, void* stream) {
    using namespace h2gcn::edge_scores;
    return scores_backward<Params, false>(edge_scores_backward_kernel<false>, edge_scores_backward_kernel<true>, plan, hop_mask, l_dev, ldl,
                                          r_dev, ldr, 1, negative_slope, dscores_dev, dl_dev, lddl, dr_dev, lddr, stream);
}

}  // extern "C"
