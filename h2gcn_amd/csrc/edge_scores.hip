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
// Arithmetic of the backward (documented in include/h2gcn_hip.h): the row softmax's tree -- 256 partials P[m mod 256] starting at
// +0 and accumulated in ascending position m of the segment, four 64-lane xor butterflies W_w, (W_0 + W_1) + (W_2 + W_3).  A
// partial is +0 + t + ..., never -0; a sum of values that are not -0 is not -0 (round to nearest); so every W_w and every
// intermediate of the tree is +0 or not a zero at all, and adding the +0 of a partial (or of a whole wave) that received no entry
// changes no bit.  That is why the 16-lane group (P[16..255] = +0), the wave (4 partials per lane) and the workgroup (1 per lane)
// give the same bits, and why an empty segment gives +0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "pattern_walk.hip.h"

namespace h2gcn {
namespace edge_scores {

using namespace pattern;
constexpr int kGroup = 16;       // lanes of a lane group: the longest segment it serves
constexpr int kPartials = 256;   // partial sums of a segment: entry m belongs to P[m mod 256]
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

// the 64-lane xor butterfly over lane distances 1 .. 32
__device__ __forceinline__ float bfly64(float v) {
    v = bfly16<Add>(v);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

// Lane group gi = lane >> 4 stands for row i0 + gi of the wave: its entries [beg, beg + n) in selected hop s.  n = -1 where the
// group has nothing to write: no such row, or the segment belongs to a long-segment workgroup -- BY_ROW (the adjoint's list):
// the row is long in ANY selected hop.  All 64 lanes must be active.
template <bool BY_ROW>
__device__ __forceinline__ void group_segment(const Geom& g, int s, int i0, int64_t row0, int64_t rp, int lane, int64_t* beg, int64_t* n) {
    const int rpw = g.rows_per_wave;
    const int i = i0 + (lane >> 4);
    const int ic = i < rpw ? i : rpw - 1;
    const int src = rp_lane(g, s, ic);
    *beg = bpermute64(rp, src);
    int64_t len = bpermute64(rp, src + 1) - *beg;
    bool is_long = len >= g.long_threshold;
    if (BY_ROW)
        for (int s2 = 0; s2 < g.n_sel; ++s2) {
            const int src2 = rp_lane(g, s2, ic);
            is_long = is_long || bpermute64(rp, src2 + 1) - bpermute64(rp, src2) >= g.long_threshold;
        }
    if (i >= rpw || row0 + i >= g.n_rows || is_long) len = -1;
    *n = len;
}

__device__ __forceinline__ float leaky(float pre, float slope) { return pre > 0.f ? pre : pre * slope; }

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

// The sum of a segment of any length n >= 0 on NW waves (1: a wave of the tile walk, four partials per lane; 4: the workgroup of a
// long segment, wave w holding the partials 64w .. 64w+63).  Either way lane l of accumulator / wave w holds P[64w + l],
// accumulated in ascending m, with four entries per lane in flight.  NW = 4: every thread of the block must call; `lds` is free
// for the next call on return.
template <bool T, int NW>
__device__ __forceinline__ float segment_sum(const Params& p, int s, float self, int64_t beg, int64_t n, int lane, int wave, float* lds) {
    constexpr int NA = 4 / NW;                           // accumulators per lane
    constexpr int kStride = NW == 1 ? kWave : kPartials;   // between the four entries of a lane in one iteration
    const int first = NW == 1 ? 0 : wave * kWave;        // (wave-uniform)
    float acc[NA];
#pragma unroll
    for (int u = 0; u < NA; ++u) acc[u] = 0.f;
    for (int64_t base = 0; base < n; base += 4 * kStride) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t m0 = base + k * kStride + first;
            t[k] = 0.f;
            if (m0 < n) {   // (wave-uniform)
                const bool ok = m0 + lane < n;
                const float v = term<T>(p, s, self, beg + (ok ? m0 + lane : m0));
                t[k] = ok ? v : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[NW == 1 ? k : 0] = acc[NW == 1 ? k : 0] + t[k];   // ascending m within every partial
    }
    if (NW == 1) {
        float W[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            W[u] = 0.f;
            if (u * kWave < n) W[u] = bfly64(acc[u < NA ? u : 0]);   // (wave-uniform; a wave of +0 sums to +0)
        }
        return (W[0] + W[1]) + (W[2] + W[3]);
    }
    const float Ww = bfly64(acc[0]);
    if (lane == 0) lds[wave] = Ww;
    __syncthreads();
    const float total = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return total;
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
            const float total = segment_sum<T, kWavesPerBlock>(p, s, self, beg, end - beg, lane, wave, lds);
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
                    const float total = bfly64(0.f + t[k]);
                    if (lane == 0) p.out[(row0 + i0 + k) * p.ld_out + s] = total;
                }
                continue;
            }
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t bk = readlane64(beg, k * kGroup), nk = readlane64(n, k * kGroup);
                if (nk < 0) continue;   // (wave-uniform)
                const int64_t row = row0 + i0 + k;
                const float total = segment_sum<T, 1>(p, s, p.self[row * p.ld_self + s], bk, nk, lane, 0, nullptr);
                if (lane == 0) p.out[row * p.ld_out + s] = total;
            }
        }
}

// ------------------------------------------------------------------------------------------------------------ host
int check_node_operands(const PatternView& v, const float* l, int64_t ldl, const float* r, int64_t ldr) {
    if (ldl < v.n_sel) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldl = %lld < H_sel = %d", (long long)ldl, v.n_sel);
    if (ldr < v.n_sel) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldr = %lld < H_sel = %d", (long long)ldr, v.n_sel);
    if (selected_nnz(v) > 0 && !l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "l is NULL");
    if (selected_nnz(v) > 0 && !r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "r is NULL");
    return H2GCN_OK;
}

void fill(Params* p, const PatternView& v, const float* self, int64_t ld_self, const float* other, int64_t ld_other, float slope) {
    for (int s = 0; s < v.n_sel; ++s) p->idx[s] = v.colidx[s];
    p->self = self, p->ld_self = ld_self;
    p->other = other, p->ld_other = ld_other;
    p->slope = slope;
}

int forward(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr, float slope,
            float* const* scores, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_node_operands(v, l, ldl, r, ldr)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, "scores", scores)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        fill(&p, v, l, ldl, r, ldr, slope);
        for (int s = 0; s < v.n_sel; ++s) p.score[s] = scores[s];
        hipLaunchKernelGGL(edge_scores_hops_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_hops_f32");
    }
}

// One side of the backward, in two steps so that both sides' refusals come before either side's launch.
template <bool T>
struct Side {
    Params p;
    int64_t n_blocks = 0;
    int n_sel = 0;
    int64_t n_rows = 0;

    int prepare(const h2gcn_plan_t* plan, const PatternView& v, const uint32_t* const* perm, const float* self, int64_t ld_self,
                const float* other, int64_t ld_other, float slope, const float* const* g, float* out, int64_t ld_out, hipStream_t stream) {
        memset(&p, 0, sizeof(p));
        n_sel = v.n_sel, n_rows = v.n_rows;
        const int st = launch_geometry(plan, v, stream, &p.geom, &n_blocks, T);
        if (st != H2GCN_OK || n_blocks == 0) {
            p.out = out, p.ld_out = ld_out;
            return st;
        }
        fill(&p, v, self, ld_self, other, ld_other, slope);
        for (int s = 0; s < v.n_sel; ++s) p.g[s] = g[s], p.perm[s] = T ? perm[s] : nullptr;
        p.out = out, p.ld_out = ld_out;
        return H2GCN_OK;
    }
    int run(hipStream_t stream) {
        if (n_blocks == 0) {   // a selection without nonzeros: every segment is empty
            if (n_rows > 0) H2GCN_HIP_TRY(hipMemset2DAsync(p.out, (size_t)p.ld_out * sizeof(float), 0, (size_t)n_sel * sizeof(float), (size_t)n_rows, stream));
            return H2GCN_OK;
        }
        hipLaunchKernelGGL((edge_scores_backward_kernel<T>), dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    }
};

int backward(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr, float slope,
             const float* const* g, float* dl, int64_t lddl, float* dr, int64_t lddr, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v, tv;
        const uint32_t* perm[H2GCN_MAX_HOPS] = {};
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (!dl && !dr) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dl and dr are both NULL: nothing to compute");
        if ((st = check_node_operands(v, l, ldl, r, ldr)) != H2GCN_OK) return st;
        if (dl && lddl < v.n_sel) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddl = %lld < H_sel = %d", (long long)lddl, v.n_sel);
        if (dr && lddr < v.n_sel) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddr = %lld < H_sel = %d", (long long)lddr, v.n_sel);
        if ((st = check_hop_arrays(v, "dscores", g)) != H2GCN_OK) return st;
        if (dr && (st = adjoint_view(plan, hop_mask, &tv, perm)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Side<false> rows;
        Side<true> cols;
        if (dl && (st = rows.prepare(plan, v, nullptr, l, ldl, r, ldr, slope, g, dl, lddl, stream)) != H2GCN_OK) return st;
        if (dr && (st = cols.prepare(plan, tv, perm, r, ldr, l, ldl, slope, g, dr, lddr, stream)) != H2GCN_OK) return st;
        if (dl && (st = rows.run(stream)) != H2GCN_OK) return st;
        if (dr && (st = cols.run(stream)) != H2GCN_OK) return st;
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_backward_hops_f32");
    }
}

}  // namespace edge_scores
}  // namespace h2gcn

extern "C" {

int h2gcn_edge_scores_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                               int64_t ldr, float negative_slope, float* const* scores_dev, void* stream) {
    return h2gcn::edge_scores::forward(plan, hop_mask, l_dev, ldl, r_dev, ldr, negative_slope, scores_dev, stream);
}

int h2gcn_edge_scores_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                        const float* r_dev, int64_t ldr, float negative_slope, const float* const* dscores_dev,
                                        float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, void* stream) {
    return h2gcn::edge_scores::backward(plan, hop_mask, l_dev, ldl, r_dev, ldr, negative_slope, dscores_dev, dl_dev, lddl, dr_dev,
                                        lddr, stream);
}

}  // extern "C"
