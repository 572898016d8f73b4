// row_softmax.hip -- softmax over every (row, hop) segment of the CSR pattern of the selected hops, and its backward:
//
//     forward    alpha[e]  = exp(score[e] - m) / S        m = max_j score_j,  S = sum_j exp(score_j - m)
//     backward   dscore[e] = alpha[e] * (dalpha[e] - D)   D = sum_j alpha_j * dalpha_j
//
// over the entries j = 0..n-1 of the segment [rowptr[i], rowptr[i+1]) in stored order -- the attention coefficients over the
// 1-hop / 2-hop rings that hop_spmm(plan, x, values=[...]) consumes.  fp32 only.  A translation unit of its own: no existing
// kernel is compiled differently because of it.
//
// Mapping (gfx950, wave64; a streaming kernel: no atomics, no scratch, a few bytes of LDS on the long path only):
//   * the pattern walk of pattern_walk.hip.h: a wave owns rows_per_wave consecutive rows;
//   * per hop the wave walks its rows FOUR at a time (a step), lane group gi (16 lanes) standing for row i0 + gi:
//       - all four segments <= 16 entries: one 16-lane group per segment, one load and one store instruction for the four
//         (consecutive rows of one hop are consecutive in memory, so the load is contiguous up to the masked lanes);
//       - all four <= 64 entries: one register per segment;
//       - all four <= 256 entries: four registers per segment (one read, one write), the loads of the four segments go out
//         before the first reduction;
//       - otherwise one segment after the other, those beyond 256 entries in passes over memory;
//     the loads of step t + 1 (first two classes) are issued before step t computes;
//   * segments of the plan's forward long-segment list (>= long_row_threshold entries) belong to workgroups of their own: wave w
//     takes the 64-entry chunks = w (mod 4), the wave maxima and wave totals cross through 8 floats of LDS.  Up to 1024 entries
//     stay in registers (four per lane: one read, one write); longer ones run in passes of 1024 entries (max; sum; recompute
//     and store -- backward two) that re-read from L2, four loads per lane in flight.
//   All loads and stores are lane-contiguous; a lane writes only entries it has read (alpha may overwrite scores, dscore dalpha).
//
// Arithmetic (documented in include/h2gcn_hip.h): ONE order per segment, a function of its contents alone -- the tree of
// segment_ops.hip.h, which is why all the mappings above give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "segment_ops.hip.h"

namespace h2gcn {
namespace row_softmax {

using namespace pattern;

struct Params {
    Geom geom;
    const float* a[H2GCN_MAX_HOPS];          // forward: scores; backward: alpha   (the selected hops, packed as geom.rowptr)
    const float* g[H2GCN_MAX_HOPS];          // backward: dalpha
    float* out[H2GCN_MAX_HOPS];              // forward: alpha; backward: dscores
};

// ---- a segment of at most 64 entries on the wave, one register: x / y are entry `lane`
template <bool BWD>
__device__ __forceinline__ void seg64(float x, float y, bool ok, float* dst) {
    if (!BWD) {
        float m = bfly64<Max>(x);
        if (__ballot(x != x) != 0ull) m = quiet_nan();
        const float e = ok ? exp_t(x - m) : 0.f;
        const float S = bfly64<Add>(e);              // = (W_0 + 0) + (0 + 0)
        const float r = 1.0f / S;
        if (ok) *dst = e * r;
    } else {
        const float D = bfly64<Add>(__builtin_fmaf(x, y, 0.f));
        if (ok) *dst = x * (y - D);
    }
}

// ---- a segment of at most 256 entries on the wave, four registers per lane: one read (load256), one write (seg256).  Pointers
// at the segment's first entry; len = 0 loads nothing.
template <bool BWD>
__device__ __forceinline__ void load256(const float* a, const float* g, int len, int lane, float (&x)[4], float (&y)[4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int j = w * kWave + lane;
        x[w] = j < len ? a[j] : (BWD ? 0.f : neg_inf());
        y[w] = BWD && j < len ? g[j] : 0.f;
    }
}
template <bool BWD>
__device__ __forceinline__ void seg256(float (&x)[4], const float (&y)[4], float* out, int len, int lane) {
    float m = 0.f;
    if (!BWD) {
        m = bfly64<Max>(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
        if (__ballot(x[0] != x[0] || x[1] != x[1] || x[2] != x[2] || x[3] != x[3]) != 0ull) m = quiet_nan();
    }
    float W[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int j = w * kWave + lane;
        if (!BWD) x[w] = j < len ? exp_t(x[w] - m) : 0.f;                 // x becomes e
        W[w] = 0.f;
        if (w * kWave < len) W[w] = bfly64<Add>(BWD ? __builtin_fmaf(x[w], y[w], 0.f) : x[w]);   // (wave-uniform)
    }
    const float T = (W[0] + W[1]) + (W[2] + W[3]);
    const float r = 1.0f / T;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int j = w * kWave + lane;
        if (j < len) out[j] = BWD ? x[w] * (y[w] - T) : x[w] * r;
    }
}


// ---- the tile walk.  A STEP is four consecutive rows of one hop, lane group gi standing for row i0 + gi; its class is
// wave-uniform.  step_begin reads the step's row pointers and, for the two register-light classes, issues its loads; the kernel
// begins step t + 1 before it finishes step t, so the loads of two steps are in flight (the segments of different steps never
// overlap, so reading ahead of the previous step's stores is safe for the in-place calls too).
enum { kNone = 0, kGroups = 1, kQuad = 2, kRegs = 3, kMixed = 4 };
//   kGroups: all four segments <= 16 entries -- one 16-lane group each: one load and one store instruction for the four
//   kQuad:   all four <= 64 -- one register each
//   kRegs:   all four <= 256 -- four registers each, the loads of the four segments go out before the first reduction
//   kMixed:  one after the other; the segments beyond 256 entries in passes

struct Step {
    int s;         // hop slot
    int cls;
    int64_t beg;   // first entry and length of the segment of the lane's own group
    int n;         // (0: nothing to do -- an empty row, a row beyond the wave's, a long segment)
    float x[4], y[4];   // kGroups: [0] = entry lane & 15 of the group's segment; kQuad: [gi] = entry `lane` of segment gi
};

template <bool BWD>
__device__ __forceinline__ void step_begin(const Params& p, int t, int quads, int64_t row0, int64_t rp, int lane, Step& st) {
    const int rpw = p.geom.rows_per_wave;
    const int s = t / quads, i = 4 * (t - s * quads) + (lane >> 4);
    const int src = rp_lane(p.geom, s, i < rpw ? i : rpw - 1);
    const int64_t beg = bpermute64(rp, src);
    int64_t n = bpermute64(rp, src + 1) - beg;
    if (i >= rpw || row0 + i >= p.geom.n_rows || n >= p.geom.long_threshold) n = 0;   // (long segments: workgroups of their own)
    st.s = s;
    st.beg = beg;
    st.n = (int)(n < 0x7fffffff ? n : 0x7fffffff);
    st.cls = __ballot(n > 0) == 0ull ? kNone : __ballot(n > kGroup) == 0ull ? kGroups : __ballot(n > kWave) == 0ull ? kQuad
             : __ballot(n > kPartials) == 0ull ? kRegs : kMixed;
    const float pad = BWD ? 0.f : neg_inf();
#pragma unroll
    for (int k = 0; k < 4; ++k) st.x[k] = pad, st.y[k] = 0.f;
    const float* a = p.a[s];
    const float* g = p.g[s];
    if (st.cls == kGroups) {
        const int q = lane & (kGroup - 1);
        if (q < st.n) {
            st.x[0] = a[beg + q];
            if (BWD) st.y[0] = g[beg + q];
        }
    } else if (st.cls == kQuad) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t b = readlane64(beg, k * kGroup);
            if (lane < __builtin_amdgcn_readlane(st.n, k * kGroup)) {
                st.x[k] = a[b + lane];
                if (BWD) st.y[k] = g[b + lane];
            }
        }
    }
}

template <bool BWD>
__device__ __forceinline__ void step_finish(const Params& p, Step& st, int lane) {
    if (st.cls == kNone) return;
    const float* a = p.a[st.s];
    const float* g = BWD ? p.g[st.s] : nullptr;
    float* out = p.out[st.s];
    if (st.cls == kGroups) {
        const int q = lane & (kGroup - 1);
        seg16<BWD>(st.x[0], st.y[0], q < st.n, out + st.beg + q, lane);
        return;
    }
    int64_t b[4];
    int n[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = readlane64(st.beg, k * kGroup);
        n[k] = __builtin_amdgcn_readlane(st.n, k * kGroup);
    }
    if (st.cls == kQuad) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (n[k] > 0) seg64<BWD>(st.x[k], st.y[k], lane < n[k], out + b[k] + lane);   // (wave-uniform)
    } else if (st.cls == kRegs) {
        float x[4][4], y[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load256<BWD>(a + b[k], g + b[k], n[k], lane, x[k], y[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (n[k] > 0) seg256<BWD>(x[k], y[k], out + b[k], n[k], lane);
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const int64_t bk = readlane64(st.beg, k * kGroup);
            const int nk = __builtin_amdgcn_readlane(st.n, k * kGroup);
            if (nk <= 0) continue;
            if (nk <= kPartials) {
                float x[4], y[4];
                load256<BWD>(a + bk, g + bk, nk, lane, x, y);
                seg256<BWD>(x, y, out + bk, nk, lane);
            } else {
                loop_segment<BWD, 1, false>(a + bk, g + bk, out + bk, nk, kUnitStride, lane, 0, nullptr);
            }
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(kBlock) void row_softmax_hops_kernel(const Params p) {
    __shared__ float lds[8];   // long segments: wave maxima [0..3], wave totals [4..7]
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        if (end <= beg) return;   // (the same for the whole block)
        loop_segment<BWD, kWavesPerBlock, false>(p.a[s] + beg, BWD ? p.g[s] + beg : nullptr, p.out[s] + beg, end - beg, kUnitStride, lane,
                                                 wave, lds);
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows, four at a time ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int quads = (p.geom.rows_per_wave + 3) >> 2, n_steps = p.geom.n_sel * quads;
    Step cur;
    step_begin<BWD>(p, 0, quads, row0, rp, lane, cur);
    for (int t = 0; t < n_steps; ++t) {
        Step next;
        next.cls = kNone;
        if (t + 1 < n_steps) step_begin<BWD>(p, t + 1, quads, row0, rp, lane, next);   // its loads fly while this step computes
        step_finish<BWD>(p, cur, lane);
        cur = next;
    }
}

}  // namespace row_softmax
}  // namespace h2gcn

extern "C" {

int h2gcn_row_softmax_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* scores, float* const* alpha,
                               void* stream) {
    using namespace h2gcn::row_softmax;
    return softmax_launch<Params, false, false>(row_softmax_hops_kernel<false>, plan, hop_mask, scores, "scores", nullptr, "", alpha, "alpha", 1,
                                                stream);
}

int h2gcn_row_softmax_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* alpha,
                                        const float* const* dalpha, float* const* dscores, void* stream) {
    using namespace h2gcn::row_softmax;
    return softmax_launch<Params, false, true>(row_softmax_hops_kernel<true>, plan, hop_mask, alpha, "alpha", dalpha, "dalpha", dscores,
                                               "dscores", 1, stream);
}

}  // extern "C"
