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
// Arithmetic (documented in include/h2gcn_hip.h): ONE order per segment, a function of its contents alone -- 256 partials
// P[j mod 256] accumulated in ascending j, four 64-lane xor butterflies, (W0 + W1) + (W2 + W3).  A partial without an entry is +0
// and adding +0 changes no bit here, which is why all the mappings above give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "pattern_walk.hip.h"

namespace h2gcn {
namespace row_softmax {

using namespace pattern;
constexpr int kGroup = 16;       // lanes of a lane group: the longest segment it serves
constexpr int kPartials = 256;   // partial sums of a segment: entry j belongs to P[j mod 256]

struct Params {
    Geom geom;
    const float* a[H2GCN_MAX_HOPS];          // forward: scores; backward: alpha   (the selected hops, packed as geom.rowptr)
    const float* g[H2GCN_MAX_HOPS];          // backward: dalpha
    float* out[H2GCN_MAX_HOPS];              // forward: alpha; backward: dscores
};

struct Max {   // (drops NaN like v_max_f32: the callers carry NaN in a flag of their own)
    static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
};

// the 16-lane xor butterfly, and on over distances 16 and 32: the 64 lanes of the wave
template <typename Op>
__device__ __forceinline__ float bfly64(float v) {
    v = bfly16<Op>(v);
    v = Op::op(v, __shfl_xor(v, 16));
    v = Op::op(v, __shfl_xor(v, 32));
    return v;
}

// THE exponential of every path: v_exp_f32 (2^x, 1 ulp) on the fp32 product t * log2(e)
__device__ __forceinline__ float exp_t(float t) { return __builtin_amdgcn_exp2f(t * 1.44269504088896340736f); }

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ float neg_inf() { return __int_as_float((int)0xff800000u); }

// ---- a segment of at most 16 entries on the lane's own 16-lane group: x / y are entry q = lane & 15 (padding where !ok)
template <bool BWD>
__device__ __forceinline__ void seg16(float x, float y, bool ok, float* dst, int lane) {
    if (!BWD) {
        const unsigned long long nan_lanes = __ballot(x != x);
        float m = bfly16<Max>(x);
        if ((nan_lanes >> (lane & 48)) & 0xffffull) m = quiet_nan();
        const float e = ok ? exp_t(x - m) : 0.f;    // P[q] = +0 + e
        const float S = bfly16<Add>(e);              // = W_0: the partials 16 .. 255 are +0
        const float r = 1.0f / S;
        if (ok) *dst = e * r;
    } else {
        const float D = bfly16<Add>(__builtin_fmaf(x, y, 0.f));
        if (ok) *dst = x * (y - D);
    }
}

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

// ---- one segment of any length on NW waves (1: a wave of the tile walk, four accumulators per lane; 4: the workgroup of a long
// segment, wave w taking the 64-entry chunks = w (mod 4), one accumulator per lane).  Either way lane l of accumulator / wave w
// holds the partial P[64 w + l], accumulated in ascending j, and an iteration covers NW * 256 entries with FOUR loads per lane in
// flight.  A segment that fits one iteration (256 entries on one wave, 1024 on the workgroup) stays in registers: one read, one
// write; a longer one runs in passes (max; sum; recompute and store -- backward two) that re-read from L2.
template <bool BWD, int NW>
struct Span {
    static constexpr int NA = 4 / NW;   // accumulators per lane
    float x[NW][NA], y[NW][NA];
    __device__ __forceinline__ int64_t index(int64_t base, int first, int c, int u) const { return base + c * kPartials + first + u * kWave; }
    __device__ __forceinline__ void fetch(const float* a, const float* g, int64_t base, int first, int64_t len) {
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                const int64_t j = index(base, first, c, u);
                x[c][u] = j < len ? a[j] : (BWD ? 0.f : neg_inf());
                y[c][u] = BWD && j < len ? g[j] : 0.f;
            }
    }
};

template <bool BWD, int NW>
__device__ __forceinline__ void loop_segment(const float* a, const float* g, float* out, int64_t len, int lane, int wave, float* lds) {
    constexpr int NA = 4 / NW;
    constexpr int kSpan = NW * kPartials;
    const int first = NW == 1 ? lane : wave * kWave + lane;
    const bool single = len <= kSpan;   // (wave- and block-uniform)
    Span<BWD, NW> sp;
    if (single) sp.fetch(a, g, 0, first, len);
    float m = 0.f;
    if (!BWD) {
        float mx = neg_inf();
        bool nn = false;
        for (int64_t base = 0; base < len; base += kSpan) {
            if (!single) sp.fetch(a, g, base, first, len);
#pragma unroll
            for (int c = 0; c < NW; ++c)
#pragma unroll
                for (int u = 0; u < NA; ++u) {
                    mx = fmaxf(mx, sp.x[c][u]);
                    nn = nn || sp.x[c][u] != sp.x[c][u];
                }
        }
        m = bfly64<Max>(mx);
        if (__ballot(nn) != 0ull) m = quiet_nan();
        if (NW > 1) {
            if (lane == 0) lds[wave] = m;
            __syncthreads();
            const float m0 = lds[0], m1 = lds[1], m2 = lds[2], m3 = lds[3];
            m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
            if (m0 != m0 || m1 != m1 || m2 != m2 || m3 != m3) m = quiet_nan();
        }
    }
    float acc[NA];
#pragma unroll
    for (int u = 0; u < NA; ++u) acc[u] = 0.f;
    for (int64_t base = 0; base < len; base += kSpan) {
        if (!single) sp.fetch(a, g, base, first, len);
#pragma unroll
        for (int c = 0; c < NW; ++c)       // ascending j within every partial
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                if (!BWD) acc[u] = acc[u] + (sp.index(base, first, c, u) < len ? exp_t(sp.x[c][u] - m) : 0.f);
                else acc[u] = __builtin_fmaf(sp.x[c][u], sp.y[c][u], acc[u]);   // (beyond the segment: fma(0, 0, acc) = acc)
            }
    }
    float T;
    if (NW == 1) {
        float W[NA];
#pragma unroll
        for (int u = 0; u < NA; ++u) W[u] = bfly64<Add>(acc[u]);
        T = (W[0] + W[NA > 1 ? 1 : 0]) + (W[NA > 2 ? 2 : 0] + W[NA > 3 ? 3 : 0]);
    } else {
        const float Ww = bfly64<Add>(acc[0]);
        if (lane == 0) lds[4 + wave] = Ww;
        __syncthreads();
        T = (lds[4] + lds[5]) + (lds[6] + lds[7]);
    }
    const float r = 1.0f / T;
    for (int64_t base = 0; base < len; base += kSpan) {
        if (!single) sp.fetch(a, g, base, first, len);
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                const int64_t j = sp.index(base, first, c, u);
                // (forward: the same instructions on the same operands as in the sum: the same e_j)
                if (j < len) out[j] = BWD ? sp.x[c][u] * (sp.y[c][u] - T) : exp_t(sp.x[c][u] - m) * r;
            }
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
                loop_segment<BWD, 1>(a + bk, g + bk, out + bk, nk, lane, 0, nullptr);
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
        loop_segment<BWD, kWavesPerBlock>(p.a[s] + beg, BWD ? p.g[s] + beg : nullptr, p.out[s] + beg, end - beg, lane, wave, lds);
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

template <bool BWD>
int launch(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* a, const char* a_name, const float* const* g,
           const char* g_name, float* const* out, const char* out_name, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, a_name, a)) != H2GCN_OK) return st;
        if (BWD && (st = check_hop_arrays(v, g_name, g)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, out_name, out)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) {
            p.a[s] = a[s];
            p.g[s] = BWD ? g[s] : nullptr;
            p.out[s] = out[s];
        }
        hipLaunchKernelGGL((row_softmax_hops_kernel<BWD>), dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in row_softmax%s_hops_f32", BWD ? "_backward" : "");
    }
}

}  // namespace row_softmax
}  // namespace h2gcn

extern "C" {

int h2gcn_row_softmax_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* scores, float* const* alpha,
                               void* stream) {
    return h2gcn::row_softmax::launch<false>(plan, hop_mask, scores, "scores", nullptr, "", alpha, "alpha", stream);
}

int h2gcn_row_softmax_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* alpha,
                                        const float* const* dalpha, float* const* dscores, void* stream) {
    return h2gcn::row_softmax::launch<true>(plan, hop_mask, alpha, "alpha", dalpha, "dalpha", dscores, "dscores", stream);
}

}  // extern "C"
