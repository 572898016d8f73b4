// segment_ops.hip.h -- the arithmetic of a segment, written ONCE for every kernel that promises its bits: edge_scores.hip,
// row_softmax.hip, sddmm.hip, spmm_values.hip, attention_heads.hip and attention_fused.hip.  Per head the head-batched calls give the
// bits of the single-head calls, and the fused forward the bits of the chain, because all of them run the code below.
//
// The tree of a segment's sum (documented in include/h2gcn_hip.h): ONE order per segment, a function of its contents alone -- 256
// partials P[j mod 256], starting at +0 and accumulated in ascending position j, four 64-lane xor butterflies W_w over
// P[64w .. 64w+63], (W_0 + W_1) + (W_2 + W_3).  A partial is +0 + t + ..., never -0; a sum of values that are not -0 is not -0 (round
// to nearest); so every W_w and every intermediate of the tree is +0 or not a zero at all, and adding the +0 of a partial (or of a
// whole wave) that received no entry changes no bit.  That is why the 16-lane group (P[16..255] = +0), the wave (four partials per
// lane) and the workgroup (one per lane) give the same bits, and why an empty segment sums to +0.
//
// The host half (below the device code) is the launch path of the edge scores and of the row softmax, single-head and head-batched.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

#include "pattern_walk.hip.h"

namespace h2gcn {
namespace pattern {

constexpr int kGroup = 16;       // lanes of a lane group: the longest segment it serves
constexpr int kPartials = 256;   // partial sums of a segment: entry j belongs to P[j mod 256]

struct Max {   // (drops NaN like v_max_f32: the callers carry NaN in a flag of their own -- a NaN entry makes the maximum NaN)
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

// (NaN takes the slope branch)
__device__ __forceinline__ float leaky(float pre, float slope) { return pre > 0.f ? pre : pre * slope; }

// Lane group gi = lane >> 4 stands for row i0 + gi of the wave: its entries [beg, beg + n) in selected hop s.  n = -1 where the
// group has nothing to write: no such row, or the segment belongs to a long-segment workgroup -- BY_ROW (the adjoint's list):
// the row is long in ANY selected hop (the segment's own length is then tested first, else last: the order of the tests is not
// the result's business, but the compiler's schedule follows it).  All 64 lanes must be active.
template <bool BY_ROW>
__device__ __forceinline__ void group_segment(const Geom& g, int s, int i0, int64_t row0, int64_t rp, int lane, int64_t* beg, int64_t* n) {
    const int rpw = g.rows_per_wave;
    const int i = i0 + (lane >> 4);
    const int ic = i < rpw ? i : rpw - 1;
    const int src = rp_lane(g, s, ic);
    *beg = bpermute64(rp, src);
    int64_t len = bpermute64(rp, src + 1) - *beg;
    bool row_long = BY_ROW && len >= g.long_threshold;
    if (BY_ROW)
        for (int s2 = 0; s2 < g.n_sel; ++s2) {
            const int src2 = rp_lane(g, s2, ic);
            row_long = row_long || bpermute64(rp, src2 + 1) - bpermute64(rp, src2) >= g.long_threshold;
        }
    if (i >= rpw || row0 + i >= g.n_rows || (!BY_ROW && len >= g.long_threshold) || row_long) len = -1;
    *n = len;
}

// ------------------------------------------------------------------------------------------------------------ row softmax
//     forward    alpha_j  = exp(x_j - m) / S        m = max_j x_j,  S = sum_j exp(x_j - m)       (x: scores)
//     backward   dscore_j = x_j * (y_j - D)         D = sum_j x_j * y_j                          (x: alpha, y: dalpha)
// S and D by the tree above; backward entry j adds fma(x_j, y_j, P) to its partial.

// A segment of at most 16 entries on the lane's own 16-lane group: x / y are entry q = lane & 15 (padding where !ok).
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

// The distance between consecutive entries of a segment: kUnitStride (a compile-time 1: the single-head arrays) or a run-time
// int64_t K (one head of an entry-major [nnz, K] array).
constexpr std::integral_constant<int64_t, 1> kUnitStride{};

// The registers of one iteration of loop_segment.
template <bool BWD, int NW>
struct Span {
    static constexpr int NA = 4 / NW;   // accumulators per lane
    float x[NW][NA], y[NW][NA];
    __device__ __forceinline__ int64_t index(int64_t base, int first, int c, int u) const { return base + c * kPartials + first + u * kWave; }
    template <typename Stride>
    __device__ __forceinline__ void fetch(const float* a, const float* g, int64_t base, int first, int64_t len, Stride K) {
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                const int64_t j = index(base, first, c, u);
                x[c][u] = j < len ? a[j * K] : (BWD ? 0.f : neg_inf());
                y[c][u] = BWD && j < len ? g[j * K] : 0.f;
            }
    }
};

// One segment of any length on NW waves (1: a wave of the tile walk, four accumulators per lane; 4: the workgroup of a long segment,
// wave w taking the 64-entry chunks = w (mod 4), one accumulator per lane): entry j at a[j * K].  Either way lane l of accumulator /
// wave w holds the partial P[64 w + l], accumulated in ascending j, and an iteration covers NW * 256 entries with FOUR loads per lane
// in flight.  A segment that fits one iteration (256 entries on one wave, 1024 on the workgroup) stays in registers: one read, one
// write; a longer one runs in passes (max; sum; recompute and store -- backward two) that re-read from L2.  NW = 4: every thread of
// the block must call; SYNC: a barrier at the end frees `lds` for the next call (the next head's wave totals must not overtake this
// head's reads).
template <bool BWD, int NW, bool SYNC, typename Stride>
__device__ __forceinline__ void loop_segment(const float* a, const float* g, float* out, int64_t len, Stride K, int lane, int wave,
                                             float* lds) {
    constexpr int NA = 4 / NW;
    constexpr int kSpan = NW * kPartials;
    const int first = NW == 1 ? lane : wave * kWave + lane;
    const bool single = len <= kSpan;   // (wave- and block-uniform)
    Span<BWD, NW> sp;
    if (single) sp.fetch(a, g, 0, first, len, K);
    float m = 0.f;
    if (!BWD) {
        float mx = neg_inf();
        bool nn = false;
        for (int64_t base = 0; base < len; base += kSpan) {
            if (!single) sp.fetch(a, g, base, first, len, K);
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
        if (!single) sp.fetch(a, g, base, first, len, K);
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
        if (!single) sp.fetch(a, g, base, first, len, K);
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                const int64_t j = sp.index(base, first, c, u);
                // (forward: the same instructions on the same operands as in the sum: the same e_j)
                if (j < len) out[j * K] = BWD ? sp.x[c][u] * (sp.y[c][u] - T) : exp_t(sp.x[c][u] - m) * r;
            }
    }
    if (SYNC && NW > 1) __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------ score backward
// The sum of term(m), m = 0 .. n-1 (n >= 0), on NW waves (1: a wave of the tile walk, four partials per lane; 4: the workgroup of a
// long segment, wave w holding the partials 64w .. 64w+63).  Either way lane l of accumulator / wave w holds P[64w + l], accumulated
// in ascending m, with four entries per lane in flight.  NW = 4: every thread of the block must call; `lds` (4 floats) is free for
// the next call on return.
template <int NW, typename Term>
__device__ __forceinline__ float segment_sum(Term term, int64_t n, int lane, int wave, float* lds) {
    constexpr int NA = 4 / NW;                             // accumulators per lane
    constexpr int kStride = NW == 1 ? kWave : kPartials;   // between the four entries of a lane in one iteration
    const int first = NW == 1 ? 0 : wave * kWave;          // (wave-uniform)
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
                const float v = term(ok ? m0 + lane : m0);
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
            if (u * kWave < n) W[u] = bfly64<Add>(acc[u < NA ? u : 0]);   // (wave-uniform; a wave of +0 sums to +0)
        }
        return (W[0] + W[1]) + (W[2] + W[3]);
    }
    const float Ww = bfly64<Add>(acc[0]);
    if (lane == 0) lds[wave] = Ww;
    __syncthreads();
    const float total = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return total;
}

// ------------------------------------------------------------------------------------------------------------ feature quads
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte accesses need only dword alignment on gfx950

struct Quad {
    float v[4];
};

// Columns c0 .. c0+3 of a feature row; columns >= d read as +0 and are never loaded.  TAIL = false: d is a multiple of 4 (and so
// is c0), a quad is whole or absent.
template <bool TAIL = true>
__device__ __forceinline__ Quad load_quad(const float* row, int c0, int d) {
    Quad r;
    r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0.f;
    if (TAIL ? c0 + 3 < d : c0 < d) {
        const float4u t = *reinterpret_cast<const float4u*>(row + c0);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else if (TAIL) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < d) r.v[k] = row[c0 + k];
    }
    return r;
}
__device__ __forceinline__ void store_quad(float* row, int c0, int d, const Quad& r) {
    if (c0 + 3 < d) {
        float4u t;
        t.x = r.v[0]; t.y = r.v[1]; t.z = r.v[2]; t.w = r.v[3];
        *reinterpret_cast<float4u*>(row + c0) = t;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < d) row[c0 + k] = r.v[k];
    }
}

// ---- bf16 feature quads (attention_bf16.hip).  A bf16 element is the upper half of an fp32: widening is exact (a shift or a mask),
// so every operation after it is the fp32 kernel's; an output is rounded ONCE, to nearest even, where it is stored.  d is even and
// every row starts on a dword (checked on the host), so a quad holds 4, 2 or 0 valid columns.
struct bf16_t {
    uint16_t bits;
};
typedef uint32_t uint2a __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte accesses need only dword alignment on gfx950

// Four bf16 as they were loaded: they stay packed until the FMA that consumes them.
struct PackedQuad {
    uint32_t lo, hi;
};
// What a gather of four columns of element type E keeps in registers.
template <typename E>
struct Gathered {
    using type = Quad;
};
template <>
struct Gathered<bf16_t> {
    using type = PackedQuad;
};

template <bool TAIL = true>
__device__ __forceinline__ Quad load_gathered(const float* row, int c0, int d) { return load_quad<TAIL>(row, c0, d); }
template <bool TAIL = true>
__device__ __forceinline__ PackedQuad load_gathered(const bf16_t* row, int c0, int d) {
    PackedQuad r;
    r.lo = r.hi = 0;
    if (TAIL ? c0 + 3 < d : c0 < d) {
        const uint2a t = *reinterpret_cast<const uint2a*>(row + c0);
        r.lo = t.x; r.hi = t.y;
    } else if (TAIL && c0 + 1 < d) {
        r.lo = *reinterpret_cast<const uint32_t*>(row + c0);
    }
    return r;
}
__device__ __forceinline__ const Quad& widen(const Quad& q) { return q; }
__device__ __forceinline__ Quad widen(const PackedQuad& w) {
    Quad r;
    r.v[0] = __uint_as_float(w.lo << 16); r.v[1] = __uint_as_float(w.lo & 0xffff0000u);
    r.v[2] = __uint_as_float(w.hi << 16); r.v[3] = __uint_as_float(w.hi & 0xffff0000u);
    return r;
}
template <bool TAIL = true>
__device__ __forceinline__ Quad load_quad(const bf16_t* row, int c0, int d) { return widen(load_gathered<TAIL>(row, c0, d)); }

// round to nearest even, two at a time: v_cvt_pk_bf16_f32 (torch's .to(torch.bfloat16), ties and overflow to inf included)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ void store_quad(bf16_t* row, int c0, int d, const Quad& r) {
    if (c0 + 3 < d) {
        uint2a t;
        t.x = pack_bf16x2(r.v[0], r.v[1]); t.y = pack_bf16x2(r.v[2], r.v[3]);
        *reinterpret_cast<uint2a*>(row + c0) = t;
    } else if (c0 + 1 < d) {
        *reinterpret_cast<uint32_t*>(row + c0) = pack_bf16x2(r.v[0], r.v[1]);
    }
}
// Columns c, c + 1 (c even, c + 1 < d) of a row: one dword for a bf16 row, so that no 2-byte store has a neighbour to race with.
__device__ __forceinline__ void store_pair(float* row, int c, float a, float b) { row[c] = a, row[c + 1] = b; }
__device__ __forceinline__ void store_pair(bf16_t* row, int c, float a, float b) {
    *reinterpret_cast<uint32_t*>(row + c) = pack_bf16x2(a, b);
}

// The quad value of the SDDMM's documented order: t = g0*x0, then fma(g1, x1, t), fma(g2, x2, t), fma(g3, x3, t).
__device__ __forceinline__ float dot_quad(const Quad& g, const Quad& x) {
    float t = g.v[0] * x.v[0];
    t = __builtin_fmaf(g.v[1], x.v[1], t);
    t = __builtin_fmaf(g.v[2], x.v[2], t);
    t = __builtin_fmaf(g.v[3], x.v[3], t);
    return t;
}

// ============================================================================================================ host
// The launch paths that edge_scores.hip / row_softmax.hip share with their head-batched forms in attention_heads.hip.  P: the unit's
// Params; HEADS: P has a head count K and the refusals speak of n_heads (the single-head entry points pass K = 1).  Every check comes
// before the device is touched.
template <typename P>
using Kernel = void (*)(const P);

template <typename P, bool HEADS, bool BWD>
int softmax_launch(Kernel<P> kernel, const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* a, const char* a_name,
                   const float* const* g, const char* g_name, float* const* out, const char* out_name, int32_t K, void* stream_v) {
    try {
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (K < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", K);
        if ((st = check_hop_arrays(v, a_name, a)) != H2GCN_OK) return st;
        if (BWD && (st = check_hop_arrays(v, g_name, g)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, out_name, out)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        P p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) {
            p.a[s] = a[s];
            p.g[s] = BWD ? g[s] : nullptr;
            p.out[s] = out[s];
        }
        if constexpr (HEADS) p.K = K;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in row_softmax%s_hops%s_f32", BWD ? "_backward" : "", HEADS ? "_heads" : "");
    }
}

// ld >= n_sel * K of one node operand of the edge scores, in the wording of the entry point.
template <bool HEADS>
int check_score_ld(const PatternView& v, int32_t K, const char* name, int64_t ld) {
    const int64_t need = (int64_t)v.n_sel * K;
    if (ld >= need) return H2GCN_OK;
    if (HEADS) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s = %lld < H_sel * n_heads = %lld", name, (long long)ld, (long long)need);
    return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s = %lld < H_sel = %d", name, (long long)ld, v.n_sel);
}

template <bool HEADS>
int check_node_operands(const PatternView& v, int32_t K, const float* l, int64_t ldl, const float* r, int64_t ldr) {
    int st;
    if ((st = check_score_ld<HEADS>(v, K, "ldl", ldl)) != H2GCN_OK) return st;
    if ((st = check_score_ld<HEADS>(v, K, "ldr", ldr)) != H2GCN_OK) return st;
    if (selected_nnz(v) > 0 && !l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "l is NULL");
    if (selected_nnz(v) > 0 && !r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "r is NULL");
    return H2GCN_OK;
}

template <typename P, bool HEADS>
void fill(P* p, const PatternView& v, const float* self, int64_t ld_self, const float* other, int64_t ld_other, int32_t K, float slope) {
    for (int s = 0; s < v.n_sel; ++s) p->idx[s] = v.colidx[s];
    p->self = self, p->ld_self = ld_self;
    p->other = other, p->ld_other = ld_other;
    if constexpr (HEADS) p->K = K;
    p->slope = slope;
}

template <typename P, bool HEADS>
int scores_forward(Kernel<P> kernel, const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr,
                   int32_t K, float slope, float* const* scores, void* stream_v) {
    try {
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (K < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", K);
        if ((st = check_node_operands<HEADS>(v, K, l, ldl, r, ldr)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, "scores", scores)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        P p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        fill<P, HEADS>(&p, v, l, ldl, r, ldr, K, slope);
        for (int s = 0; s < v.n_sel; ++s) p.score[s] = scores[s];
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_hops%s_f32", HEADS ? "_heads" : "");
    }
}

// One side of the score backward (T: the column side, on the adjoint operand), in two steps so that both sides' refusals come
// before either side's launch.
template <typename P, bool HEADS, bool T>
struct Side {
    P p;
    int64_t n_blocks = 0;
    int n_sel = 0, K = 1;
    int64_t n_rows = 0;

    int prepare(const h2gcn_plan_t* plan, const PatternView& v, const uint32_t* const* perm, const float* self, int64_t ld_self,
                const float* other, int64_t ld_other, int32_t n_heads, float slope, const float* const* g, float* out, int64_t ld_out,
                hipStream_t stream) {
        memset(&p, 0, sizeof(p));
        n_sel = v.n_sel, n_rows = v.n_rows, K = n_heads;
        const int st = launch_geometry(plan, v, stream, &p.geom, &n_blocks, T);
        p.out = out, p.ld_out = ld_out;
        if (st != H2GCN_OK || n_blocks == 0) return st;
        fill<P, HEADS>(&p, v, self, ld_self, other, ld_other, K, slope);
        for (int s = 0; s < v.n_sel; ++s) p.g[s] = g[s], p.perm[s] = T ? perm[s] : nullptr;
        return H2GCN_OK;
    }
    int run(Kernel<P> kernel, hipStream_t stream) {
        if (n_blocks == 0) {   // a selection without nonzeros: every segment is empty
            if (n_rows > 0)
                H2GCN_HIP_TRY(hipMemset2DAsync(p.out, (size_t)p.ld_out * sizeof(float), 0, (size_t)n_sel * K * sizeof(float), (size_t)n_rows,
                                               stream));
            return H2GCN_OK;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    }
};

template <typename P, bool HEADS>
int scores_backward(Kernel<P> row_kernel, Kernel<P> col_kernel, const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl,
                    const float* r, int64_t ldr, int32_t K, float slope, const float* const* g, float* dl, int64_t lddl, float* dr,
                    int64_t lddr, void* stream_v) {
    try {
        PatternView v, tv;
        const uint32_t* perm[H2GCN_MAX_HOPS] = {};
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (K < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", K);
        if (!dl && !dr) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dl and dr are both NULL: nothing to compute");
        if ((st = check_node_operands<HEADS>(v, K, l, ldl, r, ldr)) != H2GCN_OK) return st;
        if (dl && (st = check_score_ld<HEADS>(v, K, "lddl", lddl)) != H2GCN_OK) return st;
        if (dr && (st = check_score_ld<HEADS>(v, K, "lddr", lddr)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, "dscores", g)) != H2GCN_OK) return st;
        if (dr && (st = adjoint_view(plan, hop_mask, &tv, perm)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Side<P, HEADS, false> rows;
        Side<P, HEADS, true> cols;
        if (dl && (st = rows.prepare(plan, v, nullptr, l, ldl, r, ldr, K, slope, g, dl, lddl, stream)) != H2GCN_OK) return st;
        if (dr && (st = cols.prepare(plan, tv, perm, r, ldr, l, ldl, K, slope, g, dr, lddr, stream)) != H2GCN_OK) return st;
        if (dl && (st = rows.run(row_kernel, stream)) != H2GCN_OK) return st;
        if (dr && (st = cols.run(col_kernel, stream)) != H2GCN_OK) return st;
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_backward_hops%s_f32", HEADS ? "_heads" : "");
    }
}

}  // namespace pattern
}  // namespace h2gcn
