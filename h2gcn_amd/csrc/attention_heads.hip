// attention_heads.hip -- the head dimension of the attention chain: the SDDMM, the row softmax and the additive edge scores of
// sddmm.hip / row_softmax.hip / edge_scores.hip for K heads in ONE launch each, on ENTRY-MAJOR per-entry arrays: element
// (e, h) of a selected hop sits at e * K + h, the layout the hop SpMM on per-launch values reads fastest.
//
//     sddmm      dvals[s][e*K + h] = sum_{c in head h} dY[i, s, c] * X[j, c]            head h: columns h*w .. (h+1)*w - 1, w = d / K
//     softmax    one softmax per (row, hop, head) segment, forward and backward
//     scores     score[s][e*K + h] = leaky(l[i, s, h] + r[j, s, h]);  dl / dr the row / column sums of t per head
//
// A translation unit of its own: no existing kernel is compiled differently because of it.  Nothing is new in the arithmetic:
// per head every call gives the bits of its single-head counterpart on that head alone (include/h2gcn_hip.h), because every
// reduction below is the documented tree of that call, from the one copy in segment_ops.hip.h -- the lane that holds an element
// and the order of the additions are the same, only the address of element (e, h) differs.
//
// Mapping (gfx950, wave64; the pattern walk of pattern_walk.hip.h, no atomics, no scratch, no workspace):
//   * softmax / score backward: the wave that owns a segment loops over the heads INSIDE the segment, so the K passes read lines
//     that the first pass brought in, and colidx / perm / the node rows of an entry come from memory once.  Segments of at most
//     16 entries take FOUR heads per pass (lane group gi = head h0 + gi, lane q = entry q: the single-head call's 16-lane
//     group); segments of at most 64 entries also take four heads per pass -- lane = entry, the four heads of an entry in one
//     16-byte access, four independent one-register reductions; longer ones one head per pass on the whole wave (four partials
//     per lane), long segments on their workgroup;
//   * score forward (no reduction): one lane per entry writes its K contiguous scores from one gather of r[j, s, 0..K-1];
//   * sddmm, w in {4, 8, 16, 32} (PACKED): a 16-lane group keeps loading 64 contiguous columns = 64 / w whole heads of a
//     neighbour row; the xor butterfly stops below quad distance w / 4, so every head's w / 4 lanes hold that head's block
//     total.  One walk of the pattern and one full-width gather of each neighbour row serve all heads; a lane keeps the totals of
//     the rounds r = q (mod w / 4) and the 64 * K results of a chunk leave together into the chunk's contiguous 256 * K bytes;
//   * sddmm, any other w: head-aligned blocks -- block b of head h covers the columns h*w + 64b + 4q (masked to < w): the
//     single-head walk on the head's column slice.  The heads of a 64-entry chunk run back to back on column ids fetched once, so
//     a line that two heads share is still in cache; with w a multiple of 64 no line is shared at all.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "segment_ops.hip.h"

namespace h2gcn {
namespace heads {

using namespace pattern;

// ====================================================================================================== row softmax
namespace softmax {

struct Params {
    Geom geom;
    const float* a[H2GCN_MAX_HOPS];   // forward: scores; backward: alpha   ([nnz_k, K], the selected hops packed)
    const float* g[H2GCN_MAX_HOPS];   // backward: dalpha
    float* out[H2GCN_MAX_HOPS];       // forward: alpha; backward: dscores
    int K;
};

// A segment of at most 64 entries, up to FOUR heads per pass: lane `lane` holds entry `lane` of the heads h0 .. h0 + nh - 1 (one
// 16-byte access when nh == 4) and the wave runs the single-head call's one-register reduction once per head, the four of them
// independent of each other.  a / g / out at element (first entry, h0); nh in 1..4 is wave-uniform.
template <bool BWD>
__device__ __forceinline__ void seg64_heads(const float* a, const float* g, float* out, int len, int64_t K, int nh, int lane) {
    const bool ok = lane < len;
    const int64_t at = (int64_t)lane * K;
    const float pad = BWD ? 0.f : neg_inf();
    float x[4] = {pad, pad, pad, pad}, y[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (ok) {
        if (nh == 4) {
            const float4u t = *reinterpret_cast<const float4u*>(a + at);
            x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
            if (BWD) {
                const float4u u = *reinterpret_cast<const float4u*>(g + at);
                y[0] = u.x, y[1] = u.y, y[2] = u.z, y[3] = u.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < nh) {
                    x[k] = a[at + k];
                    if (BWD) y[k] = g[at + k];
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= nh) continue;   // (wave-uniform)
        if (!BWD) {
            float m = bfly64<Max>(x[k]);
            if (__ballot(x[k] != x[k]) != 0ull) m = quiet_nan();
            const float e = ok ? exp_t(x[k] - m) : 0.f;
            const float S = bfly64<Add>(e);   // = (W_0 + 0) + (0 + 0)
            o[k] = e * (1.0f / S);
        } else {
            const float D = bfly64<Add>(__builtin_fmaf(x[k], y[k], 0.f));
            o[k] = x[k] * (y[k] - D);
        }
    }
    if (ok) {
        if (nh == 4) {
            float4u t;
            t.x = o[0], t.y = o[1], t.z = o[2], t.w = o[3];
            *reinterpret_cast<float4u*>(out + at) = t;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < nh) out[at + k] = o[k];
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(kBlock) void row_softmax_heads_kernel(const Params p) {
    __shared__ float lds[8];   // long segments: wave maxima [0..3], wave totals [4..7]
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t K = p.K;
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        if (end <= beg) return;   // (the same for the whole block)
        for (int h = 0; h < p.K; ++h)
            loop_segment<BWD, kWavesPerBlock, true>(p.a[s] + beg * K + h, BWD ? p.g[s] + beg * K + h : nullptr, p.out[s] + beg * K + h,
                                                    end - beg, K, lane, wave, lds);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int rpw = p.geom.rows_per_wave;
    const int q = lane & (kGroup - 1), gi = lane >> 4;
    for (s = 0; s < p.geom.n_sel; ++s) {
        const float* a = p.a[s];
        const float* g = p.g[s];
        float* out = p.out[s];
        for (int i = 0; i < rpw && row0 + i < p.geom.n_rows; ++i) {
            segment(p.geom, rp, s, i, &beg, &end);
            const int64_t len = end - beg;
            if (len <= 0 || len >= p.geom.long_threshold) continue;
            if (len <= kGroup) {
                // four heads per pass: lane group gi is head h0 + gi, lane q entry q
                for (int h0 = 0; h0 < p.K; h0 += 4) {
                    const bool ok = q < len && h0 + gi < p.K;
                    const int64_t at = (beg + q) * K + h0 + gi;
                    const float x = ok ? a[at] : (BWD ? 0.f : neg_inf());
                    const float y = BWD && ok ? g[at] : 0.f;
                    seg16<BWD>(x, y, ok, out + at, lane);
                }
            } else if (len <= kWave) {
                for (int h0 = 0; h0 < p.K; h0 += 4)
                    seg64_heads<BWD>(a + beg * K + h0, BWD ? g + beg * K + h0 : nullptr, out + beg * K + h0, (int)len, K,
                                     p.K - h0 < 4 ? p.K - h0 : 4, lane);
            } else {
                for (int h = 0; h < p.K; ++h)
                    loop_segment<BWD, 1, true>(a + beg * K + h, BWD ? g + beg * K + h : nullptr, out + beg * K + h, len, K, lane, 0, nullptr);
            }
        }
    }
}

}  // namespace softmax

// ====================================================================================================== edge scores
namespace scores {

struct Params {
    Geom geom;                              // of the walked operand: A_k (forward, row side) or A_k^T (column side)
    const int32_t* idx[H2GCN_MAX_HOPS];     // its colidx: the OTHER node of every walked entry   (the selected hops, packed)
    const uint32_t* perm[H2GCN_MAX_HOPS];   // column side: the forward entry behind every walked entry
    const float* g[H2GCN_MAX_HOPS];         // backward: dscores [nnz_k, K], in forward entry order
    float* score[H2GCN_MAX_HOPS];           // forward: scores [nnz_k, K]
    const float* self;                      // the walked rows' operand: l (forward, row side) / r (column side) ...
    const float* other;                     // ... and the gathered one; element (node, s, h) at node * ld + s * K + h
    float* out;                             // backward: dl (row side) / dr (column side)
    int64_t ld_self, ld_other, ld_out;
    int K;
    float slope;
};


// The K scores of one entry: self / other / dst at head 0 of the entry's (row, s) / (column, s) / own element.
__device__ __forceinline__ void entry_scores(const float* self, const float* other, float* dst, int K, float slope) {
    int h = 0;
    for (; h + 4 <= K; h += 4) {
        const float4u a = *reinterpret_cast<const float4u*>(self + h), b = *reinterpret_cast<const float4u*>(other + h);
        float4u o;
        o.x = leaky(a.x + b.x, slope), o.y = leaky(a.y + b.y, slope), o.z = leaky(a.z + b.z, slope), o.w = leaky(a.w + b.w, slope);
        *reinterpret_cast<float4u*>(dst + h) = o;
    }
    for (; h < K; ++h) dst[h] = leaky(self[h] + other[h], slope);
}

__global__ __launch_bounds__(kBlock) void edge_scores_heads_kernel(const Params p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t K = p.K;
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        const float* self = p.self + row * p.ld_self + s * K;
        const int32_t* idx = p.idx[s];
        for (int64_t e = beg + threadIdx.x; e < end; e += kBlock)
            entry_scores(self, p.other + (int64_t)idx[e] * p.ld_other + s * K, p.score[s] + e * K, p.K, p.slope);
        return;
    }
    // the tile walk: the entries of a wave's rows in one hop are ONE contiguous range, streamed 64 entries at a time; every lane
    // finds the row of its entry by bisection among the wave's row pointers (as the single-head kernel does)
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int rpw = p.geom.rows_per_wave;
    int top = 1;
    while (2 * top < rpw) top *= 2;
    for (s = 0; s < p.geom.n_sel; ++s) {
        const int32_t* idx = p.idx[s];
        const int l0 = rp_lane(p.geom, s, 0);
        const int64_t first = readlane64(rp, l0), last = readlane64(rp, l0 + rpw);
        for (int64_t e0 = first; e0 < last; e0 += kWave) {   // (wave-uniform: bpermute needs every lane)
            const int64_t e = e0 + lane;
            int i = 0;
            for (int step = top; step > 0; step >>= 1) {
                const int c = i + step < rpw ? i + step : rpw;
                if (bpermute64(rp, l0 + c) <= e) i = c;
            }
            const int64_t lo = bpermute64(rp, l0 + i), hi = bpermute64(rp, l0 + (i < rpw ? i + 1 : rpw));   // the segment of e
            if (e < last && hi - lo < p.geom.long_threshold)   // (a long segment: a workgroup of its own)
                entry_scores(p.self + (row0 + i) * p.ld_self + s * K, p.other + (int64_t)idx[e] * p.ld_other + s * K,
                             p.score[s] + e * K, p.K, p.slope);
        }
    }
}

// t of walked entry e of selected hop s, head h.  T: the column side -- e is an entry of A_k^T, g sits at the forward entry perm[e].
template <bool T>
__device__ __forceinline__ float term(const Params& p, int s, int h, float self, int64_t e) {
    const int64_t o = p.idx[s][e];
    const float g = p.g[s][(T ? (int64_t)p.perm[s][e] : e) * p.K + h];
    const float oth = p.other[o * p.ld_other + (int64_t)s * p.K + h];
    const float pre = T ? oth + self : self + oth;   // l[i] + r[j]
    return pre > 0.f ? g : g * p.slope;
}

template <bool T>
__global__ __launch_bounds__(kBlock) void edge_scores_heads_backward_kernel(const Params p) {
    __shared__ float lds[kWavesPerBlock];   // long segments: the wave totals
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t K = p.K;
    if ((int)blockIdx.x < p.geom.n_long) {
        // a long segment (row side) / every selected hop of a long row (column side): 64-entry chunks over the 4 waves
        const int64_t e = p.geom.long_list[blockIdx.x];
        const int64_t row = T ? e : e >> 4;
        const int s0 = T ? 0 : (int)(e & 15), s1 = T ? p.geom.n_sel : s0 + 1;
        for (int s = s0; s < s1; ++s) {
            const int64_t beg = p.geom.rowptr[s][row], end = p.geom.rowptr[s][row + 1];
            for (int h = 0; h < p.K; ++h) {
                const float self = p.self[row * p.ld_self + s * K + h];
                const float total = segment_sum<kWavesPerBlock>([&](int64_t m) { return term<T>(p, s, h, self, beg + m); }, end - beg, lane,
                                                                wave, lds);
                if (threadIdx.x == 0) p.out[row * p.ld_out + s * K + h] = total;
            }
        }
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    const int rpw = p.geom.rows_per_wave;
    const int q = lane & (kGroup - 1), gi = lane >> 4;
    for (int s = 0; s < p.geom.n_sel; ++s)
        for (int i0 = 0; i0 < rpw; i0 += 4) {
            int64_t gbeg, gn;
            group_segment<T>(p.geom, s, i0, row0, rp, lane, &gbeg, &gn);
            if (__ballot(gn >= 0) == 0ull) continue;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t beg = readlane64(gbeg, k * kGroup), n = readlane64(gn, k * kGroup);
                if (n < 0) continue;   // (wave-uniform)
                const int64_t row = row0 + i0 + k;
                const float* self = p.self + row * p.ld_self + s * K;
                float* out = p.out + row * p.ld_out + s * K;
                if (n <= kGroup) {
                    // four heads per pass on the 16-lane groups: P[q] = +0 + t, the partials 16 .. 255 are +0
                    for (int h0 = 0; h0 < p.K; h0 += 4) {
                        const int h = h0 + gi;
                        float t = 0.f;
                        if (q < n && h < p.K) t = term<T>(p, s, h, self[h], beg + q);
                        const float total = bfly16<Add>(0.f + t);
                        if (q == 0 && h < p.K) out[h] = total;   // (an empty segment: +0)
                    }
                } else if (n <= kWave) {
                    // one entry per lane, up to four heads per pass from ONE gather of the entry's g and node row (16 bytes each
                    // when four heads remain); P[lane] = +0 + t, the partials 64 .. 255 are +0
                    const bool ok = lane < n;
                    const int64_t e = beg + (ok ? lane : 0);
                    const float* ge = p.g[s] + (T ? (int64_t)p.perm[s][e] : e) * K;
                    const float* oe = p.other + (int64_t)p.idx[s][e] * p.ld_other + s * K;
                    for (int h0 = 0; h0 < p.K; h0 += 4) {
                        const int nh = p.K - h0 < 4 ? p.K - h0 : 4;   // (wave-uniform)
                        float gv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
                        if (nh == 4) {
                            const float4u a = *reinterpret_cast<const float4u*>(ge + h0), b = *reinterpret_cast<const float4u*>(oe + h0);
                            gv[0] = a.x, gv[1] = a.y, gv[2] = a.z, gv[3] = a.w;
                            ov[0] = b.x, ov[1] = b.y, ov[2] = b.z, ov[3] = b.w;
                        } else {
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                if (k < nh) gv[k] = ge[h0 + k], ov[k] = oe[h0 + k];
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (k >= nh) continue;   // (wave-uniform)
                            const float sf = self[h0 + k];
                            const float pre = T ? ov[k] + sf : sf + ov[k];   // l[i] + r[j]
                            const float t = ok ? (pre > 0.f ? gv[k] : gv[k] * p.slope) : 0.f;
                            const float total = bfly64<Add>(0.f + t);
                            if (lane == 0) out[h0 + k] = total;
                        }
                    }
                } else {
                    for (int h = 0; h < p.K; ++h) {
                        const float sf = self[h];
                        const float total = segment_sum<1>([&](int64_t m) { return term<T>(p, s, h, sf, beg + m); }, n, lane, 0, nullptr);
                        if (lane == 0) out[h] = total;
                    }
                }
            }
        }
}

// the row side and the column side (named here, ahead of the SDDMM's kernels: the code object keeps its kernels in this order)
constexpr Kernel<Params> kBackward[2] = {edge_scores_heads_backward_kernel<false>, edge_scores_heads_backward_kernel<true>};

}  // namespace scores

// ====================================================================================================== sddmm
namespace sddmm {

constexpr int kBlockCols = 64;   // columns one lane group covers per load: 16 lanes x 4

struct Params {
    Geom geom;
    const int32_t* colidx[H2GCN_MAX_HOPS];   // the selected hops, packed as geom.rowptr
    float* dvals[H2GCN_MAX_HOPS];            // [nnz_k, K]
    int d, K, w;                             // w = d / K
    const float* g;                          // dY, [n_rows, n_sel, d] through ldg_row / ldg_hop (elements)
    int64_t ldg_row, ldg_hop;
    const float* x;                          // X, [n_cols, d] through ldx
    int64_t ldx;
};

// The first steps of bfly16 over the L = w / 4 lanes of one head (an aligned run of L lanes): afterwards they all hold the sum
// of the head's quads in the single-head call's order.  Its remaining steps would add quads of +0: v + (+0) changes no bit but
// -0 -> +0, and the element's `+0 + B` does that anyway.
template <int L>
__device__ __forceinline__ float bfly_head(float v) {
    if (L >= 2) v = v + dpp<0xB1>(v);    // lane ^ 1
    if (L >= 4) v = v + dpp<0x4E>(v);    // lane ^ 2
    if (L >= 8) v = v + dpp<0x141>(v);   // row_half_mirror: lane ^ 4 up to a permutation of equals
    return v;
}

// ---- PACKED, w = 4 L in {4, 8, 16, 32}: `count` (1..64) consecutive entries of one segment, all heads.  A column pass covers
// NB blocks of 64 columns = NB * 16 / L heads; a lane keeps the totals of the rounds r = q (mod L): NB * 16 / L registers.
template <int L, int NB, int U>
__device__ __forceinline__ void walk_chunk_packed(const Params& p, const float* grow, const int32_t* cols, int count, float* out, int lane) {
    constexpr int kKeep = 16 / L;   // totals a lane keeps per block; also the heads of a block
    const int q = lane & 15, gi = lane >> 4;
    const int my_n = q * 4 + gi;
    const int mycol = cols[my_n < count ? my_n : count - 1];
    const int rounds = (count + 3) >> 2;
    for (int cbase = 0; cbase < p.d; cbase += NB * kBlockCols) {
        Quad g[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = load_quad<false>(grow, cbase + b * kBlockCols + 4 * q, p.d);
        float res[NB][kKeep];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kKeep; ++k) res[b][k] = 0.f;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += U) {
            if (r0 < rounds) {   // (wave-uniform) a batch: its gathers go out before the first multiply
                Quad xv[U][NB];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (r0 + u < rounds) {
                        const int c = __builtin_amdgcn_ds_bpermute(((lane & 48) + r0 + u) << 2, mycol);
                        const float* xrow = p.x + (int64_t)c * p.ldx;
#pragma unroll
                        for (int b = 0; b < NB; ++b) xv[u][b] = load_quad<false>(xrow, cbase + b * kBlockCols + 4 * q, p.d);
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (r0 + u < rounds) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const float t = bfly_head<L>(dot_quad(g[b], xv[u][b]));
                            if ((q & (L - 1)) == ((r0 + u) & (L - 1))) res[b][(r0 + u) / L] = 0.f + t;   // element = +0 + B_0
                        }
                    }
            }
        }
        // lane (gi, q) holds, per block b and k, head cbase / w + b * kKeep + q / L of entry 4 (k L + q mod L) + gi
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kKeep; ++k) {
                const int n = 4 * (k * L + (q & (L - 1))) + gi;
                const int h = cbase / (4 * L) + b * kKeep + q / L;
                if (n < count && h < p.K) out[(int64_t)n * p.K + h] = res[b][k];
            }
    }
}

// ---- head-aligned blocks, any w that is a multiple of 4: the single-head walk on head h's column slice (grow / x at the head's
// first column), the chunk's column ids in `mycol`.  Lane q == r keeps entry 4r + gi.
template <int NB, int U>
__device__ __forceinline__ float walk_chunk_head(const Params& p, const float* grow, const float* x, int mycol, int rounds, int lane) {
    const int q = lane & 15;
    float res = 0.f;
    for (int cbase = 0; cbase < p.w; cbase += NB * kBlockCols) {
        Quad g[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = load_quad<false>(grow, cbase + b * kBlockCols + 4 * q, p.w);
        for (int r0 = 0; r0 < rounds; r0 += U) {
            Quad xv[U][NB];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r0 + u < rounds) {
                    const int c = __builtin_amdgcn_ds_bpermute(((lane & 48) + r0 + u) << 2, mycol);
                    const float* xrow = x + (int64_t)c * p.ldx;
#pragma unroll
                    for (int b = 0; b < NB; ++b) xv[u][b] = load_quad<false>(xrow, cbase + b * kBlockCols + 4 * q, p.w);
                }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r0 + u < rounds) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float t = bfly16<Add>(dot_quad(g[b], xv[u][b]));
                        if (q == r0 + u) res = res + t;   // block totals in ascending block order, starting from +0
                    }
                }
        }
    }
    return res;
}

// L > 0: packed with w = 4 L; L == 0: head-aligned blocks.
template <int L, int NB>
__device__ __forceinline__ void walk_chunk(const Params& p, const float* grow, const int32_t* cols, int count, float* out, int lane) {
    constexpr int U = 8 / NB;   // rounds per batch: 8 load instructions (8 KiB per wave) in flight
    if constexpr (L > 0) {
        walk_chunk_packed<L, NB, U>(p, grow, cols, count, out, lane);
    } else {
        const int q = lane & 15, gi = lane >> 4;
        const int my_n = q * 4 + gi;
        const int mycol = cols[my_n < count ? my_n : count - 1];
        const int rounds = (count + 3) >> 2;
        for (int h = 0; h < p.K; ++h) {
            const float res = walk_chunk_head<NB, U>(p, grow + h * p.w, p.x + h * p.w, mycol, rounds, lane);
            if (my_n < count) out[(int64_t)my_n * p.K + h] = res;
        }
    }
}

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void sddmm_heads_kernel(const Params p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        const float* grow = p.g + row * p.ldg_row + (int64_t)s * p.ldg_hop;
        for (int64_t c = beg + (int64_t)wave * kWave; c < end; c += kBlock) {
            const int count = (int)(end - c < kWave ? end - c : kWave);
            walk_chunk<L, NB>(p, grow, p.colidx[s] + c, count, p.dvals[s] + c * p.K, lane);
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            const int64_t len = end - beg;
            if (len <= 0 || len >= p.geom.long_threshold) continue;
            const float* grow = p.g + (row0 + i) * p.ldg_row + (int64_t)s * p.ldg_hop;
            for (int64_t c = beg; c < end; c += kWave) {
                const int count = (int)(end - c < kWave ? end - c : kWave);
                walk_chunk<L, NB>(p, grow, p.colidx[s] + c, count, p.dvals[s] + c * p.K, lane);
            }
        }
    }
}

int launch(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY, int64_t ldg_row, int64_t ldg_hop, const float* X, int64_t ldx,
           int32_t d, int32_t n_heads, float* const* dvals, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
        if (n_heads < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", n_heads);
        if (d % n_heads) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d is not a multiple of n_heads = %d", d, n_heads);
        const int w = d / n_heads;
        if (n_heads > 1 && (w & 3))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "with n_heads = %d > 1 the head width d / n_heads = %d must be a multiple of 4", n_heads, w);
        // one head: the single-head call itself ([nnz_k, 1] is [nnz_k]); it repeats the remaining checks
        if (n_heads == 1) return h2gcn_sddmm_hops_f32(plan, hop_mask, dY, ldg_row, ldg_hop, X, ldx, d, dvals, stream_v);
        if (ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ldx, d);
        if (ldg_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_row = %lld < d = %d", (long long)ldg_row, d);
        if (ldg_hop < 0 || (v.n_sel > 1 && ldg_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_hop = %lld < d = %d: the hops' gradients would overlap", (long long)ldg_hop, d);
        if (selected_nnz(v) > 0 && !dY) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dY is NULL");
        if (selected_nnz(v) > 0 && !X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "X is NULL");
        if ((st = check_hop_arrays(v, "dvals", dvals)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) {
            p.colidx[s] = v.colidx[s];
            p.dvals[s] = dvals[s];
        }
        p.d = d, p.K = n_heads, p.w = w;
        p.g = dY, p.ldg_row = ldg_row, p.ldg_hop = ldg_hop;
        p.x = X, p.ldx = ldx;
        const dim3 grid((unsigned)n_blocks), block(kBlock);
        // (the bits do not depend on the geometry: the order of summation is a function of w alone)
        if (w == 4) hipLaunchKernelGGL((sddmm_heads_kernel<1, 1>), grid, block, 0, stream, p);
        else if (w == 8) hipLaunchKernelGGL((sddmm_heads_kernel<2, 2>), grid, block, 0, stream, p);
        else if (w == 16) hipLaunchKernelGGL((sddmm_heads_kernel<4, 2>), grid, block, 0, stream, p);
        else if (w == 32) hipLaunchKernelGGL((sddmm_heads_kernel<8, 2>), grid, block, 0, stream, p);
        else if (w <= kBlockCols) hipLaunchKernelGGL((sddmm_heads_kernel<0, 1>), grid, block, 0, stream, p);
        else if (w <= 2 * kBlockCols) hipLaunchKernelGGL((sddmm_heads_kernel<0, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((sddmm_heads_kernel<0, 4>), grid, block, 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in sddmm_hops_heads_f32");
    }
}

}  // namespace sddmm
}  // namespace heads
}  // namespace h2gcn


extern "C" {

int h2gcn_sddmm_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY_dev, int64_t ldg_row, int64_t ldg_hop,
                               const float* X_dev, int64_t ldx, int32_t d, int32_t n_heads, float* const* dvals_dev, void* stream) {
    return h2gcn::heads::sddmm::launch(plan, hop_mask, dY_dev, ldg_row, ldg_hop, X_dev, ldx, d, n_heads, dvals_dev, stream);
}

int h2gcn_row_softmax_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* scores_dev,
                                     float* const* alpha_dev, int32_t n_heads, void* stream) {
    using namespace h2gcn::heads;
    return softmax_launch<softmax::Params, true, false>(softmax::row_softmax_heads_kernel<false>, plan, hop_mask, scores_dev, "scores", nullptr, "",
                                                        alpha_dev, "alpha", n_heads, stream);
}

int h2gcn_row_softmax_backward_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* alpha_dev,
                                              const float* const* dalpha_dev, float* const* dscores_dev, int32_t n_heads, void* stream) {
    using namespace h2gcn::heads;
    return softmax_launch<softmax::Params, true, true>(softmax::row_softmax_heads_kernel<true>, plan, hop_mask, alpha_dev, "alpha", dalpha_dev,
                                                       "dalpha", dscores_dev, "dscores", n_heads, stream);
}

int h2gcn_edge_scores_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                     int64_t ldr, int32_t n_heads, float negative_slope, float* const* scores_dev, void* stream) {
    using namespace h2gcn::heads;
    return scores_forward<scores::Params, true>(scores::edge_scores_heads_kernel, plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope,
                                                scores_dev, stream);
}

int h2gcn_edge_scores_backward_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                              const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope,
                                              const float* const* dscores_dev, float* dl_dev, int64_t lddl, float* dr_dev,
                                              int64_t lddr, void* stream) {
    using namespace h2gcn::heads;
    return scores_backward<scores::Params, true>(scores::kBackward[0], scores::kBackward[1], plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, dscores_dev, dl_dev, lddl, dr_dev,
                                                 lddr, stream);
}

}  // extern "C"
