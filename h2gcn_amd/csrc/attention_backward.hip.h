// attention_backward.hip.h -- the device functions of the recomputing attention backward (attention_backward.hip has the description
// of the two sides), shared with attention_dropout.hip, whose kernels run the same passes with a dropout factor per (entry, head).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "segment_ops.hip.h"

// Every product and sum below is the operation written: the one-wave and the four-wave form of a segment are two instantiations of
// the same source and must give the same bits, so the compiler may not fuse `dscore * slope` into the partial's addition in one of
// them and not in the other.  The fused multiply-adds of the documented orders are written out (__builtin_fmaf).
#pragma clang fp contract(off)

namespace h2gcn {
namespace attention_backward {

using namespace pattern;
constexpr int kBlockCols = 64;   // columns one lane group covers per load: 16 lanes x 4
constexpr int kMaxBlocks = 4;    // 64-column blocks per row: d <= 256
constexpr int kMaxHeads = 16;    // the tiles are 64 x kMaxHeads floats per wave
constexpr int kSets = 4;         // chunk t of a segment belongs to set t mod 4

// E: the element type of the wide inputs x, y, g; TD: of dx (float, or bf16_t: attention_bf16.hip).  l, r, stats, delta, dl and dr
// are fp32 whatever they are.
template <typename E = float, typename TD = E>
struct ParamsT {
    Geom geom;                             // of the walked operand: A_s (row side) or A_s^T (column side)
    const int32_t* idx[H2GCN_MAX_HOPS];    // its colidx: the OTHER node of every walked entry (the selected hops, packed)
    const float *l, *r;
    const E* x;
    const float* stats;
    const E *y, *g;
    float *delta, *dl, *dr;
    TD* dx;
    int64_t ldl, ldr, ldx, ldstats, ldy_row, ldy_hop, ldg_row, ldg_hop, lddelta, lddl, lddr, lddx;
    int d, K, w;                           // w = d / K
    float slope;
};
using Params = ParamsT<>;

// COL: the column side (the row side has no alpha tile and no dx totals).
template <int NB, bool COL>
struct Shared {
    float dtile[kWavesPerBlock][kWave * kMaxHeads];   // per wave: dalpha of the chunk at hand, element (n, h) at n * K + h
    float atile[kWavesPerBlock][COL ? kWave * kMaxHeads : 1];   // column side: alpha of the chunk at hand
    float delta[kWavesPerBlock][kMaxHeads];           // row side: delta of the segment at hand
    float w[kWavesPerBlock][kSets][kMaxHeads];        // the set totals W_u of every head (long path: [0][wave])
    float tot[kWavesPerBlock][COL ? NB * kBlockCols : 1];   // column side, long path: the set totals T_u of dx
};

// What one lane writes into LDS another lane of the same wave reads next: a wave's LDS operations complete in order, the fence
// keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The first steps of bfly16 over the L = w / 4 lanes of one head (an aligned run of L lanes): the sum of the head's quads in the
// order of the SDDMM on the head's column slice (its remaining steps would add quads of +0).
template <int L>
__device__ __forceinline__ float bfly_head(float v) {
    if (L >= 2) v = v + dpp<0xB1>(v);    // lane ^ 1
    if (L >= 4) v = v + dpp<0x4E>(v);    // lane ^ 2
    if (L >= 8) v = v + dpp<0x141>(v);   // row_half_mirror: lane ^ 4 up to a permutation of equals
    return v;
}

// sum over the lanes {l, l^16}, then {l, l^32}: (P[gi] + P[gi^1]) + (P[gi^2] + P[gi^3])
__device__ __forceinline__ float fold_groups(float v) {
    v = v + __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

template <int NB>
__device__ __forceinline__ void clear(Quad (&acc)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[b].v[k] = 0.f;
}

// The held row of the packed geometry: columns 64 b + 4 q .. of `row`.
template <int NB, typename P, typename E>
__device__ __forceinline__ void load_row(const P& p, const E* row, int q, Quad (&a)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = load_quad<false>(row, b * kBlockCols + 4 * q, p.d);
}

// The per-head dot products of the held row (`a`: packed; `arow`: its address) with ONE other row `brow`, the same on every lane
// group: head h to dst[h].  The order is the SDDMM's on the head's column slice.  All 64 lanes must be active.
template <int L, int NB, typename P, typename E>
__device__ __forceinline__ void row_dots(const P& p, const Quad (&a)[NB], const E* arow, const E* brow, int lane, float* dst) {
    const int q = lane & 15, gi = lane >> 4;
    if constexpr (L > 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float t = bfly_head<L>(dot_quad(a[b], load_quad<false>(brow, b * kBlockCols + 4 * q, p.d)));
            const int hd = b * (16 / L) + q / L;
            if (gi == 0 && (q & (L - 1)) == 0 && hd < p.K) dst[hd] = 0.f + t;
        }
    } else {
        for (int h = 0; h < p.K; ++h) {
            float res = 0.f;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c0 = b * kBlockCols + 4 * q;
                res = res + bfly16<Add>(dot_quad(load_quad(arow + h * p.w, c0, p.w), load_quad(brow + h * p.w, c0, p.w)));
            }
            if (lane == 0) dst[h] = res;
        }
    }
}

// `count` (1..64) consecutive walked entries, their other nodes in `ecol` of lane n (clamped): dalpha of entry n, head h, to
// dtile[n * K + h] -- the held row (`a` / `arow`) against row ecol[n] of `src` (ld_src apart).  COL: the same loads also go into
// the dx accumulators, entry n into the partial of lane group n & 3 with one fmaf on atile[n * K + head].  All lanes active.
template <int L, int NB, bool COL, typename P, typename E>
__device__ __forceinline__ void chunk_dots(const P& p, const Quad (&a)[NB], const E* arow, const E* src, int64_t ld_src, int ecol,
                                           int count, int lane, float* dtile, const float* atile, const int (&head)[NB], Quad (&accx)[NB]) {
    // rounds per batch: 8 load instructions (8 KiB per wave) in flight; 16 of a bf16 row, 8 KiB again
    constexpr int U = (sizeof(E) == 2 ? 16 : 8) / NB;
    using XV = typename Gathered<E>::type;   // (bf16: packed until the operation that consumes it)
    const int q = lane & 15, gi = lane >> 4;
    const int rounds = (count + 3) >> 2;
    if constexpr (L > 0 || COL) {
        for (int r0 = 0; r0 < rounds; r0 += U) {   // (wave-uniform)
            XV xv[U][NB];
            float av[U][NB];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r0 + u < rounds) {
                    const int n = 4 * (r0 + u) + gi < count ? 4 * (r0 + u) + gi : count - 1;
                    const int c = __builtin_amdgcn_ds_bpermute(n << 2, ecol);
                    const E* row = src + (int64_t)c * ld_src;
                    if (COL) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) av[u][b] = atile[n * p.K + head[b]];
                    }
#pragma unroll
                    for (int b = 0; b < NB; ++b) xv[u][b] = load_gathered<(L == 0)>(row, b * kBlockCols + 4 * q, p.d);
                }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r0 + u < rounds) {
                    const int n = 4 * (r0 + u) + gi;
                    if constexpr (L > 0) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const float t = bfly_head<L>(dot_quad(a[b], widen(xv[u][b])));
                            const int hd = b * (16 / L) + q / L;
                            if (n < count && (q & (L - 1)) == 0 && hd < p.K) dtile[n * p.K + hd] = 0.f + t;   // element = +0 + B_0
                        }
                    }
                    if (COL && n < count) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const Quad& xq = widen(xv[u][b]);
#pragma unroll
                            for (int k = 0; k < 4; ++k) accx[b].v[k] = __builtin_fmaf(av[u][b], xq.v[k], accx[b].v[k]);
                        }
                    }
                }
        }
    }
    if constexpr (L == 0) {
        // head-aligned blocks: the single-head SDDMM walk on the column slice of head h
        for (int h = 0; h < p.K; ++h) {
            Quad ah[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) ah[b] = load_quad(arow + h * p.w, b * kBlockCols + 4 * q, p.w);
            for (int r0 = 0; r0 < rounds; r0 += U) {
                XV xv[U][NB];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (r0 + u < rounds) {
                        const int n = 4 * (r0 + u) + gi < count ? 4 * (r0 + u) + gi : count - 1;
                        const int c = __builtin_amdgcn_ds_bpermute(n << 2, ecol);
                        const E* row = src + (int64_t)c * ld_src + h * p.w;
#pragma unroll
                        for (int b = 0; b < NB; ++b) xv[u][b] = load_gathered(row, b * kBlockCols + 4 * q, p.w);
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (r0 + u < rounds) {
                        const int n = 4 * (r0 + u) + gi;
                        float res = 0.f;
#pragma unroll
                        for (int b = 0; b < NB; ++b) res = res + bfly16<Add>(dot_quad(ah[b], widen(xv[u][b])));   // block totals, ascending
                        if (n < count && q == 0) dtile[n * p.K + h] = res;
                    }
            }
        }
    }
}

// alpha of (entry, head): the forward's own operations on the stored statistics.
__device__ __forceinline__ float alpha_of(float pre, float slope, float m, float rinv) { return exp_t(leaky(pre, slope) - m) * rinv; }

// The set totals of one segment to its (W_0 + W_1) + (W_2 + W_3): `w` holds W_u of head h at w[u][h] (a set without a chunk: +0).
__device__ __forceinline__ float combine_sets(const float (*w)[kMaxHeads], int h) { return (w[0][h] + w[1][h]) + (w[2][h] + w[3][h]); }

// ---- host: the launch path both entry points share (attention_backward.hip).  `pair` NULL: the kernels of attention_backward.hip;
// else the caller's kernels of the geometry (L, NB) the path chose, with the forward view of the selection and `ctx` handed through.
using PairLauncher = void (*)(int L, int NB, const Params* rows, int64_t row_blocks, const Params* cols, int64_t col_blocks,
                              const PatternView& v, const void* ctx, hipStream_t stream);
int run(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr, int32_t K, float slope,
        const float* X, int64_t ldx, int32_t d, const float* stats, int64_t ldstats, const float* Y, int64_t ldy_row, int64_t ldy_hop,
        const float* G, int64_t ldg_row, int64_t ldg_hop, float* delta, int64_t lddelta, float* dl, int64_t lddl, float* dr, int64_t lddr,
        float* dX, int64_t lddx, void* stream_v, PairLauncher pair = nullptr, const void* ctx = nullptr);

}  // namespace attention_backward
}  // namespace h2gcn
