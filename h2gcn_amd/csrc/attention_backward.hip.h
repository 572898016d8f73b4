// attention_backward.hip.h -- the recomputing attention backward (attention_backward.hip has the description of the two sides): its
// device functions, the ONE row_segment and the ONE col_row that the kernels of attention_backward.hip, attention_dropout_backward.hip
// (a dropout factor per (entry, head)) and attention_bf16.hip (bf16 x, y, g) wrap, and the one host launch path behind their entry
// points.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

#include "attention_dropout.hip.h"
#include "segment_ops.hip.h"

// Every product and sum below is the operation written: the one-wave and the four-wave form of a segment are two instantiations of
// the same source and must give the same bits, so the compiler may not fuse `dscore * slope` into the partial's addition in one of
// them and not in the other.  The fused multiply-adds of the documented orders are written out (__builtin_fmaf).  Every function of
// this header that does fp32 arithmetic opens with the pragma below, so its scope is that function's body, whatever a unit includes
// or defines before or after this header.
#define H2GCN_NO_FP_CONTRACT _Pragma("clang fp contract(off)")

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
    using X = E;
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
    H2GCN_NO_FP_CONTRACT
    if (L >= 2) v = v + dpp<0xB1>(v);    // lane ^ 1
    if (L >= 4) v = v + dpp<0x4E>(v);    // lane ^ 2
    if (L >= 8) v = v + dpp<0x141>(v);   // row_half_mirror: lane ^ 4 up to a permutation of equals
    return v;
}

// sum over the lanes {l, l^16}, then {l, l^32}: (P[gi] + P[gi^1]) + (P[gi^2] + P[gi^3])
__device__ __forceinline__ float fold_groups(float v) {
    H2GCN_NO_FP_CONTRACT
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
    H2GCN_NO_FP_CONTRACT
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
    H2GCN_NO_FP_CONTRACT
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
__device__ __forceinline__ float alpha_of(float pre, float slope, float m, float rinv) {
    H2GCN_NO_FP_CONTRACT
    return exp_t(leaky(pre, slope) - m) * rinv;
}

// The set totals of one segment to its (W_0 + W_1) + (W_2 + W_3): `w` holds W_u of head h at w[u][h] (a set without a chunk: +0).
__device__ __forceinline__ float combine_sets(const float (*w)[kMaxHeads], int h) {
    H2GCN_NO_FP_CONTRACT
    return (w[0][h] + w[1][h]) + (w[2][h] + w[3][h]);
}

// ---- the two sides.  P: the parameter struct (its X the element type of x, y and g); D: the dropout policy -- NoDropout, or
// attention_dropout_backward.hip's: `kept(i, j, s, K)`, the kept heads of the entry (row i, column j) of the forward operand of
// selected hop s as a bit mask, `factor(keep, h)`, f in {0, 1/keep} of head h, and `undropped`, the column side's third tile.
struct NoDropout {
    static constexpr bool kOn = false;
};

// ---------------------------------------------------------------------------------------------------------------- row side
// Segment (row, s) = entries [beg, beg + len) on NW waves (1: the calling wave, the sets in turn; 4: every thread of the block must
// call, wave w = set w).  Stores delta[row, s, :] -- <g, y> on the y the forward stored -- and, if wanted, dl[row, s, :].
template <int L, int NB, int NW, typename P, typename D>
__device__ __forceinline__ void row_segment(const P& p, const D& dp, Shared<NB, false>& sh, int64_t row, int s, int64_t beg, int64_t len,
                                            int lane, int wave) {
    H2GCN_NO_FP_CONTRACT
    const int q = lane & 15;
    const typename P::X* grow = p.g + row * p.ldg_row + (int64_t)s * p.ldg_hop;
    const float* lrow = p.l + row * p.ldl + (int64_t)s * p.K;
    const float* st = p.stats + row * p.ldstats + (int64_t)s * 2 * p.K;
    float* dtile = sh.dtile[wave];
    float* delta = sh.delta[wave];
    float (*wtot)[kMaxHeads] = sh.w[NW == 1 ? wave : 0];
    Quad a[NB];
    int head[NB] = {};
    load_row(p, grow, q, a);
    wave_lds_sync();   // the previous segment's reads of delta and of the set totals come first
    row_dots<L, NB>(p, a, grow, p.y + row * p.ldy_row + (int64_t)s * p.ldy_hop, lane, delta);
    wave_lds_sync();
    if (p.delta && (NW == 1 || wave == 0) && lane < p.K) p.delta[row * p.lddelta + (int64_t)s * p.K + lane] = delta[lane];
    if (!p.dl) return;   // (the same for the whole grid)
    if (NW == 1) (&wtot[0][0])[lane] = 0.f;   // a set without a chunk: +0
    const int32_t* cols = p.idx[s] + beg;
    const float* rbase = p.r + (int64_t)s * p.K;
    for (int u = (NW == 1 ? 0 : wave); u < (NW == 1 ? kSets : wave + 1); ++u) {
        if (NW == 1 && (int64_t)u * kWave >= len) break;   // (wave-uniform)
        float acc[kMaxHeads];
#pragma unroll
        for (int h = 0; h < kMaxHeads; ++h) acc[h] = 0.f;
        for (int64_t c = (int64_t)u * kWave; c < len; c += kSets * kWave) {   // (wave-uniform)
            const int count = (int)(len - c < kWave ? len - c : kWave);
            const bool ok = lane < count;
            const int ecol = cols[c + (ok ? lane : count - 1)];
            wave_lds_sync();   // the previous chunk's reads of the tile come first
            chunk_dots<L, NB, false>(p, a, grow, p.x, p.ldx, ecol, count, lane, dtile, nullptr, head, a);
            wave_lds_sync();
            const float* rrow = rbase + (int64_t)ecol * p.ldr;
            uint32_t keep = 0;
            if constexpr (D::kOn) keep = dp.kept(row, ecol, s, p.K);
#pragma unroll
            for (int h = 0; h < kMaxHeads; ++h) {
                if (h >= p.K) continue;   // (wave-uniform)
                const float pre = lrow[h] + rrow[h];
                float dalpha = dtile[lane * p.K + h];
                if constexpr (D::kOn) dalpha = dp.factor(keep, h) * dalpha;   // dalpha = f * dot
                const float ds = alpha_of(pre, p.slope, st[h], st[p.K + h]) * (dalpha - delta[h]);
                const float dpre = pre > 0.f ? ds : ds * p.slope;
                acc[h] = acc[h] + (ok ? dpre : 0.f);   // P[64 u + lane], ascending position
            }
        }
#pragma unroll
        for (int h = 0; h < kMaxHeads; ++h) {
            if (h >= p.K) continue;   // (wave-uniform)
            const float W = bfly64<Add>(acc[h]);
            if (lane == 0) wtot[u][h] = W;
        }
    }
    if (NW == 1) wave_lds_sync();
    else __syncthreads();
    if ((NW == 1 || wave == 0) && lane < p.K) p.dl[row * p.lddl + (int64_t)s * p.K + lane] = combine_sets(wtot, lane);
    if (NW > 1) __syncthreads();
}

// The body of a row-side kernel.
template <int L, int NB, typename P, typename D>
__device__ __forceinline__ void rows_walk(const P& p, const D& dp, Shared<NB, false>& sh) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        row_segment<L, NB, kWavesPerBlock>(p, dp, sh, row, s, beg, end - beg, lane, wave);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i)
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            if (end - beg >= p.geom.long_threshold) continue;   // a workgroup of its own
            row_segment<L, NB, 1>(p, dp, sh, row0 + i, s, beg, end - beg, lane, wave);
        }
}

// ------------------------------------------------------------------------------------------------------------- column side
// Column j of the forward operands = row j of every selected A_s^T, on NW waves (as row_segment).  Stores dr[j, :, :] and, as TD,
// dx[j, :] -- rounded once, after the sum over the hops -- where wanted.  Under dropout the coefficient the dx fmafs read is alpha * f,
// as the forward forms it, and dscore uses the undropped alpha, kept per chunk in dp.undropped (lane = entry writes and reads its own
// row of it).
template <typename TD, int L, int NB, int NW, typename P, typename D>
__device__ __forceinline__ void col_row(const P& p, const D& dp, Shared<NB, true>& sh, int64_t j, int lane, int wave) {
    H2GCN_NO_FP_CONTRACT
    // the long path's epilogue keeps one column per thread; with a bf16 operand one PAIR (d is then even: a bf16 pair is one dword)
    constexpr int CW = std::is_same<TD, float>::value && std::is_same<typename P::X, float>::value ? 1 : 2;
    const int q = lane & 15, gi = lane >> 4;
    const typename P::X* xrow = p.x + j * p.ldx;
    float* dtile = sh.dtile[wave];
    float* atile = sh.atile[wave];
    const float* utile = atile;   // alpha for dscore
    if constexpr (D::kOn) utile = dp.undropped;
    float (*wtot)[kMaxHeads] = sh.w[NW == 1 ? wave : 0];
    Quad a[NB], accx[NB];
    int head[NB];
    load_row(p, xrow, q, a);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int h = (b * kBlockCols + 4 * q) / p.w;
        head[b] = h < p.K ? h : p.K - 1;   // (a quad beyond d: its sums are never stored)
    }
    Quad dxq;          // NW == 1: the running hop sum of the quad this lane stores
    float dxc[CW];     // NW == 4: the running hop sums of the columns CW threadIdx.x ..
#pragma unroll
    for (int k = 0; k < 4; ++k) dxq.v[k] = 0.f;
#pragma unroll
    for (int k = 0; k < CW; ++k) dxc[k] = 0.f;
    for (int s = 0; s < p.geom.n_sel; ++s) {
        const int64_t beg = p.geom.rowptr[s][j], len = p.geom.rowptr[s][j + 1] - beg;
        const int32_t* rows = p.idx[s] + beg;
        const float* rrow = p.r + j * p.ldr + (int64_t)s * p.K;
        const float* lbase = p.l + (int64_t)s * p.K;
        const float* sbase = p.stats + (int64_t)s * 2 * p.K;
        const float* dbase = p.delta + (int64_t)s * p.K;
        Quad hop;   // NW == 1: ((T0 + T1) + T2) + T3 of this hop, the lane's quad
#pragma unroll
        for (int k = 0; k < 4; ++k) hop.v[k] = 0.f;
        if (NW == 1) {
            wave_lds_sync();   // the previous hop's reads of the set totals come first
            (&wtot[0][0])[lane] = 0.f;   // a set without a chunk: +0
        }
        for (int u = (NW == 1 ? 0 : wave); u < (NW == 1 ? kSets : wave + 1); ++u) {
            if (NW == 1 && u > 0 && (int64_t)u * kWave >= len) break;   // (wave-uniform; set 0 of an empty segment: +0 throughout)
            float acc[kMaxHeads];
#pragma unroll
            for (int h = 0; h < kMaxHeads; ++h) acc[h] = 0.f;
            clear(accx);
            for (int64_t c = (int64_t)u * kWave; c < len; c += kSets * kWave) {   // (wave-uniform)
                const int count = (int)(len - c < kWave ? len - c : kWave);
                const bool ok = lane < count;
                const int64_t ei = rows[c + (ok ? lane : count - 1)];
                const float* lrow = lbase + ei * p.ldl;
                const float* st = sbase + ei * p.ldstats;
                uint32_t keep = 0;
                if constexpr (D::kOn) keep = dp.kept(ei, j, s, p.K);   // the walked entry is (row ei, column j) of the forward operand
                wave_lds_sync();   // the previous chunk's reads of the tiles come first
#pragma unroll
                for (int h = 0; h < kMaxHeads; ++h) {
                    if (h >= p.K) continue;   // (wave-uniform)
                    const float alpha = alpha_of(lrow[h] + rrow[h], p.slope, st[h], st[p.K + h]);
                    if constexpr (D::kOn) {
                        dp.undropped[lane * p.K + h] = alpha;
                        atile[lane * p.K + h] = alpha * dp.factor(keep, h);
                    } else {
                        atile[lane * p.K + h] = alpha;
                    }
                }
                wave_lds_sync();
                chunk_dots<L, NB, true>(p, a, xrow, p.g + (int64_t)s * p.ldg_hop, p.ldg_row, (int)ei, count, lane, dtile, atile, head, accx);
                wave_lds_sync();
                if (p.dr) {   // (the same for the whole grid)
                    const float* drow = dbase + ei * p.lddelta;
#pragma unroll
                    for (int h = 0; h < kMaxHeads; ++h) {
                        if (h >= p.K) continue;   // (wave-uniform)
                        const float pre = lrow[h] + rrow[h];
                        float dalpha = dtile[lane * p.K + h];
                        if constexpr (D::kOn) dalpha = dp.factor(keep, h) * dalpha;   // dalpha = f * dot
                        const float ds = utile[lane * p.K + h] * (dalpha - drow[h]);
                        const float dpre = pre > 0.f ? ds : ds * p.slope;
                        acc[h] = acc[h] + (ok ? dpre : 0.f);   // P[64 u + lane], ascending position
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < kMaxHeads; ++h) {
                if (h >= p.K) continue;   // (wave-uniform)
                const float W = bfly64<Add>(acc[h]);
                if (lane == 0) wtot[u][h] = W;
            }
            // T_u: (P0 + P1) + (P2 + P3) of every column; the lane keeps the quad of block gi
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t = fold_groups(accx[b].v[k]);
                    if (NW == 1) {
                        if (gi == b) hop.v[k] = u == 0 ? t : hop.v[k] + t;
                    } else if (gi == b) {
                        sh.tot[wave][b * kBlockCols + 4 * q + k] = t;
                    }
                }
        }
        if (NW == 1) {
            wave_lds_sync();
#pragma unroll
            for (int k = 0; k < 4; ++k) dxq.v[k] = s == 0 ? hop.v[k] : dxq.v[k] + hop.v[k];
        } else {
            __syncthreads();
            const int c = CW * threadIdx.x;
            if (c < NB * kBlockCols) {
#pragma unroll
                for (int k = 0; k < CW; ++k) {
                    const float t = ((sh.tot[0][c + k] + sh.tot[1][c + k]) + sh.tot[2][c + k]) + sh.tot[3][c + k];
                    dxc[k] = s == 0 ? t : dxc[k] + t;
                }
            }
        }
        if (p.dr && (NW == 1 || wave == 0) && lane < p.K) p.dr[j * p.lddr + (int64_t)s * p.K + lane] = combine_sets(wtot, lane);
        if (NW > 1) __syncthreads();
    }
    if (!p.dx) return;
    TD* dxrow = static_cast<TD*>(p.dx) + j * p.lddx;
    if (NW == 1) {
        if (gi < NB) store_quad(dxrow, gi * kBlockCols + 4 * q, p.d, dxq);
    } else if (CW * (int)threadIdx.x < p.d) {
        if constexpr (CW == 1) dxrow[threadIdx.x] = dxc[0];
        else store_pair(dxrow, 2 * (int)threadIdx.x, dxc[0], dxc[1]);
    }
}

// The body of a column-side kernel.
template <typename TD, int L, int NB, typename P, typename D>
__device__ __forceinline__ void cols_walk(const P& p, const D& dp, Shared<NB, true>& sh) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x < p.geom.n_long) {   // a row that is long in any selected hop (the adjoint's list): all its hops
        col_row<TD, L, NB, kWavesPerBlock>(p, dp, sh, p.geom.long_list[blockIdx.x], lane, wave);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
        bool is_long = false;
        for (int s = 0; s < p.geom.n_sel; ++s) {
            int64_t beg, end;
            segment(p.geom, rp, s, i, &beg, &end);
            is_long = is_long || end - beg >= p.geom.long_threshold;
        }
        if (is_long) continue;   // a workgroup of its own
        col_row<TD, L, NB, 1>(p, dp, sh, row0 + i, lane, wave);
    }
}

// ---- host
// The seven geometries (L, NB) of a kernel pair: head widths 4, 8, 16, 32 with d <= 128 packed (L = w / 4 lanes per head), any other
// shape head-aligned blocks (L = 0) in the narrowest NB that covers d.  The bits do not depend on the geometry: the orders are
// functions of w and of the segment alone.  `launch(std::integral_constant<int, L>, std::integral_constant<int, NB>)` launches it.
template <typename F>
void for_geometry(int d, int K, F&& launch) {
    using std::integral_constant;
    const int w = d / K;
    if (K > 1 && d <= 2 * kBlockCols && w == 4) launch(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    else if (K > 1 && d <= 2 * kBlockCols && w == 8) launch(integral_constant<int, 2>{}, integral_constant<int, 2>{});
    else if (K > 1 && d <= 2 * kBlockCols && w == 16) launch(integral_constant<int, 4>{}, integral_constant<int, 2>{});
    else if (K > 1 && d <= 2 * kBlockCols && w == 32) launch(integral_constant<int, 8>{}, integral_constant<int, 2>{});
    else if (d <= kBlockCols) launch(integral_constant<int, 0>{}, integral_constant<int, 1>{});
    else if (d <= 2 * kBlockCols) launch(integral_constant<int, 0>{}, integral_constant<int, 2>{});
    else launch(integral_constant<int, 0>{}, integral_constant<int, kMaxBlocks>{});
}

// The one launch path of the three backward entry points (attention_backward.hip).
struct Call {   // in the order of the entry points' arguments
    const h2gcn_plan_t* plan;
    uint32_t hop_mask;
    const float* l;
    int64_t ldl;
    const float* r;
    int64_t ldr;
    int32_t K;
    float slope;
    int x_dtype;               // H2GCN_DTYPE_*, of X, Y and G: bf16 names the `_bf16` entry point, which takes either dX; fp32 stores fp32
    const void* X;
    int64_t ldx;
    int32_t d;
    const float* stats;
    int64_t ldstats;
    const void* Y;
    int64_t ldy_row, ldy_hop;
    const void* G;
    int64_t ldg_row, ldg_hop;
    float* delta;
    int64_t lddelta;
    float* dl;
    int64_t lddl;
    float* dr;
    int64_t lddr;
    int dx_dtype;
    void* dX;
    int64_t lddx;
    const attention_dropout::Draw* dropout;    // NULL: none (else fp32 operands)
    void* stream;
};
int run(const Call& c);

// The kernel pairs of the three units behind it, each launched by its own unit.  `cols` NULL: the row side alone.
using Params16 = ParamsT<bf16_t, void>;   // (dX's element type is the column kernel's template parameter)
void launch_pair(const Params& rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, hipStream_t stream);   // attention_backward.hip
void launch_pair_dropout(const Params& rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, const attention_dropout::Args& da,
                         hipStream_t stream);                                                     // attention_dropout_backward.hip
void launch_pair_bf16(const Params16& rows, int64_t row_blocks, const Params16* cols, int64_t col_blocks, bool dx16,
                      hipStream_t stream);                                                        // attention_bf16.hip

}  // namespace attention_backward
}  // namespace h2gcn
