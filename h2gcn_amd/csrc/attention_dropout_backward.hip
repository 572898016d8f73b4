// attention_dropout_backward.hip -- the recomputing attention backward (attention_backward.hip) under dropout on the coefficients: the
// factor f[e, h] in {0, 1/keep} of every (entry, head) is drawn again from the generator of attention_dropout.hip.h, keyed by the
// entry's (hop, row, column) in the plan's FORWARD operand on both sides, so the row side (walking A_s) and the column side (walking
// A_s^T, no permutation) see the mask of the forward.  With y = sum_e (alpha f) x_j:
//
//     dalpha[e,h] = f * sum_{c in head h} g[i,s,c] * x[j,c]        delta[i,s,h] = sum_{c in head h} g[i,s,c] * y[i,s,c]   (unchanged:
//     dscore = alpha * (dalpha - delta)                             y carries f, so delta is still sum_e alpha * dalpha)
//     dx[j,c] = sum_s sum over column j of (alpha * f) * g[i,s,c]
//
// f enters in three places: the row side's dalpha (one multiply on the tile's value), the column side's dalpha (the same), and the
// coefficient alpha * f (one multiply, as the forward forms it) the column side feeds to the dx fmafs.  dscore uses the undropped
// alpha, which the column side keeps per chunk in a third LDS tile (lane = entry writes and reads its own row of it): forming it again
// would gather l, m and 1/S of every entry a second time.  The passes, the geometry and every summation order are those of attention_backward.hip; its device functions
// (attention_backward.hip.h) are used unchanged, row_segment / col_row are COPIES with the factor: no existing kernel is compiled
// differently.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_backward.hip.h"
#include "attention_dropout.hip.h"

namespace h2gcn {
namespace attention_dropout {

using namespace attention_backward;

// ---------------------------------------------------------------------------------------------------------------- row side
// Segment (row, s) = entries [beg, beg + len) on NW waves (1: the calling wave, the sets in turn; 4: every thread of the block must
// call, wave w = set w).  Stores delta[row, s, :] and, if wanted, dl[row, s, :].  `hop`: the plan's index of selected hop s.
template <int L, int NB, int NW>
__device__ __forceinline__ void row_segment(const Params& p, const Mask& mk, int hop, Shared<NB, false>& sh, int64_t row, int s, int64_t beg,
                                            int64_t len, int lane, int wave) {
    const int q = lane & 15;
    const float* grow = p.g + row * p.ldg_row + (int64_t)s * p.ldg_hop;
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
            const uint32_t keep = kept_heads(mk, entry_base(mk, row, ecol, hop), p.K);
#pragma unroll
            for (int h = 0; h < kMaxHeads; ++h) {
                if (h >= p.K) continue;   // (wave-uniform)
                const float pre = lrow[h] + rrow[h];
                const float f = (keep >> h) & 1u ? mk.inv_keep : 0.f;
                const float ds = alpha_of(pre, p.slope, st[h], st[p.K + h]) * (f * dtile[lane * p.K + h] - delta[h]);   // dalpha = f * dot
                const float dp = pre > 0.f ? ds : ds * p.slope;
                acc[h] = acc[h] + (ok ? dp : 0.f);   // P[64 u + lane], ascending position
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

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_rows_dropout_kernel(const Params p, const Args da) {
    __shared__ Shared<NB, false> sh;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Mask mk = make_mask(da);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        row_segment<L, NB, kWavesPerBlock>(p, mk, da.hop[s], sh, row, s, beg, end - beg, lane, wave);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i)
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            if (end - beg >= p.geom.long_threshold) continue;   // a workgroup of its own
            row_segment<L, NB, 1>(p, mk, da.hop[s], sh, row0 + i, s, beg, end - beg, lane, wave);
        }
}

// ------------------------------------------------------------------------------------------------------------- column side
// Column j of the forward operands = row j of every selected A_s^T, on NW waves (as row_segment).  Stores dr[j, :, :] and dx[j, :]
// where wanted.
template <int L, int NB, int NW>
__device__ __forceinline__ void col_row(const Params& p, const Mask& mk, const Args& da, Shared<NB, true>& sh, float* utile, int64_t j, int lane,
                                        int wave) {
    const int q = lane & 15, gi = lane >> 4;
    const float* xrow = p.x + j * p.ldx;
    float* dtile = sh.dtile[wave];
    float* atile = sh.atile[wave];
    float (*wtot)[kMaxHeads] = sh.w[NW == 1 ? wave : 0];
    Quad a[NB], accx[NB];
    int head[NB];
    load_row(p, xrow, q, a);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int h = (b * kBlockCols + 4 * q) / p.w;
        head[b] = h < p.K ? h : p.K - 1;   // (a quad beyond d: its sums are never stored)
    }
    Quad dxq;        // NW == 1: the running hop sum of the quad this lane stores
    float dxc = 0.f; // NW == 4: the running hop sum of column threadIdx.x
#pragma unroll
    for (int k = 0; k < 4; ++k) dxq.v[k] = 0.f;
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
                // the walked entry is (row ei, column j) of the forward operand
                const uint32_t keep = kept_heads(mk, entry_base(mk, ei, j, da.hop[s]), p.K);
                wave_lds_sync();   // the previous chunk's reads of the tiles come first
#pragma unroll
                for (int h = 0; h < kMaxHeads; ++h) {
                    if (h >= p.K) continue;   // (wave-uniform)
                    const float f = (keep >> h) & 1u ? mk.inv_keep : 0.f;
                    const float alpha = alpha_of(lrow[h] + rrow[h], p.slope, st[h], st[p.K + h]);
                    utile[lane * p.K + h] = alpha;       // the undropped alpha, for this lane's dscore below
                    atile[lane * p.K + h] = alpha * f;   // alpha * f, as the forward forms it
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
                        const float f = (keep >> h) & 1u ? mk.inv_keep : 0.f;
                        const float ds = utile[lane * p.K + h] * (f * dtile[lane * p.K + h] - drow[h]);   // the undropped alpha
                        const float dp = pre > 0.f ? ds : ds * p.slope;
                        acc[h] = acc[h] + (ok ? dp : 0.f);   // P[64 u + lane], ascending position
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
            const int c = threadIdx.x;
            if (c < NB * kBlockCols) {
                const float t = ((sh.tot[0][c] + sh.tot[1][c]) + sh.tot[2][c]) + sh.tot[3][c];
                dxc = s == 0 ? t : dxc + t;
            }
        }
        if (p.dr && (NW == 1 || wave == 0) && lane < p.K) p.dr[j * p.lddr + (int64_t)s * p.K + lane] = combine_sets(wtot, lane);
        if (NW > 1) __syncthreads();
    }
    if (!p.dx) return;
    if (NW == 1) {
        if (gi < NB) store_quad(p.dx + j * p.lddx, gi * kBlockCols + 4 * q, p.d, dxq);
    } else if ((int)threadIdx.x < p.d) {
        p.dx[j * p.lddx + threadIdx.x] = dxc;
    }
}

template <int L, int NB>
// (three waves per SIMD are asked for -- the column side's occupancy without dropout: left alone one form took scratch)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void attention_backward_cols_dropout_kernel(const Params p,
                                                                                                                   const Args da) {
    __shared__ Shared<NB, true> sh;
    __shared__ float undropped[kWavesPerBlock][kWave * kMaxHeads];   // per wave: alpha of the chunk at hand before the factor (lane = entry)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Mask mk = make_mask(da);
    if ((int)blockIdx.x < p.geom.n_long) {   // a row that is long in any selected hop (the adjoint's list): all its hops
        col_row<L, NB, kWavesPerBlock>(p, mk, da, sh, undropped[wave], p.geom.long_list[blockIdx.x], lane, wave);
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
        col_row<L, NB, 1>(p, mk, da, sh, undropped[wave], row0 + i, lane, wave);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
template <int L, int NB>
void launch_pair(const Params* rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, const Args& da, hipStream_t stream) {
    if (rows)
        hipLaunchKernelGGL((attention_backward_rows_dropout_kernel<L, NB>), dim3((unsigned)row_blocks), dim3(kBlock), 0, stream, *rows, da);
    if (cols)
        hipLaunchKernelGGL((attention_backward_cols_dropout_kernel<L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols, da);
}

// (L, NB): the geometry the shared path chose, one of the seven of attention_backward.hip
static void launch_dropout(int L, int NB, const Params* rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, const PatternView& v,
                           const void* ctx_v, hipStream_t stream) {
    const Context& c = *static_cast<const Context*>(ctx_v);
    const Args da = make_args(c.plan, v.mask, v.n_cols, c.keep_prob, c.seed, c.step_dev);   // (v: the forward view on both sides)
    if (L == 1) launch_pair<1, 2>(rows, row_blocks, cols, col_blocks, da, stream);
    else if (L == 2) launch_pair<2, 2>(rows, row_blocks, cols, col_blocks, da, stream);
    else if (L == 4) launch_pair<4, 2>(rows, row_blocks, cols, col_blocks, da, stream);
    else if (L == 8) launch_pair<8, 2>(rows, row_blocks, cols, col_blocks, da, stream);
    else if (NB == 1) launch_pair<0, 1>(rows, row_blocks, cols, col_blocks, da, stream);
    else if (NB == 2) launch_pair<0, 2>(rows, row_blocks, cols, col_blocks, da, stream);
    else launch_pair<0, kMaxBlocks>(rows, row_blocks, cols, col_blocks, da, stream);
}

}  // namespace attention_dropout
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_backward_dropout_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                                    const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope,
                                                    const float* X_dev, int64_t ldx, int32_t d, const float* stats_dev, int64_t ldstats,
                                                    const float* Y_dev, int64_t ldy_row, int64_t ldy_hop, const float* G_dev, int64_t ldg_row,
                                                    int64_t ldg_hop, float* delta_dev, int64_t lddelta, float* dl_dev, int64_t lddl,
                                                    float* dr_dev, int64_t lddr, float* dX_dev, int64_t lddx, float keep_prob, uint64_t seed,
                                                    const int64_t* step_dev, void* stream) {
    using namespace h2gcn::attention_dropout;
    if (check_keep_prob(keep_prob) != H2GCN_OK) return H2GCN_ERR_INVALID_ARGUMENT;
    const Context ctx = {plan, keep_prob, seed, step_dev};
    // keep_prob = 1: nothing is dropped and 1/keep = 1 -- the launches without dropout, their bits
    return h2gcn::attention_backward::run(plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d, stats_dev, ldstats,
                                          Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev, lddl, dr_dev, lddr,
                                          dX_dev, lddx, stream, keep_prob == 1.f ? nullptr : launch_dropout, &ctx);
}

}  // extern "C"
