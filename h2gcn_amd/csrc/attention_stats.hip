// attention_stats.hip -- h2gcn_attention_hops_heads_stats_f32: the fused attention forward of attention_fused.hip that ALSO STORES
// the softmax statistics (m, 1/S) of every (row, hop, head) -- stats[i, s, 0, h] = m, stats[i, s, 1, h] = 1/S, what the recomputing
// backward (attention_backward.hip) needs to form alpha again per entry.  The values are the ones the walk holds anyway, in
// Shared::stat or in registers on the single-chunk and short paths; Y is bit for bit attention_fused_kernel's: the walk, the device
// functions (attention_fused.hip.h) and every operation on the way to Y are the same.  An empty segment stores (+0, +0).
//
// A translation unit of its own, and a COPY of the kernel's walk with the stores added, not a template flag on it: the three
// instantiations of attention_fused_kernel keep their registers, LDS and occupancy to the line, which a shared body did not give.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_fused {

// attention_fused_kernel, storing the softmax statistics of every (row, hop, head) as well -- values the walk holds anyway.
template <int NB>
__global__ __launch_bounds__(kBlock) void attention_fused_stats_kernel(const Params p, float* stats, int64_t ldstats) {
    __shared__ Shared<NB> sh;
    constexpr int U = kLoads / NB;
    constexpr int kPassCols = NB * kBlockCols;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 15, gi = lane >> 4;
    float* tile = sh.tile[wave];
    int head[NB];
    Quad acc[NB];
    const bool one_pass = p.d <= kPassCols;   // the heads of the lane's blocks are then the same for every segment
    pass_heads(p, 0, q, head);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        const int64_t len = end - beg;   // (the same for the whole block)
        const float* lrow = p.l + row * p.ldl + (int64_t)s * p.K;
        const int32_t* cols = p.colidx[s] + beg;
        float* out = p.y + row * p.ldy_row + (int64_t)s * p.ldy_hop;
        if (len > 0) segment_stats<kWavesPerBlock>(p, s, lrow, cols, len, lane, wave, sh.red, sh.stat[0]);
        __syncthreads();
        {
            float* st = stat_row(p, stats, ldstats, row, s);
            if (len > 0) store_stats(p, sh.stat[0], st, threadIdx.x);
            else if ((int)threadIdx.x < 2 * p.K) st[threadIdx.x] = 0.f;
        }
        for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
            clear(acc);
            if (!one_pass) pass_heads(p, cbase, q, head);
            for (int64_t c = (int64_t)wave * kWave; c < len; c += kBlock) {
                const int count = (int)(len - c < kWave ? len - c : kWave);
                const int ecol = cols[c + (lane < count ? lane : count - 1)];
                wave_lds_sync();   // the previous chunk's reads of the tile come first
                chunk_tile(p, s, lrow, ecol, count, lane, sh.stat[0], tile);
                wave_lds_sync();
                gather_chunk<NB, U>(p, tile, head, cbase, count, ecol, 0, lane, acc);
            }
            const Quad mine = fold_blocks(acc, gi);
            if (gi < NB) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sh.tot[wave][gi * kBlockCols + 4 * q + k] = mine.v[k];
            }
            __syncthreads();
            const int c = threadIdx.x;
            if (c < kPassCols && cbase + c < p.d) out[cbase + c] = ((sh.tot[0][c] + sh.tot[1][c]) + sh.tot[2][c]) + sh.tot[3][c];
            __syncthreads();
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    float* stat = sh.stat[wave];
    const int rpw = p.geom.rows_per_wave;
    for (s = 0; s < p.geom.n_sel; ++s) {
        for (int i0 = 0; i0 < rpw && row0 + i0 < p.geom.n_rows; i0 += 4) {
            // lane group gi looks at row i0 + gi: segments of at most 16 entries get their coefficients FOUR AT A TIME
            int64_t gbeg, glen;
            group_segment<false>(p.geom, s, i0, row0, rp, lane, &gbeg, &glen);
            const bool is_short = glen >= 1 && glen <= kGroup;
            int ecol = 0;
            wave_lds_sync();   // the previous segments' reads of the tile come first
            if (__ballot(is_short) != 0ull)
                ecol = short_tiles_stats(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile,
                                         stat_row(p, stats, ldstats, row0 + i0 + gi, s));
            wave_lds_sync();
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len < 0 || len > kGroup) continue;   // (wave-uniform) no such row, a long segment, or one for the loop below
                float* out = p.y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                if (len == 0 && lane < 2 * p.K) stat_row(p, stats, ldstats, row0 + i0 + k, s)[lane] = 0.f;   // an empty segment
                for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                    clear(acc);
                    if (!one_pass) pass_heads(p, cbase, q, head);
                    if (len > 0) gather_chunk<NB, U>(p, tile + k * kGroup * p.K, head, cbase, (int)len, ecol, k * kGroup, lane, acc);
                    const Quad mine = fold_blocks(acc, gi);   // (an empty segment: +0)
                    if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
                }
            }
            // the longer segments of these rows, one at a time on the whole wave
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len <= kGroup) continue;   // (wave-uniform)
                beg = readlane64(gbeg, k * kGroup);
                const float* lrow = p.l + (row0 + i0 + k) * p.ldl + (int64_t)s * p.K;
                const int32_t* cols = p.colidx[s] + beg;
                float* out = p.y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                const bool single = len <= kWave;   // (wave-uniform)
                wave_lds_sync();   // the previous segment's reads of the tile and of the statistics come first
                if (single) {
                    ecol = cols[lane < len ? lane : len - 1];
                    single_chunk_tile_stats(p, s, lrow, ecol, (int)len, lane, tile, stat_row(p, stats, ldstats, row0 + i0 + k, s));
                } else {
                    segment_stats<1>(p, s, lrow, cols, len, lane, 0, nullptr, stat);
                }
                wave_lds_sync();
                if (!single) store_stats(p, stat, stat_row(p, stats, ldstats, row0 + i0 + k, s), lane);
                for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                    clear(acc);
                    if (!one_pass) pass_heads(p, cbase, q, head);
                    if (single) {
                        gather_chunk<NB, U>(p, tile, head, cbase, (int)len, ecol, 0, lane, acc);
                    } else {
                        for (int64_t c = 0; c < len; c += kWave) {
                            const int count = (int)(len - c < kWave ? len - c : kWave);
                            ecol = cols[c + (lane < count ? lane : count - 1)];
                            wave_lds_sync();
                            chunk_tile(p, s, lrow, ecol, count, lane, stat, tile);
                            wave_lds_sync();
                            gather_chunk<NB, U>(p, tile, head, cbase, count, ecol, 0, lane, acc);
                        }
                    }
                    const Quad mine = fold_blocks(acc, gi);
                    if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
                }
            }
        }
    }
}

static void launch_stats(const Params& p, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream) {
    const dim3 block(kBlock);
    // (the geometries of the plain forward)
    if (p.d <= kBlockCols) hipLaunchKernelGGL((attention_fused_stats_kernel<1>), grid, block, 0, stream, p, stats, ldstats);
    else if (p.d <= 2 * kBlockCols) hipLaunchKernelGGL((attention_fused_stats_kernel<2>), grid, block, 0, stream, p, stats, ldstats);
    else hipLaunchKernelGGL((attention_fused_stats_kernel<kMaxBlocks>), grid, block, 0, stream, p, stats, ldstats);
}

}  // namespace attention_fused
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_stats_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                         int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                         float* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats, void* stream) {
    using namespace h2gcn::attention_fused;
    return run(launch_stats, stats_dev, ldstats, plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d, Y_dev,
               ldy_row, ldy_hop, stream);
}

}  // extern "C"
