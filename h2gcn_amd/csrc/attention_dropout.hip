// attention_dropout.hip -- dropout on the attention coefficients, drawn INSIDE the kernels: the forward half.
//
//   * h2gcn_attention_hops_heads_stats_dropout_f32: attention_fused_stats_kernel (attention_stats.hip) with the coefficient of every
//     (entry, head) multiplied by its dropout factor f in {0, 1/keep} before it enters the aggregation tree -- ONE fp32 multiply,
//     alpha * f, on the value in the wave's tile; a dropped entry still multiplies (0 * inf = NaN, as in the chain).  The softmax
//     statistics are those of the launch without dropout, bit for bit: the dropout comes after the softmax.
//   * h2gcn_attention_dropout_factors_hops_f32: the factors themselves, f_k [nnz_k, K] entry-major, for the chain and the tests.
//
// The factor is a function of (seed, step, hop, row, column, head) alone (attention_dropout.hip.h): no mask is stored, and the backward
// (attention_dropout_backward.hip) draws the same one again.  The forward kernel keeps a copy of the walk of attention_fused.hip.h, for
// the measured reason at the kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "attention_dropout.hip.h"
#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_dropout {

using namespace attention_fused;

// The lane's own coefficients (entry n = lane of `tile`, written by this lane just before) times the factors of its entry.
__device__ __forceinline__ void drop_tile(const Params& p, const Mask& mk, uint64_t base, bool ok, int lane, float* tile) {
    if (!ok) return;
    float* t = tile + lane * p.K;
    for (int hp = 0; 2 * hp < p.K; ++hp) {
        const uint32_t w = pair_word(mk, base, hp);
        t[2 * hp] = t[2 * hp] * factor(mk, w, 0);
        if (2 * hp + 1 < p.K) t[2 * hp + 1] = t[2 * hp + 1] * factor(mk, w, 1);
    }
}

// attention_fused_stats_kernel whose tiles hold alpha * f: the walk of forward_walk<float, NB, true> (attention_fused.hip.h) with a
// drop_tile call after each of the four places a tile is written.  It is this kernel's OWN COPY of the walk, the one kept copy of the
// refactor that left one walk: built as a wrapper around forward_walk with a tile hook, the kernel kept its registers and occupancy
// (NB = 2: 134 VGPRs against 136, three waves per SIMD either way) but ran the products shape (d = 128, K = 8, keep 0.5) in 44.3 ms
// against 33.4 -- 33.5 ms, and arxiv in 0.66 -- 0.67 ms against 0.59 (profiles/r25_attention_one_walk_parent_vs_this.txt); the occupancy
// attribute was already there.  A fix to forward_walk has to be made here too.  Three waves per SIMD are asked for: NB = 1 then keeps the statistics
// kernel's occupancy (left alone it takes 173 VGPRs and drops to two); NB = 2 and 4 do not reach the statistics kernel's four without
// VGPR spills (it sits at exactly 128 VGPRs) and run at three.
template <int NB>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void attention_fused_stats_dropout_kernel(
    const Params p, float* stats, int64_t ldstats, const Args da) {
    __shared__ Shared<NB> sh;
    constexpr int U = Loads<float>::value / NB;
    constexpr int kPassCols = NB * kBlockCols;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 15, gi = lane >> 4;
    const Mask mk = make_mask(da);
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
                drop_tile(p, mk, entry_base(mk, row, ecol, da.hop[s]), lane < count, lane, tile);
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
            if (__ballot(is_short) != 0ull) {
                ecol = short_tiles<true>(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile,
                                         stat_row(p, stats, ldstats, row0 + i0 + gi, s));
                drop_tile(p, mk, entry_base(mk, row0 + i0 + gi, ecol, da.hop[s]), is_short && q < glen, lane, tile);
            }
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
                    single_chunk_tile<true>(p, s, lrow, ecol, (int)len, lane, tile, stat_row(p, stats, ldstats, row0 + i0 + k, s));
                    drop_tile(p, mk, entry_base(mk, row0 + i0 + k, ecol, da.hop[s]), lane < len, lane, tile);
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
                            drop_tile(p, mk, entry_base(mk, row0 + i0 + k, ecol, da.hop[s]), lane < count, lane, tile);
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

}  // namespace attention_dropout

void attention_fused::launch_stats_dropout(const Params& p, float* stats, int64_t ldstats, const attention_dropout::Args& da, dim3 grid,
                                           hipStream_t stream) {
    for_blocks(p.d, [&](auto nb) {
        hipLaunchKernelGGL((attention_dropout::attention_fused_stats_dropout_kernel<decltype(nb)::value>), grid, dim3(kBlock), 0, stream, p,
                           stats, ldstats, da);
    });
}

namespace attention_dropout {

// ---------------------------------------------------------------------------------------------------------------- the factors
struct FactorParams {
    Geom geom;
    const int32_t* colidx[H2GCN_MAX_HOPS];   // the selected hops, packed as geom.rowptr
    float* f[H2GCN_MAX_HOPS];                // f[s][e * ldf[s] + h]
    int64_t ldf[H2GCN_MAX_HOPS];
    int K;
};

__device__ __forceinline__ void write_factors(const FactorParams& p, const Mask& mk, int64_t row, int s, int hop, int64_t e) {
    const uint64_t base = entry_base(mk, row, p.colidx[s][e], hop);
    float* out = p.f[s] + e * p.ldf[s];
    for (int hp = 0; 2 * hp < p.K; ++hp) {
        const uint32_t w = pair_word(mk, base, hp);
        out[2 * hp] = factor(mk, w, 0);
        if (2 * hp + 1 < p.K) out[2 * hp + 1] = factor(mk, w, 1);
    }
}

// The pattern walk, one lane per entry: reads rowptr / colidx only.
__global__ __launch_bounds__(kBlock) void attention_dropout_factors_kernel(const FactorParams p, const Args da) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Mask mk = make_mask(da);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        for (int64_t e = beg + threadIdx.x; e < end; e += kBlock) write_factors(p, mk, row, s, da.hop[s], e);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i)
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            if (end - beg >= p.geom.long_threshold) continue;   // a workgroup of its own
            for (int64_t e = beg + lane; e < end; e += kWave) write_factors(p, mk, row0 + i, s, da.hop[s], e);
        }
}

static int run_factors(const h2gcn_plan_t* plan, uint32_t hop_mask, int32_t K, float keep_prob, uint64_t seed, const int64_t* step_dev,
                       float* const* f, const int64_t* ldf, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (K < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", K);
        if (K > kMaxHeads)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d > %d: the attention dropout generator serves at most %d heads", K, kMaxHeads,
                        kMaxHeads);
        if ((st = check_keep_prob(keep_prob)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, "f", f)) != H2GCN_OK) return st;
        if (selected_nnz(v) == 0) return H2GCN_OK;
        if (!ldf) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldf_entry is NULL");
        for (int s = 0; s < v.n_sel; ++s)
            if (v.nnz[s] > 0 && ldf[s] < K)
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldf_entry[%d] = %lld < n_heads = %d", s, (long long)ldf[s], K);
        hipStream_t stream = (hipStream_t)stream_v;
        FactorParams p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) p.colidx[s] = v.colidx[s], p.f[s] = f[s], p.ldf[s] = ldf[s];
        p.K = K;
        const Args da = make_args(plan, v.mask, v.n_cols, keep_prob, seed, step_dev);
        hipLaunchKernelGGL(attention_dropout_factors_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, p, da);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_dropout_factors_hops_f32");
    }
}

}  // namespace attention_dropout
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_stats_dropout_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                                 const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev,
                                                 int64_t ldx, int32_t d, float* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev,
                                                 int64_t ldstats, float keep_prob, uint64_t seed, const int64_t* step_dev, void* stream) {
    using namespace h2gcn::attention_dropout;
    if (h2gcn::attention_dropout::check_keep_prob(keep_prob) != H2GCN_OK) return H2GCN_ERR_INVALID_ARGUMENT;
    if (keep_prob == 1.f)   // nothing is dropped and 1/keep = 1: the launch without dropout, its bits
        return h2gcn_attention_hops_heads_stats_f32(plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d, Y_dev,
                                                    ldy_row, ldy_hop, stats_dev, ldstats, stream);
    const h2gcn::attention_dropout::Draw dropout = {keep_prob, seed, step_dev};
    return h2gcn::attention_fused::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_F32, X_dev, ldx, d,
                                        H2GCN_DTYPE_F32, Y_dev, ldy_row, ldy_hop, true, stats_dev, ldstats, &dropout, stream});
}

int h2gcn_attention_dropout_factors_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, int32_t n_heads, float keep_prob, uint64_t seed,
                                             const int64_t* step_dev, float* const* f_dev, const int64_t* ldf_entry, void* stream) {
    return h2gcn::attention_dropout::run_factors(plan, hop_mask, n_heads, keep_prob, seed, step_dev, f_dev, ldf_entry, stream);
}

}  // extern "C"
