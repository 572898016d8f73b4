// attention_fused.hip -- the forward of the attention chain in ONE launch, for every forward that needs no gradient:
//
//     Y[i, s, c] = sum_e alpha_s[e, h(c)] * X[j_e, c]          e over row i of selected hop s, h(c) = c / (d / K)
//     alpha_s[., h] = softmax over the segment of leaky(l[i, s, h] + r[j_e, s, h])
//
// what h2gcn_edge_scores_hops_heads_f32 -> h2gcn_row_softmax_hops_heads_f32 -> h2gcn_spmm_hops_values_f32 compute through two
// entry-major [nnz_k, K] arrays, BIT FOR BIT, without those arrays: nothing of size nnz is written or allocated, the only store
// is Y.  A translation unit of its own: no existing kernel is compiled differently because of it.
//
// Why the bits are the chain's.  Every value the chain stores is a function of operands this kernel also has, so it is computed
// again with the chain's own operations wherever it is needed (include/h2gcn_hip.h has the three orders):
//   * score = leaky(l + r): one addition, one multiplication on the `pre > 0`-false branch -- per (entry, head), no order;
//   * m: a maximum has no order; a NaN score is carried in a flag beside it, per head, and makes m NaN;
//   * e_j = exp2((score_j - m) * log2e), the one hardware exponential; P[j mod 256] accumulated from +0 in ascending j -- a lane
//     that is entry j mod 64 of chunk j / 64 keeps P[64 u + lane] for the chunks = u (mod 4); W_u the xor butterfly over
//     P[64u .. 64u+63]; S = (W_0 + W_1) + (W_2 + W_3); one correctly rounded 1/S; alpha_j = e_j * (1/S), e_j recomputed by the same
//     two operations.  A partial that got no entry is +0 and adds no bit, so W_u of an absent chunk class is skipped;
//   * the aggregation is spmm_values.hip's walk with the loads of V[e, h] replaced by reads of alpha: entry jj of a chunk goes
//     into P[jj & 3] of lane group jj & 3 with one fmaf, the element is (P0 + P1) + (P2 + P3), long segments ((T0 + T1) + T2) + T3.
//
// Mapping (gfx950, wave64; the pattern walk of pattern_walk.hip.h; no atomics, no scratch, no workspace):
//   * a segment belongs to the wave that owns its row, a segment of the plan's long list to a workgroup whose wave w takes the
//     chunks = w (mod 4): exactly the owner of W_w in the softmax tree and of T_w in the aggregation tree;
//   * walk A, lane = entry: colidx 64 at a time, r[j, s, h0 .. h0+3] in one 16-byte gather, FOUR heads per pass (the head group);
//     per head group one sweep for the maxima and one for the partial sums; (m, 1/S) of all heads go to 2 K floats of LDS;
//   * a segment of at most 64 entries (most of them) is one chunk: its scores stay in registers between the sweeps and the
//     coefficients e * (1/S) go straight into the tile -- one exponential per (entry, head);
//   * segments of at most 16 entries take walk A FOUR AT A TIME, lane group gi the segment of row i0 + gi: the reductions stay
//     inside the 16-lane group (DPP only), the colidx / r latencies of four segments overlap, and group gi's coefficients are the
//     entries 16 gi .. of the tile; walk B then serves the four segments in turn;
//   * walk B, per chunk: lane = entry writes the K coefficients of its entry into the wave's 64 x K LDS tile (entry-major, as the
//     chain's array), then the geometry of spmm_values.hip -- 16 lanes x 4 columns per 64-column block, group gi the entries
//     = gi (mod 4) -- reads tile[n * K + head] where that kernel loads V: the staged tile saves 16 redundant exponentials per
//     (entry, head).  Column ids are fetched once per chunk (lane = entry) and handed out with ds_bpermute;
//   * a width beyond 256 columns repeats walk B per column pass, never walk A.
// LDS: 4 tiles of 64 x 16 floats (16 KiB) + statistics and cross-wave words (1 KiB) + the long path's wave totals (1 - 4 KiB).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_fused {

template <int NB>
__global__ __launch_bounds__(kBlock) void attention_fused_kernel(const Params p) {
    constexpr int U = kLoads / NB;
    constexpr int kPassCols = NB * kBlockCols;
    __shared__ Shared<NB> sh;
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
            if (__ballot(is_short) != 0ull) ecol = short_tiles(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile);
            wave_lds_sync();
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len < 0 || len > kGroup) continue;   // (wave-uniform) no such row, a long segment, or one for the loop below
                float* out = p.y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
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
                    single_chunk_tile(p, s, lrow, ecol, (int)len, lane, tile);
                } else {
                    segment_stats<1>(p, s, lrow, cols, len, lane, 0, nullptr, stat);
                }
                wave_lds_sync();
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

// the three geometries of attention_fused_kernel
static void launch_forward(const Params& p, float*, int64_t, dim3 grid, hipStream_t stream) {
    const dim3 block(kBlock);
    const int d = p.d;
    // blocks of accumulators a lane keeps: the narrowest geometry that covers d in one column pass, four blocks beyond 256 columns
    // (the bits are the same for all three: every column has its own tree)
    if (d <= kBlockCols) hipLaunchKernelGGL((attention_fused_kernel<1>), grid, block, 0, stream, p);
    else if (d <= 2 * kBlockCols) hipLaunchKernelGGL((attention_fused_kernel<2>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((attention_fused_kernel<kMaxBlocks>), grid, block, 0, stream, p);
}

// ------------------------------------------------------------------------------------------------------------ host
// The launch path of h2gcn_attention_hops_heads_f32 (stats_launcher NULL) and of h2gcn_attention_hops_heads_stats_f32
// (attention_stats.hip: its launcher, and stats [n_rows, H_sel, 2, K] through ldstats).
int run(Launcher stats_launcher, float* stats, int64_t ldstats, const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl,
        const float* r, int64_t ldr, int32_t n_heads, float slope, const float* X, int64_t ldx, int32_t d, float* Y, int64_t ldy_row,
        int64_t ldy_hop, void* stream_v, ViewLauncher view_launcher, const void* ctx) {
    try {
        // every check below comes before the device is touched
        const bool with_stats = stats_launcher || view_launcher;
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
        if (n_heads < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", n_heads);
        if (n_heads > kMaxHeads)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d > %d: the fused attention forward serves at most %d heads (run the chain)",
                        n_heads, kMaxHeads, kMaxHeads);
        if (d % n_heads) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d is not a multiple of n_heads = %d", d, n_heads);
        if (n_heads > 1 && (d / n_heads) % 4)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "d / n_heads = %d is not a multiple of 4 (a lane's four columns must lie in one head)",
                        d / n_heads);
        const int64_t need = (int64_t)v.n_sel * n_heads;
        if (ldl < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldl = %lld < H_sel * n_heads = %lld", (long long)ldl, (long long)need);
        if (ldr < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldr = %lld < H_sel * n_heads = %lld", (long long)ldr, (long long)need);
        if (ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ldx, d);
        if (ldy_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_row = %lld < d = %d", (long long)ldy_row, d);
        if (ldy_hop < 0 || (v.n_sel > 1 && ldy_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_hop = %lld < d = %d: hop outputs would overlap", (long long)ldy_hop, d);
        if (v.n_rows == 0) return H2GCN_OK;   // nothing to store
        if (!Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y is NULL");
        if (selected_nnz(v) > 0 && !l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "l is NULL");
        if (selected_nnz(v) > 0 && !r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "r is NULL");
        if (selected_nnz(v) > 0 && !X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "X is NULL");
        if (Y == X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases X");
        if (Y == l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases l");
        if (Y == r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases r");
        if (with_stats) {
            if (ldstats < 2 * need)
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldstats = %lld < H_sel * 2 * n_heads = %lld", (long long)ldstats, (long long)(2 * need));
            if (!stats) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats is NULL");
            if (stats == Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases Y");
            if (stats == X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases X");
            if (stats == l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases l");
            if (stats == r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases r");
        }
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) {   // a selection without nonzeros: every row is empty
            for (int s = 0; s < v.n_sel; ++s)
                H2GCN_HIP_TRY(hipMemset2DAsync(Y + (int64_t)s * ldy_hop, (size_t)ldy_row * sizeof(float), 0, (size_t)d * sizeof(float),
                                               (size_t)v.n_rows, stream));
            if (with_stats)   // every segment is empty: (+0, +0)
                H2GCN_HIP_TRY(hipMemset2DAsync(stats, (size_t)ldstats * sizeof(float), 0, (size_t)(2 * need) * sizeof(float), (size_t)v.n_rows,
                                               stream));
            return H2GCN_OK;
        }
        for (int s = 0; s < v.n_sel; ++s) p.colidx[s] = v.colidx[s];
        p.l = l, p.ldl = ldl;
        p.r = r, p.ldr = ldr;
        p.x = X, p.ldx = ldx;
        p.y = Y, p.ldy_row = ldy_row, p.ldy_hop = ldy_hop;
        p.d = d, p.K = n_heads, p.head_cols = d / n_heads;
        p.slope = slope;
        if (view_launcher) view_launcher(p, stats, ldstats, v, ctx, dim3((unsigned)n_blocks), stream);
        else (stats_launcher ? stats_launcher : launch_forward)(p, stats, ldstats, dim3((unsigned)n_blocks), stream);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads%s_f32", view_launcher ? "_stats_dropout" : (stats_launcher ? "_stats" : ""));
    }
}

}  // namespace attention_fused
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                   int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                   float* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream) {
    return h2gcn::attention_fused::run(nullptr, nullptr, 0, plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d,
                                       Y_dev, ldy_row, ldy_hop, stream);
}

}  // extern "C"
