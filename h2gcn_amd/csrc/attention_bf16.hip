// attention_bf16.hip -- the three launches of the recomputing hop attention on bf16 embeddings:
//
//     h2gcn_attention_hops_heads_bf16            attention_fused.hip's forward,            X bf16, Y bf16 or fp32
//     h2gcn_attention_hops_heads_stats_bf16      attention_stats.hip's forward + (m, 1/S), X bf16, Y bf16 or fp32
//     h2gcn_attention_hops_heads_backward_bf16   attention_backward.hip's two sides,       X, Y, G bf16, dX bf16 or fp32
//
// The contract is the bf16 SpMM's: every gathered bf16 element is WIDENED EXACTLY (a shift or a mask), every operation of the fp32
// kernel runs in fp32 in the documented order, and an output is rounded ONCE, to nearest even, where it is stored.  So an fp32 output
// has the bits of the fp32 launch on the upcast operands and a bf16 output is that value rounded; l, r, stats, delta, dl and dr -- K
// wide, not d wide -- stay fp32.  The device functions are the fp32 units' own (attention_fused.hip.h, attention_backward.hip.h,
// segment_ops.hip.h) with the element type of the wide operand as a template parameter; walk A, which reads l and r only, is the same
// code.  The kernels below are the fp32 walks with three differences:
//   * a bf16 quad is ONE 8-byte load (4, 2 or 0 valid columns: d is even) that stays packed until the FMA / dot product that
//     consumes it.  The backward's batches keep 16 of them in flight instead of 8 -- the same 8 KiB per wave, the registers of the
//     fp32 batch; the forward keeps 8: with 16 its batch also holds the coefficients and row addresses of twice the rounds, which
//     cost it half its occupancy and were measured slower (kLoadsBf16 in attention_fused.hip.h);
//   * Y and dX are packed with v_cvt_pk_bf16_f32 and stored as dwords.  The two epilogues that write one column per thread in the
//     fp32 kernels (a long segment's Y, a long column's dX) write one PAIR of columns per thread here, so that no 2-byte store has a
//     neighbour to race with;
//   * dX is rounded after the sum over the hops.
// A translation unit of its own: no existing kernel is compiled differently because of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

#include "attention_fused.hip.h"
#include "attention_backward.hip.h"   // (#pragma clang fp contract(off) from here on, as in the fp32 backward)

namespace h2gcn {
namespace attention_bf16 {

using namespace pattern;

// bf16 arrays: 4-byte aligned base, even strides (elements) and an even width (the rule of the bf16 SpMM launches)
static int check_bf16_layout(const char* what, const void* ptr, int64_t ld_row, int64_t ld_hop, int32_t d) {
    if (reinterpret_cast<uintptr_t>(ptr) & 3u)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: the base address must be 4-byte aligned", what);
    if ((ld_row & 1) || (ld_hop & 1))
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: row / hop strides must be even (got %lld / %lld elements)", what,
                    (long long)ld_row, (long long)ld_hop);
    if (d & 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: the feature width d must be even (got %d)", what, d);
    return H2GCN_OK;
}

static int check_dtype(const char* what, int dtype) {
    if (dtype != H2GCN_DTYPE_F32 && dtype != H2GCN_DTYPE_BF16)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s = %d: must be H2GCN_DTYPE_F32 (%d) or H2GCN_DTYPE_BF16 (%d)", what, dtype,
                    H2GCN_DTYPE_F32, H2GCN_DTYPE_BF16);
    return H2GCN_OK;
}

// `width` elements of `elem` bytes in each of `n` rows `ld` elements apart: +0 in either format
static int zero_rows(void* out, int64_t ld, int64_t width, int64_t n, size_t elem, hipStream_t stream) {
    if (out && n > 0 && width > 0) H2GCN_HIP_TRY(hipMemset2DAsync(out, (size_t)ld * elem, 0, (size_t)width * elem, (size_t)n, stream));
    return H2GCN_OK;
}

// ================================================================================================================ forward
namespace fwd {

using namespace attention_fused;
using P16 = ParamsT<bf16_t, void>;   // (the output's element type is the kernel's template parameter)

// attention_fused_kernel / attention_fused_stats_kernel (STATS) on a bf16 X, storing TY.
template <typename TY, int NB, bool STATS>
__global__ __launch_bounds__(kBlock) void attention_bf16_kernel(const P16 p, float* stats, int64_t ldstats) {
    __shared__ Shared<NB> sh;
    constexpr int U = kLoadsBf16 / NB;
    constexpr int kPassCols = NB * kBlockCols;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 15, gi = lane >> 4;
    float* tile = sh.tile[wave];
    TY* const y = static_cast<TY*>(p.y);
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
        TY* out = y + row * p.ldy_row + (int64_t)s * p.ldy_hop;
        if (len > 0) segment_stats<kWavesPerBlock>(p, s, lrow, cols, len, lane, wave, sh.red, sh.stat[0]);
        __syncthreads();
        if constexpr (STATS) {
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
            const int c = 2 * threadIdx.x;   // one PAIR of columns per thread (d is even): a bf16 pair is one dword
            if (c < kPassCols && cbase + c < p.d)
                store_pair(out, cbase + c, ((sh.tot[0][c] + sh.tot[1][c]) + sh.tot[2][c]) + sh.tot[3][c],
                           ((sh.tot[0][c + 1] + sh.tot[1][c + 1]) + sh.tot[2][c + 1]) + sh.tot[3][c + 1]);
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
                if constexpr (STATS)
                    ecol = short_tiles_stats(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile,
                                             stat_row(p, stats, ldstats, row0 + i0 + gi, s));
                else ecol = short_tiles(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile);
            }
            wave_lds_sync();
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len < 0 || len > kGroup) continue;   // (wave-uniform) no such row, a long segment, or one for the loop below
                TY* out = y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                if (STATS && len == 0 && lane < 2 * p.K) stat_row(p, stats, ldstats, row0 + i0 + k, s)[lane] = 0.f;   // an empty segment
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
                TY* out = y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                const bool single = len <= kWave;   // (wave-uniform)
                wave_lds_sync();   // the previous segment's reads of the tile and of the statistics come first
                if (single) {
                    ecol = cols[lane < len ? lane : len - 1];
                    if constexpr (STATS)
                        single_chunk_tile_stats(p, s, lrow, ecol, (int)len, lane, tile, stat_row(p, stats, ldstats, row0 + i0 + k, s));
                    else single_chunk_tile(p, s, lrow, ecol, (int)len, lane, tile);
                } else {
                    segment_stats<1>(p, s, lrow, cols, len, lane, 0, nullptr, stat);
                }
                wave_lds_sync();
                if (STATS && !single) store_stats(p, stat, stat_row(p, stats, ldstats, row0 + i0 + k, s), lane);
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

template <typename TY, bool STATS>
static void launch(const P16& p, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream) {
    const dim3 block(kBlock);
    // (the geometries of the fp32 forward: the bits are the same for all three, every column has its own tree)
    if (p.d <= kBlockCols) hipLaunchKernelGGL((attention_bf16_kernel<TY, 1, STATS>), grid, block, 0, stream, p, stats, ldstats);
    else if (p.d <= 2 * kBlockCols) hipLaunchKernelGGL((attention_bf16_kernel<TY, 2, STATS>), grid, block, 0, stream, p, stats, ldstats);
    else hipLaunchKernelGGL((attention_bf16_kernel<TY, kMaxBlocks, STATS>), grid, block, 0, stream, p, stats, ldstats);
}

// The launch path of both forward entry points: the checks of attention_fused::run in its order, the layout rule of every bf16 array
// after the strides it speaks of.
static int run(bool with_stats, float* stats, int64_t ldstats, const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl,
               const float* r, int64_t ldr, int32_t n_heads, float slope, const uint16_t* X, int64_t ldx, int32_t d, int y_dtype, void* Y,
               int64_t ldy_row, int64_t ldy_hop, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_dtype("y_dtype", y_dtype)) != H2GCN_OK) return st;
        const bool y16 = y_dtype == H2GCN_DTYPE_BF16;
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
        if ((st = check_bf16_layout("X", X, ldx, 0, d)) != H2GCN_OK) return st;
        if (y16 && (st = check_bf16_layout("Y", Y, ldy_row, ldy_hop, d)) != H2GCN_OK) return st;
        if (v.n_rows == 0) return H2GCN_OK;   // nothing to store
        if (!Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y is NULL");
        if (selected_nnz(v) > 0 && !l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "l is NULL");
        if (selected_nnz(v) > 0 && !r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "r is NULL");
        if (selected_nnz(v) > 0 && !X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "X is NULL");
        if (Y == (const void*)X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases X");
        if (Y == (const void*)l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases l");
        if (Y == (const void*)r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases r");
        if (with_stats) {
            if (ldstats < 2 * need)
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldstats = %lld < H_sel * 2 * n_heads = %lld", (long long)ldstats, (long long)(2 * need));
            if (!stats) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats is NULL");
            if ((void*)stats == Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases Y");
            if ((const void*)stats == (const void*)X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases X");
            if (stats == l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases l");
            if (stats == r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases r");
        }
        hipStream_t stream = (hipStream_t)stream_v;
        P16 p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) {   // a selection without nonzeros: every row is empty
            const size_t elem = y16 ? sizeof(uint16_t) : sizeof(float);
            for (int s = 0; s < v.n_sel; ++s)
                if ((st = zero_rows((char*)Y + (size_t)s * (size_t)ldy_hop * elem, ldy_row, d, v.n_rows, elem, stream)) != H2GCN_OK) return st;
            if (with_stats) return zero_rows(stats, ldstats, 2 * need, v.n_rows, sizeof(float), stream);   // every segment: (+0, +0)
            return H2GCN_OK;
        }
        for (int s = 0; s < v.n_sel; ++s) p.colidx[s] = v.colidx[s];
        p.l = l, p.ldl = ldl;
        p.r = r, p.ldr = ldr;
        p.x = reinterpret_cast<const bf16_t*>(X), p.ldx = ldx;
        p.y = Y, p.ldy_row = ldy_row, p.ldy_hop = ldy_hop;
        p.d = d, p.K = n_heads, p.head_cols = d / n_heads;
        p.slope = slope;
        const dim3 grid((unsigned)n_blocks);
        if (with_stats) (y16 ? launch<bf16_t, true> : launch<float, true>)(p, stats, ldstats, grid, stream);
        else (y16 ? launch<bf16_t, false> : launch<float, false>)(p, nullptr, 0, grid, stream);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads%s_bf16", with_stats ? "_stats" : "");
    }
}

}  // namespace fwd

// =============================================================================================================== backward
namespace bwd {

using namespace attention_backward;
using P16 = ParamsT<bf16_t, void>;   // (dX's element type is the column kernel's template parameter)

// ---------------------------------------------------------------------------------------------------------------- row side
// attention_backward.hip's row_segment on bf16 g, y and x: delta = <g, y> on the bf16 y the forward stored.
template <int L, int NB, int NW>
__device__ __forceinline__ void row_segment(const P16& p, Shared<NB, false>& sh, int64_t row, int s, int64_t beg, int64_t len, int lane, int wave) {
    const int q = lane & 15;
    const bf16_t* grow = p.g + row * p.ldg_row + (int64_t)s * p.ldg_hop;
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
#pragma unroll
            for (int h = 0; h < kMaxHeads; ++h) {
                if (h >= p.K) continue;   // (wave-uniform)
                const float pre = lrow[h] + rrow[h];
                const float ds = alpha_of(pre, p.slope, st[h], st[p.K + h]) * (dtile[lane * p.K + h] - delta[h]);
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
__global__ __launch_bounds__(kBlock) void attention_backward_rows_bf16_kernel(const P16 p) {
    __shared__ Shared<NB, false> sh;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        row_segment<L, NB, kWavesPerBlock>(p, sh, row, s, beg, end - beg, lane, wave);
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i)
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            if (end - beg >= p.geom.long_threshold) continue;   // a workgroup of its own
            row_segment<L, NB, 1>(p, sh, row0 + i, s, beg, end - beg, lane, wave);
        }
}

// ------------------------------------------------------------------------------------------------------------- column side
// attention_backward.hip's col_row on bf16 x and g, storing dx as TD -- rounded once, after the sum over the hops.
template <typename TD, int L, int NB, int NW>
__device__ __forceinline__ void col_row(const P16& p, Shared<NB, true>& sh, int64_t j, int lane, int wave) {
    const int q = lane & 15, gi = lane >> 4;
    const bf16_t* xrow = p.x + j * p.ldx;
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
    Quad dxq;                    // NW == 1: the running hop sum of the quad this lane stores
    float dxc0 = 0.f, dxc1 = 0.f;   // NW == 4: the running hop sums of the columns 2 threadIdx.x and 2 threadIdx.x + 1
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
                wave_lds_sync();   // the previous chunk's reads of the tiles come first
#pragma unroll
                for (int h = 0; h < kMaxHeads; ++h) {
                    if (h >= p.K) continue;   // (wave-uniform)
                    atile[lane * p.K + h] = alpha_of(lrow[h] + rrow[h], p.slope, st[h], st[p.K + h]);
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
                        const float ds = atile[lane * p.K + h] * (dtile[lane * p.K + h] - drow[h]);
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
            const int c = 2 * threadIdx.x;   // one PAIR of columns per thread: a bf16 pair is one dword
            if (c < NB * kBlockCols) {
                const float t0 = ((sh.tot[0][c] + sh.tot[1][c]) + sh.tot[2][c]) + sh.tot[3][c];
                const float t1 = ((sh.tot[0][c + 1] + sh.tot[1][c + 1]) + sh.tot[2][c + 1]) + sh.tot[3][c + 1];
                dxc0 = s == 0 ? t0 : dxc0 + t0;
                dxc1 = s == 0 ? t1 : dxc1 + t1;
            }
        }
        if (p.dr && (NW == 1 || wave == 0) && lane < p.K) p.dr[j * p.lddr + (int64_t)s * p.K + lane] = combine_sets(wtot, lane);
        if (NW > 1) __syncthreads();
    }
    if (!p.dx) return;
    TD* dxrow = static_cast<TD*>(p.dx) + j * p.lddx;
    if (NW == 1) {
        if (gi < NB) store_quad(dxrow, gi * kBlockCols + 4 * q, p.d, dxq);
    } else if (2 * (int)threadIdx.x < p.d) {   // (d is even)
        store_pair(dxrow, 2 * (int)threadIdx.x, dxc0, dxc1);
    }
}

template <typename TD, int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_cols_bf16_kernel(const P16 p) {
    __shared__ Shared<NB, true> sh;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x < p.geom.n_long) {   // a row that is long in any selected hop (the adjoint's list): all its hops
        col_row<TD, L, NB, kWavesPerBlock>(p, sh, p.geom.long_list[blockIdx.x], lane, wave);
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
        col_row<TD, L, NB, 1>(p, sh, row0 + i, lane, wave);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
template <int L, int NB>
static void launch_pair(const P16* rows, int64_t row_blocks, const P16* cols, int64_t col_blocks, bool dx16, hipStream_t stream) {
    if (rows) hipLaunchKernelGGL((attention_backward_rows_bf16_kernel<L, NB>), dim3((unsigned)row_blocks), dim3(kBlock), 0, stream, *rows);
    if (!cols) return;
    if (dx16) hipLaunchKernelGGL((attention_backward_cols_bf16_kernel<bf16_t, L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols);
    else hipLaunchKernelGGL((attention_backward_cols_bf16_kernel<float, L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols);
}

// The checks of attention_backward::run in its order, the layout rule of every bf16 array after the strides it speaks of.
static int run(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr, int32_t K, float slope,
               const uint16_t* X, int64_t ldx, int32_t d, const float* stats, int64_t ldstats, const uint16_t* Y, int64_t ldy_row,
               int64_t ldy_hop, const uint16_t* G, int64_t ldg_row, int64_t ldg_hop, float* delta, int64_t lddelta, float* dl, int64_t lddl,
               float* dr, int64_t lddr, int dx_dtype, void* dX, int64_t lddx, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v, tv;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_dtype("dx_dtype", dx_dtype)) != H2GCN_OK) return st;
        const bool dx16 = dx_dtype == H2GCN_DTYPE_BF16;
        if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
        if (K < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", K);
        if (K > kMaxHeads)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d > %d: the recomputing attention backward serves at most %d heads (run the chain)",
                        K, kMaxHeads, kMaxHeads);
        if (d % K) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d is not a multiple of n_heads = %d", d, K);
        if (K > 1 && (d / K) % 4)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "d / n_heads = %d is not a multiple of 4 (a lane's four columns must lie in one head)", d / K);
        if (d > kMaxBlocks * kBlockCols)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d > %d: the recomputing attention backward serves at most %d columns (run the chain)", d,
                        kMaxBlocks * kBlockCols, kMaxBlocks * kBlockCols);
        if (!dl && !dr && !dX) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dl, dr and dX are all NULL: nothing to compute");
        const bool col_side = dr || dX;
        const int64_t need = (int64_t)v.n_sel * K;
        if (ldl < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldl = %lld < H_sel * n_heads = %lld", (long long)ldl, (long long)need);
        if (ldr < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldr = %lld < H_sel * n_heads = %lld", (long long)ldr, (long long)need);
        if (ldstats < 2 * need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldstats = %lld < H_sel * 2 * n_heads = %lld", (long long)ldstats, (long long)(2 * need));
        if (ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ldx, d);
        if (ldy_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_row = %lld < d = %d", (long long)ldy_row, d);
        if (ldy_hop < 0 || (v.n_sel > 1 && ldy_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_hop = %lld < d = %d: the hops' outputs would overlap", (long long)ldy_hop, d);
        if (ldg_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_row = %lld < d = %d", (long long)ldg_row, d);
        if (ldg_hop < 0 || (v.n_sel > 1 && ldg_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_hop = %lld < d = %d: the hops' gradients would overlap", (long long)ldg_hop, d);
        if (delta && lddelta < need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddelta = %lld < H_sel * n_heads = %lld", (long long)lddelta, (long long)need);
        if (dl && lddl < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddl = %lld < H_sel * n_heads = %lld", (long long)lddl, (long long)need);
        if (dr && lddr < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddr = %lld < H_sel * n_heads = %lld", (long long)lddr, (long long)need);
        if (dX && lddx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddx = %lld < d = %d", (long long)lddx, d);
        if ((st = check_bf16_layout("X", X, ldx, 0, d)) != H2GCN_OK) return st;
        if ((st = check_bf16_layout("Y", Y, ldy_row, ldy_hop, d)) != H2GCN_OK) return st;
        if ((st = check_bf16_layout("G", G, ldg_row, ldg_hop, d)) != H2GCN_OK) return st;
        if (dX && dx16 && (st = check_bf16_layout("dX", dX, lddx, 0, d)) != H2GCN_OK) return st;
        if (col_side && !delta)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "delta is NULL: dr and dX need the [n_rows, H_sel, n_heads] buffer the row side fills");
        if (col_side && (st = adjoint_pattern_view(plan, hop_mask, &tv)) != H2GCN_OK) return st;
        if (selected_nnz(v) > 0) {
            const struct { const char* name; const void* ptr; } ins[] = {{"l", l}, {"r", r}, {"X", X}, {"stats", stats}, {"Y", Y}, {"G", G}};
            const struct { const char* name; const void* ptr; } outs[] = {{"delta", delta}, {"dl", dl}, {"dr", dr}, {"dX", dX}};
            for (const auto& in : ins)
                if (!in.ptr) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s is NULL", in.name);
            for (const auto& out : outs)
                for (const auto& in : ins)
                    if (out.ptr && out.ptr == in.ptr) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s aliases %s", out.name, in.name);
            for (int a = 0; a < 4; ++a)
                for (int b = a + 1; b < 4; ++b)
                    if (outs[a].ptr && outs[a].ptr == outs[b].ptr)
                        return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s aliases %s", outs[a].name, outs[b].name);
        }
        hipStream_t stream = (hipStream_t)stream_v;
        P16 rows, cols;
        memset(&rows, 0, sizeof(rows));
        int64_t row_blocks = 0, col_blocks = 0;
        if ((st = launch_geometry(plan, v, stream, &rows.geom, &row_blocks)) != H2GCN_OK) return st;
        rows.l = l, rows.r = r, rows.x = reinterpret_cast<const bf16_t*>(X), rows.stats = stats;
        rows.y = reinterpret_cast<const bf16_t*>(Y), rows.g = reinterpret_cast<const bf16_t*>(G);
        rows.delta = delta, rows.dl = dl, rows.dr = dr, rows.dx = dX;
        rows.ldl = ldl, rows.ldr = ldr, rows.ldx = ldx, rows.ldstats = ldstats, rows.ldy_row = ldy_row, rows.ldy_hop = ldy_hop;
        rows.ldg_row = ldg_row, rows.ldg_hop = ldg_hop, rows.lddelta = lddelta, rows.lddl = lddl, rows.lddr = lddr, rows.lddx = lddx;
        rows.d = d, rows.K = K, rows.w = d / K;
        rows.slope = slope;
        cols = rows;
        for (int s = 0; s < v.n_sel; ++s) rows.idx[s] = v.colidx[s];
        if (col_side) {
            memset(&cols.geom, 0, sizeof(cols.geom));
            if ((st = launch_geometry(plan, tv, stream, &cols.geom, &col_blocks, true)) != H2GCN_OK) return st;
            for (int s = 0; s < v.n_sel; ++s) cols.idx[s] = tv.colidx[s];
        }
        if (row_blocks == 0) {   // a selection without nonzeros: every sum is empty
            if ((st = zero_rows(delta, lddelta, need, v.n_rows, sizeof(float), stream)) != H2GCN_OK) return st;
            if ((st = zero_rows(dl, lddl, need, v.n_rows, sizeof(float), stream)) != H2GCN_OK) return st;
            if ((st = zero_rows(dr, lddr, need, v.n_cols, sizeof(float), stream)) != H2GCN_OK) return st;
            return zero_rows(dX, lddx, d, v.n_cols, dx16 ? sizeof(uint16_t) : sizeof(float), stream);
        }
        const P16* rp = &rows;
        const P16* cp = col_side && col_blocks > 0 ? &cols : nullptr;
        const int w = d / K;
        // (the geometries of the fp32 backward: the orders are functions of w and of the segment alone)
        if (K > 1 && d <= 2 * kBlockCols && w == 4) launch_pair<1, 2>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 8) launch_pair<2, 2>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 16) launch_pair<4, 2>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 32) launch_pair<8, 2>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else if (d <= kBlockCols) launch_pair<0, 1>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else if (d <= 2 * kBlockCols) launch_pair<0, 2>(rp, row_blocks, cp, col_blocks, dx16, stream);
        else launch_pair<0, kMaxBlocks>(rp, row_blocks, cp, col_blocks, dx16, stream);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads_backward_bf16");
    }
}

}  // namespace bwd
}  // namespace attention_bf16
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                    int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                    int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream) {
    return h2gcn::attention_bf16::fwd::run(false, nullptr, 0, plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d,
                                           y_dtype, Y_dev, ldy_row, ldy_hop, stream);
}

int h2gcn_attention_hops_heads_stats_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                          int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                          int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats,
                                          void* stream) {
    return h2gcn::attention_bf16::fwd::run(true, stats_dev, ldstats, plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev,
                                           ldx, d, y_dtype, Y_dev, ldy_row, ldy_hop, stream);
}

int h2gcn_attention_hops_heads_backward_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                             int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                             const float* stats_dev, int64_t ldstats, const uint16_t* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                                             const uint16_t* G_dev, int64_t ldg_row, int64_t ldg_hop, float* delta_dev, int64_t lddelta,
                                             float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, int dx_dtype, void* dX_dev, int64_t lddx,
                                             void* stream) {
    return h2gcn::attention_bf16::bwd::run(plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d, stats_dev, ldstats,
                                           Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev, lddl, dr_dev, lddr,
                                           dx_dtype, dX_dev, lddx, stream);
}

}  // extern "C"
