// attention_backward.hip -- the backward of the attention chain WITHOUT its per-entry arrays: every per-entry quantity is computed
// again from node quantities and the softmax statistics (m, 1/S) that h2gcn_attention_hops_heads_stats_f32 stored,
//
//     pre = l[i,s,h] + r[j,s,h]      alpha[e,h]  = exp(leaky(pre) - m[i,s,h]) * rinv[i,s,h]
//     dalpha[e,h] = sum_{c in head h} g[i,s,c] * x[j,c]          delta[i,s,h] = sum_{c in head h} g[i,s,c] * y[i,s,c]
//     dscore = alpha * (dalpha - delta)                          dpre = pre > 0 ? dscore : dscore * slope
//     dl[i,s,h] = sum over row i of dpre      dr[j,s,h] = sum over column j of dpre      dx[j,c] = sum_s sum over column j of alpha * g[i,s,c]
//
// in two gather-bound launches: the ROW side walks A_s, gathers x[j] and r[j,s], stores delta and dl; the COLUMN side walks A_s^T
// (t_rowptr / t_colidx only: there is no per-entry array to index, so no permutation), gathers g[i,s] and the 4 K node floats
// l, m, 1/S, delta of row i, stores dr and dx.  Nothing of size nnz is read, written or allocated.  A translation unit of its own: no
// existing kernel is compiled differently because of it.
//
// Mapping (gfx950, wave64; the pattern walk of pattern_walk.hip.h; no atomics, no scratch, no workspace):
//   * a segment is walked in 64-entry chunks; chunk t of a segment belongs to SET t mod 4.  A wave of the tile walk serves the four
//     sets one after the other, the workgroup of a long segment / long row gives set w to wave w: the same additions either way, so
//     the bits do not depend on long_row_threshold or rows_per_wave;
//   * per chunk the gather runs in the geometry of sddmm.hip -- 16 lanes x 4 columns per 64-column block, lane group gi the entries
//     = gi (mod 4) -- and leaves dalpha of the chunk in a 64 x K LDS tile (entry-major); the column side adds alpha * g to its dx
//     accumulators from the SAME loads (alpha from a second tile, written lane = entry before the gather);
//   * then lane = entry: alpha, dscore, dpre per head, added to the lane's partial of the set;
//   * head widths 4, 8, 16, 32 with d <= 128 (PACKED): one full-width gather of a row serves all heads, the butterfly stops at the
//     head; any other width: head-aligned blocks, one head after the other (and the column side gathers the row once more for dx).
// The summation orders are in include/h2gcn_hip.h.
#include "attention_backward.hip.h"

namespace h2gcn {
namespace attention_backward {

// ---------------------------------------------------------------------------------------------------------------- row side
// Segment (row, s) = entries [beg, beg + len) on NW waves (1: the calling wave, the sets in turn; 4: every thread of the block must
// call, wave w = set w).  Stores delta[row, s, :] and, if wanted, dl[row, s, :].
template <int L, int NB, int NW>
__device__ __forceinline__ void row_segment(const Params& p, Shared<NB, false>& sh, int64_t row, int s, int64_t beg, int64_t len, int lane, int wave) {
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
__global__ __launch_bounds__(kBlock) void attention_backward_rows_kernel(const Params p) {
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
// Column j of the forward operands = row j of every selected A_s^T, on NW waves (as row_segment).  Stores dr[j, :, :] and dx[j, :]
// where wanted.
template <int L, int NB, int NW>
__device__ __forceinline__ void col_row(const Params& p, Shared<NB, true>& sh, int64_t j, int lane, int wave) {
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
__global__ __launch_bounds__(kBlock) void attention_backward_cols_kernel(const Params p) {
    __shared__ Shared<NB, true> sh;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((int)blockIdx.x < p.geom.n_long) {   // a row that is long in any selected hop (the adjoint's list): all its hops
        col_row<L, NB, kWavesPerBlock>(p, sh, p.geom.long_list[blockIdx.x], lane, wave);
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
        col_row<L, NB, 1>(p, sh, row0 + i, lane, wave);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
template <int L, int NB>
void launch_pair(const Params* rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, hipStream_t stream) {
    if (rows) hipLaunchKernelGGL((attention_backward_rows_kernel<L, NB>), dim3((unsigned)row_blocks), dim3(kBlock), 0, stream, *rows);
    if (cols) hipLaunchKernelGGL((attention_backward_cols_kernel<L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols);
}

int zero_rows(float* out, int64_t ld, int64_t width, int64_t n, hipStream_t stream) {
    if (out && n > 0 && width > 0)
        H2GCN_HIP_TRY(hipMemset2DAsync(out, (size_t)ld * sizeof(float), 0, (size_t)width * sizeof(float), (size_t)n, stream));
    return H2GCN_OK;
}

int run(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l, int64_t ldl, const float* r, int64_t ldr, int32_t K, float slope,
        const float* X, int64_t ldx, int32_t d, const float* stats, int64_t ldstats, const float* Y, int64_t ldy_row, int64_t ldy_hop,
        const float* G, int64_t ldg_row, int64_t ldg_hop, float* delta, int64_t lddelta, float* dl, int64_t lddl, float* dr, int64_t lddr,
        float* dX, int64_t lddx, void* stream_v, PairLauncher pair, const void* ctx) {
    try {
        // every check below comes before the device is touched
        PatternView v, tv;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
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
        if (col_side && !delta)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "delta is NULL: dr and dX need the [n_rows, H_sel, n_heads] buffer the row side fills");
        if (col_side && (st = adjoint_pattern_view(plan, hop_mask, &tv)) != H2GCN_OK) return st;
        if (selected_nnz(v) > 0) {
            const struct { const char* name; const float* ptr; } ins[] = {{"l", l}, {"r", r}, {"X", X}, {"stats", stats}, {"Y", Y}, {"G", G}};
            const struct { const char* name; const float* ptr; } outs[] = {{"delta", delta}, {"dl", dl}, {"dr", dr}, {"dX", dX}};
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
        Params rows, cols;
        memset(&rows, 0, sizeof(rows));
        int64_t row_blocks = 0, col_blocks = 0;
        if ((st = launch_geometry(plan, v, stream, &rows.geom, &row_blocks)) != H2GCN_OK) return st;
        rows.l = l, rows.r = r, rows.x = X, rows.stats = stats, rows.y = Y, rows.g = G;
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
            if ((st = zero_rows(delta, lddelta, need, v.n_rows, stream)) != H2GCN_OK) return st;
            if ((st = zero_rows(dl, lddl, need, v.n_rows, stream)) != H2GCN_OK) return st;
            if ((st = zero_rows(dr, lddr, need, v.n_cols, stream)) != H2GCN_OK) return st;
            return zero_rows(dX, lddx, d, v.n_cols, stream);
        }
        const Params* rp = &rows;
        const Params* cp = col_side && col_blocks > 0 ? &cols : nullptr;
        const int w = d / K;
        // (the bits do not depend on the geometry: the orders are functions of w and of the segment alone)
        const bool packed = K > 1 && d <= 2 * kBlockCols && (w == 4 || w == 8 || w == 16 || w == 32);
        if (pair)
            pair(packed ? w / 4 : 0, packed ? 2 : (d <= kBlockCols ? 1 : (d <= 2 * kBlockCols ? 2 : kMaxBlocks)), rp, row_blocks, cp, col_blocks, v,
                 ctx, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 4) launch_pair<1, 2>(rp, row_blocks, cp, col_blocks, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 8) launch_pair<2, 2>(rp, row_blocks, cp, col_blocks, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 16) launch_pair<4, 2>(rp, row_blocks, cp, col_blocks, stream);
        else if (K > 1 && d <= 2 * kBlockCols && w == 32) launch_pair<8, 2>(rp, row_blocks, cp, col_blocks, stream);
        else if (d <= kBlockCols) launch_pair<0, 1>(rp, row_blocks, cp, col_blocks, stream);
        else if (d <= 2 * kBlockCols) launch_pair<0, 2>(rp, row_blocks, cp, col_blocks, stream);
        else launch_pair<0, kMaxBlocks>(rp, row_blocks, cp, col_blocks, stream);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads_backward_f32");
    }
}

}  // namespace attention_backward
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_backward_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                            int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                            const float* stats_dev, int64_t ldstats, const float* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                                            const float* G_dev, int64_t ldg_row, int64_t ldg_hop, float* delta_dev, int64_t lddelta,
                                            float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, float* dX_dev, int64_t lddx,
                                            void* stream) {
    return h2gcn::attention_backward::run(plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, X_dev, ldx, d, stats_dev, ldstats,
                                          Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev, lddl, dr_dev, lddr,
                                          dX_dev, lddx, stream);
}

}  // extern "C"
