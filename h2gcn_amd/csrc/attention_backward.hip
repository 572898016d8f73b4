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
// l, m, 1/S, delta of row i, stores dr and dx.  Nothing of size nnz is read, written or allocated.  The two sides themselves
// (row_segment, col_row) are in attention_backward.hip.h, one text for this unit's kernels, the dropout pair and the bf16 pair; this
// unit has the fp32 kernels without dropout and the host launch path of all three entry points.
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
#include "attention_dropout.hip.h"

namespace h2gcn {
namespace attention_backward {

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_rows_kernel(const Params p) {
    __shared__ Shared<NB, false> sh;
    rows_walk<L, NB>(p, NoDropout{}, sh);
}

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_cols_kernel(const Params p) {
    __shared__ Shared<NB, true> sh;
    cols_walk<float, L, NB>(p, NoDropout{}, sh);
}

void launch_pair(const Params& rows, int64_t row_blocks, const Params* cols, int64_t col_blocks, hipStream_t stream) {
    for_geometry(rows.d, rows.K, [&](auto l, auto nb) {
        constexpr int L = decltype(l)::value, NB = decltype(nb)::value;
        hipLaunchKernelGGL((attention_backward_rows_kernel<L, NB>), dim3((unsigned)row_blocks), dim3(kBlock), 0, stream, rows);
        if (cols) hipLaunchKernelGGL((attention_backward_cols_kernel<L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols);
    });
}

// ------------------------------------------------------------------------------------------------------------ host
// What follows the checks: the geometries of the two sides, the parameter structs of the element type of x, the launch of the unit that
// has the kernels.
template <typename P>
static int launch(const Call& c, const PatternView& v, const PatternView& tv, bool col_side) {
    const int64_t need = (int64_t)v.n_sel * c.K;
    hipStream_t stream = (hipStream_t)c.stream;
    P rows, cols;
    memset(&rows, 0, sizeof(rows));
    int64_t row_blocks = 0, col_blocks = 0;
    int st = launch_geometry(c.plan, v, stream, &rows.geom, &row_blocks);
    if (st != H2GCN_OK) return st;
    rows.l = c.l, rows.r = c.r, rows.x = static_cast<decltype(rows.x)>(c.X), rows.stats = c.stats;
    rows.y = static_cast<decltype(rows.y)>(c.Y), rows.g = static_cast<decltype(rows.g)>(c.G);
    rows.delta = c.delta, rows.dl = c.dl, rows.dr = c.dr, rows.dx = static_cast<decltype(rows.dx)>(c.dX);
    rows.ldl = c.ldl, rows.ldr = c.ldr, rows.ldx = c.ldx, rows.ldstats = c.ldstats, rows.ldy_row = c.ldy_row, rows.ldy_hop = c.ldy_hop;
    rows.ldg_row = c.ldg_row, rows.ldg_hop = c.ldg_hop, rows.lddelta = c.lddelta, rows.lddl = c.lddl, rows.lddr = c.lddr, rows.lddx = c.lddx;
    rows.d = c.d, rows.K = c.K, rows.w = c.d / c.K;
    rows.slope = c.slope;
    cols = rows;
    for (int s = 0; s < v.n_sel; ++s) rows.idx[s] = v.colidx[s];
    if (col_side) {
        memset(&cols.geom, 0, sizeof(cols.geom));
        if ((st = launch_geometry(c.plan, tv, stream, &cols.geom, &col_blocks, true)) != H2GCN_OK) return st;
        for (int s = 0; s < v.n_sel; ++s) cols.idx[s] = tv.colidx[s];
    }
    if (row_blocks == 0) {   // a selection without nonzeros: every sum is empty
        if ((st = zero_rows(c.delta, c.lddelta, need, v.n_rows, sizeof(float), stream)) != H2GCN_OK) return st;
        if ((st = zero_rows(c.dl, c.lddl, need, v.n_rows, sizeof(float), stream)) != H2GCN_OK) return st;
        if ((st = zero_rows(c.dr, c.lddr, need, v.n_cols, sizeof(float), stream)) != H2GCN_OK) return st;
        return zero_rows(c.dX, c.lddx, c.d, v.n_cols, c.dx_dtype == H2GCN_DTYPE_BF16 ? sizeof(uint16_t) : sizeof(float), stream);
    }
    const P* cp = col_side && col_blocks > 0 ? &cols : nullptr;
    if constexpr (std::is_same<P, Params16>::value) {
        launch_pair_bf16(rows, row_blocks, cp, col_blocks, c.dx_dtype == H2GCN_DTYPE_BF16, stream);
    } else if (c.dropout) {   // (v: the forward view on both sides)
        launch_pair_dropout(rows, row_blocks, cp, col_blocks,
                            attention_dropout::make_args(c.plan, v.mask, v.n_cols, c.dropout->keep_prob, c.dropout->seed, c.dropout->step_dev),
                            stream);
    } else {
        launch_pair(rows, row_blocks, cp, col_blocks, stream);
    }
    H2GCN_HIP_TRY(hipGetLastError());
    return H2GCN_OK;
}

// The launch path of h2gcn_attention_hops_heads_backward{,_dropout}_f32 and h2gcn_attention_hops_heads_backward_bf16.  The checks of the
// bf16 entry point are the fp32 ones in their order, dX's element type first and the layout rule of every bf16 array after the strides
// it speaks of.
int run(const Call& c) {
    const bool x16 = c.x_dtype == H2GCN_DTYPE_BF16;
    try {
        // every check below comes before the device is touched
        const int32_t d = c.d, K = c.K;
        PatternView v, tv;
        int st = pattern_view(c.plan, c.hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (x16 && (st = check_dtype("dx_dtype", c.dx_dtype)) != H2GCN_OK) return st;
        const bool dx16 = c.dx_dtype == H2GCN_DTYPE_BF16;
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
        if (!c.dl && !c.dr && !c.dX) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dl, dr and dX are all NULL: nothing to compute");
        const bool col_side = c.dr || c.dX;
        const int64_t need = (int64_t)v.n_sel * K;
        if (c.ldl < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldl = %lld < H_sel * n_heads = %lld", (long long)c.ldl, (long long)need);
        if (c.ldr < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldr = %lld < H_sel * n_heads = %lld", (long long)c.ldr, (long long)need);
        if (c.ldstats < 2 * need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldstats = %lld < H_sel * 2 * n_heads = %lld", (long long)c.ldstats, (long long)(2 * need));
        if (c.ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)c.ldx, d);
        if (c.ldy_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_row = %lld < d = %d", (long long)c.ldy_row, d);
        if (c.ldy_hop < 0 || (v.n_sel > 1 && c.ldy_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_hop = %lld < d = %d: the hops' outputs would overlap", (long long)c.ldy_hop, d);
        if (c.ldg_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_row = %lld < d = %d", (long long)c.ldg_row, d);
        if (c.ldg_hop < 0 || (v.n_sel > 1 && c.ldg_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_hop = %lld < d = %d: the hops' gradients would overlap", (long long)c.ldg_hop, d);
        if (c.delta && c.lddelta < need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddelta = %lld < H_sel * n_heads = %lld", (long long)c.lddelta, (long long)need);
        if (c.dl && c.lddl < need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddl = %lld < H_sel * n_heads = %lld", (long long)c.lddl, (long long)need);
        if (c.dr && c.lddr < need)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddr = %lld < H_sel * n_heads = %lld", (long long)c.lddr, (long long)need);
        if (c.dX && c.lddx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddx = %lld < d = %d", (long long)c.lddx, d);
        if (x16) {
            if ((st = check_bf16_layout("X", c.X, c.ldx, 0, d)) != H2GCN_OK) return st;
            if ((st = check_bf16_layout("Y", c.Y, c.ldy_row, c.ldy_hop, d)) != H2GCN_OK) return st;
            if ((st = check_bf16_layout("G", c.G, c.ldg_row, c.ldg_hop, d)) != H2GCN_OK) return st;
        }
        if (c.dX && dx16 && (st = check_bf16_layout("dX", c.dX, c.lddx, 0, d)) != H2GCN_OK) return st;
        if (col_side && !c.delta)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "delta is NULL: dr and dX need the [n_rows, H_sel, n_heads] buffer the row side fills");
        if (col_side && (st = adjoint_pattern_view(c.plan, c.hop_mask, &tv)) != H2GCN_OK) return st;
        if (selected_nnz(v) > 0) {
            const struct { const char* name; const void* ptr; } ins[] = {{"l", c.l}, {"r", c.r}, {"X", c.X}, {"stats", c.stats}, {"Y", c.Y}, {"G", c.G}};
            const struct { const char* name; const void* ptr; } outs[] = {{"delta", c.delta}, {"dl", c.dl}, {"dr", c.dr}, {"dX", c.dX}};
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
        return x16 ? launch<Params16>(c, v, tv, col_side) : launch<Params>(c, v, tv, col_side);
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads_backward_%s", x16 ? "bf16" : "f32");
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
    return h2gcn::attention_backward::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_F32, X_dev, ldx, d,
                                           stats_dev, ldstats, Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev,
                                           lddl, dr_dev, lddr, H2GCN_DTYPE_F32, dX_dev, lddx, nullptr, stream});
}

}  // extern "C"
