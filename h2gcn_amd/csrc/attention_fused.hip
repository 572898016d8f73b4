// attention_fused.hip -- the forward of the attention chain in ONE launch, for every forward that needs no gradient:
//
//     Y[i, s, c] = sum_e alpha_s[e, h(c)] * X[j_e, c]          e over row i of selected hop s, h(c) = c / (d / K)
//     alpha_s[., h] = softmax over the segment of leaky(l[i, s, h] + r[j_e, s, h])
//
// what h2gcn_edge_scores_hops_heads_f32 -> h2gcn_row_softmax_hops_heads_f32 -> h2gcn_spmm_hops_values_f32 compute through two
// entry-major [nnz_k, K] arrays, BIT FOR BIT, without those arrays: nothing of size nnz is written or allocated, the only store
// is Y.  The walk itself is `forward_walk` in attention_fused.hip.h, one text for this unit's kernel and for the kernels that also
// store the softmax statistics (attention_stats.hip) or read a bf16 X (attention_bf16.hip); attention_dropout.hip keeps a copy;
// this unit has the plain fp32 kernel and the host launch path of all five forward entry points.
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

#include "attention_dropout.hip.h"
#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_fused {

template <int NB>
__global__ __launch_bounds__(kBlock) void attention_fused_kernel(const Params p) {
    __shared__ Shared<NB> sh;
    forward_walk<float, NB, false>(p, sh, nullptr, 0);
}

void launch_forward(const Params& p, dim3 grid, hipStream_t stream) {
    for_blocks(p.d, [&](auto nb) { hipLaunchKernelGGL((attention_fused_kernel<decltype(nb)::value>), grid, dim3(kBlock), 0, stream, p); });
}

// ------------------------------------------------------------------------------------------------------------ host
// What follows the checks: the geometry, the parameter struct of the element type of x, the launch of the unit that has the kernel.
template <typename P>
static int launch(const Call& c, const PatternView& v) {
    const bool y16 = c.y_dtype == H2GCN_DTYPE_BF16;
    const int64_t need = (int64_t)v.n_sel * c.n_heads;
    hipStream_t stream = (hipStream_t)c.stream;
    P p;
    memset(&p, 0, sizeof(p));
    int64_t n_blocks;
    int st = launch_geometry(c.plan, v, stream, &p.geom, &n_blocks);
    if (st != H2GCN_OK) return st;
    if (n_blocks == 0) {   // a selection without nonzeros: every row is empty
        const size_t elem = y16 ? sizeof(uint16_t) : sizeof(float);
        for (int s = 0; s < v.n_sel; ++s)
            if ((st = zero_rows((char*)c.Y + (size_t)s * (size_t)c.ldy_hop * elem, c.ldy_row, c.d, v.n_rows, elem, stream)) != H2GCN_OK) return st;
        if (c.with_stats) return zero_rows(c.stats, c.ldstats, 2 * need, v.n_rows, sizeof(float), stream);   // every segment: (+0, +0)
        return H2GCN_OK;
    }
    for (int s = 0; s < v.n_sel; ++s) p.colidx[s] = v.colidx[s];
    p.l = c.l, p.ldl = c.ldl;
    p.r = c.r, p.ldr = c.ldr;
    p.x = static_cast<decltype(p.x)>(c.X), p.ldx = c.ldx;
    p.y = static_cast<decltype(p.y)>(c.Y), p.ldy_row = c.ldy_row, p.ldy_hop = c.ldy_hop;
    p.d = c.d, p.K = c.n_heads, p.head_cols = c.d / c.n_heads;
    p.slope = c.slope;
    const dim3 grid((unsigned)n_blocks);
    if constexpr (std::is_same<P, Params16>::value) {
        launch_bf16(p, y16, c.with_stats, c.stats, c.ldstats, grid, stream);
    } else if (c.dropout) {
        launch_stats_dropout(p, c.stats, c.ldstats,
                             attention_dropout::make_args(c.plan, v.mask, v.n_cols, c.dropout->keep_prob, c.dropout->seed, c.dropout->step_dev),
                             grid, stream);
    } else if (c.with_stats) {
        launch_stats(p, c.stats, c.ldstats, grid, stream);
    } else {
        launch_forward(p, grid, stream);
    }
    H2GCN_HIP_TRY(hipGetLastError());
    return H2GCN_OK;
}

// The launch path of h2gcn_attention_hops_heads{,_stats,_stats_dropout}_f32 and h2gcn_attention_hops_heads{,_stats}_bf16.  The checks
// of a bf16 entry point are the fp32 ones in their order, the output's element type first and the layout rule of every bf16 array
// after the strides it speaks of.
int run(const Call& c) {
    const bool x16 = c.x_dtype == H2GCN_DTYPE_BF16;
    try {
        // every check below comes before the device is touched
        const int32_t d = c.d, n_heads = c.n_heads;
        PatternView v;
        int st = pattern_view(c.plan, c.hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (x16 && (st = check_dtype("y_dtype", c.y_dtype)) != H2GCN_OK) return st;
        const bool y16 = c.y_dtype == H2GCN_DTYPE_BF16;
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
        if (c.ldl < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldl = %lld < H_sel * n_heads = %lld", (long long)c.ldl, (long long)need);
        if (c.ldr < need) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldr = %lld < H_sel * n_heads = %lld", (long long)c.ldr, (long long)need);
        if (c.ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)c.ldx, d);
        if (c.ldy_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_row = %lld < d = %d", (long long)c.ldy_row, d);
        if (c.ldy_hop < 0 || (v.n_sel > 1 && c.ldy_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_hop = %lld < d = %d: hop outputs would overlap", (long long)c.ldy_hop, d);
        if (x16 && (st = check_bf16_layout("X", c.X, c.ldx, 0, d)) != H2GCN_OK) return st;
        if (y16 && (st = check_bf16_layout("Y", c.Y, c.ldy_row, c.ldy_hop, d)) != H2GCN_OK) return st;
        if (v.n_rows == 0) return H2GCN_OK;   // nothing to store
        if (!c.Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y is NULL");
        if (selected_nnz(v) > 0 && !c.l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "l is NULL");
        if (selected_nnz(v) > 0 && !c.r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "r is NULL");
        if (selected_nnz(v) > 0 && !c.X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "X is NULL");
        if (c.Y == c.X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases X");
        if (c.Y == (const void*)c.l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases l");
        if (c.Y == (const void*)c.r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "Y aliases r");
        if (c.with_stats) {
            if (c.ldstats < 2 * need)
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldstats = %lld < H_sel * 2 * n_heads = %lld", (long long)c.ldstats,
                            (long long)(2 * need));
            if (!c.stats) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats is NULL");
            if ((void*)c.stats == c.Y) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases Y");
            if ((const void*)c.stats == c.X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases X");
            if (c.stats == c.l) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases l");
            if (c.stats == c.r) return fail(H2GCN_ERR_INVALID_ARGUMENT, "stats aliases r");
        }
        return x16 ? launch<Params16>(c, v) : launch<Params>(c, v);
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in attention_hops_heads%s%s_%s", c.with_stats ? "_stats" : "",
                    c.dropout ? "_dropout" : "", x16 ? "bf16" : "f32");
    }
}

}  // namespace attention_fused
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                   int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                   float* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream) {
    return h2gcn::attention_fused::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_F32, X_dev, ldx, d,
                                        H2GCN_DTYPE_F32, Y_dev, ldy_row, ldy_hop, false, nullptr, 0, nullptr, stream});
}

}  // extern "C"
