// attention_bf16.hip -- the three launches of the recomputing hop attention on bf16 embeddings:
//
//     h2gcn_attention_hops_heads_bf16            attention_fused.hip's forward,            X bf16, Y bf16 or fp32
//     h2gcn_attention_hops_heads_stats_bf16      attention_stats.hip's forward + (m, 1/S), X bf16, Y bf16 or fp32
//     h2gcn_attention_hops_heads_backward_bf16   attention_backward.hip's two sides,       X, Y, G bf16, dX bf16 or fp32
//
// The contract is the bf16 SpMM's: every gathered bf16 element is WIDENED EXACTLY (a shift or a mask), every operation of the fp32
// kernel runs in fp32 in the documented order, and an output is rounded ONCE, to nearest even, where it is stored.  So an fp32 output
// has the bits of the fp32 launch on the upcast operands and a bf16 output is that value rounded; l, r, stats, delta, dl and dr -- K
// wide, not d wide -- stay fp32.  The kernels below wrap the ONE forward walk (attention_fused.hip.h) and the ONE row_segment / col_row
// (attention_backward.hip.h) of the fp32 units, instantiated on the element types of the wide operands; walk A, which reads l and r
// only, is the same code.  What the element types change in them:
//   * a bf16 quad is ONE 8-byte load (4, 2 or 0 valid columns: d is even) that stays packed until the FMA / dot product that
//     consumes it.  The backward's batches keep 16 of them in flight instead of 8 -- the same 8 KiB per wave, the registers of the
//     fp32 batch; the forward keeps 8: with 16 its batch also holds the coefficients and row addresses of twice the rounds, which
//     cost it half its occupancy and were measured slower (Loads in attention_fused.hip.h);
//   * Y and dX are packed with v_cvt_pk_bf16_f32 and stored as dwords.  The two epilogues that write one column per thread in the
//     fp32 kernels (a long segment's Y, a long column's dX) write one PAIR of columns per thread here, so that no 2-byte store has a
//     neighbour to race with;
//   * dX is rounded after the sum over the hops.
// The host launch paths are the fp32 units' too (attention_fused::run, attention_backward::run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_backward.hip.h"
#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_bf16 {

using namespace pattern;

// ================================================================================================================ forward
namespace fwd {

using namespace attention_fused;
using P16 = Params16;

// attention_fused_kernel / attention_fused_stats_kernel (STATS) on a bf16 X, storing TY.
template <typename TY, int NB, bool STATS>
__global__ __launch_bounds__(kBlock) void attention_bf16_kernel(const P16 p, float* stats, int64_t ldstats) {
    __shared__ Shared<NB> sh;
    forward_walk<TY, NB, STATS>(p, sh, stats, ldstats);
}

template <typename TY, bool STATS>
static void launch(const P16& p, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream) {
    for_blocks(p.d, [&](auto nb) {
        hipLaunchKernelGGL((attention_bf16_kernel<TY, decltype(nb)::value, STATS>), grid, dim3(kBlock), 0, stream, p, stats, ldstats);
    });
}

}  // namespace fwd

// =============================================================================================================== backward
namespace bwd {

using namespace attention_backward;
using P16 = Params16;

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_rows_bf16_kernel(const P16 p) {
    __shared__ Shared<NB, false> sh;
    rows_walk<L, NB>(p, NoDropout{}, sh);
}

template <typename TD, int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_cols_bf16_kernel(const P16 p) {
    __shared__ Shared<NB, true> sh;
    cols_walk<TD, L, NB>(p, NoDropout{}, sh);
}

}  // namespace bwd
}  // namespace attention_bf16

void attention_fused::launch_bf16(const Params16& p, bool y16, bool with_stats, float* stats, int64_t ldstats, dim3 grid,
                                  hipStream_t stream) {
    using namespace attention_bf16::fwd;
    if (with_stats) (y16 ? launch<bf16_t, true> : launch<float, true>)(p, stats, ldstats, grid, stream);
    else (y16 ? launch<bf16_t, false> : launch<float, false>)(p, nullptr, 0, grid, stream);
}

void attention_backward::launch_pair_bf16(const Params16& rows, int64_t row_blocks, const Params16* cols, int64_t col_blocks, bool dx16,
                                          hipStream_t stream) {
    using namespace attention_bf16::bwd;
    for_geometry(rows.d, rows.K, [&](auto l, auto nb) {
        constexpr int L = decltype(l)::value, NB = decltype(nb)::value;
        const dim3 grid((unsigned)col_blocks), block(kBlock);
        hipLaunchKernelGGL((attention_backward_rows_bf16_kernel<L, NB>), dim3((unsigned)row_blocks), block, 0, stream, rows);
        if (!cols) return;
        if (dx16) hipLaunchKernelGGL((attention_backward_cols_bf16_kernel<bf16_t, L, NB>), grid, block, 0, stream, *cols);
        else hipLaunchKernelGGL((attention_backward_cols_bf16_kernel<float, L, NB>), grid, block, 0, stream, *cols);
    });
}

}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                    int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                    int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream) {
    return h2gcn::attention_fused::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_BF16, X_dev, ldx, d,
                                        y_dtype, Y_dev, ldy_row, ldy_hop, false, nullptr, 0, nullptr, stream});
}

int h2gcn_attention_hops_heads_stats_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                          int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                          int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats,
                                          void* stream) {
    return h2gcn::attention_fused::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_BF16, X_dev, ldx, d,
                                        y_dtype, Y_dev, ldy_row, ldy_hop, true, stats_dev, ldstats, nullptr, stream});
}

int h2gcn_attention_hops_heads_backward_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                             int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                             const float* stats_dev, int64_t ldstats, const uint16_t* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                                             const uint16_t* G_dev, int64_t ldg_row, int64_t ldg_hop, float* delta_dev, int64_t lddelta,
                                             float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, int dx_dtype, void* dX_dev, int64_t lddx,
                                             void* stream) {
    return h2gcn::attention_backward::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_BF16, X_dev, ldx, d,
                                           stats_dev, ldstats, Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev,
                                           lddl, dr_dev, lddr, dx_dtype, dX_dev, lddx, nullptr, stream});
}

}  // extern "C"
