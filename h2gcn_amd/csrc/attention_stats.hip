// attention_stats.hip -- h2gcn_attention_hops_heads_stats_f32: the fused attention forward of attention_fused.hip that ALSO STORES
// the softmax statistics (m, 1/S) of every (row, hop, head) -- stats[i, s, 0, h] = m, stats[i, s, 1, h] = 1/S, what the recomputing
// backward (attention_backward.hip) needs to form alpha again per entry.  The values are the ones the walk holds anyway, in
// Shared::stat or in registers on the single-chunk and short paths; Y is bit for bit attention_fused_kernel's: the walk, the device
// functions (attention_fused.hip.h) and every operation on the way to Y are the same.  An empty segment stores (+0, +0).
//
// The kernel is the one walk of attention_fused.hip.h with its STATS flag set.  It is a kernel and a translation unit of its own so that
// the forward that needs no gradient carries no statistics pointer and no store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_fused.hip.h"

namespace h2gcn {
namespace attention_fused {

// attention_fused_kernel, storing the softmax statistics of every (row, hop, head) as well -- values the walk holds anyway.
template <int NB>
__global__ __launch_bounds__(kBlock) void attention_fused_stats_kernel(const Params p, float* stats, int64_t ldstats) {
    __shared__ Shared<NB> sh;
    forward_walk<float, NB, true>(p, sh, stats, ldstats);
}

void launch_stats(const Params& p, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream) {
    for_blocks(p.d, [&](auto nb) {
        hipLaunchKernelGGL((attention_fused_stats_kernel<decltype(nb)::value>), grid, dim3(kBlock), 0, stream, p, stats, ldstats);
    });
}

}  // namespace attention_fused
}  // namespace h2gcn

extern "C" {

int h2gcn_attention_hops_heads_stats_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                         int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                         float* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats, void* stream) {
    return h2gcn::attention_fused::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_F32, X_dev, ldx, d,
                                        H2GCN_DTYPE_F32, Y_dev, ldy_row, ldy_hop, true, stats_dev, ldstats, nullptr, stream});
}

}  // extern "C"
