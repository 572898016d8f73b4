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
// would gather l, m and 1/S of every entry a second time.  The passes, the geometry and every summation order are those of
// attention_backward.hip: the kernels below wrap its row_segment / col_row (attention_backward.hip.h) with the dropout policy `Dropped`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_backward.hip.h"
#include "attention_dropout.hip.h"

namespace h2gcn {
namespace attention_dropout {

using namespace attention_backward;

// The dropout policy of row_segment / col_row: the mask, the plan's hop index of every selected hop, and (column side) the wave's tile
// of undropped coefficients.
struct Dropped {
    static constexpr bool kOn = true;
    Mask mk;
    const int32_t* hop;
    float* undropped;
    __device__ __forceinline__ uint32_t kept(int64_t i, int64_t j, int s, int K) const { return kept_heads(mk, entry_base(mk, i, j, hop[s]), K); }
    __device__ __forceinline__ float factor(uint32_t keep, int h) const { return (keep >> h) & 1u ? mk.inv_keep : 0.f; }
};

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void attention_backward_rows_dropout_kernel(const Params p, const Args da) {
    __shared__ Shared<NB, false> sh;
    rows_walk<L, NB>(p, Dropped{make_mask(da), da.hop, nullptr}, sh);
}

template <int L, int NB>
// (three waves per SIMD are asked for -- the column side's occupancy without dropout: left alone one form took scratch)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void attention_backward_cols_dropout_kernel(const Params p,
                                                                                                                   const Args da) {
    __shared__ Shared<NB, true> sh;
    __shared__ float undropped[kWavesPerBlock][kWave * kMaxHeads];   // per wave: alpha of the chunk at hand before the factor (lane = entry)
    cols_walk<float, L, NB>(p, Dropped{make_mask(da), da.hop, undropped[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]}, sh);
}

}  // namespace attention_dropout

void attention_backward::launch_pair_dropout(const Params& rows, int64_t row_blocks, const Params* cols, int64_t col_blocks,
                                             const attention_dropout::Args& da, hipStream_t stream) {
    using namespace attention_dropout;
    for_geometry(rows.d, rows.K, [&](auto l, auto nb) {
        constexpr int L = decltype(l)::value, NB = decltype(nb)::value;
        hipLaunchKernelGGL((attention_backward_rows_dropout_kernel<L, NB>), dim3((unsigned)row_blocks), dim3(kBlock), 0, stream, rows, da);
        if (cols)
            hipLaunchKernelGGL((attention_backward_cols_dropout_kernel<L, NB>), dim3((unsigned)col_blocks), dim3(kBlock), 0, stream, *cols, da);
    });
}

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
    // keep_prob = 1: nothing is dropped and 1/keep = 1 -- the launches without dropout, their bits
    const h2gcn::attention_dropout::Draw dropout = {keep_prob, seed, step_dev};
    return h2gcn::attention_backward::run({plan, hop_mask, l_dev, ldl, r_dev, ldr, n_heads, negative_slope, H2GCN_DTYPE_F32, X_dev, ldx, d,
                                           stats_dev, ldstats, Y_dev, ldy_row, ldy_hop, G_dev, ldg_row, ldg_hop, delta_dev, lddelta, dl_dev,
                                           lddl, dr_dev, lddr, H2GCN_DTYPE_F32, dX_dev, lddx, keep_prob == 1.f ? nullptr : &dropout, stream});
}

}  // extern "C"
