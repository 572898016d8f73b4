// classifier.hip -- the classifier side of an H2GCN training step as hand-written gfx950 kernels on the fp32 matrix cores:
//
//     Z = (X .* M / keep) @ W + b          (forward)          X: [N, K] concat buffer, K = 7 * hidden (448), W: [K, C], C <= 64
//     dX = (G @ W^T) .* M / keep           (backward, data)   G: [N, C]
//     dW = (X .* M / keep)^T @ G           (backward, weights)
//
// Reference: keras `Dropout(rate)` followed by the output `Dense` -- `D0.5-MO` of the network-setup DSL (reference
// h2gcn/models/H2GCN.py:235-257 builds the two layers, :308-325 calls them in order; SURVEY.md 8(f) rank 2/3: "the final
// dense classifier", "training loop on device").  With stock kernels this is five passes over the 4.3 GB buffer of the
// products shape (dropout forward, skinny GEMM, two backward GEMMs, dropout backward: ~15 of a 68 ms step, the GEMMs at
// 1.1-1.9 TB/s because C = 47 outputs starve a general GEMM tile).  Here every pass streams X (or writes dX) ONCE:
//   * the dropout mask is a COUNTER-BASED function of (seed, step, row, column) -- one keyed round of a 32-bit avalanche hash
//     per group of four elements -- recomputed wherever it is needed instead of stored or applied in a pass of its own;
//   * the products run on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain), C padded to 16-column tiles (47 -> 48),
//     W staged through LDS in 64-row chunks whose layout makes the B-fragment reads conflict-free;
//   * dW is accumulated per workgroup in registers over a contiguous row range and reduced in fixed order (deterministic).
// Where the time goes (products shape, measured by knocking parts out -- tools/classifier_kernels.py): the fp32
// matrix pipe alone needs 0.84 ms per pass at the clock the chip holds under this load (50.4 M MFMAs x 32 cycles over 1024
// SIMDs at ~1.9-2.1 GHz; SQ_VALU_MFMA_BUSY_CYCLES confirms the count), the X stream alone 0.86 ms (5 TB/s); the mask VALU work
// shares the issue port with the MFMAs (+0.1-0.3 ms); the two do not overlap perfectly at 3-4 waves per SIMD:
// 1.44 / 1.60 / 1.33 ms (forward / dX / dW) = 0.58 / 0.52 / 0.63 of the matrix-pipe floor, 3.0 / 2.7 / 3.2 TB/s of X.
// The kernels and their launch code live in classifier_kernels.hip.h, templates over the element types of X and dX: this unit
// holds the fp32 instantiations (and the process-wide tunables), classifier_bf16.hip the bf16 ones.
#include "classifier_kernels.hip.h"

namespace {
int64_t g_small_rows = 12288;   // operands of at most this many rows (and C <= kSmallCP, K <= kSmallMaxK) take the small kernels; 0 = never
                                // (measured crossover at K = 448, C = 7: 8 192 rows 16 / 14 us small vs 19 / 19 matrix-core, 16 384 rows 27 / 22 vs
                                //  20 / 19, 32 768 rows 51 / 47 vs 23 / 22 -- profiles/r04_cora_epoch_kernels.txt)
}  // namespace

extern "C" {

int64_t h2gcn_dropout_dense_small_rows(int64_t rows) {
    const int64_t old = g_small_rows;
    if (rows >= 0) g_small_rows = rows;
    return old;
}

size_t h2gcn_dropout_dense_workspace_bytes(int64_t n_rows, int32_t k, int32_t c) {
    if (n_rows < 0 || k < 1 || c < 1 || c > 64) return 0;
    return shape_of(n_rows, k, c).total;
}

int h2gcn_dropout_dense_f32(const float* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* bias,
                            float keep_prob, uint64_t seed, const int64_t* step_dev, float* Y, int64_t ldy, void* workspace,
                            size_t workspace_bytes, void* stream_v) {
    return dropout_dense_forward<float>(X, ldx, n_rows, K, W, C, bias, keep_prob, seed, step_dev, Y, ldy, workspace, workspace_bytes, stream_v);
}

int h2gcn_dropout_dense_backward_f32(const float* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* G,
                                     int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev, float* dX, int64_t lddx,
                                     float* dW, void* workspace, size_t workspace_bytes, void* stream_v) {
    return dropout_dense_backward<float, float>(X, ldx, n_rows, K, W, C, G, ldg, keep_prob, seed, step_dev, dX, lddx, dW, workspace,
                                                workspace_bytes, stream_v);
}

}  // extern "C"
