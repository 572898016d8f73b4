// classifier_bf16.hip -- the bf16-X instantiations of the classifier kernels (classifier_kernels.hip.h: TX = bf16, TD = bf16 or
// float) behind h2gcn_dropout_dense_bf16 / h2gcn_dropout_dense_backward_bf16.  A translation unit of its own, like
// spmm_bf16.hip: the fp32 instantiations in classifier.hip must keep their registers and occupancy.  Same kernels, same
// arithmetic: a lane's fragment of X is one 8-byte load of four bf16 widened exactly to fp32, the products run on
// v_mfma_f32_16x16x4_f32 with fp32 W and G, a bf16 dX is the finished fp32 value (after mask and scale) rounded to nearest even
// and written with one 8-byte store per lane and row tile.  So Z and dW are bit-identical to the _f32 entry points called on the
// upcast X, an fp32 dX too, and a bf16 dX is that value's .to(bfloat16).
#include "classifier_kernels.hip.h"

extern "C" {

int h2gcn_dropout_dense_bf16(const uint16_t* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* bias,
                             float keep_prob, uint64_t seed, const int64_t* step_dev, float* Z, int64_t ldz, void* workspace,
                             size_t workspace_bytes, void* stream_v) {
    const char* fn = "dropout_dense_bf16";
    if (!X && n_rows > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: X_dev is NULL", fn);
    if (!W) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: W_dev is NULL", fn);
    if (!Z && n_rows > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: Z_dev is NULL", fn);
    int st = check_bf16_array(fn, "X_dev", X, "ldx", ldx);
    if (st != H2GCN_OK) return st;
    return dropout_dense_forward(reinterpret_cast<const bf16*>(X), ldx, n_rows, K, W, C, bias, keep_prob, seed, step_dev, Z, ldz, workspace,
                                 workspace_bytes, stream_v);
}

int h2gcn_dropout_dense_backward_bf16(const uint16_t* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* G,
                                      int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev, int dx_dtype, void* dX,
                                      int64_t lddx, float* dW, void* workspace, size_t workspace_bytes, void* stream_v) {
    const char* fn = "dropout_dense_backward_bf16";
    if (!X && n_rows > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: X_dev is NULL", fn);
    if (!W) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: W_dev is NULL", fn);
    if (!G && n_rows > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: G_dev is NULL", fn);
    if (dx_dtype != H2GCN_DTYPE_F32 && dx_dtype != H2GCN_DTYPE_BF16)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: dx_dtype = %d is neither H2GCN_DTYPE_F32 nor H2GCN_DTYPE_BF16", fn, dx_dtype);
    int st = check_bf16_array(fn, "X_dev", X, "ldx", ldx);
    if (st != H2GCN_OK) return st;
    const bf16* Xb = reinterpret_cast<const bf16*>(X);
    if (dx_dtype == H2GCN_DTYPE_BF16) {
        if (dX && (st = check_bf16_array(fn, "dX_dev", dX, "lddx", lddx)) != H2GCN_OK) return st;
        return dropout_dense_backward(Xb, ldx, n_rows, K, W, C, G, ldg, keep_prob, seed, step_dev, static_cast<bf16*>(dX), lddx, dW, workspace,
                                      workspace_bytes, stream_v);
    }
    return dropout_dense_backward(Xb, ldx, n_rows, K, W, C, G, ldg, keep_prob, seed, step_dev, static_cast<float*>(dX), lddx, dW, workspace,
                                  workspace_bytes, stream_v);
}

}  // extern "C"
