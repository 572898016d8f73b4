// classifier_rows.hip -- the ROW-SELECTED instantiations of the classifier kernels (classifier_kernels.hip.h: ROWS = true, TX = float
// or bf16, TD = float or bf16) behind h2gcn_dropout_dense_rows_f32 / _rows_bf16 / _backward_rows_f32 / _backward_rows_bf16.  A
// translation unit of its own, like classifier_bf16.hip: the full-matrix instantiations must keep their registers and occupancy
// (profiles/r09_train_rows_only_kernel_resources.txt).  Same kernels, same arithmetic: row i of the compact Z / G / dX is row
// rows[i] of X, the dropout mask is keyed by rows[i], every summation order over k (forward) and c (dX) is the full call's -- so
// Z_c and dX_c carry the bits of the full call's rows; dW is reduced in a fixed order over the n_sel list entries.
#include "classifier_kernels.hip.h"

namespace {

// what every row-selected call checks before the device is touched
int check_rows(const char* fn, const void* X, int64_t n_rows, const void* W, const int32_t* rows, int64_t n_sel) {
    if (n_rows < 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: n_rows = %lld is negative", fn, (long long)n_rows);
    if (n_sel < 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: n_sel = %lld is negative", fn, (long long)n_sel);
    if (n_sel > n_rows) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: n_sel = %lld exceeds n_rows = %lld (rows_dev is unique)", fn, (long long)n_sel, (long long)n_rows);
    if (n_rows > INT32_MAX) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: n_rows = %lld does not fit the int32 entries of rows_dev", fn, (long long)n_rows);
    if (!rows && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: rows_dev is NULL", fn);
    if (!X && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: X_dev is NULL", fn);
    if (!W) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: W_dev is NULL", fn);
    return H2GCN_OK;
}

}  // namespace

extern "C" {

int h2gcn_dropout_dense_rows_f32(const float* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* bias,
                                 float keep_prob, uint64_t seed, const int64_t* step_dev, float* Z, int64_t ldz, void* workspace,
                                 size_t workspace_bytes, void* stream_v, const int32_t* rows, int64_t n_sel) {
    const char* fn = "dropout_dense_rows_f32";
    int st = check_rows(fn, X, n_rows, W, rows, n_sel);
    if (st != H2GCN_OK) return st;
    if (!Z && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: Z_dev is NULL", fn);
    return dropout_dense_forward<float, true>(X, ldx, n_sel, K, W, C, bias, keep_prob, seed, step_dev, Z, ldz, workspace, workspace_bytes, stream_v,
                                              rows, n_rows);
}

int h2gcn_dropout_dense_rows_bf16(const uint16_t* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* bias,
                                  float keep_prob, uint64_t seed, const int64_t* step_dev, float* Z, int64_t ldz, void* workspace,
                                  size_t workspace_bytes, void* stream_v, const int32_t* rows, int64_t n_sel) {
    const char* fn = "dropout_dense_rows_bf16";
    int st = check_rows(fn, X, n_rows, W, rows, n_sel);
    if (st != H2GCN_OK) return st;
    if (!Z && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: Z_dev is NULL", fn);
    if ((st = check_bf16_array(fn, "X_dev", X, "ldx", ldx)) != H2GCN_OK) return st;
    return dropout_dense_forward<bf16, true>(reinterpret_cast<const bf16*>(X), ldx, n_sel, K, W, C, bias, keep_prob, seed, step_dev, Z, ldz, workspace,
                                             workspace_bytes, stream_v, rows, n_rows);
}

int h2gcn_dropout_dense_backward_rows_f32(const float* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* G,
                                          int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev, float* dX, int64_t lddx,
                                          float* dW, void* workspace, size_t workspace_bytes, void* stream_v, const int32_t* rows,
                                          int64_t n_sel) {
    const char* fn = "dropout_dense_backward_rows_f32";
    int st = check_rows(fn, X, n_rows, W, rows, n_sel);
    if (st != H2GCN_OK) return st;
    if (!G && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: G_dev is NULL", fn);
    return dropout_dense_backward<float, float, true>(X, ldx, n_sel, K, W, C, G, ldg, keep_prob, seed, step_dev, dX, lddx, dW, workspace,
                                                      workspace_bytes, stream_v, rows, n_rows);
}

int h2gcn_dropout_dense_backward_rows_bf16(const uint16_t* X, int64_t ldx, int64_t n_rows, int32_t K, const float* W, int32_t C, const float* G,
                                           int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev, int dx_dtype, void* dX,
                                           int64_t lddx, float* dW, void* workspace, size_t workspace_bytes, void* stream_v,
                                           const int32_t* rows, int64_t n_sel) {
    const char* fn = "dropout_dense_backward_rows_bf16";
    int st = check_rows(fn, X, n_rows, W, rows, n_sel);
    if (st != H2GCN_OK) return st;
    if (!G && n_sel > 0) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: G_dev is NULL", fn);
    if (dx_dtype != H2GCN_DTYPE_F32 && dx_dtype != H2GCN_DTYPE_BF16)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s: dx_dtype = %d is neither H2GCN_DTYPE_F32 nor H2GCN_DTYPE_BF16", fn, dx_dtype);
    if ((st = check_bf16_array(fn, "X_dev", X, "ldx", ldx)) != H2GCN_OK) return st;
    const bf16* Xb = reinterpret_cast<const bf16*>(X);
    if (dx_dtype == H2GCN_DTYPE_BF16) {
        if (dX && (st = check_bf16_array(fn, "dX_dev", dX, "lddx", lddx)) != H2GCN_OK) return st;
        return dropout_dense_backward<bf16, bf16, true>(Xb, ldx, n_sel, K, W, C, G, ldg, keep_prob, seed, step_dev, static_cast<bf16*>(dX), lddx, dW,
                                                        workspace, workspace_bytes, stream_v, rows, n_rows);
    }
    return dropout_dense_backward<bf16, float, true>(Xb, ldx, n_sel, K, W, C, G, ldg, keep_prob, seed, step_dev, static_cast<float*>(dX), lddx, dW,
                                                     workspace, workspace_bytes, stream_v, rows, n_rows);
}

}  // extern "C"
