// capi_internal.h -- error plumbing shared by the translation units of libh2gcn_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "h2gcn_hip.h"

namespace h2gcn {

// Records the message behind h2gcn_last_error() for the calling thread and returns `st` as int.
int fail(h2gcn_status st, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// What the mirror pass of H2GCN_PLAN_SYMMETRIC_PATTERN (symmetric.hip) reports for one hop.
struct MirrorStatus {
    unsigned long long missing_key;  // row << 32 | col of the first entry (in (row, col) order) without a mirror; ~0: none
    unsigned flags;                  // kMirror*
    unsigned pad;
};
constexpr unsigned kMirrorValuesDiffer = 1u;  // some vals[partner[e]] differs from vals[e] in its bits
constexpr unsigned kMirrorUnsorted = 2u;      // a row's columns are not strictly ascending
constexpr unsigned kMirrorRange = 4u;         // a column id outside [0, n)

hipError_t mirror_pass(int64_t n, int64_t nnz, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                       uint32_t* partner, float* t_vals, MirrorStatus* status, hipStream_t stream);

// What the pattern kernels (pattern_walk.hip.h: sddmm.hip, row_softmax.hip) need of a plan: the forward arrays of the selected
// hops, packed in ascending hop order, and the tunables that map rows to waves.  pattern_view touches no device; pattern_long_list
// returns the forward long-segment list of the selection (row << 4 | s per entry), building and caching it on the selection's first
// launch exactly as the forward launch does -- including the refusal to build it while `stream` is being captured.
struct PatternView {
    int n_sel;
    int64_t n_rows, n_cols;
    const int64_t* rowptr[H2GCN_MAX_HOPS];
    const int32_t* colidx[H2GCN_MAX_HOPS];
    int64_t nnz[H2GCN_MAX_HOPS];
    int long_threshold;
    int rows_per_wave;
    uint32_t mask;
};
int pattern_view(const h2gcn_plan* plan, uint32_t hop_mask, PatternView* out);
int pattern_long_list(const h2gcn_plan* plan, uint32_t mask, hipStream_t stream, const int64_t** list_dev, int* n_long,
                      bool adjoint = false);

// The adjoint view of a hop selection, for the column side of edge_scores.hip: `out` describes A_k^T (n_rows = the plan's n_cols,
// rowptr / colidx = t_rowptr / t_colidx -- the forward arrays of a symmetric plan) and perm[s][e'] is the forward entry behind
// transposed entry e' (a symmetric plan's partner).  Touches no device.  H2GCN_ERR_NO_TRANSPOSE on a plan without transposed
// operands, H2GCN_ERR_INVALID_ARGUMENT on one created without H2GCN_PLAN_KEEP_PERMUTATION.  The long-segment list that goes with
// it is pattern_long_list(..., adjoint = true): one entry per ROW that is long in any selected hop (no `<< 4 | s`), the list the
// adjoint launch of the selection uses.
int adjoint_view(const h2gcn_plan* plan, uint32_t hop_mask, PatternView* out, const uint32_t** perm);

// adjoint_view for a kernel that walks A_k^T but indexes no per-entry array (attention_backward.hip): the same PatternView, no
// permutation asked for -- a plan created without H2GCN_PLAN_KEEP_PERMUTATION is served.  H2GCN_ERR_NO_TRANSPOSE as above.
int adjoint_pattern_view(const h2gcn_plan* plan, uint32_t hop_mask, PatternView* out);

// The number of hops the plan was created with (a view's `mask` has a bit per hop of the plan): what the attention dropout generator
// (attention_dropout.hip) keys an entry by, together with the plan's hop index.  `plan` must not be NULL.
int plan_hop_count(const h2gcn_plan* plan);

}  // namespace h2gcn

#define H2GCN_HIP_TRY(expr)                                                                          \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return ::h2gcn::fail(_e == hipErrorOutOfMemory ? H2GCN_ERR_OUT_OF_MEMORY : H2GCN_ERR_HIP, \
                                 "%s failed: %s", #expr, hipGetErrorString(_e));                     \
    } while (0)
