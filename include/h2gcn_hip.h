/*
 * h2gcn_hip.h -- C ABI of libh2gcn_hip.so: the MI355X (gfx950) hop-aggregation path of H2GCN.
 *
 * The library replaces exactly one thing in the reference (GemsLab/H2GCN): the sparse aggregation that
 * `GCNLayer.call` performs through TensorFlow,
 *
 *     tf.stack([tf.sparse.sparse_dense_matmul(A_k, X) for A_k in adjhops], axis=-2)      -> [N, H, d]
 *
 * (reference h2gcn/models/_layers.py:54-81; the op underneath is TensorFlow's SparseTensorDenseMatMul,
 * call sites _layers.py:74,76) and its gradient wrt X (`dX = sum_k A_k^T dY[:,k,:]`, reached from
 * tape.gradient at h2gcn/models/H2GCN.py:66-74) -- and, for callers whose adjacency values are trainable, the op's
 * other gradient, wrt the stored values (h2gcn_sddmm_hops_*).  There is no native boundary in the reference to copy:
 * the reference's native boundary is TensorFlow's op registry.  Each entry point below cites the reference
 * behaviour it stands in for.
 *
 * Conventions
 *   - plain C linkage, POD arguments, no C++/torch types, no exceptions across the boundary;
 *   - every pointer named *_dev is a DEVICE pointer of the current HIP device, owned by the caller and
 *     required to outlive the plan / the launch that uses it;
 *   - every function returning int returns H2GCN_OK (0) or a negative h2gcn_status; the message for the last
 *     failure on the calling thread is h2gcn_last_error();
 *   - launches are asynchronous on the given stream (a hipStream_t passed as void*; NULL = default stream);
 *   - a plan is immutable after creation, so concurrent launches that share a plan are safe.
 *
 * Operand layout (what `sparse2Tensor` + `tf.sparse.reorder` produce in the reference,
 * h2gcn/datasets/_dataset.py:528-535, re-expressed as CSR):
 *   rowptr  int64 [n_rows+1]   ascending, rowptr[0] == 0
 *   colidx  int32 [nnz]        ascending inside each row (row-major canonical order), 0 <= col < n_cols
 *   vals    fp32  [nnz]        the normalised adjacency values (SYM: D^-1/2 A_k D^-1/2, RW: D^-1 A_k;
 *                              _dataset.py:109-124) -- the kernel is agnostic to how they were normalised.
 */
#ifndef H2GCN_HIP_H_
#define H2GCN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2GCN_ABI_VERSION 5
#define H2GCN_MAX_HOPS 8

typedef enum h2gcn_status {
    H2GCN_OK = 0,
    H2GCN_ERR_INVALID_ARGUMENT = -1, /* NULL pointer, bad size/stride/alignment, bad hop mask            */
    H2GCN_ERR_HIP = -2,              /* a HIP runtime call failed (message carries hipGetErrorString)     */
    H2GCN_ERR_OUT_OF_MEMORY = -3,    /* host or device allocation failed                                  */
    H2GCN_ERR_BAD_INDEX = -4,        /* rowptr not monotone / colidx out of range (TF: InvalidArgument)   */
    H2GCN_ERR_NO_TRANSPOSE = -5,     /* adjoint launch on a plan created without H2GCN_PLAN_BUILD_TRANSPOSE */
    H2GCN_ERR_INTERNAL = -6,
    H2GCN_ERR_EXCHANGE_TIMEOUT = -7  /* a peer's shard did not arrive within the exchange's time limit      */
} h2gcn_status;

/* flags for h2gcn_plan_opts.flags */
#define H2GCN_PLAN_BUILD_TRANSPOSE 0x1u /* also build A_k^T (needed by h2gcn_spmm_hops_T_f32)               */
#define H2GCN_PLAN_SKIP_VALIDATION 0x2u /* skip the one-time column-range check on the device               */
#define H2GCN_PLAN_HOST_TRANSPOSE  0x4u /* build A_k^T with the host counting sort instead of the device radix
                                           sort (debug / cross-check; same result)                            */

#define H2GCN_PLAN_KEEP_PERMUTATION 0x8u /* with BUILD_TRANSPOSE: remember which forward entry every transposed entry
                                           came from, so that h2gcn_plan_set_values can refresh A_k^T (+4 B/nonzero) */

#define H2GCN_PLAN_SYMMETRIC_PATTERN 0x10u /* with BUILD_TRANSPOSE: every A_k is square and stores (j, i) exactly when it stores
                                           (i, j); the adjoint then runs on the caller's arrays, no transposed copy is built
                                           (verified at creation -- see h2gcn_plan_create)                                   */

/* Tunables of the CSR-adaptive schedule.  Zero in a field means "library default". */
typedef struct h2gcn_plan_opts {
    uint32_t struct_size;        /* = sizeof(h2gcn_plan_opts), for forward compatibility                   */
    uint32_t flags;              /* H2GCN_PLAN_*                                                            */
    int32_t long_row_threshold;  /* (row,hop) segments with >= this many nonzeros are split across the
                                    waves of one workgroup (LDS-staged partial sums); default 256          */
    int32_t rows_per_wave;       /* consecutive rows a wave walks in the regular path; default 4           */
    int32_t variant;             /* segment walks of the kernel: 0 = default, CSR-adaptive -- long segments
                                    (>= long_row_threshold): one workgroup each, always; launches of >= ~50 k rows whose segments
                                    average < 16 nonzeros: in-tile short-row mode (G consecutive short rows per
                                    round, one lane group each) when the slice is 64 or 128 columns, else the wave
                                    walk with index prefetch across segments; MIXED launches (mean >= 16 but at
                                    least 5 % of the segments have <= 16 nonzeros, slice 64 / 128): list-driven by
                                    segment class -- short segments from the plan's binned list, one lane group
                                    each, medium ones one wave each; otherwise one wave per segment.
                                    1 = scalar-addressed float2 gathers at d=128; 2 = wave walk, always prefetch;
                                    3 = plain wave walk; 4 = default, but never use the slice-major scratch copy
                                    (A/B measurements); 5 = force the in-tile short-row mode; 6 = force the
                                    list-driven launch (whenever a short segment exists).  Variants 0, 2, 3, 4, 5,
                                    6 give identical bits.                                                      */
    int32_t slice_cols;          /* feature columns per slice of the slice-major schedule: 64 / 128 / 256,
                                    0 = heuristic (narrower slices when X is far beyond the Infinity Cache).
                                    All three give identical bits (one canonical summation tree); widths
                                    below 64 columns run as one masked 64-column slice                            */
    int32_t reserved[2];
} h2gcn_plan_opts;

/* Opaque: segment-class bins (long-segment lists, binned short-segment lists), optional transposed CSR, launch geometry. */
typedef struct h2gcn_plan h2gcn_plan_t;

/* ABI version of the loaded library (== H2GCN_ABI_VERSION it was built with). */
int h2gcn_abi_version(void);

/* Message of the last failure on this thread ("" if none).  Never NULL; valid until the next failing call
 * on the same thread. */
const char* h2gcn_last_error(void);

/* Number of HIP devices visible; negative h2gcn_status when the runtime cannot be initialised. */
int h2gcn_device_count(void);

/*
 * Build the launch plan for a list of hop matrices A_0..A_{H-1} that share one row space.
 * Stands in for: the once-per-run construction of `tensors.adj_hops`
 * (reference h2gcn/datasets/_dataset.py:559-576) as far as the device side is concerned -- the normalised
 * values themselves are computed by the caller.
 *
 *   n_hops            1..H2GCN_MAX_HOPS  (H2GCN uses 2: exact-1-hop and exact-2-hop neighbourhoods; the reference takes
 *                     as many groups as --adj_nhood lists).  Every hop count gives the same per-row summation tree.
 *                     Scheduling above 4 SELECTED hops: the forward keeps its per-hop short-segment lists at any
 *                     count; the adjoint (SUM mode: one list of the rows that are short in every selected hop, staged
 *                     through LDS per hop) keeps its list for selections of up to 4 hops and walks the row tiles for
 *                     5..8 -- a scheduling difference only, the bits do not change.  rows_per_wave is at most 7, so
 *                     (rows_per_wave + 1) * n_hops never exceeds the 64 row pointers one wave-wide load holds.
 *   n_rows, n_cols    matrix shape; n_rows != n_cols is allowed (row-partitioned shards: n_rows = N/P)
 *   rowptr_dev[k], colidx_dev[k], vals_dev[k]   CSR of hop k, device pointers (see layout above)
 *   opts              NULL for defaults
 *   stream            stream used for the one-time validation / transposition work; the call returns after
 *                     that work has completed (it synchronises the stream)
 *
 * Index validity (monotone rowptr, 0 <= col < n_cols) is checked here, once -- not per launch.  TensorFlow's
 * CPU kernel reports out-of-range indices as InvalidArgument at run time; this returns H2GCN_ERR_BAD_INDEX.
 *
 * H2GCN_PLAN_SYMMETRIC_PATTERN (opt-in; modifies H2GCN_PLAN_BUILD_TRANSPOSE).  The caller states that every A_k is square and
 * symmetric in PATTERN -- what the adjacency rings of an undirected graph are.  A^T of such a matrix has the row pointers and
 * column ids of A itself, so the adjoint operand of hop k aliases rowptr_dev[k] / colidx_dev[k]: no radix transposition runs and
 * no transposed index arrays are stored.  Everything that works on a plan with built transposes works unchanged (adjoint
 * launches, h2gcn_plan_schedule / h2gcn_plan_segment_classes with adjoint = 1, the adjoint row lists; h2gcn_plan_info reports
 * has_transpose = 1), and the adjoint's arrays hold exactly what the transposition would have produced: the same bits come out.
 *   The statement is always verified -- by the pass that also constructs what is left to construct.  For every stored entry
 *   e = (i, j) a device kernel binary-searches row j for column i (this relies on the ascending column order of the layout
 *   above, which the pass checks too, strictly); the position found is partner[e], and vals[partner[e]] is the value of
 *   entry e of A_k^T.  H2GCN_PLAN_SKIP_VALIDATION still skips only the separate column-range check.
 *   Values, per hop:  bit-symmetric (bits(vals[partner[e]]) == bits(vals[e]) for all e, e.g. SYM normalisation) and no
 *   H2GCN_PLAN_KEEP_PERMUTATION: the adjoint aliases vals_dev[k] as well, the plan owns nothing per nonzero.  Otherwise (e.g.
 *   RW normalisation) the plan owns t_vals[e] = vals[partner[e]], 4 B per nonzero.  With H2GCN_PLAN_KEEP_PERMUTATION the plan
 *   always owns t_vals and keeps partner (uint32) as the hop's permutation -- "the forward entry transposed entry e came
 *   from", as for a built transpose -- so h2gcn_plan_set_values works for any new values, symmetric or not.
 *   Errors:  an entry without a mirror: H2GCN_ERR_BAD_INDEX, "hop 1: entry (12, 40) has no mirror entry (40, 12): pattern not
 *   symmetric" -- of the lowest such hop, the entry that comes first in (row, col) order (a deterministic function of the
 *   operands); a row whose columns are not strictly ascending: H2GCN_ERR_BAD_INDEX; n_rows != n_cols, the flag together with
 *   H2GCN_PLAN_HOST_TRANSPOSE or without H2GCN_PLAN_BUILD_TRANSPOSE, a hop of >= 2^32 nonzeros: H2GCN_ERR_INVALID_ARGUMENT.
 *   A refused creation leaves nothing allocated.
 */
int h2gcn_plan_create(int n_hops, int64_t n_rows, int64_t n_cols,
                      const int64_t* const* rowptr_dev, const int32_t* const* colidx_dev,
                      const float* const* vals_dev, const h2gcn_plan_opts* opts, void* stream,
                      h2gcn_plan_t** out_plan);

/* Release the plan and everything it owns (never the caller's CSR arrays).  NULL is a no-op. */
void h2gcn_plan_destroy(h2gcn_plan_t* plan);

/*
 * Replace the VALUES of hop `hop` (same sparsity pattern: rowptr/colidx unchanged).  Stands in for what
 * SparseDropout does to the sparse feature operand every training step (reference h2gcn/models/_layers.py:7-19:
 * a fresh Bernoulli mask on `input.values`, survivors scaled by 1/keep_prob): the caller writes the new values
 * (dropped entries as explicit zeros) and points the plan at them; transposed operands are refreshed on `stream`
 * (needs H2GCN_PLAN_KEEP_PERMUTATION).  `vals_dev` must stay alive like the original array.  This MUTATES the plan:
 * it must not run concurrently with launches of the same plan on other streams.
 * Plans created with H2GCN_PLAN_SYMMETRIC_PATTERN: the same rule -- with H2GCN_PLAN_KEEP_PERMUTATION the plan-owned values of
 * A_k^T are refreshed through the mirror positions (the new values need not be symmetric; the PATTERN is what was verified),
 * without it the call fails as on any plan with transposed operands, whether or not the adjoint aliased the old values.
 * A hop that was row-constant (h2gcn_plan_row_constant) falls back to the value stream for good: the new values are not
 * examined.  The first such call on a row-constant hop releases the plan's row values (one hipFree; inside a stream capture
 * they stay allocated until the plan is destroyed); every later call does nothing on that account -- no detection, no
 * synchronisation.
 */
int h2gcn_plan_set_values(h2gcn_plan_t* plan, int hop, const float* vals_dev, void* stream);

/* Introspection (for reports and tests).  Any out pointer may be NULL. */
int h2gcn_plan_info(const h2gcn_plan_t* plan, int hop, int64_t* n_rows, int64_t* n_cols, int64_t* nnz,
                    int64_t* n_long_segments, int32_t* has_transpose);

/* What the adjoint operand of hop `hop` shares with the caller's forward arrays: 0 = nothing (built transpose, or a plan without
 * transposes), 1 = rowptr and colidx, 2 = rowptr, colidx and vals (see H2GCN_PLAN_SYMMETRIC_PATTERN).  Negative: h2gcn_status. */
int h2gcn_plan_transpose_sharing(const h2gcn_plan_t* plan, int hop);

/* Whether hop `hop` is ROW-CONSTANT: 1 when every stored value of each row of A_k carries the same bit pattern as the row's
 * first stored value (D^-1 A_k, an unnormalised 0/1 adjacency, mean aggregation ...; compared as 32-bit words: +0.0 next to
 * -0.0 is not constant, NaNs of one payload are; empty rows and a hop without nonzeros are), 0 otherwise.  Established once,
 * at h2gcn_plan_create (one read of vals, whether or not H2GCN_PLAN_SKIP_VALIDATION is set), cleared for good by
 * h2gcn_plan_set_values on that hop.  The plan keeps one fp32 value per row of a row-constant hop (n_rows * 4 bytes), and a
 * forward launch with an fp32 output that walks 64-column slices over at most two selected hops, ALL of them row-constant,
 * takes a row's value from there instead of reading vals -- same neighbours, same summation tree, same bits.  Everything else
 * (adjoint launches: A_k^T of a row-normalised matrix is not row-constant; per-launch values; the pattern kernels) reads the
 * value arrays as before.  Negative: h2gcn_status. */
int h2gcn_plan_row_constant(const h2gcn_plan_t* plan, int hop);

/* Device memory the plan owns at this moment, in bytes: transposed arrays, permutations, the values of A_k^T of a symmetric
 * plan, the row values of row-constant hops, and the device row lists built so far (they grow with the first launch of a hop
 * selection).  Never the caller's arrays.  0 for NULL. */
size_t h2gcn_plan_device_bytes(const h2gcn_plan_t* plan);

/* The schedule a launch of this plan would use for feature width d and source row stride ld_src (reports, tests):
 * columns per slice of the slice-major schedule, number of slices, segment walk (0 = wave per segment, 1 = the same
 * with index prefetch across segments, 2 = in-tile short-row mode: rounds of consecutive short rows one lane group per
 * segment, 3 = list-driven by segment class: short segments from the binned list, one lane group each, medium ones one wave
 * each -- see h2gcn_plan_segment_classes), whether a launch that is given
 * scratch would gather from a slice-major copy.  adjoint != 0 asks about h2gcn_spmm_hops_T_f32 (ld_src = ldg_row,
 * hop stride d).  Any out pointer may be NULL. */
int h2gcn_plan_schedule(const h2gcn_plan_t* plan, uint32_t hop_mask, int adjoint, int64_t ld_src, int32_t d,
                        int32_t* slice_cols, int32_t* n_slices, int32_t* segment_walk, int32_t* scratch_copy);

/* CSR-adaptive dispatch, introspection: the plan bins every (row, hop) segment by length -- short (<= 16 nonzeros, empty
 * ones included), medium, long (>= long_row_threshold) -- and a launch serves each class with its own walk (see
 * h2gcn_plan_opts.variant).  For the s-th selected hop, segments[3 s + {0, 1, 2}] / nonzeros[3 s + {0, 1, 2}] receive the
 * number of short / medium / long segments and the nonzeros they hold (adjoint != 0: of A_k^T); *listed receives how many
 * segments (adjoint: output rows, i.e. rows whose segments of ALL selected hops are short) a launch at width d / source
 * stride ld_src serves from the binned short list -- 0 when that launch leaves the short class to the wave walk, -1 when it
 * runs in the in-tile short-row mode (rounds of consecutive short rows are grouped on the fly, no list).  Any out
 * pointer may be NULL; segments / nonzeros need 3 * (number of selected hops) entries. */
int h2gcn_plan_segment_classes(const h2gcn_plan_t* plan, uint32_t hop_mask, int adjoint, int64_t ld_src, int32_t d,
                               int64_t* segments, int64_t* nonzeros, int64_t* listed);

/*
 * Fused multi-hop aggregation, forward:
 *
 *     Y[i*ldy_row + s*ldy_hop + c] = sum_j A_k[i,j] * X[j*ldx + c]      0<=i<n_rows, 0<=c<d
 *
 * for every selected hop k (bit k of hop_mask set; s = rank of k among the selected hops, ascending).
 * Stands in for GCNLayer.call (reference h2gcn/models/_layers.py:78-81): with ldy_hop = d and
 * ldy_row = H_sel*d the output is the stacked [n_rows, H_sel, d] tensor, already flattened the way the
 * following `V` (Flatten) layer wants it (h2gcn/models/H2GCN.py:271-272); other strides let the caller land
 * the hops directly inside a wider concat buffer (ConcatLayer, _layers.py:90-96).
 * `hop_mask` reproduces GCNLayer(hops=...) (_layers.py:57-59,80-81); 0 means "all hops of the plan".
 * Rows without nonzeros produce zeros (TF zero-initialises the output).  Offsets are 64-bit throughout:
 * the reference's column-split workaround for nnz*d > 2^31 (_layers.py:65-74) has no counterpart here.
 *
 *   X_dev   fp32, n_cols rows of d values, row stride ldx >= d (elements)
 *   Y_dev   fp32, must not alias X
 *   d       feature width >= 1, any value, any 4-byte aligned X / Y and any strides (the reference accepts any
 *           b.shape[1], _layers.py:62-76; raw feature widths such as Cora's 1433 occur).  Every d >= 4 runs on the
 *           float4 gather kernels, in place: 16-byte global loads and stores need only dword alignment on gfx950, and
 *           in a row whose width is not a multiple of 4 the lane that straddles the end gathers the row's last four
 *           columns (overlapping its neighbour) and stores the ones it owns.  d < 4 takes a generic column-tiled
 *           kernel.  Fastest when rows are cache-line aligned (ldx a multiple of 32 floats).
 *
 * Floating point: fp32 multiply-add per nonzero in ONE canonical summation tree per output element -- neighbour j of
 * the row (ascending column order, the reference's order after tf.sparse.reorder, _dataset.py:535) is added into
 * partial P[j mod 4], the element is (P0 + P1) + (P2 + P3) -- for every kernel, slice width, feature chunking,
 * scratch copy and segment walk (rows with >= long_row_threshold nonzeros: the same tree per wave over the wave's
 * 64-neighbour chunks, wave totals added in order).  The bits of Y depend only on the row's nonzeros, X and
 * long_row_threshold: a row-partitioned multi-GPU run equals the single-GPU run bit-for-bit.
 * Subnormals are kept: the library is built without any flush-to-zero option, and the multiply-adds, the bf16 conversion of the
 * store and the SDDMM chains below handle fp32 / bf16 subnormal operands, partial sums and results as IEEE 754 does (checked bit
 * for bit against the CPU restatements on all-subnormal operands, tests/test_special_values_gpu.py).  NaN and Inf propagate: a
 * stored entry whose value is an explicit zero still multiplies its neighbour (0 * Inf = NaN, the pattern decides).
 *
 * hipGraph capture: a launch may be issued on a capturing stream, with one proviso.  The device-side row lists of a hop
 * selection (its long-segment list; its per-class lists once a launch is list-driven) are built by the FIRST launch of
 * that selection -- a device allocation and a synchronous upload under the plan's lock, neither of which may happen inside
 * a capture.  The all-hops selection is prepared by h2gcn_plan_create; for any other hop_mask (and for the adjoint, per
 * hop_mask) run the launch once eagerly at the width you are going to capture -- a warm-up step -- before capturing it.
 * A launch that would have to build a list while its stream is capturing returns H2GCN_ERR_INVALID_ARGUMENT with that
 * advice (it never falls back to another walk silently: the graph would replay the slower schedule for ever).  The same
 * first launch is also where an eager caller pays the one-off host synchronisation.
 */
int h2gcn_spmm_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* X_dev, int64_t ldx,
                        int32_t d, float* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream);

/*
 * Same launch with options.
 *
 * workspace / workspace_bytes: caller-provided scratch for a slice-major copy of the gather source (one streaming pass,
 *   a few % of the launch), from which the launch then gathers.  h2gcn_spmm_workspace_bytes() says how much scratch a
 *   launch wants (0 = the plain launch is already the fastest); NULL / too small simply selects the plain launch.
 *   The copy is a pure performance device, used (a) when the row stride of X is a multiple of 1 KiB (e.g. a contiguous
 *   [N, 256] embedding) and the operand is far beyond the caches: gathering column slices straight out of such rows
 *   wastes three quarters of the cache sets; (b) when the rows are wide and do not start on cache lines (base or ld*4 not
 *   a multiple of 128; forward d > 128, adjoint d > 256) on such an operand: the copy's 64-column blocks are aligned
 *   (zero-padded when d is not a multiple of 4).  Rows that DO start on cache lines are sliced 64 columns wide in place.  Results are bit-identical with and without scratch (canonical summation tree).
 *   The scratch is only used by this launch (on `stream`); launches that may run concurrently need separate scratch.
 * bias / H2GCN_LAUNCH_RELU: fused epilogue of the store, Y = act(A X + bias[c]) -- what SparseDense.call applies
 *   after its sparse product (reference h2gcn/models/_layers.py:45-52: `+ self.bias`, then `self.activation`), so
 *   that the feature embedding needs no second pass over its output.  bias: d floats (device) or NULL.  Forward only.
 *   The ReLU is `t < 0 ? 0 : t` on the finished fp32 sum (after the bias): a NaN sum stays NaN -- as tf.nn.relu, torch.relu and
 *   np.maximum propagate it, and unlike C's fmaxf, which would return the other operand and store 0 -- so an embedding
 *   kernel that has diverged stays visible downstream; -Inf becomes 0, +Inf stays +Inf.
 *
 * h2gcn_spmm_workspace_bytes: adjoint != 0 asks about h2gcn_spmm_hops_T_opts_f32; src_dev / ld_src / ld_src_hop
 *   describe the gather source of that launch (forward: X_dev, ldx, 0; adjoint: dY_dev, ldg_row, ldg_hop); the pointer
 *   is only inspected (do its rows start on 128-byte cache lines?), never dereferenced.
 */
#define H2GCN_LAUNCH_RELU 0x1u
#define H2GCN_LAUNCH_ACCUMULATE 0x2u   /* adjoint only: dX += A^T dY instead of dX = A^T dY (see h2gcn_spmm_hops_T_opts_f32) */
typedef struct h2gcn_launch_opts {
    uint32_t struct_size;      /* = sizeof(h2gcn_launch_opts)                                               */
    uint32_t flags;            /* H2GCN_LAUNCH_*                                                             */
    void* workspace_dev;       /* scratch or NULL                                                            */
    size_t workspace_bytes;
    const float* bias_dev;     /* d floats or NULL                                                           */
} h2gcn_launch_opts;
size_t h2gcn_spmm_workspace_bytes(const h2gcn_plan_t* plan, uint32_t hop_mask, int adjoint, const float* src_dev,
                                  int64_t ld_src, int64_t ld_src_hop, int32_t d);
int h2gcn_spmm_hops_opts_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* X_dev, int64_t ldx,
                             int32_t d, float* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                             const h2gcn_launch_opts* opts, void* stream);

/*
 * Adjoint (backward wrt X):
 *
 *     dX[j*ldx + c] = sum_s sum_i A_k[i,j] * dY[i*ldg_row + s*ldg_hop + c]   0<=j<n_cols
 *
 * Stands in for the TF-registered gradient of SparseTensorDenseMatMul wrt its dense operand
 * (adjoint_a=True SpMM), summed over the hops that `tf.stack` fanned out, as reached from
 * tape.gradient (reference h2gcn/models/H2GCN.py:66-74).  The gradient wrt the adjacency values, which TF
 * also computes and the reference discards, is a launch of its own: h2gcn_sddmm_hops_f32 below.  Requires H2GCN_PLAN_BUILD_TRANSPOSE.
 * dX is overwritten (not accumulated into).
 */
int h2gcn_spmm_hops_T_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY_dev, int64_t ldg_row,
                          int64_t ldg_hop, int32_t d, float* dX_dev, int64_t ldx, void* stream);
/* The adjoint with options: workspace_dev / workspace_bytes and the flag H2GCN_LAUNCH_ACCUMULATE (bias_dev must be NULL).  With
 * scratch the stacked gradient is copied slice-major per hop when its rows are wide (d > 256) and not cache-line
 * aligned on an operand far beyond the caches -- same bits as the plain launch.
 * H2GCN_LAUNCH_ACCUMULATE: dX[j, c] += sum ... -- the adjoint's result is ADDED to what dX holds, each element as
 * `old + sum` with `sum` the canonical-tree value of the plain launch.  This is the backward of the concat-free propagation:
 * the gradient slot of r_{k-1} inside the [N, 448] gradient of the representation already holds the classifier's
 * contribution, and the round's adjoint lands on top of it without a separate `+=` pass (h2gcn/models/_layers.py:90-96 is the
 * concat whose gradient this adds up).  dX must not overlap dY.  Runs on the general-store kernels (no short-row / index
 * prefetch variants): meant for the wave-per-segment regime (see h2gcn_plan_schedule). */
int h2gcn_spmm_hops_T_opts_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY_dev, int64_t ldg_row,
                               int64_t ldg_hop, int32_t d, float* dX_dev, int64_t ldx,
                               const h2gcn_launch_opts* opts, void* stream);

/*
 * bf16 embeddings (ABI 5).  The same two launches with the GATHER SOURCE in bf16 -- X for the forward, dY for the adjoint --
 * and an fp32 or a bf16 output.  Adjacency values stay fp32 and the plan is the same: one plan serves fp32 and bf16 launches.
 * At d = 128 the gathered feature row is 256 B instead of 512 B per aggregated edge, so the dominant stream of a launch
 * roughly halves.  The suffix names the source dtype, as _f32 does.  Strides are in ELEMENTS.
 *
 *   y_dtype / dx_dtype   H2GCN_DTYPE_F32 or H2GCN_DTYPE_BF16 (any other value: H2GCN_ERR_INVALID_ARGUMENT)
 *
 * Arithmetic: every gathered bf16 element is widened exactly to fp32 (bf16 -> fp32 is exact), then multiplied and added in
 * fp32 in the canonical summation tree above.  An fp32 output is therefore BIT-IDENTICAL to the fp32 launch on the upcast
 * source (X.float()), for every segment walk, slice width, hop selection, feature chunking, row block, rows_per_wave and
 * long_row_threshold.  A bf16 output is the round-to-nearest-even of exactly that fp32 value (torch's .to(torch.bfloat16),
 * ties and overflow to inf included).  The forward's bias / H2GCN_LAUNCH_RELU epilogue runs on the fp32 value, before the
 * rounding; bias stays fp32.
 * Accuracy against the fp32 launch on an fp32 source x: with fp32 output, |Y(bf16(x)) - Y(x)| <= 2^-7 * sum_j |a_j| |x_j|
 * element-wise -- rounding x to bf16 contributes at most 2^-8 (the unit roundoff of an 8-bit significand) relative to each
 * term, and the two fp32 trees add a few fp32 ulps.
 *
 * Supported: bf16 -> fp32 and bf16 -> bf16, forward and adjoint (fp32 -> fp32 is the _f32 entry points; fp32 -> bf16 does not
 * exist).  H2GCN_LAUNCH_ACCUMULATE is accepted with an fp32 dX only (old + sum, as for the fp32 adjoint); with a bf16 dX it is
 * H2GCN_ERR_INVALID_ARGUMENT.
 * Alignment: every bf16 array needs a 4-byte aligned base, even row and hop strides and an even d (d = 2 included), so that
 * every lane's 8- / 4-byte load and store is dword-aligned; anything else is H2GCN_ERR_INVALID_ARGUMENT, with a message that
 * names the rule.  (The bf16 widths of H2GCN -- 64, 128, 256 and their concat slices -- are all even.)
 * Scratch: a bf16 launch never uses the slice-major scratch copy; opts->workspace_dev / workspace_bytes are ignored, and
 * h2gcn_spmm_workspace_bytes keeps describing fp32 launches.
 * Schedule: a bf16 launch takes the fp32 schedule for the same d and element strides -- h2gcn_plan_schedule and
 * h2gcn_plan_segment_classes describe it, except that it gathers in place where they report a scratch copy.
 * Offsets: whether the 32-bit gather offsets apply is decided in bytes of the real element size, so a bf16 source beyond 4 GiB
 * takes the 64-bit kernels.
 * hipGraph capture: the same condition as the fp32 launches (one eager launch per hop selection and width first).  Arguments
 * are validated before the device is touched.
 */
#define H2GCN_DTYPE_F32 0
#define H2GCN_DTYPE_BF16 1
int h2gcn_spmm_hops_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const uint16_t* X_dev, int64_t ldx, int32_t d,
                         int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, const h2gcn_launch_opts* opts, void* stream);
int h2gcn_spmm_hops_T_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const uint16_t* dY_dev, int64_t ldg_row, int64_t ldg_hop,
                           int32_t d, int dx_dtype, void* dX_dev, int64_t ldx, const h2gcn_launch_opts* opts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient with respect to the adjacency VALUES (an additive extension of ABI 5: look the symbols up before calling a build
 * that may predate it).  The second gradient of SparseTensorDenseMatMul -- a sampled dense-dense product over the CSR
 * pattern (SDDMM):
 *
 *     dvals[s][e] = sum_c dY[i*ldg_row + s*ldg_hop + c] * X[j*ldx + c]      for every stored entry e = (i, j) of hop k
 *
 * for every selected hop k (s = rank of k among the selected hops, ascending).  The reference never needs it (its adjacency is
 * constant); a caller whose hop values depend on something trainable -- learned or signed edge weights, attention coefficients
 * over the 1-hop / 2-hop rings, a per-edge gate -- does.
 *
 *   dY_dev     [n_rows, H_sel, d] through ldg_row / ldg_hop (elements; ldg_row >= d, ldg_hop >= d when H_sel > 1)
 *   X_dev      [n_cols, d], row stride ldx >= d.  n_rows != n_cols is allowed (shard plans, row-selected sub-plans)
 *   d          any width >= 1
 *   dvals_dev  HOST array of H_sel device pointers; entry s receives nnz_k fp32 values in the entry order of colidx_dev[k] and
 *              is OVERWRITTEN (never accumulated into).  An entry may be NULL only when its hop has no nonzeros.
 *
 * Only the plan's forward arrays rowptr / colidx are read -- neither its values nor its transposes -- so the call works on a
 * plan created without H2GCN_PLAN_BUILD_TRANSPOSE, and a stored entry whose current value is an explicit zero is computed like
 * any other: the pattern decides.  All offsets are 64-bit.  The call allocates nothing besides the long-segment list of a hop
 * selection that has not been launched before (see the capture rule).
 *
 * bf16 (h2gcn_sddmm_hops_bf16): BOTH operands are bf16; every element is widened exactly, all arithmetic is fp32 and the output
 * is fp32.  Layout as for the bf16 launches above: 4-byte aligned bases, even strides, even d -- anything else is
 * H2GCN_ERR_INVALID_ARGUMENT with a message that names the rule.
 *
 * Arithmetic: ONE order per element, a function of d alone.  The columns are cut into blocks of 64 (block b: columns
 * 64b .. 64b+63) and every block into 16 quads of 4 (quad q of block b: columns 64b+4q .. 64b+4q+3); a column >= d enters as +0
 * on both sides.
 *   quad value    t = g0*x0;  t = fma(g1, x1, t);  t = fma(g2, x2, t);  t = fma(g3, x3, t)
 *   block total   the 16 quad values summed by the xor butterfly over quad distances 1, 2, 4, 8:
 *                 v1[q] = t[q] + t[q^1],  v2[q] = v1[q] + v1[q^2],  v4[q] = v2[q] + v2[q^4],  B = v4[q] + v4[q^8]
 *   element       ((((+0 + B_0) + B_1) + B_2) ... + B_last),  blocks in ascending order, ceil(d / 64) of them
 * The bits therefore never depend on row length or segment class, long_row_threshold, rows_per_wave, slice_cols, the hop
 * selection, strides, or on which kernel geometry (1, 2 or 4 blocks in registers; column passes beyond 256 columns) served the
 * launch; and since bf16 widens exactly into the same order, h2gcn_sddmm_hops_bf16(g, x) is BIT-IDENTICAL to
 * h2gcn_sddmm_hops_f32 on the widened operands.  No atomics: two launches give the same bits.
 * Error bound: any order of a d-term fp32 dot product satisfies |dV - exact| <= gamma_d * sum_c |g_c x_c| (+ d * 2^-149 for
 * underflow), gamma_d = d*u / (1 - d*u), u = 2^-24.
 *
 * hipGraph capture: the condition of the forward launch of the same hop selection.  Segments with >= long_row_threshold
 * nonzeros are served from the plan's forward long-segment list of the selection -- the list h2gcn_spmm_hops_* uses; it is
 * built by the FIRST launch of that selection, whichever of the two it is, and the all-hops list at plan creation.  A launch
 * that would have to build it while its stream is being captured returns H2GCN_ERR_INVALID_ARGUMENT with the same advice (run
 * the launch once eagerly first).
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, d < 1, ldx / ldg_row / ldg_hop smaller than d, the bf16 layout rules, a
 * NULL dY / X / dvals table when the selection has nonzeros, a NULL dvals entry of a selected hop with nonzeros.
 */
int h2gcn_sddmm_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY_dev, int64_t ldg_row, int64_t ldg_hop,
                         const float* X_dev, int64_t ldx, int32_t d, float* const* dvals_dev, void* stream);
int h2gcn_sddmm_hops_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const uint16_t* dY_dev, int64_t ldg_row, int64_t ldg_hop,
                          const uint16_t* X_dev, int64_t ldx, int32_t d, float* const* dvals_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row softmax over the hop pattern and its backward (an additive extension of ABI 5: look the symbols up before calling a
 * build that may predate it) -- what turns per-entry scores into the attention coefficients that h2gcn_plan_set_values /
 * h2gcn_spmm_hops_* consume and h2gcn_sddmm_hops_* differentiates.  For every selected hop k (s = its rank among the selected
 * hops) and every row i the SEGMENT is the entries e of [rowptr_k[i], rowptr_k[i+1]), j = 0 .. n-1 in stored order:
 *
 *     forward    alpha[s][e]   = exp(scores[s][e] - m) / S          m = max_j score_j,  S = sum_j exp(score_j - m)
 *     backward   dscores[s][e] = alpha[s][e] * (dalpha[s][e] - D)   D = sum_j alpha_j * dalpha_j
 *
 * fp32 only; one softmax per (row, hop) segment (no joint softmax across hops).
 *
 *   scores_dev / alpha_dev / dalpha_dev / dscores_dev   HOST arrays of H_sel device pointers; entry s holds nnz_k floats in the
 *              entry order of colidx_dev[k].  Outputs are OVERWRITTEN.  An entry may be NULL only when its hop has no nonzeros.
 *   Aliasing:  alpha_dev[s] == scores_dev[s] and dscores_dev[s] == dalpha_dev[s] are allowed (a lane writes only entries it has
 *              read, after every read of the segment's sums); any other overlap between an output and any input or other
 *              output is undefined.
 *
 * Only the plan's forward rowptr arrays are read -- neither columns, values nor transposes -- so the calls work on plans
 * created without H2GCN_PLAN_BUILD_TRANSPOSE, on shard plans and on row-selected sub-plans.  Empty segments write nothing.
 * All offsets are 64-bit.  No atomics: two launches give the same bits.
 *
 * Arithmetic: ONE order per segment, a function of the segment's own contents (its n values in order) and of nothing else.
 *   t_j = score_j - m                           one fp32 subtraction
 *   e_j = exp2(t_j * 0x1.715476p+0f)            one fp32 multiplication by log2(e) rounded to fp32, then the hardware 2^x
 *                                               (v_exp_f32, 1 ulp) -- the ONE device exponential of every path
 *   256 partials P[l], l = j mod 256, each starting at +0 and accumulated sequentially in ascending j:
 *       forward   P[l] = P[l] + e_j             backward   P[l] = fma(alpha_j, dalpha_j, P[l])
 *   W_w, w = 0..3: the xor butterfly over lane distances 1, 2, 4, 8, 16, 32 of P[64w .. 64w+63]
 *       (v1[l] = P[l] + P[l^1], v2[l] = v1[l] + v1[l^2], ... W_w = v32[l] + v32[l^32])
 *   segment total S (forward) or D (backward) = (W_0 + W_1) + (W_2 + W_3)
 *   alpha_j  = e_j * (1 / S)                    1 / S ONE correctly rounded fp32 division per segment, then one multiplication
 *   dscore_j = alpha_j * (dalpha_j - D)         one subtraction, one multiplication
 * A partial that received no entry is +0 and adding +0 changes no bit here (every e_j >= +0; an fma onto +0 never gives -0), so
 * the bits never depend on which mapping served the segment (16-lane group, one wave in registers, one wave in passes, 4-wave
 * workgroup), on long_row_threshold, rows_per_wave, variant, slice_cols, the hop selection, the row the segment sits in or the
 * alignment of its first entry.
 * Error bounds (u = 2^-24, T = max_j |score_j - m|, every e_j a normal number):
 *   |alpha_j - exact| <= (6T + n + 6) * u * exact   and   |dscore_j - exact(alpha, dalpha)| <= alpha_j * gamma_{n+2} *
 *   (|dalpha_j| + sum_i |alpha_i dalpha_i|) + 2^-149,  gamma_k = k*u / (1 - k*u).
 * Non-finite scores follow softmax on the segment as IEEE arithmetic gives it: a segment that contains a NaN or a +inf is NaN
 * throughout (the maximum carries NaN explicitly: v_max_f32 would drop it), a segment made only of -inf is NaN throughout, and
 * -inf next to finite scores gives exactly +0.  Other segments are not affected.
 *
 * hipGraph capture: the condition of the forward launch of the same hop selection, as for h2gcn_sddmm_hops_*: segments with
 * >= long_row_threshold entries are served from the plan's forward long-segment list of the selection, built by the FIRST
 * launch of that selection (of any of these kernels; the all-hops list at plan creation).  A launch that would have to build
 * it while its stream is being captured returns H2GCN_ERR_INVALID_ARGUMENT with the same advice (run the launch once eagerly).
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, a NULL table when the selection has nonzeros, a NULL entry of a selected
 * hop that has nonzeros.
 */
int h2gcn_row_softmax_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* scores_dev,
                               float* const* alpha_dev, void* stream);
int h2gcn_row_softmax_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* alpha_dev,
                                        const float* const* dalpha_dev, float* const* dscores_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Additive (GAT-style) edge scores on the hop pattern and their backward (an additive extension of ABI 5: look the symbols up
 * before calling a build that may predate it) -- what PRODUCES the per-entry scores that h2gcn_row_softmax_hops_f32 turns into
 * attention coefficients, and what takes their gradient back to the nodes.  For every selected hop k (s = its rank among the
 * selected hops) and every stored entry e = (i, j) of A_k:
 *
 *     forward    pre[e]      = l[i*ldl + s] + r[j*ldr + s]                one fp32 addition
 *                score[s][e] = pre > 0 ? pre : pre * negative_slope       one fp32 multiplication on the negative branch
 *     backward   t[e]        = pre > 0 ? g[s][e] : g[s][e] * negative_slope     pre recomputed as above; a NaN pre takes the
 *                                                                               slope branch (as torch's leaky_relu does)
 *                dl[i*lddl + s] = sum of t[e] over row i of A_k           in stored order
 *                dr[j*lddr + s] = sum of t[e] over column j of A_k        = over row j of A_k^T, in A_k^T's stored order
 *
 * fp32 only.  No row-of-entry index exists anywhere: the kernels walk the CSR pattern.
 *
 *   l_dev      [n_rows, H_sel], row stride ldl >= H_sel (elements), column stride 1
 *   r_dev      [n_cols, H_sel], row stride ldr >= H_sel.  n_rows != n_cols is allowed (shard plans, row-selected sub-plans)
 *   scores_dev / dscores_dev   HOST arrays of H_sel device pointers; entry s holds nnz_k floats in the entry order of
 *              colidx_dev[k].  An entry may be NULL only when its hop has no nonzeros.
 *   dl_dev     [n_rows, H_sel] through lddl >= H_sel;  dr_dev [n_cols, H_sel] through lddr >= H_sel.  Either may be NULL: that
 *              side is not computed (both NULL is an error).
 * Outputs are OVERWRITTEN.  dl / dr are written for every row / column of every selected hop; an empty segment writes +0 (a
 * per-node output has no "write nothing").  Outputs must not overlap any input or each other.
 *
 * The ROW side (scores, dl) reads only the plan's forward rowptr / colidx -- neither values nor transposes -- so it works on
 * plans created without H2GCN_PLAN_BUILD_TRANSPOSE.  The COLUMN side (dr) walks the plan's adjoint operand A_k^T through its
 * permutation: for transposed entry e' of row j, i = t_colidx[e'], g = dscores[s][perm[e']], pre = l[i] + r[j]; nothing of size
 * nnz is materialised.  It needs H2GCN_PLAN_BUILD_TRANSPOSE and H2GCN_PLAN_KEEP_PERMUTATION (what h2gcn_plan_set_values
 * requires already); a H2GCN_PLAN_SYMMETRIC_PATTERN plan with the permutation kept serves it on the forward arrays.  Without
 * transposed operands the call returns H2GCN_ERR_NO_TRANSPOSE, without the permutation H2GCN_ERR_INVALID_ARGUMENT with a message
 * that names H2GCN_PLAN_KEEP_PERMUTATION -- both before the device is touched and before the row side runs.
 * All offsets are 64-bit.  No atomics: two launches give the same bits.
 *
 * Arithmetic of dl / dr: ONE order per segment (a row of A_k, or a row of A_k^T), a function of the segment's own terms t_m,
 * m = 0 .. n-1 in stored order, and of nothing else -- the row softmax's tree:
 *   256 partials P[q], q = m mod 256, each starting at +0 and accumulated sequentially in ascending m:  P[q] = P[q] + t_m
 *   W_w, w = 0..3: the xor butterfly over lane distances 1, 2, 4, 8, 16, 32 of P[64w .. 64w+63]
 *       (v1[q] = P[q] + P[q^1], v2[q] = v1[q] + v1[q^2], ... W_w = v32[q] + v32[q^32])
 *   total = (W_0 + W_1) + (W_2 + W_3)
 * A partial that starts at +0 and is only added to is never -0 (+0 + -0 = +0), and neither is any sum of values that are not
 * -0; so a partial, a wave total or a pair total that received no entry is +0 and adding it changes no bit.  The bits of dl /
 * dr therefore never depend on which mapping served the segment (16-lane group, one wave, 4-wave workgroup), on
 * long_row_threshold, rows_per_wave, variant, slice_cols or the hop selection, and the column side of a symmetric plan equals
 * that of a plan with built transposes.
 * Error bound: every term is exact or one rounding (g * slope), and any order of an n-term fp32 sum satisfies
 *   |dl - exact| <= gamma_{n+1} * sum_m |t_m| + (n + 1) * 2^-149,   gamma_k = k*u / (1 - k*u), u = 2^-24
 * (exact: real arithmetic on the fp32 inputs with the branch taken from the fp32 pre), and the same for dr.
 * Non-finite inputs follow IEEE arithmetic entry by entry: a NaN or an inf - inf in pre gives a NaN score there and t = g * slope;
 * only the dl / dr elements whose segment contains a non-finite t are non-finite, every other element keeps its bits.
 *
 * hipGraph capture: the condition of the forward launch of the same hop selection, as for h2gcn_sddmm_hops_*: segments with
 * >= long_row_threshold entries are served from the plan's long-segment list of the selection -- the forward launch's list for
 * scores and dl, the adjoint launch's for dr -- built by the FIRST launch of that selection (of any kernel that uses it; the
 * all-hops lists at plan creation).  A launch that would have to build one while its stream is being captured returns
 * H2GCN_ERR_INVALID_ARGUMENT with the same advice (run the launch once eagerly first).
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, ldl / ldr / lddl / lddr smaller than H_sel, a NULL l / r when the selection
 * has nonzeros, a NULL table or a NULL entry of a selected hop that has nonzeros, dl and dr both NULL.
 */
int h2gcn_edge_scores_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                               const float* r_dev, int64_t ldr, float negative_slope, float* const* scores_dev, void* stream);
int h2gcn_edge_scores_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                        const float* r_dev, int64_t ldr, float negative_slope, const float* const* dscores_dev,
                                        float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The head dimension of the three calls above (added within ABI 5; found by symbol like them): the SDDMM, the row softmax and
 * the edge scores for n_heads = K >= 1 heads in ONE launch each -- the links of the attention chain around
 * h2gcn_spmm_hops_values_f32, which takes its heads in one launch already.
 *
 * Layout: every per-entry array of selected hop s is CONTIGUOUS ENTRY-MAJOR: element (e, h) at e * K + h, e in the entry order of
 * colidx_dev[k]; nnz_k * K floats each (the layout h2gcn_spmm_hops_*values_f32 reads fastest: ldv_entry = K, ldv_head = 1).
 * fp32 only.  Tables, NULL entries, aliasing and OVERWRITTEN outputs as in the single-head calls.
 *
 *   sddmm      dvals[s][e*K + h] = sum_{c in head h} dY[i*ldg_row + s*ldg_hop + c] * X[j*ldx + c]
 *              head h owns the columns h*w .. (h+1)*w - 1, w = d / K.  Needs d % K == 0 and, for K > 1, w % 4 == 0 (the rule of
 *              h2gcn_spmm_hops_values_f32); K == 1 takes any d.  dY / X / strides as for h2gcn_sddmm_hops_f32.
 *   softmax    one softmax per (row, hop, head) segment: alpha[s][e*K + h] over the entries of e's row, head h alone; backward
 *              likewise.  alpha_dev[s] == scores_dev[s] and dscores_dev[s] == dalpha_dev[s] are allowed.
 *   scores     l_dev [n_rows, H_sel, K]: element (i, s, h) at i*ldl + s*K + h, ldl >= H_sel*K; r_dev, dl_dev, dr_dev likewise
 *              (ldr, lddl, lddr >= H_sel*K).  score[s][e*K + h] = leaky(l[i, s, h] + r[j, s, h]); dl[i, s, h] / dr[j, s, h] are the
 *              row / column sums of t[e, h].  Either of dl_dev / dr_dev may be NULL (both NULL is an error).  The column side has
 *              the plan requirements and the two refusals of h2gcn_edge_scores_backward_hops_f32 (H2GCN_ERR_NO_TRANSPOSE;
 *              H2GCN_ERR_INVALID_ARGUMENT naming H2GCN_PLAN_KEEP_PERMUTATION), before the device is touched and before the
 *              row side runs.
 *
 * Arithmetic: NOTHING NEW.  For every head h the bits equal those of the single-head entry point applied to head h alone:
 *   h2gcn_sddmm_hops_heads_f32            = h2gcn_sddmm_hops_f32 with d := w on the head's column slice of dY and X;
 *   h2gcn_row_softmax*_hops_heads_f32     = h2gcn_row_softmax*_hops_f32 on a contiguous copy of column h;
 *   h2gcn_edge_scores*_hops_heads_f32     = h2gcn_edge_scores*_hops_f32 on l[:, :, h] and r[:, :, h].
 * The bit-invariance and error-bound statements of those calls carry over per (segment, head) / (entry, head): the bits do not
 * depend on long_row_threshold, rows_per_wave, variant, the hop selection or on which kernel geometry served the launch; the
 * SDDMM's bound is gamma_w * sum_c |g_c x_c| + w * 2^-149, the softmax and edge-score bounds are unchanged.
 * Non-finite inputs stay inside their (segment, head) or (entry, head): a NaN in head h never changes a bit of another head.
 * Empty segments write nothing (softmax) or +0 (dl, dr).  No atomics, no workspace, all offsets 64-bit.
 *
 * hipGraph capture: the rule of the single-head calls (the long-segment lists of the selection: the forward launch's for the
 * SDDMM, the softmax, the scores and dl, the adjoint launch's for dr).
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, n_heads < 1, d % n_heads != 0, w % 4 != 0 with n_heads > 1, ldx / ldg_row /
 * ldg_hop smaller than d, ldl / ldr / lddl / lddr smaller than H_sel * n_heads, a NULL operand or table when the selection has
 * nonzeros, a NULL entry of a selected hop that has nonzeros, dl and dr both NULL.
 */
int h2gcn_sddmm_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY_dev, int64_t ldg_row, int64_t ldg_hop,
                               const float* X_dev, int64_t ldx, int32_t d, int32_t n_heads, float* const* dvals_dev, void* stream);
int h2gcn_row_softmax_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* scores_dev,
                                     float* const* alpha_dev, int32_t n_heads, void* stream);
int h2gcn_row_softmax_backward_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* alpha_dev,
                                              const float* const* dalpha_dev, float* const* dscores_dev, int32_t n_heads,
                                              void* stream);
int h2gcn_edge_scores_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                     const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope,
                                     float* const* scores_dev, void* stream);
int h2gcn_edge_scores_backward_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                              const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope,
                                              const float* const* dscores_dev, float* dl_dev, int64_t lddl, float* dr_dev,
                                              int64_t lddr, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * DYNAMIC (GATv2, Brody et al.) edge scores on the hop pattern and their backward (added within ABI 5; found by symbol like the
 * launches above).  leaky(l[i] + r[j]) is monotone in r[j]: inside a row every node ranks its neighbours alike.  Here the
 * nonlinearity sits between the gather and the reduction over the columns of a head:
 *
 *     forward    p_c   = u[i*ldu + c] + v[j*ldv + c]                    one fp32 addition
 *                q_c   = p_c > 0 ? p_c : p_c * negative_slope           a NaN p takes the slope branch
 *                score[s][e*K + h] = sum_{c in head h} a[s*lda + c] * q_c            e = (i, j) a stored entry of selected hop s
 *     backward   dq_c  = ds[s][e*K + h(c)] * a[s*lda + c]               one multiplication; p, q recomputed as above
 *                dp_c  = p_c > 0 ? dq_c : dq_c * negative_slope
 *                du[i*lddu + c] = sum_s sum_{e in row i of A_s}    dp_c
 *                dv[j*lddv + c] = sum_s sum_{e in column j of A_s} dp_c
 *                da[s*ldda + c] = sum_{e in A_s} ds[s][e*K + h(c)] * q_c
 *
 * with h(c) = c / w, w = d / K: head h owns the columns h*w .. (h+1)*w - 1.  Nothing of size nnz x d exists anywhere.
 *
 *   u_dev      [n_rows, d], row stride ldu >= d;  v_dev [n_cols, d], row stride ldv >= d (n_rows != n_cols is allowed)
 *   a_dev      [H_sel, d], row stride lda >= d: row s belongs to the s-th selected hop
 *   scores_dev / dscores_dev   HOST arrays of H_sel device pointers; entry s holds nnz_k * K floats, contiguous ENTRY-MAJOR (element
 *              (e, h) at e*K + h; K = 1: [nnz_k]), in the entry order of colidx_dev[k]; dscores in FORWARD entry order
 *   du_dev / dv_dev / da_dev   [n_rows, d] / [n_cols, d] / [H_sel, d] through lddu / lddv / ldda >= d.  Each may be NULL: not wanted
 *              (all three NULL is an error)
 *   workspace_dev   h2gcn_edge_scores_dynamic_workspace_bytes(plan, hop_mask, d) bytes, 4-byte aligned, used on `stream`: needed
 *              when da_dev is given (0 is returned for arguments the launch would refuse)
 * fp32 only.  Limits: d <= 256 (a node row stays in registers), d % n_heads == 0, w % 4 == 0 when n_heads > 1 (n_heads == 1 takes any
 * d <= 256).  Outputs are OVERWRITTEN and must not overlap any input or each other.  A row / column without entries writes +0;
 * a selection without nonzeros zeroes the requested outputs without a launch.  All offsets are 64-bit.  No float atomics.
 *
 * scores, du and da read the plan's forward rowptr / colidx only: plans without transposes serve them.  dv walks A_s^T through its
 * permutation (i = t_colidx[e'], ds at perm[e']) exactly as the column side of h2gcn_edge_scores_backward_hops_heads_f32 does and has
 * its two refusals -- H2GCN_ERR_NO_TRANSPOSE; H2GCN_ERR_INVALID_ARGUMENT naming H2GCN_PLAN_KEEP_PERMUTATION -- before the device is
 * touched and before the row side runs.  A symmetric plan with the permutation kept serves it on the forward arrays, with the bits of
 * a plan with built transposes.
 *
 * Arithmetic of a score: the order of h2gcn_sddmm_hops_heads_f32 (n_heads == 1: of h2gcn_sddmm_hops_f32) with g_c := a[s, c] and
 * x_c := q_c -- quad value t = a0*q0, fma(a1, q1, t), fma(a2, q2, t), fma(a3, q3, t); the head's xor butterfly over its quads; block
 * totals in ascending order from +0.  The bits of a score are therefore a function of a[s], u[i], v[j], d, K and the slope alone: not
 * of the segment class, long_row_threshold, rows_per_wave, the hop selection or the strides; and with u = +0 they are the bits of
 * h2gcn_sddmm_hops_heads_f32 on dY[i, s] = a[s], X = leaky(v).
 * Error bound (exact: real arithmetic on the fp32 inputs, the branch taken from the fp32 p): two roundings go into q_c, then any order
 * of a w-term dot product:  |score - exact| <= gamma_{w+2} * sum_c |a_c q_c| + (w + 2) * 2^-149,  gamma_k = k*u / (1 - k*u), u = 2^-24.
 *
 * Arithmetic of du / dv (contraction off: every product and every sum rounds on its own): ONE order per node, a function of the terms
 * of the node's segments and of long_row_threshold at most -- never of rows_per_wave, of which other outputs were asked for, or of
 * the run.  It is the canonical tree of h2gcn_spmm_hops_T_values_f32:
 *   - entry m of a segment (m counted from the segment's first entry) adds dp_c to the partial P[m mod 4], P = P + dp_c, every partial
 *     starting from +0 and running on across the selected hops in ascending order; the element is (P0 + P1) + (P2 + P3);
 *   - a node whose segment has >= long_row_threshold entries in ANY selected hop: every hop's segment is dealt in 64-entry chunks to 4
 *     waves (chunk c of a hop's segment to wave c mod 4), each wave builds that tree over its chunks, and the wave totals are added
 *     ((T0 + T1) + T2) + T3.
 * Error bound: |du - exact| <= gamma_{n+2} * sum |dp| + (n + 2) * 2^-149, n the entries of the row over the selected hops; dv likewise.
 * Arithmetic of da: two stages.  G = min(2048, blocks of the forward tile walk) workgroups stride over the blocks of the forward walk
 * hop by hop, every lane group adding its entries' ds * q_c in the order it meets them, and write ONE partial row per selected hop
 * into the workspace ([G, H_sel, d]); a second kernel adds row g into accumulator (g / 16) mod 4 of part g mod 16, (A0 + A1) +
 * (A2 + A3) per part, the 16 parts in ascending order from +0 -- a tree that is a function of G alone.  The bits of da depend on
 * the launch geometry (n_rows, rows_per_wave, long_row_threshold, the hop selection) but never on the run, nor on du / dv being asked for.
 * Error bound: |da - exact| <= gamma_{nnz_s+3} * sum |ds q| + (nnz_s + 3) * 2^-149.
 * Non-finite inputs follow IEEE arithmetic column by column: a NaN in column c of u[i] or v[j] reaches only the scores of the entries
 * that touch that node, in the head of c, and only column c of du / dv of the nodes whose segments hold such an entry.
 *
 * hipGraph capture: the rule of the SDDMM and edge-score calls -- the long-segment lists of the selection (the forward launch's for
 * scores, du and da, the adjoint launch's for dv), built by the FIRST launch of that selection; a launch that would have to build one
 * while its stream is being captured returns H2GCN_ERR_INVALID_ARGUMENT with the existing advice.
 *
 * Validation, in the order of h2gcn_sddmm_hops_heads_f32, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a
 * message naming the argument: a NULL plan, a hop mask outside the plan, d < 1, n_heads < 1, d % n_heads != 0, w % 4 != 0 with
 * n_heads > 1, d > 256, ldu / ldv / lda (lddu / lddv / ldda of a requested output) smaller than d, a NULL u / v / a or table when the
 * selection has nonzeros, a NULL entry of a selected hop that has nonzeros, du, dv and da all NULL, a workspace that is NULL or
 * smaller than h2gcn_edge_scores_dynamic_workspace_bytes when da is asked for.
 */
size_t h2gcn_edge_scores_dynamic_workspace_bytes(const h2gcn_plan_t* plan, uint32_t hop_mask, int32_t d);
int h2gcn_edge_scores_dynamic_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u_dev, int64_t ldu, const float* v_dev,
                                       int64_t ldv, const float* a_dev, int64_t lda, int32_t d, int32_t n_heads, float negative_slope,
                                       float* const* scores_dev, void* stream);
int h2gcn_edge_scores_dynamic_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u_dev, int64_t ldu,
                                                const float* v_dev, int64_t ldv, const float* a_dev, int64_t lda, int32_t d, int32_t n_heads,
                                                float negative_slope, const float* const* dscores_dev, float* du_dev, int64_t lddu,
                                                float* dv_dev, int64_t lddv, float* da_dev, int64_t ldda, void* workspace_dev,
                                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The hop aggregation on values that are an ARGUMENT of the launch, with an optional head dimension (added within ABI 5;
 * found by symbol like the launches above) -- the last link of the attention chain without h2gcn_plan_set_values:
 *
 *   forward:  Y[i, s, c]  = sum_e  V_s[e, h(c)] * X[j_e, c]                       e over row i of selected hop s
 *   adjoint:  dX[j, c]    = sum_s sum_e' V_s[perm_s[e'], h(c)] * dY[i_e', s, c]   e' over row j of A_s^T
 *
 * with h(c) = c / (d / n_heads): head h owns the columns h*d/n_heads .. (h+1)*d/n_heads - 1.
 *
 * values_dev[s] is the values array of the s-th SELECTED hop (ascending hop order, as for the softmax tables); element (e, h)
 * -- e in FORWARD entry order, also for the adjoint -- is values_dev[s][e * ldv_entry[s] + h * ldv_head[s]].  ldv_entry and
 * ldv_head are HOST arrays with one entry per selected hop, in elements: an [nnz, K] array is (K, 1), a [K, nnz] buffer is
 * (1, nnz) without a copy; n_heads == 1 with ldv_entry = 1 is the plain SpMM on the values handed in.
 *   n_heads >= 1, d % n_heads == 0; for n_heads > 1 also (d / n_heads) % 4 == 0 (a lane's four columns lie in one head).
 *   n_heads == 1 takes any d >= 1, any 4-byte-aligned bases and any strides, as h2gcn_sddmm_hops_f32 does.
 * X [n_cols, d] through ldx, Y [n_rows, H_sel, d] through ldy_row / ldy_hop, dY likewise through ldg_row / ldg_hop, dX
 * [n_cols, d] through ldx (elements; unit column stride).  The output must not overlap the gathered operand.  fp32 only; no
 * accumulate flag, no bias / ReLU epilogue, no workspace.  Every element of the output is written; an empty row stores +0.
 *
 * The plan gives the PATTERN only.  Its stored values (and transposed values) are never read and nothing in the plan changes:
 * launches with different values may share a plan, also concurrently.  The forward needs rowptr / colidx alone -- plans
 * without transposes, sub-plans of selected rows and n_rows != n_cols all work.  The adjoint walks the plan's transposed
 * operands (the forward arrays of a symmetric plan) and reads the values through their permutation: H2GCN_ERR_NO_TRANSPOSE on a
 * plan without them, H2GCN_ERR_INVALID_ARGUMENT naming H2GCN_PLAN_KEEP_PERMUTATION on a plan created without it.
 *
 * Arithmetic: THE canonical tree of "Floating point" above, nothing new -- the bits are those of h2gcn_spmm_hops_f32 /
 * h2gcn_spmm_hops_T_f32 on a plan whose installed values are V_s[:, h], applied per head to that head's column slice:
 *   - neighbour jj of a 64-entry chunk goes with one fmaf(v, x, P) into P[jj & 3], every partial starting from +0;
 *   - the element is (P0 + P1) + (P2 + P3);
 *   - forward: a segment of >= long_row_threshold entries is dealt in 64-entry chunks round-robin to 4 waves, each wave builds
 *     that tree over its chunks, and the wave totals are added ((T0 + T1) + T2) + T3;
 *   - adjoint: the partials run on across the selected hops (ascending); a row is long when it is long in ANY selected hop,
 *     and then every hop's segment is dealt to the 4 waves (chunk c of a hop's segment to wave c mod 4);
 *   - an empty row stores +0; an explicit-zero value still multiplies (0 * inf = NaN); the library is built without
 *     flush-to-zero, so subnormals are kept.
 * Two launches give the same bits (no atomics).  Where (P0 + P1) + (P2 + P3) has a NaN the payload is not specified.
 * Error bound (any order of an n-term fp32 sum of products, n the row length -- adjoint: summed over the selected hops):
 *   |y - exact| <= gamma_{n+2} * sum |v||x| + (n + 2) * 2^-149,   gamma_k = k*u / (1 - k*u), u = 2^-24.
 *
 * hipGraph capture: the rule of the forward launch.  Long segments (adjoint: long rows) are served from the plan's list of the
 * selection -- h2gcn_spmm_hops_values_f32 uses the forward launch's, h2gcn_spmm_hops_T_values_f32 the adjoint launch's -- built
 * by the FIRST launch of that selection (of any kernel that uses it; the all-hops lists at plan creation).  A launch that would
 * have to build one while its stream is being captured returns H2GCN_ERR_INVALID_ARGUMENT with the existing advice.
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, d < 1, n_heads < 1, d % n_heads, (d / n_heads) % 4 with heads, row
 * strides smaller than d, hop strides that make the hops' slots overlap, a NULL X / Y / dY / dX, an output that IS the gathered
 * operand, NULL stride arrays, a NULL table or a NULL entry of a selected hop that has nonzeros.
 */
int h2gcn_spmm_hops_values_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* values_dev, const int64_t* ldv_entry,
                               const int64_t* ldv_head, int32_t n_heads, const float* X_dev, int64_t ldx, int32_t d, float* Y_dev,
                               int64_t ldy_row, int64_t ldy_hop, void* stream);
int h2gcn_spmm_hops_T_values_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* values_dev, const int64_t* ldv_entry,
                                 const int64_t* ldv_head, int32_t n_heads, const float* dY_dev, int64_t ldg_row, int64_t ldg_hop, int32_t d,
                                 float* dX_dev, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The forward of the attention chain in ONE launch (added within ABI 5; found by symbol like the launches above) -- for every
 * forward that needs no gradient (validation and test passes, inference): scores, softmax and aggregation without the two
 * entry-major [nnz_k, K] arrays the chain writes and reads back.  For every selected hop s, row i and column c, h = c / (d / K):
 *
 *     Y[i, s, c] = sum_e alpha_s[e, h] * X[j_e, c]                             e over row i of selected hop s
 *     alpha_s[., h] = softmax over that segment of leaky(l[i, s, h] + r[j_e, s, h])
 *
 *   l_dev [n_rows, H_sel, K]: element (i, s, h) at i*ldl + s*K + h, ldl >= H_sel*K; r_dev [n_cols, H_sel, K] likewise through
 *   ldr -- the operands of h2gcn_edge_scores_hops_heads_f32.  X_dev [n_cols, d] through ldx; Y_dev [n_rows, H_sel, d] through
 *   ldy_row / ldy_hop -- those of h2gcn_spmm_hops_values_f32.  n_heads = K: K == 1 takes any d; K > 1 needs d % K == 0 and
 *   (d / K) % 4 == 0; K <= 16 is served, a larger K is refused with H2GCN_ERR_INVALID_ARGUMENT naming the limit (run the chain).
 * The launch reads only rowptr / colidx: no transposes are needed, n_rows != n_cols is legal (sub-plans of selected rows), the
 * plan's stored values are never read and nothing in the plan changes.  No workspace, no atomics, no allocation; all offsets
 * 64-bit; fp32 only.  Every element of Y is written; an empty segment stores +0.  Forward only: there is no backward, the chain
 * is what training runs.
 *
 * THE CONTRACT IS THE CHAIN'S BITS.  For every head, Y equals bit for bit what these three launches give on the same operands:
 *   1. h2gcn_edge_scores_hops_heads_f32      scores
 *   2. h2gcn_row_softmax_hops_heads_f32      alpha
 *   3. h2gcn_spmm_hops_values_f32            Y, with entry-major values (ldv_entry = K, ldv_head = 1)
 * Nothing is new in the arithmetic; the three orders above are reproduced, every stored value recomputed by its own operations:
 *   score    one fp32 addition, one multiplication on the `pre > 0`-false branch (a NaN pre takes the slope branch);
 *   softmax  t_j = score_j - m; e_j = exp2(t_j * log2e) with the one hardware exponential; 256 partials P[j mod 256], each from
 *            +0, accumulated in ascending j; W_w the xor butterfly over index distances 1..32 of P[64w .. 64w+63];
 *            S = (W_0 + W_1) + (W_2 + W_3); one correctly rounded 1/S per segment; alpha_j = e_j * (1/S).  The butterfly is
 *            defined on the partial's index: any lane placement with the same pairings gives the same bits;
 *   non-finite: a NaN or a +inf score makes its segment NaN throughout, a segment of -inf only is NaN throughout, -inf next to
 *            finite scores gives exactly +0; a head that holds a NaN never changes a bit of another head;
 *   aggregation: the canonical tree -- entry jj of a 64-entry chunk goes into P[jj & 3] with one fmaf from +0, the element is
 *            (P0 + P1) + (P2 + P3); a segment of the plan's long list is dealt in 64-entry chunks to 4 waves and the wave
 *            totals are combined as ((T0 + T1) + T2) + T3; an explicit-zero coefficient still multiplies (0 * inf = NaN).
 * The bits therefore do not depend on long_row_threshold, rows_per_wave, the hop selection or the kernel geometry, exactly as the
 * chain's do not.  Where the chain's result is NaN this one is NaN; the payload is not specified.
 *
 * hipGraph capture: the rule of the forward launch (the long-segment list of the selection, built by the first launch of that
 * selection; a launch that would have to build one during capture returns H2GCN_ERR_INVALID_ARGUMENT with the existing advice).
 * A selection without nonzeros is a memset of the output.
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument: a NULL
 * plan ("plan is NULL"), a hop mask outside the plan, d < 1, n_heads < 1, n_heads > 16, d % n_heads, (d / n_heads) % 4 with
 * heads, ldl / ldr smaller than H_sel * n_heads, ldx / ldy_row smaller than d, an ldy_hop that makes the hop outputs overlap, a
 * NULL Y, a NULL l / r / X when the selection has nonzeros, a Y that IS X, l or r.
 */
int h2gcn_attention_hops_heads_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                   int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                   float* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training attention without per-entry arrays (added within ABI 5; found by symbol like the launches above): the forward above
 * that ALSO STORES THE SOFTMAX STATISTICS, and a RECOMPUTING BACKWARD that reads them.  Nothing of size nnz is read, written or
 * allocated by either; no workspace, no atomics; all offsets 64-bit; fp32 only.
 *
 * h2gcn_attention_hops_heads_stats_f32: the arguments of h2gcn_attention_hops_heads_f32 plus stats_dev [n_rows, H_sel, 2, K]
 * through ldstats >= H_sel*2*K: element (i, s, 0, h) at i*ldstats + s*2*K + h is m, the maximum score of the segment, element
 * (i, s, 1, h) at i*ldstats + s*2*K + K + h is 1/S -- the values the walk holds anyway.  Y is bit for bit what
 * h2gcn_attention_hops_heads_f32 stores (hence the chain's bits); an empty segment stores (+0, +0); a segment whose maximum is NaN
 * stores NaN.  The same validation, plus: ldstats too small, a NULL stats, a stats that IS Y, X, l or r.  K <= 16.
 *
 * h2gcn_attention_hops_heads_backward_f32: given G = dLoss/dY [n_rows, H_sel, d] (through ldg_row / ldg_hop), the forward's l, r,
 * X, stats and Y, for every entry e = (i, j) of selected hop s and head h (columns c of head h):
 *
 *     pre = l[i,s,h] + r[j,s,h]       alpha[e,h] = exp2((leaky(pre) - m[i,s,h]) * log2e) * rinv[i,s,h]      (the forward's operations)
 *     dalpha[e,h] = sum_c G[i,s,c] * X[j,c]                delta[i,s,h] = sum_c G[i,s,c] * Y[i,s,c]
 *     dscore = alpha * (dalpha - delta)                    dpre = pre > 0 ? dscore : dscore * negative_slope   (a NaN pre: the slope branch)
 *     dl[i,s,h] = sum_{e in row i} dpre      dr[j,s,h] = sum_{e in column j} dpre      dX[j,c] = sum_s sum_{e in column j} alpha[e,h(c)] * G[i,s,c]
 *
 * Outputs, each optional (NULL: not wanted; at least one must be wanted): dl_dev [n_rows, H_sel, K] through lddl, dr_dev [n_cols,
 * H_sel, K] through lddr, dX_dev [n_cols, d] through lddx; delta_dev [n_rows, H_sel, K] through lddelta is a caller-provided buffer
 * that the ROW SIDE fills and the COLUMN SIDE reads (it may be NULL when only dl is wanted).  Two launches: the row side (always)
 * walks A_s and gathers X[j], r[j,s]; the column side (when dr or dX is wanted) walks A_s^T and gathers G[i,s] and the 4 K node
 * floats l, m, 1/S, delta of row i.  THE COLUMN SIDE READS t_rowptr / t_colidx ONLY, never the permutation: a plan created with
 * H2GCN_PLAN_BUILD_TRANSPOSE but without H2GCN_PLAN_KEEP_PERMUTATION is served, and so is a symmetric plan on its forward arrays;
 * a plan without transposes gets H2GCN_ERR_NO_TRANSPOSE when dr or dX is wanted (dl alone needs none).
 * Widths: K == 1 takes any d up to 256; K > 1 needs d % K == 0 and (d / K) % 4 == 0; d > 256 is refused with a message naming the
 * limit (run the chain), as is K > 16.
 *
 * THE GRADIENTS ARE DETERMINISTIC BUT NOT THE CHAIN'S BITS: two launches on the same operands give the same bits, yet delta comes
 * from <G, Y> over the head's columns, not from the chain's sum of alpha * dalpha over the segment (the two are equal in exact
 * arithmetic because Y is the alpha-weighted sum of the X[j]), and the sums below have orders of their own.  THE SUMMATION ORDERS:
 *   per-entry dot products (dalpha, delta): the SDDMM's order on the head's column slice -- per quad of 4 columns t = g0*x0, then
 *            fma(g1, x1, t), fma(g2, x2, t), fma(g3, x3, t); the 16 quads of a 64-column block by the xor butterfly over quad
 *            distances 1, 2, 4, 8; block totals added in ascending order from +0;
 *   dl / dr: the row-softmax tree over the WALKED segment (row i of A_s for dl, row j of A_s^T for dr): 256 partials P[t mod 256], each
 *            from +0, accumulated in ascending position t; W_w the xor butterfly over index distances 1..32 of P[64w .. 64w+63];
 *            the element is (W_0 + W_1) + (W_2 + W_3);
 *   dX:      per selected hop the canonical aggregation tree over row j of A_s^T -- the 64-entry chunks of the segment are dealt to
 *            four sets, chunk t to set t mod 4; within a set entry jj of a chunk goes into P[jj & 3] with one fmaf from +0, chunks in
 *            ascending order, T_u = (P0 + P1) + (P2 + P3); the hop's total is ((T0 + T1) + T2) + T3; the element is the sum of the hop
 *            totals in ascending hop order.
 * One tree per output element: the bits do not depend on long_row_threshold, rows_per_wave or the kernel geometry; dl / dr of a hop
 * do not depend on which other hops are selected.  A non-finite operand reaches exactly the elements whose sums touch it.
 *
 * hipGraph capture: the rule of the forward launch -- both long-segment lists of the selection (the forward's and the adjoint's)
 * are built by the first launch of that selection, so a training step can be captured after one eager warm-up.  A selection
 * without nonzeros is a memset of the outputs.
 *
 * Validation, all before the device is touched, each H2GCN_ERR_INVALID_ARGUMENT with a message naming the argument unless noted: a
 * NULL plan ("plan is NULL"), a hop mask outside the plan, d < 1, n_heads < 1, n_heads > 16, d % n_heads, (d / n_heads) % 4 with
 * heads, d > 256, no output wanted, a leading dimension too small, hop strides that overlap, a NULL delta when dr or dX is
 * wanted, a plan without transposes when dr or dX is wanted (H2GCN_ERR_NO_TRANSPOSE), a NULL input when the selection has
 * nonzeros, an output that IS an input or another output.
 */
int h2gcn_attention_hops_heads_stats_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                         int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                         float* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats, void* stream);
int h2gcn_attention_hops_heads_backward_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                            int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev, int64_t ldx, int32_t d,
                                            const float* stats_dev, int64_t ldstats, const float* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                                            const float* G_dev, int64_t ldg_row, int64_t ldg_hop, float* delta_dev, int64_t lddelta,
                                            float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, float* dX_dev, int64_t lddx,
                                            void* stream);

/* ATTENTION DROPOUT: dropout on the attention coefficients (GAT's attn_drop) of the recomputing pair above, with the mask DRAWN IN
 * THE KERNELS (h2gcn_amd/csrc/attention_dropout.hip, attention_dropout_backward.hip).  Added within ABI 5: find the entry points by
 * symbol.  Every (entry, head) has a factor f[e,h] in {+0, 1/keep_prob}; nothing of size nnz holds it, forward or backward.
 *
 * THE GENERATOR.  f is a pure function of (seed, step, k, i, j, h): k the PLAN's hop index (not the position in the selection), (i, j)
 * the row and column of the stored entry in the plan's forward operand, h the head.  It does not depend on the entry's position in
 * colidx or t_colidx, on the segment classes, long_row_threshold or rows_per_wave, on which hops are selected, or on whether the
 * column side walks a built transpose or a symmetric plan's forward arrays.  With all integer arithmetic modulo 2^32 unless noted:
 *     mix32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *     step = step_dev ? *step_dev : 0   (64 bits, read on the device when the kernel runs)
 *     k0 = mix32(lo32(seed) ^ mix32(lo32(step) + 0x9E3779B9))       k1 = mix32(hi32(seed) ^ hi32(step) ^ k0 ^ 0x85EBCA6B)
 *       (the key derivation of the classifier's dropout, the same constants)
 *     gid = ((uint64(i) * n_cols + j) * n_hops_of_plan + k) * 8 + (h >> 1)       (modulo 2^64; one word per PAIR of heads)
 *     w = lo32(gid) ^ rot16(hi32(gid)) ^ k0;  w ^= w >> 16;  w *= 0x7FEB352D;  w ^= k1;  w ^= w >> 15;  w *= 0x846CA68B;  w ^= w >> 16
 *     field = (w >> 16 * (h & 1)) & 0xFFFF        kept iff field < thr,  thr = floor(keep_prob * 65536) computed in double (65536 at 1)
 *     f = kept ? inv_keep : +0,   inv_keep = 1.f / keep_prob, one fp32 division on the host
 * Any keep_prob in (0, 1] is served by this single mode; the realised keep probability is thr / 65536.
 *
 * WHERE f ENTERS (each time ONE fp32 multiply, never contracted into a neighbour):
 *   forward       Y[i,s,c] = sum_e (alpha[e,h] * f[e,h]) * X[j_e,c]: the coefficient alpha * f is formed before it enters the aggregation
 *                 tree of h2gcn_attention_hops_heads_f32, so Y has the bits of h2gcn_spmm_hops_values_f32 on the values alpha_k * f_k.  A
 *                 dropped entry STILL multiplies: (alpha * 0) * inf is NaN, as in the chain.  stats are those of the launch without
 *                 dropout, bit for bit (the dropout comes after the softmax);
 *   row side      dalpha[e,h] = f[e,h] * <G[i,s], X[j]>_h;  delta = <G, Y>_h unchanged (Y carries f, so delta is still sum_e alpha * dalpha);
 *   column side   dalpha the same;  dscore = alpha * (dalpha - delta) with the UNDROPPED alpha;  dX[j,c] += (alpha * f) * G[i,s,c], alpha * f
 *                 one multiply as the forward forms it.
 * dpre, dl, dr, the summation orders and every limit (K <= 16; backward d <= 256) are those of the pair above.
 *
 * h2gcn_attention_hops_heads_stats_dropout_f32 / h2gcn_attention_hops_heads_backward_dropout_f32: the arguments of
 * h2gcn_attention_hops_heads_stats_f32 / h2gcn_attention_hops_heads_backward_f32 plus keep_prob, seed and step_dev (a device pointer to
 * one int64, or NULL for step 0); the backward must be given the forward's (keep_prob, seed, *step_dev).  keep_prob == 1 dispatches to
 * the launches without dropout: their bits.  keep_prob outside (0, 1] (NaN included) is refused FIRST, "keep_prob = ... outside (0, 1]";
 * then the validation of the entry point without dropout, in its order, all before the device is touched.  hipGraph capture: the rule
 * of those launches; step_dev is read when the kernel runs, so a replay after a stream-ordered bump of the counter draws a fresh mask.
 *
 * h2gcn_attention_dropout_factors_hops_f32: the factors themselves, for a chain that multiplies its alpha by them and for tests --
 * f_dev[s][e * ldf_entry[s] + h] = f[e,h] for the entries e of selected hop s (ascending hop order) and h < n_heads; reads rowptr /
 * colidx only.  Refused: a NULL plan, a hop mask outside the plan, n_heads < 1 or > 16, keep_prob outside (0, 1], and -- when the
 * selection has nonzeros -- a NULL f_dev or f_dev[s], a NULL ldf_entry, ldf_entry[s] < n_heads.
 */
int h2gcn_attention_hops_heads_stats_dropout_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                                 const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope, const float* X_dev,
                                                 int64_t ldx, int32_t d, float* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev,
                                                 int64_t ldstats, float keep_prob, uint64_t seed, const int64_t* step_dev, void* stream);
int h2gcn_attention_hops_heads_backward_dropout_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl,
                                                    const float* r_dev, int64_t ldr, int32_t n_heads, float negative_slope,
                                                    const float* X_dev, int64_t ldx, int32_t d, const float* stats_dev, int64_t ldstats,
                                                    const float* Y_dev, int64_t ldy_row, int64_t ldy_hop, const float* G_dev, int64_t ldg_row,
                                                    int64_t ldg_hop, float* delta_dev, int64_t lddelta, float* dl_dev, int64_t lddl,
                                                    float* dr_dev, int64_t lddr, float* dX_dev, int64_t lddx, float keep_prob, uint64_t seed,
                                                    const int64_t* step_dev, void* stream);
int h2gcn_attention_dropout_factors_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, int32_t n_heads, float keep_prob, uint64_t seed,
                                             const int64_t* step_dev, float* const* f_dev, const int64_t* ldf_entry, void* stream);

/* BF16 EMBEDDINGS IN THE RECOMPUTING ATTENTION (h2gcn_amd/csrc/attention_bf16.hip; added within ABI 5: find the entry points by
 * symbol).  The three launches above -- forward, forward + statistics, recomputing backward -- on bf16 wide operands, under the
 * contract of h2gcn_spmm_hops_bf16: every gathered bf16 element is WIDENED EXACTLY, EVERY OPERATION OF THE FP32 KERNEL RUNS IN FP32
 * IN THE DOCUMENTED ORDER, AND AN OUTPUT IS ROUNDED ONCE, TO NEAREST EVEN, AT THE FINAL STORE.  Consequently an fp32 output of a bf16
 * launch is bit-identical to the fp32 launch on the upcast operands, and a bf16 output is that value rounded to nearest even (ties
 * and overflow to infinity as torch's .to(torch.bfloat16)).  l, r, stats, delta, dl and dr stay fp32: they are K wide, not d wide.
 *
 * THE SUMMATION ORDERS are those of the fp32 launches, word for word: the softmax tree, the aggregation tree of Y, the SDDMM order of
 * dalpha and delta, the row-softmax tree of dl / dr and the per-hop aggregation tree of dX; dX is rounded once, after the sum over
 * the hops.  The bits do not depend on long_row_threshold, rows_per_wave, the hop selection or the kernel geometry.
 *
 * Argument orders follow the fp32 calls; X_dev (and in the backward Y_dev and G_dev) are bf16 (uint16_t storage); y_dtype / dx_dtype
 * are H2GCN_DTYPE_F32 or H2GCN_DTYPE_BF16 and give the element type behind Y_dev / dX_dev (any other value:
 * H2GCN_ERR_INVALID_ARGUMENT); every leading dimension is in ELEMENTS of its array.  In the backward X, Y and G are all bf16:
 * delta = <G, Y> is taken on the bf16 Y that the forward stored.  Limits are those of the fp32 calls: K <= 16; K > 1 needs d % K == 0
 * and (d / K) % 4 == 0; the backward needs d <= 256; the forward takes any even d.
 *
 * Validation: that of the fp32 calls, in their order and with their messages, all before the device is touched; plus the dtype
 * code (after the plan and the hop mask) and, after the stride checks, the layout rule of every bf16 array -- a 4-byte aligned base,
 * even row / hop strides and an even d ("bf16 X: ...", the messages of h2gcn_spmm_hops_bf16).  A selection without nonzeros is a
 * memset of the outputs in the element size of each.  hipGraph capture: the rule of the fp32 launches.
 */
int h2gcn_attention_hops_heads_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                    int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                    int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, void* stream);
int h2gcn_attention_hops_heads_stats_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                          int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                          int y_dtype, void* Y_dev, int64_t ldy_row, int64_t ldy_hop, float* stats_dev, int64_t ldstats,
                                          void* stream);
int h2gcn_attention_hops_heads_backward_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* l_dev, int64_t ldl, const float* r_dev,
                                             int64_t ldr, int32_t n_heads, float negative_slope, const uint16_t* X_dev, int64_t ldx, int32_t d,
                                             const float* stats_dev, int64_t ldstats, const uint16_t* Y_dev, int64_t ldy_row, int64_t ldy_hop,
                                             const uint16_t* G_dev, int64_t ldg_row, int64_t ldg_hop, float* delta_dev, int64_t lddelta,
                                             float* dl_dev, int64_t lddl, float* dr_dev, int64_t lddr, int dx_dtype, void* dX_dev, int64_t lddx,
                                             void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Operand construction on the device: exact-k-hop neighbourhood rings and their normalisation -- the step that
 * FEEDS the aggregation.  Stands in for TransformSPAdj.nhoodSplit (reference h2gcn/datasets/_dataset.py:138-158:
 * `mt <- bin(mt @ (A + I))`, ring_k = mt_k - mt_{k-1}, a host SpGEMM in scipy) and TransformSPAdj.normalize
 * (:109-124).  A ring is a SET expression over CSR patterns, evaluated row by row in a two-level LDS bitmap
 * (h2gcn_amd/csrc/rings.hip):
 *
 *     out[i] = ( U_{j in F[i]} A[j]  U  U_p ADD_p[i]  U  ({i} if add_diag) )  \  ( U_q SUB_q[i]  U  ({i} if sub_diag) )
 *
 *   ring_k (k >= 1):  F = ring_{k-1} (ring_0 = I, i.e. F[i] = {i}; for k = 1 simply pass F = I or use ring_1 = A),
 *                     SUB = ring_1 .. ring_{k-1}, sub_diag = 1
 *   merged group "0,1" of --adj_nhood (getTensors, :560-572):  no F, ADD = {ring_1}, add_diag = 1
 *
 * All patterns are n x n CSR (int64 rowptr, int32 colidx, no values), every column in [0, n); outputs have strictly
 * ascending columns.  What a row of each operand may hold: SUB_q and F rows must be strictly ascending (rows with more
 * than 131072 columns to choose from binary-search the SUB rows, and a repeated frontier node would count its A-row twice
 * towards the row's candidate count); ADD_p and A rows are taken as they are -- any order, repeated columns allowed -- since
 * candidates are only ever united.  A SUB column that is no candidate is ignored.  Nothing of this is checked.
 * Two passes: h2gcn_ring_count writes out_rowptr[0..n] (row pointers of the result) and returns the number of
 * nonzeros (it synchronises the stream -- the caller has to allocate out_colidx); h2gcn_ring_fill, called with the
 * SAME inputs, writes the columns.  `scratch` is h2gcn_ring_scratch_bytes(n) bytes of device memory.
 * F == NULL (f_rowptr NULL) means "no expansion"; a_* may then be NULL as well.
 */
size_t h2gcn_ring_scratch_bytes(int64_t n);
int h2gcn_ring_count(int64_t n, const int64_t* a_rowptr_dev, const int32_t* a_colidx_dev,
                     const int64_t* f_rowptr_dev, const int32_t* f_colidx_dev,
                     int n_add, const int64_t* const* add_rowptr_dev, const int32_t* const* add_colidx_dev, int add_diag,
                     int n_sub, const int64_t* const* sub_rowptr_dev, const int32_t* const* sub_colidx_dev, int sub_diag,
                     int64_t* out_rowptr_dev, int64_t* nnz_out, void* scratch_dev, size_t scratch_bytes, void* stream);
int h2gcn_ring_fill(int64_t n, const int64_t* a_rowptr_dev, const int32_t* a_colidx_dev,
                    const int64_t* f_rowptr_dev, const int32_t* f_colidx_dev,
                    int n_add, const int64_t* const* add_rowptr_dev, const int32_t* const* add_colidx_dev, int add_diag,
                    int n_sub, const int64_t* const* sub_rowptr_dev, const int32_t* const* sub_colidx_dev, int sub_diag,
                    const int64_t* out_rowptr_dev, int32_t* out_colidx_dev, void* scratch_dev, size_t scratch_bytes,
                    void* stream);
/*
 * The same for a ROW WINDOW [row_begin, row_begin + n_rows) -- what one rank of a row-partitioned run needs (SURVEY.md
 * 8(e)): F, ADD, SUB and the result are CSRs of that window (n_rows + 1 local row pointers each), A is the whole n x n
 * matrix (the frontier names global ids), {i} is the global row id.  Ring k of the window needs the whole A and the
 * window's rows of the lower rings only, so each rank builds 1/P of every ring (the reference builds everything on one
 * host, _dataset.py:147-157).  h2gcn_ring_count / _fill are the window [0, n).
 */
int h2gcn_ring_count_rows(int64_t n, int64_t row_begin, int64_t n_rows, const int64_t* a_rowptr_dev, const int32_t* a_colidx_dev,
                          const int64_t* f_rowptr_dev, const int32_t* f_colidx_dev,
                          int n_add, const int64_t* const* add_rowptr_dev, const int32_t* const* add_colidx_dev, int add_diag,
                          int n_sub, const int64_t* const* sub_rowptr_dev, const int32_t* const* sub_colidx_dev, int sub_diag,
                          int64_t* out_rowptr_dev, int64_t* nnz_out, void* scratch_dev, size_t scratch_bytes, void* stream);
int h2gcn_ring_fill_rows(int64_t n, int64_t row_begin, int64_t n_rows, const int64_t* a_rowptr_dev, const int32_t* a_colidx_dev,
                         const int64_t* f_rowptr_dev, const int32_t* f_colidx_dev,
                         int n_add, const int64_t* const* add_rowptr_dev, const int32_t* const* add_colidx_dev, int add_diag,
                         int n_sub, const int64_t* const* sub_rowptr_dev, const int32_t* const* sub_colidx_dev, int sub_diag,
                         const int64_t* out_rowptr_dev, int32_t* out_colidx_dev, void* scratch_dev, size_t scratch_bytes,
                         void* stream);
/*
 * Values of a hop matrix given as a square CSR PATTERN (every stored entry is 1, as nhoodSplit produces):
 *   mode 0 ORDINARY: 1;  mode 1 SYM: fp32((s[deg_i] * 1.0) * s[deg_j]);  mode 2 RW: fp32(s[deg_i] * 1.0)
 * with deg = the row lengths of THIS matrix (reference: D = rowsum(A_k) of that hop matrix, :115-123) and
 * s_table[k] = the fp64 scaling of a row with k entries (k^-1/2 resp. k^-1, inf -> 0), supplied by the caller -- the
 * Python front end computes it with the reference's own numpy call, which keeps the fp64 products and the fp32 cast
 * of sparse2Tensor (:528-535) bit-identical to the reference.  s_table_len > max row length (checked).
 */
int h2gcn_hop_normalize(int64_t n, const int64_t* rowptr_dev, const int32_t* colidx_dev, int mode,
                        const double* s_table_dev, int64_t s_table_len, float* vals_dev, void* stream);
/* Row-window form: the pattern holds n_rows rows of the matrix; col_len_dev[j] = length of row j of the WHOLE matrix
 * (needed by SYM for s[deg_j]; NULL = the pattern is the whole square matrix).  Both calls check every row length
 * against s_table_len on the device and return H2GCN_ERR_INVALID_ARGUMENT when the table is too short (they
 * synchronise the stream for that). */
int h2gcn_hop_normalize_rows(int64_t n_rows, const int64_t* rowptr_dev, const int32_t* colidx_dev, int mode,
                             const double* s_table_dev, int64_t s_table_len, const int64_t* col_len_dev,
                             float* vals_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The classifier side of a training step: keras `Dropout(rate)` followed by the output `Dense` -- `D0.5-MO` of the
 * network-setup DSL (reference h2gcn/models/H2GCN.py:235-257 builds the two layers, :308-325 calls them in order) -- as
 * ONE pass over the [N, K] concat buffer per direction, on the fp32 matrix cores (h2gcn_amd/csrc/classifier.hip):
 *
 *     forward    Z[n, c]  = sum_k D[n, k] * W[k, c] + bias[c]          D[n, k] = keep(n, k) ? X[n, k] / keep_prob : 0
 *     backward   dX[n, k] = keep(n, k) ? (sum_c G[n, c] * W[k, c]) / keep_prob : 0
 *                dW[k, c] = sum_n D[n, k] * G[n, c]                     (db = column sums of G: left to the caller)
 *   The mask is a SELECT in every kernel (matrix-core and small-operand alike), never a multiplication by 0: a dropped element of
 *   D or dX is exactly 0 even where X or the sum over c is Inf / NaN.
 *
 * The dropout mask is COUNTER-BASED, recomputed wherever it is needed instead of stored.  One keyed hash per aligned group
 * of four columns of a row:
 *     gid = n * ceil(K / 4) + k / 4  (64-bit),
 *     h = lo32(gid) ^ rotl16(hi32(gid)) ^ key0;  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= key1;  h ^= h >> 15;  h *= 0x846CA68B;
 *     w0 = h ^ (h >> 16)                                                                              (all mod 2^32)
 *     key0 = mix(lo32(seed) ^ mix(lo32(step) + 0x9E3779B9)),   key1 = mix(hi32(seed) ^ hi32(step) ^ key0 ^ 0x85EBCA6B),
 *     mix(h): h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16
 *   T = floor(keep_prob * 65536).  T a multiple of 256 (keep_prob a multiple of 1/256: 0.5, 0.75, 0.875, ...):
 *     keep(n, k)  <=>  byte (k % 4) of w0  <  T / 256                                                  (8-bit fields)
 *   otherwise  w1 = mix(w0 ^ 0x85EBCA6B),  field = (w0 & 0xffff, w0 >> 16, w1 & 0xffff, w1 >> 16),
 *     keep(n, k)  <=>  field[k % 4] < T                                                                (16-bit fields)
 * The survivors' 1 / keep_prob scale is applied to the finished sums (Z, dW) or at the store (dX).
 * `step` is read from DEVICE memory (*step_dev; NULL = 0) so that a captured hipGraph draws a fresh mask on every replay
 * (the caller bumps the counter with a stream-ordered op); the backward call must see the value its forward saw.
 * keep_prob = 1 switches the mask off (evaluation).  TensorFlow's stateful RNG stream cannot be reproduced by any other
 * implementation, so parity with the reference is statistical here (keep rate) and exact for everything that is a
 * function of the mask (oracle/classifier.py restates the generator bit for bit).
 *
 *   X        fp32 [n_rows, K], row stride ldx (any 4-byte aligned base / stride)      W   fp32 [K, C] contiguous, C <= 64
 *   G        fp32 [n_rows, C], row stride ldg                                         dX  fp32 [n_rows, K], row stride lddx, or NULL
 *   dW       fp32 [K, C] contiguous (overwritten), or NULL; partial sums are added in a fixed order (deterministic)
 *   workspace  h2gcn_dropout_dense_workspace_bytes(n_rows, K, C) bytes, 16-byte aligned, used by this call on `stream`
 * Arithmetic: v_mfma_f32_16x16x4_f32, i.e. exact fp32 multiply-adds (no reduced precision); the summation order over k
 * (forward), c (dX) and rows (dW) is fixed by the shapes.
 */
/* Operands of at most this many rows (default 12288) with C <= 16 classes are latency-bound and take three plain kernels instead
 * of the matrix-core ones (same mask, same scale placement, deterministic; Cora: ~18 -> ~5 us per pass).  Sets the bound when
 * rows >= 0 (0 = never; a process-wide tunable, meant for tests and measurements) and returns the previous one. */
int64_t h2gcn_dropout_dense_small_rows(int64_t rows);
size_t h2gcn_dropout_dense_workspace_bytes(int64_t n_rows, int32_t k, int32_t c);
int h2gcn_dropout_dense_f32(const float* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                            const float* bias_dev, float keep_prob, uint64_t seed, const int64_t* step_dev,
                            float* Z_dev, int64_t ldz, void* workspace_dev, size_t workspace_bytes, void* stream);
int h2gcn_dropout_dense_backward_f32(const float* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                     const float* G_dev, int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                     float* dX_dev, int64_t lddx, float* dW_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream);
/*
 * The same two calls on a bf16 X (an additive extension of ABI 5: look the symbols up before calling a build that may predate
 * them).  X is the bf16 concat buffer a bf16 propagation leaves behind (h2gcn_spmm_hops_bf16 with a bf16 output); W, bias, G,
 * Z, dW and every accumulation stay fp32; dX is written as dx_dtype = H2GCN_DTYPE_BF16 or H2GCN_DTYPE_F32.  Same argument
 * order as the _f32 pair (dx_dtype in front of dX_dev), strides in ELEMENTS, the workspace of
 * h2gcn_dropout_dense_workspace_bytes, the same h2gcn_dropout_dense_small_rows bound.
 * Arithmetic: a lane loads four bf16 with one 8-byte load and widens them exactly (bf16 -> fp32 is a 16-bit shift); from there
 * on the kernels ARE the fp32 ones -- v_mfma_f32_16x16x4_f32, the same mask generator, the same placement of the 1 / keep_prob
 * scale, the same summation orders and fixed-order dW reduction.  Hence:
 *   Z and dW   bit-identical to the _f32 entry points called on the upcast X (X.float())
 *   dX fp32    bit-identical to the _f32 call;   dX bf16   that value rounded to nearest even (torch's .to(torch.bfloat16)),
 *              after mask and scale, two at a time (v_cvt_pk_bf16_f32), one 8-byte store per lane and row tile
 * Layout: X (and a bf16 dX) needs a 4-byte aligned base and an even row stride, so that every 8-byte access is dword-aligned; K
 * may be odd (the tail of a row is loaded and stored by element).  Arguments are validated before the device is touched: a NULL
 * operand, a dx_dtype other than the two above, an odd ldx / lddx or a misaligned base give H2GCN_ERR_INVALID_ARGUMENT with a
 * message that names the argument.  hipGraph capture: no condition (these launches allocate nothing).
 */
int h2gcn_dropout_dense_bf16(const uint16_t* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                             const float* bias_dev, float keep_prob, uint64_t seed, const int64_t* step_dev,
                             float* Z_dev, int64_t ldz, void* workspace_dev, size_t workspace_bytes, void* stream);
int h2gcn_dropout_dense_backward_bf16(const uint16_t* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                      const float* G_dev, int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                      int dx_dtype, void* dX_dev, int64_t lddx, float* dW_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream);
/*
 * The four calls restricted to a SELECTION of rows (an additive extension of ABI 5: look the symbols up before calling a build
 * that may predate them).  A semi-supervised loss lives on the labelled rows only, so its logit gradient is zero everywhere
 * else: these calls compute the logits of, and the gradient through, n_sel selected rows and touch no other row of X.
 * Arguments: those of the full calls, followed by
 *   rows_dev  int32 [n_sel], ASCENDING and UNIQUE, every entry in [0, n_rows) -- guaranteed by the caller (not checked on the
 *             device; h2gcn_amd's HopPlan.select_rows builds and checks such a list)
 *   n_sel     its length (0 <= n_sel <= n_rows; 0: dW is zero-filled, nothing else is written)
 * X stays the full [n_rows, K] matrix; Z, G and dX are COMPACT, one row per list entry.  With r = rows_dev[i]:
 *     forward    Z_c[i, c]  = sum_k D[r, k] * W[k, c] + bias[c]                         Z_c  fp32 [n_sel, C], row stride ldz
 *     backward   dX_c[i, k] = keep(r, k) ? (sum_c G_c[i, c] * W[k, c]) / keep_prob : 0  G_c  fp32 [n_sel, C], row stride ldg
 *                dW[k, c]   = sum_i D[rows_dev[i], k] * G_c[i, c]                       dX_c [n_sel, K], row stride lddx, or NULL
 * The dropout mask is keyed by the ORIGINAL row r (gid = r * ceil(K / 4) + k / 4), not by i, and every summation over k and c
 * runs in the full call's order.  Hence, for fp32 and bf16 X alike:
 *   Z_c    bit-identical to rows rows_dev[] of the full call's Z
 *   dX_c   bit-identical to rows rows_dev[] of the full call's dX when that call gets G_c scattered into a zero [n_rows, C] G
 *   dW     deterministic (fixed-order reduction over the list); equal to the full call's dW on the scattered G up to the
 *          summation tree over rows, not bit for bit
 * The small-operand rule (h2gcn_dropout_dense_small_rows) applies to n_rows, the row count of X -- a row-selected call runs the
 * kernels the full call on the same X runs, however short the list is: the two kernel families sum in different orders, and the
 * bit identities above hold between calls of one family only.  The workspace is
 * h2gcn_dropout_dense_workspace_bytes(n_sel, K, C).  Arguments are validated before the device is touched -- a negative
 * n_sel or n_rows, n_sel > n_rows, a NULL rows_dev with n_sel > 0, a NULL operand and the layout rules of the full calls give
 * H2GCN_ERR_INVALID_ARGUMENT with a message that names the argument.  hipGraph capture: no condition (nothing is allocated,
 * rows_dev is read by the kernels only).
 */
int h2gcn_dropout_dense_rows_f32(const float* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                 const float* bias_dev, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                 float* Z_dev, int64_t ldz, void* workspace_dev, size_t workspace_bytes, void* stream,
                                 const int32_t* rows_dev, int64_t n_sel);
int h2gcn_dropout_dense_rows_bf16(const uint16_t* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                  const float* bias_dev, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                  float* Z_dev, int64_t ldz, void* workspace_dev, size_t workspace_bytes, void* stream,
                                  const int32_t* rows_dev, int64_t n_sel);
int h2gcn_dropout_dense_backward_rows_f32(const float* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                          const float* G_dev, int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                          float* dX_dev, int64_t lddx, float* dW_dev, void* workspace_dev, size_t workspace_bytes,
                                          void* stream, const int32_t* rows_dev, int64_t n_sel);
int h2gcn_dropout_dense_backward_rows_bf16(const uint16_t* X_dev, int64_t ldx, int64_t n_rows, int32_t k, const float* W_dev, int32_t c,
                                           const float* G_dev, int64_t ldg, float keep_prob, uint64_t seed, const int64_t* step_dev,
                                           int dx_dtype, void* dX_dev, int64_t lddx, float* dW_dev, void* workspace_dev,
                                           size_t workspace_bytes, void* stream, const int32_t* rows_dev, int64_t n_sel);

/* ------------------------------------------------------------------------------------------------------------
 * Masked softmax cross-entropy and masked accuracy (reference h2gcn/models/_metrics.py:8-25; called per mask by train_step /
 * test_step, h2gcn/models/H2GCN.py:66-74, 77-107) in ONE pass over the logits (h2gcn_amd/csrc/metrics.hip).  A "set" m is a
 * label matrix Y_m [n_rows, C] (one-hot or all-zero rows; any non-negative rows work) plus a row-weight vector w_m [n_rows]
 * -- the reference's `mask / mean(mask) / n_rows`, i.e. mask / sum(mask); a row-partitioned run divides by the GLOBAL sum:
 *
 *     loss[m] = sum_n w_m[n] * ( - sum_c Y_m[n, c] * log_softmax(Z[n])[c] )
 *     acc[m]  = sum_n w_m[n] * [ argmax_c Z[n, c] == argmax_c Y_m[n, c] ]          (first maximum on ties)
 *
 * Rows whose weight is zero in every set are not read; a label matrix is read only at the rows of non-zero weight.  Per-row
 * terms are fp32, the sums over rows run in fp64 per workgroup and are combined in a fixed order (deterministic).
 * Accuracy at any offset: softmax cross-entropy is shift-invariant, and both kernels work on the SHIFTED logits z_c - max_c z --
 * the row's term is (sum_c Y_c) * log(sum_c exp(z_c - max)) - sum_c Y_c * (z_c - max), the softmax of the gradient is
 * exp((z_c - max) - log(sum)) -- like the reference's tf.nn.softmax_cross_entropy_with_logits.  The error of a row's term
 * therefore does not grow with the magnitude of the logits (unnormalised features, confident late-epoch models): the tolerances
 * that hold for logits around 0 hold for logits around 1e6.
 * DIVERGENCE from the reference on non-finite logits: the reference MULTIPLIES every row's term by its mask weight
 * (_metrics.py:12-14, 22-24), so a NaN / Inf logit in a row the mask excludes still yields NaN there (0 * NaN); here such a
 * row is skipped and the result stays finite.  Rows the mask includes propagate NaN / Inf exactly as the reference does, so a
 * diverged model is still visible through any set that covers the affected rows.
 * h2gcn_masked_ce_backward_f32 is the gradient of loss (one set) with respect to Z, times the scalar *gscale_dev (NULL = 1):
 *     dZ[n, c] = g * w[n] * ( softmax(Z[n])[c] * sum_c' Y[n, c'] - Y[n, c] )     (rows of weight 0: zeros).
 *   Z  fp32 [n_rows, C] row stride ldz, C <= 64      Y, ldy, w  HOST arrays of n_sets (<= H2GCN_METRICS_MAX_SETS) device pointers /
 *   strides      loss_out, acc_out  DEVICE fp32 [n_sets] (acc_out may be NULL)      workspace  h2gcn_masked_metrics_workspace_bytes(n_rows)
 */
#define H2GCN_METRICS_MAX_SETS 4
size_t h2gcn_masked_metrics_workspace_bytes(int64_t n_rows);
int h2gcn_masked_metrics_f32(const float* Z_dev, int64_t ldz, int64_t n_rows, int32_t c, int32_t n_sets, const float* const* Y_dev,
                             const int64_t* ldy, const float* const* w_dev, float* loss_out_dev, float* acc_out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int h2gcn_masked_ce_backward_f32(const float* Z_dev, int64_t ldz, int64_t n_rows, int32_t c, const float* Y_dev, int64_t ldy,
                                 const float* w_dev, const float* gscale_dev, float* dZ_dev, int64_t lddz, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The reference's optimizer step: Keras Adam as `optimizer.apply_gradients` runs it (reference h2gcn/models/H2GCN.py:62-63, 73;
 * TensorFlow's ApplyAdam, a third-party kernel absent from the reference tree), for ALL parameter tensors in one launch:
 *     alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)                          t = 1-based step, all arithmetic fp32
 *     m += (g - m) * (1 - beta_1);  v += (g*g - v) * (1 - beta_2);  param -= (m * alpha) / (sqrt(v) + epsilon)
 * (epsilon joins the UNCORRECTED sqrt(v): Keras / TensorFlow semantics, not torch.optim.Adam's).  params / grads / m / v / sizes
 * are HOST arrays of n_tensors device pointers / element counts (contiguous fp32 tensors; m and v zero before step 1).
 * t is read from *step_dev when step_dev != NULL (device memory: the caller bumps it with a stream-ordered op, so a captured
 * hipGraph advances it on every replay), else from `step`.
 */
#define H2GCN_ADAM_MAX_TENSORS 16   /* tensors per launch; longer lists are processed in groups */
int h2gcn_adam_keras_f32(int32_t n_tensors, float* const* params_dev, const float* const* grads_dev, float* const* m_dev,
                         float* const* v_dev, const int64_t* sizes, float lr, float beta1, float beta2, float epsilon,
                         const int64_t* step_dev, int64_t step, void* stream);

/* The same step with the keras `regularizers.l2(w)` of the dense kernels (reference h2gcn/models/H2GCN.py:239-240, 247-248) folded
 * in: l2 is a HOST array of n_tensors coefficients (0 = tensor not regularised; NULL = none) and the update uses
 * g + 2 * l2 * param as the gradient -- with the roundings of autograd's separate multiply and add, so a run that keeps the
 * penalty out of the autograd graph and passes it here follows the one that does not bit for bit.  h2gcn_l2_penalty_f32 is the
 * VALUE of that penalty, sum_k l2[k] * sum(param_k^2) (fp64 inside a tensor, fp32 across tensors in order), for the loss a step
 * reports (H2GCN.py:363-367): one launch for up to H2GCN_ADAM_MAX_TENSORS tensors.  workspace: h2gcn_l2_penalty_workspace_bytes()
 * bytes of device memory, 8-byte aligned, ZERO before its first use (the kernel re-arms it); out_dev: one float. */
int h2gcn_adam_keras_l2_f32(int32_t n_tensors, float* const* params_dev, const float* const* grads_dev, float* const* m_dev,
                            float* const* v_dev, const int64_t* sizes, const float* l2, float lr, float beta_1, float beta_2,
                            float epsilon, const int64_t* step_dev, int64_t step, void* stream);
size_t h2gcn_l2_penalty_workspace_bytes(void);
int h2gcn_l2_penalty_f32(int32_t n_tensors, const float* const* params_dev, const int64_t* sizes, const float* l2,
                         float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row-shard exchange between the GPUs of one node (no counterpart in the reference: it is single-process,
 * single-device -- SURVEY.md 8(e) adds the row partition).  Before a hop aggregation every rank needs the whole
 * embedding X[N, d] while it owns only X[rows_p, :]; this object performs that all-gather WITHOUT a collective
 * library: every rank stages its shard into a buffer it has exported with hipIpcGetMemHandle, tells its peers
 * (a sequence number stored into their flag words over xGMI), and pulls the peers' shards straight out of their
 * exported buffers -- either with copy-engine transfers (hipMemcpyAsync device-to-device, one stream per peer:
 * no CU is used, every point-to-point xGMI link carries its own transfer) or with one small copy kernel.
 * It is an alternative to ncclAllGather behind the same Python interface (h2gcn_amd/partition.py); which is
 * faster is a property of the node and is measured, not assumed (bench.py).
 *
 * Life cycle (one object per rank, all ranks make the same calls in the same order):
 *   create -> export (blob) -> [blobs of all ranks are exchanged by the caller, e.g. torch.distributed
 *   all_gather_object] -> connect -> { allgather_begin(channel) ... allgather_end(channel) }* -> [caller
 *   barrier] -> destroy.
 * A "channel" is an independent double-buffered send slot with its own sequence counter (the feature-chunk
 * pipeline uses one channel per chunk).  Nothing here blocks the host; a peer that never posts makes the waiting
 * GPU give up after `timeout_ms` and the failure is reported by h2gcn_xchg_status().
 */
typedef struct h2gcn_xchg h2gcn_xchg_t;

#define H2GCN_XCHG_BLOB_BYTES 192          /* size of the opaque blob h2gcn_xchg_export writes                  */
#define H2GCN_XCHG_COPY_ENGINE 0           /* mode: pulls are hipMemcpyAsync D2D on one stream per peer (SDMA)  */
#define H2GCN_XCHG_COPY_KERNEL 1           /* mode: pulls are one copy kernel reading the peers' memory         */

/*   world, rank      number of ranks / this rank (one rank per process; peers must be other processes)
 *   n_channels       independent slots (1..64)
 *   slot_bytes       capacity of one slot = the largest shard (rows_per_rank * width * 4) posted on a channel
 *   mode             H2GCN_XCHG_COPY_ENGINE or H2GCN_XCHG_COPY_KERNEL
 *   timeout_ms       how long a GPU waits for a peer's shard before giving up (0 = default 10000)            */
int h2gcn_xchg_create(int world, int rank, int n_channels, size_t slot_bytes, int mode, int timeout_ms,
                      h2gcn_xchg_t** out);
/* Writes H2GCN_XCHG_BLOB_BYTES bytes describing this rank's exported buffers. */
int h2gcn_xchg_export(const h2gcn_xchg_t* x, void* blob_out);
/* `blobs` = the world blobs in rank order (world * H2GCN_XCHG_BLOB_BYTES bytes); opens every peer's buffers. */
int h2gcn_xchg_connect(h2gcn_xchg_t* x, const void* blobs);
/*
 * Start the all-gather of one shard on `channel`:
 *   src_dev   this rank's rows, fp32 [rows, width] with row stride ld_src (elements); rows <= rows_per_rank
 *   full_dev  destination, fp32 [world * rows_per_rank, width] contiguous; rank q's shard lands in rows
 *             [q*rows_per_rank, (q+1)*rows_per_rank) (rows beyond a short last shard are zero)
 *   stream    the stream that produced src_dev; the staging copy and the notification are ordered on it, and
 *             the pulls (internal streams) start only after everything enqueued on it so far -- so a kernel that
 *             is still reading full_dev from the previous use is safe.
 * Returns immediately.  Exactly one allgather_end must follow before the next begin on the same channel. */
int h2gcn_xchg_allgather_begin(h2gcn_xchg_t* x, int channel, const float* src_dev, int64_t ld_src, int64_t rows,
                               int64_t rows_per_rank, int32_t width, float* full_dev, void* stream);
/* The same in two halves, for pipelines over several channels: `post` stages and announces (ordered on `stream`),
 * `pull` issues the pulls (same rows_per_rank / width / full_dev).  Posting ALL channels before pulling any keeps a
 * later channel's announcement from queueing behind an earlier channel's wait when streams share a hardware queue.
 * begin == post immediately followed by pull. */
int h2gcn_xchg_allgather_post(h2gcn_xchg_t* x, int channel, const float* src_dev, int64_t ld_src, int64_t rows,
                              int64_t rows_per_rank, int32_t width, float* full_dev, void* stream);
int h2gcn_xchg_allgather_pull(h2gcn_xchg_t* x, int channel, int64_t rows_per_rank, int32_t width, float* full_dev);
/* Halo form of the pull (copy-kernel mode, width % 4 == 0): from peer q only the rows rows_dev[q][0 .. counts[q]) (ascending LOCAL
 * row ids of q's shard, int32, device memory; rows_dev / counts are HOST arrays of `world` entries, the own rank's is ignored) -- the
 * rows of the embedding this rank's hop matrices really name.  Rows not listed stay untouched in full_dev.  Same protocol, same
 * allgather_end.  Dense pulls remain the right thing whenever (nearly) every row is named: the synthetic shapes, products-like 2-hop rings. */
int h2gcn_xchg_allgather_pull_rows(h2gcn_xchg_t* x, int channel, int64_t rows_per_rank, int32_t width, float* full_dev,
                                   const int32_t* const* rows_dev, const int64_t* counts);
/* Make `stream` wait (device-side, no host block) until every shard of `channel` has landed in full_dev. */
int h2gcn_xchg_allgather_end(h2gcn_xchg_t* x, int channel, void* stream);
/*
 * The mirror image for the backward pass: every rank holds a full-height contribution src_dev
 * [world * rows_per_rank, width] (contiguous) -- the shard adjoint A_k[rows_p, :]^T dY_p -- and needs the sum over
 * ranks of ITS row block: out_dev[r, :] = sum_q src_q[rank * rows_per_rank + r, :].  Same protocol: the matrix is
 * staged into the exported slot (slot_bytes must cover the whole matrix), announced, and every rank pulls its block
 * out of every peer's slot; `end` sums the blocks in ascending rank order (deterministic) on `stream`.
 * Shares the channel's sequence counter with the all-gather: every rank must issue the same sequence of calls.
 */
int h2gcn_xchg_reduce_scatter_begin(h2gcn_xchg_t* x, int channel, const float* src_dev, int64_t rows_per_rank,
                                    int32_t width, float* out_dev, void* stream);
int h2gcn_xchg_reduce_scatter_end(h2gcn_xchg_t* x, int channel, void* stream);
/*
 * hipGraph capture (H2GCN_XCHG_COPY_KERNEL only): every call above may be issued on a capturing stream -- sequence
 * numbers and slot parity live in device memory, so a replayed graph advances the protocol exactly like an eager call
 * (all ranks must replay the same graphs in the same order).  Call h2gcn_xchg_reset_dependencies() right before a
 * capture begins, with the device idle: the object then forgets the events of earlier (un-captured or other-capture)
 * steps, which a capturing stream must not wait on; whole graphs are ordered by the stream they are replayed on.
 * Copy-engine mode cannot be captured (hipMemcpyAsync needs the slot address on the host).
 */
int h2gcn_xchg_reset_dependencies(h2gcn_xchg_t* x);
/* H2GCN_OK, or H2GCN_ERR_EXCHANGE_TIMEOUT if any wait on this object has ever given up (results are then
 * undefined).  Does not synchronise: call after the streams involved have been synchronised. */
int h2gcn_xchg_status(const h2gcn_xchg_t* x);
/* Release everything.  The caller must make sure (barrier) that no peer is still pulling from this rank. */
void h2gcn_xchg_destroy(h2gcn_xchg_t* x);

#ifdef __cplusplus
}
#endif
#endif /* H2GCN_HIP_H_ */
