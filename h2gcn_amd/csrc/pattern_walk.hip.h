// pattern_walk.hip.h -- the frame of sddmm.hip and row_softmax.hip, the kernels that walk the CSR PATTERN of the selected hops:
// blocks [0, n_long) serve one segment each of the plan's forward long-segment list (>= long_threshold entries); the blocks after
// them walk row tiles of 4 waves x rows_per_wave rows, every XCD a contiguous range of tiles, and skip the long segments.
#pragma once

#include "capi_internal.h"

namespace h2gcn {
namespace pattern {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;
constexpr int kNumXcd = 8;

struct Geom {
    const int64_t* rowptr[H2GCN_MAX_HOPS];   // the selected hops, packed
    int n_sel;
    int64_t n_rows;
    const int64_t* long_list;   // row << 4 | s per long segment
    int n_long, long_threshold, rows_per_wave;
    int64_t n_tiles, tiles_per_xcd;
};

__device__ __forceinline__ int64_t readlane64(int64_t v, int src) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t bpermute64(int64_t v, int src) {
    const uint32_t lo = __builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
struct Add {
    static __device__ __forceinline__ float op(float a, float b) { return a + b; }
};

// xor butterfly over lane distances 1, 2, 4, 8 of a 16-lane group, every step `v op partner`: afterwards its 16 lanes hold the
// same bits (row_half_mirror / row_ror:8 read from lanes that hold the partner's value).  All 64 lanes must be active.
template <typename Op>
__device__ __forceinline__ float bfly16(float v) {
    v = Op::op(v, dpp<0xB1>(v));    // quad_perm [1,0,3,2]: lane ^ 1
    v = Op::op(v, dpp<0x4E>(v));    // quad_perm [2,3,0,1]: lane ^ 2
    v = Op::op(v, dpp<0x141>(v));   // row_half_mirror: lane ^ 4 up to a permutation of equals
    v = Op::op(v, dpp<0x128>(v));   // row_ror:8: lane ^ 8
    return v;
}

// Whether this block serves a long segment, and which: row `row` of selected hop `s`, entries [beg, end).
__device__ __forceinline__ bool long_segment(const Geom& g, uint32_t block, int64_t* row, int* s, int64_t* beg, int64_t* end) {
    if ((int)block >= g.n_long) return false;
    const int64_t e = g.long_list[block];
    *row = e >> 4, *s = (int)(e & 15);
    *beg = g.rowptr[*s][*row], *end = g.rowptr[*s][*row + 1];
    return true;
}

// The lane of wave_rows' `rp` that holds rowptr_s[row0 + i], i = 0 .. rows_per_wave.
__device__ __forceinline__ int rp_lane(const Geom& g, int s, int i) { return s * (g.rows_per_wave + 1) + i; }

// The tile walk of a block that serves no long segment: wave `wave` owns the rows row0 .. row0 + rows_per_wave - 1 below n_rows
// and `rp` holds their row pointers from ONE wave-wide load -- lane rp_lane(g, s, i) has rowptr_s[min(row0 + i, n_rows)]:
// (rows_per_wave + 1) * n_sel <= 64 is an invariant of the plan.  Returns false when the wave has nothing to do.  A segment of
// >= long_threshold entries belongs to a long_segment block: the caller skips it.
__device__ __forceinline__ bool wave_rows(const Geom& g, uint32_t block, int wave, int lane, int64_t* row0, int64_t* rp) {
    const int64_t tb = (int64_t)block - g.n_long;
    const int64_t tile = (tb % kNumXcd) * g.tiles_per_xcd + tb / kNumXcd;
    if (tile >= g.n_tiles) return false;
    const int rpw = g.rows_per_wave;
    *row0 = (tile * kWavesPerBlock + wave) * rpw;
    if (*row0 >= g.n_rows) return false;
    *rp = 0;
    if (lane < (rpw + 1) * g.n_sel) {
        const int s = lane / (rpw + 1), i = lane - s * (rpw + 1);
        const int64_t r = *row0 + i < g.n_rows ? *row0 + i : g.n_rows;
        *rp = g.rowptr[s][r];
    }
    return true;
}

// The entries [beg, end) of row row0 + i in selected hop s, wave-uniform (s and i must be).
__device__ __forceinline__ void segment(const Geom& g, int64_t rp, int s, int i, int64_t* beg, int64_t* end) {
    *beg = readlane64(rp, rp_lane(g, s, i)), *end = readlane64(rp, rp_lane(g, s, i + 1));
}

// ---- the host epilogue of a launcher, after its own operand checks
inline int64_t selected_nnz(const PatternView& v) {
    int64_t nnz = 0;
    for (int s = 0; s < v.n_sel; ++s) nnz += v.nnz[s];
    return nnz;
}

// A table of one device array per selected hop: it may be NULL, and so may its entries, only where there is nothing to store.
template <typename T>
int check_hop_arrays(const PatternView& v, const char* name, T* const* ptrs) {
    if (selected_nnz(v) == 0) return H2GCN_OK;
    if (!ptrs) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s is NULL", name);
    for (int s = 0; s < v.n_sel; ++s)
        if (v.nnz[s] > 0 && !ptrs[s])
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s[%d] is NULL (selected hop %d of the launch has %lld nonzeros)", name, s, s,
                        (long long)v.nnz[s]);
    return H2GCN_OK;
}

// bf16 arrays: 4-byte aligned base, even strides (elements) and an even width (the rule of the bf16 SpMM launches)
inline int check_bf16_layout(const char* what, const void* ptr, int64_t ld_row, int64_t ld_hop, int32_t d) {
    if (reinterpret_cast<uintptr_t>(ptr) & 3u)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: the base address must be 4-byte aligned", what);
    if ((ld_row & 1) || (ld_hop & 1))
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: row / hop strides must be even (got %lld / %lld elements)", what,
                    (long long)ld_row, (long long)ld_hop);
    if (d & 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "bf16 %s: the feature width d must be even (got %d)", what, d);
    return H2GCN_OK;
}

inline int check_dtype(const char* what, int dtype) {
    if (dtype != H2GCN_DTYPE_F32 && dtype != H2GCN_DTYPE_BF16)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s = %d: must be H2GCN_DTYPE_F32 (%d) or H2GCN_DTYPE_BF16 (%d)", what, dtype,
                    H2GCN_DTYPE_F32, H2GCN_DTYPE_BF16);
    return H2GCN_OK;
}

// `width` elements of `elem` bytes in each of `n` rows `ld` elements apart: +0 in either format
inline int zero_rows(void* out, int64_t ld, int64_t width, int64_t n, size_t elem, hipStream_t stream) {
    if (out && n > 0 && width > 0) H2GCN_HIP_TRY(hipMemset2DAsync(out, (size_t)ld * elem, 0, (size_t)width * elem, (size_t)n, stream));
    return H2GCN_OK;
}

// Fills `g` and the grid size (0: nothing to launch).  The first step that touches the device (the long list): checks come before.
// `adjoint`: v is an adjoint_view and the list is the adjoint's -- one entry per row that is long in any selected hop, bare (no
// `<< 4 | s`): long_segment does not read it.
inline int launch_geometry(const h2gcn_plan* plan, const PatternView& v, hipStream_t stream, Geom* g, int64_t* n_blocks,
                           bool adjoint = false) {
    *n_blocks = 0;
    if (selected_nnz(v) == 0 || v.n_rows == 0) return H2GCN_OK;
    const int st = pattern_long_list(plan, v.mask, stream, &g->long_list, &g->n_long, adjoint);
    if (st != H2GCN_OK) return st;
    for (int s = 0; s < v.n_sel; ++s) g->rowptr[s] = v.rowptr[s];
    g->n_sel = v.n_sel;
    g->n_rows = v.n_rows;
    g->long_threshold = v.long_threshold;
    g->rows_per_wave = v.rows_per_wave;
    const int64_t rows_per_tile = (int64_t)g->rows_per_wave * kWavesPerBlock;
    g->n_tiles = (g->n_rows + rows_per_tile - 1) / rows_per_tile;
    g->tiles_per_xcd = (g->n_tiles + kNumXcd - 1) / kNumXcd;
    const int64_t n = (int64_t)g->n_long + g->tiles_per_xcd * kNumXcd;
    if (n > 0x7fffffffLL) return fail(H2GCN_ERR_INVALID_ARGUMENT, "grid too large (%lld blocks)", (long long)n);
    *n_blocks = n;
    return H2GCN_OK;
}

}  // namespace pattern
}  // namespace h2gcn
