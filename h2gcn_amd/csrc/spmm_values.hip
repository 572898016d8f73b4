// spmm_values.hip -- the hop aggregation on values that are an ARGUMENT of the launch, with an optional head dimension:
//
//     forward    Y[i, s, c] = sum_e  V_s[e, h(c)] * X[j_e, c]                      e over row i of selected hop s
//     adjoint    dX[j, c]   = sum_s sum_e' V_s[perm_s[e'], h(c)] * dY[i_e', s, c]  e' over row j of A_s^T
//
// with h(c) = c / (d / n_heads).  The plan gives the PATTERN only (rowptr / colidx, for the adjoint the transposed arrays and
// their permutation): its stored values are never read and nothing in it changes, so two attention layers can share one plan
// and a launch may run next to others of the same plan.  fp32 only; no accumulate flag, no epilogue, no workspace.  A
// translation unit of its own: no existing kernel is compiled differently because of it.
//
// Mapping (gfx950, wave64; gather-bound, no atomics, no inline assembly; LDS on the long path only) -- the geometry of sddmm.hip:
//   * 16 lanes x 4 columns cover a 64-column block; the 4 lane groups of a wave gather 4 neighbour rows per load instruction;
//   * group gi serves the entries = gi (mod 4) of a 64-entry chunk, in ascending order: its accumulators ARE the partial
//     P[gi] of the canonical tree (include/h2gcn_hip.h, "Floating point");
//   * a lane keeps up to four blocks (256 columns) of accumulators; a wider d walks the segment again per 256-column pass;
//   * column ids (and perm, and for n_heads == 1 the values) are fetched 64 at a time -- lane (gi, q) loads entry 4q + gi --
//     and handed out with ds_bpermute; the gathers of a batch of rounds (8 load instructions) go out before the first FMA;
//   * with heads a lane needs V[e, h] for the head of every block it holds: one 4-byte load per (round, block), the same
//     address in all lanes of a group whose columns lie in one head (a broadcast from one cache line);
//   * the fold is lane ^ 16, then lane ^ 32 (v_permlane16_swap / v_permlane32_swap): (P0 + P1) + (P2 + P3) in every group --
//     fp32 addition commutes, so the four groups end with the same bits -- and group gi stores block gi;
//   * a segment (adjoint: a row) of the plan's long list belongs to a workgroup: wave w takes the chunks = w (mod 4) of every
//     segment it serves, and the four wave totals cross through LDS (4 KiB per column pass): ((T0 + T1) + T2) + T3.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "segment_ops.hip.h"

namespace h2gcn {
namespace spmm_values {

using namespace pattern;
constexpr int kBlockCols = 64;   // columns one lane group covers per load: 16 lanes x 4
constexpr int kMaxBlocks = 4;    // 64-column blocks of accumulators a lane keeps (one column pass: 256 columns)
constexpr int kLoads = 8;        // gather instructions in flight per batch of rounds (8 KiB per wave)

struct Params {
    Geom geom;                                // of the walked operand: A_k (forward) or A_k^T (adjoint)
    const int32_t* colidx[H2GCN_MAX_HOPS];    // its column ids: the gathered row of every walked entry (the selected hops, packed)
    const uint32_t* perm[H2GCN_MAX_HOPS];     // adjoint: the forward entry behind every walked entry
    const float* vals[H2GCN_MAX_HOPS];        // element (e, h) at vals[s][e * ldv_entry[s] + h * ldv_head[s]], e a FORWARD entry
    int64_t ldv_entry[H2GCN_MAX_HOPS], ldv_head[H2GCN_MAX_HOPS];
    int d, n_heads, head_cols;                // head_cols = d / n_heads
    const float* src;                         // X [n_cols, d] (forward) / dY [n_rows, n_sel, d] (adjoint)
    int64_t ld_src, ld_src_hop;               // (ld_src_hop: adjoint only)
    float* dst;                               // Y [n_rows, n_sel, d] (forward) / dX [n_cols, d] (adjoint)
    int64_t ld_dst, ld_dst_hop;               // (ld_dst_hop: forward only)
};

// sum over the lanes {l, l^16}, then {l, l^32}: (P[gi] + P[gi^1]) + (P[gi^2] + P[gi^3])
__device__ __forceinline__ float fold_groups(float v) {
    unsigned u = __float_as_uint(v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    u = __float_as_uint(v);
    auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// One batch of U rounds of a chunk: group gi serves entry 4r + gi in round r.  FULL: every round of the batch exists.  All the
// gathers of the batch go out before its first FMA; an entry beyond `count` loads (a clamped, valid address) and adds nothing.
template <bool ADJ, bool HEADS, int NB, int U, bool FULL>
__device__ __forceinline__ void batch(const Params& p, const float* src, const float* vals, int64_t ldv_entry, const int64_t (&hoff)[NB],
                                      int cbase, int r0, int rounds, int count, int64_t ebase, int mycol, uint32_t myidx, float myval,
                                      int lane, Quad (&acc)[NB]) {
    constexpr int NV = HEADS ? NB : 1;
    const int q = lane & 15, gi = lane >> 4;
    Quad xv[U][NB];
    float vv[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
            const int r = r0 + u;
            const int from = ((lane & 48) + r) << 2;
            const int c = __builtin_amdgcn_ds_bpermute(from, mycol);
            const float* xrow = src + (int64_t)c * p.ld_src;
            if (HEADS) {
                const int n = 4 * r + gi < count ? 4 * r + gi : count - 1;
                const int64_t e = ADJ ? (int64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)myidx) : ebase + n;
                const float* vrow = vals + e * ldv_entry;
#pragma unroll
                for (int b = 0; b < NB; ++b) vv[u][b] = vrow[hoff[b]];
            } else {
                vv[u][0] = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(myval)));
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) xv[u][b] = load_quad(xrow, cbase + b * kBlockCols + 4 * q, p.d);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
            if (4 * (r0 + u) + gi < count) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float v = vv[u][HEADS ? b : 0];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[b].v[k] = __builtin_fmaf(v, xv[u][b].v[k], acc[b].v[k]);
                }
            }
        }
    }
}

// `count` (1..64) consecutive walked entries of selected hop s, the first one entry `ebase`: every entry goes into the partial
// of its group, in ascending order.  All 64 lanes must be active.
template <bool ADJ, bool HEADS, int NB, int U>
__device__ __forceinline__ void walk_chunk(const Params& p, int s, const float* src, const int64_t (&hoff)[NB], int cbase, int64_t ebase,
                                           int count, int lane, Quad (&acc)[NB]) {
    const int q = lane & 15, gi = lane >> 4;
    const int my_n = q * 4 + gi;
    const int64_t me = ebase + (my_n < count ? my_n : count - 1);
    const int mycol = p.colidx[s][me];
    const uint32_t myidx = ADJ ? p.perm[s][me] : 0u;
    const float* vals = p.vals[s];
    const int64_t ldv_entry = p.ldv_entry[s];
    float myval = 0.f;
    if (!HEADS) myval = vals[(ADJ ? (int64_t)myidx : me) * ldv_entry];
    const int rounds = (count + 3) >> 2;
    int r0 = 0;
    for (; r0 + U <= rounds; r0 += U)
        batch<ADJ, HEADS, NB, U, true>(p, src, vals, ldv_entry, hoff, cbase, r0, rounds, count, ebase, mycol, myidx, myval, lane, acc);
    if (r0 < rounds)
        batch<ADJ, HEADS, NB, U, false>(p, src, vals, ldv_entry, hoff, cbase, r0, rounds, count, ebase, mycol, myidx, myval, lane, acc);
}

// The 64-entry chunks chunk0, chunk0 + step, ... of the walked entries [beg, end) of selected hop s, columns cbase .. of the pass.
template <bool ADJ, bool HEADS, int NB, int U>
__device__ __forceinline__ void walk_segment(const Params& p, int s, const int (&head)[NB], int cbase, int64_t beg, int64_t end, int chunk0,
                                             int step, int lane, Quad (&acc)[NB]) {
    const float* src = p.src + (ADJ ? (int64_t)s * p.ld_src_hop : 0);
    int64_t hoff[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) hoff[b] = HEADS ? head[b] * p.ldv_head[s] : 0;
    for (int64_t c = beg + (int64_t)chunk0 * kWave; c < end; c += (int64_t)step * kWave) {
        const int count = (int)(end - c < kWave ? end - c : kWave);
        walk_chunk<ADJ, HEADS, NB, U>(p, s, src, hoff, cbase, c, count, lane, acc);
    }
}

// The head of every block of the pass for this lane's quad (a quad beyond d: the last head, its sums are never stored).
template <int NB>
__device__ __forceinline__ void pass_heads(const Params& p, int cbase, int q, int (&head)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int h = (cbase + b * kBlockCols + 4 * q) / p.head_cols;
        head[b] = h < p.n_heads ? h : p.n_heads - 1;
    }
}

template <int NB>
__device__ __forceinline__ void clear(Quad (&acc)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[b].v[k] = 0.f;
}

// (P0 + P1) + (P2 + P3) of every accumulator; returns the quad of block gi (the one this lane's group stores).
template <int NB>
__device__ __forceinline__ Quad fold_blocks(const Quad (&acc)[NB], int gi) {
    Quad mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) mine.v[k] = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = fold_groups(acc[b].v[k]);
            if (gi == b) mine.v[k] = t;
        }
    return mine;
}

template <bool ADJ, bool HEADS, int NB>
__global__ __launch_bounds__(kBlock) void spmm_values_kernel(const Params p) {
    constexpr int U = kLoads / NB;
    constexpr int kPassCols = NB * kBlockCols;
    __shared__ float lds[kWavesPerBlock][kPassCols];   // the long path: the wave totals of one column pass
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 15, gi = lane >> 4;
    int head[NB];
    Quad acc[NB];
    if ((int)blockIdx.x < p.geom.n_long) {
        // ---- a long segment (forward) / every selected hop of a long row (adjoint): 64-entry chunks over the 4 waves ----
        const int64_t e = p.geom.long_list[blockIdx.x];
        const int64_t row = ADJ ? e : e >> 4;
        const int s0 = ADJ ? 0 : (int)(e & 15), s1 = ADJ ? p.geom.n_sel : s0 + 1;
        float* out = p.dst + row * p.ld_dst + (ADJ ? 0 : (int64_t)s0 * p.ld_dst_hop);
        for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
            clear(acc);
            pass_heads(p, cbase, q, head);
            for (int s = s0; s < s1; ++s)
                walk_segment<ADJ, HEADS, NB, U>(p, s, head, cbase, p.geom.rowptr[s][row], p.geom.rowptr[s][row + 1], wave, kWavesPerBlock,
                                                lane, acc);
            const Quad mine = fold_blocks(acc, gi);
            if (gi < NB) {
#pragma unroll
                for (int k = 0; k < 4; ++k) lds[wave][gi * kBlockCols + 4 * q + k] = mine.v[k];
            }
            __syncthreads();
            const int c = threadIdx.x;
            if (c < kPassCols && cbase + c < p.d) out[cbase + c] = ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
            __syncthreads();
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
        int64_t beg, end;
        if (ADJ) {
            // one output row: the partials run on across the selected hops; a row that is long in any of them has its own block
            bool is_long = false;
            for (int s = 0; s < p.geom.n_sel; ++s) {
                segment(p.geom, rp, s, i, &beg, &end);
                is_long = is_long || end - beg >= p.geom.long_threshold;
            }
            if (is_long) continue;
            float* out = p.dst + (row0 + i) * p.ld_dst;
            for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                clear(acc);
                pass_heads(p, cbase, q, head);
                for (int s = 0; s < p.geom.n_sel; ++s) {
                    segment(p.geom, rp, s, i, &beg, &end);
                    walk_segment<ADJ, HEADS, NB, U>(p, s, head, cbase, beg, end, 0, 1, lane, acc);
                }
                const Quad mine = fold_blocks(acc, gi);
                if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
            }
        } else {
            for (int s = 0; s < p.geom.n_sel; ++s) {
                segment(p.geom, rp, s, i, &beg, &end);
                if (end - beg >= p.geom.long_threshold) continue;
                float* out = p.dst + (row0 + i) * p.ld_dst + (int64_t)s * p.ld_dst_hop;
                for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                    clear(acc);
                    pass_heads(p, cbase, q, head);
                    walk_segment<ADJ, HEADS, NB, U>(p, s, head, cbase, beg, end, 0, 1, lane, acc);
                    const Quad mine = fold_blocks(acc, gi);   // (an empty segment: +0)
                    if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
template <bool ADJ, bool HEADS>
void launch(const Params& p, int64_t n_blocks, hipStream_t stream) {
    const dim3 grid((unsigned)n_blocks), block(kBlock);
    // blocks of accumulators a lane keeps: the narrowest geometry that covers d in one column pass, four blocks beyond 256 columns
    // (the bits are the same for all three: every column has its own tree)
    if (p.d <= kBlockCols) hipLaunchKernelGGL((spmm_values_kernel<ADJ, HEADS, 1>), grid, block, 0, stream, p);
    else if (p.d <= 2 * kBlockCols) hipLaunchKernelGGL((spmm_values_kernel<ADJ, HEADS, 2>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((spmm_values_kernel<ADJ, HEADS, kMaxBlocks>), grid, block, 0, stream, p);
}

// The launch behind both entry points.  src / dst: X / Y (forward), dY / dX (adjoint).
template <bool ADJ>
int run(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* values, const int64_t* ldv_entry, const int64_t* ldv_head,
        int32_t n_heads, const float* src, int64_t ld_src, int64_t ld_src_hop, int32_t d, float* dst, int64_t ld_dst, int64_t ld_dst_hop,
        void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        const uint32_t* perm[H2GCN_MAX_HOPS] = {};
        int st = ADJ ? adjoint_view(plan, hop_mask, &v, perm) : pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
        if (n_heads < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d", n_heads);
        if (d % n_heads) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d is not a multiple of n_heads = %d", d, n_heads);
        if (n_heads > 1 && (d / n_heads) % 4)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "d / n_heads = %d is not a multiple of 4 (a lane's four columns must lie in one head)",
                        d / n_heads);
        if (ADJ) {
            if (ld_dst < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ld_dst, d);
            if (ld_src < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_row = %lld < d = %d", (long long)ld_src, d);
            if (ld_src_hop < 0 || (v.n_sel > 1 && ld_src_hop < d))
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_hop = %lld < d = %d: the hops' gradients would overlap", (long long)ld_src_hop, d);
        } else {
            if (ld_src < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ld_src, d);
            if (ld_dst < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_row = %lld < d = %d", (long long)ld_dst, d);
            if (ld_dst_hop < 0 || (v.n_sel > 1 && ld_dst_hop < d))
                return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldy_hop = %lld < d = %d: hop outputs would overlap", (long long)ld_dst_hop, d);
        }
        if (v.n_rows == 0) return H2GCN_OK;   // nothing to store
        if (!dst) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s is NULL", ADJ ? "dX" : "Y");
        if (selected_nnz(v) > 0 && !src) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s is NULL", ADJ ? "dY" : "X");
        if (dst == src) return fail(H2GCN_ERR_INVALID_ARGUMENT, "%s", ADJ ? "dX aliases dY" : "Y aliases X");
        if (selected_nnz(v) > 0 && (!ldv_entry || !ldv_head)) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldv_entry / ldv_head is NULL");
        if ((st = check_hop_arrays(v, "values", values)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks, ADJ)) != H2GCN_OK) return st;
        if (n_blocks == 0) {   // a selection without nonzeros: every row is empty
            const int n_slots = ADJ ? 1 : v.n_sel;
            for (int s = 0; s < n_slots; ++s)
                H2GCN_HIP_TRY(hipMemset2DAsync(dst + (int64_t)s * ld_dst_hop, (size_t)ld_dst * sizeof(float), 0, (size_t)d * sizeof(float),
                                               (size_t)v.n_rows, stream));
            return H2GCN_OK;
        }
        for (int s = 0; s < v.n_sel; ++s) {
            p.colidx[s] = v.colidx[s];
            p.perm[s] = perm[s];
            p.vals[s] = values[s];
            p.ldv_entry[s] = ldv_entry[s];
            p.ldv_head[s] = ldv_head[s];
        }
        p.d = d;
        p.n_heads = n_heads;
        p.head_cols = d / n_heads;
        p.src = src, p.ld_src = ld_src, p.ld_src_hop = ld_src_hop;
        p.dst = dst, p.ld_dst = ld_dst, p.ld_dst_hop = ld_dst_hop;
        if (n_heads > 1) launch<ADJ, true>(p, n_blocks, stream);
        else launch<ADJ, false>(p, n_blocks, stream);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in spmm_hops_%svalues_f32", ADJ ? "T_" : "");
    }
}

}  // namespace spmm_values
}  // namespace h2gcn

extern "C" {

int h2gcn_spmm_hops_values_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* values_dev, const int64_t* ldv_entry,
                               const int64_t* ldv_head, int32_t n_heads, const float* X_dev, int64_t ldx, int32_t d, float* Y_dev,
                               int64_t ldy_row, int64_t ldy_hop, void* stream) {
    return h2gcn::spmm_values::run<false>(plan, hop_mask, values_dev, ldv_entry, ldv_head, n_heads, X_dev, ldx, 0, d, Y_dev, ldy_row,
                                          ldy_hop, stream);
}

int h2gcn_spmm_hops_T_values_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* const* values_dev, const int64_t* ldv_entry,
                                 const int64_t* ldv_head, int32_t n_heads, const float* dY_dev, int64_t ldg_row, int64_t ldg_hop, int32_t d,
                                 float* dX_dev, int64_t ldx, void* stream) {
    return h2gcn::spmm_values::run<true>(plan, hop_mask, values_dev, ldv_entry, ldv_head, n_heads, dY_dev, ldg_row, ldg_hop, d, dX_dev,
                                         ldx, 0, stream);
}

}  // extern "C"
