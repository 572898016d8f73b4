// edge_scores_dynamic.hip -- DYNAMIC (GATv2) attention scores on the hop pattern and their backward:
//
//     score[s][e*K + h] = sum_{c in head h} a[s, c] * leaky(u[i, c] + v[j, c])          e = (i, j) a stored entry of selected hop s
//     du[i, c] / dv[j, c] = the row / column sums of dp_c = leaky'(p_c) * ds[s][e*K + h(c)] * a[s, c] over the selected hops
//     da[s, c]            = the sum over the hop's entries of ds[s][e*K + h(c)] * leaky(p_c)
//
// The nonlinearity sits between the gather and the reduction over c, so no composition of the existing launches gives it without an
// nnz x d array: this is the SDDMM's gather with three more VALU operations per element.  A translation unit of its own: no existing
// kernel is compiled differently because of it.  Arithmetic: include/h2gcn_hip.h.
//
// Mapping (gfx950, wave64; the pattern walk of pattern_walk.hip.h, the quads and butterflies of segment_ops.hip.h; no atomics, no scratch):
//   * forward: the lane mapping of sddmm_heads_kernel -- 16 lanes x 4 columns per 64-column block, the four lane groups serve the
//     entries 4r + gi of a 64-entry chunk, column ids fetched 64 at a time and handed out by ds_bpermute, 8 gather instructions in
//     flight before the first ALU use; PACKED forms for w = 4 L in {4, 8, 16, 32} (one full-width gather serves all heads), head-aligned
//     blocks for any other w and for K = 1 (any d).  The hop's `a` row and the segment's `u` row sit in registers beside each other, the
//     dot product's second operand is leaky(u + x).  Long segments: a workgroup each, the four waves taking chunks in turn;
//   * backward, rows (du) and columns (dv): ONE kernel template.  The walked node's row (u_i / v_j) sits in registers (at most four blocks
//     per lane: d <= 256), the other node's row is gathered, ds of the entry's head is one 4-byte load per lane and block; lane group gi
//     accumulates the partial P[gi] of the node's row in registers, two xor steps over lane distances 16 and 32 give (P0 + P1) + (P2 + P3).
//     A row that is long in any selected hop has a workgroup: chunks in turn over the four waves, wave totals through LDS;
//   * backward, da: a launch of its own (coef kernel).  Folding it into the row side would keep 4 NB more accumulators PER SELECTED HOP
//     alive across the row loop (du's order runs the hops inside a row, da's sum runs over the rows inside a hop), or an LDS flush per
//     segment: either costs the row side an occupancy step.  At most kCoefBlocks workgroups stride over the blocks of the forward walk,
//     every one writes ONE partial row per selected hop into the workspace, and a small kernel adds the partial rows in a tree that is a
//     function of the number of workgroups alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "segment_ops.hip.h"

#ifndef H2GCN_NO_FP_CONTRACT
#define H2GCN_NO_FP_CONTRACT _Pragma("clang fp contract(off)")
#endif

namespace h2gcn {
namespace dynamic_scores {

using namespace pattern;

constexpr int kBlockCols = 64;     // columns one lane group covers per load: 16 lanes x 4
constexpr int kMaxWidth = 256;     // four blocks of a node row per lane
constexpr int kCoefBlocks = 2048;  // workgroups of the da launch at most (a multiple of kNumXcd): rows of the workspace per hop

// ====================================================================================================== forward
struct Params {
    Geom geom;
    const int32_t* colidx[H2GCN_MAX_HOPS];   // the selected hops, packed as geom.rowptr
    float* score[H2GCN_MAX_HOPS];            // [nnz_k, K]
    int d, K, w;                             // w = d / K
    const float* u;                          // [n_rows, d] through ldu
    const float* v;                          // [n_cols, d] through ldv
    const float* a;                          // [n_sel, d] through lda
    int64_t ldu, ldv, lda;
    float slope;
};

// q = leaky(u + x), column by column: one fp32 add, one multiply on the slope branch
__device__ __forceinline__ Quad leaky_sum(const Quad& u, const Quad& x, float slope) {
    Quad r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = leaky(u.v[k] + x.v[k], slope);
    return r;
}

// The first steps of bfly16 over the L = w / 4 lanes of one head (the SDDMM's: its remaining steps would add quads of +0).
template <int L>
__device__ __forceinline__ float bfly_head(float t) {
    if (L >= 2) t = t + dpp<0xB1>(t);    // lane ^ 1
    if (L >= 4) t = t + dpp<0x4E>(t);    // lane ^ 2
    if (L >= 8) t = t + dpp<0x141>(t);   // row_half_mirror: lane ^ 4 up to a permutation of equals
    return t;
}

// ---- PACKED, w = 4 L in {4, 8, 16, 32}: `count` (1..64) consecutive entries of one segment, all heads (sddmm_heads_kernel's walk).
template <int L, int NB, int U>
__device__ __forceinline__ void walk_chunk_packed(const Params& p, const float* arow, const float* urow, const int32_t* cols, int count,
                                                  float* out, int lane) {
    constexpr int kKeep = 16 / L;   // totals a lane keeps per block; also the heads of a block
    const int q = lane & 15, gi = lane >> 4;
    const int my_n = q * 4 + gi;
    const int mycol = cols[my_n < count ? my_n : count - 1];
    const int rounds = (count + 3) >> 2;
    for (int cbase = 0; cbase < p.d; cbase += NB * kBlockCols) {
        Quad g[NB], ur[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            g[b] = load_quad<false>(arow, cbase + b * kBlockCols + 4 * q, p.d);
            ur[b] = load_quad<false>(urow, cbase + b * kBlockCols + 4 * q, p.d);
        }
        float res[NB][kKeep];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kKeep; ++k) res[b][k] = 0.f;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += U) {
            if (r0 < rounds) {   // (wave-uniform) a batch: its gathers go out before the first add
                Quad xv[U][NB];
#pragma unroll
                for (int t = 0; t < U; ++t)
                    if (r0 + t < rounds) {
                        const int c = __builtin_amdgcn_ds_bpermute(((lane & 48) + r0 + t) << 2, mycol);
                        const float* xrow = p.v + (int64_t)c * p.ldv;
#pragma unroll
                        for (int b = 0; b < NB; ++b) xv[t][b] = load_quad<false>(xrow, cbase + b * kBlockCols + 4 * q, p.d);
                    }
#pragma unroll
                for (int t = 0; t < U; ++t)
                    if (r0 + t < rounds) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const float tot = bfly_head<L>(dot_quad(g[b], leaky_sum(ur[b], xv[t][b], p.slope)));
                            if ((q & (L - 1)) == ((r0 + t) & (L - 1))) res[b][(r0 + t) / L] = 0.f + tot;   // element = +0 + B_0
                        }
                    }
            }
        }
        // lane (gi, q) holds, per block b and k, head cbase / w + b * kKeep + q / L of entry 4 (k L + q mod L) + gi
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kKeep; ++k) {
                const int n = 4 * (k * L + (q & (L - 1))) + gi;
                const int h = cbase / (4 * L) + b * kKeep + q / L;
                if (n < count && h < p.K) out[(int64_t)n * p.K + h] = res[b][k];
            }
    }
}

// ---- head-aligned blocks, any w (K = 1: any d): the single-head walk on head h's column slice (arow / urow / x at the head's first
// column), the chunk's column ids in `mycol`.  Lane q == r keeps entry 4r + gi.
template <int NB, int U>
__device__ __forceinline__ float walk_chunk_head(const Params& p, const float* arow, const float* urow, const float* x, int mycol, int rounds,
                                                 int lane) {
    const int q = lane & 15;
    float res = 0.f;
    for (int cbase = 0; cbase < p.w; cbase += NB * kBlockCols) {
        Quad g[NB], ur[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            g[b] = load_quad(arow, cbase + b * kBlockCols + 4 * q, p.w);
            ur[b] = load_quad(urow, cbase + b * kBlockCols + 4 * q, p.w);
        }
        for (int r0 = 0; r0 < rounds; r0 += U) {
            Quad xv[U][NB];
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (r0 + t < rounds) {
                    const int c = __builtin_amdgcn_ds_bpermute(((lane & 48) + r0 + t) << 2, mycol);
                    const float* xrow = x + (int64_t)c * p.ldv;
#pragma unroll
                    for (int b = 0; b < NB; ++b) xv[t][b] = load_quad(xrow, cbase + b * kBlockCols + 4 * q, p.w);
                }
#pragma unroll
            for (int t = 0; t < U; ++t)
                if (r0 + t < rounds) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float tot = bfly16<Add>(dot_quad(g[b], leaky_sum(ur[b], xv[t][b], p.slope)));
                        if (q == r0 + t) res = res + tot;   // block totals in ascending block order, starting from +0
                    }
                }
        }
    }
    return res;
}

// L > 0: packed with w = 4 L; L == 0: head-aligned blocks.
template <int L, int NB>
__device__ __forceinline__ void walk_chunk(const Params& p, const float* arow, const float* urow, const int32_t* cols, int count, float* out,
                                           int lane) {
    constexpr int U = 8 / NB;   // rounds per batch: 8 load instructions (8 KiB per wave) in flight
    if constexpr (L > 0) {
        walk_chunk_packed<L, NB, U>(p, arow, urow, cols, count, out, lane);
    } else {
        const int q = lane & 15, gi = lane >> 4;
        const int my_n = q * 4 + gi;
        const int mycol = cols[my_n < count ? my_n : count - 1];
        const int rounds = (count + 3) >> 2;
        for (int h = 0; h < p.K; ++h) {
            const float res = walk_chunk_head<NB, U>(p, arow + h * p.w, urow + h * p.w, p.v + h * p.w, mycol, rounds, lane);
            if (my_n < count) out[(int64_t)my_n * p.K + h] = res;
        }
    }
}

template <int L, int NB>
__global__ __launch_bounds__(kBlock) void edge_scores_dynamic_kernel(const Params p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        const float* urow = p.u + row * p.ldu;
        const float* arow = p.a + (int64_t)s * p.lda;
        for (int64_t c = beg + (int64_t)wave * kWave; c < end; c += kBlock) {
            const int count = (int)(end - c < kWave ? end - c : kWave);
            walk_chunk<L, NB>(p, arow, urow, p.colidx[s] + c, count, p.score[s] + c * p.K, lane);
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
        for (s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            const int64_t len = end - beg;
            if (len <= 0 || len >= p.geom.long_threshold) continue;
            const float* urow = p.u + (row0 + i) * p.ldu;
            const float* arow = p.a + (int64_t)s * p.lda;
            for (int64_t c = beg; c < end; c += kWave) {
                const int count = (int)(end - c < kWave ? end - c : kWave);
                walk_chunk<L, NB>(p, arow, urow, p.colidx[s] + c, count, p.score[s] + c * p.K, lane);
            }
        }
    }
}

// ====================================================================================================== backward
struct BwdParams {
    Geom geom;                              // of the walked operand: A_k (rows, coef) or A_k^T (columns)
    const int32_t* idx[H2GCN_MAX_HOPS];     // its colidx: the OTHER node of every walked entry   (the selected hops, packed)
    const uint32_t* perm[H2GCN_MAX_HOPS];   // column side: the forward entry behind every walked entry
    const float* g[H2GCN_MAX_HOPS];         // dscores [nnz_k, K], in forward entry order
    const float* self;                      // the walked nodes' operand: u (rows, coef) / v (columns) ...
    const float* other;                     // ... and the gathered one
    const float* a;                         // [n_sel, d] through lda
    int64_t ld_self, ld_other, lda;
    float* out;                             // du / dv through ld_out; coef: the workspace, [gridDim.x, n_sel, d]
    int64_t ld_out;
    int64_t n_virtual;                      // coef: blocks of the forward walk the workgroups stride over
    int d, K, w;
    float slope;
};

enum Side { kRows = 0, kCols = 1, kCoef = 2 };

template <int NB>
struct NodeRow {
    Quad v[NB];
};

template <int NB>
__device__ __forceinline__ NodeRow<NB> load_row(const float* row, int d, int lane) {
    NodeRow<NB> r;
#pragma unroll
    for (int b = 0; b < NB; ++b) r.v[b] = load_quad(row, b * kBlockCols + 4 * (lane & 15), d);
    return r;
}
template <int NB>
__device__ __forceinline__ NodeRow<NB> zero_row() {
    NodeRow<NB> r;
#pragma unroll
    for (int b = 0; b < NB; ++b) r.v[b].v[0] = r.v[b].v[1] = r.v[b].v[2] = r.v[b].v[3] = 0.f;
    return r;
}

// The heads of a lane's quads (a quad lies in ONE head: w % 4 == 0, or K == 1); a quad at or beyond d reads no dscore.
template <int NB>
struct Heads {
    int h[NB];
    bool in[NB];
};

// `count` (1..64) consecutive walked entries of selected hop s, starting at e0: lane group gi adds the terms of the entries 4r + gi, in
// ascending r, to acc -- the partial P[gi] of the walked node.  S == kCoef: the terms are ds * q (acc: the hop's da partial).
template <int S, int NB>
__device__ __forceinline__ void add_chunk(const BwdParams& p, int s, const NodeRow<NB>& self, const NodeRow<NB>& a, const Heads<NB>& hd, int64_t e0,
                                          int count, NodeRow<NB>& acc, int lane) {
    H2GCN_NO_FP_CONTRACT
    constexpr int U = 8 / NB;   // rounds per batch: 8 gather instructions in flight
    const int q = lane & 15, gi = lane >> 4;
    const int my_n = q * 4 + gi;
    const int64_t e = e0 + (my_n < count ? my_n : count - 1);
    const int mynode = p.idx[s][e];
    const int64_t myg = (S == kCols ? (int64_t)p.perm[s][e] : e) * p.K;   // the entry's dscores: forward entry order
    const int rounds = (count + 3) >> 2;
    for (int r0 = 0; r0 < rounds; r0 += U) {
        Quad xv[U][NB];
        float gv[U][NB];
#pragma unroll
        for (int t = 0; t < U; ++t)
            if (r0 + t < rounds) {   // (wave-uniform)
                const int src = (lane & 48) + r0 + t;
                const int c = __builtin_amdgcn_ds_bpermute(src << 2, mynode);
                const float* orow = p.other + (int64_t)c * p.ld_other;
                const float* ge = p.g[s] + bpermute64(myg, src);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    xv[t][b] = load_quad(orow, b * kBlockCols + 4 * q, p.d);
                    gv[t][b] = hd.in[b] ? ge[hd.h[b]] : 0.f;
                }
            }
#pragma unroll
        for (int t = 0; t < U; ++t)
            if (r0 + t < rounds) {
                const bool valid = 4 * (r0 + t) + gi < count;
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float pre = S == kCols ? xv[t][b].v[k] + self.v[b].v[k] : self.v[b].v[k] + xv[t][b].v[k];   // u[i] + v[j]
                        float term;
                        if (S == kCoef) {
                            term = gv[t][b] * leaky(pre, p.slope);
                        } else {
                            const float dq = gv[t][b] * a.v[b].v[k];
                            term = pre > 0.f ? dq : dq * p.slope;
                        }
                        if (valid) acc.v[b].v[k] = acc.v[b].v[k] + term;
                    }
            }
    }
}

// (P0 + P1) + (P2 + P3) of the four lane groups' partials, in every lane
template <int NB>
__device__ __forceinline__ void combine_groups(NodeRow<NB>& acc) {
    H2GCN_NO_FP_CONTRACT
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = acc.v[b].v[k];
            t = t + __shfl_xor(t, 16);
            t = t + __shfl_xor(t, 32);
            acc.v[b].v[k] = t;
        }
}

// The four wave totals of a workgroup, added ((T0 + T1) + T2) + T3 per column; every thread of the block must call.  Thread c returns
// column c's total (c < NB * 64).  `lds` is free for the next call on return.
template <int NB>
__device__ __forceinline__ float combine_waves(const NodeRow<NB>& tot, float (*lds)[NB * kBlockCols], int lane, int wave) {
    H2GCN_NO_FP_CONTRACT
    if ((lane >> 4) == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) lds[wave][b * kBlockCols + 4 * lane + k] = tot.v[b].v[k];
    }
    __syncthreads();
    float r = 0.f;
    const int c = threadIdx.x;
    if (c < NB * kBlockCols) r = ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
    __syncthreads();
    return r;
}

template <int NB>
__device__ __forceinline__ Heads<NB> lane_heads(const BwdParams& p, int lane) {
    Heads<NB> hd;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int c0 = b * kBlockCols + 4 * (lane & 15);
        hd.in[b] = c0 < p.d;
        hd.h[b] = hd.in[b] ? c0 / p.w : 0;
    }
    return hd;
}

// du (S == kRows, on A_k) / dv (S == kCols, on A_k^T through its permutation).
template <int S, int NB>
__global__ __launch_bounds__(kBlock) void edge_scores_dynamic_backward_kernel(const BwdParams p) {
    static_assert(S == kRows || S == kCols, "the node sides");
    __shared__ float lds[kWavesPerBlock][NB * kBlockCols];   // long rows: the wave totals
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Heads<NB> hd = lane_heads<NB>(p, lane);
    if ((int)blockIdx.x < p.geom.n_long) {
        // ---- a row that is long in some selected hop: every hop's segment in 64-entry chunks, chunk c to wave c mod 4 ----
        const int64_t e = p.geom.long_list[blockIdx.x];
        const int64_t row = S == kCols ? e : e >> 4;
        if (S == kRows) {   // the forward list names segments: the row's FIRST long segment serves the row (block-uniform)
            for (int s = 0; s < (int)(e & 15); ++s)
                if (p.geom.rowptr[s][row + 1] - p.geom.rowptr[s][row] >= p.geom.long_threshold) return;
        }
        const NodeRow<NB> self = load_row<NB>(p.self + row * p.ld_self, p.d, lane);
        NodeRow<NB> acc = zero_row<NB>();
        for (int s = 0; s < p.geom.n_sel; ++s) {
            const int64_t beg = p.geom.rowptr[s][row], end = p.geom.rowptr[s][row + 1];
            const NodeRow<NB> a = load_row<NB>(p.a + (int64_t)s * p.lda, p.d, lane);
            for (int64_t c = beg + (int64_t)wave * kWave; c < end; c += kBlock)
                add_chunk<S, NB>(p, s, self, a, hd, c, (int)(end - c < kWave ? end - c : kWave), acc, lane);
        }
        combine_groups<NB>(acc);
        const float total = combine_waves<NB>(acc, lds, lane, wave);
        if ((int)threadIdx.x < p.d) p.out[row * p.ld_out + threadIdx.x] = total;
        return;
    }
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
        int64_t beg, end;
        bool is_long = false;
        for (int s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            is_long = is_long || end - beg >= p.geom.long_threshold;
        }
        if (is_long) continue;   // (wave-uniform)
        const int64_t row = row0 + i;
        const NodeRow<NB> self = load_row<NB>(p.self + row * p.ld_self, p.d, lane);
        NodeRow<NB> acc = zero_row<NB>();
        for (int s = 0; s < p.geom.n_sel; ++s) {
            segment(p.geom, rp, s, i, &beg, &end);
            if (end <= beg) continue;
            const NodeRow<NB> a = load_row<NB>(p.a + (int64_t)s * p.lda, p.d, lane);
            for (int64_t c = beg; c < end; c += kWave)
                add_chunk<S, NB>(p, s, self, a, hd, c, (int)(end - c < kWave ? end - c : kWave), acc, lane);
        }
        combine_groups<NB>(acc);   // (a node without entries: +0)
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) store_quad(p.out + row * p.ld_out, b * kBlockCols + 4 * lane, p.d, acc.v[b]);
        }
    }
}

// da, first stage: workgroup g strides over the blocks g, g + gridDim.x, ... of the forward walk, hop by hop, and writes one partial row
// per selected hop: workspace[(g * n_sel + s) * d + c].  The order of a partial depends on the launch geometry, never on the run.
template <int NB>
__global__ __launch_bounds__(kBlock) void edge_scores_dynamic_coef_kernel(const BwdParams p) {
    __shared__ float lds[kWavesPerBlock][NB * kBlockCols];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Heads<NB> hd = lane_heads<NB>(p, lane);
    const NodeRow<NB> none = zero_row<NB>();
    for (int s = 0; s < p.geom.n_sel; ++s) {
        NodeRow<NB> acc = zero_row<NB>();
        for (int64_t vb = blockIdx.x; vb < p.n_virtual; vb += gridDim.x) {
            if (vb < p.geom.n_long) {
                const int64_t e = p.geom.long_list[vb];
                if ((int)(e & 15) != s) continue;
                const int64_t row = e >> 4;
                const int64_t beg = p.geom.rowptr[s][row], end = p.geom.rowptr[s][row + 1];
                const NodeRow<NB> self = load_row<NB>(p.self + row * p.ld_self, p.d, lane);
                for (int64_t c = beg + (int64_t)wave * kWave; c < end; c += kBlock)
                    add_chunk<kCoef, NB>(p, s, self, none, hd, c, (int)(end - c < kWave ? end - c : kWave), acc, lane);
                continue;
            }
            int64_t row0, rp;
            if (!wave_rows(p.geom, (uint32_t)vb, wave, lane, &row0, &rp)) continue;
            for (int i = 0; i < p.geom.rows_per_wave && row0 + i < p.geom.n_rows; ++i) {
                int64_t beg, end;
                segment(p.geom, rp, s, i, &beg, &end);
                if (end <= beg || end - beg >= p.geom.long_threshold) continue;
                const NodeRow<NB> self = load_row<NB>(p.self + (row0 + i) * p.ld_self, p.d, lane);
                for (int64_t c = beg; c < end; c += kWave)
                    add_chunk<kCoef, NB>(p, s, self, none, hd, c, (int)(end - c < kWave ? end - c : kWave), acc, lane);
            }
        }
        combine_groups<NB>(acc);
        const float total = combine_waves<NB>(acc, lds, lane, wave);
        if ((int)threadIdx.x < p.d) p.out[((int64_t)blockIdx.x * p.geom.n_sel + s) * p.d + threadIdx.x] = total;
    }
}

// da, second stage: da[s, c] from the n_part partial rows.  Thread (part, col) of a 16 x 16 block adds the rows part, part + 16, ... into
// four accumulators in turn (row g into accumulator (g / 16) mod 4), (A0 + A1) + (A2 + A3), and the 16 parts are added in ascending order
// from +0: a tree that is a function of n_part alone.
__global__ __launch_bounds__(kBlock) void edge_scores_dynamic_coef_reduce_kernel(const float* partial, int n_part, int n_sel, int d, float* da,
                                                                                 int64_t ldda) {
    H2GCN_NO_FP_CONTRACT
    __shared__ float lds[16][16];
    const int s = blockIdx.y, cl = threadIdx.x & 15, part = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + cl;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (col < d)
        for (int g0 = part; g0 < n_part; g0 += 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = g0 + 16 * k;
                if (g < n_part) acc[k] = acc[k] + partial[((int64_t)g * n_sel + s) * d + col];
            }
        }
    lds[part][cl] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (part == 0 && col < d) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t = t + lds[k][cl];
        da[(int64_t)s * ldda + col] = t;
    }
}

// ====================================================================================================== host
// Workgroups of the da launch: the blocks of the forward tile walk, kCoefBlocks at most -- a function of n_rows and rows_per_wave, so
// that the workspace can be sized without the long-segment list.
int64_t coef_blocks(const PatternView& v) {
    if (v.n_rows <= 0) return 0;
    const int64_t rows_per_tile = (int64_t)v.rows_per_wave * kWavesPerBlock;
    const int64_t n_tiles = (v.n_rows + rows_per_tile - 1) / rows_per_tile;
    const int64_t n = (n_tiles + kNumXcd - 1) / kNumXcd * kNumXcd;
    return n < kCoefBlocks ? n : kCoefBlocks;
}

size_t workspace_bytes(const PatternView& v, int32_t d) { return (size_t)coef_blocks(v) * v.n_sel * d * sizeof(float); }

// The checks the forward and the backward share, in the order of sddmm_hops_heads_f32's.
int check_operands(const PatternView& v, int32_t d, int32_t n_heads, const float* u, int64_t ldu, const float* x, int64_t ldv, const float* a,
                   int64_t lda) {
    if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
    if (n_heads < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "n_heads = %d < 1", n_heads);
    if (d % n_heads) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d is not a multiple of n_heads = %d", d, n_heads);
    if (n_heads > 1 && ((d / n_heads) & 3))
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "with n_heads = %d > 1 the head width d / n_heads = %d must be a multiple of 4", n_heads,
                    d / n_heads);
    if (d > kMaxWidth)
        return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d > %d: the dynamic edge scores keep a node row in registers (four 64-column blocks)", d,
                    kMaxWidth);
    if (ldu < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldu = %lld < d = %d", (long long)ldu, d);
    if (ldv < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldv = %lld < d = %d", (long long)ldv, d);
    if (lda < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lda = %lld < d = %d", (long long)lda, d);
    if (selected_nnz(v) > 0 && !u) return fail(H2GCN_ERR_INVALID_ARGUMENT, "u is NULL");
    if (selected_nnz(v) > 0 && !x) return fail(H2GCN_ERR_INVALID_ARGUMENT, "v is NULL");
    if (selected_nnz(v) > 0 && !a) return fail(H2GCN_ERR_INVALID_ARGUMENT, "a is NULL");
    return H2GCN_OK;
}

int forward(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u, int64_t ldu, const float* x, int64_t ldv, const float* a, int64_t lda,
            int32_t d, int32_t n_heads, float slope, float* const* scores, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_operands(v, d, n_heads, u, ldu, x, ldv, a, lda)) != H2GCN_OK) return st;
        if ((st = check_hop_arrays(v, "scores", scores)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) {
            p.colidx[s] = v.colidx[s];
            p.score[s] = scores[s];
        }
        const int w = d / n_heads;
        p.d = d, p.K = n_heads, p.w = w;
        p.u = u, p.ldu = ldu;
        p.v = x, p.ldv = ldv;
        p.a = a, p.lda = lda;
        p.slope = slope;
        const dim3 grid((unsigned)n_blocks), block(kBlock);
        // (the bits do not depend on the geometry: the order of summation is a function of w alone)
        if (n_heads > 1 && w == 4) hipLaunchKernelGGL((edge_scores_dynamic_kernel<1, 1>), grid, block, 0, stream, p);
        else if (n_heads > 1 && w == 8) hipLaunchKernelGGL((edge_scores_dynamic_kernel<2, 2>), grid, block, 0, stream, p);
        else if (n_heads > 1 && w == 16) hipLaunchKernelGGL((edge_scores_dynamic_kernel<4, 2>), grid, block, 0, stream, p);
        else if (n_heads > 1 && w == 32) hipLaunchKernelGGL((edge_scores_dynamic_kernel<8, 2>), grid, block, 0, stream, p);
        else if (w <= kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_kernel<0, 1>), grid, block, 0, stream, p);
        else if (w <= 2 * kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_kernel<0, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((edge_scores_dynamic_kernel<0, 4>), grid, block, 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_dynamic_hops_f32");
    }
}

template <int S>
int launch_side(const BwdParams& p, int64_t n_blocks, hipStream_t stream) {
    const dim3 grid((unsigned)n_blocks), block(kBlock);
    if (p.d <= kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_backward_kernel<S, 1>), grid, block, 0, stream, p);
    else if (p.d <= 2 * kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_backward_kernel<S, 2>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((edge_scores_dynamic_backward_kernel<S, 4>), grid, block, 0, stream, p);
    H2GCN_HIP_TRY(hipGetLastError());
    return H2GCN_OK;
}

int backward(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u, int64_t ldu, const float* x, int64_t ldv, const float* a, int64_t lda,
             int32_t d, int32_t n_heads, float slope, const float* const* g, float* du, int64_t lddu, float* dv, int64_t lddv, float* da,
             int64_t ldda, void* workspace, size_t ws_bytes, void* stream_v) {
    try {
        // every check below comes before the device is touched
        PatternView v, tv;
        const uint32_t* perm[H2GCN_MAX_HOPS] = {};
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if ((st = check_operands(v, d, n_heads, u, ldu, x, ldv, a, lda)) != H2GCN_OK) return st;
        if (!du && !dv && !da) return fail(H2GCN_ERR_INVALID_ARGUMENT, "du, dv and da are all NULL: nothing to compute");
        if (du && lddu < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddu = %lld < d = %d", (long long)lddu, d);
        if (dv && lddv < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "lddv = %lld < d = %d", (long long)lddv, d);
        if (da && ldda < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldda = %lld < d = %d", (long long)ldda, d);
        if ((st = check_hop_arrays(v, "dscores", g)) != H2GCN_OK) return st;
        const size_t need = da ? workspace_bytes(v, d) : 0;
        if (need > 0 && !workspace) return fail(H2GCN_ERR_INVALID_ARGUMENT, "workspace is NULL (da needs %zu bytes)", need);
        if (need > ws_bytes)
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "workspace_bytes = %zu < %zu (h2gcn_edge_scores_dynamic_workspace_bytes)", ws_bytes, need);
        if (dv && (st = adjoint_view(plan, hop_mask, &tv, perm)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        BwdParams rows, cols;
        memset(&rows, 0, sizeof(rows));
        memset(&cols, 0, sizeof(cols));
        int64_t n_rows_blocks = 0, n_cols_blocks = 0;
        if ((du || da) && (st = launch_geometry(plan, v, stream, &rows.geom, &n_rows_blocks)) != H2GCN_OK) return st;
        if (dv && (st = launch_geometry(plan, tv, stream, &cols.geom, &n_cols_blocks, true)) != H2GCN_OK) return st;
        if (selected_nnz(v) == 0 || v.n_rows == 0) {   // a selection without nonzeros: every sum is empty
            if ((st = zero_rows(du, lddu, d, v.n_rows, sizeof(float), stream)) != H2GCN_OK) return st;
            if ((st = zero_rows(dv, lddv, d, v.n_cols, sizeof(float), stream)) != H2GCN_OK) return st;
            return zero_rows(da, ldda, d, v.n_sel, sizeof(float), stream);
        }
        rows.self = u, rows.ld_self = ldu, rows.other = x, rows.ld_other = ldv;
        cols.self = x, cols.ld_self = ldv, cols.other = u, cols.ld_other = ldu;
        for (BwdParams* p : {&rows, &cols}) {
            p->a = a, p->lda = lda;
            p->d = d, p->K = n_heads, p->w = d / n_heads;
            p->slope = slope;
            for (int s = 0; s < v.n_sel; ++s) p->g[s] = g[s];
        }
        for (int s = 0; s < v.n_sel; ++s) {
            rows.idx[s] = v.colidx[s];
            if (dv) cols.idx[s] = tv.colidx[s], cols.perm[s] = perm[s];
        }
        if (du) {
            rows.out = du, rows.ld_out = lddu;
            if ((st = launch_side<kRows>(rows, n_rows_blocks, stream)) != H2GCN_OK) return st;
        }
        if (dv) {
            cols.out = dv, cols.ld_out = lddv;
            if ((st = launch_side<kCols>(cols, n_cols_blocks, stream)) != H2GCN_OK) return st;
        }
        if (da) {
            BwdParams coef = rows;
            const int64_t n_part = coef_blocks(v);
            coef.out = (float*)workspace, coef.ld_out = d;
            coef.n_virtual = n_rows_blocks;
            const dim3 grid((unsigned)n_part), block(kBlock);
            if (d <= kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_coef_kernel<1>), grid, block, 0, stream, coef);
            else if (d <= 2 * kBlockCols) hipLaunchKernelGGL((edge_scores_dynamic_coef_kernel<2>), grid, block, 0, stream, coef);
            else hipLaunchKernelGGL((edge_scores_dynamic_coef_kernel<4>), grid, block, 0, stream, coef);
            H2GCN_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(edge_scores_dynamic_coef_reduce_kernel, dim3((unsigned)((d + 15) / 16), (unsigned)v.n_sel), block, 0, stream,
                               (const float*)workspace, (int)n_part, v.n_sel, d, da, ldda);
            H2GCN_HIP_TRY(hipGetLastError());
        }
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in edge_scores_dynamic_backward_hops_f32");
    }
}

}  // namespace dynamic_scores
}  // namespace h2gcn

extern "C" {

size_t h2gcn_edge_scores_dynamic_workspace_bytes(const h2gcn_plan_t* plan, uint32_t hop_mask, int32_t d) {
    h2gcn::PatternView v;
    if (d < 1 || d > h2gcn::dynamic_scores::kMaxWidth || h2gcn::pattern_view(plan, hop_mask, &v) != H2GCN_OK) return 0;
    return h2gcn::dynamic_scores::workspace_bytes(v, d);
}

int h2gcn_edge_scores_dynamic_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u_dev, int64_t ldu, const float* v_dev,
                                       int64_t ldv, const float* a_dev, int64_t lda, int32_t d, int32_t n_heads, float negative_slope,
                                       float* const* scores_dev, void* stream) {
    return h2gcn::dynamic_scores::forward(plan, hop_mask, u_dev, ldu, v_dev, ldv, a_dev, lda, d, n_heads, negative_slope, scores_dev, stream);
}

int h2gcn_edge_scores_dynamic_backward_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* u_dev, int64_t ldu,
                                                const float* v_dev, int64_t ldv, const float* a_dev, int64_t lda, int32_t d, int32_t n_heads,
                                                float negative_slope, const float* const* dscores_dev, float* du_dev, int64_t lddu,
                                                float* dv_dev, int64_t lddv, float* da_dev, int64_t ldda, void* workspace_dev,
                                                size_t workspace_bytes, void* stream) {
    return h2gcn::dynamic_scores::backward(plan, hop_mask, u_dev, ldu, v_dev, ldv, a_dev, lda, d, n_heads, negative_slope, dscores_dev, du_dev,
                                           lddu, dv_dev, lddv, da_dev, ldda, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
