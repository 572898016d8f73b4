// sddmm.hip -- the gradient of the hop aggregation with respect to the stored adjacency values: a sampled dense-dense
// product over the CSR pattern of every selected hop (SDDMM),
//
//     dV_s[e] = sum_c dY[i, s, c] * X[j, c]          for every stored entry e = (i, j) of selected hop s.
//
// Stands in for the gradient TensorFlow registers for SparseTensorDenseMatMul wrt the values of its sparse operand (the
// reference never asks for it: its adjacency is constant; a caller with learned / gated / attention edge weights does).
// A translation unit of its own: no existing kernel is compiled differently because of it.
//
// Mapping (gfx950, wave64; gather-bound like the forward launch, no MFMA, no LDS memory, no atomics):
//   * ONE lane geometry: 16 lanes x 4 columns cover a 64-column block of a feature row, so the 4 lane groups of a wave
//     gather 4 neighbour rows of X per load instruction (16 bytes per lane fp32, 8 bytes bf16);
//   * a wave walks the (row, hop) segments of its row tile (the pattern walk of pattern_walk.hip.h).  Per segment it keeps the
//     dY row in registers -- lane (group, quad q) holds columns 4q..4q+3 of up to four 64-column blocks, replicated over the groups;
//   * column ids are fetched 64 at a time -- lane (group gi, quad q) loads entry 4q + gi of the chunk, so the 64 lanes read
//     the chunk's 256 bytes once -- and handed to the group's lanes with ds_bpermute; in round r group gi serves entry
//     4r + gi: a chunk of n entries takes ceil(n / 4) rounds, whatever n;
//   * rounds are issued in batches: all gathers of a batch (8 load instructions fp32 = 8 KiB per wave; bf16 16, or the 8
//     rounds of a one-block row) go out before the first multiply;
//   * the 16 quads of a block are summed by an xor butterfly in DPP (one row of 16 lanes), the lane with q == r keeps the
//     entry's result, and after the last round the 64 results of the chunk leave with ONE store instruction into the chunk's
//     256 bytes of dV;
//   * segments with >= long_row_threshold nonzeros belong to workgroups of their own: the 4 waves take 64-entry chunks in turn.
//     Every result belongs to one entry, so nothing is summed across waves.
//
// Arithmetic (documented in include/h2gcn_hip.h): one order per element, a function of d alone -- see batch / walk_chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "segment_ops.hip.h"

namespace h2gcn {
namespace sddmm {

using namespace pattern;
constexpr int kBlockCols = 64;   // columns one lane group covers per load: 16 lanes x 4
constexpr int kMaxBlocks = 4;    // 64-column blocks of the dY row a lane keeps in registers (one column pass: 256 columns)

struct bf16 {
    uint16_t bits;
};

struct Params {
    Geom geom;
    const int32_t* colidx[H2GCN_MAX_HOPS];   // the selected hops, packed as geom.rowptr
    float* dvals[H2GCN_MAX_HOPS];
    int d;
    const void* g;   // dY, [n_rows, n_sel, d] through ldg_row / ldg_hop (elements)
    int64_t ldg_row, ldg_hop;
    const void* x;   // X, [n_cols, d] through ldx
    int64_t ldx;
};

typedef uint32_t uint2u __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte loads need only dword alignment on gfx950

// Columns c0 .. c0+3 of a feature row, widened to fp32; columns >= d read as +0 and are never loaded.  fp32: segment_ops.hip.h
using pattern::load_quad;
// bf16: d is even and every row starts on a dword, so a quad holds 4, 2 or 0 valid columns
__device__ __forceinline__ Quad load_quad(const bf16* row, int c0, int d) {
    Quad r;
    uint32_t lo = 0, hi = 0;
    if (c0 + 3 < d) {
        const uint2u t = *reinterpret_cast<const uint2u*>(row + c0);
        lo = t.x; hi = t.y;
    } else if (c0 + 1 < d) {
        lo = *reinterpret_cast<const uint32_t*>(row + c0);
    }
    r.v[0] = __uint_as_float(lo << 16); r.v[1] = __uint_as_float(lo & 0xffff0000u);
    r.v[2] = __uint_as_float(hi << 16); r.v[3] = __uint_as_float(hi & 0xffff0000u);
    return r;
}

// One batch of U rounds of a chunk: group gi serves entry 4r + gi in round r.  FULL: every round of the batch exists.
template <typename TS, int NB, int U, bool FULL>
__device__ __forceinline__ void batch(const Params& p, const Quad (&g)[NB], int cbase, int r0, int rounds, int mycol, int lane,
                                      float& res) {
    const int q = lane & 15;
    const TS* x = reinterpret_cast<const TS*>(p.x);
    Quad xv[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
            const int c = __builtin_amdgcn_ds_bpermute(((lane & 48) + r0 + u) << 2, mycol);
            const TS* xrow = x + (int64_t)c * p.ldx;
#pragma unroll
            for (int b = 0; b < NB; ++b) xv[u][b] = load_quad(xrow, cbase + b * kBlockCols + 4 * q, p.d);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                // the total of one 64-column block: the 16 quads' values (dot_quad) summed by the xor butterfly over lane distances
                // 1, 2, 4, 8 (blocks that start at or beyond d hold +0 on both sides: they add +0, as the documented order says)
                const float t = bfly16<Add>(dot_quad(g[b], xv[u][b]));
                if (q == r0 + u) res = res + t;   // block totals in ascending block order, starting from +0
            }
        }
    }
}

// `count` (1..64) consecutive entries of one segment: cols / out point at the chunk's first entry, grow at the segment's dY row.
// Column passes of NB blocks each (one pass up to 64 * NB columns); the entry's running total stays in a register across passes.
template <typename TS, int NB, int U>
__device__ __forceinline__ void walk_chunk(const Params& p, const TS* grow, const int32_t* cols, int count, float* out, int lane) {
    const int q = lane & 15, gi = lane >> 4;
    const int my_n = q * 4 + gi;
    const int mycol = cols[my_n < count ? my_n : count - 1];
    const int rounds = (count + 3) >> 2;
    float res = 0.f;
    for (int cbase = 0; cbase < p.d; cbase += NB * kBlockCols) {
        Quad g[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = load_quad(grow, cbase + b * kBlockCols + 4 * q, p.d);
        int r0 = 0;
        for (; r0 + U <= rounds; r0 += U) batch<TS, NB, U, true>(p, g, cbase, r0, rounds, mycol, lane, res);
        if (r0 < rounds) batch<TS, NB, U, false>(p, g, cbase, r0, rounds, mycol, lane, res);
    }
    if (my_n < count) out[my_n] = res;
}

template <typename TS, int NB>
__global__ __launch_bounds__(kBlock) void sddmm_hops_kernel(const Params p) {
    // rounds per batch: 8 load instructions in flight (fp32: 8 KiB per wave), 16 for bf16 (8 KiB again), at most 8 rounds
    constexpr int kLoads = std::is_same<TS, bf16>::value ? 16 : 8;
    constexpr int U = kLoads / NB < 8 ? kLoads / NB : 8;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TS* g = reinterpret_cast<const TS*>(p.g);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        const TS* grow = g + row * p.ldg_row + (int64_t)s * p.ldg_hop;
        for (int64_t c = beg + (int64_t)wave * kWave; c < end; c += kBlock) {
            const int count = (int)(end - c < kWave ? end - c : kWave);
            walk_chunk<TS, NB, U>(p, grow, p.colidx[s] + c, count, p.dvals[s] + c, lane);
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
            const TS* grow = g + (row0 + i) * p.ldg_row + (int64_t)s * p.ldg_hop;
            for (int64_t c = beg; c < end; c += kWave) {
                const int count = (int)(end - c < kWave ? end - c : kWave);
                walk_chunk<TS, NB, U>(p, grow, p.colidx[s] + c, count, p.dvals[s] + c, lane);
            }
        }
    }
}

template <typename TS>
int sddmm_hops(const h2gcn_plan_t* plan, uint32_t hop_mask, const void* dY, int64_t ldg_row, int64_t ldg_hop, const void* X,
               int64_t ldx, int32_t d, float* const* dvals, void* stream_v) {
    constexpr bool kBf16 = std::is_same<TS, bf16>::value;
    try {
        // every check below comes before the device is touched
        PatternView v;
        int st = pattern_view(plan, hop_mask, &v);
        if (st != H2GCN_OK) return st;
        if (d < 1) return fail(H2GCN_ERR_INVALID_ARGUMENT, "d = %d", d);
        if (ldx < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldx = %lld < d = %d", (long long)ldx, d);
        if (ldg_row < d) return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_row = %lld < d = %d", (long long)ldg_row, d);
        if (ldg_hop < 0 || (v.n_sel > 1 && ldg_hop < d))
            return fail(H2GCN_ERR_INVALID_ARGUMENT, "ldg_hop = %lld < d = %d: the hops' gradients would overlap", (long long)ldg_hop, d);
        if (kBf16) {
            if ((st = check_bf16_layout("dY", dY, ldg_row, ldg_hop, d)) != H2GCN_OK) return st;
            if ((st = check_bf16_layout("X", X, ldx, 0, d)) != H2GCN_OK) return st;
        }
        if (selected_nnz(v) > 0 && !dY) return fail(H2GCN_ERR_INVALID_ARGUMENT, "dY is NULL");
        if (selected_nnz(v) > 0 && !X) return fail(H2GCN_ERR_INVALID_ARGUMENT, "X is NULL");
        if ((st = check_hop_arrays(v, "dvals", dvals)) != H2GCN_OK) return st;
        hipStream_t stream = (hipStream_t)stream_v;
        Params p;
        memset(&p, 0, sizeof(p));
        int64_t n_blocks;
        if ((st = launch_geometry(plan, v, stream, &p.geom, &n_blocks)) != H2GCN_OK) return st;
        if (n_blocks == 0) return H2GCN_OK;
        for (int s = 0; s < v.n_sel; ++s) {
            p.colidx[s] = v.colidx[s];
            p.dvals[s] = dvals[s];
        }
        p.d = d;
        p.g = dY;
        p.ldg_row = ldg_row;
        p.ldg_hop = ldg_hop;
        p.x = X;
        p.ldx = ldx;
        const dim3 grid((unsigned)n_blocks), block(kBlock);
        // blocks of the dY row a lane keeps: the narrowest geometry that covers d in one column pass, four blocks beyond 256
        // columns (the bits are the same for all three: the order of summation is a function of d alone)
        if (d <= kBlockCols) hipLaunchKernelGGL((sddmm_hops_kernel<TS, 1>), grid, block, 0, stream, p);
        else if (d <= 2 * kBlockCols) hipLaunchKernelGGL((sddmm_hops_kernel<TS, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((sddmm_hops_kernel<TS, kMaxBlocks>), grid, block, 0, stream, p);
        H2GCN_HIP_TRY(hipGetLastError());
        return H2GCN_OK;
    } catch (...) {
        return fail(H2GCN_ERR_INTERNAL, "unexpected exception in sddmm_hops_%s", kBf16 ? "bf16" : "f32");
    }
}

}  // namespace sddmm
}  // namespace h2gcn

extern "C" {

int h2gcn_sddmm_hops_f32(const h2gcn_plan_t* plan, uint32_t hop_mask, const float* dY, int64_t ldg_row, int64_t ldg_hop,
                         const float* X, int64_t ldx, int32_t d, float* const* dvals, void* stream) {
    return h2gcn::sddmm::sddmm_hops<float>(plan, hop_mask, dY, ldg_row, ldg_hop, X, ldx, d, dvals, stream);
}

int h2gcn_sddmm_hops_bf16(const h2gcn_plan_t* plan, uint32_t hop_mask, const uint16_t* dY, int64_t ldg_row, int64_t ldg_hop,
                          const uint16_t* X, int64_t ldx, int32_t d, float* const* dvals, void* stream) {
    return h2gcn::sddmm::sddmm_hops<h2gcn::sddmm::bf16>(plan, hop_mask, dY, ldg_row, ldg_hop, X, ldx, d, dvals, stream);
}

}  // extern "C"
