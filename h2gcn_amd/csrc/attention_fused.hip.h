// attention_fused.hip.h -- the fused attention forward (attention_fused.hip has the description): its device functions and the ONE
// segment walk, `forward_walk`, that the kernels of attention_fused.hip, attention_stats.hip (+ the softmax statistics),
// and attention_bf16.hip (a bf16 x) wrap (attention_dropout.hip keeps a copy of it with the dropout factors, for a measured reason), and the one host launch path behind their
// entry points.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "attention_dropout.hip.h"
#include "segment_ops.hip.h"

namespace h2gcn {
namespace attention_fused {

using namespace pattern;
constexpr int kBlockCols = 64;   // columns one lane group covers per load: 16 lanes x 4
constexpr int kMaxBlocks = 4;    // 64-column blocks of accumulators a lane keeps (one column pass: 256 columns)
constexpr int kMaxHeads = 16;    // K beyond it is refused: the tile is 64 x kMaxHeads floats per wave

// Gather instructions in flight per batch of rounds, by the element type of x: 8 KiB per wave on an fp32 x.  A bf16 quad is 8 bytes,
// so 16 would keep those 8 KiB in flight -- and did, at 177 VGPRs and 2 waves per SIMD in the 128-column geometry against 115 and 4
// (the row addresses and the coefficients of twice the rounds), 1.5x the fp32 launch's time at the products shape.  8 keeps the fp32
// kernel's registers and occupancy, and the launch then runs in 0.84x the fp32 time (profiles/r24_attention_bf16_step.txt).  So the value
// is 8 for both element types today; it stays a trait of TX because the right depth is a property of the element size (the backward's
// chunk_dots does take 16 on bf16), and a specialisation is where the next element type or a retuned bf16 depth goes.
template <typename TX>
struct Loads {
    static constexpr int value = 8;
};

// TX / TY: the element types of the wide operands (float, or bf16_t: attention_bf16.hip).  l, r and everything walk A touches
// are fp32 whatever they are.
template <typename TX = float, typename TY = TX>
struct ParamsT {
    using X = TX;
    Geom geom;
    const int32_t* colidx[H2GCN_MAX_HOPS];   // the selected hops, packed as geom.rowptr
    const float* l;                          // [n_rows, n_sel, K]: element (i, s, h) at i * ldl + s * K + h
    const float* r;                          // [n_cols, n_sel, K]
    const TX* x;                             // [n_cols, d] through ldx
    TY* y;                                   // [n_rows, n_sel, d] through ldy_row / ldy_hop
    int64_t ldl, ldr, ldx, ldy_row, ldy_hop;
    int d, K, head_cols;                     // head_cols = d / K
    float slope;
};
using Params = ParamsT<>;

// The LDS of a block.  NB: 64-column blocks of a column pass.
template <int NB>
struct Shared {
    float tile[kWavesPerBlock][kWave * kMaxHeads];   // per wave: alpha of the chunk at hand, element (n, h) at n * K + h
    float stat[kWavesPerBlock][2 * kMaxHeads];       // per wave (long path: [0]): m of head h at [h], 1/S at [kMaxHeads + h]
    float red[2][kWavesPerBlock][4];                 // long path: wave maxima / wave totals of the head group at hand
    float tot[kWavesPerBlock][NB * kBlockCols];      // long path: the wave totals of one column pass
};

// ---- the last two butterfly steps of the softmax's reductions (the scalars and the 16-lane steps: segment_ops.hip.h)
// v[lane] op v[lane ^ 16], then the same over lane ^ 32: the last two steps of the xor butterfly.  v_permlane16_swap / v_permlane32_swap
// hand a lane its partner's value without an LDS round trip; both operations commute, so which of the pair comes first is the same
// bits (the maximum up to the sign of a zero, which no exponential sees: score - (+-0) differs from score only for score = +-0,
// and exp2 of either zero is 1).
template <typename Op>
__device__ __forceinline__ float bfly_groups(float v) {
    unsigned u = __float_as_uint(v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = Op::op(__uint_as_float(a[0]), __uint_as_float(a[1]));
    u = __float_as_uint(v);
    auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return Op::op(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float bfly64_add(float v) { return bfly_groups<Add>(bfly16<Add>(v)); }
__device__ __forceinline__ float bfly64_max(float v) { return bfly_groups<Max>(bfly16<Max>(v)); }

// What one lane writes into LDS another lane of the same wave reads next: a wave's LDS operations complete in order, the fence
// keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Heads h0 .. h0 + nh - 1 (nh in 1..4, wave-uniform) of a node row at `row` (its head 0): absent heads read as +0.
__device__ __forceinline__ void load_heads(const float* row, int h0, int nh, float (&v)[4]) {
    float a, b = 0.f, c = 0.f, e = 0.f;
    if (nh == 4) {
        const float4u t = *reinterpret_cast<const float4u*>(row + h0);
        a = t.x, b = t.y, c = t.z, e = t.w;
    } else {
        a = row[h0];
        if (nh > 1) b = row[h0 + 1];
        if (nh > 2) c = row[h0 + 2];
    }
    v[0] = a, v[1] = b, v[2] = c, v[3] = e;
}

// The scores of the head group of the entry whose column is `col`: lv = l[i, s, h0 ..].
template <typename P>
__device__ __forceinline__ void group_scores(const P& p, int s, int col, int h0, int nh, const float (&lv)[4], float (&sc)[4]) {
    float rv[4];
    load_heads(p.r + (int64_t)col * p.ldr + (int64_t)s * p.K, h0, nh, rv);
#pragma unroll
    for (int k = 0; k < 4; ++k) sc[k] = leaky(lv[k] + rv[k], p.slope);
}

// (m, 1/S) of heads h0 .. h0 + nh - 1 of a segment of `len` >= 1 entries whose column ids start at `cols`, on NW waves: NW = 1 the
// calling wave alone; NW = 4 every thread of the block must call, wave w takes the chunks = w (mod 4) and `red` is free again on
// return.  All lanes return the same values.
template <int NW, typename P>
__device__ __forceinline__ void group_stats(const P& p, int s, const int32_t* cols, int64_t len, int h0, int nh, const float (&lv)[4],
                                            int lane, int wave, float (*red)[kWavesPerBlock][4], float (&m)[4], float (&rinv)[4]) {
    constexpr int NA = 4 / NW;   // partials a lane keeps per head
    const int64_t first = NW == 1 ? 0 : (int64_t)wave * kWave;
    float mx[4];
    bool nn[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mx[k] = neg_inf(), nn[k] = false;
    for (int64_t j0 = first; j0 < len; j0 += NW * kWave) {   // (wave-uniform)
        const bool ok = j0 + lane < len;
        float sc[4];
        group_scores(p, s, cols[ok ? j0 + lane : j0], h0, nh, lv, sc);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok) {
                mx[k] = fmaxf(mx[k], sc[k]);
                nn[k] = nn[k] || sc[k] != sc[k];
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m[k] = 0.f;
        if (k >= nh) continue;   // (wave-uniform)
        m[k] = bfly64_max(mx[k]);
        if (__ballot(nn[k]) != 0ull) m[k] = quiet_nan();
    }
    if (NW > 1) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[0][wave][k] = m[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float m0 = red[0][0][k], m1 = red[0][1][k], m2 = red[0][2][k], m3 = red[0][3][k];
            m[k] = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
            if (m0 != m0 || m1 != m1 || m2 != m2 || m3 != m3) m[k] = quiet_nan();
        }
    }
    float acc[NA][4];
#pragma unroll
    for (int u = 0; u < NA; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[u][k] = 0.f;
    for (int64_t base = 0; base < len; base += kPartials) {
#pragma unroll
        for (int u = 0; u < NA; ++u) {   // ascending j within every partial
            const int64_t j0 = base + (NW == 1 ? u * kWave : first);
            if (j0 >= len) continue;   // (wave-uniform)
            const bool ok = j0 + lane < len;
            float sc[4];
            group_scores(p, s, cols[ok ? j0 + lane : j0], h0, nh, lv, sc);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[u][k] = acc[u][k] + (ok ? exp_t(sc[k] - m[k]) : 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rinv[k] = 0.f;
        if (k >= nh) continue;   // (wave-uniform)
        float S;
        if (NW == 1) {
            float W[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                W[u] = 0.f;
                if ((int64_t)u * kWave < len) W[u] = bfly64_add(acc[u < NA ? u : 0][k]);   // (wave-uniform; partials of +0 sum to +0)
            }
            S = (W[0] + W[1]) + (W[2] + W[3]);
        } else {
            const float Ww = bfly64_add(acc[0][k]);
            if (lane == 0) red[1][wave][k] = Ww;
            __syncthreads();
            S = (red[1][0][k] + red[1][1][k]) + (red[1][2][k] + red[1][3][k]);
        }
        rinv[k] = 1.0f / S;
    }
    if (NW > 1) __syncthreads();   // the next head group's words must not overtake this one's reads
}

// A segment of `len` in 1..64 entries, lane = entry (col: its column, clamped): the coefficients of all heads into `tile`.
// STATS: (m, 1/S) of every head also go to `st` (head h at st[h] and st[K + h]).
template <bool STATS, typename P>
__device__ __forceinline__ void single_chunk_tile(const P& p, int s, const float* lrow, int col, int len, int lane, float* tile, float* st) {
    const bool ok = lane < len;
    for (int h0 = 0; h0 < p.K; h0 += 4) {
        const int nh = p.K - h0 < 4 ? p.K - h0 : 4;   // (wave-uniform)
        float lv[4], sc[4];
        load_heads(lrow, h0, nh, lv);
        group_scores(p, s, col, h0, nh, lv, sc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nh) continue;   // (wave-uniform)
            const float x = ok ? sc[k] : neg_inf();
            float m = bfly64_max(x);
            if (__ballot(x != x) != 0ull) m = quiet_nan();
            const float e = ok ? exp_t(x - m) : 0.f;   // P[lane] = +0 + e, the partials 64 .. 255 are +0
            const float S = bfly64_add(e);             // = (W_0 + 0) + (0 + 0)
            const float rinv = 1.0f / S;
            const float a = e * rinv;
            if (ok) tile[lane * p.K + h0 + k] = a;
            if (STATS && lane == 0) st[h0 + k] = m, st[p.K + h0 + k] = rinv;
        }
    }
}

// Up to FOUR segments of at most 16 entries at once, lane group gi the segment of row `row` (per lane: its group's), lane q its
// entry q: `len` in 0..16 entries from `beg` (0: the group has no such segment).  The reductions stay inside the 16-lane group --
// the partials 16 .. 255 are +0, and W_0 + 0 adds no bit -- and the coefficients of group gi go to the entries 16 gi .. of `tile`.
// STATS: (m, 1/S) of the group's segment also go to `st` (per lane: its group's row; head h at st[h] and st[K + h]).
// Returns the column of the lane's entry.
template <bool STATS, typename P>
__device__ __forceinline__ int short_tiles(const P& p, int s, int64_t row, int64_t beg, int len, int lane, float* tile, float* st) {
    const bool ok = (lane & (kGroup - 1)) < len;
    int col = 0;
    if (ok) col = p.colidx[s][beg + (lane & (kGroup - 1))];
    const float* lrow = p.l + row * p.ldl + (int64_t)s * p.K;
    const float* rrow = p.r + (int64_t)col * p.ldr + (int64_t)s * p.K;
    for (int h0 = 0; h0 < p.K; h0 += 4) {
        const int nh = p.K - h0 < 4 ? p.K - h0 : 4;   // (wave-uniform)
        float lv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            load_heads(lrow, h0, nh, lv);
            load_heads(rrow, h0, nh, rv);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nh) continue;   // (wave-uniform)
            const float x = ok ? leaky(lv[k] + rv[k], p.slope) : neg_inf();
            const unsigned long long nan_lanes = __ballot(x != x);
            float m = bfly16<Max>(x);
            if ((nan_lanes >> (lane & 48)) & 0xffffull) m = quiet_nan();
            const float e = ok ? exp_t(x - m) : 0.f;   // P[q] = +0 + e
            const float S = bfly16<Add>(e);            // = W_0
            const float rinv = 1.0f / S;
            const float a = e * rinv;
            if (ok) tile[lane * p.K + h0 + k] = a;
            if (STATS && ok && (lane & (kGroup - 1)) == 0) st[h0 + k] = m, st[p.K + h0 + k] = rinv;
        }
    }
    return col;
}

// The coefficients of `count` (1..64) entries of a longer segment, lane = entry (col: its column, clamped), from the segment's
// statistics `stat`: e and alpha by the operations that produced S.
template <typename P>
__device__ __forceinline__ void chunk_tile(const P& p, int s, const float* lrow, int col, int count, int lane, const float* stat,
                                           float* tile) {
    const bool ok = lane < count;
    for (int h0 = 0; h0 < p.K; h0 += 4) {
        const int nh = p.K - h0 < 4 ? p.K - h0 : 4;   // (wave-uniform)
        float lv[4], sc[4];
        load_heads(lrow, h0, nh, lv);
        group_scores(p, s, col, h0, nh, lv, sc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nh) continue;   // (wave-uniform)
            const float a = exp_t(sc[k] - stat[h0 + k]) * stat[kMaxHeads + h0 + k];
            if (ok) tile[lane * p.K + h0 + k] = a;
        }
    }
}

// sum over the lanes {l, l^16}, then {l, l^32}: (P[gi] + P[gi^1]) + (P[gi^2] + P[gi^3])
__device__ __forceinline__ float fold_groups(float v) { return bfly_groups<Add>(v); }

// One batch of U rounds of a chunk: group gi serves entry 4r + gi in round r.  FULL: every round of the batch exists.  All the
// gathers of the batch go out before its first FMA; an entry beyond `count` loads (a clamped, valid address) and adds nothing.
template <int NB, int U, bool FULL, typename P>
__device__ __forceinline__ void batch(const P& p, const float* tile, const int (&head)[NB], int cbase, int r0, int rounds, int count,
                                      int ecol, int lane0, int lane, Quad (&acc)[NB]) {
    const int q = lane & 15, gi = lane >> 4;
    typename Gathered<typename P::X>::type xv[U][NB];   // (bf16: packed until the FMA below)
    float vv[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
            const int n = 4 * (r0 + u) + gi < count ? 4 * (r0 + u) + gi : count - 1;
            const int c = __builtin_amdgcn_ds_bpermute((lane0 + n) << 2, ecol);
            const typename P::X* xrow = p.x + (int64_t)c * p.ldx;
#pragma unroll
            for (int b = 0; b < NB; ++b) vv[u][b] = tile[n * p.K + head[b]];
#pragma unroll
            for (int b = 0; b < NB; ++b) xv[u][b] = load_gathered(xrow, cbase + b * kBlockCols + 4 * q, p.d);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (FULL || r0 + u < rounds) {
            if (4 * (r0 + u) + gi < count) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const Quad& xq = widen(xv[u][b]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[b].v[k] = __builtin_fmaf(vv[u][b], xq.v[k], acc[b].v[k]);
                }
            }
        }
    }
}

// `count` (1..64) consecutive entries whose coefficients are in `tile` (entry n at n * K) and whose columns are in `ecol` of the
// lanes lane0 + n: every entry goes into the partial of its group, in ascending order.  All 64 lanes must be active.
template <int NB, int U, typename P>
__device__ __forceinline__ void gather_chunk(const P& p, const float* tile, const int (&head)[NB], int cbase, int count, int ecol,
                                             int lane0, int lane, Quad (&acc)[NB]) {
    const int rounds = (count + 3) >> 2;
    int r0 = 0;
    for (; r0 + U <= rounds; r0 += U) batch<NB, U, true>(p, tile, head, cbase, r0, rounds, count, ecol, lane0, lane, acc);
    if (r0 < rounds) batch<NB, U, false>(p, tile, head, cbase, r0, rounds, count, ecol, lane0, lane, acc);
}

// The head of every block of the pass for this lane's quad (a quad beyond d: the last head, its sums are never stored).
template <int NB, typename P>
__device__ __forceinline__ void pass_heads(const P& p, int cbase, int q, int (&head)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int h = (cbase + b * kBlockCols + 4 * q) / p.head_cols;
        head[b] = h < p.K ? h : p.K - 1;
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

// The statistics of all heads of a segment of `len` >= 1 entries into `stat` (see group_stats for NW).
template <int NW, typename P>
__device__ __forceinline__ void segment_stats(const P& p, int s, const float* lrow, const int32_t* cols, int64_t len, int lane,
                                              int wave, float (*red)[kWavesPerBlock][4], float* stat) {
    for (int h0 = 0; h0 < p.K; h0 += 4) {
        const int nh = p.K - h0 < 4 ? p.K - h0 : 4;   // (wave-uniform)
        float lv[4], m[4], rinv[4];
        load_heads(lrow, h0, nh, lv);
        group_stats<NW>(p, s, cols, len, h0, nh, lv, lane, wave, red, m, rinv);
        if (lane == 0 && (NW == 1 || wave == 0)) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nh) stat[h0 + k] = m[k], stat[kMaxHeads + h0 + k] = rinv[k];
        }
    }
}

// ---- the statistics rows (STATS)
// The statistics of (row, selected hop s): m of head h at [h], 1/S at [K + h].
template <typename P>
__device__ __forceinline__ float* stat_row(const P& p, float* stats, int64_t ldstats, int64_t row, int s) {
    return stats + row * ldstats + (int64_t)s * 2 * p.K;
}
// `stat` (m at [h], 1/S at [kMaxHeads + h], written by this wave or behind a barrier) to the statistics row `st`.
template <typename P>
__device__ __forceinline__ void store_stats(const P& p, const float* stat, float* st, int t) {
    if (t < p.K) st[t] = stat[t], st[p.K + t] = stat[kMaxHeads + t];
}

// ---- the walk
// The walk of one block (attention_fused.hip describes it): long segment, or per wave groups of four short segments -> single chunk
// -> multi-chunk, each with its column passes.  P: the parameter struct (its X the element type of x); TY: of y; NB: 64-column blocks
// of a column pass; STATS: (m, 1/S) of every (row, hop, head) also go to `stats` (an empty segment: (+0, +0)).  Every kernel is a
// wrapper that declares the LDS and calls this, rather than having the walk as its body: the call depth alone moves the registers of
// the NB = 1 forms (the parent's plain kernel: 141 VGPRs, 3 waves per SIMD as a body, 119 and 4 behind one inlined call), and the
// wrappers' form is the faster one where they differ (d = 64 at the products shape: 21.9 ms against 26.2).  The dropout kernel
// (attention_dropout.hip) is the one that does NOT call it: it keeps a copy with its drop_tile calls, for the time measured there.
template <typename TY, int NB, bool STATS, typename P>
__device__ __forceinline__ void forward_walk(const P& p, Shared<NB>& sh, float* stats, int64_t ldstats) {
    constexpr int U = Loads<typename P::X>::value / NB;
    constexpr int kPassCols = NB * kBlockCols;
    // the long path's epilogue writes one column per thread; with a bf16 operand one PAIR (d is then even: a bf16 pair is one dword,
    // and no 2-byte store has a neighbour to race with).  The sums per column are the same either way.
    constexpr int CW = std::is_same<TY, float>::value && std::is_same<typename P::X, float>::value ? 1 : 2;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane & 15, gi = lane >> 4;
    float* tile = sh.tile[wave];
    TY* const y = static_cast<TY*>(p.y);
    int head[NB];
    Quad acc[NB];
    const bool one_pass = p.d <= kPassCols;   // the heads of the lane's blocks are then the same for every segment
    pass_heads(p, 0, q, head);
    int64_t row, beg, end;
    int s;
    if (long_segment(p.geom, blockIdx.x, &row, &s, &beg, &end)) {
        // ---- a long segment: 64-entry chunks over the 4 waves ----
        const int64_t len = end - beg;   // (the same for the whole block)
        const float* lrow = p.l + row * p.ldl + (int64_t)s * p.K;
        const int32_t* cols = p.colidx[s] + beg;
        TY* out = y + row * p.ldy_row + (int64_t)s * p.ldy_hop;
        if (len > 0) segment_stats<kWavesPerBlock>(p, s, lrow, cols, len, lane, wave, sh.red, sh.stat[0]);
        __syncthreads();
        if constexpr (STATS) {
            float* st = stat_row(p, stats, ldstats, row, s);
            if (len > 0) store_stats(p, sh.stat[0], st, threadIdx.x);
            else if ((int)threadIdx.x < 2 * p.K) st[threadIdx.x] = 0.f;
        }
        for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
            clear(acc);
            if (!one_pass) pass_heads(p, cbase, q, head);
            for (int64_t c = (int64_t)wave * kWave; c < len; c += kBlock) {
                const int count = (int)(len - c < kWave ? len - c : kWave);
                const int ecol = cols[c + (lane < count ? lane : count - 1)];
                wave_lds_sync();   // the previous chunk's reads of the tile come first
                chunk_tile(p, s, lrow, ecol, count, lane, sh.stat[0], tile);
                wave_lds_sync();
                gather_chunk<NB, U>(p, tile, head, cbase, count, ecol, 0, lane, acc);
            }
            const Quad mine = fold_blocks(acc, gi);
            if (gi < NB) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sh.tot[wave][gi * kBlockCols + 4 * q + k] = mine.v[k];
            }
            __syncthreads();
            const int c = CW * threadIdx.x;
            if (c < kPassCols && cbase + c < p.d) {
                float t[CW];
#pragma unroll
                for (int k = 0; k < CW; ++k) t[k] = ((sh.tot[0][c + k] + sh.tot[1][c + k]) + sh.tot[2][c + k]) + sh.tot[3][c + k];
                if constexpr (CW == 1) out[cbase + c] = t[0];
                else store_pair(out, cbase + c, t[0], t[1]);
            }
            __syncthreads();
        }
        return;
    }
    // ---- the tile walk: each wave walks rows_per_wave consecutive rows ----
    int64_t row0, rp;
    if (!wave_rows(p.geom, blockIdx.x, wave, lane, &row0, &rp)) return;
    float* stat = sh.stat[wave];
    const int rpw = p.geom.rows_per_wave;
    for (s = 0; s < p.geom.n_sel; ++s) {
        for (int i0 = 0; i0 < rpw && row0 + i0 < p.geom.n_rows; i0 += 4) {
            // lane group gi looks at row i0 + gi: segments of at most 16 entries get their coefficients FOUR AT A TIME
            int64_t gbeg, glen;
            group_segment<false>(p.geom, s, i0, row0, rp, lane, &gbeg, &glen);
            const bool is_short = glen >= 1 && glen <= kGroup;
            int ecol = 0;
            wave_lds_sync();   // the previous segments' reads of the tile come first
            if (__ballot(is_short) != 0ull) {
                ecol = short_tiles<STATS>(p, s, row0 + i0 + gi, gbeg, is_short ? (int)glen : 0, lane, tile,
                                          STATS ? stat_row(p, stats, ldstats, row0 + i0 + gi, s) : nullptr);
            }
            wave_lds_sync();
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len < 0 || len > kGroup) continue;   // (wave-uniform) no such row, a long segment, or one for the loop below
                TY* out = y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                if (STATS && len == 0 && lane < 2 * p.K) stat_row(p, stats, ldstats, row0 + i0 + k, s)[lane] = 0.f;   // an empty segment
                for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                    clear(acc);
                    if (!one_pass) pass_heads(p, cbase, q, head);
                    if (len > 0) gather_chunk<NB, U>(p, tile + k * kGroup * p.K, head, cbase, (int)len, ecol, k * kGroup, lane, acc);
                    const Quad mine = fold_blocks(acc, gi);   // (an empty segment: +0)
                    if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
                }
            }
            // the longer segments of these rows, one at a time on the whole wave
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int64_t len = readlane64(glen, k * kGroup);
                if (len <= kGroup) continue;   // (wave-uniform)
                beg = readlane64(gbeg, k * kGroup);
                const float* lrow = p.l + (row0 + i0 + k) * p.ldl + (int64_t)s * p.K;
                const int32_t* cols = p.colidx[s] + beg;
                TY* out = y + (row0 + i0 + k) * p.ldy_row + (int64_t)s * p.ldy_hop;
                const bool single = len <= kWave;   // (wave-uniform)
                wave_lds_sync();   // the previous segment's reads of the tile and of the statistics come first
                if (single) {
                    ecol = cols[lane < len ? lane : len - 1];
                    single_chunk_tile<STATS>(p, s, lrow, ecol, (int)len, lane, tile,
                                             STATS ? stat_row(p, stats, ldstats, row0 + i0 + k, s) : nullptr);
                } else {
                    segment_stats<1>(p, s, lrow, cols, len, lane, 0, nullptr, stat);
                }
                wave_lds_sync();
                if (STATS && !single) store_stats(p, stat, stat_row(p, stats, ldstats, row0 + i0 + k, s), lane);
                for (int cbase = 0; cbase < p.d; cbase += kPassCols) {
                    clear(acc);
                    if (!one_pass) pass_heads(p, cbase, q, head);
                    if (single) {
                        gather_chunk<NB, U>(p, tile, head, cbase, (int)len, ecol, 0, lane, acc);
                    } else {
                        for (int64_t c = 0; c < len; c += kWave) {
                            const int count = (int)(len - c < kWave ? len - c : kWave);
                            ecol = cols[c + (lane < count ? lane : count - 1)];
                            wave_lds_sync();
                            chunk_tile(p, s, lrow, ecol, count, lane, stat, tile);
                            wave_lds_sync();
                            gather_chunk<NB, U>(p, tile, head, cbase, count, ecol, 0, lane, acc);
                        }
                    }
                    const Quad mine = fold_blocks(acc, gi);
                    if (gi < NB) store_quad(out, cbase + gi * kBlockCols + 4 * q, p.d, mine);
                }
            }
        }
    }
}

// The three geometries of a forward kernel: the narrowest that covers d in one column pass, four blocks beyond 256 columns (the bits
// are the same for all three: every column has its own tree).  `launch(std::integral_constant<int, NB>)` launches it.
template <typename F>
void for_blocks(int d, F&& launch) {
    if (d <= kBlockCols) launch(std::integral_constant<int, 1>{});
    else if (d <= 2 * kBlockCols) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, kMaxBlocks>{});
}

// ---- host: the one launch path of the five forward entry points (attention_fused.hip)
struct Call {   // in the order of the entry points' arguments
    const h2gcn_plan_t* plan;
    uint32_t hop_mask;
    const float* l;
    int64_t ldl;
    const float* r;
    int64_t ldr;
    int32_t n_heads;
    float slope;
    int x_dtype;               // H2GCN_DTYPE_*: a bf16 x names the `_bf16` entry points, which take either y; an fp32 x stores fp32
    const void* X;
    int64_t ldx;
    int32_t d;
    int y_dtype;
    void* Y;
    int64_t ldy_row, ldy_hop;
    bool with_stats;
    float* stats;              // [n_rows, H_sel, 2, K] through ldstats
    int64_t ldstats;
    const attention_dropout::Draw* dropout;    // NULL: none (else an fp32 x, with statistics)
    void* stream;
};
int run(const Call& c);

// The kernels of the four units behind it, each launched by its own unit (`stats` NULL: the kernels without statistics).
using Params16 = ParamsT<bf16_t, void>;   // (the output's element type is the kernel's template parameter)
void launch_forward(const Params& p, dim3 grid, hipStream_t stream);                                 // attention_fused.hip
void launch_stats(const Params& p, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream);    // attention_stats.hip
void launch_stats_dropout(const Params& p, float* stats, int64_t ldstats, const attention_dropout::Args& da, dim3 grid,
                          hipStream_t stream);                                                       // attention_dropout.hip
void launch_bf16(const Params16& p, bool y16, bool with_stats, float* stats, int64_t ldstats, dim3 grid, hipStream_t stream);   // attention_bf16.hip

}  // namespace attention_fused
}  // namespace h2gcn
