// symmetric.hip -- the mirror pass of H2GCN_PLAN_SYMMETRIC_PATTERN: verifies that a square CSR stores (j, i) whenever it
// stores (i, j) and, in the same walk, produces what the adjoint operand of such a hop still needs.
//
// A pattern-symmetric A has A^T's row pointers and column ids equal to its own (both in row-major, ascending-column order), so
// the adjoint launch can read the caller's arrays; only the VALUES of A^T may differ: t_vals[e] = vals[partner[e]], where
// partner[e] is the position of (j, i) for the entry e = (i, j).  That position is the "source forward entry of transposed
// entry e", i.e. exactly what the radix transposition (transpose.hip) keeps as `perm`.  Instead of a stable sort over all
// nonzeros this is one binary search per entry in a row the forward launches read anyway:
//   * a group of G lanes walks one row (the row index is known, no search for it), one entry per lane and round;
//   * the lane reads the bounds of row j once and keeps them in registers; the ~log2(row length) probes are element-granular
//     gathers served by L2 / the Infinity Cache (neighbouring rows of a graph share most of their lines);
//   * results per hop: missing mirror -> the (row, col) that comes first in (row, col) order (64-bit atomicMin on row << 32 | col,
//     one atomic per wave at most), values bit-symmetric or not, and whether every row was strictly ascending -- the search
//     relies on that order, and with it every found position is THE mirror, so partner is an involution.
// Deterministic: the outputs are plain stores of searched positions; the only atomics are a min and an or.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "capi_internal.h"

namespace h2gcn {

namespace {

template <int G>
__global__ __launch_bounds__(256) void mirror_pass_kernel(int64_t n, const int64_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colidx, const float* __restrict__ vals,
                                                          uint32_t* __restrict__ partner, float* __restrict__ t_vals,
                                                          MirrorStatus* status) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t n_groups = ((int64_t)gridDim.x * blockDim.x) / G;
    unsigned flags = 0;
    unsigned long long miss = ~0ull;
    for (int64_t i = group; i < n; i += n_groups) {
        const int64_t b = rowptr[i], e = rowptr[i + 1];
        for (int64_t t = b + sub; t < e; t += G) {
            const int32_t j = colidx[t];
            const int32_t prev = t > b ? colidx[t - 1] : -1;
            if (j <= prev) flags |= kMirrorUnsorted;
            if (j < 0 || (int64_t)j >= n) {   // (plans created with H2GCN_PLAN_SKIP_VALIDATION: never index rowptr with it)
                flags |= kMirrorRange;
                continue;
            }
            int64_t p = t;   // a diagonal entry is its own mirror
            if ((int64_t)j != i) {
                const int64_t lo = rowptr[j];
                const uint32_t len = (uint32_t)(rowptr[j + 1] - lo);
                const int32_t* __restrict__ row = colidx + lo;
                // largest base with row[base] <= i (when row[0] <= i); the answer stays inside [base, base + m)
                uint32_t base = 0, m = len;
                while (m > 1) {
                    const uint32_t half = m >> 1;
                    if (row[base + half] <= (int32_t)i) base += half;
                    m -= half;
                }
                if (len == 0 || row[base] != (int32_t)i) {
                    const unsigned long long key = ((unsigned long long)i << 32) | (unsigned long long)(uint32_t)j;
                    miss = key < miss ? key : miss;
                    continue;
                }
                p = lo + base;
            }
            const float v = vals[p];
            if (__float_as_uint(v) != __float_as_uint(vals[t])) flags |= kMirrorValuesDiffer;
            if (partner) partner[t] = (uint32_t)p;
            if (t_vals) t_vals[t] = v;
        }
    }
    // one atomic per wave and kind at most
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(miss, off);
        miss = other < miss ? other : miss;
        flags |= __shfl_xor(flags, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (miss != ~0ull) atomicMin(&status->missing_key, miss);
        if (flags) atomicOr(&status->flags, flags);
    }
}

}  // namespace

// Launches the mirror pass of one hop on `stream` (asynchronous).  `status` must hold {~0, 0}.  partner / t_vals: nnz entries
// each, or NULL for an output the caller does not keep.
hipError_t mirror_pass(int64_t n, int64_t nnz, const int64_t* rowptr, const int32_t* colidx, const float* vals,
                       uint32_t* partner, float* t_vals, MirrorStatus* status, hipStream_t stream) {
    if (n <= 0 || nnz <= 0) return hipSuccess;
    // short rows: 16-lane groups, so that a row of a handful of entries does not idle three quarters of a wave
    const bool narrow = nnz < 32 * n;
    const int64_t per_block = narrow ? 256 / 16 : 256 / 64;
    const int64_t want = (n + per_block - 1) / per_block;
    const dim3 grid((unsigned)(want > 16384 ? 16384 : want));
    if (narrow)
        hipLaunchKernelGGL(mirror_pass_kernel<16>, grid, dim3(256), 0, stream, n, rowptr, colidx, vals, partner, t_vals, status);
    else
        hipLaunchKernelGGL(mirror_pass_kernel<64>, grid, dim3(256), 0, stream, n, rowptr, colidx, vals, partner, t_vals, status);
    return hipGetLastError();
}

}  // namespace h2gcn
