// attention_dropout.hip.h -- the generator of the attention dropout (documented in include/h2gcn_hip.h; tests/attention_dropout_ref.py
// restates it bit for bit), ONE definition for the forward, the two sides of the backward and the kernel that writes the factors.
//
// The factor of (entry, head) is a pure function of (seed, step, k, i, j, h): k the PLAN's hop index, (i, j) the entry's row and column
// in the plan's forward operand, h the head.  It knows nothing of the entry's position in colidx / t_colidx, of the segment classes or of
// the hop selection -- so the row side (walking A_k) and the column side (walking A_k^T, or a symmetric plan's forward arrays) draw the
// same mask without a permutation, and nothing of size nnz holds it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_internal.h"

namespace h2gcn {
namespace attention_dropout {

// What a launch hands its kernel: the mask's arguments as the caller gave them, and the geometry of the plan's forward operand.
struct Args {
    uint64_t seed;
    const int64_t* step_dev;       // read on the device at run time (NULL: step 0): a replayed graph draws a fresh mask
    uint32_t thr;                  // a 16-bit field is kept iff field < thr = floor(keep_prob * 65536)
    float inv_keep;                // 1.f / keep_prob, one fp32 division on the host
    uint64_t n_cols;               // of the plan's FORWARD operand, on either side
    uint32_t n_hops;               // of the plan
    int32_t hop[H2GCN_MAX_HOPS];   // the plan's hop index of selected hop s
};

// mix32 and the key derivation of classifier_kernels.hip.h (the same constants)
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    return h ^ (h >> 16);
}
struct Mask {
    uint32_t k0, k1, thr;
    float inv_keep;
    uint64_t n_cols;
    uint32_t n_hops;
};
__device__ __forceinline__ Mask make_mask(const Args& a) {
    const uint64_t step = a.step_dev ? (uint64_t)*a.step_dev : 0;
    const uint32_t k0 = mix32((uint32_t)a.seed ^ mix32((uint32_t)step + 0x9E3779B9u));
    const uint32_t k1 = mix32((uint32_t)(a.seed >> 32) ^ (uint32_t)(step >> 32) ^ k0 ^ 0x85EBCA6Bu);
    return Mask{k0, k1, a.thr, a.inv_keep, a.n_cols, a.n_hops};
}

// gid of head pair 0 of the entry (i, j) of the plan's hop k: ((i * n_cols + j) * n_hops + k) * 8, in 64 bits
__device__ __forceinline__ uint64_t entry_base(const Mask& m, int64_t i, int64_t j, int k) {
    return (((uint64_t)i * m.n_cols + (uint64_t)j) * m.n_hops + (uint32_t)k) * 8u;
}
// the word of head pair hp (heads 2 hp and 2 hp + 1) of the entry: the keyed avalanche round of the classifier's group_word on
// gid = base + hp
__device__ __forceinline__ uint32_t pair_word(const Mask& m, uint64_t base, int hp) {
    const uint64_t gid = base + (uint32_t)hp;
    const uint32_t hi = (uint32_t)(gid >> 32);
    uint32_t h = (uint32_t)gid ^ ((hi << 16) | (hi >> 16)) ^ m.k0;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= m.k1;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    return h ^ (h >> 16);
}
// head h owns the 16-bit field h & 1 of its pair's word
__device__ __forceinline__ bool kept(const Mask& m, uint32_t word, int h) { return ((word >> (16 * (h & 1))) & 0xFFFFu) < m.thr; }
__device__ __forceinline__ float factor(const Mask& m, uint32_t word, int h) { return kept(m, word, h) ? m.inv_keep : 0.f; }

// bit h set: head h of the entry is kept (K <= 16)
__device__ __forceinline__ uint32_t kept_heads(const Mask& m, uint64_t base, int K) {
    uint32_t bits = 0;
    for (int hp = 0; 2 * hp < K; ++hp) {
        const uint32_t w = pair_word(m, base, hp);
        bits |= (uint32_t)kept(m, w, 0) << (2 * hp) | (uint32_t)kept(m, w, 1) << (2 * hp + 1);
    }
    return bits;
}

// ---- host
// floor(keep_prob * 65536), 65536 for keep_prob = 1: keep_threshold of classifier_kernels.hip.h
inline uint32_t keep_threshold(float keep_prob) {
    const double t = (double)keep_prob * 65536.0;
    return t >= 65536.0 ? 65536u : (uint32_t)t;
}
// (NaN fails the first comparison)
inline int check_keep_prob(float keep_prob) {
    if (!(keep_prob > 0.f) || keep_prob > 1.f) return fail(H2GCN_ERR_INVALID_ARGUMENT, "keep_prob = %g outside (0, 1]", (double)keep_prob);
    return H2GCN_OK;
}
// The mask's arguments as the caller gave them: what a dropout entry point hands the launch path it shares with the entry points without.
struct Draw {
    float keep_prob;
    uint64_t seed;
    const int64_t* step_dev;
};
// `mask`: the resolved hop mask of a view of `plan`
inline Args make_args(const h2gcn_plan* plan, uint32_t mask, int64_t n_cols, float keep_prob, uint64_t seed, const int64_t* step_dev) {
    Args a = {};
    a.seed = seed, a.step_dev = step_dev;
    a.thr = keep_threshold(keep_prob), a.inv_keep = 1.f / keep_prob;
    a.n_cols = (uint64_t)n_cols, a.n_hops = (uint32_t)plan_hop_count(plan);
    for (int k = 0, s = 0; k < (int)a.n_hops; ++k)
        if (mask & (1u << k)) a.hop[s++] = k;
    return a;
}

}  // namespace attention_dropout
}  // namespace h2gcn
