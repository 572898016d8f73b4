"""The recomputing attention backward, restated in numpy from the formulas of include/h2gcn_hip.h (the comment above
h2gcn_attention_hops_heads_backward_f32 and, for the factor f, "ATTENTION DROPOUT ... WHERE f ENTERS") -- not from the kernels: no
torch, no autograd, no GPU, entry-wise over the COO rows (np.add.at / np.maximum.at), never dense.

`backward` computes everything from scratch in ONE dtype and returns, next to delta, dl, dr and dX, the sum of the absolute values
of the terms of every element: the scale an error of that element is weighed against (`rho`), so that a wrong short segment is not
hidden behind the largest element of its array.  `sweep_hops` builds the operands of tests/test_attention_backward_sweep_gpu.py:
prescribed segment lengths on the rows AND on the columns of one small square graph."""
import functools

import numpy as np
import scipy.sparse as sp

import spmm_driver as drv

# 64 / 65: one chunk becomes two; 255 .. 258: the four sets are filled, then set 0 gets a second round; 319 .. 321: that round's chunk
# is partial or full; 31 .. 33 and 255 .. 257 straddle the plan thresholds 32 and 256; 0: the empty segment
SWEEP_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321,
                 340]
SWEEP_SIDE = 342


def _rot(a, k):
    k %= len(a)
    return list(a[k:]) + list(a[:k])


@functools.lru_cache(maxsize=None)
def sweep_hops(n_hops=2):
    """Per hop k the square operand block_diag(R_k, C_k): R_k [29, 342] has the lengths of SWEEP_LENGTHS rotated by 11 k on its rows,
    C_k [342, 29] those rotated by 11 k + 5 on its COLUMNS.  371 x 371; the column and the row that close a block are never
    referenced."""
    out = []
    for k in range(n_hops):
        rows = drv.hop_from_lengths(_rot(SWEEP_LENGTHS, 11 * k), SWEEP_SIDE, seed=71 + k)
        cols = drv.hop_with_transposed_lengths(_rot(SWEEP_LENGTHS, 11 * k + 5), SWEEP_SIDE, seed=81 + k)
        a = sp.block_diag((rows, cols), format="csr").astype(np.float32)
        a.sort_indices()
        out.append(sp.csr_matrix((a.data, a.indices.astype(np.int32), a.indptr.astype(np.int64)), shape=a.shape))
    return tuple(out)


def coo_rows(m):
    return np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(m.indptr))


def backward(hops, x, l, r, g, slope, factors=None, dtype=np.float64):
    """hops: per selected hop (indptr, indices) or a scipy CSR matrix; x [n_cols, d], l [n_rows, H, K], r [n_cols, H, K],
    g [n_rows, H, d]; factors: per hop [nnz, K] (dropout) or None -> ((delta, dl, dr, dx), (their magnitude arrays)), all `dtype`.
    An empty segment and a column nobody references give exact zeros in both."""
    dt = np.dtype(dtype).type
    x, l, r, g = (np.asarray(t).astype(dt) for t in (x, l, r, g))
    slope = dt(slope)
    n_rows, n_hops, k = l.shape
    n_cols, d = x.shape
    w = d // k
    delta, dl, dr = np.zeros((n_rows, n_hops, k), dt), np.zeros((n_rows, n_hops, k), dt), np.zeros((n_cols, n_hops, k), dt)
    m_delta, m_dl, m_dr = np.zeros_like(delta), np.zeros_like(dl), np.zeros_like(dr)
    dx, m_dx = np.zeros((n_cols, d), dt), np.zeros((n_cols, d), dt)
    for s, hop in enumerate(hops):
        indptr, indices = (hop.indptr, hop.indices) if hasattr(hop, "indptr") else hop
        indptr = np.asarray(indptr, dtype=np.int64)
        j = np.asarray(indices, dtype=np.int64)
        i = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr))
        f = np.ones((len(j), k), dt) if factors is None else np.asarray(factors[s]).astype(dt)
        pre = l[i, s] + r[j, s]                                                          # [nnz, K]
        score = np.where(pre > 0, pre, pre * slope)
        top = np.full((n_rows, k), -np.inf, dt)
        np.maximum.at(top, i, score)
        e = np.exp(score - top[i])
        total = np.zeros((n_rows, k), dt)
        np.add.at(total, i, e)
        alpha = e / total[i]
        af = np.repeat(alpha * f, w, axis=1)                                             # the coefficient of y and dX, per column
        xs, gs = x[j], g[i, s]                                                           # [nnz, d]
        y = np.zeros((n_rows, d), dt)
        np.add.at(y, i, af * xs)
        gx, gy = gs * xs, g[:, s] * y
        dalpha = f * gx.reshape(-1, k, w).sum(axis=2)
        delta[:, s] = gy.reshape(n_rows, k, w).sum(axis=2)                               # <g, y>_h: from y, as the kernel forms it
        m_delta[:, s] = np.abs(gy).reshape(n_rows, k, w).sum(axis=2)
        dscore = alpha * (dalpha - delta[i, s])
        dpre = np.where(pre > 0, dscore, dscore * slope)
        m_dpre = alpha * (f * np.abs(gx).reshape(-1, k, w).sum(axis=2) + m_delta[i, s]) * np.where(pre > 0, dt(1), np.abs(slope))
        np.add.at(dl[:, s], i, dpre)
        np.add.at(m_dl[:, s], i, m_dpre)
        np.add.at(dr[:, s], j, dpre)
        np.add.at(m_dr[:, s], j, m_dpre)
        np.add.at(dx, j, af * gs)
        np.add.at(m_dx, j, af * np.abs(gs))
    return (delta, dl, dr, dx), (m_delta, m_dl, m_dr, m_dx)


def rho(got, want, mag):
    """max_i |got_i - want_i| / A_i over the elements with A_i > 0 (the others must be exact zeros: `zeros_exact`)."""
    got, want, mag = (np.asarray(t, dtype=np.float64) for t in (got, want, mag))
    live = mag > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - want)[live] / mag[live]).max())


def zeros_exact(got32, mag, signed=False):
    """Where A_i == 0 the float32 array holds +0 on the bits (signed=True: a zero of either sign)."""
    dead = np.asarray(mag) == 0
    vals = np.ascontiguousarray(got32, dtype=np.float32)
    return bool((vals[dead] == 0).all()) if signed else not vals.view(np.int32)[dead].any()
