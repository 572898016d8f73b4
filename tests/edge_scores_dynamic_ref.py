"""The dynamic (GATv2) edge scores of include/h2gcn_hip.h restated in numpy, in fp64: scores, du, dv, da and the magnitudes their
error bounds are stated in.  "Exact" as the header defines it: real arithmetic (here fp64) on the fp32 inputs, the branch of the
leaky_relu taken from the fp32 sum p = u[i] + v[j].  No GPU, no library."""
import numpy as np

CHUNK = 1 << 14   # entries per pass: nothing of size nnz x d is held here either

U = 2.0 ** -24
TINY = 2.0 ** -149


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-24"""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def entries(m):
    """(row, column) of every stored entry of a scipy CSR matrix, in stored order."""
    return np.repeat(np.arange(m.shape[0]), np.diff(m.indptr)), m.indices.astype(np.int64)


def _indicator(node, n):
    """[n, len(node)] with a one at (node[m], m): `indicator @ terms` sums the terms of every node."""
    import scipy.sparse as sp

    return sp.csr_matrix((np.ones(len(node)), (node, np.arange(len(node)))), shape=(n, len(node)))


class Reference:
    """scores / mag_scores per selected hop ([nnz_k, K]); with `ds` (a list of [nnz_k, K] arrays) also du, dv, da, their magnitudes
    (the sums of |dp| / |ds q|) and the number of terms of every row / column / hop."""

    def __init__(self, hops, u, v, a, n_heads, slope, ds=None, sel=None):
        sel = list(range(len(hops))) if sel is None else list(sel)
        u32, v32 = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
        u64, v64, a64 = u32.astype(np.float64), v32.astype(np.float64), np.asarray(a, dtype=np.float32).astype(np.float64).reshape(len(sel), -1)
        sl = float(np.float32(slope))
        n_rows, n_cols = hops[0].shape
        d = u32.shape[1]
        w = d // n_heads
        self.scores, self.mag_scores = [], []
        if ds is not None:
            self.du, self.mag_du, self.n_du = np.zeros((n_rows, d)), np.zeros((n_rows, d)), np.zeros(n_rows, dtype=np.int64)
            self.dv, self.mag_dv, self.n_dv = np.zeros((n_cols, d)), np.zeros((n_cols, d)), np.zeros(n_cols, dtype=np.int64)
            self.da, self.mag_da = np.zeros((len(sel), d)), np.zeros((len(sel), d))
            self.n_da = np.array([hops[k].nnz for k in sel], dtype=np.int64)
        for s, k in enumerate(sel):
            rows, cols = entries(hops[k])
            nnz = len(rows)
            sc, mg = np.zeros((nnz, n_heads)), np.zeros((nnz, n_heads))
            for lo in range(0, nnz, CHUNK):
                r, c = rows[lo:lo + CHUNK], cols[lo:lo + CHUNK]
                with np.errstate(all="ignore"):
                    pos = (u32[r] + v32[c]) > 0          # the branch of the fp32 sum; a NaN takes the slope branch
                    p = u64[r] + v64[c]
                    q = np.where(pos, p, p * sl)
                    aq = a64[s][None, :] * q
                    sc[lo:lo + CHUNK] = aq.reshape(len(r), n_heads, w).sum(axis=2)
                    mg[lo:lo + CHUNK] = np.abs(aq).reshape(len(r), n_heads, w).sum(axis=2)
                    if ds is not None:
                        g = np.repeat(np.asarray(ds[s], dtype=np.float32).astype(np.float64).reshape(nnz, n_heads)[lo:lo + CHUNK], w, axis=1)
                        dq = g * a64[s][None, :]
                        dp = np.where(pos, dq, dq * sl)
                        by_row, by_col = _indicator(r, n_rows), _indicator(c, n_cols)
                        self.du += by_row @ dp
                        self.mag_du += by_row @ np.abs(dp)
                        self.dv += by_col @ dp
                        self.mag_dv += by_col @ np.abs(dp)
                        self.da[s] += (g * q).sum(axis=0)
                        self.mag_da[s] += np.abs(g * q).sum(axis=0)
            if ds is not None:
                self.n_du += np.bincount(rows, minlength=n_rows)
                self.n_dv += np.bincount(cols, minlength=n_cols)
            self.scores.append(sc)
            self.mag_scores.append(mg)
        self.w = w

    def score_bound(self, s):
        return gamma(self.w + 2) * self.mag_scores[s] + (self.w + 2) * TINY

    def du_bound(self):
        return gamma(self.n_du + 2)[:, None] * self.mag_du + (self.n_du + 2)[:, None] * TINY

    def dv_bound(self):
        return gamma(self.n_dv + 2)[:, None] * self.mag_dv + (self.n_dv + 2)[:, None] * TINY

    def da_bound(self):
        return gamma(self.n_da + 3)[:, None] * self.mag_da + (self.n_da + 3)[:, None] * TINY
