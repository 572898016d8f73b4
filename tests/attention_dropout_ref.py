"""The attention dropout generator, restated in numpy from the text of include/h2gcn_hip.h ("ATTENTION DROPOUT ... THE GENERATOR"):
a scalar form that follows the header line by line, and a vectorised one the tests use."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def mix32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def keys(seed: int, step: int) -> tuple:
    seed &= M64
    step &= M64
    k0 = mix32((seed & M32) ^ mix32(((step & M32) + 0x9E3779B9) & M32))
    k1 = mix32((seed >> 32) ^ (step >> 32) ^ k0 ^ 0x85EBCA6B)
    return k0, k1


def keep_threshold(keep_prob: float) -> int:
    """floor(keep_prob * 65536) of the float32 ``keep_prob``, computed in double; 65536 at 1."""
    t = float(np.float32(keep_prob)) * 65536.0
    return 65536 if t >= 65536.0 else int(t)


def inv_keep(keep_prob: float) -> np.float32:
    return np.float32(1.0) / np.float32(keep_prob)


def factor_scalar(i: int, j: int, k: int, h: int, n_cols: int, n_hops: int, keep_prob: float, seed: int, step: int) -> np.float32:
    k0, k1 = keys(seed, step)
    gid = (((i * n_cols + j) * n_hops + k) * 8 + (h >> 1)) & M64
    hi = gid >> 32
    w = (gid & M32) ^ (((hi << 16) | (hi >> 16)) & M32) ^ k0
    w ^= w >> 16
    w = (w * 0x7FEB352D) & M32
    w ^= k1
    w ^= w >> 15
    w = (w * 0x846CA68B) & M32
    w ^= w >> 16
    field = (w >> (16 * (h & 1))) & 0xFFFF
    return inv_keep(keep_prob) if field < keep_threshold(keep_prob) else np.float32(0.0)


def words(rows: np.ndarray, cols: np.ndarray, n_cols: int, n_hops: int, k: int, n_pairs: int, seed: int, step: int) -> np.ndarray:
    """The 32-bit word of every (entry, head pair) -> uint32 ``[nnz, n_pairs]``."""
    k0, k1 = keys(seed, step)
    with np.errstate(over="ignore"):
        base = ((rows.astype(np.uint64) * np.uint64(n_cols) + cols.astype(np.uint64)) * np.uint64(n_hops) + np.uint64(k)) * np.uint64(8)
        gid = base[:, None] + np.arange(n_pairs, dtype=np.uint64)[None, :]
        hi = (gid >> np.uint64(32)).astype(np.uint32)
        w = gid.astype(np.uint32) ^ ((hi << np.uint32(16)) | (hi >> np.uint32(16))) ^ np.uint32(k0)
        w ^= w >> np.uint32(16)
        w *= np.uint32(0x7FEB352D)
        w ^= np.uint32(k1)
        w ^= w >> np.uint32(15)
        w *= np.uint32(0x846CA68B)
        w ^= w >> np.uint32(16)
    return w


def kept(rowptr, colidx, n_cols: int, n_hops: int, k: int, K: int, keep_prob: float, seed: int, step: int) -> np.ndarray:
    """bool ``[nnz_k, K]``: which (entry, head) the mask keeps."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    cols = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    w = words(rows, cols, n_cols, n_hops, k, (K + 1) // 2, seed, step)
    heads = np.arange(K)
    field = (w[:, heads >> 1] >> (16 * (heads & 1)).astype(np.uint32)[None, :]) & np.uint32(0xFFFF)
    return field < np.uint32(keep_threshold(keep_prob)) if keep_threshold(keep_prob) < 65536 else np.ones(field.shape, dtype=bool)


def factors(rowptr, colidx, n_cols: int, n_hops: int, k: int, K: int, keep_prob: float, seed: int, step: int) -> np.ndarray:
    """float32 ``[nnz_k, K]``: ``1 / keep_prob`` (one fp32 division) where kept, ``+0`` where dropped."""
    return np.where(kept(rowptr, colidx, n_cols, n_hops, k, K, keep_prob, seed, step), inv_keep(keep_prob), np.float32(0.0)).astype(np.float32)
