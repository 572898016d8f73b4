"""CPU suite: the attention dropout generator as include/h2gcn_hip.h states it, through its numpy restatement
(attention_dropout_ref.py, which the GPU suite holds the kernels to bit for bit): the scalar and the vectorised form agree, the
factor depends on (seed, step, hop, row, column, head) alone, and the mask has the statistics of independent draws."""
import numpy as np
import pytest
import scipy.sparse as sp

import attention_dropout_ref as ref
from test_spmm_values_gpu import square_hops

SEED = 0x1234_5678_9ABC_DEF1


def small_pattern(seed=0, n_rows=23, n_cols=37):
    m = sp.random(n_rows, n_cols, density=0.2, random_state=seed, format="csr")
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


@pytest.mark.parametrize("keep", (0.5, 0.4, 0.9375, 1.0))
@pytest.mark.parametrize("n_heads", (1, 3, 8, 16))
def test_scalar_and_vectorised_restatement_agree(n_heads, keep):
    rowptr, colidx = small_pattern()
    n_cols, n_hops, k = 37, 3, 2
    for seed, step in ((SEED, 0), (7, 2 ** 40 + 3)):
        got = ref.factors(rowptr, colidx, n_cols, n_hops, k, n_heads, keep, seed, step)
        assert got.dtype == np.float32 and got.shape == (len(colidx), n_heads)
        rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        want = np.array([[ref.factor_scalar(int(i), int(j), k, h, n_cols, n_hops, keep, seed, step) for h in range(n_heads)]
                         for i, j in zip(rows, colidx)], dtype=np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert set(np.unique(got)) <= {np.float32(0), np.float32(1) / np.float32(keep)}


def test_a_large_graph_uses_the_high_word():
    """gid beyond 2^32: the rotation of the high word enters, and 64-bit wrap-around is the header's modulo 2^64."""
    for i, j, n_cols in ((3_000_000, 2_999_999, 3_000_000), (2 ** 40, 5, 2 ** 41)):
        rowptr = np.zeros(2, dtype=np.int64)
        rowptr[1] = 1
        vec = ref.words(np.array([i]), np.array([j]), n_cols, 2, 1, 8, SEED, 5)
        for hp in range(8):
            k0, k1 = ref.keys(SEED, 5)
            gid = (((i * n_cols + j) * 2 + 1) * 8 + hp) & ref.M64
            hi = gid >> 32
            w = (gid & ref.M32) ^ (((hi << 16) | (hi >> 16)) & ref.M32) ^ k0
            w ^= w >> 16
            w = (w * 0x7FEB352D) & ref.M32
            w ^= k1
            w ^= w >> 15
            w = (w * 0x846CA68B) & ref.M32
            w ^= w >> 16
            assert int(vec[0, hp]) == w


def test_the_factor_depends_on_hop_row_column_head_seed_and_step_only():
    rowptr, colidx = small_pattern(1)
    n_rows, n_cols, n_hops, n_heads, keep = 23, 37, 2, 8, 0.4
    base = ref.factors(rowptr, colidx, n_cols, n_hops, 1, n_heads, keep, SEED, 4)
    rows = np.repeat(np.arange(n_rows), np.diff(rowptr))
    # permuting the entries within every row permutes the factors
    rng = np.random.default_rng(0)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(rowptr[:-1], rowptr[1:])]).astype(np.int64)
    assert np.array_equal(ref.factors(rowptr, colidx[perm], n_cols, n_hops, 1, n_heads, keep, SEED, 4), base[perm])
    # a sub-pattern (other rows_per_wave, other neighbours, another selection) leaves the factors of its entries alone
    pick = np.flatnonzero(rng.uniform(size=len(colidx)) < 0.5)
    sub_rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[pick], minlength=n_rows))]).astype(np.int64)
    assert np.array_equal(ref.factors(sub_rowptr, colidx[pick], n_cols, n_hops, 1, n_heads, keep, SEED, 4), base[pick])
    # head h of K heads is head h of any other head count
    assert np.array_equal(ref.factors(rowptr, colidx, n_cols, n_hops, 1, 3, keep, SEED, 4), base[:, :3])
    # the transposed pattern, keyed by the FORWARD (row, column) as the column side keys it, gives the transposed factors
    t = sp.csr_matrix((np.arange(1, len(colidx) + 1), colidx, rowptr), shape=(n_rows, n_cols)).T.tocsr()
    t.sort_indices()
    t_rows = np.repeat(np.arange(n_cols), np.diff(t.indptr))                         # = the forward column
    w = ref.words(t.indices.astype(np.int64), t_rows.astype(np.int64), n_cols, n_hops, 1, 4, SEED, 4)
    heads = np.arange(n_heads)
    t_kept = ((w[:, heads >> 1] >> (16 * (heads & 1)).astype(np.uint32)[None, :]) & np.uint32(0xFFFF)) < ref.keep_threshold(keep)
    assert np.array_equal(t_kept, (base != 0)[t.data - 1])
    # every argument of the key matters
    for other in (ref.factors(rowptr, colidx, n_cols, n_hops, 0, n_heads, keep, SEED, 4),
                  ref.factors(rowptr, colidx, n_cols, n_hops, 1, n_heads, keep, SEED + 1, 4),
                  ref.factors(rowptr, colidx, n_cols, n_hops, 1, n_heads, keep, SEED, 5),
                  ref.factors(rowptr, colidx, n_cols + 1, n_hops, 1, n_heads, keep, SEED, 4)):
        assert not np.array_equal(other, base)


def test_thresholds():
    assert ref.keep_threshold(1.0) == 65536 and ref.keep_threshold(0.5) == 32768 and ref.keep_threshold(0.9375) == 61440
    assert ref.keep_threshold(0.4) == int(float(np.float32(0.4)) * 65536.0) == 26214
    rowptr, colidx = small_pattern(2)
    assert bool((ref.factors(rowptr, colidx, 37, 2, 0, 16, 1.0, SEED, 1) == 1).all()), "thr = 65536 keeps all"
    assert ref.inv_keep(0.4) == np.float32(1) / np.float32(0.4)


@pytest.mark.parametrize("keep", (0.5, 0.4, 0.9375))
def test_statistics_on_the_square_graph(keep):
    """Within 5 sigma of independent draws with p = thr / 65536: the kept share overall, per head and per hop, and the share of
    positions in which two consecutive steps differ (2 p (1 - p))."""
    hops = square_hops()
    n_heads, p = 8, ref.keep_threshold(keep) / 65536.0
    kept = [[ref.kept(m.indptr, m.indices, m.shape[1], 2, k, n_heads, keep, SEED, step) for k, m in enumerate(hops)] for step in (6, 7)]

    def within(share, q, n, what):
        sigma = np.sqrt(q * (1 - q) / n)
        assert abs(share - q) <= 5 * sigma, f"{what}: {share:.5f} against {q:.5f}, {abs(share - q) / sigma:.1f} sigma (n = {n})"

    both = np.concatenate(kept[0])
    within(both.mean(), p, both.size, "all samples")
    for h in range(n_heads):
        within(both[:, h].mean(), p, both.shape[0], f"head {h}")
    for k in range(2):
        within(kept[0][k].mean(), p, kept[0][k].size, f"hop {k}")
    differ = np.concatenate(kept[0]) != np.concatenate(kept[1])
    within(differ.mean(), 2 * p * (1 - p), differ.size, "two consecutive steps")
