"""CPU suite: the numpy restatement of the recomputing attention backward (attention_backward_ref.py) against the two autograd
replicas the GPU suites already trust -- test_attention_recompute_gpu.dense_grads and test_attention_dropout_gpu.dense_grads with
the mask of attention_dropout_ref.factors -- in fp64 within 1e-12, its magnitude arrays against a brute-force loop, and the
operands of the sweep (attention_backward_ref.sweep_hops) against what tests/test_attention_backward_sweep_gpu.py says of them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import attention_backward_ref as ref
import attention_dropout_ref as dropout_ref
import spmm_driver as drv
from test_attention_dropout_gpu import dense_grads as dense_grads_dropout
from test_attention_recompute_gpu import dense_grads

RTOL = 1e-12
SEED, STEP, KEEP = 0x1234_5678_9ABC_DEF1, 9, 0.5


def random_graph(n_rows, n_cols, density, seed):
    """Two random hops; row 2 and the last column are empty in both."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        mask = rng.random((n_rows, n_cols)) < density
        mask[2, :] = False
        mask[:, -1] = False
        m = sp.csr_matrix(mask.astype(np.float32))
        m.sort_indices()
        out.append(m)
    return tuple(out)


def operands(hops, d, k, seed):
    n_rows, n_cols = hops[0].shape
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n_cols, d)), rng.uniform(-3, 3, (n_rows, 2, k)), rng.uniform(-3, 3, (n_cols, 2, k)),
            rng.uniform(-1, 1, (n_rows, 2, d)))


def close(got, want, where):
    scale = np.abs(want).max()
    assert scale > 0, where
    err = np.abs(got - want).max() / scale
    assert err <= RTOL, f"{where}: relative error {err:.3e}"


GRAPHS = [(23, 31, 0.3, 12, 3, 1), (40, 40, 0.15, 20, 5, 2)]      # (n_rows, n_cols, density, d, K, seed)


@pytest.mark.parametrize("n_rows,n_cols,density,d,k,seed", GRAPHS)
def test_restatement_equals_the_autograd_replica(n_rows, n_cols, density, d, k, seed):
    hops = random_graph(n_rows, n_cols, density, seed)
    x, l, r, g = operands(hops, d, k, seed)
    (delta, dl, dr, dx), mags = ref.backward(hops, x, l, r, g, 0.2)
    want = dense_grads(hops, x, l, r, g, 0.2, torch.float64)
    for name, got, w in zip(("dl", "dr", "dx"), (dl, dr, dx), want):
        close(got, w, name)
    assert not dl[2].any() and not delta[2].any() and not dr[-1].any() and not dx[-1].any(), "an empty segment is not an exact zero"
    assert all(not m[2].any() for m in mags[:2]) and all(not m[-1].any() for m in mags[2:])
    assert all((m >= 0).all() for m in mags)


@pytest.mark.parametrize("n_rows,n_cols,density,d,k,seed", GRAPHS)
def test_restatement_with_factors_equals_the_dropout_replica(n_rows, n_cols, density, d, k, seed):
    hops = random_graph(n_rows, n_cols, density, seed)
    x, l, r, g = operands(hops, d, k, seed)
    factors, dense_f = [], []
    for s, m in enumerate(hops):
        f = dropout_ref.factors(m.indptr, m.indices, n_cols, 2, s, k, KEEP, SEED, STEP)
        assert 0.2 < (f != 0).mean() < 0.8
        full = torch.zeros((n_rows, n_cols, k), dtype=torch.float64)
        full[torch.from_numpy(ref.coo_rows(m)), torch.from_numpy(m.indices.astype(np.int64))] = torch.from_numpy(f).double()
        factors.append(f)
        dense_f.append(full)
    (_, dl, dr, dx), _ = ref.backward(hops, x, l, r, g, 0.2, factors)
    want = dense_grads_dropout(hops, x, l, r, g, 0.2, torch.float64, dense_f)
    for name, got, w in zip(("dl", "dr", "dx"), (dl, dr, dx), want):
        close(got, w, name)
    plain = ref.backward(hops, x, l, r, g, 0.2)[0]
    assert not np.array_equal(plain[3], dx), "the factors changed nothing"


def test_delta_is_the_sum_of_alpha_dalpha_and_fp32_runs_in_fp32():
    hops = random_graph(23, 31, 0.3, 1)
    x, l, r, g = operands(hops, 12, 3, 1)
    (delta, dl, dr, dx), _ = ref.backward(hops, x, l, r, g, 0.2)
    # in exact arithmetic <g, y>_h = sum_e alpha * dalpha, hence the dpre of every segment sum to zero where the slope is 1
    flat = ref.backward(hops, x, l, r, g, 1.0)[0][1]
    assert np.abs(flat).max() <= 1e-13
    out32, mags32 = ref.backward(hops, x, l, r, g, 0.2, dtype=np.float32)
    assert all(t.dtype == np.float32 for t in out32 + mags32)
    for a, b in zip(out32, (delta, dl, dr, dx)):
        err = np.abs(a - b).max() / np.abs(b).max()
        assert 0 < err < 1e-5


def test_magnitudes_equal_a_brute_force_loop():
    n_rows, n_cols, d, k, slope = 7, 9, 8, 2, 0.2
    w = d // k
    hops = random_graph(n_rows, n_cols, 0.4, 5)
    x, l, r, g = operands(hops, d, k, 5)
    factors = [dropout_ref.factors(m.indptr, m.indices, n_cols, 2, s, k, KEEP, SEED, STEP) for s, m in enumerate(hops)]
    for fs in (None, factors):
        _, (m_delta, m_dl, m_dr, m_dx) = ref.backward(hops, x, l, r, g, slope, fs)
        b_delta, b_dl, b_dr, b_dx = np.zeros((n_rows, 2, k)), np.zeros((n_rows, 2, k)), np.zeros((n_cols, 2, k)), np.zeros((n_cols, d))
        for s, m in enumerate(hops):
            for i in range(n_rows):
                lo, hi = m.indptr[i], m.indptr[i + 1]
                for h in range(k):
                    cs = slice(h * w, (h + 1) * w)
                    pre = [l[i, s, h] + r[m.indices[e], s, h] for e in range(lo, hi)]
                    sc = [p if p > 0 else p * slope for p in pre]
                    ex = [np.exp(v - max(sc)) for v in sc]
                    alpha = [v / sum(ex) for v in ex]
                    f = [1.0 if fs is None else float(fs[s][e, h]) for e in range(lo, hi)]
                    y = sum((a * ff * x[m.indices[e], cs] for a, ff, e in zip(alpha, f, range(lo, hi))), np.zeros(w))
                    b_delta[i, s, h] = np.abs(g[i, s, cs] * y).sum()
                    for a, ff, p, e in zip(alpha, f, pre, range(lo, hi)):
                        j = m.indices[e]
                        term = a * (ff * np.abs(g[i, s, cs] * x[j, cs]).sum() + b_delta[i, s, h]) * (1.0 if p > 0 else slope)
                        b_dl[i, s, h] += term
                        b_dr[j, s, h] += term
                        b_dx[j, cs] += a * ff * np.abs(g[i, s, cs])
        for name, got, want in zip(("delta", "dl", "dr", "dx"), (m_delta, m_dl, m_dr, m_dx), (b_delta, b_dl, b_dr, b_dx)):
            close(got, want, name)
            assert np.array_equal(got == 0, want == 0), name


def test_rho_weighs_every_element_by_its_own_terms():
    want, mag = np.array([100.0, 1e-3, 0.0]), np.array([200.0, 2e-3, 0.0])
    got = want + np.array([0.0, 1e-4, 0.0])
    assert ref.rho(got, want, mag) == pytest.approx(0.05)                               # (max |err| / max |want| would say 1e-6)
    assert np.isnan(ref.rho(np.array([np.nan, 0, 0]), want, mag))
    assert ref.zeros_exact(np.array([5.0, 1.0, 0.0], np.float32), mag)
    assert not ref.zeros_exact(np.array([5.0, 1.0, -0.0], np.float32), mag) and ref.zeros_exact(np.array([5.0, 1.0, -0.0], np.float32), mag, True)
    assert not ref.zeros_exact(np.array([5.0, 1.0, 1e-30], np.float32), mag, True)


def test_sweep_operands_have_the_prescribed_lengths_on_both_sides():
    hops = ref.sweep_hops()
    lengths = sorted(ref.SWEEP_LENGTHS)
    n_rows_block = len(ref.SWEEP_LENGTHS)
    by_row, by_col = [], []
    for m in hops:
        assert m.shape == (371, 371) and m.nnz == 7274 and m.has_sorted_indices
        rows, cols = drv.row_lengths(m), drv.transposed_lengths(m)
        assert sorted(rows[:n_rows_block]) == lengths, "the first block does not put every length on a row"
        assert sorted(cols[ref.SWEEP_SIDE:]) == lengths, "the second block does not put every length on a column"
        assert set(lengths) <= set(rows) and set(lengths) <= set(cols)
        assert cols[ref.SWEEP_SIDE - 1] == 0 and rows[-1] == 0, "a node nobody references"
        by_row.append(rows)
        by_col.append(cols)
    for name, (a, b) in (("rows", by_row), ("columns", by_col)):
        mixed = int((((a >= 256) & (b < 32)) | ((b >= 256) & (a < 32))).sum())
        assert mixed == 6, f"{name}: {mixed} are long in one hop and under 32 in the other"
