"""tests/edge_scores_dynamic_ref.py held to an independent restatement -- dense torch fp64 under autograd for scores, du, dv and da,
a brute-force Python loop for the magnitude arrays -- and the exact-operand generator of tests/test_edge_scores_dynamic_sweep_gpu.py
held to its condition.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import attention_backward_ref as sweep
import edge_scores_dynamic_ref as ref
import test_edge_scores_dynamic_sweep_gpu as sweep_gpu

N = 40
SLOPE = 0.2


def small_hops():
    out = []
    for k in range(2):
        full = sp.random(N, N, density=0.15, format="csr", random_state=np.random.default_rng(7 + k), dtype=np.float32).toarray()
        full[11 + k, :] = full[:, 13 + k] = 0                # a row and a column without entries
        m = sp.csr_matrix(full)
        m.sort_indices()
        out.append(sp.csr_matrix((m.data, m.indices.astype(np.int32), m.indptr.astype(np.int64)), shape=m.shape))
    assert all(m.nnz > 100 for m in out) and any((np.diff(m.indptr) == 0).any() for m in out)
    return tuple(out)


def small_case(d, k, sel):
    hops = small_hops()
    rng = np.random.default_rng(100 * d + k)
    u, v = (rng.uniform(-1, 1, (N, d)).astype(np.float32) for _ in range(2))
    u[3, 0], v[5, 0] = 0.25, -0.25                       # p == 0 exactly: the slope branch
    a = rng.uniform(-1, 1, (len(sel), d)).astype(np.float32)
    ds = [rng.uniform(-1, 1, (hops[s].nnz, k)).astype(np.float32) for s in sel]
    return hops, u, v, a, ds


def dense(hops, u, v, a, ds, k, sel):
    """scores per selected hop, du, dv, da by dense torch fp64 operations and autograd; the branch from the fp32 sum."""
    d = u.shape[1]
    pos = torch.from_numpy(u[:, None, :] + v[None, :, :] > 0)                        # fp32 addition
    U, V, A = (torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (u, v, a))
    p = U[:, None, :] + V[None, :, :]
    q = torch.where(pos, p, p * float(np.float32(SLOPE)))
    scores, loss = [], 0
    for slot, s in enumerate(sel):
        full = (q * A[slot]).view(N, N, k, d // k).sum(dim=3)
        rows, cols = ref.entries(hops[s])
        sc = full[torch.from_numpy(rows), torch.from_numpy(cols)]
        scores.append(sc.detach().numpy())
        loss = loss + (sc * torch.from_numpy(ds[slot].astype(np.float64))).sum()
    loss.backward()
    return scores, U.grad.numpy(), V.grad.numpy(), A.grad.numpy()


def close(got, want):
    return np.abs(got - want).max(initial=0.0) <= 1e-12 * max(np.abs(want).max(initial=0.0), 1e-300)


@pytest.mark.parametrize("d,k,sel", [(10, 1, [0, 1]), (12, 3, [0, 1]), (12, 3, [1]), (7, 1, [0])])
def test_reference_equals_the_dense_autograd_restatement(d, k, sel):
    hops, u, v, a, ds = small_case(d, k, sel)
    want = dense(hops, u, v, a, ds, k, sel)
    got = ref.Reference(hops, u, v, a, k, SLOPE, ds=ds, sel=None if sel == [0, 1] else sel)
    assert len(got.scores) == len(sel) and all(close(x, y) for x, y in zip(got.scores, want[0]))
    assert close(got.du, want[1]) and close(got.dv, want[2]) and close(got.da, want[3])
    assert np.abs(want[1]).max() > 0.1 and np.abs(want[3]).max() > 0.1


@pytest.mark.parametrize("d,k,sel", [(12, 3, [0, 1]), (7, 1, [1])])
def test_magnitudes_equal_a_brute_force_loop(d, k, sel):
    hops, u, v, a, ds = small_case(d, k, sel)
    got = ref.Reference(hops, u, v, a, k, SLOPE, ds=ds, sel=sel)
    w, sl = d // k, float(np.float32(SLOPE))
    m_du, m_dv, m_da = np.zeros((N, d)), np.zeros((N, d)), np.zeros((len(sel), d))
    n_du, n_dv = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for slot, s in enumerate(sel):
        m = hops[s]
        m_sc = np.zeros((m.nnz, k))
        for i in range(N):
            for e in range(m.indptr[i], m.indptr[i + 1]):
                j = int(m.indices[e])
                n_du[i] += 1
                n_dv[j] += 1
                for c in range(d):
                    pos = np.float32(u[i, c]) + np.float32(v[j, c]) > 0
                    p = float(u[i, c]) + float(v[j, c])
                    q = p if pos else p * sl
                    g = float(ds[slot][e, c // w])
                    m_sc[e, c // w] += abs(float(a[slot, c]) * q)
                    dp = g * float(a[slot, c]) * (1.0 if pos else sl)
                    m_du[i, c] += abs(dp)
                    m_dv[j, c] += abs(dp)
                    m_da[slot, c] += abs(g * q)
        assert close(got.mag_scores[slot], m_sc)
    assert close(got.mag_du, m_du) and close(got.mag_dv, m_dv) and close(got.mag_da, m_da)
    assert np.array_equal(got.n_du, n_du) and np.array_equal(got.n_dv, n_dv) and list(got.n_da) == [hops[s].nnz for s in sel]
    assert got.w == w


def test_exact_operands_keep_every_partial_sum_an_fp32_number():
    """64 * magnitude < 2^24 at the widest head (w = 256: the scores), at the most heads, and on the operand with the most entries
    per hop (da); the exact reference is then a multiple of 1/64 that fp32 holds, and a violated condition is noticed."""
    largest = max(sweep_gpu.PARTITION_CASES, key=lambda c: sum(m.nnz for m in sweep_gpu.partition_hops(c[0], c[1])))
    for hops, shapes in ((sweep.sweep_hops(), [(256, 1), (256, 64), (1, 1)]), (sweep_gpu.partition_hops(largest[0], largest[1]), [(256, 1), (256, 4)]),
                         (sweep.sweep_hops(sweep_gpu.N_HOPS_MANY), [(256, 32)])):
        for d, k in shapes:
            u, v, a, ds = data = sweep_gpu.exact_operands(hops, d, k, seed=d + k)
            for t, unit, top in ((u, 8, 2), (v, 8, 2), (a, 4, 2), (np.concatenate(ds), 1, 2)):
                assert (t * unit == np.round(t * unit)).all() and np.abs(t).max() <= top
            assert all((np.abs(t) >= 1).all() for t in ds)
            want = sweep_gpu.reference(hops, data, k, True)                       # (asserts exact_condition)
            for t in list(want.scores) + [want.du, want.dv, want.da]:
                assert (t * 64 == np.round(t * 64)).all() and np.array_equal(t.astype(np.float32).astype(np.float64), t)
    want.mag_da[0, 0] = 2.0 ** 18
    assert not sweep_gpu.exact_condition(want)
