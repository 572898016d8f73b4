"""GPU suite: the gradient that the fused propagation hands to ``r0`` (layers._backward_walk behind fused_propagation and
fused_propagation_classify_rows) against a replica written out here -- an explicit loop over ``plan.spmm_t`` and column slices,
in the order of operations of the bf16 specification ("bf16 embeddings through the model")::

    t       = spmm_t(g_k)  accumulated and returned in fp32
    t      += slot_{k-1}(g) widened exactly to fp32
    g_{k-1} = t rounded to bf16 (nearest even)   for k > 1
    d r_0   = t, left in fp32                    for k = 1

(fp32: the same walk without the roundings; rows-only: round K through ``sel.plan``, the slot added to rows ``sel.rows``).  Same
launches, same elementwise ops, same order: ``torch.equal``, no tolerance.  Two operands, the smallest on which each branch of
the walk is taken: (a) rows of every length including one long row, where ``private_grad`` accumulates in place; (b) short rows
throughout, where the adjoint would run in the in-tile short-row mode and ``private_grad`` takes the out-of-place fallback."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
H, W0, N_LABELLED = 2, 8, 64
SHORT_ROWS = "lane group per segment (short rows)"


def _row_normalised(m):
    m = sp.csr_matrix(m, dtype=np.float32)
    m.data[:] = 1.0
    deg = np.asarray(m.sum(1)).reshape(-1)
    return sp.csr_matrix(sp.diags(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)) @ m).astype(np.float32)


def _operand_a():
    """N = 512, symmetric pattern, mean degree about 20, row (and column) 0 with >= 256 nonzeros."""
    n, hops = 512, []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        m = sp.random(n, n, 10.0 / n, format="lil", random_state=seed, dtype=np.float32)
        m[0, rng.choice(n, 300, replace=False)] = 1.0
        m = sp.csr_matrix(m)
        m = _row_normalised(m + m.T)
        assert m.getrow(0).nnz >= 256 and 12 <= m.nnz / n <= 28, (m.getrow(0).nnz, m.nnz / n)
        hops.append(m)
    return hops


def _operand_b():
    """N = 65 536, four entries in every row."""
    n, hops = 65536, []
    for seed in (3, 4):
        rng = np.random.default_rng(seed)
        cols = (np.arange(n)[:, None] + rng.integers(1, n, (n, 1)) + 16381 * np.arange(4)[None, :]) % n   # four distinct columns per row
        hops.append(sp.csr_matrix((np.full(4 * n, 0.25, np.float32), cols.reshape(-1), 4 * np.arange(n + 1)), shape=(n, n)))
    return hops


@pytest.fixture(scope="module", params=["a: n=512 with a long row", "b: n=65536 degree 4"])
def operand(request):
    from h2gcn_amd import HopPlan
    plan = HopPlan.from_scipy(_operand_a() if request.param.startswith("a") else _operand_b(), DEV, build_transpose=True)
    rows = torch.from_numpy(np.sort(np.random.default_rng(9).choice(plan.n_rows, N_LABELLED, replace=False))).to(DEV)
    if request.param.startswith("a"):
        rows[0] = 0                                   # the long row is labelled
    return request.param[0], plan, plan.select_rows(rows)


def _slots(K):
    """(offset, width) of r_0 .. r_K in [r_K | r_0 | ... | r_{K-1}], written out."""
    widths = [W0 * H ** k for k in range(K + 1)]
    return [(widths[K] + sum(widths[:k]), widths[k]) for k in range(K)] + [(0, widths[K])]


def _cols(t, slot):
    return t[:, slot[0]:slot[0] + slot[1]]


def replica(plan, G, K, bf16, sel=None):
    """d r_0 from the buffer's gradient G ([n, W]; rows-only: the compact [m, W] of rows sel.rows)."""
    slots = _slots(K)
    g_k = _cols(G, slots[K]).contiguous()
    for k in range(K, 0, -1):
        p = sel.plan if sel is not None and k == K else plan
        t = p.spmm_t(g_k.unflatten(1, (H, slots[k - 1][1])).contiguous(), out_dtype=torch.float32)
        addend = _cols(G, slots[k - 1]).float()
        if sel is None:
            t = t + addend
        else:
            t.index_add_(0, sel.rows_long, addend)
        g_k = t.to(BF) if bf16 and k > 1 else t
    assert g_k.dtype == torch.float32
    return g_k


def _r0_and_gradient(plan, K, dtype, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r0 = torch.randn((plan.n_cols, W0), device=DEV, generator=gen).requires_grad_(True)
    G = torch.randn((plan.n_rows, sum(w for _, w in _slots(K))), device=DEV, generator=gen).to(dtype)
    return r0, G


@pytest.mark.parametrize("K", (1, 2, 3))
@pytest.mark.parametrize("mode", ("fp32", "bf16"))
def test_full_walk_equals_the_written_out_loop(operand, mode, K):
    from h2gcn_amd import layers as L
    name, plan, _ = operand
    dtype = BF if mode == "bf16" else torch.float32
    r0, G = _r0_and_gradient(plan, K, dtype, 10 * K + (mode == "bf16"))
    short = plan.schedule(W0, adjoint=True)["segment_walk"]
    print(f"operand {name}: adjoint schedule at width {W0}: {short!r}; in place from the buffer's stride: "
          f"{plan.schedule(W0, ld_src=G.stride(0), adjoint=True)['segment_walk']!r}")
    if name == "b":   # the private_grad walk below must take its out-of-place fallback here
        assert short == SHORT_ROWS
        assert plan.schedule(W0, ld_src=G.stride(0), adjoint=True)["segment_walk"] == SHORT_ROWS
    want = replica(plan, G, K, mode == "bf16")
    keep = G.clone()
    L.fused_propagation(plan, r0, K, dtype=dtype).backward(G)
    assert r0.grad.dtype == torch.float32 and torch.equal(r0.grad, want), (name, mode, K)
    assert torch.equal(G, keep), "the caller's gradient tensor was modified"
    if mode == "bf16":
        return
    plain, r0.grad = r0.grad, None
    L.fused_propagation(plan, r0, K, private_grad=True).backward(G)
    assert torch.equal(r0.grad, want) and torch.equal(r0.grad, plain), (name, K)
    slot0 = _slots(K)[0]
    if name == "a":   # round 1 was accumulated into the slot of r_0 inside G: the in-place branch ran
        assert torch.equal(_cols(G, slot0), want) and not torch.equal(_cols(G, slot0), _cols(keep, slot0))
    else:             # round 1 (width 8) ran out of place
        assert torch.equal(_cols(G, slot0), _cols(keep, slot0))


@pytest.mark.parametrize("K", (1, 2, 3))
@pytest.mark.parametrize("mode", ("fp32", "bf16"))
def test_rows_only_walk_equals_the_written_out_loop(operand, mode, K):
    from h2gcn_amd import layers as L
    name, plan, sel = operand
    dtype = BF if mode == "bf16" else torch.float32
    r0, _ = _r0_and_gradient(plan, K, dtype, 20 * K + (mode == "bf16"))
    torch.manual_seed(K)
    total = sum(w for _, w in _slots(K))
    dense = L.DropoutDense(total, 7, True, 0.0, seed=5).to(DEV)          # no dropout: keep_prob 1, no step
    g = torch.randn((len(sel), 7), device=DEV, generator=torch.Generator(device=DEV).manual_seed(K))
    z = L.fused_propagation_classify_rows(plan, sel, r0, K, dense, dtype=dtype)
    z.backward(g)
    # the compact gradient of the buffer's rows sel.rows, from the classifier's own backward call (pinned by
    # test_classifier_rows_gpu.py); the walk from there on is the replica's
    with torch.no_grad():
        buf = L.fused_propagation(plan, r0, K, dtype=dtype)
        g_c, _ = L._classifier_backward(buf, dense.kernel.detach().contiguous(), g, 1.0, dense.seed, None, True, False, sel)
    assert g_c.dtype == dtype and g_c.shape == (N_LABELLED, total)
    want = replica(plan, g_c, K, mode == "bf16", sel)
    assert r0.grad.dtype == torch.float32 and torch.equal(r0.grad, want), (name, mode, K)
