"""GPU suite: the fused attention forward (HopPlan.attention_heads / hop_attention_heads, h2gcn_amd/csrc/attention_fused.hip).

The contract is the chain's bits: every comparison is torch.equal on the int32 view against edge_scores_heads -> row_softmax_heads
-> spmm_values run in the same test on the same operands.  Outputs are guarded views in NaN-filled buffers, launched twice
(spmm_driver._launch_twice).  The operands with prescribed segment lengths are those of test_spmm_values_gpu."""
import functools

import numpy as np
import pytest
import torch

import spmm_driver as drv
import test_attention_heads_gpu as heads_gpu
import test_spmm_values_gpu as values_gpu
from test_spmm_values_gpu import DEV, GRID_HEADS, GRID_K1, N_BIG, N_SMALL, THRESHOLDS, bits, launch, make_plan, strided_rows

pytestmark = pytest.mark.gpu


def node_terms(n_rows, n_cols, h_sel, n_heads, seed):
    """l [n_rows, h_sel, K], r [n_cols, h_sel, K] on the host: scores of a few units either way, so that no softmax is flat."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-3, 3, (n_rows, h_sel, n_heads)).astype(np.float32), rng.uniform(-3, 3, (n_cols, h_sel, n_heads)).astype(np.float32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def chain(plan, x, l, r, slope=0.2, hops=None, out=None):
    """The three launches the fused one stands for."""
    with torch.no_grad():
        alpha = plan.row_softmax_heads(plan.edge_scores_heads(l, r, slope, hops=hops), hops=hops)
        return plan.spmm_values(x, alpha, hops=hops, out=out)


def fused_equals_chain(plan, x, l, r, where, slope=0.2, hops=None):
    h_sel = plan.n_selected(hops)
    got = launch(lambda out: plan.attention_heads(x, l, r, slope, hops=hops, out=out), (plan.n_rows, h_sel, x.shape[1]), where)
    want = chain(plan, x, l, r, slope, hops)
    assert not bool(torch.isnan(want).any()), where + ": the chain's own result has a NaN"
    assert torch.equal(bits(got), bits(want)), where + ": the fused launch differs from the chain"
    return got


# ------------------------------------------------------------------ 1. segment classes
@pytest.mark.parametrize("rpw", (1, 3, 7))
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_segment_classes(thr, rpw):
    hops = values_gpu.forward_hops()
    assert hops[0].shape == (N_SMALL, N_BIG)                                      # n_rows != n_cols
    plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
    for d, n_heads in ((128, 8), (20, 1), (48, 3)):
        l, r = node_terms(N_SMALL, N_BIG, 2, n_heads, seed=thr + rpw)
        x, _ = values_gpu.operands(d)
        fused_equals_chain(plan, dev(x), dev(l), dev(r), f"thr {thr} rpw {rpw} d {d} K {n_heads}", slope=0.2 if n_heads > 1 else 0.01)


# ------------------------------------------------------------------ 2. the (d, K) grid, strided operands
@pytest.mark.parametrize("d,n_heads", GRID_K1 + GRID_HEADS)
def test_the_grid_on_strided_operands(d, n_heads):
    hops = values_gpu.forward_hops()
    l, r = node_terms(N_SMALL, N_BIG, 2, n_heads, seed=d)
    x, _ = values_gpu.operands(d)
    xt, lt, rt = strided_rows(x), strided_rows(l), strided_rows(r)
    assert xt.stride(0) == d + 4 and lt.stride(0) == 2 * n_heads + 4 and rt.stride(0) == 2 * n_heads + 4
    for thr in THRESHOLDS:
        plan = make_plan(hops, long_row_threshold=thr)
        where = f"d {d} K {n_heads} thr {thr}"
        want = chain(plan, xt, lt, rt)
        # Y goes into a wider NaN-filled buffer through ldy_row AND ldy_hop: a guard band after every hop slot
        wide = torch.full((N_SMALL, 2, d + 2 * drv.GUARD), float("nan"), dtype=torch.float32, device=DEV)
        y = plan.attention_heads(xt, lt, rt, out=wide[:, :, drv.GUARD:drv.GUARD + d])
        assert y.stride(1) == d + 2 * drv.GUARD and y.data_ptr() == wide[:, :, drv.GUARD:].data_ptr()
        assert bool(torch.isnan(wide[:, :, :drv.GUARD]).all()) and bool(torch.isnan(wide[:, :, drv.GUARD + d:]).all()), where + ": a guard column was written"
        assert torch.equal(bits(y), bits(want)), where
        assert torch.equal(bits(plan.attention_heads(xt, lt, rt)), bits(want)), where + " (out allocated by the call)"


# ------------------------------------------------------------------ 3. selections and plan kinds
def test_hop_selections():
    hops = values_gpu.forward_hops()
    d, n_heads = 64, 4
    x, _ = values_gpu.operands(d)
    l, r = node_terms(N_SMALL, N_BIG, 2, n_heads, seed=1)
    xt, lt, rt = dev(x), dev(l), dev(r)
    plan = make_plan(hops, long_row_threshold=256)
    both = fused_equals_chain(plan, xt, lt, rt, "both hops")
    for k in range(2):
        alone = fused_equals_chain(plan, xt, lt[:, k:k + 1], rt[:, k:k + 1], f"hop {k} alone", hops=[k])   # (slices: ldl = 2 K)
        assert torch.equal(bits(alone), bits(both[:, k:k + 1])), f"hop {k} alone differs from its slot of the launch on both"


def test_eight_hops_fill_the_row_pointer_lanes():
    d, n_heads = 64, 2
    hops = values_gpu.forward_hops(8)
    plan = make_plan(hops, long_row_threshold=256, rows_per_wave=7)
    x = np.random.default_rng(8).uniform(-1, 1, (N_BIG, d)).astype(np.float32)
    l, r = node_terms(N_SMALL, N_BIG, 8, n_heads, seed=8)
    fused_equals_chain(plan, dev(x), dev(l), dev(r), "8 hops, 7 rows per wave")


def test_sub_plan_symmetric_plan_and_plan_without_transposes():
    d, n_heads = 128, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    rng = np.random.default_rng(9)
    x = dev(rng.uniform(-1, 1, (n, d)).astype(np.float32))
    l, r = (dev(t) for t in node_terms(n, n, 2, n_heads, seed=9))
    plain = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    y = fused_equals_chain(plain, x, l, r, "square plan")
    sym = make_plan(hops, build_transpose=True, keep_permutation=True, symmetric_pattern=True, long_row_threshold=256)
    assert sym.transpose_sharing[0] != "none"
    assert torch.equal(bits(fused_equals_chain(sym, x, l, r, "symmetric plan")), bits(y))
    bare = make_plan(hops, build_transpose=False, long_row_threshold=256)
    assert not bare.has_transpose
    assert torch.equal(bits(fused_equals_chain(bare, x, l, r, "plan without transposes")), bits(y))
    rows = np.sort(rng.choice(n, 211, replace=False))
    sub = plain.select_rows(torch.from_numpy(rows), build_transpose=False)
    rows_dev = torch.from_numpy(rows).to(DEV)
    ys = fused_equals_chain(sub.plan, x, l[rows_dev], r, "sub-plan of selected rows")
    assert torch.equal(bits(ys), bits(y[rows_dev])), "the sub-plan's rows differ from the same rows of the full plan"


# ------------------------------------------------------------------ 4. special values
def same_bits_nan_aware(got, want):
    """NaN in the same places (the payload is not specified), every other element bit for bit."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    return torch.equal(nan_g, nan_w) and torch.equal(got.view(torch.int32)[~nan_g], want.view(torch.int32)[~nan_w])


SPECIALS = (np.nan, np.inf, -np.inf, 1e-40, -0.0, 1e30)
HARMLESS = (1e-40, -0.0, 1e30, -1e-42)


@functools.lru_cache(maxsize=None)
def special_operands(d=32, n_heads=8):
    """x, l, r on the 600-node square graph with NaN, +-inf, subnormals, -0 and 1e30 planted: whole rows of l (all heads of one hop),
    single (node, hop, head) elements of l and r, and 0.1 % of the elements of x -- sparse enough that most of the chain's output
    stays finite (the rows here have some 250 entries: every planted element of x reaches a few hundred outputs)."""
    n = values_gpu.square_hops()[0].shape[0]
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    l, r = node_terms(n, n, 2, n_heads, seed=77)
    for i, row in enumerate(rng.choice(n, 6, replace=False)):                     # a few rows of l
        l[row, i % 2, :] = SPECIALS[i]
    for i in range(36):                                                           # single heads of l
        l[rng.integers(n), rng.integers(2), rng.integers(n_heads)] = SPECIALS[i % 6]
    for i, col in enumerate(rng.choice(n, 12, replace=False)):                    # a few columns of r, one head each
        r[col, i % 2, rng.integers(n_heads)] = SPECIALS[i % 6]
    hit = rng.random(x.shape) < 0.001
    x[hit] = np.asarray(SPECIALS, dtype=np.float32)[rng.integers(0, 6, int(hit.sum()))]
    return x, l, r


def test_special_values_have_the_chains_bits():
    d, n_heads = 32, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    x, l, r = (dev(t) for t in special_operands(d, n_heads))
    for thr in (32, 1024):
        plan = values_gpu.adjoint_plan(hops, long_row_threshold=thr)
        want = chain(plan, x, l, r)
        frac = float(torch.isnan(want).float().mean())
        print(f"thr {thr}: {100 * frac:.1f} % of the chain's output is NaN")
        assert 0.05 <= frac <= 0.75, f"the comparison would be vacuous: {100 * frac:.1f} % of the chain's output is NaN"
        got = launch(lambda out: plan.attention_heads(x, l, r, out=out), (n, 2, d), f"specials thr {thr}")
        assert same_bits_nan_aware(got, want), f"thr {thr}: NaN positions or bits differ from the chain"


def test_a_nan_stays_inside_its_head():
    d, n_heads, bad = 32, 8, 5
    w = d // n_heads
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    rng = np.random.default_rng(78)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    l, r = node_terms(n, n, 2, n_heads, seed=78)
    for t in (x, l, r):                                                           # subnormals, -0, 1e30 everywhere: finite results
        hit = rng.random(t.shape) < 0.01
        t[hit] = np.asarray(HARMLESS, dtype=np.float32)[rng.integers(0, 4, int(hit.sum()))]
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    clean = fused_equals_chain(plan, dev(x), dev(l), dev(r), "subnormals, -0 and 1e30")
    keep = [c for c in range(d) if c // w != bad]
    for v in (np.nan, np.inf, -np.inf):
        x2, l2, r2 = x.copy(), l.copy(), r.copy()
        l2[rng.choice(n, 20, replace=False), :, bad] = v
        r2[rng.choice(n, 3, replace=False), :, bad] = v
        x2[rng.choice(n, 3, replace=False), bad * w + 1] = v
        got = launch(lambda out: plan.attention_heads(dev(x2), dev(l2), dev(r2), out=out), (n, 2, d), f"head {bad} holds {v}")
        assert same_bits_nan_aware(got, chain(plan, dev(x2), dev(l2), dev(r2)))
        assert torch.equal(bits(got[:, :, keep]), bits(clean[:, :, keep])), f"{v} in head {bad} changed a bit of another head"
        assert bool(torch.isnan(got[:, :, bad * w:(bad + 1) * w]).any())


# ------------------------------------------------------------------ 5. no per-entry arrays
def test_the_fused_launch_allocates_no_per_entry_array():
    d, n_heads = 32, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    x = dev(np.random.default_rng(5).uniform(-1, 1, (n, d)).astype(np.float32))
    l, r = (dev(t) for t in node_terms(n, n, 2, n_heads, seed=5))
    out = torch.empty((n, 2, d), dtype=torch.float32, device=DEV)
    one_array = hops[0].nnz * n_heads * 4

    def extra(fn):
        fn()                                                                      # (whatever the first launch of a selection sets up)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused, chained = extra(lambda: plan.attention_heads(x, l, r, out=out)), extra(lambda: chain(plan, x, l, r, out=out))
    print(f"extra device memory: fused {fused} B, chain {chained} B; one [nnz_0, K] fp32 array {one_array} B")
    assert fused < one_array
    assert chained >= 2 * one_array


# ------------------------------------------------------------------ 6. the front end
@functools.lru_cache(maxsize=None)
def graphs():
    """(name, Graph) of the crafted 600-node graph and of Cora, as test_attention_heads_gpu builds them."""
    return (("crafted", heads_gpu.Graph(values_gpu.square_hops())), ("cora", heads_gpu.Graph(values_gpu.cora_hops())))


LINKS = ("edge_scores", "edge_scores_heads", "row_softmax", "row_softmax_heads", "spmm_values", "spmm", "sddmm", "sddmm_heads")


def test_no_grad_is_one_launch_and_a_gradient_takes_the_chain(monkeypatch):
    from h2gcn_amd import HopPlan, hop_attention_heads, hop_edge_scores_heads, hop_softmax_heads, hop_spmm_values

    d, n_heads = 32, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    x = dev(np.random.default_rng(6).uniform(-1, 1, (n, d)).astype(np.float32))
    l, r = (dev(t) for t in node_terms(n, n, 2, n_heads, seed=6))
    rr = heads_gpu.uniform((n, 2, d), 61)
    vals = [v.clone() for v in plan.vals]
    want = chain(plan, x, l, r)

    # with a gradient: the chain's output and the chain's gradients
    grads = []
    for fn in (lambda a, b, c: hop_attention_heads(plan, a, b, c, 0.2),
               lambda a, b, c: hop_spmm_values(plan, a, hop_softmax_heads(plan, hop_edge_scores_heads(plan, b, c, 0.2)))):
        a, b, c = (t.clone().requires_grad_(True) for t in (x, l, r))
        y = fn(a, b, c)
        assert y.requires_grad and torch.equal(bits(y), bits(want))
        (y * rr).sum().backward()
        grads.append((a.grad, b.grad, c.grad))
    for name, g, h in zip(("dx", "dl", "dr"), *grads):
        assert torch.equal(bits(g), bits(h)) and float(g.abs().max()) > 0, name

    # without one: exactly one library launch, no link of the chain
    launches = []
    real = HopPlan.attention_heads
    for name in LINKS:
        monkeypatch.setattr(HopPlan, name, lambda *a, **k: pytest.fail("a link of the chain was launched"))
    monkeypatch.setattr(HopPlan, "attention_heads", lambda self, *a, **k: launches.append(1) or real(self, *a, **k))
    y = hop_attention_heads(plan, x, l, r)                                        # nothing requires a gradient
    assert len(launches) == 1 and not y.requires_grad and torch.equal(bits(y), bits(want))
    with torch.no_grad():
        y = hop_attention_heads(plan, x.clone().requires_grad_(True), l[:, 1:2].clone().requires_grad_(True), r[:, 1:2], hops=[1])
    assert len(launches) == 2 and not y.requires_grad and torch.equal(bits(y), bits(want[:, 1:2]))
    monkeypatch.undo()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plan.vals, vals)), "the plan's values changed"


@pytest.mark.parametrize("heads", (1, 4, 8))
def test_layer_without_gradients_has_the_bits_of_the_layer_with(heads, monkeypatch):
    """The layer stays on the chain in every gradient mode (the launch is not faster at every shape); the one launch on the
    layer's own projections gives the layer's bits."""
    from h2gcn_amd import HopPlan, MultiHeadHopAttention, hop_attention_heads

    d = 32
    w = d // heads
    for name, graph in graphs():
        plan = graph.plan(**heads_gpu.KNOBS[0]) if name == "crafted" else graph.plan()
        x = heads_gpu.uniform((graph.n, d), 21)
        torch.manual_seed(23)
        layer = MultiHeadHopAttention(d, heads).to(DEV)
        vals = [v.clone() for v in plan.vals]
        with_grad = layer(plan, x)
        assert with_grad.requires_grad
        with torch.no_grad():
            without = layer(plan, x)
            ls = [x[:, h * w:(h + 1) * w] @ layer.a_l[:, h, :].t() for h in range(heads)]
            rs = [x[:, h * w:(h + 1) * w] @ layer.a_r[:, h, :].t() for h in range(heads)]
            for link in LINKS:
                monkeypatch.setattr(HopPlan, link, lambda *a, **k: pytest.fail("a link of the chain was launched"))
            fused = hop_attention_heads(plan, x, torch.stack(ls, dim=2), torch.stack(rs, dim=2), layer.negative_slope, layer.hops)
            monkeypatch.undo()
        assert not without.requires_grad and not fused.requires_grad
        assert torch.equal(bits(without), bits(with_grad)), f"{name}, {heads} heads: the no_grad forward differs from the grad-enabled one"
        assert torch.equal(bits(fused), bits(with_grad)), f"{name}, {heads} heads: the one launch differs from the layer"
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plan.vals, vals)), "the plan's values changed"


def test_captured_no_grad_forward_replays_to_the_eager_result():
    from h2gcn_amd import hop_attention_heads

    d, n_heads = 32, 8
    crafted = graphs()[0][1]
    plan = crafted.plan(**heads_gpu.KNOBS[0])
    n = crafted.n
    x = heads_gpu.uniform((n, d), 41)
    l, r = heads_gpu.uniform((n, 2, n_heads), 43) * 3, heads_gpu.uniform((n, 2, n_heads), 44) * 3
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = hop_attention_heads(plan, x, l, r)                            # the eager warm-up
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(bits(eager), bits(chain(plan, x, l, r)))
        static_x = x.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = hop_attention_heads(plan, static_x, l, r)
        y.fill_(float("nan"))                                                     # (capture runs nothing)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(eager))
        static_x.copy_(heads_gpu.uniform((n, d), 42))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(chain(plan, static_x, l, r))) and not torch.equal(bits(y), bits(eager))
