"""GPU suite: the head dimension of the SDDMM, the row softmax and the edge scores (HopPlan.sddmm_heads, row_softmax_heads,
edge_scores_heads and their backwards; hop_softmax_heads / hop_edge_scores_heads; MultiHeadHopAttention on them).

The oracle is the existing single-head call: per head every new call must give ITS bits (torch.equal).  Operands: Cora
(tests/golden) and the 600-node graph of test_hop_attention_heads_gpu.py with prescribed row lengths, under three settings of
(long_row_threshold, rows_per_wave).  Measured ratios of test_autograd_functions_against_the_dense_fp64_replica: DESIGN.md."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spmm_driver as drv
from conftest import load_planetoid_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRAIN = dict(build_transpose=True, keep_permutation=True)
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025]
KNOBS = [dict(long_row_threshold=32, rows_per_wave=1), dict(long_row_threshold=256, rows_per_wave=3),
         dict(long_row_threshold=1024, rows_per_wave=7)]
U = 2.0 ** -24


class Graph:
    def __init__(self, mats):
        self.mats = [sp.csr_matrix(m).astype(np.float32) for m in mats]
        self.n = self.mats[0].shape[0]
        coo = [m.tocoo() for m in self.mats]
        self.rows = [torch.from_numpy(c.row.astype(np.int64)).to(DEV) for c in coo]
        self.cols = [torch.from_numpy(c.col.astype(np.int64)).to(DEV) for c in coo]
        self.nnz = [m.nnz for m in self.mats]
        self._plans = {}

    def plan(self, **kw):
        from h2gcn_amd import HopPlan

        key = tuple(sorted(kw.items()))
        if key not in self._plans:
            self._plans[key] = HopPlan.from_scipy(self.mats, DEV, **{**TRAIN, **kw})
        return self._plans[key]


@pytest.fixture(scope="module")
def cora():
    g = load_planetoid_golden("cora")
    return Graph([g["hop1_sym"], g["hop2_sym"]])


@pytest.fixture(scope="module")
def crafted():
    n, mats = 600, []
    for k in range(2):
        base = LENGTHS[7 * k:] + LENGTHS[:7 * k]
        lens = [min(v, n - 1) for v in (base * (n // len(base) + 1))[:n]]
        a = drv.hop_from_lengths(lens, n, seed=71 + k)
        pat = ((a != 0) + (a != 0).T).tocsr()
        pat.sort_indices()
        mats.append(sp.csr_matrix((np.ones(pat.nnz, dtype=np.float32), pat.indices, pat.indptr), shape=(n, n)))
    return Graph(mats)


def uniform(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def plans_of(graph):
    return [graph.plan(**kn) for kn in KNOBS]


def same_bits(a, b):
    """torch.equal that also tells NaN payload-free NaNs and the sign of zero apart (the calls promise BITS)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. SDDMM
def sddmm_per_head(plan, g, x, heads, hops=None):
    w = x.shape[1] // heads
    per = [plan.sddmm(g[:, :, h * w:(h + 1) * w], x[:, h * w:(h + 1) * w], hops=hops) for h in range(heads)]
    return [torch.stack([p[s] for p in per], dim=1) for s in range(len(per[0]))]


@pytest.mark.parametrize("w", (4, 8, 12, 16, 20, 32, 48, 64, 68, 128, 260))
def test_sddmm_heads_has_the_bits_of_the_per_head_calls(w, crafted, cora):
    case = 0
    for heads in (1, 2, 3, 5, 8, 16):
        d = w * heads
        if d > 520:
            continue
        for graph, plan in [(crafted, p) for p in plans_of(crafted)][case % 3:case % 3 + 1] + ([(cora, cora.plan())] if heads in (2, 8) else []):
            g, x = uniform((graph.n, 2, d), 100 + d), uniform((graph.n, d), 200 + d)
            got = plan.sddmm_heads(g, x, heads)
            assert [tuple(t.shape) for t in got] == [(n, heads) for n in graph.nnz] and all(t.is_contiguous() for t in got)
            want = sddmm_per_head(plan, g, x, heads)
            assert all(same_bits(a, b) for a, b in zip(got, want)), (w, heads)
        case += 1


@pytest.mark.parametrize("w,heads", [(16, 8), (4, 3), (20, 2), (64, 2), (68, 3)])
def test_sddmm_heads_strides_hop_subsets_and_out(w, heads, crafted):
    d, n = w * heads, crafted.n
    plan = crafted.plan(**KNOBS[(w + heads) % 3])
    gbuf, xbuf = uniform((n, 3, d + 9), 31), uniform((n, d + 5), 32)
    g, x = gbuf[:, 1:, 3:3 + d], xbuf[:, 1:1 + d]                              # a slot of a wider buffer; a strided x
    want = sddmm_per_head(plan, g.contiguous(), x.contiguous(), heads)
    assert all(same_bits(a, b) for a, b in zip(plan.sddmm_heads(g, x, heads), want))
    for hop in (0, 1):
        one = plan.sddmm_heads(g[:, hop:hop + 1], x, heads, hops=[hop])
        assert len(one) == 1 and same_bits(one[0], want[hop])
    out = [torch.full((m, heads), 7.0, device=DEV) for m in crafted.nnz]
    assert plan.sddmm_heads(g, x, heads, out=out)[0] is out[0] and all(same_bits(a, b) for a, b in zip(out, want))


def test_sddmm_heads_on_a_row_selected_sub_plan(crafted):
    plan = crafted.plan(**KNOBS[0])
    rows = torch.arange(3, crafted.n, 7, device=DEV)
    sub = plan.select_rows(rows).plan
    assert sub.n_rows == rows.numel() != sub.n_cols
    for w, heads in ((16, 4), (12, 3)):
        g, x = uniform((sub.n_rows, 2, w * heads), 41), uniform((sub.n_cols, w * heads), 42)
        assert all(same_bits(a, b) for a, b in zip(sub.sddmm_heads(g, x, heads), sddmm_per_head(sub, g, x, heads)))


@pytest.mark.parametrize("w,heads", [(4, 16), (16, 8), (32, 5), (48, 3), (260, 2)])
def test_sddmm_heads_accuracy_against_fp64(w, heads, crafted):
    """|dv - dv64| <= gamma_w * sum_c |g_c x_c| + w * 2^-149, no factor."""
    d = w * heads
    plan = crafted.plan(**KNOBS[1])
    g, x = uniform((crafted.n, 2, d), 51), uniform((crafted.n, d), 52)
    got = plan.sddmm_heads(g, x, heads)
    gamma = w * U / (1 - w * U)
    for s in range(2):
        prod = (g[crafted.rows[s], s].double() * x[crafted.cols[s]].double()).view(-1, heads, w)
        err = (got[s].double() - prod.sum(dim=2)).abs()
        bound = gamma * prod.abs().sum(dim=2) + w * 2.0 ** -149
        print(f"w {w} K {heads} hop {s}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# ------------------------------------------------------------------ 2. row softmax
def columns(tensors, h):
    return [t[:, h].contiguous() for t in tensors]


@pytest.mark.parametrize("heads", (1, 2, 3, 8, 16))
def test_row_softmax_heads_has_the_bits_of_the_per_head_calls(heads, crafted, cora):
    for i, (graph, plan) in enumerate([(crafted, p) for p in plans_of(crafted)] + [(cora, cora.plan())]):
        scores = [uniform((n, heads), 60 + s + i) * 6 for s, n in enumerate(graph.nnz)]
        grads = [uniform((n, heads), 70 + s + i) for s, n in enumerate(graph.nnz)]
        alpha = plan.row_softmax_heads(scores)
        dscores = plan.row_softmax_heads_backward(alpha, grads)
        assert [tuple(t.shape) for t in alpha] == [(n, heads) for n in graph.nnz]
        for h in range(heads):
            a_h = plan.row_softmax(columns(scores, h))
            d_h = plan.row_softmax_backward(a_h, columns(grads, h))
            assert all(same_bits(a[:, h], b) for a, b in zip(alpha, a_h)), (heads, h)
            assert all(same_bits(a[:, h], b) for a, b in zip(dscores, d_h)), (heads, h)
        # in place: alpha over the scores, dscores over the incoming gradient
        s2, g2 = [t.clone() for t in scores], [t.clone() for t in grads]
        assert plan.row_softmax_heads(s2, out=s2)[0] is s2[0] and all(same_bits(a, b) for a, b in zip(s2, alpha))
        plan.row_softmax_heads_backward(alpha, g2, out=g2)
        assert all(same_bits(a, b) for a, b in zip(g2, dscores))
        one = plan.row_softmax_heads(scores[1:], hops=[1])
        assert len(one) == 1 and same_bits(one[0], alpha[1])


# ------------------------------------------------------------------ 3. edge scores
def edge_per_head(plan, l, r, grads, heads, **kw):
    out = [plan.edge_scores_backward(l[:, :, h], r[:, :, h], columns(grads, h), **kw) for h in range(heads)]
    return tuple(None if out[0][side] is None else torch.stack([o[side] for o in out], dim=2) for side in (0, 1))


@pytest.mark.parametrize("heads", (1, 2, 3, 8, 16))
def test_edge_scores_heads_have_the_bits_of_the_per_head_calls(heads, crafted, cora):
    configs = [(crafted, p) for p in plans_of(crafted)] + [(cora, cora.plan()), (crafted, crafted.plan(symmetric_pattern=True, **KNOBS[0]))]
    for i, (graph, plan) in enumerate(configs):
        lbuf, r = uniform((graph.n, 2 * heads + 3), 80 + i), uniform((graph.n, 2, heads), 81 + i)
        l = lbuf[:, 1:1 + 2 * heads].view(graph.n, 2, heads)                     # a row stride passes through
        grads = [uniform((n, heads), 82 + s + i) for s, n in enumerate(graph.nnz)]
        scores = plan.edge_scores_heads(l, r, 0.2)
        assert [tuple(t.shape) for t in scores] == [(n, heads) for n in graph.nnz]
        for h in range(heads):
            assert all(same_bits(a[:, h], b) for a, b in zip(scores, plan.edge_scores(l[:, :, h], r[:, :, h], 0.2))), (heads, h)
        dl, dr = plan.edge_scores_heads_backward(l, r, grads, 0.2)
        want_dl, want_dr = edge_per_head(plan, l, r, grads, heads, negative_slope=0.2)
        assert same_bits(dl, want_dl) and same_bits(dr, want_dr), heads
        only_l = plan.edge_scores_heads_backward(l, r, grads, 0.2, need_dr=False)
        only_r = plan.edge_scores_heads_backward(l, r, grads, 0.2, need_dl=False)
        assert only_l[1] is None and only_r[0] is None and same_bits(only_l[0], dl) and same_bits(only_r[1], dr)
        one = plan.edge_scores_heads_backward(l[:, 1:], r[:, 1:], grads[1:], 0.2, hops=[1])
        assert same_bits(one[0], dl[:, 1:]) and same_bits(one[1], dr[:, 1:])


def test_edge_scores_heads_column_side_refusals(crafted):
    from h2gcn_amd import HopPlan, _capi

    heads, n = 4, crafted.n
    plan = crafted.plan(**KNOBS[0])
    no_t = HopPlan.from_scipy(crafted.mats, DEV)
    no_perm = HopPlan.from_scipy(crafted.mats, DEV, build_transpose=True)
    l, r = uniform((n, 2, heads), 90), uniform((n, 2, heads), 91)
    grads = [uniform((m, heads), 92) for m in crafted.nnz]
    for bad in (no_t, no_perm):
        with pytest.raises(ValueError, match="keep_permutation=True"):
            bad.edge_scores_heads_backward(l, r, grads)
        assert same_bits(bad.edge_scores_heads_backward(l, r, grads, need_dr=False)[0], plan.edge_scores_heads_backward(l, r, grads)[0])
    # the C ABI's own two refusals, before the device is touched and before the row side runs
    L = _capi.lib()
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in grads])
    dl, dr = torch.full((n, 2, heads), 7.0, device=DEV), torch.full((n, 2, heads), 7.0, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (0, C.c_void_p(l.data_ptr()), 2 * heads, C.c_void_p(r.data_ptr()), 2 * heads, heads, 0.2, ptrs,
            C.c_void_p(dl.data_ptr()), 2 * heads, C.c_void_p(dr.data_ptr()), 2 * heads)
    fn = L.h2gcn_edge_scores_backward_hops_heads_f32
    assert fn(no_t._handle, *args, stream) == _capi.ERR_NO_TRANSPOSE and b"H2GCN_PLAN_BUILD_TRANSPOSE" in L.h2gcn_last_error()
    assert fn(no_perm._handle, *args, stream) == _capi.ERR_INVALID_ARGUMENT and b"H2GCN_PLAN_KEEP_PERMUTATION" in L.h2gcn_last_error()
    short = args[:9] + (2 * heads - 1,) + args[10:]
    assert fn(plan._handle, *short, stream) == _capi.ERR_INVALID_ARGUMENT and b"lddl" in L.h2gcn_last_error()
    assert L.h2gcn_sddmm_hops_heads_f32(plan._handle, 0, None, 24, 24, None, 24, 24, 4, ptrs, stream) == _capi.ERR_INVALID_ARGUMENT
    assert b"multiple of 4" in L.h2gcn_last_error()
    assert L.h2gcn_row_softmax_hops_heads_f32(plan._handle, 0, ptrs, ptrs, 0, stream) == _capi.ERR_INVALID_ARGUMENT
    assert b"n_heads" in L.h2gcn_last_error()
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()) and bool((dr == 7.0).all())


# ------------------------------------------------------------------ 4. non-finite values stay in their head
SPECIALS = (float("nan"), float("inf"), float("-inf"))


def test_non_finite_values_stay_inside_their_head(crafted):
    heads, w, n, bad = 4, 8, crafted.n, 2
    plan = crafted.plan(**KNOBS[1])
    d = heads * w
    keep = [h for h in range(heads) if h != bad]
    tiny = torch.tensor([1e-40, -1e-42, -0.0, 0.0], device=DEV)

    def seeded(t, seed):                                                       # subnormals and signed zeros everywhere
        idx = torch.randint(0, t.numel(), (t.numel() // 7,), generator=torch.Generator().manual_seed(seed)).to(DEV)
        t.view(-1)[idx] = tiny[idx % 4]
        return t

    g, x = seeded(uniform((n, 2, d), 1), 2), seeded(uniform((n, d), 3), 4)
    l, r = seeded(uniform((n, 2, heads), 5), 6), seeded(uniform((n, 2, heads), 7), 8)
    scores = [seeded(uniform((m, heads), 9 + s) * 4, 11 + s) for s, m in enumerate(crafted.nnz)]
    grads = [seeded(uniform((m, heads), 13 + s), 15 + s) for s, m in enumerate(crafted.nnz)]
    clean_dv = plan.sddmm_heads(g, x, heads)
    clean_alpha = plan.row_softmax_heads(scores)
    clean_ds = plan.row_softmax_heads_backward(clean_alpha, grads)
    clean_sc = plan.edge_scores_heads(l, r)
    clean_dl, clean_dr = plan.edge_scores_heads_backward(l, r, grads)
    # the clean run itself has the per-head bits (subnormals, -0)
    assert all(same_bits(a, b) for a, b in zip(clean_dv, sddmm_per_head(plan, g, x, heads)))
    for v in SPECIALS:
        degree = [torch.bincount(rows, minlength=n) for rows in crafted.rows]
        node = int(torch.minimum(*degree).argmax())                               # a node with neighbours in both hops
        x2 = x.clone()
        x2[node, bad * w + 3] = v
        dv = plan.sddmm_heads(g, x2, heads)
        for s in range(2):
            assert same_bits(dv[s][:, keep], clean_dv[s][:, keep])
            touched = crafted.cols[s] == node
            assert same_bits(dv[s][~touched], clean_dv[s][~touched]) and not bool(torch.isfinite(dv[s][touched, bad]).all())
        sc2 = [t.clone() for t in scores]
        for s in range(2):
            sc2[s][crafted.nnz[s] // 2, bad] = v
        alpha = plan.row_softmax_heads(sc2)
        ds = plan.row_softmax_heads_backward(alpha, grads)
        for s in range(2):
            hit = crafted.rows[s] == crafted.rows[s][crafted.nnz[s] // 2]          # the one segment
            assert same_bits(alpha[s][:, keep], clean_alpha[s][:, keep]) and same_bits(ds[s][:, keep], clean_ds[s][:, keep])
            assert same_bits(alpha[s][~hit], clean_alpha[s][~hit]) and same_bits(ds[s][~hit], clean_ds[s][~hit])
            if v != float("-inf"):                                              # (-inf next to finite scores: exactly +0 there)
                assert bool(torch.isnan(alpha[s][hit, bad]).all())
        for name in ("l", "r"):
            l2, r2 = l.clone(), r.clone()
            (l2 if name == "l" else r2)[node, :, bad] = v
            sc = plan.edge_scores_heads(l2, r2)
            dl, dr = plan.edge_scores_heads_backward(l2, r2, grads)
            for s in range(2):
                hit = (crafted.rows[s] if name == "l" else crafted.cols[s]) == node
                assert same_bits(sc[s][:, keep], clean_sc[s][:, keep]) and same_bits(sc[s][~hit], clean_sc[s][~hit])
            assert same_bits(dl[:, :, keep], clean_dl[:, :, keep]) and same_bits(dr[:, :, keep], clean_dr[:, :, keep])
            want = edge_per_head(plan, l2, r2, grads, heads)
            assert same_bits(dl, want[0]) and same_bits(dr, want[1])


# ------------------------------------------------------------------ 5. empty hop, empty rows, no rows, one head
def test_degenerate_shapes():
    from h2gcn_amd import HopPlan

    n = 40
    dense = (np.random.default_rng(3).random((n, n)) < 0.2).astype(np.float32)
    dense[5:9] = 0
    a = sp.csr_matrix(dense)
    empty = sp.csr_matrix((n, n), dtype=np.float32)
    plan = HopPlan.from_scipy([a, empty], DEV, **TRAIN)
    for heads in (1, 4):
        d = 8 * heads
        g, x = uniform((n, 2, d), 1), uniform((n, d), 2)
        l, r = uniform((n, 2, heads), 3), uniform((n, 2, heads), 4)
        dv = plan.sddmm_heads(g, x, heads)
        assert [tuple(t.shape) for t in dv] == [(a.nnz, heads), (0, heads)]
        assert all(same_bits(p, q) for p, q in zip(dv, sddmm_per_head(plan, g, x, heads)))
        sc = plan.edge_scores_heads(l, r)
        alpha = plan.row_softmax_heads(sc)
        assert tuple(alpha[1].shape) == (0, heads)
        assert same_bits(alpha[0][:, 0], plan.row_softmax([sc[0][:, 0].contiguous(), sc[1][:, 0].contiguous()])[0])
        dl, dr = plan.edge_scores_heads_backward(l, r, alpha)
        assert not bool(dl[5:9].any()) and not bool(torch.signbit(dl[5:9]).any())   # empty rows: +0
        assert not bool(dl[:, 1].any()) and not bool(dr[:, 1].any())               # the empty hop: +0 everywhere
        only = plan.edge_scores_heads_backward(l[:, 1:], r[:, 1:], alpha[1:], hops=[1])
        assert not bool(only[0].any()) and not bool(only[1].any()) and tuple(only[0].shape) == (n, 1, heads)
    none = HopPlan([torch.zeros(1, dtype=torch.int64, device=DEV)], [torch.zeros(0, dtype=torch.int32, device=DEV)],
                   [torch.zeros(0, device=DEV)], n)
    assert none.n_rows == 0
    assert tuple(none.sddmm_heads(torch.zeros(0, 1, 8, device=DEV), uniform((n, 8), 5), 2)[0].shape) == (0, 2)
    assert tuple(none.row_softmax_heads([torch.zeros(0, 2, device=DEV)])[0].shape) == (0, 2)
    assert tuple(none.edge_scores_heads(torch.zeros(0, 1, 2, device=DEV), uniform((n, 1, 2), 6))[0].shape) == (0, 2)
    assert tuple(none.edge_scores_heads_backward(torch.zeros(0, 1, 2, device=DEV), uniform((n, 1, 2), 6),
                                                 [torch.zeros(0, 2, device=DEV)], need_dr=False)[0].shape) == (0, 1, 2)


# ------------------------------------------------------------------ 6. the layer
def per_head_chain(layer, plan, x):
    """MultiHeadHopAttention.forward as it was before the head-batched calls: the public per-head functions."""
    from h2gcn_amd import hop_edge_scores, hop_softmax, hop_spmm_values

    n_heads, w = layer.heads, layer.in_dim // layer.heads
    alpha = []
    for h in range(n_heads):
        x_h = x[:, h * w:(h + 1) * w]
        l, r = x_h @ layer.a_l[:, h, :].t(), x_h @ layer.a_r[:, h, :].t()
        alpha.append(hop_softmax(plan, hop_edge_scores(plan, l, r, layer.negative_slope, layer.hops), layer.hops))
    values = [torch.stack([alpha[h][s] for h in range(n_heads)], dim=0).t() for s in range(layer.a_l.shape[0])]
    return hop_spmm_values(plan, x, values, layer.hops)


@pytest.mark.parametrize("d,heads", [(32, 4), (32, 8), (24, 2)])
def test_layer_has_the_bits_of_the_per_head_chain(d, heads, crafted, cora, monkeypatch):
    from h2gcn_amd import HopPlan, MultiHeadHopAttention

    for graph, plan in ((crafted, crafted.plan(**KNOBS[0])), (cora, cora.plan())):
        x0, rr = uniform((graph.n, d), 21), uniform((graph.n, 2, d), 22)
        torch.manual_seed(23)
        layer = MultiHeadHopAttention(d, heads).to(DEV)
        outs = []
        for chain in (per_head_chain, None):
            layer.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            if chain is None:                                                   # the layer itself must not make a per-head call
                for name in ("sddmm", "row_softmax", "row_softmax_backward", "edge_scores", "edge_scores_backward"):
                    monkeypatch.setattr(HopPlan, name, lambda *a, **k: pytest.fail("a per-head call"))
            y = layer(plan, x) if chain is None else chain(layer, plan, x)
            (y * rr).sum().backward()
            outs.append((y.detach(), x.grad, layer.a_l.grad.clone(), layer.a_r.grad.clone()))
            monkeypatch.undo()
        for name, a, b in zip(("y", "dx", "da_l", "da_r"), *outs):
            assert same_bits(a, b), f"d {d} K {heads}: {name} differs from the per-head chain"
        assert float(outs[1][2].abs().max()) > 0 and float(outs[1][1].abs().max()) > 0


# ------------------------------------------------------------------ 7. the autograd functions against the dense fp64 replica
def _dense_chain(graph, l0, r0, rr, dtype):
    """leaky(l_i + r_j) on the pattern, softmax per row / hop / head, weighted by rr and summed: torch's own autograd."""
    n, _, heads = l0.shape
    l, r = (t.to(dtype).clone().requires_grad_(True) for t in (l0, r0))
    total = torch.zeros((), dtype=dtype, device=DEV)
    for s, (rows, cols) in enumerate(zip(graph.rows, graph.cols)):
        mask = torch.zeros((n, n), dtype=torch.bool, device=DEV).index_put((rows, cols), torch.ones((), dtype=torch.bool, device=DEV))
        for h in range(heads):
            e = torch.nn.functional.leaky_relu(l[:, s, h][:, None] + r[:, s, h][None, :], 0.2)
            A = torch.softmax(e.masked_fill(~mask & mask.any(dim=1, keepdim=True), float("-inf")), dim=1)
            total = total + (A[rows, cols] * rr[s][:, h].to(dtype)).sum()
    total.backward()
    return l.grad, r.grad


@pytest.mark.parametrize("which,heads", [("cora", 4), ("crafted", 8)])
def test_autograd_functions_against_the_dense_fp64_replica(which, heads, request):
    """max|g - g64| / max|g64| for dl and dr: at most 4 x the figure of the dense fp32 torch replica (the existing rule)."""
    from h2gcn_amd import hop_edge_scores_heads, hop_softmax_heads

    graph = request.getfixturevalue(which)
    plan = graph.plan()
    l0, r0 = uniform((graph.n, 2, heads), 31), uniform((graph.n, 2, heads), 32)
    rr = [uniform((m, heads), 33 + s) for s, m in enumerate(graph.nnz)]
    l, r = l0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    alpha = hop_softmax_heads(plan, hop_edge_scores_heads(plan, l, r, 0.2))
    sum((a * w).sum() for a, w in zip(alpha, rr)).backward()
    g64, g32 = _dense_chain(graph, l0, r0, rr, torch.float64), _dense_chain(graph, l0, r0, rr, torch.float32)
    for name, g, r64, r32 in zip(("l", "r"), (l.grad, r.grad), g64, g32):
        scale = float(r64.abs().max())
        ours, theirs = float((g.double() - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
        print(f"{which} K {heads} d{name}: max|g - g64| / max|g64| = {ours:.3e}; dense fp32 replica {theirs:.3e}; ratio {ours / theirs:.2f}")
        assert ours <= 4.0 * theirs, (name, ours, theirs)


# ------------------------------------------------------------------ 8. hipGraph
def test_captured_training_step_replays_to_the_eager_result(crafted):
    from h2gcn_amd import MultiHeadHopAttention

    d = 32
    x, rr = uniform((crafted.n, d), 41), uniform((crafted.n, 2, d), 42)
    plan = crafted.plan(**KNOBS[0])
    torch.manual_seed(43)
    net = MultiHeadHopAttention(d, 8).to(DEV)
    init = [p.detach().clone() for p in net.parameters()]

    def step():
        for p in net.parameters():
            p.grad = None
        (net(plan, x) * rr).sum().backward()
        with torch.no_grad():
            for p in net.parameters():
                p.sub_(0.05 * p.grad)

    def reset():
        with torch.no_grad():
            for p, q in zip(net.parameters(), init):
                p.copy_(q)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                    # the eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    reset()
    step()
    eager = [p.detach().clone() for p in net.parameters()]
    reset()
    for p in net.parameters():
        p.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    reset()                                                                       # (capture runs nothing)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), q) for p, q in zip(net.parameters(), eager))
    assert all(not torch.equal(p, q) for p, q in zip(eager, init))
