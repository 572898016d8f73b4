"""GPU suite: attention training without per-entry arrays -- the forward that stores the softmax statistics
(HopPlan.attention_heads_stats, h2gcn_amd/csrc/attention_stats.hip), the recomputing backward (HopPlan.attention_heads_backward,
h2gcn_amd/csrc/attention_backward.hip), hop_attention_recompute and RecomputeMultiHeadHopAttention.

The forward's contract is the bits of HopPlan.attention_heads and exact statistics; the gradients are judged against a dense fp64
replica with a bound the NEW path does not set: 4 x the larger error of the chain (unchanged code) and of a dense fp32 replica on
the same operands.  Outputs of the raw launches are guarded views in NaN-filled buffers, every launch is made twice.  The operands
with prescribed segment lengths are those of test_spmm_values_gpu / test_attention_fused_gpu."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import spmm_driver as drv
import test_attention_heads_gpu as heads_gpu
import test_spmm_values_gpu as values_gpu
from test_attention_fused_gpu import SPECIALS, dev, node_terms
from test_spmm_values_gpu import DEV, N_BIG, N_SMALL, THRESHOLDS, bits, launch, make_plan, strided_rows

pytestmark = pytest.mark.gpu
G = drv.GUARD


# ------------------------------------------------------------------ raw launches on guarded buffers
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guards_untouched(buf, width, where):
    assert bool(torch.isnan(buf[..., :G]).all()) and bool(torch.isnan(buf[..., G + width:]).all()), f"{where}: a guard word was written"


def raw_stats(plan, x, l, r, slope=0.2, hops=None):
    """h2gcn_attention_hops_heads_stats_f32 with Y AND stats as guarded views (ldy_row / ldy_hop / ldstats wider than needed), twice
    -> (y, stats [n_rows, H_sel, 2, K])."""
    from h2gcn_amd import _capi

    h_sel, n, d, k = plan.n_selected(hops), plan.n_rows, x.shape[1], l.shape[2]
    outs = []
    for _ in range(2):
        ybuf, y = drv._guarded((n, h_sel, d), torch.float32, DEV)
        sbuf, s = drv._guarded((n, h_sel * 2 * k), torch.float32, DEV)
        st = _capi.lib().h2gcn_attention_hops_heads_stats_f32(
            plan._handle, plan._mask(hops), _ptr(l), l.stride(0), _ptr(r), r.stride(0), k, slope, _ptr(x), x.stride(0), d, _ptr(y), y.stride(0),
            y.stride(1), _ptr(s), s.stride(0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        _guards_untouched(ybuf, d, "Y")
        _guards_untouched(sbuf, h_sel * 2 * k, "stats")
        outs.append((y, s.reshape(n, h_sel, 2, k)))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), "the second call differs"
    return outs[0]


def raw_backward(plan, x, l, r, stats, y, g, slope=0.2, hops=None, needs=(True, True, True)):
    """h2gcn_attention_hops_heads_backward_f32 with delta, dl, dr, dX as guarded views, twice -> (dl, dr, dx), None where unwanted."""
    from h2gcn_amd import _capi

    h_sel, d, k = plan.n_selected(hops), x.shape[1], l.shape[2]
    stats, y, g = stats.contiguous(), y.contiguous(), g.contiguous()
    shapes = ((plan.n_rows, h_sel * k), (plan.n_rows, h_sel * k), (plan.n_cols, h_sel * k), (plan.n_cols, d))
    runs = []
    for _ in range(2):
        pairs = [drv._guarded(sh, torch.float32, DEV) if want else (None, None) for sh, want in zip(shapes, (True,) + tuple(needs))]
        views = [v for _, v in pairs]
        args = []
        for v, sh in zip(views, shapes):
            args += [_ptr(v), sh[1] + 2 * G]
        st = _capi.lib().h2gcn_attention_hops_heads_backward_f32(
            plan._handle, plan._mask(hops), _ptr(l), l.stride(0), _ptr(r), r.stride(0), k, slope, _ptr(x), x.stride(0), d, _ptr(stats),
            h_sel * 2 * k, _ptr(y), h_sel * d, d, _ptr(g), h_sel * d, d, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        for (buf, _), sh, name in zip(pairs, shapes, ("delta", "dl", "dr", "dX")):
            if buf is not None:
                _guards_untouched(buf, sh[1], name)
        runs.append(views[1:])
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), "the second backward launch differs from the first"
    dl, dr, dx = runs[0]
    return (None if dl is None else dl.reshape(plan.n_rows, h_sel, k), None if dr is None else dr.reshape(plan.n_cols, h_sel, k), dx)


# ------------------------------------------------------------------ 1 + 2. forward bits and exact statistics
def check_stats(hops, plan, l, r, stats, slope, where):
    """stats[..., 0, :] = the segment maximum of the chain's scores; stats[..., 1, :] = the chain's coefficient at an entry that
    attains it (there e = exp2(0) = 1, so alpha = 1/S), bit for bit; (+0, +0) for an empty segment."""
    with torch.no_grad():
        scores = plan.edge_scores_heads(l, r, slope)
        alpha = plan.row_softmax_heads(scores)
    st = stats.cpu().numpy()
    n_empty = 0
    for s, m in enumerate(hops):
        sc, al = scores[s].cpu().numpy(), alpha[s].cpu().numpy()
        for i in range(m.shape[0]):
            lo, hi = m.indptr[i], m.indptr[i + 1]
            if lo == hi:
                assert not st[i, s].view(np.int32).any(), f"{where}: an empty segment does not hold (+0, +0)"
                n_empty += 1
                continue
            top = sc[lo:hi].max(axis=0)
            assert np.array_equal(st[i, s, 0], top), f"{where}: row {i} hop {s}: m is not the maximum score"
            at = sc[lo:hi].argmax(axis=0)
            want = al[lo + at, np.arange(sc.shape[1])]
            assert np.array_equal(st[i, s, 1].view(np.int32), want.view(np.int32)), f"{where}: row {i} hop {s}: 1/S differs"
    assert n_empty > 0


@pytest.mark.parametrize("rpw", (1, 3, 7))
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_forward_bits_and_exact_statistics(thr, rpw):
    hops = values_gpu.forward_hops()
    plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
    for d, n_heads in ((128, 8), (20, 1), (48, 3)):
        where = f"thr {thr} rpw {rpw} d {d} K {n_heads}"
        slope = 0.2 if n_heads > 1 else 0.01
        l, r = (dev(t) for t in node_terms(N_SMALL, N_BIG, 2, n_heads, seed=thr + rpw))
        x = dev(values_gpu.operands(d)[0])
        y, stats = raw_stats(plan, x, l, r, slope)
        with torch.no_grad():
            want = plan.attention_heads(x, l, r, slope)
        assert torch.equal(bits(y), bits(want)), where + ": Y differs from the plain fused forward"
        check_stats(hops, plan, l, r, stats, slope, where)
        y2, stats2 = plan.attention_heads_stats(x, l, r, slope)
        assert torch.equal(bits(y2), bits(want)) and torch.equal(bits(stats2), bits(stats)), where + " (the method)"


def test_forward_on_strided_operands_eight_hops_and_a_guarded_out():
    d, n_heads = 64, 2
    hops = values_gpu.forward_hops(8)
    plan = make_plan(hops, long_row_threshold=256, rows_per_wave=7)
    x = np.random.default_rng(8).uniform(-1, 1, (N_BIG, d)).astype(np.float32)
    l, r = node_terms(N_SMALL, N_BIG, 8, n_heads, seed=8)
    xt, lt, rt = strided_rows(x), strided_rows(l), strided_rows(r)
    assert xt.stride(0) == d + 4 and lt.stride(0) == 8 * n_heads + 4
    with torch.no_grad():
        want = plan.attention_heads(xt, lt, rt)
    y, stats = raw_stats(plan, xt, lt, rt)
    assert torch.equal(bits(y), bits(want))
    check_stats(hops, plan, lt, rt, stats, 0.2, "8 hops, strided")
    got = launch(lambda out: plan.attention_heads_stats(xt, lt, rt, out=out)[0], (N_SMALL, 8, d), "out= of the method")
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ 3. gradients against fp64
def dense_grads(hops, x, l, r, gy, slope, dtype):
    """Masked softmax attention on dense [n_rows, n_cols, K] arrays, torch autograd on the CPU -> (dl, dr, dx) as float64 numpy."""
    X, L, R = (torch.from_numpy(np.asarray(t)).to(dtype).requires_grad_(True) for t in (x, l, r))
    gy = torch.from_numpy(np.asarray(gy)).to(dtype)
    n_rows, n_cols, k = L.shape[0], R.shape[0], L.shape[2]
    ys = []
    for s, m in enumerate(hops):
        mask = torch.zeros((n_rows, n_cols), dtype=torch.bool)
        coo = m.tocoo()
        mask[torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))] = True
        sc = torch.nn.functional.leaky_relu(L[:, None, s, :] + R[None, :, s, :], slope)
        sc = sc.masked_fill(~mask[:, :, None], float("-inf"))
        sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))      # (an empty row: no NaN on the way back)
        alpha = torch.softmax(sc, dim=1) * mask[:, :, None].to(dtype)
        ys.append(torch.einsum("ijh,jhw->ihw", alpha, X.view(n_cols, k, -1)).reshape(n_rows, -1))
    (torch.stack(ys, dim=1) * gy).sum().backward()
    return tuple(t.grad.double().numpy() for t in (L, R, X))


def rel_err(got, want64):
    return float(np.abs(got.detach().double().cpu().numpy() - want64).max() / np.abs(want64).max())


@functools.lru_cache(maxsize=None)
def gradient_case(kind, d, n_heads):
    """Operands, the fp64 gradients and the bound of condition 3 -- 4 x max(err of the chain, err of a dense fp32 replica) per
    gradient -- for the 600-node square graph or the rectangular forward_hops plan."""
    from h2gcn_amd import hop_attention_heads

    hops = values_gpu.square_hops() if kind == "square" else values_gpu.forward_hops()
    n_rows, n_cols = hops[0].shape
    rng = np.random.default_rng(100 + d + n_heads)
    x = rng.uniform(-1, 1, (n_cols, d)).astype(np.float32)
    gy = rng.uniform(-1, 1, (n_rows, 2, d)).astype(np.float32)
    l, r = node_terms(n_rows, n_cols, 2, n_heads, seed=d + n_heads)
    want = dense_grads(hops, x, l, r, gy, 0.2, torch.float64)
    dense32 = dense_grads(hops, x, l, r, gy, 0.2, torch.float32)
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    a, b, c = (dev(t).requires_grad_(True) for t in (x, l, r))
    (hop_attention_heads(plan, a, b, c, 0.2) * dev(gy)).sum().backward()                # the chain: unchanged code
    chain = (b.grad, c.grad, a.grad)
    bound = tuple(4 * max(rel_err(g, w), float(np.abs(g32 - w).max() / np.abs(w).max())) for g, g32, w in zip(chain, dense32, want))
    return hops, plan, dev(x), dev(l), dev(r), dev(gy), want, bound, tuple(rel_err(g, w) for g, w in zip(chain, want))


CASES = [("square", d, k) for k in (1, 4, 8) for d in (32, 128)] + [("rect", 128, 8)]


@pytest.mark.parametrize("kind,d,n_heads", CASES)
def test_gradients_against_fp64(kind, d, n_heads):
    hops, plan, x, l, r, gy, want, bound, chain_err = gradient_case(kind, d, n_heads)
    y, stats = plan.attention_heads_stats(x, l, r, 0.2)
    grads = raw_backward(plan, x, l, r, stats, y, gy)
    for name, g, w, b, ce in zip(("dl", "dr", "dx"), grads, want, bound, chain_err):
        err = rel_err(g, w)
        print(f"{kind} d {d} K {n_heads} {name}: err {err:.3e}  chain {ce:.3e}  bound {b:.3e}  ratio to the chain {err / ce:.2f}")
        assert err <= b, f"{name}: relative error {err:.3e} beyond 4 x max(chain, dense fp32) = {b:.3e}"
    for g, h in zip(grads, plan.attention_heads_backward(x, l, r, stats, y, gy)):
        assert torch.equal(bits(g), bits(h)), "the method differs from the raw launch"


# ------------------------------------------------------------------ 4. determinism and selection
def test_determinism_need_flags_and_hop_selection():
    hops, plan, x, l, r, gy, want, bound, _ = gradient_case("square", 32, 8)
    y, stats = plan.attention_heads_stats(x, l, r)
    full = raw_backward(plan, x, l, r, stats, y, gy)                                    # (launched twice: equal bits)
    for needs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = raw_backward(plan, x, l, r, stats, y, gy, needs=tuple(bool(v) for v in needs))
        via = plan.attention_heads_backward(x, l, r, stats, y, gy, need_dl=bool(needs[0]), need_dr=bool(needs[1]), need_dx=bool(needs[2]))
        for want_it, a, b, f in zip(needs, got, via, full):
            if want_it:
                assert torch.equal(bits(a), bits(f)) and torch.equal(bits(b), bits(f)), needs
            else:
                assert a is None and b is None, needs
    dx_sum = 0
    for k in range(2):
        sl = slice(k, k + 1)
        ya, sa = plan.attention_heads_stats(x, l[:, sl], r[:, sl], hops=[k])
        assert torch.equal(bits(ya), bits(y[:, sl])) and torch.equal(bits(sa), bits(stats[:, sl]))
        dl, dr, dx = raw_backward(plan, x, l[:, sl], r[:, sl], sa, ya, gy[:, sl], hops=[k])
        assert torch.equal(bits(dl), bits(full[0][:, sl])), f"dl of hop {k} alone differs from its slot"
        assert torch.equal(bits(dr), bits(full[1][:, sl])), f"dr of hop {k} alone differs from its slot"
        dx_sum = dx_sum + dx.double()
    assert rel_err(dx_sum, want[2]) <= bound[2]


# ------------------------------------------------------------------ 5. plan kinds
def test_plan_kinds_and_thresholds_give_the_same_bits():
    hops, plain, x, l, r, gy, _, _, _ = gradient_case("square", 32, 8)
    y, stats = plain.attention_heads_stats(x, l, r)
    full = raw_backward(plain, x, l, r, stats, y, gy)
    noperm = make_plan(hops, build_transpose=True, keep_permutation=False, long_row_threshold=256)
    assert noperm.has_transpose and not noperm.keep_permutation
    sym = make_plan(hops, build_transpose=True, keep_permutation=True, symmetric_pattern=True, long_row_threshold=256)
    assert sym.transpose_sharing[0] != "none"
    others = [("no permutation", noperm), ("symmetric", sym)]
    others += [(f"thr {thr} rpw {rpw}", values_gpu.adjoint_plan(hops, long_row_threshold=thr, rows_per_wave=rpw))
               for thr, rpw in zip(THRESHOLDS, (1, 3, 7))]
    for name, plan in others:
        # the statistics have no order; Y has the forward's tree, which follows the plan's long list: the backward is a function of
        # its operands, so every plan gets the SAME y
        assert torch.equal(bits(plan.attention_heads_stats(x, l, r)[1]), bits(stats)), name
        for g, f in zip(raw_backward(plan, x, l, r, stats, y, gy), full):
            assert torch.equal(bits(g), bits(f)), f"{name}: the bits differ from the plain plan's"
    bare = make_plan(hops, build_transpose=False, long_row_threshold=256)
    assert not bare.has_transpose
    dl, dr, dx = bare.attention_heads_backward(x, l, r, stats, y, gy, need_dr=False, need_dx=False)
    assert dr is None and dx is None and torch.equal(bits(dl), bits(full[0]))
    for needs in (dict(need_dl=False, need_dx=False), dict(need_dl=False, need_dr=False), dict()):
        with pytest.raises(ValueError, match=r"Build the plan with HopPlan\(\.\.\., build_transpose=True\)"):
            bare.attention_heads_backward(x, l, r, stats, y, gy, **needs)
    from h2gcn_amd import _capi
    with pytest.raises(_capi.H2GCNError, match="H2GCN_PLAN_BUILD_TRANSPOSE"):
        raw_backward(bare, x, l, r, stats, y, gy, needs=(False, True, False))           # (the library's own refusal)


def test_the_rectangular_plan_over_every_threshold():
    hops, plain, x, l, r, gy, _, _, _ = gradient_case("rect", 128, 8)
    y, stats = plain.attention_heads_stats(x, l, r)
    full = raw_backward(plain, x, l, r, stats, y, gy)
    for thr, rpw in ((32, 1), (1024, 7)):
        plan = make_plan(hops, build_transpose=True, long_row_threshold=thr, rows_per_wave=rpw)
        assert torch.equal(bits(plan.attention_heads_stats(x, l, r)[1]), bits(stats))
        for g, f in zip(raw_backward(plan, x, l, r, stats, y, gy), full):                # (the same operands, y included)
            assert torch.equal(bits(g), bits(f)), f"thr {thr} rpw {rpw}"


# ------------------------------------------------------------------ 6. non-finite inputs
def test_a_planted_value_reaches_only_the_sums_that_touch_it():
    d, n_heads = 32, 8
    w = d // n_heads
    hops, plan, x0, l0, r0, gy, _, _, _ = gradient_case("square", d, n_heads)
    n = hops[0].shape[0]
    x, l, r = x0.clone(), l0.clone(), r0.clone()
    lbad, rbad = (torch.zeros((n, 2, n_heads), dtype=torch.bool) for _ in range(2))
    xbad = torch.zeros((n, n_heads), dtype=torch.bool)                                  # (a planted column of x, by head)
    # NaN, +-inf, a subnormal, -0 and 1e30, one element each, in six different heads: heads 6 and 7 stay clean
    l[17, 0, 0], l[301, 1, 1] = SPECIALS[0], SPECIALS[1]
    r[44, 0, 2], r[512, 1, 3] = SPECIALS[2], SPECIALS[3]
    x[99, 4 * w + 1], x[400, 5 * w + 2] = SPECIALS[4], SPECIALS[5]
    lbad[17, 0, 0] = lbad[301, 1, 1] = rbad[44, 0, 2] = rbad[512, 1, 3] = xbad[99, 4] = xbad[400, 5] = True
    # a segment (i, s, h) is touched if its l is planted or a column it holds has a planted r or x; dl is that, dr / dx are touched
    # if any segment of their column is (delta, m, 1/S and y of a touched segment are all suspect)
    row_t, col_t = [], []
    for s, m in enumerate(hops):
        pat = torch.zeros((n, n))
        coo = m.tocoo()
        pat[torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))] = 1.0     # (the stored pattern)
        rt = lbad[:, s] | ((pat @ (rbad[:, s] | xbad).float()) > 0)
        row_t.append(rt)
        col_t.append((pat.t() @ rt.float()) > 0)
    dl_t, dr_t = torch.stack(row_t, dim=1), torch.stack(col_t, dim=1)
    dx_t = (col_t[0] | col_t[1]).repeat_interleave(w, dim=1)
    yc, sc = plan.attention_heads_stats(x0, l0, r0)
    clean = raw_backward(plan, x0, l0, r0, sc, yc, gy)
    yd, sd = raw_stats(plan, x, l, r)
    dirty = raw_backward(plan, x, l, r, sd, yd, gy)                                     # (no guard word is written: raw_backward asserts)
    for name, c, g, t in zip(("dl", "dr", "dx"), clean, dirty, (dl_t, dr_t, dx_t)):
        keep = ~t
        frac = float(keep.float().mean())
        print(f"{name}: {100 * frac:.1f} % of the elements touch no planted value")
        assert frac >= 0.2, f"{name}: the comparison would be vacuous"
        assert torch.equal(bits(g)[keep], bits(c)[keep]), f"{name}: a planted value changed an element whose sums do not touch it"
    assert bool(torch.isnan(dirty[0]).any())


# ------------------------------------------------------------------ 7. no per-entry allocation
def test_a_training_step_allocates_no_per_entry_array():
    from h2gcn_amd import hop_attention_recompute

    d, n_heads = 32, 8
    hops, plan, x, l, r, gy, _, _, _ = gradient_case("square", d, n_heads)
    n = hops[0].shape[0]
    sizes = {"y": n * 2 * d, "stats": n * 2 * 2 * n_heads, "delta": n * 2 * n_heads, "dl": n * 2 * n_heads, "dr": n * 2 * n_heads, "dx": n * d}
    bound = sum(4 * v + 512 for v in sizes.values())
    assert bound < 4 * n_heads * hops[0].nnz, "a single [nnz_0, K] array must break the bound"
    a, b, c = (t.clone().requires_grad_(True) for t in (x, l, r))

    def step():
        return torch.autograd.grad(hop_attention_recompute(plan, a, b, c), (a, b, c), gy)

    step()                                                                          # (whatever the first launches of a selection set up)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    grads = step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"extra device memory of one forward + backward: {extra} B; bound {bound} B; one [nnz_0, K] fp32 array {4 * n_heads * hops[0].nnz} B")
    assert extra <= bound
    assert all(g is not None and float(g.abs().max()) > 0 for g in grads)


# ------------------------------------------------------------------ 8. the layer
@functools.lru_cache(maxsize=None)
def crafted():
    return heads_gpu.Graph(values_gpu.square_hops())


def dense_layer_grads(layer, graph, x, rr, dtype):
    """The gradients of a_l, a_r of sum(layer(x) * rr) through the dense replica on the CPU, as float64 numpy."""
    heads, d = layer.heads, layer.in_dim
    w = d // heads
    a_l, a_r = (p.detach().to(dtype).cpu().requires_grad_(True) for p in (layer.a_l, layer.a_r))
    X = x.to(dtype).cpu()
    L = torch.stack([X[:, h * w:(h + 1) * w] @ a_l[:, h, :].t() for h in range(heads)], dim=2)
    R = torch.stack([X[:, h * w:(h + 1) * w] @ a_r[:, h, :].t() for h in range(heads)], dim=2)
    ys = []
    for s, m in enumerate(graph.mats):
        mask = torch.zeros((graph.n, graph.n), dtype=torch.bool)
        mask[graph.rows[s].cpu(), graph.cols[s].cpu()] = True
        sc = torch.nn.functional.leaky_relu(L[:, None, s, :] + R[None, :, s, :], layer.negative_slope).masked_fill(~mask[:, :, None], float("-inf"))
        sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))
        alpha = torch.softmax(sc, dim=1) * mask[:, :, None].to(dtype)
        ys.append(torch.einsum("ijh,jhw->ihw", alpha, X.view(graph.n, heads, w)).reshape(graph.n, d))
    (torch.stack(ys, dim=1) * rr.to(dtype).cpu()).sum().backward()
    return a_l.grad.double().numpy(), a_r.grad.double().numpy()


@pytest.mark.parametrize("heads", (1, 8))
def test_layer_output_bits_and_parameter_gradients(heads):
    from h2gcn_amd import MultiHeadHopAttention, RecomputeMultiHeadHopAttention

    d = 32
    graph = crafted()
    plan = graph.plan(**heads_gpu.KNOBS[1])
    x, rr = heads_gpu.uniform((graph.n, d), 21), heads_gpu.uniform((graph.n, 2, d), 22)
    torch.manual_seed(23)
    old = MultiHeadHopAttention(d, heads).to(DEV)
    new = RecomputeMultiHeadHopAttention(d, heads).to(DEV)
    new.load_state_dict(old.state_dict())
    outs = []
    for layer in (old, new):
        y = layer(plan, x)
        (y * rr).sum().backward()
        outs.append(y)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "the output differs from the chain layer's"
    want, dense32 = (dense_layer_grads(old, graph, x, rr, dt) for dt in (torch.float64, torch.float32))
    for name, p_old, p_new, w64, w32 in zip(("a_l", "a_r"), (old.a_l, old.a_r), (new.a_l, new.a_r), want, dense32):
        e_old, e_new, e_32 = rel_err(p_old.grad, w64), rel_err(p_new.grad, w64), float(np.abs(w32 - w64).max() / np.abs(w64).max())
        print(f"{heads} heads {name}: err {e_new:.3e}, the chain layer {e_old:.3e}, dense fp32 {e_32:.3e}")
        assert e_new <= 4 * max(e_old, e_32), f"{name}: {e_new:.3e} beyond 4 x max(chain layer {e_old:.3e}, dense fp32 {e_32:.3e})"


def _net(d, heads, seed):
    from h2gcn_amd import GCNLayer, RecomputeMultiHeadHopAttention

    torch.manual_seed(seed)
    a, b, gcn = RecomputeMultiHeadHopAttention(d, heads).to(DEV), RecomputeMultiHeadHopAttention(d, heads).to(DEV), GCNLayer()
    params = list(a.parameters()) + list(b.parameters())

    def forward(plan, x):
        h = a(plan, x)
        return b(plan, torch.tanh(h[:, 0] + h[:, 1])) + gcn(plan, x)                    # two attention layers and a GCNLayer on ONE plan

    return forward, params


def test_two_layers_and_a_gcn_layer_share_a_plan_and_sgd_is_deterministic():
    d = 32
    graph = crafted()
    plan = graph.plan(**heads_gpu.KNOBS[0])
    x, rr = heads_gpu.uniform((graph.n, d), 31), heads_gpu.uniform((graph.n, 2, d), 32)
    vals = [v.clone() for v in plan.vals]
    finals = []
    for _ in range(2):
        forward, params = _net(d, 8, seed=33)
        init = [p.detach().clone() for p in params]
        for _ in range(2):
            for p in params:
                p.grad = None
            (forward(plan, x) * rr).sum().backward()
            with torch.no_grad():
                for p in params:
                    p.sub_(0.05 * p.grad)
        assert all(not torch.equal(p.detach(), q) for p, q in zip(params, init))
        finals.append([p.detach().clone() for p in params])
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(*finals)), "two runs of two SGD steps differ"
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plan.vals, vals)), "the plan's values changed"


def test_captured_training_step_replays_to_the_eager_result():
    d = 32
    graph = crafted()
    plan = graph.plan(**heads_gpu.KNOBS[0])
    x, rr = heads_gpu.uniform((graph.n, d), 41), heads_gpu.uniform((graph.n, 2, d), 42)
    forward, params = _net(d, 8, seed=43)
    init = [p.detach().clone() for p in params]

    def step():
        for p in params:
            p.grad = None
        (forward(plan, x) * rr).sum().backward()
        with torch.no_grad():
            for p in params:
                p.sub_(0.05 * p.grad)

    def reset():
        with torch.no_grad():
            for p, q in zip(params, init):
                p.copy_(q)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                      # the eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    reset()
    step()
    eager = [p.detach().clone() for p in params]
    reset()
    for p in params:
        p.grad = None
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        step()
    reset()                                                                         # (capture runs nothing)
    graph_.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), q) for p, q in zip(params, eager))
    assert all(not torch.equal(p, q) for p, q in zip(eager, init))
