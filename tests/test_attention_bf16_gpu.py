"""GPU suite: bf16 embeddings in the recomputing hop attention (h2gcn_amd/csrc/attention_bf16.hip; HopPlan.attention_heads_bf16,
attention_heads_stats_bf16, attention_heads_backward_bf16; hop_attention_recompute and RecomputeMultiHeadHopAttention on a bfloat16
input).

The contract is the bf16 SpMM's: widen exactly, the fp32 kernel's operations in fp32 in its order, ONE rounding to nearest even at the
store.  So every check but one is a BIT comparison against the existing fp32 launches on the upcast operands, run in the same test:
an fp32 output has their bits, a bf16 output is that value .to(torch.bfloat16).  The raw launches write guarded NaN-filled views and
are made twice.  The operands with prescribed segment lengths are those of test_spmm_values_gpu (48 x 1100, segment lengths 0 ..
1025); the layer tests run on its 600-node square graph."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import spmm_driver as drv
import test_attention_heads_gpu as heads_gpu
import test_spmm_values_gpu as values_gpu
from test_attention_fused_gpu import SPECIALS, dev, node_terms, special_operands
from test_attention_recompute_gpu import crafted
from test_spmm_values_gpu import DEV, N_BIG, N_SMALL, THRESHOLDS, bits, make_plan, strided_rows

pytestmark = pytest.mark.gpu
G = drv.GUARD
BF = torch.bfloat16
KNOBS = tuple(zip(THRESHOLDS, (1, 3, 7)))                         # (long_row_threshold, rows_per_wave)
FORWARD_GRID = [(8, 2), (22, 1), (48, 3), (64, 16), (128, 8), (260, 1), (320, 5)]
BACKWARD_GRID = [(8, 2), (64, 8), (48, 3), (128, 4), (128, 8), (22, 1), (100, 1), (192, 2), (256, 4)]
NEEDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))     # (those of test_attention_recompute_gpu)


def bits_of(t):
    """The bit patterns of a float32 / bfloat16 tensor, on the host."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits_of(a), bits_of(b))


def same_nan_aware(got, want):
    """NaN exactly where `want` has one (payload and sign of a NaN are not compared), every other element bit for bit -- the
    comparison of test_special_values_gpu for bf16 outputs."""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = torch.isnan(got).cpu(), torch.isnan(want).cpu()
    return torch.equal(gn, wn) and torch.equal(bits_of(got)[~gn], bits_of(want)[~wn])


def bf16_operand(a):
    """The host array rounded to bfloat16, on the device."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(BF)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _code(dtype):
    from h2gcn_amd import _capi

    return _capi.DTYPE_BF16 if dtype == BF else _capi.DTYPE_F32


def _guards_untouched(buf, width, where):
    assert bool(torch.isnan(buf[..., :G]).all()) and bool(torch.isnan(buf[..., G + width:]).all()), f"{where}: a guard element was written"


# ------------------------------------------------------------------ raw launches on guarded buffers
def raw_forward(plan, x, l, r, y_dtype, with_stats, slope=0.2, hops=None):
    """h2gcn_attention_hops_heads_bf16 / ..._stats_bf16 with Y (and stats) as guarded views, twice -> (y, stats or None)."""
    from h2gcn_amd import _capi

    h_sel, n, d, k = plan.n_selected(hops), plan.n_rows, x.shape[1], l.shape[2]
    outs = []
    for _ in range(2):
        ybuf, y = drv._guarded((n, h_sel, d), y_dtype, DEV)
        sbuf, s = drv._guarded((n, h_sel * 2 * k), torch.float32, DEV)
        args = (plan._handle, plan._mask(hops), _ptr(l), l.stride(0), _ptr(r), r.stride(0), k, slope, _ptr(x), x.stride(0), d, _code(y_dtype),
                _ptr(y), y.stride(0), y.stride(1))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if with_stats:
            st = _capi.lib().h2gcn_attention_hops_heads_stats_bf16(*args, _ptr(s), s.stride(0), stream)
        else:
            st = _capi.lib().h2gcn_attention_hops_heads_bf16(*args, stream)
        _capi.check(st)
        _guards_untouched(ybuf, d, "Y")
        if with_stats:
            _guards_untouched(sbuf, h_sel * 2 * k, "stats")
        else:
            assert bool(torch.isnan(sbuf).all())
        outs.append((y, s.reshape(n, h_sel, 2, k) if with_stats else None))
    assert same(outs[0][0], outs[1][0]) and (not with_stats or same(outs[0][1], outs[1][1])), "the second call differs from the first"
    return outs[0]


def raw_backward(plan, wide_dtype, x, l, r, stats, y, g, dx_dtype=torch.float32, slope=0.2, hops=None, needs=(True, True, True)):
    """The recomputing backward with delta, dl, dr, dX as guarded views, twice -> (delta, dl, dr, dx), None where unwanted:
    h2gcn_attention_hops_heads_backward_bf16 (wide_dtype bfloat16: x, y, g bf16) or ..._f32 (float32: the reference)."""
    from h2gcn_amd import _capi

    assert x.dtype == y.dtype == g.dtype == wide_dtype
    h_sel, d, k = plan.n_selected(hops), x.shape[1], l.shape[2]
    stats, y, g = stats.contiguous(), y.contiguous(), g.contiguous()
    shapes = ((plan.n_rows, h_sel * k), (plan.n_rows, h_sel * k), (plan.n_cols, h_sel * k), (plan.n_cols, d))
    dtypes = (torch.float32, torch.float32, torch.float32, dx_dtype)
    runs = []
    for _ in range(2):
        pairs = [drv._guarded(sh, dt, DEV) if want else (None, None) for sh, dt, want in zip(shapes, dtypes, (True,) + tuple(needs))]
        views = [v for _, v in pairs]
        args = []
        for i, (v, sh) in enumerate(zip(views, shapes)):
            args += ([_code(dx_dtype)] if i == 3 and wide_dtype == BF else []) + [_ptr(v), sh[1] + 2 * G]
        fn = _capi.lib().h2gcn_attention_hops_heads_backward_bf16 if wide_dtype == BF else _capi.lib().h2gcn_attention_hops_heads_backward_f32
        st = fn(plan._handle, plan._mask(hops), _ptr(l), l.stride(0), _ptr(r), r.stride(0), k, slope, _ptr(x), x.stride(0), d, _ptr(stats),
                h_sel * 2 * k, _ptr(y), h_sel * d, d, _ptr(g), h_sel * d, d, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        for (buf, _), sh, name in zip(pairs, shapes, ("delta", "dl", "dr", "dX")):
            if buf is not None:
                _guards_untouched(buf, sh[1], name)
        runs.append(views)
    for a, b in zip(*runs):
        assert (a is None and b is None) or same(a, b), "the second backward launch differs from the first"
    delta, dl, dr, dx = runs[0]
    shape3 = lambda t, n: None if t is None else t.reshape(n, h_sel, k)     # noqa: E731
    return shape3(delta, plan.n_rows), shape3(dl, plan.n_rows), shape3(dr, plan.n_cols), dx


# ------------------------------------------------------------------ 1. forward and statistics
@functools.lru_cache(maxsize=None)
def forward_case(d, n_heads):
    """x (bf16), l, r on the 48 x 1100 operands."""
    l, r = (dev(t) for t in node_terms(N_SMALL, N_BIG, 2, n_heads, seed=d + n_heads))
    return bf16_operand(values_gpu.operands(d)[0]), l, r


@pytest.mark.parametrize("d,n_heads", FORWARD_GRID)
def test_forward_and_statistics_have_the_bits_of_the_fp32_launches(d, n_heads):
    hops = values_gpu.forward_hops()
    x, l, r = forward_case(d, n_heads)
    slope = 0.2 if n_heads > 1 else 0.01
    for thr, rpw in KNOBS:
        where = f"d {d} K {n_heads} thr {thr} rpw {rpw}"
        plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
        with torch.no_grad():
            want, want_stats = plan.attention_heads_stats(x.float(), l, r, slope)
            assert same(plan.attention_heads(x.float(), l, r, slope), want)
        assert not bool(torch.isnan(want).any())
        for with_stats in (False, True):
            y32, s32 = raw_forward(plan, x, l, r, torch.float32, with_stats, slope)
            y16, s16 = raw_forward(plan, x, l, r, BF, with_stats, slope)
            assert same(y32, want), where + ": the fp32 Y differs from the fp32 launch on the upcast x"
            assert same(y16, want.to(BF)), where + ": the bf16 Y is not that value rounded to nearest even"
            if with_stats:
                assert same(s32, want_stats) and same(s16, want_stats), where + ": stats differ from the fp32 launch's"
        # the methods: bfloat16 by default, out_dtype, out=
        assert same(plan.attention_heads_bf16(x, l, r, slope), want.to(BF)), where
        y, s = plan.attention_heads_stats_bf16(x, l, r, slope, out_dtype=torch.float32)
        assert same(y, want) and same(s, want_stats), where


def test_forward_on_strided_operands_eight_hops_a_single_hop_and_a_wider_out():
    d, n_heads = 64, 2
    hops = values_gpu.forward_hops(8)
    plan = make_plan(hops, long_row_threshold=256, rows_per_wave=7)
    x = np.random.default_rng(8).uniform(-1, 1, (N_BIG, d)).astype(np.float32)
    l, r = node_terms(N_SMALL, N_BIG, 8, n_heads, seed=8)
    lt, rt = strided_rows(l), strided_rows(r)
    xbuf = torch.full((N_BIG, d + 4), float("nan"), dtype=BF, device=DEV)
    xbuf[:, :d] = bf16_operand(x)
    xt = xbuf[:, :d]
    assert xt.stride(0) == d + 4 and lt.stride(0) == 8 * n_heads + 4
    with torch.no_grad():
        want, want_stats = plan.attention_heads_stats(xt.float(), lt, rt)
    for dtype in (torch.float32, BF):
        y, s = raw_forward(plan, xt, lt, rt, dtype, True)
        assert same(y, want.to(dtype)) and same(s, want_stats), f"8 hops, strided, {dtype}"
    # a caller's out= with wider row AND hop strides: a guard band after every hop slot
    wide = torch.full((N_SMALL, 8, d + 2 * G), float("nan"), dtype=BF, device=DEV)
    y, s = plan.attention_heads_stats_bf16(xt, lt, rt, out=wide[:, :, G:G + d])
    assert y.data_ptr() == wide[:, :, G:].data_ptr() and y.stride(1) == d + 2 * G
    assert bool(torch.isnan(wide[:, :, :G]).all()) and bool(torch.isnan(wide[:, :, G + d:]).all()), "a guard column was written"
    assert same(y, want.to(BF)) and same(s, want_stats)
    # hops=[1]: the slot of the full launch
    two = make_plan(values_gpu.forward_hops(), long_row_threshold=256)
    x2, l2, r2 = forward_case(128, 8)
    with torch.no_grad():
        both = two.attention_heads(x2.float(), l2, r2)
    alone, _ = raw_forward(two, x2, l2[:, 1:2], r2[:, 1:2], BF, False, hops=[1])
    assert same(alone, both[:, 1:2].to(BF))
    assert same(two.attention_heads_bf16(x2, l2[:, 1:2], r2[:, 1:2], hops=[1]), both[:, 1:2].to(BF))


# ------------------------------------------------------------------ 2. backward
@functools.lru_cache(maxsize=None)
def backward_case(d, n_heads):
    """x, g (bf16), l, r on the 48 x 1100 operands."""
    x, l, r = forward_case(d, n_heads)
    return x, l, r, bf16_operand(values_gpu.operands(d)[1][:N_SMALL])


def check_backward(plan, x, l, r, g, where, needs=(True, True, True), slope=0.2):
    """The bf16 backward on the bf16 forward's own y against the fp32 backward on the upcast operands: delta, dl, dr and an fp32 dX
    bit for bit, a bf16 dX its rounding."""
    y, stats = plan.attention_heads_stats_bf16(x, l, r, slope)
    assert y.dtype == BF
    want = raw_backward(plan, torch.float32, x.float(), l, r, stats, y.float(), g.float(), slope=slope, needs=needs)
    got32 = raw_backward(plan, BF, x, l, r, stats, y, g, torch.float32, slope=slope, needs=needs)
    got16 = raw_backward(plan, BF, x, l, r, stats, y, g, BF, slope=slope, needs=needs)
    for name, w, a, b in zip(("delta", "dl", "dr", "dx"), want, got32, got16):
        if w is None:
            assert a is None and b is None, (where, name)
            continue
        assert not bool(torch.isnan(w).any())
        assert same(a, w), f"{where}: {name} (fp32 dX launch) differs from the fp32 backward on the upcast operands"
        assert same(b, w.to(BF) if name == "dx" else w), f"{where}: {name} (bf16 dX launch) differs"
    via = plan.attention_heads_backward_bf16(x, l, r, stats, y, g, slope, need_dl=needs[0], need_dr=needs[1], need_dx=needs[2])
    via32 = plan.attention_heads_backward_bf16(x, l, r, stats, y, g, slope, need_dl=needs[0], need_dr=needs[1], need_dx=needs[2],
                                               dx_dtype=torch.float32)
    for a, b, c in zip(via, via32, got16[1:]):
        assert (a is None and b is None and c is None) or (same(a, c) and same(b.to(c.dtype), c)), where + " (the method)"
    return want


@pytest.mark.parametrize("d,n_heads", BACKWARD_GRID)
def test_backward_has_the_bits_of_the_fp32_backward(d, n_heads):
    hops = values_gpu.forward_hops()
    x, l, r, g = backward_case(d, n_heads)
    for thr, rpw in KNOBS:
        plan = make_plan(hops, build_transpose=True, long_row_threshold=thr, rows_per_wave=rpw)
        check_backward(plan, x, l, r, g, f"d {d} K {n_heads} thr {thr} rpw {rpw}", slope=0.2 if n_heads > 1 else 0.01)


def test_backward_need_flags_a_symmetric_plan_and_a_plan_without_permutation():
    hops = values_gpu.forward_hops()
    x, l, r, g = backward_case(64, 8)
    plan = make_plan(hops, build_transpose=True, long_row_threshold=256, rows_per_wave=3)
    for needs in NEEDS:
        check_backward(plan, x, l, r, g, f"needs {needs}", needs=tuple(bool(v) for v in needs))
    sq = values_gpu.square_hops()
    n = sq[0].shape[0]
    rng = np.random.default_rng(12)
    xs, gs = bf16_operand(rng.uniform(-1, 1, (n, 128))), bf16_operand(rng.uniform(-1, 1, (n, 2, 128)))
    ls, rs = (dev(t) for t in node_terms(n, n, 2, 8, seed=12))
    sym = make_plan(sq, build_transpose=True, keep_permutation=True, symmetric_pattern=True, long_row_threshold=256)
    assert sym.transpose_sharing[0] != "none"
    noperm = make_plan(sq, build_transpose=True, keep_permutation=False, long_row_threshold=256)
    assert noperm.has_transpose and not noperm.keep_permutation
    a = check_backward(sym, xs, ls, rs, gs, "symmetric plan")
    b = check_backward(noperm, xs, ls, rs, gs, "plan without permutation", needs=(False, True, True))
    assert same(a[2], b[2]) and same(a[3], b[3]), "the two plans' column sides differ"


# ------------------------------------------------------------------ 3. special values
def test_special_values_have_the_bits_of_the_fp32_launch_rounded():
    d, n_heads = 32, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    x, l, r = (dev(t) for t in special_operands(d, n_heads))
    x = x.to(BF)                                                                    # (1e-40 -> a bf16 subnormal, 1e30 -> bf16(1e30))
    rng = np.random.default_rng(79)
    g = rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)
    hit = rng.random(g.shape) < 0.001
    g[hit] = np.asarray(SPECIALS, dtype=np.float32)[rng.integers(0, 6, int(hit.sum()))]
    g = bf16_operand(g)
    for thr in (32, 1024):
        plan = values_gpu.adjoint_plan(hops, long_row_threshold=thr)
        with torch.no_grad():
            want, want_stats = plan.attention_heads_stats(x.float(), l, r)
        frac = float(torch.isnan(want).float().mean())
        print(f"thr {thr}: {100 * frac:.1f} % of the fp32 forward's output is NaN")
        assert 0.05 <= frac <= 0.75, "the comparison would be vacuous"
        y16, s16 = raw_forward(plan, x, l, r, BF, True)
        y32, _ = raw_forward(plan, x, l, r, torch.float32, False)
        assert same_nan_aware(y32, want) and same_nan_aware(y16, want.to(BF)) and same_nan_aware(s16, want_stats), f"thr {thr}: forward"
        want_b = raw_backward(plan, torch.float32, x.float(), l, r, s16, y16.float(), g.float())
        got = raw_backward(plan, BF, x, l, r, s16, y16, g, BF)
        for name, w, a in zip(("delta", "dl", "dr", "dx"), want_b, got):
            assert same_nan_aware(a, w.to(BF) if name == "dx" else w), f"thr {thr}: {name}"
        assert bool(torch.isnan(got[3]).any()) and bool(torch.isfinite(got[3]).any())


def test_an_fp32_sum_beyond_bf16_rounds_to_infinity():
    """dX = g0 + g1 with alpha = 1 (every row has one entry): 2^127 + 2^127 * 0.99609375 is finite in fp32 and lies exactly between
    the largest finite bf16 and 2^128 -- the tie goes to even, which is infinity, as torch rounds it."""
    import scipy.sparse as sp

    n, d = 8, 8
    eye = sp.identity(n, dtype=np.float32, format="csr")
    hops = (eye, eye.copy())
    plan = make_plan(hops, build_transpose=True)
    x = bf16_operand(np.ones((n, d)))
    l, r = dev(np.zeros((n, 2, 2), dtype=np.float32)), dev(np.zeros((n, 2, 2), dtype=np.float32))
    g = np.zeros((n, 2, d), dtype=np.float32)
    g[:, 0], g[:, 1] = 2.0 ** 127, 2.0 ** 127 * 0.99609375
    g[3] = 1.0
    g = bf16_operand(g)
    assert float(g[0, 0, 0]) == 2.0 ** 127 and float(g[0, 1, 0]) == 2.0 ** 127 * 0.99609375              # (bf16 holds both exactly)
    y, stats = plan.attention_heads_stats_bf16(x, l, r)
    assert same(y, torch.ones((n, 2, d), dtype=BF, device=DEV))
    only_dx = (False, False, True)
    want = raw_backward(plan, torch.float32, x.float(), l, r, stats, y.float(), g.float(), needs=only_dx)[3]
    assert bool(torch.isfinite(want).all()) and float(want[0, 0]) == 2.0 ** 127 * 1.99609375
    got = raw_backward(plan, BF, x, l, r, stats, y, g, BF, needs=only_dx)[3]
    assert same(got, want.to(BF))
    assert bool(torch.isinf(got[0]).all()) and float(got[3, 0]) == 2.0


# ------------------------------------------------------------------ 4. the layer
@pytest.mark.parametrize("d,heads", ((128, 8), (32, 1)))
def test_layer_output_bits_and_gradients(d, heads):
    from h2gcn_amd import RecomputeMultiHeadHopAttention
    from h2gcn_amd.layers import _StackHeads

    graph = crafted()
    plan = graph.plan(**heads_gpu.KNOBS[1])
    x = heads_gpu.uniform((graph.n, d), 21).to(BF)
    rr = heads_gpu.uniform((graph.n, 2, d), 22).to(BF)
    torch.manual_seed(23)
    layer = RecomputeMultiHeadHopAttention(d, heads).to(DEV)
    # the fp32 layer on the upcast input
    y32 = layer(plan, x.float())
    layer.zero_grad()
    xin = x.clone().requires_grad_()
    y = layer(plan, xin)
    assert y.dtype == BF and same(y, y32.detach().to(BF)), "the output is not rne(the fp32 layer on x.float())"
    (y * rr).sum().backward()
    assert xin.grad is not None and xin.grad.dtype == BF and bool(torch.isfinite(xin.grad.float()).all()) and float(xin.grad.float().abs().max()) > 0
    # the parameter gradients: the fp32 plan methods on the upcast saved tensors, pushed through the same projections
    w = d // heads
    a_l, a_r = (p.detach().clone().requires_grad_() for p in (layer.a_l, layer.a_r))
    ls, rs = [], []
    for h in range(heads):
        x_h = (x if heads == 1 else x[:, h * w:(h + 1) * w]).float()
        ls.append(x_h @ a_l[:, h, :].t())
        rs.append(x_h @ a_r[:, h, :].t())
    l, r = _StackHeads.apply(*ls), _StackHeads.apply(*rs)
    y16, stats = plan.attention_heads_stats_bf16(x, l.detach(), r.detach(), layer.negative_slope)
    assert same(y16, y)
    dl, dr, dx = plan.attention_heads_backward(x.float(), l.detach(), r.detach(), stats, y16.float(), rr.float(), layer.negative_slope)
    want_l, want_r = torch.autograd.grad((l, r), (a_l, a_r), (dl, dr))
    assert same(layer.a_l.grad, want_l) and same(layer.a_r.grad, want_r), "a_l.grad / a_r.grad differ from the fp32 methods' on the upcast tensors"
    # x.grad: the rounded dx of the launch plus what flows back through the projections, summed in bfloat16 by autograd
    with torch.no_grad():
        assert same(layer(plan, x), y), "the fused bf16 launch under no_grad gives other bits"


def _net(d, heads, seed):
    from h2gcn_amd import RecomputeMultiHeadHopAttention

    torch.manual_seed(seed)
    a, b = RecomputeMultiHeadHopAttention(d, heads).to(DEV), RecomputeMultiHeadHopAttention(d, heads).to(DEV)
    params = list(a.parameters()) + list(b.parameters())

    def forward(plan, x):
        h = a(plan, x)
        return b(plan, torch.tanh(h[:, 0] + h[:, 1]))                                # two bf16 attention layers on ONE plan

    return forward, params


def test_captured_bf16_training_step_replays_to_the_eager_result():
    d = 32
    graph = crafted()
    plan = graph.plan(**heads_gpu.KNOBS[0])
    x, rr = heads_gpu.uniform((graph.n, d), 41).to(BF), heads_gpu.uniform((graph.n, 2, d), 42).to(BF)
    forward, params = _net(d, 8, seed=43)
    init = [p.detach().clone() for p in params]

    def step():
        for p in params:
            p.grad = None
        out = forward(plan, x)
        assert out.dtype == BF
        (out * rr).sum().backward()
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
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(params, eager))
    assert all(not torch.equal(p, q) for p, q in zip(eager, init))


# ------------------------------------------------------------------ 5. accuracy
def dense_forward64(hops, x, l, r, slope):
    """Masked softmax attention on dense [n_rows, n_cols, K] float64 arrays on the CPU -> y [n_rows, H_sel, d]."""
    X, L, R = (t.detach().cpu().double() for t in (x, l, r))
    n_rows, n_cols, k = L.shape[0], R.shape[0], L.shape[2]
    ys = []
    for s, m in enumerate(hops):
        mask = torch.zeros((n_rows, n_cols), dtype=torch.bool)
        coo = m.tocoo()
        mask[torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))] = True
        sc = torch.nn.functional.leaky_relu(L[:, None, s, :] + R[None, :, s, :], slope).masked_fill(~mask[:, :, None], float("-inf"))
        sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))
        alpha = torch.softmax(sc, dim=1) * mask[:, :, None].double()
        ys.append(torch.einsum("ijh,jhw->ihw", alpha, X.view(n_cols, k, -1)).reshape(n_rows, -1))
    return torch.stack(ys, dim=1)


def test_accuracy_against_fp64():
    """|y_bf16 - y64| <= 2^-8 |y64| + E32 elementwise at (128, 8) on the square graph.  y64: the dense fp64 replica on the same
    bf16-representable x.  E32: the largest error of the EXISTING fp32 launch against the same replica, measured here, never taken
    from the code under test.  The first term is derivable: y_bf16 = rne(y32), and one rounding to nearest even loses at most 2^-9
    |y32| <= 2^-9 (|y64| + E32); the second 2^-9 |y64| of the bound covers the 2^-9 E32 wherever |y64| >= E32."""
    d, n_heads = 128, 8
    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    rng = np.random.default_rng(55)
    x = bf16_operand(rng.uniform(-1, 1, (n, d)))
    l, r = (dev(t) for t in node_terms(n, n, 2, n_heads, seed=55))
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    y64 = dense_forward64(hops, x.float(), l, r, 0.2)
    with torch.no_grad():
        y32 = plan.attention_heads(x.float(), l, r)
    e32 = float((y32.cpu().double() - y64).abs().max())
    y16 = plan.attention_heads_bf16(x, l, r)
    err = (y16.cpu().double() - y64).abs()
    bound = 2.0 ** -8 * y64.abs() + e32
    print(f"E32 = {e32:.3e}; max |y_bf16 - y64| = {float(err.max()):.3e}; max of err / bound = {float((err / bound).max()):.3f}; "
          f"max |y64| = {float(y64.abs().max()):.3e}")
    assert e32 > 0 and bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond 2^-8 |y64| + E32"


# ------------------------------------------------------------------ 6. refusals that need a device
def test_refusals_of_the_library_and_of_the_methods():
    from h2gcn_amd import _capi

    hops = values_gpu.forward_hops()
    plan = make_plan(hops, build_transpose=True, long_row_threshold=256)
    x, l, r, g = backward_case(64, 8)
    d, k = 64, 8
    L = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.zeros((N_SMALL, 2, d), dtype=BF, device=DEV)
    stats = torch.zeros((N_SMALL, 2, 2, k), dtype=torch.float32, device=DEV)
    node = lambda xp, ldx: (plan._handle, plan._mask(None), _ptr(l), l.stride(0), _ptr(r), r.stride(0), k, 0.2, xp, ldx, d)     # noqa: E731
    odd = torch.zeros((N_BIG, d + 1), dtype=BF, device=DEV)
    flat = torch.zeros(N_BIG * d + 1, dtype=BF, device=DEV)
    cases = [
        ("bf16 X: the base address must be 4-byte aligned", lambda: L.h2gcn_attention_hops_heads_bf16(
            *node(C.c_void_p(flat.data_ptr() + 2), d), _capi.DTYPE_BF16, _ptr(y), 2 * d, d, stream)),
        ("bf16 X: row / hop strides must be even", lambda: L.h2gcn_attention_hops_heads_bf16(
            *node(_ptr(odd), d + 1), _capi.DTYPE_BF16, _ptr(y), 2 * d, d, stream)),
        ("bf16 Y: the base address must be 4-byte aligned", lambda: L.h2gcn_attention_hops_heads_stats_bf16(
            *node(_ptr(x), d), _capi.DTYPE_BF16, C.c_void_p(y.data_ptr() + 2), 2 * d, d, _ptr(stats), 4 * k, stream)),
        ("bf16 Y: row / hop strides must be even", lambda: L.h2gcn_attention_hops_heads_bf16(
            *node(_ptr(x), d), _capi.DTYPE_BF16, _ptr(y), 2 * d + 1, d, stream)),
        ("Y aliases X", lambda: L.h2gcn_attention_hops_heads_bf16(*node(_ptr(x), d), _capi.DTYPE_BF16, _ptr(x), 2 * d, d, stream)),
        ("y_dtype = 7", lambda: L.h2gcn_attention_hops_heads_bf16(*node(_ptr(x), d), 7, _ptr(y), 2 * d, d, stream)),
        ("bf16 G: row / hop strides must be even", lambda: L.h2gcn_attention_hops_heads_backward_bf16(
            *node(_ptr(x), d), _ptr(stats), 4 * k, _ptr(y), 2 * d, d, _ptr(g), 2 * d + 1, d, _ptr(stats), 2 * k, _ptr(stats), 2 * k, None, 2 * k,
            _capi.DTYPE_BF16, None, d, stream)),
        ("dX aliases X", lambda: L.h2gcn_attention_hops_heads_backward_bf16(
            *node(_ptr(x), d), _ptr(stats), 4 * k, _ptr(y), 2 * d, d, _ptr(g), 2 * d, d, _ptr(torch.zeros_like(stats)), 2 * k, None, 2 * k, None,
            2 * k, _capi.DTYPE_BF16, _ptr(x), d, stream)),
    ]
    for match, call in cases:
        assert call() == _capi.ERR_INVALID_ARGUMENT, match
        assert match.encode() in L.h2gcn_last_error(), (match, L.h2gcn_last_error())
    for match, call in (("4-byte aligned", lambda: plan.attention_heads_bf16(flat[1:].view(N_BIG, d), l, r)),
                        ("strides must be even", lambda: plan.attention_heads_stats_bf16(odd[:, :d], l, r)),
                        ("out overlaps the inputs", lambda: plan.attention_heads_bf16(x, l, r, out=x[:N_SMALL * 2].view(N_SMALL, 2, d)))):
        with pytest.raises(ValueError, match=match):
            call()
