"""GPU suite: bf16 embeddings in the hop SpMM and its adjoint (ABI 5), fp32-accumulated.

The contract (include/h2gcn_hip.h): every gathered bf16 element is widened exactly and summed in fp32 in the canonical tree, so
an fp32 output is BIT-IDENTICAL to the fp32 launch on the upcast operand -- hence to the oracle's tree on it -- and a bf16 output
is exactly that value rounded to nearest even (torch's ``.to(torch.bfloat16)``).  Every check below is a bit comparison, except
the documented accuracy bound against an fp32 source (test 9)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from conftest import load_planetoid_golden, load_syn_products_golden
from oracle import gcn_layer as og
from oracle import operands as oo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def rne(a) -> torch.Tensor:
    """fp32 numpy array / tensor -> bf16 tensor on the CPU, torch's rounding (round to nearest even)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a.float().cpu()
    return t.to(BF)


def same_bits(got: torch.Tensor, want) -> bool:
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    got, want = got.detach().cpu().contiguous(), want.cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int16 if got.dtype == BF else torch.int32
    return torch.equal(got.view(it), want.view(it))


def random_hops(rng, n):
    """the operands of test_spmm_gpu.py::test_bits_are_the_canonical_tree_for_every_schedule: Poisson degrees, 10 % empty rows,
    four long rows (70 / 300 / 129 / 1000 nonzeros)"""
    hops = []
    for k in range(2):
        deg = np.minimum(rng.poisson(5 * (2 * k + 1), n), n)
        deg[rng.random(n) < 0.1] = 0
        deg[rng.integers(0, n, 4)] = [70, 300, 129, 1000]
        rows = np.repeat(np.arange(n), deg)
        cols = np.concatenate([rng.choice(n, kk, replace=False) for kk in deg])
        m = sp.csr_matrix((rng.uniform(-1, 1, len(rows)).astype(np.float32), (rows, cols)), shape=(n, n))
        m.sort_indices()
        hops.append(m)
    return hops


# ---- 1. bits for every schedule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 6, 64, 100, 128, 130, 256])
@pytest.mark.parametrize("thr", [0, 20, 100])
def test_bits_are_the_canonical_tree_for_every_schedule(d, thr):
    from h2gcn_amd import HopPlan

    rng = np.random.default_rng(d * 11 + thr)
    n = 1500
    hops = random_hops(rng, n)
    xb = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(BF)
    wb = torch.from_numpy(rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)).to(BF)
    x_up, w_up = xb.float().numpy(), wb.float().numpy()
    thr_eff = thr if thr else 256
    tree = og.gcn_layer_tree(hops, x_up, long_threshold=thr_eff)
    tree_t = og.gcn_layer_grad_tree(hops, w_up, n, long_threshold=thr_eff)
    tree_b, tree_tb = rne(tree), rne(tree_t)
    xt, wt = xb.to(dev()), wb.to(dev())
    for variant in (0, 2, 3, 5, 6):
        for sc in (0, 64, 128, 256):
            plan = HopPlan.from_scipy(hops, dev(), build_transpose=True, long_row_threshold=thr, variant=variant, slice_cols=sc)
            where = (variant, sc, plan.schedule(d))
            assert same_bits(plan.spmm(xt, out_dtype=torch.float32), tree), where
            assert same_bits(plan.spmm(xt), tree_b), where
            assert same_bits(plan.spmm_t(wt, out_dtype=torch.float32), tree_t), (where, "adjoint")
            assert same_bits(plan.spmm_t(wt), tree_tb), (where, "adjoint")
            assert same_bits(plan.spmm(xt, hops=[1]), tree_b[:, 1:]), (where, "hops=[1]")
            assert same_bits(plan.spmm(xt, hops=[1], out_dtype=torch.float32), tree[:, 1:]), (where, "hops=[1]")
    plan = HopPlan.from_scipy(hops, dev(), long_row_threshold=thr)
    if d >= 32:   # feature chunks of unequal even widths, written into one output (fp32 and bf16)
        for widths in ([16, d - 16], [d - 16, 16], [2 * (d // 4), d - 2 * (d // 4)], [16, 2 * (d // 4) - 16, d - 2 * (d // 4)]):
            for odt, want in ((torch.float32, torch.from_numpy(tree)), (BF, tree_b)):
                y = torch.empty((n, 2, d), device=dev(), dtype=odt)
                c0 = 0
                for wd in widths:
                    plan.spmm(xt[:, c0:c0 + wd], out=y[:, :, c0:c0 + wd])
                    c0 += wd
                assert same_bits(y, want), (widths, odt)
    # a row block (what a rank of the row partition computes) gives the same rows
    sub = HopPlan.from_scipy([h[400:900] for h in hops], dev(), long_row_threshold=thr)
    assert same_bits(sub.spmm(xt), tree_b[400:900])
    assert same_bits(sub.spmm(xt, out_dtype=torch.float32), tree[400:900])


# ---- 2. same as fp32 on the upcast input ------------------------------------------------------------------------------------
def _golden_operands():
    g = load_planetoid_golden("cora")
    yield "cora_sym", [g["hop1_sym"], g["hop2_sym"]], g["n"]
    yield "cora_rw", [g["hop1_rw"], g["hop2_rw"]], g["n"]
    a, _, _ = load_syn_products_golden()
    yield "syn_products", oo.adj_norm_hops(oo.remove_eye(a), ("1", "2"), oo.SYM), a.shape[0]


@pytest.mark.parametrize("d", [64, 128])
def test_equals_the_fp32_launch_on_the_upcast_input(d):
    from h2gcn_amd import HopPlan

    for name, hops, n in _golden_operands():
        rng = np.random.default_rng(d)
        plan = HopPlan.from_scipy(hops, dev(), build_transpose=True)
        xb = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev()).to(BF)
        wb = torch.from_numpy(rng.standard_normal((n, 2, d)).astype(np.float32)).to(dev()).to(BF)
        y32 = plan.spmm(xb.float())
        assert same_bits(plan.spmm(xb, out_dtype=torch.float32), y32), name
        assert same_bits(plan.spmm(xb), y32.to(BF)), name
        dx32 = plan.spmm_t(wb.float())
        assert same_bits(plan.spmm_t(wb, out_dtype=torch.float32), dx32), name
        assert same_bits(plan.spmm_t(wb), dx32.to(BF)), name


# ---- 3. rounding ------------------------------------------------------------------------------------------------------------
def _one_neighbour_plan(a: float, d: int = 4):
    from h2gcn_amd import HopPlan

    m = sp.csr_matrix((np.array([a], dtype=np.float32), np.array([0]), np.array([0, 1])), shape=(1, 1))
    return HopPlan.from_scipy([m], dev(), build_transpose=True)


@pytest.mark.parametrize("a,want", [(1 + 2 ** -8, 1.0), (1 + 3 * 2 ** -8, 1 + 2 ** -6)])
def test_exact_ties_round_to_even(a, want):
    plan = _one_neighbour_plan(a)
    xb = torch.ones((1, 4), device=dev(), dtype=BF)
    y32 = plan.spmm(xb, out_dtype=torch.float32)
    assert (y32 == a).all()                     # the tie itself is exact in fp32
    y = plan.spmm(xb)
    assert y.dtype == BF and (y.float() == want).all(), y
    dx = plan.spmm_t(xb.view(1, 1, 4))
    assert (dx.float() == want).all(), dx


def test_overflow_rounds_to_inf():
    bf16_max = torch.finfo(BF).max
    a = 1 + 2 ** -8
    plan = _one_neighbour_plan(a)
    xb = torch.full((1, 4), bf16_max, device=dev(), dtype=BF)
    y32 = plan.spmm(xb, out_dtype=torch.float32)
    assert torch.isfinite(y32).all()            # finite in fp32 ...
    y = plan.spmm(xb)
    assert torch.isinf(y.float()).all() and (y.float() > 0).all()   # ... inf in bf16, as torch rounds it
    assert same_bits(y, y32.to(BF))
    y_neg = plan.spmm(-xb)
    assert same_bits(y_neg, plan.spmm(-xb, out_dtype=torch.float32).to(BF)) and torch.isinf(y_neg.float()).all()


@pytest.mark.parametrize("d", [6, 64, 128, 256])
def test_bias_relu_epilogue_runs_before_the_rounding(d):
    from h2gcn_amd import HopPlan

    rng = np.random.default_rng(5 + d)
    n = 1200
    hops = random_hops(rng, n)
    xb = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(BF)
    bias = rng.uniform(-0.5, 0.5, d).astype(np.float32)
    tree = og.gcn_layer_tree(hops, xb.float().numpy())
    want = np.maximum(tree + bias, np.float32(0))
    plan = HopPlan.from_scipy(hops, dev())
    bt = torch.from_numpy(bias).to(dev())
    assert same_bits(plan.spmm(xb.to(dev()), bias=bt, relu=True), rne(want))
    assert same_bits(plan.spmm(xb.to(dev()), bias=bt, relu=True, out_dtype=torch.float32), want)
    assert same_bits(plan.spmm(xb.to(dev()), bias=bt), rne(tree + bias))


# ---- 4. accumulate ----------------------------------------------------------------------------------------------------------
def test_accumulate_into_fp32_dx_and_rejection_for_bf16_dx():
    from h2gcn_amd import HopPlan, _capi
    from h2gcn_amd._capi import H2GCNError

    rng = np.random.default_rng(9)
    n, d = 1500, 128
    hops = random_hops(rng, n)
    wb = torch.from_numpy(rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)).to(BF)
    dx0 = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    tree_t = og.gcn_layer_grad_tree(hops, wb.float().numpy(), n)
    plan = HopPlan.from_scipy(hops, dev(), build_transpose=True)
    out = torch.from_numpy(dx0).to(dev())
    got = plan.spmm_t(wb.to(dev()), out=out, accumulate=True)
    assert got.data_ptr() == out.data_ptr()
    assert same_bits(got, dx0 + tree_t)
    out_b = torch.zeros((n, d), device=dev(), dtype=BF)
    with pytest.raises(ValueError, match="accumulate"):
        plan.spmm_t(wb.to(dev()), out=out_b, accumulate=True)
    L = _capi.lib()
    opts = _capi.LaunchOpts(struct_size=_capi.C.sizeof(_capi.LaunchOpts), flags=_capi.LAUNCH_ACCUMULATE)
    with pytest.raises(H2GCNError, match="ACCUMULATE"):
        _capi.check(L.h2gcn_spmm_hops_T_bf16(plan._handle, 0, _capi.C.c_void_p(wb.to(dev()).data_ptr()), 2 * d, d, d, _capi.DTYPE_BF16,
                                             _capi.C.c_void_p(out_b.data_ptr()), d, _capi.C.byref(opts), None))


# ---- 5. 64-bit gather offsets ----------------------------------------------------------------------------------------------
def test_x_beyond_4gib_uses_64bit_gather_offsets():
    """bf16 X of 4.35 GB: the 32-bit offset decision is made in bytes of the real element size (2 B), so the launch takes the
    64-bit-offset kernels; checked against the tree on the referenced rows of the upcast X."""
    from h2gcn_amd import HopPlan

    device = dev()
    n_cols, d, n_rows = 17_000_000, 128, 4096
    assert n_cols * d * 2 > 2 ** 32
    x = torch.empty((n_cols, d), device=device, dtype=BF)
    col = torch.arange(d, device=device, dtype=torch.float32)[None, :] * 1e-2
    for r0 in range(0, n_cols, 2_000_000):
        r1 = min(n_cols, r0 + 2_000_000)
        base = torch.arange(r0, r1, device=device, dtype=torch.float32).remainder_(1000.0).mul_(1e-3)
        x[r0:r1] = (base[:, None] + col).to(BF)
    rng = np.random.default_rng(4)
    deg = rng.integers(0, 40, n_rows)
    deg[7] = 700  # one long segment too
    deg[-1] = max(deg[-1], 1)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(n_cols, k, replace=False)) for k in deg]).astype(np.int32)
    cols[-1] = n_cols - 1  # touch the very last row of X (the last row's largest column)
    vals = rng.uniform(-1, 1, len(cols)).astype(np.float32)
    m = sp.csr_matrix((vals, cols, rowptr), shape=(n_rows, n_cols))
    m.sort_indices()
    plan = HopPlan.from_scipy([m, m[::-1]], device)
    y32 = plan.spmm(x, out_dtype=torch.float32)
    y16 = plan.spmm(x)
    used = np.unique(m.indices)
    xs = x[torch.from_numpy(used.astype(np.int64)).to(device)].float().cpu().numpy()
    del x
    remap = sp.csr_matrix((m.data, np.searchsorted(used, m.indices), m.indptr), shape=(n_rows, len(used)))
    tree = og.gcn_layer_tree([remap, remap[::-1]], xs)
    assert same_bits(y32, tree)
    assert same_bits(y16, rne(tree))


# ---- 6. hipGraph ------------------------------------------------------------------------------------------------------------
def test_captured_bf16_launches_replay_the_eager_bits():
    from h2gcn_amd import HopPlan

    rng = np.random.default_rng(6)
    n, d = 3000, 128
    hops = random_hops(rng, n)
    plan = HopPlan.from_scipy(hops, dev(), build_transpose=True)
    xb = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(dev()).to(BF)
    wb = torch.from_numpy(rng.uniform(-1, 1, (n, 1, d)).astype(np.float32)).to(dev()).to(BF)
    # eager warm-up: one launch per hop selection and width (builds the selection's device lists)
    want_y, want_y32 = plan.spmm(xb, hops=[1]), plan.spmm(xb, out_dtype=torch.float32)
    want_dx, want_dx32 = plan.spmm_t(wb, hops=[1]), plan.spmm_t(wb, hops=[1], out_dtype=torch.float32)
    torch.cuda.synchronize()
    y, y32 = torch.empty_like(want_y), torch.empty_like(want_y32)
    dx, dx32 = torch.empty_like(want_dx), torch.empty_like(want_dx32)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.spmm(xb, hops=[1], out=y)
        plan.spmm(xb, out=y32)
        plan.spmm_t(wb, hops=[1], out=dx)
        plan.spmm_t(wb, hops=[1], out=dx32)
    for _ in range(2):
        for t in (y, y32, dx, dx32):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(y, want_y) and same_bits(y32, want_y32) and same_bits(dx, want_dx) and same_bits(dx32, want_dx32)
    assert same_bits(want_y, rne(og.gcn_layer_tree([hops[1]], xb.float().cpu().numpy())))


# ---- 7. autograd ------------------------------------------------------------------------------------------------------------
def test_autograd_bf16_in_bf16_out_bf16_grad():
    from h2gcn_amd import GCNLayer, HopPlan, hop_spmm

    rng = np.random.default_rng(7)
    n, d = 1500, 64
    hops = random_hops(rng, n)
    plan = HopPlan.from_scipy(hops, dev(), build_transpose=True)
    x0 = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(BF)
    g0 = torch.from_numpy(rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)).to(BF)
    tree = og.gcn_layer_tree(hops, x0.float().numpy())
    tree_t = og.gcn_layer_grad_tree(hops, g0.float().numpy(), n)
    for f in (lambda x: hop_spmm(plan, x), lambda x: GCNLayer()(plan, x)):
        x = x0.to(dev()).requires_grad_(True)
        y = f(x)
        assert y.dtype == BF and same_bits(y, rne(tree))
        y.backward(g0.to(dev()))
        assert x.grad.dtype == BF and same_bits(x.grad, rne(tree_t))
    x = x0.to(dev()).requires_grad_(True)
    y = GCNLayer(hops=[1])(plan, x)
    y.backward(g0[:, 1:].to(dev()))
    assert same_bits(y, rne(tree[:, 1:]))
    assert same_bits(x.grad, rne(og.gcn_layer_grad_tree([hops[1]], g0[:, 1:].float().numpy(), n)))


# ---- 8. rejections ----------------------------------------------------------------------------------------------------------
def test_every_rule_is_rejected_with_a_message():
    from h2gcn_amd import HopPlan, _capi
    from h2gcn_amd._capi import H2GCNError

    C = _capi.C
    rng = np.random.default_rng(8)
    n, d = 1500, 64
    hops = random_hops(rng, n)
    plan = HopPlan.from_scipy(hops, dev(), build_transpose=True)
    xb = torch.zeros((n, d + 2), device=dev(), dtype=BF)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        plan.spmm(xb.half())
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        plan.spmm_t(torch.zeros((n, 2, d), device=dev(), dtype=torch.float16))
    with pytest.raises(ValueError, match="float32 -> bfloat16"):
        plan.spmm(xb.float(), out_dtype=BF)
    with pytest.raises(ValueError, match="float32 -> bfloat16"):
        plan.spmm(xb.float(), out=torch.empty((n, 2, d + 2), device=dev(), dtype=BF))
    with pytest.raises(ValueError, match="float32 -> bfloat16"):
        plan.spmm_t(torch.zeros((n, 2, d), device=dev()), out_dtype=BF)
    with pytest.raises(ValueError, match="d must be even"):
        plan.spmm(xb[:, :d - 1])
    with pytest.raises(ValueError, match="strides must be even"):
        plan.spmm(torch.zeros((n, d + 1), device=dev(), dtype=BF)[:, :d])
    with pytest.raises(ValueError, match="4-byte aligned"):
        plan.spmm(xb[:, 1:d + 1])
    with pytest.raises(ValueError, match="strides must be even"):
        plan.spmm(xb[:, :d], out=torch.empty((n, 2, d + 1), device=dev(), dtype=BF)[:, :, :d])
    with pytest.raises(ValueError, match="d must be even"):
        plan.spmm_t(torch.zeros((n, 2, 7), device=dev(), dtype=BF))
    with pytest.raises(ValueError, match="accumulate"):
        plan.spmm_t(torch.zeros((n, 2, d), device=dev(), dtype=BF), out=torch.zeros((n, d), device=dev(), dtype=BF), accumulate=True)
    # ... and through the C ABI directly (H2GCNError carrying the library's message)
    L = _capi.lib()
    y = torch.empty((n, 2, d + 2), device=dev(), dtype=BF)

    def fwd(x_ptr, ldx, dd, dtype, y_ptr, ldy_row, ldy_hop):
        _capi.check(L.h2gcn_spmm_hops_bf16(plan._handle, 0, C.c_void_p(x_ptr), ldx, dd, dtype, C.c_void_p(y_ptr), ldy_row, ldy_hop,
                                           None, None))

    xp, yp = xb.data_ptr(), y.data_ptr()
    fwd(xp, d + 2, d, _capi.DTYPE_BF16, yp, 2 * (d + 2), d + 2)   # the valid launch
    for args, msg in (((xp, d + 2, d, 5, yp, 2 * (d + 2), d + 2), "y_dtype"),
                      ((xp + 2, d + 2, d, _capi.DTYPE_BF16, yp, 2 * (d + 2), d + 2), "4-byte aligned"),
                      ((xp, d + 1, d, _capi.DTYPE_BF16, yp, 2 * (d + 2), d + 2), "strides must be even"),
                      ((xp, d + 2, d - 1, _capi.DTYPE_BF16, yp, 2 * (d + 2), d + 2), "d must be even"),
                      ((xp, d + 2, d, _capi.DTYPE_BF16, yp + 2, 2 * (d + 2), d + 2), "4-byte aligned"),
                      ((xp, d + 2, d, _capi.DTYPE_BF16, yp, 2 * (d + 2), d + 1), "strides must be even")):
        with pytest.raises(H2GCNError, match=msg):
            fwd(*args)
    g = torch.zeros((n, 2, d), device=dev(), dtype=BF)
    dx = torch.empty((n, d), device=dev(), dtype=BF)
    with pytest.raises(H2GCNError, match="dx_dtype"):
        _capi.check(L.h2gcn_spmm_hops_T_bf16(plan._handle, 0, C.c_void_p(g.data_ptr()), 2 * d, d, d, -1, C.c_void_p(dx.data_ptr()), d,
                                             None, None))
    with pytest.raises(H2GCNError, match="strides must be even"):
        _capi.check(L.h2gcn_spmm_hops_T_bf16(plan._handle, 0, C.c_void_p(g.data_ptr()), 2 * d, d - 1, d - 2, _capi.DTYPE_F32,
                                             C.c_void_p(dx.data_ptr()), d, None, None))


# ---- 9. accuracy against the fp32 source (the documented bound) ------------------------------------------------------------
def test_accuracy_against_the_fp32_source():
    from h2gcn_amd import HopPlan

    a, labels, _ = load_syn_products_golden()
    hops = oo.adj_norm_hops(oo.remove_eye(a), ("1", "2"), oo.SYM)
    rng = np.random.default_rng(12)
    n, d = a.shape[0], 128
    x = (rng.standard_normal((n, d)) + labels[:, None] * 0.1).astype(np.float32)
    plan = HopPlan.from_scipy(hops, dev())
    xt = torch.from_numpy(x).to(dev())
    y_b = plan.spmm(xt.to(BF), out_dtype=torch.float32).cpu().numpy()
    y_f = plan.spmm(xt).cpu().numpy()
    mag = og.gcn_layer_f64acc([abs(sp.csr_matrix(h)) for h in hops], np.abs(x))
    err = np.abs(y_b - y_f)
    assert (err <= 2.0 ** -7 * mag).all(), float((err / np.maximum(mag, 1e-30)).max())
    assert float((err / np.maximum(mag, 1e-30)).max()) > 2.0 ** -12   # (the bf16 rounding is really there)


# ---- 10. full size ----------------------------------------------------------------------------------------------------------
def _device_operands(shape):
    from h2gcn_amd import synth

    cfg = synth.SHAPES[shape]
    n, d = cfg["n"], cfg["d"]
    device = torch.device("cuda", 0)
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, device) for k in range(2)]
    x = synth.synth_features(d, synth.SEED_X, 0, n, device)
    return csr, x, n, d


def _round_bf16_host(x: np.ndarray) -> np.ndarray:
    """round to nearest even, fp32 -> bf16 bits (uint16), in numpy (no NaNs in these operands)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_arxiv_shape_every_element_against_the_tree():
    from h2gcn_amd import HopPlan
    from oracle import fullsize as fs

    csr, x, n, d = _device_operands("arxiv")
    parts, x_host, _, _ = fs.host_operands("arxiv")
    xb = x.to(BF)
    xb_host = _round_bf16_host(x_host)
    assert np.array_equal(xb.view(torch.int16).cpu().numpy().view(np.uint16), xb_host)   # device rounding == host rounding
    x_up = (xb_host.astype(np.uint32) << 16).view(np.float32)
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n)
    y32 = plan.spmm(xb, out_dtype=torch.float32)
    y16 = plan.spmm(xb)
    torch.cuda.synchronize()
    tree = fs.gcn_layer_tree_mt(parts, x_up)
    bad, first = fs.count_bit_mismatches(y32.cpu().numpy(), tree)
    assert bad == 0, f"{bad} of {tree.size} elements differ from the canonical tree, first at flat index {first}"
    assert same_bits(y16, rne(tree))


def test_products_shape_equals_the_fp32_launch_on_the_upcast_input():
    from h2gcn_amd import HopPlan, synth

    csr, x, n, d = _device_operands("products")
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n, build_transpose=True)
    xb = x.to(BF)
    del x
    x_up = xb.float()
    y_ref = plan.spmm(x_up)
    del x_up
    y16 = plan.spmm(xb)
    assert torch.equal(y16.view(torch.int16), y_ref.to(BF).view(torch.int16))
    del y16
    assert torch.equal(plan.spmm(xb, out_dtype=torch.float32).view(torch.int32), y_ref.view(torch.int32))
    del y_ref, xb
    wb = synth.synth_features(2 * d, 77, 0, n, torch.device("cuda", 0)).view(n, 2, d).to(BF)
    dx_ref = plan.spmm_t(wb.float())
    assert torch.equal(plan.spmm_t(wb, out_dtype=torch.float32).view(torch.int32), dx_ref.view(torch.int32))
    assert torch.equal(plan.spmm_t(wb).view(torch.int16), dx_ref.to(BF).view(torch.int16))
