"""GPU suite: the row-selected classifier entry points (csrc/classifier_rows.hip: h2gcn_dropout_dense_rows_f32 / _rows_bf16 /
_backward_rows_f32 / _backward_rows_bf16) against the full-matrix calls and the CPU restatement (oracle/classifier.py).

Contract (include/h2gcn_hip.h): with rows = rows_dev, Z_c == Z_full[rows] and dX_c == dX_full[rows] BIT FOR BIT (the full call
getting G_c scattered into a zero G), for fp32 and bf16 X and for fp32 and bf16 dX; dW deterministic, equal to the fp64
restatement on the zero-padded G within the tolerance the full-matrix suite asserts (2e-6 * max(sum |terms|, 1)).

Shapes (n_rows, m, K, C): one K group / one class; odd K with a partial group; the products width with 47 classes (more than one
workgroup of the full call, one row tile plus one row of the selection); four class tiles and more than one 512-column block
of dW; K with a partial 64-column chunk; m == n_rows (the identity selection).  rows always holds row 0 and row n_rows - 1; the
m == 1 shape cannot hold both and runs once with each."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import classifier as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SEED, STEP = 0x1234_5678_9ABC, 41


@pytest.fixture(autouse=True, params=["matrix-core kernels", "small-operand kernels where they apply"])
def _kernel_family(request):
    """Every test runs with the small-operand kernels switched off (h2gcn_dropout_dense_small_rows(0)) and with the shipped
    rule, which the row-selected calls apply to n_rows, as the full calls they are compared with do."""
    from h2gcn_amd import _capi
    L = _capi.lib()
    old = L.h2gcn_dropout_dense_small_rows(0 if request.param.startswith("matrix") else 12288)
    yield request.param
    L.h2gcn_dropout_dense_small_rows(old)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int16 if got.dtype == BF else torch.int32
    return torch.equal(got.detach().contiguous().view(it), want.detach().contiguous().view(it))


def _selections(n, m, rng):
    if m == 1:
        return [np.array([0]), np.array([n - 1])]
    if m == n:
        return [np.arange(n)]
    inner = rng.choice(np.arange(1, n - 1), size=m - 2, replace=False)
    return [np.sort(np.concatenate([[0, n - 1], inner]))]


def _full(L, x, w, b, g_full, keep, st, bf16, dx_dtype):
    """Z, dX (torch dtype dx_dtype) and dW of the full-matrix call."""
    from h2gcn_amd import _capi
    n, k = x.shape
    c = w.shape[1]
    ws = torch.empty(int(L.h2gcn_dropout_dense_workspace_bytes(n, k, c)), dtype=torch.uint8, device=DEV)
    z = torch.empty((n, c), device=DEV)
    dx = torch.empty((n, k + k % 2), device=DEV, dtype=dx_dtype)
    dw = torch.empty((k, c), device=DEV)
    if bf16:
        _capi.check(L.h2gcn_dropout_dense_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, SEED, _ptr(st), _ptr(z), c, _ptr(ws), ws.numel(), None))
        _capi.check(L.h2gcn_dropout_dense_backward_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g_full), c, keep, SEED, _ptr(st),
                                                        _capi.DTYPE_BF16 if dx_dtype == BF else _capi.DTYPE_F32, _ptr(dx), dx.stride(0), _ptr(dw),
                                                        _ptr(ws), ws.numel(), None))
    else:
        _capi.check(L.h2gcn_dropout_dense_f32(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, SEED, _ptr(st), _ptr(z), c, _ptr(ws), ws.numel(), None))
        _capi.check(L.h2gcn_dropout_dense_backward_f32(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g_full), c, keep, SEED, _ptr(st),
                                                       _ptr(dx), dx.stride(0), _ptr(dw), _ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    return z, dx[:, :k], dw


@pytest.mark.parametrize("n,m,k,c", [(5, 1, 4, 1), (300, 37, 7, 3), (4099, 129, 448, 47), (4099, 513, 896, 64), (1000, 300, 130, 17),
                                     (300, 300, 7, 3)])
@pytest.mark.parametrize("keep", [0.5, 0.9, 1.0])
def test_rows_calls_have_the_bits_of_the_full_calls_rows(n, m, k, c, keep):
    from h2gcn_amd import _capi
    L = _capi.lib()
    rng = np.random.default_rng(n * 7 + k + c + m)
    pad = k % 2
    x32buf = torch.zeros((n, k + 5), device=DEV)                  # strided, only 4-byte aligned rows
    x32 = x32buf[:, 1:1 + k]
    x32.copy_(torch.from_numpy(rng.uniform(-1, 1, (n, k)).astype(np.float32)))
    xbfbuf = torch.zeros((n, k + 6 + pad), device=DEV, dtype=BF)  # a column slot of a wider buffer, even row stride
    xbf = xbfbuf[:, 2:2 + k]
    xbf.copy_(x32)
    w = torch.from_numpy(rng.uniform(-0.3, 0.3, (k, c)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.uniform(-0.5, 0.5, c).astype(np.float32)).to(DEV)
    st = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    for rows_np in _selections(n, m, rng):
        rows = torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
        rl = rows.to(torch.int64)
        g_c = torch.from_numpy(rng.uniform(-1, 1, (m, c)).astype(np.float32)).to(DEV)
        g_full = torch.zeros((n, c), device=DEV)
        g_full[rl] = g_c
        ws = torch.empty(int(L.h2gcn_dropout_dense_workspace_bytes(m, k, c)), dtype=torch.uint8, device=DEV)   # sized by n_sel
        for bf16, x in ((False, x32), (True, xbf)):
            xn = x.float().cpu().numpy()
            dx_w, dw_w, _ = oc.dropout_dense_grad(xn, w.cpu().numpy(), g_full.cpu().numpy(), keep, SEED, STEP)   # fp64, once per X
            mag_w = np.abs(np.where(oc.keep_mask(n, k, keep, SEED, STEP), xn / keep, 0)).T @ np.abs(g_full.cpu().numpy())
            for dx_dtype in ((torch.float32, BF) if bf16 else (torch.float32,)):
                z_full, dx_full, _ = _full(L, x, w, b, g_full, keep, st, bf16, dx_dtype)
                zbuf = torch.full((m + 2, c + 3), 9.0, device=DEV)          # guard rows and guard columns
                dxbuf = torch.full((m + 2, k + 2 + pad), 5.0, device=DEV, dtype=dx_dtype)
                dws = []
                for _ in range(2):
                    dw = torch.empty((k, c), device=DEV)
                    if bf16:
                        _capi.check(L.h2gcn_dropout_dense_rows_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, SEED, _ptr(st),
                                                                    _ptr(zbuf[1:]), zbuf.stride(0), _ptr(ws), ws.numel(), None, _ptr(rows), m))
                        _capi.check(L.h2gcn_dropout_dense_backward_rows_bf16(
                            _ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g_c), c, keep, SEED, _ptr(st),
                            _capi.DTYPE_BF16 if dx_dtype == BF else _capi.DTYPE_F32, _ptr(dxbuf[1:]), dxbuf.stride(0), _ptr(dw), _ptr(ws), ws.numel(),
                            None, _ptr(rows), m))
                    else:
                        _capi.check(L.h2gcn_dropout_dense_rows_f32(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, SEED, _ptr(st),
                                                                   _ptr(zbuf[1:]), zbuf.stride(0), _ptr(ws), ws.numel(), None, _ptr(rows), m))
                        _capi.check(L.h2gcn_dropout_dense_backward_rows_f32(
                            _ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g_c), c, keep, SEED, _ptr(st), _ptr(dxbuf[1:]), dxbuf.stride(0), _ptr(dw),
                            _ptr(ws), ws.numel(), None, _ptr(rows), m))
                    torch.cuda.synchronize()
                    dws.append(dw)
                what = (bf16, dx_dtype, rows_np[:4])
                assert torch.equal(zbuf[1:m + 1, :c], z_full[rl]), what
                assert same_bits(dxbuf[1:m + 1, :k], dx_full[rl]), what
                assert bool((zbuf[:, c:] == 9.0).all()) and bool((zbuf[0] == 9.0).all()) and bool((zbuf[m + 1] == 9.0).all()), what
                assert bool((dxbuf[:, k:] == 5.0).all()) and bool((dxbuf[0] == 5.0).all()) and bool((dxbuf[m + 1] == 5.0).all()), what
                assert same_bits(dws[0], dws[1]), what                        # deterministic
                err = np.abs(dws[0].cpu().numpy() - dw_w)
                print(f"rows dW: bf16 X {bf16} dX {dx_dtype} max|err| {err.max():.3e} max bound {(2e-6 * np.maximum(mag_w, 1.0)).max():.3e}")
                assert (err <= 2e-6 * np.maximum(mag_w, 1.0)).all(), (what, err.max())
    assert bool((x32buf[:, 0] == 0).all()) and bool((x32buf[:, 1 + k:] == 0).all())
    assert bool((xbfbuf[:, :2] == 0).all()) and bool((xbfbuf[:, 2 + k:] == 0).all())


def test_dx_alone_dw_alone_and_an_empty_selection():
    from h2gcn_amd import _capi
    L = _capi.lib()
    n, m, k, c = 300, 37, 130, 17
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, k)).astype(np.float32)).to(DEV)
    w = torch.from_numpy(rng.uniform(-0.3, 0.3, (k, c)).astype(np.float32)).to(DEV)
    g_c = torch.from_numpy(rng.uniform(-1, 1, (m, c)).astype(np.float32)).to(DEV)
    rows = torch.from_numpy(_selections(n, m, rng)[0].astype(np.int32)).to(DEV)
    st = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    ws = torch.empty(int(L.h2gcn_dropout_dense_workspace_bytes(m, k, c)), dtype=torch.uint8, device=DEV)

    def call(dx, dw, n_sel=m):
        _capi.check(L.h2gcn_dropout_dense_backward_rows_f32(_ptr(x), k, n, k, _ptr(w), c, _ptr(g_c), c, 0.5, SEED, _ptr(st), _ptr(dx), k, _ptr(dw),
                                                            _ptr(ws), ws.numel(), None, _ptr(rows), n_sel))
        torch.cuda.synchronize()
    dx_both, dw_both = torch.empty((m, k), device=DEV), torch.empty((k, c), device=DEV)
    call(dx_both, dw_both)
    dx_only, dw_only = torch.empty((m, k), device=DEV), torch.empty((k, c), device=DEV)
    call(dx_only, None)
    call(None, dw_only)
    assert torch.equal(dx_only, dx_both) and torch.equal(dw_only, dw_both)
    dw0 = torch.full((k, c), 3.0, device=DEV)
    call(None, dw0, n_sel=0)                                                  # nothing selected: dW is zero-filled
    assert bool((dw0 == 0).all())


def test_module_logits_of_a_row_subset():
    """DropoutDense(x, rows=sel) under no_grad: the rows of the full logits, bit for bit, in evaluation and (same step) training."""
    import scipy.sparse as sp
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import DropoutDense

    torch.manual_seed(3)
    n, k, c = 500, 64, 7
    plan = HopPlan.from_scipy([sp.random(n, n, 0.01, format="csr", random_state=0, dtype=np.float32)], DEV)
    sel = plan.select_rows([0, 17, 255, n - 1], build_transpose=False)
    layer = DropoutDense(k, c, use_bias=True, drop_prob=0.5).to(DEV)
    for x in (torch.randn((n, k), device=DEV), torch.randn((n, k), device=DEV).to(BF)):
        with torch.no_grad():
            assert torch.equal(layer.eval()(x, rows=sel), layer(x)[sel.rows_long])
            layer.train()
            full = layer(x)
            layer._step -= 1                                                  # the same step: the same mask
            assert torch.equal(layer(x, rows=sel), full[sel.rows_long])
    with pytest.raises(ValueError, match="cannot return a gradient for x"):
        layer(torch.randn((n, k), device=DEV, requires_grad=True), rows=sel)
    z = layer(torch.randn((n, k), device=DEV), rows=sel)                      # kernel and bias still get their gradients
    z.sum().backward()
    assert layer.kernel.grad is not None and layer.bias.grad is not None
