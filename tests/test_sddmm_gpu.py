"""GPU suite: the gradient of the hop SpMM with respect to the stored adjacency values -- HopPlan.sddmm (h2gcn_sddmm_hops_f32 /
_bf16, csrc/sddmm.hip) and hop_spmm(..., values=...) / GCNLayer.forward(..., values=...) on top of it.

Operands (fixed seeds):
  * a crafted 41 x 200 operand, 3 hops of different patterns, row lengths 0, 1, 2, 15, 16, 17, 63, 64, 65 and 130 (every hop
    holds each of them, on different rows), planned with long_row_threshold = 32 (the rows of 63+ entries take the
    workgroup-split path) and with the default 256 (no row is long);
  * Cora's hop1_sym / hop2_sym from tests/golden/cora_operands.npz;
  * x and grad drawn from U(-1, 1).

Accuracy is judged against fp64 with the bound that holds for ANY order of a d-term fp32 dot product,
    |dV - exact| <= gamma_d * sum_c |g_c x_c| + d * 2^-149,   gamma_d = d*u / (1 - d*u),  u = 2^-24
(nothing measured); everything else is torch.equal: the bits are a function of d alone (include/h2gcn_hip.h).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_planetoid_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 130)
N_ROWS, N_COLS = 41, 200
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 100, 128, 130, 256, 260, 516)


def gamma(n):
    return n * U / (1.0 - n * U)


def _crafted_hops():
    rng = np.random.default_rng(11)
    mats = []
    for k in range(3):
        indptr, indices = [0], []
        for i in range(N_ROWS):
            n = LENGTHS[(i + 3 * k) % len(LENGTHS)]
            indices.extend(np.sort(rng.choice(N_COLS, size=n, replace=False)).tolist())
            indptr.append(len(indices))
        data = rng.uniform(-1, 1, len(indices)).astype(np.float32)
        data[::7] = 0.0                                   # stored entries whose value is an explicit zero: the pattern decides
        mats.append(sp.csr_matrix((data, np.asarray(indices, np.int32), np.asarray(indptr, np.int64)), shape=(N_ROWS, N_COLS)))
    return mats


@pytest.fixture(scope="module")
def crafted():
    return _crafted_hops()


@pytest.fixture(scope="module")
def cora():
    g = load_planetoid_golden("cora")
    return [sp.csr_matrix(g["hop1_sym"]), sp.csr_matrix(g["hop2_sym"])]


_PLANS = {}


def plan_of(name, mats, **kw):
    """Plans are shared among the tests of this module (building one costs a few device round trips)."""
    from h2gcn_amd import HopPlan

    key = (name, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = HopPlan.from_scipy(mats, DEV, **kw)
    return _PLANS[key]


_DATA = {}


def operands(name, mats, d, dtype=torch.float32):
    """(grad, x) for an operand set and width, and their fp64 reference, computed once: exact[s], abssum[s] per hop."""
    key = (name, d, dtype)
    if key not in _DATA:
        n_rows, n_cols = mats[0].shape
        gen = torch.Generator().manual_seed(1000 + d)
        g = (torch.rand((n_rows, len(mats), d), generator=gen) * 2 - 1).to(DEV).to(dtype)
        x = (torch.rand((n_cols, d), generator=gen) * 2 - 1).to(DEV).to(dtype)
        g64, x64 = g.double(), x.double()                # (bf16: the exactly widened values)
        exact, abssum = [], []
        for s, m in enumerate(mats):
            rows = torch.from_numpy(np.repeat(np.arange(n_rows), np.diff(m.indptr))).to(DEV)
            cols = torch.from_numpy(m.indices.astype(np.int64)).to(DEV)
            e, a = [], []
            for lo in range(0, rows.numel(), 1 << 16):   # chunked: Cora's hop 2 at d = 128 would be 88 MB per product
                r, c = rows[lo:lo + (1 << 16)], cols[lo:lo + (1 << 16)]
                prod = g64[r, s, :] * x64[c, :]
                e.append(prod.sum(-1))
                a.append(prod.abs().sum(-1))
            exact.append(torch.cat(e) if e else torch.zeros(0, dtype=torch.float64, device=DEV))
            abssum.append(torch.cat(a) if a else torch.zeros(0, dtype=torch.float64, device=DEV))
        _DATA[key] = (g, x, exact, abssum)
    return _DATA[key]


def assert_within_bound(got, exact, abssum, d, what):
    for s, (v, e, a) in enumerate(zip(got, exact, abssum)):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.shape == e.shape
        err = (v.double() - e).abs()
        bound = gamma(d) * a + d * 2.0 ** -149
        worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"{what} hop {s}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (what, s, worst)


# ------------------------------------------------------------------ 1. accuracy against fp64
@pytest.mark.parametrize("d", WIDTHS)
def test_accuracy_crafted(crafted, d):
    for thr in (32, 0):
        plan = plan_of("crafted", crafted, long_row_threshold=thr)
        if thr == 32:
            assert plan.info(0)["n_long_segments"] > 0     # the 63+ rows take the workgroup-split path
        else:
            assert all(plan.info(k)["n_long_segments"] == 0 for k in range(3))
        g, x, exact, abssum = operands("crafted", crafted, d)
        assert_within_bound(plan.sddmm(g, x), exact, abssum, d, f"crafted fp32 d={d} thr={thr}")
        if d % 2 == 0:
            gb, xb, exact_b, abssum_b = operands("crafted", crafted, d, torch.bfloat16)
            assert_within_bound(plan.sddmm(gb, xb), exact_b, abssum_b, d, f"crafted bf16 d={d} thr={thr}")


@pytest.mark.parametrize("d", (64, 128))
def test_accuracy_cora(cora, d):
    plan = plan_of("cora", cora)
    g, x, exact, abssum = operands("cora", cora, d)
    assert_within_bound(plan.sddmm(g, x), exact, abssum, d, f"cora fp32 d={d}")
    gb, xb, exact_b, abssum_b = operands("cora", cora, d, torch.bfloat16)
    assert_within_bound(plan.sddmm(gb, xb), exact_b, abssum_b, d, f"cora bf16 d={d}")


# ------------------------------------------------------------------ 2. / 4. the bits depend on d only
BIT_WIDTHS = (5, 64, 100, 130, 260, 516)
TUNABLES = (dict(long_row_threshold=256), dict(long_row_threshold=32, rows_per_wave=1), dict(long_row_threshold=32, rows_per_wave=7),
            dict(long_row_threshold=32, slice_cols=64), dict(long_row_threshold=32, slice_cols=128),
            dict(long_row_threshold=256, slice_cols=256))


def equal_lists(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("build_transpose", (True, False))
def test_bits_do_not_depend_on_plan_tunables(crafted, cora, build_transpose):
    """(build_transpose=False: the launch needs no transposed operand -- forward arrays only)"""
    for name, mats, widths in (("crafted", crafted, BIT_WIDTHS), ("cora", cora, (64,))):
        base = plan_of(name, mats, long_row_threshold=32)
        for d in widths:
            g, x, _, _ = operands(name, mats, d)
            want = base.sddmm(g, x)
            for kw in TUNABLES:
                got = plan_of(name, mats, build_transpose=build_transpose, **kw).sddmm(g, x)
                assert equal_lists(got, want), (name, d, kw)


def test_bits_hop_alone_vs_all_hops(crafted):
    plan = plan_of("crafted", crafted, long_row_threshold=32)
    for d in BIT_WIDTHS:
        g, x, _, _ = operands("crafted", crafted, d)
        want = plan.sddmm(g, x)
        for k in range(3):
            assert torch.equal(plan.sddmm(g[:, k:k + 1, :], x, hops=[k])[0], want[k]), (d, k)
        got = plan.sddmm(g[:, ::2, :], x, hops=[0, 2])   # a strided hop view: slots 0 and 2 of the stacked gradient
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[2]), d


def test_bits_row_selected_sub_plan(crafted):
    plan = plan_of("crafted", crafted, long_row_threshold=32)
    rows = [0, 3, 6, 7, 8, 9, 17, 18, 29, 40]
    sel = plan.select_rows(rows, build_transpose=False)
    assert sel.plan.n_rows == len(rows) and sel.plan.n_cols == N_COLS    # n_rows != n_cols
    for d in (5, 130, 260):
        g, x, _, _ = operands("crafted", crafted, d)
        want = plan.sddmm(g, x)
        got = sel.plan.sddmm(g[sel.rows_long], x)
        for s, m in enumerate(crafted):
            entries = np.concatenate([np.arange(m.indptr[r], m.indptr[r + 1]) for r in rows])
            assert torch.equal(got[s], want[s][torch.from_numpy(entries).to(DEV)]), (d, s)


def test_bits_strided_operands_and_repeated_launches(crafted):
    plan = plan_of("crafted", crafted, long_row_threshold=32)
    for d in (5, 64, 130, 260):
        g, x, _, _ = operands("crafted", crafted, d)
        want = plan.sddmm(g, x)
        assert equal_lists(plan.sddmm(g, x), want), d                    # two launches in a row
        wide = torch.full((N_COLS, d + 37), float("nan"), device=DEV)    # x as a column slot of a wider buffer
        wide[:, 9:9 + d] = x
        xs = wide[:, 9:9 + d]
        gwide = torch.full((N_ROWS, 3 * d + 11), float("nan"), device=DEV)   # grad as a [N, H, d] view with ldg_row > H * d
        gs = gwide[:, :3 * d].view(N_ROWS, 3, d)
        gs.copy_(g)
        assert xs.stride(0) == d + 37 and gs.stride(0) == 3 * d + 11 and not gs.is_contiguous()
        assert equal_lists(plan.sddmm(gs, xs), want), d
        out = [torch.full_like(w, float("nan")) for w in want]           # out=: overwritten, not accumulated into
        res = plan.sddmm(gs, xs, out=out)
        assert all(r is o for r, o in zip(res, out)) and equal_lists(out, want), d


# ------------------------------------------------------------------ 3. bf16
def test_bf16_is_the_fp32_launch_on_the_widened_operands(crafted, cora):
    for name, mats, widths, kw in (("crafted", crafted, (2, 4, 64, 100, 130, 256, 260, 516), dict(long_row_threshold=32)),
                                   ("cora", cora, (64, 128), {})):
        plan = plan_of(name, mats, **kw)
        for d in widths:
            gb, xb, _, _ = operands(name, mats, d, torch.bfloat16)
            assert equal_lists(plan.sddmm(gb, xb), plan.sddmm(gb.float(), xb.float())), (name, d)


def test_bf16_layout_and_mixed_dtypes_are_refused_before_any_launch(crafted, monkeypatch):
    from h2gcn_amd import _capi

    plan = plan_of("crafted", crafted, long_row_threshold=32)
    L = _capi.lib()
    calls = []
    real = {n: getattr(L, n) for n in ("h2gcn_sddmm_hops_f32", "h2gcn_sddmm_hops_bf16")}
    for n in real:
        monkeypatch.setattr(L, n, lambda *a, _n=n: calls.append(_n) or real[_n](*a))
    g = torch.zeros((N_ROWS, 3, 6), device=DEV, dtype=torch.bfloat16)
    x = torch.zeros((N_COLS, 6), device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="same dtype"):
        plan.sddmm(g.float(), x)
    with pytest.raises(ValueError, match="same dtype"):
        plan.sddmm(g, x.float())
    with pytest.raises(ValueError, match="must be even"):                 # odd d
        plan.sddmm(g[:, :, :5], x[:, :5].contiguous())
    with pytest.raises(ValueError, match="strides must be even"):         # odd row stride of x
        plan.sddmm(g, torch.zeros((N_COLS, 7), device=DEV, dtype=torch.bfloat16)[:, :6])
    with pytest.raises(ValueError, match="strides must be even"):         # odd row stride of grad
        plan.sddmm(torch.zeros((N_ROWS, 19), device=DEV, dtype=torch.bfloat16)[:, :18].view(N_ROWS, 3, 6), x)
    assert calls == []
    plan.sddmm(g, x)
    assert calls == ["h2gcn_sddmm_hops_bf16"]


# ------------------------------------------------------------------ 5. hipGraph
def test_hipgraph_replay_equals_eager(crafted):
    plan = plan_of("crafted", crafted, long_row_threshold=32)
    d = 130
    g, x, _, _ = operands("crafted", crafted, d)
    g_static, x_static = g.clone(), x.clone()
    out = [torch.empty(n, device=DEV) for n in plan.nnz]
    first = [t.clone() for t in plan.sddmm(g_static, x_static, out=out)]   # one eager all-hops launch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.sddmm(g_static, x_static, out=out)
    g2, x2, _, _ = operands("crafted", crafted, 260)
    g_static.copy_(g2[:, :, 7:7 + d])                                       # fresh contents of the static inputs
    x_static.copy_(x2[:, 3:3 + d])
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want = plan.sddmm(g_static.clone(), x_static.clone())
    assert equal_lists(out, want) and not equal_lists(out, first)


# ------------------------------------------------------------------ 6. autograd against a dense fp64 replica
def _dense64(m, vals64):
    rows = torch.from_numpy(np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))).to(DEV)
    cols = torch.from_numpy(m.indices.astype(np.int64)).to(DEV)
    a = torch.zeros(m.shape, dtype=torch.float64, device=DEV)
    return a.index_put((rows, cols), vals64), rows, cols


@pytest.mark.parametrize("symmetric", (False, True))
def test_autograd_against_dense_fp64_replica(cora, symmetric):
    from h2gcn_amd import GCNLayer, HopPlan
    from h2gcn_amd.layers import hop_spmm

    d = 64
    n = cora[0].shape[0]
    plan = HopPlan.from_scipy(cora, DEV, build_transpose=True, keep_permutation=True, symmetric_pattern=symmetric)
    assert plan.keep_permutation
    gen = torch.Generator().manual_seed(6)
    x0 = (torch.rand((n, d), generator=gen) * 2 - 1).to(DEV)
    R = (torch.rand((n, 2, d), generator=gen) * 2 - 1).to(DEV)
    # the longest row of the adjoint's operand [A_1; A_2]^T: the number of terms behind one element of d inputs
    L = int(sum(np.bincount(m.indices, minlength=n) for m in cora).max())
    for scale, layer in ((1.0, False), (2.0, True)):     # 2 x values: a stale transposed operand would give half the gradient
        values = [(scale * torch.from_numpy(m.data).to(DEV)).requires_grad_(True) for m in cora]
        x = x0.clone().requires_grad_(True)
        y = GCNLayer()(plan, x, values=values) if layer else hop_spmm(plan, x, None, values)
        (y * R).sum().backward()
        # the replica: dense fp64 matrices built from fp64 leaves, torch's own autograd
        v64 = [v.detach().double().requires_grad_(True) for v in values]
        x64 = x0.double().requires_grad_(True)
        dense = [_dense64(m, v) for m, v in zip(cora, v64)]
        y64 = torch.stack([a @ x64 for a, _, _ in dense], dim=1)
        (y64 * R.double()).sum().backward()
        assert float((y.detach().double() - y64.detach()).abs().max()) < 1e-4
        for k, (a, rows, cols) in enumerate(dense):
            abssum = (R.double()[rows, k, :].abs() * x0.double()[cols, :].abs()).sum(-1)
            err = (values[k].grad.double() - v64[k].grad).abs()
            bound = gamma(d) * abssum + d * 2.0 ** -149
            print(f"values[{k}].grad scale {scale}: worst err / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (scale, k)
        absdx = sum(a.detach().abs().t() @ R.double()[:, k, :].abs() for k, (a, _, _) in enumerate(dense))
        err = (x.grad.double() - x64.grad).abs()
        bound = gamma(L) * absdx + L * 2.0 ** -149
        print(f"inputs.grad scale {scale}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), scale


def test_autograd_selects_only_the_hops_that_want_a_gradient(cora):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_spmm

    d = 64
    plan = HopPlan.from_scipy(cora, DEV)
    g, x, exact, abssum = operands("cora", cora, d)
    v1 = torch.from_numpy(cora[1].data).to(DEV).requires_grad_(True)
    seen = []
    real = plan.sddmm
    plan.sddmm = lambda grad, xx, hops=None, out=None: seen.append(tuple(hops)) or real(grad, xx, hops=hops, out=out)
    y = hop_spmm(plan, x, values=[None, v1])
    (y * g).sum().backward()
    assert seen == [(1,)]
    assert_within_bound([v1.grad], exact[1:], abssum[1:], d, "hop 1 alone through autograd")


# ------------------------------------------------------------------ 7. one exact line-search step
def test_one_exact_line_search_step_lowers_the_loss(cora):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_spmm

    d = 64
    n = cora[0].shape[0]
    plan = HopPlan.from_scipy(cora, DEV)
    gen = torch.Generator().manual_seed(7)
    x = (torch.rand((n, d), generator=gen) * 2 - 1).to(DEV)
    golden = [torch.from_numpy(m.data).to(DEV) for m in cora]
    T = plan.spmm(x).double()

    def f(values):
        return 0.5 * ((hop_spmm(plan, x, values=values).double() - T) ** 2).sum()

    v = [(0.5 * w).requires_grad_(True) for w in golden]
    f0 = f(v)
    grads = torch.autograd.grad(f0, v)
    D = hop_spmm(plan, x, values=[gk.float().contiguous() for gk in grads]).double()
    g2 = float(sum((gk.double() ** 2).sum() for gk in grads))
    D2 = float((D ** 2).sum())
    eta = g2 / D2
    f1 = f([(vk.detach() - eta * gk).contiguous() for vk, gk in zip(v, grads)])
    drop = g2 * g2 / (2.0 * D2)          # what the step gains in exact arithmetic (f is quadratic in v)
    print(f"f0 {float(f0.detach()):.6e}  f1 {float(f1.detach()):.6e}  exact drop {drop:.6e}  eta {eta:.4e}")
    assert drop > 0 and float(f1.detach()) <= float(f0.detach()) - 0.5 * drop


# ------------------------------------------------------------------ 8. refusals
def test_refusals(cora):
    from h2gcn_amd import GCNLayer, HopPlan
    from h2gcn_amd.layers import hop_spmm

    d = 64
    n = cora[0].shape[0]
    x = torch.rand((n, d), device=DEV)
    vals = [torch.from_numpy(m.data).to(DEV) for m in cora]

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_spmm(Sharded(), x, values=vals)
    with pytest.raises(ValueError, match="row-partitioned"):
        GCNLayer()(Sharded(), x, values=vals)

    no_perm = HopPlan.from_scipy(cora, DEV, build_transpose=True)
    assert not no_perm.keep_permutation
    with pytest.raises(ValueError, match="keep_permutation=True"):
        hop_spmm(no_perm, x.clone().requires_grad_(True), values=vals)

    plan = HopPlan.from_scipy(cora, DEV, build_transpose=True, keep_permutation=True)
    with pytest.raises(ValueError, match=r"values\[1\] must be a float32"):
        hop_spmm(plan, x, values=[vals[0], vals[1][:-1]])
    with pytest.raises(ValueError, match=r"values\[0\] must be a float32"):
        hop_spmm(plan, x, values=[vals[0].double(), None])
    with pytest.raises(ValueError, match=r"values\[0\] must be a float32"):
        hop_spmm(plan, x, values=[vals[0].cpu(), None])
    with pytest.raises(ValueError, match="one entry per hop"):
        hop_spmm(plan, x, values=vals[:1])

    leaf = [v.clone().requires_grad_(True) for v in vals]
    y = hop_spmm(plan, x, values=leaf)
    plan.set_values(0, vals[0].clone())                   # someone changes the plan's values before the backward
    with pytest.raises(RuntimeError, match="values changed between the forward and the backward"):
        y.sum().backward()
