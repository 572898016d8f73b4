"""GPU suite: the dynamic (GATv2) edge scores (h2gcn_amd/csrc/edge_scores_dynamic.hip; HopPlan.edge_scores_dynamic /
edge_scores_dynamic_backward, layers.hop_edge_scores_dynamic, layers.DynamicHopAttention).

Operands: those of test_spmm_values_gpu (48 x 1100 with segment lengths 0 .. 1025, its adjoint form, the 600-node square graph),
plans with long_row_threshold 32 / 256 / 1024 paired with rows_per_wave 1 / 3 / 7, the (d, K) grid of test_attention_bf16_gpu.  Inputs
are uniform in (-1, 1) without exact zeros.  The raw calls write into NaN-prefilled views with guard elements on either side and are
made twice.  The fp64 target is tests/edge_scores_dynamic_ref.py; every bound is the one include/h2gcn_hip.h states."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import edge_scores_dynamic_ref as ref
import test_spmm_values_gpu as values_gpu
from test_attention_bf16_gpu import BACKWARD_GRID
from test_spmm_values_gpu import DEV, THRESHOLDS, bits, make_plan, strided_rows

pytestmark = pytest.mark.gpu

GRID = BACKWARD_GRID                          # nine points: packed w = 4, 8, 16, 32 (five, one pass each); head-aligned w = 96 (192, 2) and
#                                               w = 64 (256, 4); K = 1 with d = 22, 100.  Every geometry: test_edge_scores_dynamic_sweep_gpu
KNOBS = tuple(zip(THRESHOLDS, (1, 3, 7)))     # (long_row_threshold, rows_per_wave)
G = 8                                         # guard elements
KINDS = {"forward": values_gpu.forward_hops, "adjoint": values_gpu.adjoint_hops, "square": values_gpu.square_hops}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def uniform(rng, shape):
    """uniform in (-1, 1) without exact zeros"""
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    a[a == 0] = 0.5
    return a


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(kind, d, n_heads):
    """hops and host arrays u [n_rows, d], v [n_cols, d], a [2, d], ds (per hop [nnz, K])"""
    hops = KINDS[kind]()
    rng = np.random.default_rng(1000 * d + n_heads + len(kind))
    n_rows, n_cols = hops[0].shape
    return hops, uniform(rng, (n_rows, d)), uniform(rng, (n_cols, d)), uniform(rng, (len(hops), d)), tuple(uniform(rng, (m.nnz, n_heads)) for m in hops)


def plan_of(hops, thr=256, rpw=3, **kw):
    kw.setdefault("build_transpose", True)
    kw.setdefault("keep_permutation", True)
    return make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw, **kw)


def per_entry(t, n_heads):
    """a per-entry device array in the layout of the call: [nnz, K], K = 1: [nnz]"""
    t = t if isinstance(t, torch.Tensor) else dev(t)
    return t.reshape(-1) if n_heads == 1 else t.reshape(-1, n_heads)


def raw_scores(plan, u, v, a, n_heads, slope=0.2, hops=None, where=""):
    """h2gcn_edge_scores_dynamic_hops_f32 into guarded NaN-filled arrays, twice -> one tensor per selected hop"""
    from h2gcn_amd import _capi

    mask, sel = plan._mask(hops), plan._selected(hops)
    d = u.shape[1]
    rounds = []
    for _ in range(2):
        bufs = [torch.full((plan.colidx[k].numel() * n_heads + 2 * G,), float("nan"), device=DEV) for k in sel]
        views = [b[G:b.numel() - G] for b in bufs]
        tbl = (C.c_void_p * len(sel))(*[t.data_ptr() if t.numel() else None for t in views])
        _capi.check(_capi.lib().h2gcn_edge_scores_dynamic_hops_f32(plan._handle, mask, _ptr(u), u.stride(0), _ptr(v), v.stride(0), _ptr(a), a.stride(0), d,
                                                                   n_heads, slope, tbl, None))
        torch.cuda.synchronize()
        for b in bufs:
            assert bool(torch.isnan(b[:G]).all()) and bool(torch.isnan(b[b.numel() - G:]).all()), f"{where}: a guard element was written"
        rounds.append([per_entry(t, n_heads) for t in views])
    for x, y in zip(*rounds):
        assert same(x, y), f"{where}: the second launch differs from the first"
    return rounds[0]


def raw_backward(plan, u, v, a, n_heads, ds, needs=(True, True, True), slope=0.2, hops=None, where=""):
    """h2gcn_edge_scores_dynamic_backward_hops_f32 with du, dv, da as guarded NaN-filled views and a 0xFF-filled workspace between guard
    bytes, twice -> (du, dv, da), None where not asked for"""
    from h2gcn_amd import _capi

    L = _capi.lib()
    mask, sel = plan._mask(hops), plan._selected(hops)
    d = u.shape[1]
    tbl = (C.c_void_p * len(sel))(*[t.data_ptr() if t.numel() else None for t in ds])
    nbytes = int(L.h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, mask, d))
    assert nbytes > 0 or plan.n_rows == 0
    rounds = []
    for _ in range(2):
        outs, bufs = [], []
        for need, n in zip(needs, (plan.n_rows, plan.n_cols, len(sel))):
            buf = torch.full((n, d + 2 * G), float("nan"), device=DEV) if need else None
            bufs.append(buf)
            outs.append(buf[:, G:G + d] if need else None)
        ws = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        args = []
        for t in outs:
            args += [_ptr(t), d + 2 * G]
        _capi.check(L.h2gcn_edge_scores_dynamic_backward_hops_f32(plan._handle, mask, _ptr(u), u.stride(0), _ptr(v), v.stride(0), _ptr(a), a.stride(0),
                                                                  d, n_heads, slope, tbl, *args, C.c_void_p(ws.data_ptr() + 32) if needs[2] else None,
                                                                  nbytes if needs[2] else 0, None))
        torch.cuda.synchronize()
        for b in bufs:
            if b is not None:
                assert bool(torch.isnan(b[:, :G]).all()) and bool(torch.isnan(b[:, G + d:]).all()), f"{where}: a guard column was written"
        assert bool((ws[:32] == 0xFF).all()) and bool((ws[32 + nbytes:] == 0xFF).all()), f"{where}: written outside the workspace"
        rounds.append(outs)
    for x, y in zip(*rounds):
        assert (x is None and y is None) or same(x, y), f"{where}: the second call differs from the first"
    return tuple(rounds[0])


# ------------------------------------------------------------------ 1. the bits of the existing kernel
@pytest.mark.parametrize("d,n_heads", GRID)
def test_scores_with_u_zero_have_the_bits_of_the_sddmm(d, n_heads):
    hops, _, v, a, _ = case("forward", d, n_heads)
    n_rows = hops[0].shape[0]
    for thr, rpw in KNOBS:
        plan = plan_of(hops, thr, rpw)
        got = raw_scores(plan, torch.zeros((n_rows, d), device=DEV), dev(v), dev(a), n_heads, where=f"thr {thr}")
        grad = dev(a)[None].expand(n_rows, len(hops), d).contiguous()
        x = torch.nn.functional.leaky_relu(dev(v), 0.2)
        want = plan.sddmm(grad, x) if n_heads == 1 else plan.sddmm_heads(grad, x, n_heads)
        for s in range(len(hops)):
            assert same(got[s], want[s]), f"hop {s}, thr {thr}: the order of summation is not the SDDMM's"


# ------------------------------------------------------------------ 2. forward against fp64
@pytest.mark.parametrize("d,n_heads", GRID)
def test_scores_against_fp64(d, n_heads):
    """Worst error-to-bound ratios: DESIGN.md ("Dynamic attention")."""
    hops, u, v, a, _ = case("forward", d, n_heads)
    want = ref.Reference(hops, u, v, a, n_heads, 0.2)
    got = raw_scores(plan_of(hops), dev(u), dev(v), dev(a), n_heads)
    for s in range(len(hops)):
        err = np.abs(got[s].cpu().numpy().astype(np.float64).reshape(-1, n_heads) - want.scores[s])
        bound = want.score_bound(s)
        print(f"d {d} K {n_heads} hop {s}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), f"hop {s}: {int((err > bound).sum())} scores beyond gamma_(w+2) * sum|a q| + (w+2) * 2^-149"


# ------------------------------------------------------------------ 3. forward invariance
@pytest.mark.parametrize("d,n_heads", GRID)
def test_scores_do_not_depend_on_knobs_selection_or_strides(d, n_heads):
    hops, u, v, a, _ = case("forward", d, n_heads)
    for slope in (0.2, 0.0, 1.0):
        base = raw_scores(plan_of(hops), dev(u), dev(v), dev(a), n_heads, slope)
        for thr, rpw in KNOBS:
            plan = plan_of(hops, thr, rpw)
            got = raw_scores(plan, dev(u), dev(v), dev(a), n_heads, slope, where=f"thr {thr} rpw {rpw}")
            assert all(same(x, y) for x, y in zip(got, base)), f"slope {slope}: thr {thr} rpw {rpw} changes the bits"
            for sel in ([0], [1], [0, 1]):
                got = raw_scores(plan, dev(u), dev(v), dev(a[sel]), n_heads, slope, hops=sel)
                assert all(same(x, base[k]) for x, k in zip(got, sel)), f"slope {slope}: the selection {sel} changes the bits"
        got = raw_scores(plan_of(hops), strided_rows(u), strided_rows(v, 8), strided_rows(a, 12), n_heads, slope)
        assert all(same(x, y) for x, y in zip(got, base)), f"slope {slope}: strided operands change the bits"
        meth = plan_of(hops).edge_scores_dynamic(dev(u), dev(v), dev(a).view(len(hops), n_heads, -1), n_heads, slope)
        assert all(same(x, y) for x, y in zip(meth, base)), "the method differs from the raw call"


# ------------------------------------------------------------------ 4. backward against fp64
@functools.lru_cache(maxsize=None)
def backward_reference(kind, d, n_heads):
    hops, u, v, a, ds = case(kind, d, n_heads)
    return ref.Reference(hops, u, v, a, n_heads, 0.2, ds=ds)


@pytest.mark.parametrize("d,n_heads", GRID)
@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_against_fp64(kind, d, n_heads):
    """Worst error-to-bound ratios: DESIGN.md ("Dynamic attention")."""
    hops, u, v, a, ds = case(kind, d, n_heads)
    want = backward_reference(kind, d, n_heads)
    plan = plan_of(hops)
    du, dv, da = raw_backward(plan, dev(u), dev(v), dev(a), n_heads, [per_entry(t, n_heads) for t in ds], where=kind)
    for name, got, exact, bound in (("du", du, want.du, want.du_bound()), ("dv", dv, want.dv, want.dv_bound()), ("da", da, want.da, want.da_bound())):
        err = np.abs(got.cpu().numpy().astype(np.float64) - exact)
        print(f"{kind} d {d} K {n_heads} {name}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements beyond the bound of include/h2gcn_hip.h"
    for x, y in zip((du, dv, da), plan.edge_scores_dynamic_backward(dev(u), dev(v), dev(a), [per_entry(t, n_heads) for t in ds], n_heads)):
        assert same(x, y), "the method differs from the raw call"


# ------------------------------------------------------------------ 5. backward invariance
@pytest.mark.parametrize("d,n_heads", [(64, 8), (22, 1), (192, 2), (256, 4)])
def test_backward_need_flags_and_rows_per_wave(d, n_heads):
    for kind in ("forward", "adjoint"):
        hops, u, v, a, ds = case(kind, d, n_heads)
        ops = (dev(u), dev(v), dev(a), n_heads, [per_entry(t, n_heads) for t in ds])
        for thr in THRESHOLDS:
            full = raw_backward(plan_of(hops, thr, 3), *ops)
            for rpw in (1, 7):
                du, dv, _ = raw_backward(plan_of(hops, thr, rpw), *ops)
                assert same(du, full[0]) and same(dv, full[1]), f"{kind} thr {thr}: rows_per_wave {rpw} changes du / dv"
        plan = plan_of(hops)
        full = raw_backward(plan, *ops)
        for needs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            got = raw_backward(plan, *ops, needs=tuple(bool(x) for x in needs))
            for need, x, y in zip(needs, got, full):
                assert (x is None) if not need else same(x, y), f"{kind}: the need flags {needs} change the bits"
        du = raw_backward(make_plan(hops, long_row_threshold=256, rows_per_wave=3), *ops, needs=(True, False, True))   # (no transposes)
        assert same(du[0], full[0]) and same(du[2], full[2])


def test_dv_on_a_symmetric_plan_equals_built_transposes():
    d, n_heads = 64, 8
    hops, u, v, a, ds = case("square", d, n_heads)
    ops = (dev(u), dev(v), dev(a), n_heads, [per_entry(t, n_heads) for t in ds])
    for thr in (32, 1024):
        sym = make_plan(hops, build_transpose=True, keep_permutation=True, symmetric_pattern=True, long_row_threshold=thr)
        assert sym.transpose_sharing[0] != "none"
        want = raw_backward(plan_of(hops, thr, 0), *ops)
        got = raw_backward(sym, *ops)
        assert all(same(x, y) for x, y in zip(got, want)), f"thr {thr}: the symmetric plan differs"


# ------------------------------------------------------------------ 6. edges
def test_empty_segments_and_an_empty_hop():
    import scipy.sparse as sp

    d, n_heads = 48, 3
    hops, u, v, a, ds = case("forward", d, n_heads)
    want = ref.Reference(hops, u, v, a[:1], n_heads, 0.2, ds=ds[:1], sel=[0])     # (every row has entries in one hop or the other)
    du, dv, _ = raw_backward(plan_of(hops), dev(u), dev(v), dev(a[:1]), n_heads, [per_entry(ds[0], n_heads)], hops=[0])
    assert (want.n_du == 0).any() and (want.n_dv == 0).any()
    assert bool((bits(du)[torch.from_numpy(want.n_du == 0)] == 0).all()), "a row without entries must give +0"
    assert bool((bits(dv)[torch.from_numpy(want.n_dv == 0)] == 0).all()), "a column without entries must give +0"
    # a hop without nonzeros beside one with
    mixed = (hops[0], sp.csr_matrix(hops[0].shape, dtype=np.float32))
    plan = make_plan(mixed, build_transpose=True, keep_permutation=True, long_row_threshold=256, rows_per_wave=3)
    gs = [per_entry(ds[0], n_heads), torch.empty((0, n_heads), device=DEV)]
    du1, dv1, da1 = raw_backward(plan, dev(u), dev(v), dev(a), n_heads, gs)
    alone = raw_backward(plan_of(hops), dev(u), dev(v), dev(a[:1]), n_heads, gs[:1], hops=[0])
    assert same(du1, alone[0]) and same(dv1, alone[1]) and same(da1[:1], alone[2]) and bool((bits(da1[1]) == 0).all())
    sc = raw_scores(plan, dev(u), dev(v), dev(a), n_heads)
    assert sc[1].numel() == 0 and same(sc[0], raw_scores(plan_of(hops), dev(u), dev(v), dev(a), n_heads)[0])
    # a selection without nonzeros: the outputs are zeroed, the guards intact
    for got in raw_backward(plan, dev(u), dev(v), dev(a[1:]), n_heads, gs[1:], hops=[1]):
        assert bool((bits(got) == 0).all())
    assert raw_scores(plan, dev(u), dev(v), dev(a[1:]), n_heads, hops=[1])[0].numel() == 0


@pytest.mark.parametrize("d,n_heads", [(128, 8), (100, 1)])
def test_one_row_plan_and_all_long_segments(d, n_heads):
    rng = np.random.default_rng(d)
    one = tuple(values_gpu.drv.hop_from_lengths([n], 400, seed=3 + n) for n in (300, 77))
    long_ = tuple(values_gpu.drv.hop_from_lengths([40 + (i % 5) for i in range(24)], 90, seed=9 + k) for k in range(2))
    for name, hops, thr in (("one row", one, 256), ("one row", one, 32), ("all long", long_, 32)):
        n_rows, n_cols = hops[0].shape
        u, v, a = uniform(rng, (n_rows, d)), uniform(rng, (n_cols, d)), uniform(rng, (2, d))
        ds = [uniform(rng, (m.nnz, n_heads)) for m in hops]
        want = ref.Reference(hops, u, v, a, n_heads, 0.2, ds=ds)
        plan = make_plan(hops, build_transpose=True, keep_permutation=True, long_row_threshold=thr)
        sc = raw_scores(plan, dev(u), dev(v), dev(a), n_heads, where=name)
        for s in range(2):
            assert (np.abs(sc[s].cpu().numpy().astype(np.float64).reshape(-1, n_heads) - want.scores[s]) <= want.score_bound(s)).all(), name
        got = raw_backward(plan, dev(u), dev(v), dev(a), n_heads, [per_entry(t, n_heads) for t in ds], where=name)
        for x, exact, bound in zip(got, (want.du, want.dv, want.da), (want.du_bound(), want.dv_bound(), want.da_bound())):
            assert (np.abs(x.cpu().numpy().astype(np.float64) - exact) <= bound).all(), name


# ------------------------------------------------------------------ 7. special values
def same_nan_aware(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    return got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and \
        torch.equal(bits(torch.nan_to_num(got, nan=0.0)), bits(torch.nan_to_num(want, nan=0.0)))


@pytest.mark.parametrize("side", ["v", "u"])
def test_special_values_stay_in_their_node_and_head(side):
    d, n_heads = 64, 8
    w = d // n_heads
    hops, u, v, a, ds = case("square", d, n_heads)
    plan = plan_of(hops)
    gs = [per_entry(t, n_heads) for t in ds]
    base_sc = raw_scores(plan, dev(u), dev(v), dev(a), n_heads)
    base = raw_backward(plan, dev(u), dev(v), dev(a), n_heads, gs)
    node, head = 123, 5
    specials = (np.nan, np.inf, -np.inf, 1e-40, 1e38)
    u2, v2 = u.copy(), v.copy()
    (v2 if side == "v" else u2)[node, head * w:head * w + len(specials)] = specials
    sc = raw_scores(plan, dev(u2), dev(v2), dev(a), n_heads)
    du, dv, _ = raw_backward(plan, dev(u2), dev(v2), dev(a), n_heads, gs)
    want = ref.Reference(hops, u2, v2, a, n_heads, 0.2, ds=ds)
    cols_hit = np.zeros(d, dtype=bool)
    cols_hit[head * w:head * w + len(specials)] = True
    touched_rows, touched_cols = np.zeros(hops[0].shape[0], dtype=bool), np.zeros(hops[0].shape[1], dtype=bool)
    for s, m in enumerate(hops):
        rows, cols = ref.entries(m)
        hit = (cols == node) if side == "v" else (rows == node)
        assert hit.any()
        touched_rows[rows[hit]] = True
        touched_cols[cols[hit]] = True
        keep = np.ones((m.nnz, n_heads), dtype=bool)
        keep[hit, head] = False
        keep = torch.from_numpy(keep)
        assert torch.equal(bits(sc[s])[keep], bits(base_sc[s])[keep]), f"hop {s}: a score outside the node's entries / head changed"
        got = sc[s].cpu().numpy()[~keep.numpy()]
        assert np.array_equal(np.isnan(got), np.isnan(want.scores[s][~keep.numpy()])), f"hop {s}: NaN positions differ from IEEE arithmetic"
        assert np.isnan(got).all()          # (a NaN column makes the head's sum NaN at every entry of the node)
    for name, got, b, touched in (("du", du, base[0], touched_rows), ("dv", dv, base[1], touched_cols)):
        keep = np.ones(got.shape, dtype=bool)
        keep[np.ix_(touched, cols_hit)] = False
        keep = torch.from_numpy(keep)
        assert torch.equal(bits(got)[keep], bits(b)[keep]), f"{name}: an element outside the touched segments / columns changed"
        exact = (want.du if name == "du" else want.dv)[~keep.numpy()]
        assert np.array_equal(np.isnan(got.cpu().numpy()[~keep.numpy()]), np.isnan(exact)), f"{name}: NaN positions differ from IEEE arithmetic"


# ------------------------------------------------------------------ 8. refusals of the library
def test_library_refusals_write_nothing():
    from h2gcn_amd import _capi

    L = _capi.lib()
    d, n_heads = 64, 8
    hops, u, v, a, ds = case("forward", d, n_heads)
    plan = plan_of(hops)
    bare = make_plan(hops, long_row_threshold=256, rows_per_wave=3)
    noperm = make_plan(hops, build_transpose=True, keep_permutation=False, long_row_threshold=256)
    big = 320
    ut, vt, at = (torch.full((t.shape[0], big), 0.5, device=DEV) for t in (u, v, a))
    sc = [torch.full((m.nnz * n_heads,), float("nan"), device=DEV) for m in hops]
    gs = [per_entry(t, n_heads) for t in ds]
    outs = [torch.full((n, big), float("nan"), device=DEV) for n in (plan.n_rows, plan.n_cols, 2)]
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=DEV)
    need = int(L.h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, 3, d))
    assert 0 < need <= ws.numel() and L.h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, 3, 260) == 0
    tbl = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])

    def fwd(p=plan, d=d, k=n_heads, u=ut, ldu=big, v=vt, ldv=big, a=at, lda=big, scores=sc):
        return L.h2gcn_edge_scores_dynamic_hops_f32(p._handle, 3, _ptr(u), ldu, _ptr(v), ldv, _ptr(a), lda, d, k, 0.2, tbl(scores) if scores else None, None)

    def bwd(p=plan, d=d, k=n_heads, u=ut, ldu=big, v=vt, ldv=big, a=at, lda=big, g=gs, du=outs[0], lddu=big, dv=outs[1], lddv=big, da=outs[2],
            ldda=big, w=ws, wb=None):
        return L.h2gcn_edge_scores_dynamic_backward_hops_f32(p._handle, 3, _ptr(u), ldu, _ptr(v), ldv, _ptr(a), lda, d, k, 0.2, tbl(g) if g else None,
                                                             _ptr(du), lddu, _ptr(dv), lddv, _ptr(da), ldda, _ptr(w), ws.numel() if wb is None else wb, None)

    def refused(st, status, *words):
        msg = L.h2gcn_last_error().decode()
        assert st == status, (st, msg)
        assert all(wd in msg for wd in words), msg

    inv = _capi.ERR_INVALID_ARGUMENT
    for call in (fwd, bwd):
        refused(call(d=260, k=1), inv, "d = 260", "256")
        refused(call(d=64, k=5), inv, "d = 64", "n_heads = 5")
        refused(call(d=12, k=2), inv, "head width", "6", "multiple of 4")
        refused(call(ldu=d - 1), inv, "ldu")
        refused(call(ldv=d - 1), inv, "ldv")
        refused(call(lda=d - 1), inv, "lda")
        refused(call(u=None), inv, "u is NULL")
        refused(call(v=None), inv, "v is NULL")
        refused(call(a=None), inv, "a is NULL")
        refused(call(k=0), inv, "n_heads")
    refused(fwd(scores=None), inv, "scores is NULL")
    refused(bwd(g=None), inv, "dscores is NULL")
    refused(bwd(lddu=d - 1), inv, "lddu")
    refused(bwd(lddv=d - 1), inv, "lddv")
    refused(bwd(ldda=d - 1), inv, "ldda")
    refused(bwd(du=None, dv=None, da=None), inv, "du, dv and da are all NULL")
    refused(bwd(w=None), inv, "workspace is NULL")
    refused(bwd(wb=need - 1), inv, "workspace_bytes", "h2gcn_edge_scores_dynamic_workspace_bytes")
    refused(bwd(p=bare), _capi.ERR_NO_TRANSPOSE)
    refused(bwd(p=noperm), inv, "H2GCN_PLAN_KEEP_PERMUTATION")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in sc + outs) and bool((ws == 0xFF).all()), "a refused call wrote something"
    assert bwd(p=bare, dv=None) == 0 and bwd(da=None, w=None, wb=0) == 0     # (what the refusals leave possible)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 9. autograd and the layer
@functools.lru_cache(maxsize=None)
def square_masks():
    out = []
    for m in values_gpu.square_hops():
        mask = torch.zeros(m.shape, dtype=torch.bool, device=DEV)
        rows, cols = ref.entries(m)
        mask[torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)] = True
        out.append(mask)
    return out


def dense_replica(layer, x, gy, dtype):
    """output and gradients (x, then the parameters in state_dict order) of sum(layer(x) * gy) by dense torch operations in `dtype`"""
    n, heads, w = x.shape[0], layer.heads, layer.in_dim // layer.heads
    params = [p.detach().to(dtype).requires_grad_(True) for p in layer.parameters()]
    named = dict(zip([k for k, _ in layer.named_parameters()], params))
    X = x.detach().to(dtype).requires_grad_(True)
    U = X @ named["W_l"]
    V = U if layer.share_weights else X @ named["W_r"]
    ys = []
    for s, mask in enumerate(square_masks()):
        q = torch.nn.functional.leaky_relu(U[:, None, :] + V[None, :, :], layer.negative_slope)
        sc = (q.view(n, n, heads, w) * named["a"][s][None, None]).sum(dim=3)
        sc = sc.masked_fill(~mask[:, :, None], float("-inf"))
        sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))
        alpha = torch.softmax(sc, dim=1) * mask[:, :, None].to(dtype)
        ys.append(torch.einsum("ijh,jhw->ihw", alpha, V.view(n, heads, w)).reshape(n, -1))
    y = torch.stack(ys, dim=1)
    (y * gy.to(dtype)).sum().backward()
    return [y.detach().double()] + [t.grad.double() for t in [X] + params]


def rel_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("in_dim,heads,share", [(32, 1, False), (128, 8, False), (128, 8, True)])
def test_layer_against_the_dense_fp64_replica(in_dim, heads, share):
    from h2gcn_amd import DynamicHopAttention

    hops = values_gpu.square_hops()
    n = hops[0].shape[0]
    plan = plan_of(hops)
    torch.manual_seed(in_dim + heads)
    layer = DynamicHopAttention(in_dim, heads, share_weights=share).to(DEV)
    x = dev(uniform(np.random.default_rng(5), (n, in_dim))).requires_grad_(True)
    gy = dev(uniform(np.random.default_rng(6), (n, 2, in_dim)))
    y = layer(plan, x)
    (y * gy).sum().backward()
    got = [y.detach(), x.grad] + [p.grad for p in layer.parameters()]
    want = dense_replica(layer, x, gy, torch.float64)
    dense32 = dense_replica(layer, x, gy, torch.float32)
    names = ["y", "dx"] + ["d" + k for k, _ in layer.named_parameters()]
    for name, g, w64, w32 in zip(names, got, want, dense32):
        err, err32 = rel_err(g, w64), rel_err(w32, w64)
        print(f"({in_dim}, {heads}, share {share}) {name}: err {err:.3e}  dense fp32 {err32:.3e}  ratio {err / err32:.2f}")
        assert err <= 4 * err32, f"{name}: relative error {err:.3e} beyond 4 x the dense fp32 replica's {err32:.3e}"


def test_two_stacked_layers_and_a_captured_training_step():
    from h2gcn_amd import DynamicHopAttention

    hops = values_gpu.square_hops()
    n, d = hops[0].shape[0], 32
    plan = plan_of(hops)
    torch.manual_seed(3)
    l1, l2 = DynamicHopAttention(d, 8).to(DEV), DynamicHopAttention(d, 1, hops=[1]).to(DEV)
    x = dev(uniform(np.random.default_rng(8), (n, d)))
    params = list(l1.parameters()) + list(l2.parameters())

    def step():
        for p in params:
            p.grad = None
        h = l1(plan, x).sum(dim=1)
        loss = (l2(plan, h) ** 2).sum()
        loss.backward()
        return loss

    eager_loss = step().detach().clone()
    eager = [p.grad.clone() for p in params]
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    for p in params:
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same(loss, eager_loss)
    for p, g in zip(params, eager):
        assert same(p.grad, g), "the replayed step differs from the eager one"


# ------------------------------------------------------------------ 10. no nnz x d array
def test_peak_memory_stays_far_below_an_nnz_by_d_array():
    from h2gcn_amd import hop_edge_scores_dynamic

    d, n_heads = 128, 8
    hops, u, v, a, ds = case("square", d, n_heads)
    plan = plan_of(hops)
    ut, vt, at = (dev(t).requires_grad_(True) for t in (u, v, a))
    gs = [per_entry(t, n_heads) for t in ds]
    for measured in (False, True):               # (the first round builds what a first launch builds)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        scores = hop_edge_scores_dynamic(plan, ut, vt, at, n_heads)
        torch.autograd.backward(scores, gs)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del scores
        ut.grad = vt.grad = at.grad = None
    composite = sum(m.nnz for m in hops) * d * 4
    print(f"peak above the live set {peak} bytes; an nnz x d array {composite} bytes; ratio {peak / composite:.4f}")
    assert peak < composite / 4
