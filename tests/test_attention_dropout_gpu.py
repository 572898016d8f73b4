"""GPU suite: dropout on the attention coefficients, drawn inside the kernels (h2gcn_amd/csrc/attention_dropout.hip,
attention_dropout_backward.hip): the factor kernel against the numpy restatement of the generator (attention_dropout_ref.py), the
forward against the chain on alpha * f bit for bit, the gradients against a dense fp64 replica that applies the restatement's mask
(bound: 4 x the larger error of the chain on alpha * f and of a dense fp32 replica -- the criterion of test_attention_recompute_gpu,
which the new path does not set), determinism and independence of the plan's tunables, non-finite inputs, the layers, the memory
of a training step and its capture in a graph.  Graphs and helpers are those of test_spmm_values_gpu / test_attention_recompute_gpu."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attention_dropout_ref as ref
import spmm_driver as drv
import test_attention_heads_gpu as heads_gpu
import test_attention_recompute_gpu as rec
import test_spmm_values_gpu as values_gpu
from test_attention_fused_gpu import SPECIALS, dev, node_terms
from test_spmm_values_gpu import DEV, N_BIG, N_SMALL, THRESHOLDS, bits, launch, make_plan, strided_rows

pytestmark = pytest.mark.gpu
G = drv.GUARD
SEED = 0x1234_5678_9ABC_DEF1
KNOBS = [(thr, rpw) for thr in THRESHOLDS for rpw in (1, 3, 7)]


def step_tensor(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def ref_factors(plan, n_heads, keep, seed, step, hops=None):
    """The restatement's factor arrays for the plan's own (rowptr, colidx) -> one [nnz_k, K] device tensor per selected hop."""
    return [torch.from_numpy(ref.factors(plan.rowptr[k].cpu().numpy(), plan.colidx[k].cpu().numpy(), plan.n_cols, plan.n_hops, k, n_heads,
                                         keep, seed, step)).to(DEV) for k in plan._selected(hops)]


def chain_forward(plan, x, l, r, slope, factors, hops=None):
    with torch.no_grad():
        alpha = plan.row_softmax_heads(plan.edge_scores_heads(l, r, slope, hops=hops), hops=hops)
        return plan.spmm_values(x, [a * f for a, f in zip(alpha, factors)], hops=hops)


def raw_stats(plan, x, l, r, keep, seed, step, slope=0.2, hops=None):
    """h2gcn_attention_hops_heads_stats_dropout_f32 with Y and stats as guarded views, twice -> (y, stats)."""
    from h2gcn_amd import _capi

    h_sel, n, d, k = plan.n_selected(hops), plan.n_rows, x.shape[1], l.shape[2]
    outs = []
    for _ in range(2):
        ybuf, y = drv._guarded((n, h_sel, d), torch.float32, DEV)
        sbuf, s = drv._guarded((n, h_sel * 2 * k), torch.float32, DEV)
        st = _capi.lib().h2gcn_attention_hops_heads_stats_dropout_f32(
            plan._handle, plan._mask(hops), rec._ptr(l), l.stride(0), rec._ptr(r), r.stride(0), k, slope, rec._ptr(x), x.stride(0), d,
            rec._ptr(y), y.stride(0), y.stride(1), rec._ptr(s), s.stride(0), keep, seed, rec._ptr(step),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        rec._guards_untouched(ybuf, d, "Y")
        rec._guards_untouched(sbuf, h_sel * 2 * k, "stats")
        outs.append((y, s.reshape(n, h_sel, 2, k)))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), "the second call differs"
    return outs[0]


def raw_backward(plan, x, l, r, stats, y, g, keep, seed, step, slope=0.2, hops=None, needs=(True, True, True)):
    """h2gcn_attention_hops_heads_backward_dropout_f32 with delta, dl, dr, dX as guarded views, twice -> (dl, dr, dx)."""
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
            args += [rec._ptr(v), sh[1] + 2 * G]
        st = _capi.lib().h2gcn_attention_hops_heads_backward_dropout_f32(
            plan._handle, plan._mask(hops), rec._ptr(l), l.stride(0), rec._ptr(r), r.stride(0), k, slope, rec._ptr(x), x.stride(0), d,
            rec._ptr(stats), h_sel * 2 * k, rec._ptr(y), h_sel * d, d, rec._ptr(g), h_sel * d, d, *args, keep, seed, rec._ptr(step),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        for (buf, _), sh, name in zip(pairs, shapes, ("delta", "dl", "dr", "dX")):
            if buf is not None:
                rec._guards_untouched(buf, sh[1], name)
        runs.append(views[1:])
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), "the second backward launch differs from the first"
    dl, dr, dx = runs[0]
    return (None if dl is None else dl.reshape(plan.n_rows, h_sel, k), None if dr is None else dr.reshape(plan.n_cols, h_sel, k), dx)


# ------------------------------------------------------------------ 1. the factors
@pytest.mark.parametrize("keep", (0.5, 0.4))
@pytest.mark.parametrize("n_heads", (1, 3, 8, 16))
def test_factor_kernel_equals_the_restatement(n_heads, keep):
    hops = values_gpu.square_hops()
    step = step_tensor(3)
    first = None
    for thr, rpw in KNOBS:
        plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
        got = plan.attention_dropout_factors(n_heads, keep, SEED, step)
        if first is None:
            first = got
            for k, (f, w) in enumerate(zip(got, ref_factors(plan, n_heads, keep, SEED, 3))):
                assert f.shape == (hops[k].nnz, n_heads) and torch.equal(bits(f), bits(w)), f"hop {k}"
                share = float((f != 0).float().mean())
                assert 0.2 < share < 0.8, "the mask is degenerate"
        for f, w in zip(got, first):
            assert torch.equal(bits(f), bits(w)), f"thr {thr} rpw {rpw}: the factors depend on the plan's tunables"
    plan = make_plan(hops, long_row_threshold=256, rows_per_wave=3)
    alone = plan.attention_dropout_factors(n_heads, keep, SEED, step, hops=[1])
    assert len(alone) == 1 and torch.equal(bits(alone[0]), bits(first[1])), "hop 1 alone differs from slot 1 of the full call"
    zero = plan.attention_dropout_factors(n_heads, keep, SEED, None)                   # (no counter: step 0)
    for f, w in zip(zero, ref_factors(plan, n_heads, keep, SEED, 0)):
        assert torch.equal(bits(f), bits(w))
    assert not torch.equal(zero[0], first[0])
    ones = plan.attention_dropout_factors(n_heads, 1.0, SEED, step)
    assert all(bool((f == 1).all()) for f in ones)


def test_factors_of_the_rectangular_plan():
    hops = values_gpu.forward_hops()
    for thr, rpw in ((32, 1), (1024, 7)):
        plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
        for f, w in zip(plan.attention_dropout_factors(8, 0.4, SEED, step_tensor(2 ** 40 + 5)), ref_factors(plan, 8, 0.4, SEED, 2 ** 40 + 5)):
            assert torch.equal(bits(f), bits(w))


# ------------------------------------------------------------------ 2. forward bits
@pytest.mark.parametrize("thr,rpw", KNOBS)
def test_forward_has_the_bits_of_the_chain_on_dropped_coefficients(thr, rpw):
    hops = values_gpu.forward_hops()
    plan = make_plan(hops, long_row_threshold=thr, rows_per_wave=rpw)
    step = step_tensor(11)
    for (d, n_heads), keep in zip(((32, 1), (32, 8), (128, 8), (100, 1), (256, 16)), (0.5, 0.4, 0.5, 0.4, 0.5)):
        where = f"thr {thr} rpw {rpw} d {d} K {n_heads} keep {keep}"
        slope = 0.2 if n_heads > 1 else 0.01
        l, r = (dev(t) for t in node_terms(N_SMALL, N_BIG, 2, n_heads, seed=thr + rpw))
        x = dev(values_gpu.operands(d)[0])
        factors = plan.attention_dropout_factors(n_heads, keep, SEED, step)
        want = chain_forward(plan, x, l, r, slope, factors)
        y, stats = raw_stats(plan, x, l, r, keep, SEED, step, slope)
        assert torch.equal(bits(y), bits(want)), where + ": Y differs from spmm_values(x, alpha * f)"
        y0, stats0 = plan.attention_heads_stats(x, l, r, slope)
        assert torch.equal(bits(stats), bits(stats0)), where + ": the statistics differ from the launch without dropout"
        assert not torch.equal(bits(y), bits(y0)), where + ": nothing was dropped"
        y2, stats2 = plan.attention_heads_stats_dropout(x, l, r, keep, SEED, step, slope)
        assert torch.equal(bits(y2), bits(y)) and torch.equal(bits(stats2), bits(stats)), where + " (the method)"


def test_forward_on_strided_operands_and_a_guarded_out():
    d, n_heads, keep = 64, 2, 0.4
    hops = values_gpu.forward_hops()
    plan = make_plan(hops, long_row_threshold=256, rows_per_wave=7)
    x = np.random.default_rng(8).uniform(-1, 1, (N_BIG, d)).astype(np.float32)
    l, r = node_terms(N_SMALL, N_BIG, 2, n_heads, seed=8)
    xt, lt, rt = strided_rows(x), strided_rows(l), strided_rows(r)
    step = step_tensor(1)
    want = chain_forward(plan, xt, lt, rt, 0.2, plan.attention_dropout_factors(n_heads, keep, SEED, step))
    y, _ = raw_stats(plan, xt, lt, rt, keep, SEED, step)
    assert torch.equal(bits(y), bits(want))
    got = launch(lambda out: plan.attention_heads_stats_dropout(xt, lt, rt, keep, SEED, step, out=out)[0], (N_SMALL, 2, d),
                 "out= of the method")
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ 3. keep_prob = 1
def test_keep_prob_one_is_the_launch_without_dropout():
    hops, plan, x, l, r, gy, _, _, _ = rec.gradient_case("square", 32, 8)
    y0, stats0 = rec.raw_stats(plan, x, l, r)
    full0 = rec.raw_backward(plan, x, l, r, stats0, y0, gy)
    y, stats = raw_stats(plan, x, l, r, 1.0, SEED, step_tensor(4))
    assert torch.equal(bits(y), bits(y0)) and torch.equal(bits(stats), bits(stats0))
    for g, f in zip(raw_backward(plan, x, l, r, stats, y, gy, 1.0, SEED, step_tensor(4)), full0):
        assert torch.equal(bits(g), bits(f))


def test_a_wide_input_takes_the_chain_with_the_same_mask():
    from h2gcn_amd import hop_attention_recompute_dropout

    hops = values_gpu.square_hops()
    plan = values_gpu.adjoint_plan(hops, long_row_threshold=256)
    n, d = hops[0].shape[0], 260                                                     # beyond the backward's 256 columns: the chain
    x = dev(np.random.default_rng(4).uniform(-1, 1, (n, d)).astype(np.float32))
    l, r = (dev(t) for t in node_terms(n, n, 2, 1, seed=4))
    step = step_tensor(6)
    a = x.clone().requires_grad_(True)
    y = hop_attention_recompute_dropout(plan, a, l, r, 0.5, SEED, step, 0.01)
    assert torch.equal(bits(y), bits(chain_forward(plan, x, l, r, 0.01, plan.attention_dropout_factors(1, 0.5, SEED, step))))
    y.sum().backward()
    assert a.grad is not None and bool(torch.isfinite(a.grad).all())
    # one head: a column of the result does not know how many columns there are -- the first 256 are the fused launch's
    fused, _ = plan.attention_heads_stats_dropout(x[:, :256], l, r, 0.5, SEED, step, 0.01)
    assert torch.equal(bits(y[:, :, :256]), bits(fused))


# ------------------------------------------------------------------ 4. gradients against fp64
KEEP, STEP = 0.5, 9


def dense_grads(hops, x, l, r, gy, slope, dtype, keeps):
    """rec.dense_grads with the restatement's mask on alpha: ``keeps[s]`` the dense factor array [n_rows, n_cols, K]."""
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
        sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))
        alpha = torch.softmax(sc, dim=1) * mask[:, :, None].to(dtype) * keeps[s].to(dtype)
        ys.append(torch.einsum("ijh,jhw->ihw", alpha, X.view(n_cols, k, -1)).reshape(n_rows, -1))
    (torch.stack(ys, dim=1) * gy).sum().backward()
    return tuple(t.grad.double().numpy() for t in (L, R, X))


@functools.lru_cache(maxsize=None)
def gradient_case(kind, d, n_heads):
    """The operands of rec.gradient_case, the fp64 gradients under the restatement's mask and the bound 4 x max(err of the chain on
    alpha * f, err of the dense fp32 replica) per gradient."""
    from h2gcn_amd.layers import _dropped_chain

    hops, plan, x, l, r, gy, _, _, _ = rec.gradient_case(kind, d, n_heads)
    n_rows, n_cols = hops[0].shape
    dense_f = []
    for k, m in enumerate(hops):
        f = ref.factors(m.indptr, m.indices, n_cols, 2, k, n_heads, KEEP, SEED, STEP)
        full = torch.zeros((n_rows, n_cols, n_heads), dtype=torch.float64)
        coo_rows = np.repeat(np.arange(n_rows), np.diff(m.indptr))
        full[torch.from_numpy(coo_rows), torch.from_numpy(m.indices.astype(np.int64))] = torch.from_numpy(f).double()
        dense_f.append(full)
    host = [t.cpu().numpy() for t in (x, l, r, gy)]
    want = dense_grads(hops, *host, 0.2, torch.float64, dense_f)
    dense32 = dense_grads(hops, *host, 0.2, torch.float32, dense_f)
    a, b, c = (t.clone().requires_grad_(True) for t in (x, l, r))
    (_dropped_chain(plan, a, b, c, 0.2, None, KEEP, SEED, step_tensor(STEP)) * gy).sum().backward()
    chain = (b.grad, c.grad, a.grad)
    bound = tuple(4 * max(rec.rel_err(g, w), float(np.abs(g32 - w).max() / np.abs(w).max())) for g, g32, w in zip(chain, dense32, want))
    return hops, plan, x, l, r, gy, want, bound, tuple(rec.rel_err(g, w) for g, w in zip(chain, want))


@pytest.mark.parametrize("kind,d,n_heads", rec.CASES)
def test_gradients_against_fp64(kind, d, n_heads):
    """Measured ratios to the chain's error are in DESIGN.md ("Attention dropout in the kernels")."""
    hops, plan, x, l, r, gy, want, bound, chain_err = gradient_case(kind, d, n_heads)
    step = step_tensor(STEP)
    y, stats = plan.attention_heads_stats_dropout(x, l, r, KEEP, SEED, step, 0.2)
    grads = raw_backward(plan, x, l, r, stats, y, gy, KEEP, SEED, step)
    for name, g, w, b, ce in zip(("dl", "dr", "dx"), grads, want, bound, chain_err):
        err = rec.rel_err(g, w)
        print(f"{kind} d {d} K {n_heads} {name}: err {err:.3e}  chain {ce:.3e}  bound {b:.3e}  ratio to the chain {err / ce:.2f}")
        assert err <= b, f"{name}: relative error {err:.3e} beyond 4 x max(chain, dense fp32) = {b:.3e}"
    for g, h in zip(grads, plan.attention_heads_backward_dropout(x, l, r, stats, y, gy, KEEP, SEED, step)):
        assert torch.equal(bits(g), bits(h)), "the method differs from the raw launch"


# ------------------------------------------------------------------ 5. determinism and independence
def test_determinism_need_flags_and_hop_selection():
    hops, plan, x, l, r, gy, want, bound, _ = gradient_case("square", 32, 8)
    step = step_tensor(STEP)
    y, stats = plan.attention_heads_stats_dropout(x, l, r, KEEP, SEED, step)
    full = raw_backward(plan, x, l, r, stats, y, gy, KEEP, SEED, step)                  # (launched twice: equal bits)
    for needs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = raw_backward(plan, x, l, r, stats, y, gy, KEEP, SEED, step, needs=tuple(bool(v) for v in needs))
        for want_it, a, f in zip(needs, got, full):
            assert (a is None) if not want_it else torch.equal(bits(a), bits(f)), needs
    for k in range(2):
        sl = slice(k, k + 1)
        ya, sa = plan.attention_heads_stats_dropout(x, l[:, sl], r[:, sl], KEEP, SEED, step, hops=[k])
        assert torch.equal(bits(ya), bits(y[:, sl])), f"hop {k} alone: the mask depends on the selection"
        dl, dr, _ = raw_backward(plan, x, l[:, sl], r[:, sl], sa, ya, gy[:, sl], KEEP, SEED, step, hops=[k])
        assert torch.equal(bits(dl), bits(full[0][:, sl])), f"dl of hop {k} alone differs from its slot"
        assert torch.equal(bits(dr), bits(full[1][:, sl])), f"dr of hop {k} alone differs from its slot"
    for other in ((SEED, step_tensor(STEP + 1)), (SEED + 1, step)):
        assert not torch.equal(plan.attention_heads_stats_dropout(x, l, r, KEEP, *other)[0], y), "another step or seed, the same Y"


def test_plan_kinds_and_thresholds_give_the_same_bits():
    hops, plain, x, l, r, gy, _, _, _ = gradient_case("square", 32, 8)
    step = step_tensor(STEP)
    y, stats = plain.attention_heads_stats_dropout(x, l, r, KEEP, SEED, step)
    full = raw_backward(plain, x, l, r, stats, y, gy, KEEP, SEED, step)
    noperm = make_plan(hops, build_transpose=True, keep_permutation=False, long_row_threshold=256)
    sym = make_plan(hops, build_transpose=True, keep_permutation=True, symmetric_pattern=True, long_row_threshold=256)
    assert sym.transpose_sharing[0] != "none"
    others = [("no permutation", noperm), ("symmetric", sym)]
    others += [(f"thr {thr} rpw {rpw}", values_gpu.adjoint_plan(hops, long_row_threshold=thr, rows_per_wave=rpw))
               for thr, rpw in zip(THRESHOLDS, (1, 3, 7))]
    for name, plan in others:
        for g, f in zip(raw_backward(plan, x, l, r, stats, y, gy, KEEP, SEED, step), full):   # (the same operands, y included)
            assert torch.equal(bits(g), bits(f)), f"{name}: the bits differ from the plain plan's"


# ------------------------------------------------------------------ 6. special values
def test_a_dropped_entry_still_multiplies_and_heads_stay_apart():
    d, n_heads, head = 32, 8, 2
    w = d // n_heads
    hops, plan, x0, l, r, _, _, _, _ = gradient_case("square", d, n_heads)
    step = step_tensor(STEP)
    factors = plan.attention_dropout_factors(n_heads, KEEP, SEED, step)
    rows0 = np.repeat(np.arange(hops[0].shape[0]), np.diff(hops[0].indptr))
    dropped = np.flatnonzero(factors[0][:, head].cpu().numpy() == 0)
    e = int(dropped[len(dropped) // 2])
    i, j = int(rows0[e]), int(hops[0].indices[e])                                    # entry (i, j) of hop 0: head 2 is dropped
    x = x0.clone()
    x[j, head * w + 1] = float("inf")
    others = [n for n in range(x.shape[0]) if n != j][:len(SPECIALS)]
    for n, v in zip(others, SPECIALS):
        x[n, head * w + (n % w)] = v
    want = chain_forward(plan, x, l, r, 0.2, factors)
    y, _ = raw_stats(plan, x, l, r, KEEP, SEED, step)
    assert torch.equal(bits(y), bits(want)), "Y differs from the chain on alpha * f"
    assert bool(torch.isnan(y[i, 0, head * w + 1])), "0 * inf of the dropped entry did not reach its sum"
    clean, _ = raw_stats(plan, x0, l, r, KEEP, SEED, step)
    keep_cols = torch.ones(d, dtype=torch.bool)
    keep_cols[head * w:(head + 1) * w] = False
    assert torch.equal(bits(y)[:, :, keep_cols], bits(clean)[:, :, keep_cols]), "a planted value of one head reached another head"


# ------------------------------------------------------------------ 7. the layers
def test_layers_agree_and_eval_is_the_layer_without_dropout():
    from h2gcn_amd import MultiHeadHopAttention, RecomputeMultiHeadHopAttention

    d, heads, p = 32, 8, 0.5
    graph = rec.crafted()
    plan = graph.plan(**heads_gpu.KNOBS[1])
    x, rr = heads_gpu.uniform((graph.n, d), 21), heads_gpu.uniform((graph.n, 2, d), 22)
    torch.manual_seed(23)
    old = MultiHeadHopAttention(d, heads).set_attention_dropout(p, seed=77).to(DEV)
    new = RecomputeMultiHeadHopAttention(d, heads).to(DEV).set_attention_dropout(p, seed=77)   # (after .to(): the buffer follows the parameters)
    plain = MultiHeadHopAttention(d, heads).to(DEV)
    assert list(old.state_dict()) == list(new.state_dict()) == list(plain.state_dict()) == ["a_l", "a_r"]
    new.load_state_dict(old.state_dict())
    plain.load_state_dict(old.state_dict())
    assert "attn_dropout=0.5" in repr(old) and "attn_dropout" not in repr(plain)
    outs = []
    for layer in (old, new):
        y = layer(plan, x)
        (y * rr).sum().backward()
        outs.append(y)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "the output differs from the chain layer's"
    assert int(old._step) == int(new._step) == 1
    with torch.no_grad():
        base = plain(plan, x)
    assert not torch.equal(bits(outs[0]), bits(base))
    # the gradients: the dense replica with the mask of (seed 77, step 1)
    keep = 1.0 - p
    dense_f = []
    for k, m in enumerate(graph.mats):
        f = ref.factors(m.indptr, m.indices, graph.n, 2, k, heads, keep, 77, 1)
        full = torch.zeros((graph.n, graph.n, heads), dtype=torch.float64)
        full[torch.from_numpy(np.repeat(np.arange(graph.n), np.diff(m.indptr))), torch.from_numpy(m.indices.astype(np.int64))] = \
            torch.from_numpy(f).double()
        dense_f.append(full)

    def dense_layer_grads(dtype):
        wd = d // heads
        a_l, a_r = (q.detach().to(dtype).cpu().requires_grad_(True) for q in (old.a_l, old.a_r))
        X = x.to(dtype).cpu()
        L = torch.stack([X[:, h * wd:(h + 1) * wd] @ a_l[:, h, :].t() for h in range(heads)], dim=2)
        R = torch.stack([X[:, h * wd:(h + 1) * wd] @ a_r[:, h, :].t() for h in range(heads)], dim=2)
        ys = []
        for s in range(2):
            mask = torch.zeros((graph.n, graph.n), dtype=torch.bool)
            mask[graph.rows[s].cpu(), graph.cols[s].cpu()] = True
            sc = torch.nn.functional.leaky_relu(L[:, None, s, :] + R[None, :, s, :], old.negative_slope).masked_fill(~mask[:, :, None], float("-inf"))
            sc = torch.where(mask.any(dim=1)[:, None, None], sc, torch.zeros_like(sc))
            alpha = torch.softmax(sc, dim=1) * mask[:, :, None].to(dtype) * dense_f[s].to(dtype)
            ys.append(torch.einsum("ijh,jhw->ihw", alpha, X.view(graph.n, heads, wd)).reshape(graph.n, d))
        (torch.stack(ys, dim=1) * rr.to(dtype).cpu()).sum().backward()
        return a_l.grad.double().numpy(), a_r.grad.double().numpy()

    want, dense32 = dense_layer_grads(torch.float64), dense_layer_grads(torch.float32)
    for name, p_old, p_new, w64, w32 in zip(("a_l", "a_r"), (old.a_l, old.a_r), (new.a_l, new.a_r), want, dense32):
        e_old, e_new, e_32 = rec.rel_err(p_old.grad, w64), rec.rel_err(p_new.grad, w64), float(np.abs(w32 - w64).max() / np.abs(w64).max())
        print(f"{name}: err {e_new:.3e}, the chain layer {e_old:.3e}, dense fp32 {e_32:.3e}")
        assert e_new <= 4 * max(e_old, e_32), f"{name}: {e_new:.3e} beyond 4 x max(chain layer {e_old:.3e}, dense fp32 {e_32:.3e})"
    # eval(): the mask is off and the counter rests
    for layer in (old, new):
        layer.eval()
        with torch.no_grad():
            assert torch.equal(bits(layer(plan, x)), bits(base)), "eval() is not the layer without dropout"
        assert int(layer._step) == 1


def test_construction_draws_a_salt_only_when_it_needs_one():
    from h2gcn_amd import MultiHeadHopAttention, RecomputeMultiHeadHopAttention

    torch.manual_seed(5)
    a_l, a_r = torch.empty(2, 8, 4), torch.empty(2, 8, 4)
    torch.nn.init.xavier_uniform_(a_l)
    torch.nn.init.xavier_uniform_(a_r)                                                # what the layer without dropout has always drawn
    parent_state = torch.get_rng_state()
    for cls in (MultiHeadHopAttention, RecomputeMultiHeadHopAttention):
        for setting in (None, (0.0, None), (0.5, 3)):                                  # (no dropout, or an explicit seed: no salt is drawn)
            torch.manual_seed(5)
            layer = cls(32, 8)
            if setting is not None:
                assert layer.set_attention_dropout(*setting) is layer
            assert torch.equal(torch.get_rng_state(), parent_state), (cls.__name__, setting)
            assert torch.equal(layer.a_l, a_l) and torch.equal(layer.a_r, a_r)
            assert list(layer.state_dict()) == ["a_l", "a_r"]
        torch.manual_seed(5)
        m1, m2 = cls(32, 8).set_attention_dropout(0.5), cls(32, 8).set_attention_dropout(0.5)   # two layers of one model, seed=None
        assert m1.seed != m2.seed and torch.equal(m1.a_l, a_l)
        assert list(m1.state_dict()) == ["a_l", "a_r"]
    graph = rec.crafted()
    plan = graph.plan(**heads_gpu.KNOBS[1])
    x = heads_gpu.uniform((graph.n, 32), 21)
    m1, m2 = m1.to(DEV), m2.to(DEV)
    m2.load_state_dict(m1.state_dict())
    with torch.no_grad():
        assert not torch.equal(m1(plan, x), m2(plan, x)), "two layers with seed=None drew the same mask"


# ------------------------------------------------------------------ 8. no per-entry array
def test_a_training_step_with_dropout_allocates_no_per_entry_array():
    from h2gcn_amd import hop_attention_recompute_dropout

    d, n_heads = 32, 8
    hops, plan, x, l, r, gy, _, _, _ = gradient_case("square", d, n_heads)
    n = hops[0].shape[0]
    # what a step may hold: the result, the statistics, delta and the three gradients -- the mask costs nothing (the step counter
    # exists before the step)
    sizes = {"y": n * 2 * d, "stats": n * 2 * 2 * n_heads, "delta": n * 2 * n_heads, "dl": n * 2 * n_heads, "dr": n * 2 * n_heads, "dx": n * d}
    bound = sum(4 * v + 512 for v in sizes.values())
    assert bound < 4 * n_heads * hops[0].nnz, "a single [nnz_0, K] array must break the bound"
    a, b, c = (t.clone().requires_grad_(True) for t in (x, l, r))
    step_dev = step_tensor(STEP)

    def step():
        return torch.autograd.grad(hop_attention_recompute_dropout(plan, a, b, c, 0.5, SEED, step_dev), (a, b, c), gy)

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    grads = step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"extra device memory of one forward + backward with dropout: {extra} B; bound {bound} B; one [nnz_0, K] fp32 array "
          f"{4 * n_heads * hops[0].nnz} B")
    assert extra <= bound
    assert all(g is not None and float(g.abs().max()) > 0 for g in grads)


# ------------------------------------------------------------------ 9. capture
def test_captured_training_step_draws_a_fresh_mask_on_every_replay():
    from h2gcn_amd import RecomputeMultiHeadHopAttention

    d, heads = 32, 8
    graph = rec.crafted()
    plan = graph.plan(**heads_gpu.KNOBS[0])
    x, rr = heads_gpu.uniform((graph.n, d), 41), heads_gpu.uniform((graph.n, 2, d), 42)
    torch.manual_seed(43)
    a = RecomputeMultiHeadHopAttention(d, heads).set_attention_dropout(0.5).to(DEV)
    b = RecomputeMultiHeadHopAttention(d, heads).set_attention_dropout(0.5).to(DEV)
    params = list(a.parameters()) + list(b.parameters())
    init = [p.detach().clone() for p in params]

    def forward():
        h = a(plan, x)
        return b(plan, torch.tanh(h[:, 0] + h[:, 1]))

    def step():
        for p in params:
            p.grad = None
        (forward() * rr).sum().backward()
        with torch.no_grad():
            for p in params:
                p.sub_(0.05 * p.grad)

    def reset():
        with torch.no_grad():
            for p, q in zip(params, init):
                p.copy_(q)
            a._step.zero_()
            b._step.zero_()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                      # the eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    reset()
    for _ in range(3):
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
    for _ in range(3):
        graph_.replay()
    torch.cuda.synchronize()
    assert int(a._step) == int(b._step) == 3
    assert all(torch.equal(p.detach(), q) for p, q in zip(params, eager)), "three replays differ from three eager steps"
    assert all(not torch.equal(p, q) for p, q in zip(eager, init))
    # on fixed parameters: every replay of a captured forward has a mask of its own
    reset()
    fwd = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(fwd):
        out = forward()
    seen = []
    for _ in range(2):
        fwd.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]), "replay 2 drew the mask of replay 1"
