"""GPU suite: the recomputing attention backward (h2gcn_amd/csrc/attention_backward.hip.h: row_segment / col_row, wrapped by the fp32,
dropout and bf16 kernel pairs) over EVERY kernel geometry of `for_geometry`, against an independent reference.

The reference is tests/attention_backward_ref.py, a numpy restatement of the header's formulas run in fp64; the error of every element
is weighed against the sum of the absolute values of ITS OWN terms (rho), and the bound is 4 x the larger rho of the restatement run
in fp32 and of the unchanged chain (hop_attention_heads under autograd) -- the rule of test_attention_recompute_gpu.gradient_case,
made per element, and never set by the code under test.  The operands (attention_backward_ref.sweep_hops) prescribe the segment
lengths of the rows AND of the columns: one chunk, two, four sets, a second round of set 0, the thresholds of the three plans.  Every
input of a raw launch is a view with NaN between its rows (and between the hop slots of y and g): an over-read that is consumed
shows as a NaN.  Per shape: (a) fp32 against fp64, (b) the bits across the plans' knobs, (c) the bits of a head against the
single-head launch on that head's column slice, (d) the need flags, (e) the bf16 pair against the fp32 pair on these operands,
(f) dropout against fp64 under the restated mask, (g) hop selection."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attention_backward_ref as ref
import attention_dropout_ref as dropout_ref
import spmm_driver as drv
import test_attention_bf16_gpu as bf16_gpu
from test_attention_dropout_gpu import KEEP, SEED, STEP, step_tensor
from test_attention_fused_gpu import dev, node_terms
from test_spmm_values_gpu import DEV, adjoint_plan, bits, make_plan

pytestmark = pytest.mark.gpu
G = drv.GUARD
SLOPE = 0.2
KNOBS = ((32, 1), (256, 3), (1024, 7))                              # (long_row_threshold, rows_per_wave); the last: no long segment
NAMES = ("delta", "dl", "dr", "dx")

SHAPES = {
    (1, 2): [(8, 2), (20, 5), (64, 16)],                            # packed, w = 4
    (2, 2): [(16, 2), (72, 9), (128, 16)],                          # w = 8
    (4, 2): [(48, 3), (80, 5), (128, 8)],                           # w = 16
    (8, 2): [(64, 2), (96, 3), (128, 4)],                           # w = 32
    (0, 1): [(1, 1), (3, 1), (4, 1), (5, 1), (22, 1), (63, 1), (64, 1), (24, 2), (60, 3), (56, 2)],
    (0, 2): [(65, 1), (100, 1), (127, 1), (128, 1), (72, 3), (96, 2), (120, 2), (128, 2)],
    (0, 4): [(129, 1), (255, 1), (256, 1), (132, 3), (144, 12), (160, 5), (192, 2), (192, 16), (256, 2), (256, 4), (256, 16)],
}
GRID = [shape for shapes in SHAPES.values() for shape in shapes]
HOP_SELECTION = {shapes[0] if geom != (0, 1) else (24, 2) for geom, shapes in SHAPES.items()}       # (g): one shape per geometry


def geometry(d, k):
    """for_geometry of attention_backward.hip.h -> (L, NB)."""
    w = d // k
    if k > 1 and d <= 128 and w in (4, 8, 16, 32):
        return w // 4, 2
    return 0, 1 if d <= 64 else 2 if d <= 128 else 4


def test_every_geometry_is_reached_by_three_shapes():
    reached = {}
    for d, k in GRID:
        assert d % k == 0 and (k == 1 or (d // k) % 4 == 0) and d <= 256 and k <= 16
        reached.setdefault(geometry(d, k), []).append((d, k))
    assert set(reached) == {(1, 2), (2, 2), (4, 2), (8, 2), (0, 1), (0, 2), (0, 4)}
    assert all(len(v) >= 3 for v in reached.values()), reached
    assert all(geometry(d, k) == geom for geom, shapes in SHAPES.items() for d, k in shapes), "a shape is filed under another geometry"
    assert len(set(GRID)) == len(GRID) and sorted(geometry(*shape) for shape in HOP_SELECTION) == sorted(SHAPES)
    for geom in ((0, 1), (0, 2), (0, 4)):                           # the head-aligned blocks: single heads, tails and several heads
        assert sum(k == 1 for _, k in reached[geom]) >= 3 and sum(k > 1 for _, k in reached[geom]) >= 3


# ------------------------------------------------------------------ operands and plans
def plan_of(knob):
    thr, rpw = KNOBS[knob]
    return make_plan(ref.sweep_hops(), build_transpose=True, long_row_threshold=thr, rows_per_wave=rpw)


def padded(t, pad=4):
    """A device copy of `t` as a view with `pad` NaN elements after every row of its LAST dimension."""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), float("nan"), dtype=torch.float32, device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf[..., :t.shape[-1]]


def padded_rows(t):
    """`t` [n, ...] as a view whose rows, flattened, are 4 NaN elements apart (l, r, stats: one leading dimension in the ABI)."""
    return padded(t.reshape(t.shape[0], -1)).unflatten(1, tuple(t.shape[1:]))


@functools.lru_cache(maxsize=None)
def host_case(d, k):
    hops = ref.sweep_hops()
    n = hops[0].shape[0]
    rng = np.random.default_rng(1000 + 17 * d + k)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)
    l, r = node_terms(n, n, 2, k, seed=d + k)
    return hops, x, l, r, g


def references(d, k, factors, chain):
    """The fp64 restatement, its magnitude arrays and, per array, (rho of the fp32 restatement, rho of the chain or None)."""
    from h2gcn_amd._capi import H2GCNError

    hops, x, l, r, g = host_case(d, k)
    want, mags = ref.backward(hops, x, l, r, g, SLOPE, factors)
    got32, _ = ref.backward(hops, x, l, r, g, SLOPE, factors, dtype=np.float32)
    rho32 = [ref.rho(a, w, m) for a, w, m in zip(got32, want, mags)]
    rho_chain = [None] * 4
    a, b, c = (dev(t).requires_grad_(True) for t in (x, l, r))
    try:
        y = chain(a, b, c)
    except (ValueError, H2GCNError) as refusal:                     # (the chain's term of the bound alone may be missing)
        print(f"d {d} K {k}: the chain refuses the shape ({refusal}): the fp32 restatement alone sets the bound")
    else:
        (y * dev(g)).sum().backward()
        for n_, grad in ((1, b.grad), (2, c.grad), (3, a.grad)):
            rho_chain[n_] = ref.rho(grad.cpu().numpy(), want[n_], mags[n_])
    return want, mags, rho32, rho_chain


def launch_backward(plan, x, l, r, stats, y, g, hops=None, needs=(True, True, True), dropout=None):
    """h2gcn_attention_hops_heads_backward_f32 (dropout=(keep, seed, step tensor): ..._dropout_f32) on the operands AS THEY LIE: every
    leading dimension is the view's stride.  delta, dl, dr, dX are guarded views; launched twice -> (delta, dl, dr, dx)."""
    from h2gcn_amd import _capi

    h_sel, d, k = plan.n_selected(hops), x.shape[1], l.shape[2]
    assert tuple(stats.shape) == (plan.n_rows, h_sel, 2, k) and stats.stride(1) == 2 * k and stats.stride(2) == k and stats.stride(3) == 1
    assert l.stride(1) == k and r.stride(1) == k and tuple(y.shape) == tuple(g.shape) == (plan.n_rows, h_sel, d)
    assert all(t.stride(-1) == 1 or t.shape[-1] == 1 for t in (x, l, r, y, g))
    shapes = ((plan.n_rows, h_sel * k), (plan.n_rows, h_sel * k), (plan.n_cols, h_sel * k), (plan.n_cols, d))
    extra = () if dropout is None else (dropout[0], dropout[1], C.c_void_p(dropout[2].data_ptr()))
    fn = _capi.lib().h2gcn_attention_hops_heads_backward_f32 if dropout is None else _capi.lib().h2gcn_attention_hops_heads_backward_dropout_f32
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    runs = []
    for _ in range(2):
        pairs = [drv._guarded(sh, torch.float32, DEV) if want else (None, None) for sh, want in zip(shapes, (True,) + tuple(needs))]
        args = []
        for (_, v), sh in zip(pairs, shapes):
            args += [ptr(v), sh[1] + 2 * G]
        st = fn(plan._handle, plan._mask(hops), ptr(l), l.stride(0), ptr(r), r.stride(0), k, SLOPE, ptr(x), x.stride(0), d, ptr(stats),
                stats.stride(0), ptr(y), y.stride(0), y.stride(1), ptr(g), g.stride(0), g.stride(1), *args, *extra,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _capi.check(st)
        for (buf, _), sh, name in zip(pairs, shapes, NAMES):
            if buf is not None:
                assert bool(torch.isnan(buf[..., :G]).all()) and bool(torch.isnan(buf[..., G + sh[1]:]).all()), f"{name}: a guard word was written"
        runs.append([v for _, v in pairs])
    for name, a, b in zip(NAMES, *runs):
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), f"{name}: the second launch differs from the first"
    delta, dl, dr, dx = runs[0]
    shape3 = lambda t, n: None if t is None else t.reshape(n, h_sel, k)     # noqa: E731
    return shape3(delta, plan.n_rows), shape3(dl, plan.n_rows), shape3(dr, plan.n_cols), dx


def forward(plan, x, l, r, dropout=None):
    """y in a buffer with NaN after every hop slot, stats with NaN after every row."""
    d = x.shape[1]
    ybuf = torch.full((plan.n_rows, 2, d + 4), float("nan"), dtype=torch.float32, device=DEV)
    if dropout is None:
        y, stats = plan.attention_heads_stats(x, l, r, SLOPE, out=ybuf[:, :, :d])
    else:
        y, stats = plan.attention_heads_stats_dropout(x, l, r, *dropout, SLOPE, out=ybuf[:, :, :d])
    assert y.data_ptr() == ybuf.data_ptr() and y.stride(1) == d + 4
    return y, padded_rows(stats)


def same_bits(got, want, where, failures):
    for name, a, b in zip(NAMES, got, want):
        if a is None or b is None:
            continue
        if not torch.equal(bits(a), bits(b)):
            failures.append(f"{where}: {name} differs in {int((bits(a) != bits(b)).sum())} of {a.numel()} elements")


def against_fp64(got, refs, where, failures, worst):
    """(a) / (f): rho per array against 4 x max(fp32 restatement, chain); exact +0 where no term exists."""
    want, mags, rho32, rho_chain = refs
    for n, (name, a, w, m) in enumerate(zip(NAMES, got, want, mags)):
        a = a.cpu().numpy()
        rho = ref.rho(a, w, m)
        bound = 4 * max(rho32[n], rho_chain[n] or 0.0)
        chain = "none" if rho_chain[n] is None else f"{rho_chain[n]:.3e}"
        print(f"{where} {name}: rho {rho:.3e}  fp32 restatement {rho32[n]:.3e}  chain {chain}  bound {bound:.3e}")
        worst[name] = max(worst.get(name, 0.0), rho / bound if rho == rho and bound > 0 else float("inf"))
        if not rho <= bound:
            ratio = np.where(m > 0, np.abs(a - w) / np.where(m > 0, m, 1), 0)
            at = np.unravel_index(np.argmax(np.nan_to_num(ratio, nan=np.inf)), a.shape)
            failures.append(f"{where}: {name} rho {rho:.3e} beyond 4 x max(fp32 restatement {rho32[n]:.3e}, chain {chain}) = {bound:.3e}"
                            f" (worst element {at}, NaNs {int(np.isnan(a).sum())})")
        if not ref.zeros_exact(a, m, signed=(name == "delta")):
            failures.append(f"{where}: {name} of an element without terms (an empty segment, a column nobody references) is not +0")
    return worst


@pytest.mark.parametrize("d,k", GRID)
def test_sweep(d, k):
    from h2gcn_amd import hop_attention_heads
    from h2gcn_amd.layers import _dropped_chain

    index = GRID.index((d, k))
    w = d // k
    hops, hx, hl, hr, hg = host_case(d, k)
    x, l, r, g = padded(hx), padded_rows(hl), padded_rows(hr), padded(hg)
    assert x.stride(0) == d + 4 and l.stride(0) == 2 * k + 4 and g.stride(1) == d + 4 and g.stride(0) == 2 * (d + 4)
    chain_plan = adjoint_plan(hops, long_row_threshold=256)
    failures, worst = [], {}
    where = f"d {d} K {k}"

    # ---- (a) every knob against fp64; (b) the bits of knobs 2 and 3 are those of knob 1, on the same y and stats
    refs = references(d, k, None, lambda a, b, c: hop_attention_heads(chain_plan, a, b, c, SLOPE))
    y, stats = forward(plan_of(0), x, l, r)
    full = None
    for knob in range(3):
        plan = plan_of(knob)
        assert torch.equal(bits(plan.attention_heads_stats(x, l, r, SLOPE)[1]), bits(stats)), f"{where}: stats of knob {knob}"
        got = launch_backward(plan, x, l, r, stats, y, g)
        against_fp64(got, refs, f"{where} thr {KNOBS[knob][0]} rpw {KNOBS[knob][1]}", failures, worst)
        if full is None:
            full = got
        else:
            same_bits(got, full, f"{where}: (b) knob {KNOBS[knob]} against knob {KNOBS[0]}", failures)

    # ---- (c) a head of the launch has the bits of the single-head launch (L = 0, d = w) on its column slice
    for h in sorted({0, k - 1}) if k > 1 else ():
        cs = slice(h * w, (h + 1) * w)
        one = launch_backward(plan_of(0), x[:, cs], padded_rows(l[:, :, h:h + 1]), padded_rows(r[:, :, h:h + 1]),
                              padded_rows(stats[:, :, :, h:h + 1]), y[:, :, cs], g[:, :, cs])
        want = (full[0][:, :, h:h + 1], full[1][:, :, h:h + 1], full[2][:, :, h:h + 1], full[3][:, cs])
        same_bits(one, want, f"{where}: (c) head {h} against the K = 1 launch on its columns", failures)

    # ---- (d) need flags
    for needs in ((True, False, False), (False, True, False), (False, False, True)):
        got = launch_backward(plan_of(1), x, l, r, stats, y, g, needs=needs)
        assert all((t is None) != want_it for t, want_it in zip(got[1:], needs))
        same_bits(got, full, f"{where}: (d) needs {needs}", failures)

    # ---- (e) the bf16 pair against the fp32 pair on the bf16-rounded operands, every knob
    if d % 2 == 0:
        x16, g16 = bf16_gpu.bf16_operand(hx), bf16_gpu.bf16_operand(hg)
        lc, rc = dev(hl), dev(hr)
        for knob in range(3):
            try:
                bf16_gpu.check_backward(plan_of(knob), x16, lc, rc, g16, f"{where}: (e) knob {KNOBS[knob]}", slope=SLOPE)
            except AssertionError as e:
                failures.append(str(e) or f"{where}: (e) knob {KNOBS[knob]}")

    # ---- (f) dropout against fp64 under the restated mask, one knob
    knob = index % 3
    plan = plan_of(knob)
    factors = [dropout_ref.factors(m.indptr, m.indices, m.shape[1], 2, s, k, KEEP, SEED, STEP) for s, m in enumerate(hops)]
    step = step_tensor(STEP)
    refs_f = references(d, k, factors, lambda a, b, c: _dropped_chain(chain_plan, a, b, c, SLOPE, None, KEEP, SEED, step))
    yf, stats_f = forward(plan, x, l, r, (KEEP, SEED, step))
    assert torch.equal(bits(stats_f), bits(stats)) and not torch.equal(bits(yf), bits(y))
    got_f = launch_backward(plan, x, l, r, stats_f, yf, g, dropout=(KEEP, SEED, step))
    worst_f = against_fp64(got_f, refs_f, f"{where} dropout thr {KNOBS[knob][0]} rpw {KNOBS[knob][1]}", failures, {})

    # ---- (g) hop selection: the slot's bits; dX summed over the two runs within the bound of (a)
    if (d, k) in HOP_SELECTION:
        dx_sum = 0
        for s in range(2):
            sl = slice(s, s + 1)
            one = launch_backward(plan_of(1), x, l[:, sl], r[:, sl], stats[:, sl], y[:, sl], g[:, sl], hops=[s])
            same_bits(one[:3], [t[:, sl] for t in full[:3]], f"{where}: (g) hop {s} alone against its slot", failures)
            dx_sum = dx_sum + one[3].double()
        want, mags, rho32, rho_chain = refs
        rho, bound = ref.rho(dx_sum.cpu().numpy(), want[3], mags[3]), 4 * max(rho32[3], rho_chain[3] or 0.0)
        print(f"{where} (g) dx summed over single-hop runs: rho {rho:.3e}  bound {bound:.3e}")
        if not rho <= bound:
            failures.append(f"{where}: (g) dx summed over the single-hop runs: rho {rho:.3e} beyond {bound:.3e}")

    print(f"{where} [{geometry(d, k)}] largest ratio to the bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items())
          + "  | dropout: " + "  ".join(f"{n} {v:.3f}" for n, v in worst_f.items()))
    assert not failures, "\n".join(failures)
