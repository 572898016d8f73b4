"""GPU suite: row-constant hops (h2gcn_plan_row_constant).  When every stored value of each row of every selected hop carries
the bits of the row's first one, the forward walk on the index window (plain walk, 64-column slices, fp32 output, at most two
hops) takes the row's value from the plan and never reads the value array -- the ROWVAL instantiations of spmm_hops_kernel.
The other GPU files draw random values and stay on the value stream; this one sweeps the new path:

* graphs of tests/spmm_driver.py (every segment length around the chunks of 64, the ring blocks of 128 and the long threshold,
  at every position of a wave's rows, a last wave with fewer rows, row n - 1) with their values OVERWRITTEN by row constants,
  run through ``spmm_driver.run_case``: bit for bit the canonical-tree oracle on NaN-prefilled, guard-banded outputs;
* row constants that are NaN, +-Inf, -0.0, subnormal or 3e38 (compared NaN-aware: same NaN positions, same bits elsewhere);
* the detection's edges against its numpy restatement (tests/test_row_values.py), with launches that mix a constant and a
  non-constant hop; ``set_values``; a three-hop selection (the walk next to the window).

variant = 3 is the plain tile walk; slice_cols = 64 puts d = 128 / 100 on two 64-column slices (the second one masked for 100)."""
import functools

import numpy as np
import pytest
import torch

import spmm_driver as sd
from oracle import gcn_layer as og
from test_row_values import row_constant_np, row_values_np

pytestmark = pytest.mark.gpu
F32 = np.float32
PLAIN_WALK = 3
WIDTHS = ((64, 0), (128, 64), (100, 64), (20, 0))          # (d, slice_cols)
KINDS = ("inv_deg", "ones", "per_row")
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x007fffff], dtype=np.uint32).view(F32).tolist() + [3e38, -3e38]
SMALLEST_SUBNORMAL = float(np.array([1], dtype=np.uint32).view(F32)[0])      # 2^-149: has a test of its own below


def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def base_graph(thr, rpw, rot=0):
    return sd.edges_graph(thr, rpw, rot)


def with_values(hops, kind, seed=0):
    """Copies of the hop matrices whose values are constant along every row."""
    out = []
    for k, m in enumerate(hops):
        m = m.copy()
        lengths = np.diff(m.indptr)
        rng = np.random.default_rng(1000 * seed + k)
        if kind == "inv_deg":
            per_row = (1.0 / np.maximum(lengths, 1)).astype(F32)
        elif kind == "ones":
            per_row = np.ones(len(lengths), dtype=F32)
        elif kind == "per_row":
            per_row = rng.uniform(-1, 1, len(lengths)).astype(F32)
        else:   # "special" / "tiny": every special constant on rows of every length, distinct finite ones elsewhere
            pool = np.array(SPECIALS if kind == "special" else [SMALLEST_SUBNORMAL, -SMALLEST_SUBNORMAL], dtype=F32)
            per_row = rng.uniform(-1, 1, len(lengths)).astype(F32)
            at = rng.permutation(len(lengths))[: len(lengths) // 2]
            per_row[at] = pool[np.arange(len(at)) % len(pool)]
        m.data = np.repeat(per_row, lengths).astype(F32)
        assert row_constant_np(m.indptr, m.data)
        out.append(m)
    return out


def make_plan(hops, thr=0, rpw=0, slice_cols=0, **kw):
    from h2gcn_amd import HopPlan

    return HopPlan.from_scipy(hops, dev(), long_row_threshold=thr, rows_per_wave=rpw, variant=PLAIN_WALK, slice_cols=slice_cols, **kw)


def on_the_window(plan, d, hops=None):
    s = plan.schedule(d, hops=hops)
    return s["segment_walk"] == "wave per segment" and s["slice_cols"] == 64


def same_bits_nan_aware(y, want):
    y = y.detach().cpu().contiguous().numpy()
    want = np.ascontiguousarray(want, dtype=F32)
    nan = np.isnan(want)
    return y.shape == want.shape and np.array_equal(np.isnan(y), nan) and np.array_equal(y.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def launch_and_compare(plan, hops, d, thr, sel=None, where=""):
    """One guarded forward launch (twice) of `plan` on hop selection `sel`, NaN-aware bit comparison with the tree oracle."""
    n_rows, n_cols = hops[0].shape
    x = np.random.default_rng(d).uniform(-1, 1, (n_cols, d)).astype(F32)
    xt = torch.from_numpy(x).to(dev())
    xt[n_cols - 1] = float("nan")          # the driver's graphs never reference the last column
    idx = list(range(len(hops))) if sel is None else sorted(sel)
    tree = og.gcn_layer_tree(hops, x, long_threshold=thr or sd.DEFAULT_THR)[:, idx]
    y = sd._launch_twice(lambda out: plan.spmm(xt, hops=sel, out=out), (n_rows, len(idx), d), torch.float32, dev(), where)
    assert same_bits_nan_aware(y, tree), f"{where}: bits differ from the canonical tree"
    return tree


SWEEP = [(thr, rpw, WIDTHS[i % 4], KINDS[i % 3]) for i, (thr, rpw) in enumerate((t, r) for t in (0, 16, 17, 512) for r in (1, 4, 7))]


@pytest.mark.parametrize("thr,rpw,width,kind", SWEEP, ids=[f"thr{t}-rpw{r}-d{w[0]}-{k}" for t, r, w, k in SWEEP])
def test_row_constant_values_give_the_tree(thr, rpw, width, kind):
    """Segment lengths 0, 1, 63..65, 127..129, 191..193, 254..257 and thr - 2 .. thr + 1 under the default threshold and
    thresholds 16, 17 and 512 (the long branch; a long segment stepped over inside a wave's range), rows_per_wave 1 / 4 / 7,
    every width with every kind of row constant; selections of both hops and of each one."""
    d, sc = width
    hops = with_values(base_graph(thr, rpw, rpw), kind, seed=thr + rpw)
    plan = make_plan(hops, thr, rpw, sc)
    assert plan.row_constant == [1, 1] and on_the_window(plan, d), (plan.row_constant, plan.schedule(d))
    case = sd.Case(f"row values thr={thr} rpw={rpw} d={d}/{sc} {kind}", None, d, variant=PLAIN_WALK, thr=thr, rpw=rpw, slice_cols=sc,
                   fwd=(None, [0], [1]), claims=(("fwd", None, "walk", "tile"), ("fwd", None, "n_long", lambda n: n > 0)))
    sd.run_case(case, dev(), env={}, hops=hops)


@pytest.mark.parametrize("d,sc", [(64, 0), (128, 64)])
def test_bf16_sources(d, sc):
    hops = with_values(base_graph(0, 4, 1), "inv_deg")
    case = sd.Case(f"row values bf16 d={d}", None, d, variant=PLAIN_WALK, rpw=4, slice_cols=sc, fwd=(None, [1]), adj=(None,), bf16=True,
                   claims=(("fwd", None, "walk", "tile"),))
    sd.run_case(case, dev(), env={}, hops=hops)     # (bf16 -> fp32 on the row values; bf16 -> bf16 and the adjoint on the stream)


@pytest.mark.parametrize("off,tail", [(0, 0), (1, 64), (31, 0)])
def test_colidx_views_into_poisoned_buffers(off, tail):
    """colidx starts `off` elements past a line boundary inside a buffer of poison ids (the column of X's NaN row); the value
    buffers are Inf around the views and sit at other offsets."""
    other = {0: 31, 1: 0, 31: 1}[off]
    hops = with_values(base_graph(0, 7, 2), "per_row", seed=off)
    for d, sc in ((64, 0), (128, 64)):
        case = sd.Case(f"row values views off={off} tail={tail} d={d}", None, d, variant=PLAIN_WALK, rpw=7, slice_cols=sc, fwd=(None, [1]),
                       views=(((off, other), (other, off)), tail), claims=(("fwd", None, "walk", "tile"),))
        sd.run_case(case, dev(), env={}, hops=hops)


@pytest.mark.parametrize("thr,rpw,width", [(0, 4, (64, 0)), (16, 7, (128, 64)), (512, 1, (20, 0))])
def test_special_row_constants(thr, rpw, width):
    """NaN, +-Inf, -0.0, the largest subnormal, +-3e38 as the constant of rows of every length."""
    d, sc = width
    hops = with_values(base_graph(thr, rpw, 3), "special", seed=thr)
    plan = make_plan(hops, thr, rpw, sc)
    assert plan.row_constant == [1, 1] and on_the_window(plan, d)
    for sel in (None, [0], [1]):
        tree = launch_and_compare(plan, hops, d, thr, sel, f"special thr={thr} hops={sel}")
    assert np.isnan(tree).any() and np.isinf(tree).any() and (tree == 0).any()


def test_smallest_subnormal_row_constant():
    """Row constants of +-2^-149: every product w * x with |x| <= 0.5 underflows to a signed zero.

    A partial of the tree can then be -0.0, and the sign of a zero shows what a padding slot does: with four lane groups, the
    groups that have no neighbour in a segment's last, ragged step still execute a multiply-add (gather_batch /
    gather_batch_window, the `take` predicate).  The row-value kernels pad with fma(-0.0, +0.0, p), which is p for every p, so
    they give the tree's bits; fma(+0.0, +0.0, p), the padding of the kernels on the value stream, turns a -0.0 partial into
    +0.0 (measured on a build without the -0.0: 2 of the 112 896 elements of Y on this graph, both in rows of 7 entries, with
    2^-149 as one of eight special constants).  Tile-walk segments and, under threshold 16, long ones."""
    for thr, rpw, (d, sc) in ((0, 4, (64, 0)), (16, 7, (128, 64))):
        hops = with_values(base_graph(thr, rpw, 3), "tiny", seed=thr)
        plan = make_plan(hops, thr, rpw, sc)
        assert plan.row_constant == [1, 1] and on_the_window(plan, d)
        for sel in (None, [0], [1]):
            launch_and_compare(plan, hops, d, thr, sel, f"row constants of +-2^-149, thr={thr} hops={sel}")


def _break_row(m, row, where, kind):
    """A copy of m whose row `row` has ONE entry that differs in its bits from the others (`where`: first / middle / last)."""
    m = m.copy()
    b, e = int(m.indptr[row]), int(m.indptr[row + 1])
    assert e - b >= 3, "the row needs a first, a middle and a last entry"
    at = {"first": b, "middle": (b + e) // 2, "last": e - 1}[where]
    bits = m.data.view(np.uint32)
    if kind == "mantissa":
        bits[at] ^= 1
    elif kind == "zero":
        bits[b:e] = 0x00000000
        bits[at] = 0x80000000
    else:   # two NaN payloads
        bits[b:e] = 0x7fc00000
        bits[at] = 0x7fc00001
    return m


@pytest.mark.parametrize("hop", [0, 1])
@pytest.mark.parametrize("kind", ["mantissa", "zero", "nan"])
def test_detection_edges(kind, hop):
    """One entry differs from its row's first value -- in the last mantissa bit, as -0.0 next to +0.0, as a second NaN payload --
    first, in the middle or last in its row, or in the last row; in one hop only.  row_constant equals the numpy restatement,
    the launch over both hops and the launch over the constant hop alone equal the oracle."""
    thr, rpw, d = 0, 4, 64
    rot = next(r for r in range(40) if all(np.diff(m.indptr)[-1] >= 3 for m in base_graph(thr, rpw, r)))
    clean = with_values(base_graph(thr, rpw, rot), "per_row", seed=7)
    n = clean[0].shape[0]
    mid_row = int(np.flatnonzero(np.diff(clean[hop].indptr) >= 65)[3])
    for row, where in ((mid_row, "first"), (mid_row, "middle"), (mid_row, "last"), (n - 1, "last"), (n - 1, "first")):
        hops = list(clean)
        hops[hop] = _break_row(clean[hop], row, where, kind)
        want = [row_constant_np(m.indptr, m.data) for m in hops]
        assert want == [int(k != hop) for k in range(2)]
        plan = make_plan(hops, thr, rpw)
        assert plan.row_constant == want, (row, where)
        assert on_the_window(plan, d)
        launch_and_compare(plan, hops, d, thr, None, f"{kind} hop {hop} row {row} {where}: both hops")
        launch_and_compare(plan, hops, d, thr, [1 - hop], f"{kind} hop {hop} row {row} {where}: the constant hop")
        launch_and_compare(plan, hops, d, thr, [hop], f"{kind} hop {hop} row {row} {where}: the other hop")


def test_set_values_falls_back_to_the_stream():
    thr, rpw, d = 0, 4, 64
    hops = with_values(base_graph(thr, rpw, 5), "inv_deg")
    plan = make_plan(hops, thr, rpw)
    n_rows = hops[0].shape[0]
    assert plan.row_constant == [1, 1]
    launch_and_compare(plan, hops, d, thr, None, "before set_values")
    bytes_before = plan.device_bytes()
    assert bytes_before >= 2 * 4 * n_rows
    new = hops[1].copy()
    new.data = np.random.default_rng(9).uniform(-1, 1, new.nnz).astype(F32)
    assert not row_constant_np(new.indptr, new.data)
    plan.set_values(1, torch.from_numpy(new.data).to(dev()))
    assert plan.row_constant == [1, 0]
    assert plan.device_bytes() == bytes_before - 4 * n_rows
    changed = [hops[0], new]
    launch_and_compare(plan, changed, d, thr, None, "after set_values: both hops")
    launch_and_compare(plan, changed, d, thr, [0], "after set_values: the constant hop")
    launch_and_compare(plan, changed, d, thr, [1], "after set_values: the replaced hop")
    # row-constant values brought by set_values are NOT detected again: the hop stays on the stream, with the right result
    plan.set_values(1, torch.from_numpy(hops[1].data).to(dev()))
    assert plan.row_constant == [1, 0]
    launch_and_compare(plan, hops, d, thr, None, "after a second set_values")


def test_three_row_constant_hops_keep_the_walk_next_to_the_window():
    h = with_values(base_graph(0, 4, 6), "per_row", seed=3)
    hops = [h[0], h[1], h[0]]
    case = sd.Case("row values, 3 hops", None, 64, variant=PLAIN_WALK, rpw=4, fwd=(None, [0, 2], [1]), claims=(("fwd", None, "walk", "tile"),))
    sd.run_case(case, dev(), env={}, hops=hops)
    assert make_plan(hops, 0, 4).row_constant == [1, 1, 1]


def test_rowval_bits_match_the_restatement_on_an_empty_hop():
    """A hop without nonzeros is row-constant (every row value 0) and its launch writes zeros."""
    import scipy.sparse as sp

    h = with_values(base_graph(0, 4, 6), "ones")
    empty = sp.csr_matrix(h[0].shape, dtype=F32)
    hops = [h[0], empty]
    assert row_values_np(empty.indptr, empty.data)[0]
    plan = make_plan(hops, 0, 4)
    assert plan.row_constant == [1, 1]
    tree = launch_and_compare(plan, hops, 64, 0, None, "an empty hop next to a constant one")
    assert not tree[:, 1].any()
