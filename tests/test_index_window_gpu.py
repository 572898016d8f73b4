"""GPU suite: the index window of the tile walk (h2gcn_amd/csrc/spmm_kernels.hip.h, window_tile_walk).

A wave of the tile walk streams the contiguous range of colidx / vals that its consecutive rows cover through an LDS ring, in
blocks that are line-aligned in memory, and hands (column id, value) pairs to the lane groups from there.  None of that may show
in the result: every comparison below is BIT FOR BIT against the canonical-tree oracle (``oracle_spmm_tree_f32``), forward and
adjoint.  What the cases aim at:

* segment lengths around every chunk (64), block (128) and ring (kRingCap, read from the source) boundary, next to empty rows
  and to segments of the long path, with segment starts on every residue of the element index mod 32 (a line of 128 B);
* a row count that is no multiple of a tile, empty rows first and last in a tile, rows_per_wave 1 / 4 / 7, one-hop and
  two-hop selections, the adjoint with ``accumulate``, fp32 and bf16 sources, the plain walk (on the window) and the
  prefetching variant, 128-column slices and the general store (which keep the per-segment fetch);
* hop arrays that are views at element offsets 0 / 1 / 15 / 31 (different ones for colidx and vals) into larger buffers whose
  other elements are POISON: the column id of a row of X that holds NaN (an id in range: a leak is a wrong number, not a
  fault) and the value Inf -- once with the view ending at the buffer's end (partial last line).
"""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import gcn_layer as og

pytestmark = pytest.mark.gpu

N_ROWS, N_COLS = 2003, 4096          # 2003 is no multiple of 4 * rows_per_wave for rows_per_wave 1, 4, 7
POISON_COL = N_COLS - 1              # no entry refers to it; X[POISON_COL] is NaN
RING_CAP = int(re.search(r"constexpr int kRingCap = (\d+);",
                         (Path(__file__).resolve().parents[1] / "h2gcn_amd/csrc/spmm_kernels.hip.h").read_text()).group(1))
SPECIAL = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, RING_CAP - 1, RING_CAP, RING_CAP + 1, 300, 600)
TILE_WALKS = ("wave per segment", "wave per segment + index prefetch")
BF = torch.bfloat16


def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def graph():
    """Two hops [N_ROWS, N_COLS].  Row lengths: the SPECIAL ones at random rows (0 and 1 rarely: the launch must stay a tile walk,
    i.e. fewer than 5 % short segments), 17..80 elsewhere.  Columns go round-robin over [0, POISON_COL), so that the columns'
    degrees -- the segment lengths of the adjoint -- are all about nnz / N_COLS >= 17; three hot columns add adjoint segments of
    129, 255 and 300 entries."""
    hops = []
    for k in range(2):
        rng = np.random.default_rng(100 + k)
        lens = rng.integers(17, 81, N_ROWS)
        special_rows = rng.choice(np.arange(40, N_ROWS - 1), 12 * len(SPECIAL), replace=False)
        for i, r in enumerate(special_rows):
            L = SPECIAL[i % len(SPECIAL)]
            lens[r] = L if L > 1 or i < 2 * len(SPECIAL) else 40
        # empty rows first and last in a tile of 4 * rows_per_wave rows (rows_per_wave 1, 4, 7), and the last row
        lens[[0, 3, 4, 15, 16, 27, 28, N_ROWS - 1]] = 0
        is_special = np.zeros(N_ROWS, bool)
        is_special[special_rows] = True
        hot = {5: rng.choice(np.flatnonzero(~is_special & (lens > 0)), 129, replace=False),
               6: rng.choice(np.flatnonzero(~is_special & (lens > 0)), 255, replace=False),
               7: rng.choice(np.flatnonzero(~is_special & (lens > 0)), 300, replace=False)}
        e = 11 * k
        rows, cols = [], []
        for r in range(N_ROWS):
            c = (e + 11 * np.arange(lens[r])) % POISON_COL if k else (e + np.arange(lens[r])) % POISON_COL
            e += lens[r]
            for h, hr in hot.items():
                if r in hr:
                    c = np.union1d(c, [h])
            rows.append(np.full(len(c), r))
            cols.append(c)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        m = sp.csr_matrix((rng.uniform(-1, 1, len(rows)).astype(np.float32), (rows, cols)), shape=(N_ROWS, N_COLS))
        m.sort_indices()
        got = np.diff(m.indptr)
        assert set(SPECIAL) <= set(got.tolist()), sorted(set(SPECIAL) - set(got.tolist()))
        # the special segments start on every residue of the element index mod 32
        assert len(set((m.indptr[:-1][is_special] % 32).tolist())) == 32
        assert (got <= 16).mean() < 0.05 and got.mean() >= 16
        tl = np.diff(m.T.tocsr().indptr)
        assert (tl <= 16).mean() < 0.05 and tl.mean() >= 16 and tl.max() >= 300
        hops.append(m)
    return hops


@functools.lru_cache(maxsize=None)
def operands(d):
    rng = np.random.default_rng(d)
    x = rng.uniform(-1, 1, (N_COLS, d)).astype(np.float32)
    x[POISON_COL] = np.nan
    w = rng.uniform(-1, 1, (N_ROWS, 2, d)).astype(np.float32)
    return x, w


def bf16_round(a):
    """fp32 array -> the same values rounded to bf16 (as fp32)"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).float().numpy()


@functools.lru_cache(maxsize=None)
def reference(d, thr, bf16=False):
    """(Y, Y of hop 0 alone / hop 1 alone are its slices; dX of both hops, dX of hop 1 alone) in the canonical tree"""
    hops = graph()
    x, w = operands(d)
    if bf16:
        x, w = bf16_round(x), bf16_round(w)
    y = og.gcn_layer_tree(hops, x, long_threshold=thr)
    dx = og.gcn_layer_grad_tree(hops, w, N_COLS, long_threshold=thr)
    dx1 = og.gcn_layer_grad_tree(hops[1:], w[:, 1:], N_COLS, long_threshold=thr)
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    return y, dx, dx1


def same_bits(t, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    if t.dtype == BF:
        return torch.equal(t.cpu().view(torch.int16), want.to(BF).view(torch.int16))
    return torch.equal(t.cpu().view(torch.int32), want.view(torch.int32))


def make_plan(offsets=((0, 0), (0, 0)), tail=64, **kw):
    """HopPlan on views into poisoned buffers: hop k's colidx / vals start offsets[k][0] / offsets[k][1] elements into theirs and
    are followed by `tail` more poison elements."""
    from h2gcn_amd import HopPlan

    rp, ci, va = [], [], []
    for m, (oc, ov) in zip(graph(), offsets):
        cbuf = torch.full((oc + m.nnz + tail,), POISON_COL, dtype=torch.int32, device=dev())
        vbuf = torch.full((ov + m.nnz + tail,), float("inf"), dtype=torch.float32, device=dev())
        assert cbuf.data_ptr() % 128 == 0 and vbuf.data_ptr() % 128 == 0
        cbuf[oc:oc + m.nnz] = torch.from_numpy(m.indices.astype(np.int32)).to(dev())
        vbuf[ov:ov + m.nnz] = torch.from_numpy(m.data).to(dev())
        rp.append(torch.from_numpy(m.indptr.astype(np.int64)).to(dev()))
        ci.append(cbuf[oc:oc + m.nnz])
        va.append(vbuf[ov:ov + m.nnz])
    return HopPlan(rp, ci, va, N_COLS, **kw)


def is_tile_walk(plan, d, **kw):
    return plan.schedule(d, **kw)["segment_walk"] in TILE_WALKS


@pytest.mark.parametrize("thr", [0, 2 * RING_CAP])
@pytest.mark.parametrize("d", [64, 128, 100])
def test_every_segment_length_and_tunable_gives_the_tree(d, thr):
    """Default threshold: 255 is the longest segment of the walk and the ring-sized ones go to the long path next to it; with
    long_row_threshold = 2 * kRingCap the segments of kRingCap - 1, kRingCap, kRingCap + 1 and 300 entries stream through a
    ring that is no larger than themselves."""
    y, dx, dx1 = reference(d, thr if thr else 256)
    x, w = operands(d)
    xt, wt = torch.from_numpy(x).to(dev()), torch.from_numpy(w).to(dev())
    base = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (N_COLS, d)).astype(np.float32))
    for rpw in (1, 4, 7):
        for variant in (3, 2):   # plain walk / index prefetch (PIPE)
            for sc in (0, 128) if rpw == 4 else (0,):
                plan = make_plan(offsets=((rpw, 31 - rpw), (15, 0)), build_transpose=True, long_row_threshold=thr, rows_per_wave=rpw,
                                 variant=variant, slice_cols=sc)
                where = (rpw, variant, sc)
                assert is_tile_walk(plan, d) and is_tile_walk(plan, d, adjoint=True), (where, plan.schedule(d), plan.schedule(d, adjoint=True))
                assert same_bits(plan.spmm(xt), y), where
                assert same_bits(plan.spmm(xt, hops=[0]), y[:, :1]), (where, "hops=[0]")
                assert same_bits(plan.spmm(xt, hops=[1]), y[:, 1:]), (where, "hops=[1]")
                assert same_bits(plan.spmm_t(wt), dx), (where, "adjoint")
                assert same_bits(plan.spmm_t(wt[:, 1:], hops=[1]), dx1), (where, "adjoint, hops=[1]")
                out = base.to(dev())
                plan.spmm_t(wt, out=out, accumulate=True)
                assert same_bits(out, dx + base.numpy()), (where, "adjoint, accumulate")


@pytest.mark.parametrize("d", [64, 128, 100])
def test_bf16_sources_give_the_tree_of_the_upcast_operand(d):
    y, dx, _ = reference(d, 256, bf16=True)
    x, w = operands(d)
    xb, wb = torch.from_numpy(x).to(dev()).to(BF), torch.from_numpy(w).to(dev()).to(BF)
    for rpw, variant in ((0, 0), (1, 2), (7, 3)):
        plan = make_plan(offsets=((31, 1), (1, 15)), build_transpose=True, rows_per_wave=rpw, variant=variant)
        where = (rpw, variant)
        assert is_tile_walk(plan, d) and is_tile_walk(plan, d, adjoint=True), where
        assert same_bits(plan.spmm(xb, out_dtype=torch.float32), y), where
        assert same_bits(plan.spmm(xb), y), (where, "bf16 out")
        assert same_bits(plan.spmm_t(wb, out_dtype=torch.float32), dx), (where, "adjoint")
        assert same_bits(plan.spmm_t(wb), dx), (where, "adjoint, bf16 out")


@pytest.mark.parametrize("tail", [64, 0])
@pytest.mark.parametrize("off", [0, 1, 15, 31])
def test_views_into_poisoned_buffers(off, tail):
    """The arrays of a hop start `off` elements (colidx) and another offset of the set (vals) past a line boundary; everything
    around them is poison.  tail = 0: the views end where the buffers end, so the last line of each is partial.  (What this can
    show is a poison element that is CONSUMED; an element that is read and dropped changes no number, and the allocator rounds
    buffers up, so that no lane reads outside [0, nnz) rests on block_load's element-wise bounds, not on this test.)"""
    d = 128
    y, _, _ = reference(d, 256)
    x, _ = operands(d)
    xt = torch.from_numpy(x).to(dev())
    other = {0: 31, 1: 0, 15: 1, 31: 15}[off]
    for variant in (3, 2):
        plan = make_plan(offsets=((off, other), (other, off)), tail=tail, variant=variant)
        assert is_tile_walk(plan, d)
        assert same_bits(plan.spmm(xt), y), variant
        assert same_bits(plan.spmm(xt.to(BF), out_dtype=torch.float32), reference(d, 256, bf16=True)[0]), (variant, "bf16")
    plan = make_plan(offsets=((off, off), (off, off)), tail=tail, rows_per_wave=7)
    assert same_bits(plan.spmm(xt, hops=[1]), y[:, 1:])


def test_three_hop_plan_next_to_the_window():
    """A selection of 3 hops is more than the rings are sized for and keeps the per-segment fetch inside the same kernels; the
    1- and 2-hop selections of the same plan run on the window.  All of them give the tree."""
    from h2gcn_amd import HopPlan

    d = 128
    h = graph()
    hops = [h[0], h[1], h[0]]
    x, w = operands(d)
    w3 = np.concatenate([w, w[:, :1]], axis=1)
    y = og.gcn_layer_tree(hops, x, long_threshold=256)
    dx = og.gcn_layer_grad_tree(hops, w3, N_COLS, long_threshold=256)
    dx02 = og.gcn_layer_grad_tree([h[0], h[0]], w3[:, [0, 2]], N_COLS, long_threshold=256)
    xt, wt = torch.from_numpy(x).to(dev()), torch.from_numpy(w3).to(dev())
    plan = HopPlan.from_scipy(hops, dev(), build_transpose=True, variant=3)
    assert is_tile_walk(plan, d) and is_tile_walk(plan, d, adjoint=True)
    assert same_bits(plan.spmm(xt), y)
    assert same_bits(plan.spmm(xt, hops=[0, 2]), y[:, [0, 2]])
    assert same_bits(plan.spmm(xt, hops=[1]), y[:, 1:2])
    assert same_bits(plan.spmm_t(wt), dx)
    assert same_bits(plan.spmm_t(wt[:, [0, 2]].contiguous(), hops=[0, 2]), dx02)
