"""GPU suite: the entry points of the recomputing hop attention agree with each other, bit for bit.

The forward kernels (plain, + statistics, bf16 x) wrap ONE segment walk, the dropout forward keeps a copy of it, and the three backward
kernel pairs (fp32, dropout, bf16) wrap ONE row_segment / col_row (h2gcn_amd/csrc/attention_fused.hip.h, attention_backward.hip.h);
what tells the variants apart is compile-time switches inside that text.  A switch wired to the wrong variant shows as a difference between entry points that are
documented to give the same bits, so this suite asserts those equalities on one plan that holds every segment class of the walk:

  * Y of attention_heads, attention_heads_stats, attention_heads_bf16(float32) and attention_heads_stats_bf16(float32), and the
    bfloat16 Y = that Y rounded once;
  * the statistics of attention_heads_stats, attention_heads_stats_bf16 and attention_heads_stats_dropout (the dropout comes after
    the softmax);
  * (dl, dr, dx) of attention_heads_backward on the widened operands and of attention_heads_backward_bf16(float32), and the
    bfloat16 dx = that dx rounded once.

X and G are drawn in fp32 and rounded to bf16, so both element types see the same values; the Y fed to both backwards is the
forward's fp32 Y rounded to bf16.  Nothing here is a new contract: each equality is in the docstring of the method it names."""
import functools

import numpy as np
import pytest
import torch

import spmm_driver as drv
from test_spmm_values_gpu import DEV, THRESHOLDS, make_plan

pytestmark = pytest.mark.gpu

N_COLS = 320                                   # a 257-entry segment fits (hop_from_lengths never references the last column)
# the smallest long_row_threshold above 64 of the sweeps of the recompute suite: 256 today, so 255, 256 and 257 stand twice in BASE and
# the segments of several chunks below the threshold are 65 .. 255
THRESHOLD = min(t for t in THRESHOLDS if t > 64)
RPW = 7                                        # the groups of four rows straddle the waves' row ranges
SLOPE = 0.2
# every class of the walk and its edges: empty, the 16-entry groups, one chunk, several chunks, the long list; then one group of four
# consecutive rows that mixes empty and short segments
BASE = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1] + [0, 3, 0, 16]
COPIES = 12                                    # 252 rows: several row tiles, and the run of four lands on every offset mod 4
FORWARD_SHAPES = [(4, 1), (64, 16), (64, 8), (128, 8), (128, 4), (68, 1), (132, 1), (256, 16), (260, 5)]   # (260, 5): two column passes
BACKWARD_SHAPES = FORWARD_SHAPES[:-1]          # the packed widths 4, 8, 16, 32, head-aligned blocks of 1, 2 and 4; d <= 256


def _lengths(hop):
    rows = []
    for c in range(COPIES):
        k = (5 * c) % len(BASE)
        rows += BASE[k:] + BASE[:k]
    return rows if hop == 0 else rows[::-1]    # hop 1: the same multiset in another row order


@functools.lru_cache(maxsize=None)
def _hops():
    hops = tuple(drv.hop_from_lengths(_lengths(k), N_COLS, seed=71 + k) for k in range(2))
    for k, m in enumerate(hops):
        assert np.array_equal(np.diff(m.indptr), _lengths(k))
    return hops


def _plan():
    return make_plan(_hops(), build_transpose=True, long_row_threshold=THRESHOLD, rows_per_wave=RPW)


def _bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(DEV)


@functools.lru_cache(maxsize=None)
def _operands(d, k):
    """x and g as bf16 (their fp32 forms: .float()), l and r fp32."""
    rng = np.random.default_rng(1000 * d + k)
    n_rows = len(_lengths(0))
    x = _bf16(rng.uniform(-1, 1, (N_COLS, d)).astype(np.float32))
    g = _bf16(rng.uniform(-1, 1, (n_rows, 2, d)).astype(np.float32))
    l = torch.from_numpy(rng.uniform(-2, 2, (n_rows, 2, k)).astype(np.float32)).to(DEV)
    r = torch.from_numpy(rng.uniform(-2, 2, (N_COLS, 2, k)).astype(np.float32)).to(DEV)
    return x, g, l, r


@functools.lru_cache(maxsize=None)
def _forward(d, k):
    """(Y, stats) of attention_heads_stats on the widened x: computed once per shape, for both tests."""
    x, _, l, r = _operands(d, k)
    with torch.no_grad():
        return _plan().attention_heads_stats(x.float(), l, r, SLOPE)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@pytest.mark.parametrize("d,k", FORWARD_SHAPES)
def test_forward_entry_points_agree(d, k):
    plan = _plan()
    x, _, l, r = _operands(d, k)
    y, stats = _forward(d, k)
    with torch.no_grad():
        assert _same(plan.attention_heads(x.float(), l, r, SLOPE), y), "attention_heads / attention_heads_stats: Y"
        assert _same(plan.attention_heads_bf16(x, l, r, SLOPE, out_dtype=torch.float32), y), "attention_heads_bf16(float32): Y"
        y_s16, stats16 = plan.attention_heads_stats_bf16(x, l, r, SLOPE, out_dtype=torch.float32)
        assert _same(y_s16, y), "attention_heads_stats_bf16(float32): Y"
        assert _same(stats16, stats), "attention_heads_stats_bf16: stats"
        y16 = y.to(torch.bfloat16)
        assert _same(plan.attention_heads_bf16(x, l, r, SLOPE, out_dtype=torch.bfloat16), y16), "attention_heads_bf16(bfloat16): Y"
        y_b16, stats_b16 = plan.attention_heads_stats_bf16(x, l, r, SLOPE, out_dtype=torch.bfloat16)
        assert _same(y_b16, y16), "attention_heads_stats_bf16(bfloat16): Y"
        assert _same(stats_b16, stats), "attention_heads_stats_bf16(bfloat16): stats"
        _, stats_drop = plan.attention_heads_stats_dropout(x.float(), l, r, 0.5, 1234 + d, negative_slope=SLOPE)
        assert _same(stats_drop, stats), "attention_heads_stats_dropout(keep_prob=0.5): stats"


@pytest.mark.parametrize("d,k", BACKWARD_SHAPES)
def test_backward_entry_points_agree(d, k):
    plan = _plan()
    x, g, l, r = _operands(d, k)
    y, stats = _forward(d, k)
    y16 = y.to(torch.bfloat16)
    with torch.no_grad():
        dl, dr, dx = plan.attention_heads_backward(x.float(), l, r, stats, y16.float(), g.float(), SLOPE)
        dl32, dr32, dx32 = plan.attention_heads_backward_bf16(x, l, r, stats, y16, g, SLOPE, dx_dtype=torch.float32)
        assert _same(dl32, dl) and _same(dr32, dr), "attention_heads_backward_bf16(float32): dl, dr"
        assert _same(dx32, dx), "attention_heads_backward_bf16(float32): dx"
        dl16, dr16, dx16 = plan.attention_heads_backward_bf16(x, l, r, stats, y16, g, SLOPE, dx_dtype=torch.bfloat16)
        assert _same(dl16, dl) and _same(dr16, dr), "attention_heads_backward_bf16(bfloat16): dl, dr"
        assert _same(dx16, dx.to(torch.bfloat16)), "attention_heads_backward_bf16(bfloat16): dx"
