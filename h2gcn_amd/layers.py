"""GCNLayer -- torch mirror of the reference's hop-aggregation layer, running on libh2gcn_hip.so.

Reference: ``GCNLayer`` in ``h2gcn/models/_layers.py:54-81``: ``SIGNATURE = ["adjhops", "inputs"]``, stateless,
``layer(adjhops, inputs) -> stack([A_k @ inputs for k in hops], axis=-2)`` of shape ``[N, H_sel, d]``; invoked
by the model interpreter as ``layer(adjhops, inputs)`` (``h2gcn/models/H2GCN.py:318-319``).  Differences by
design: ``adjhops`` is a :class:`h2gcn_amd.hops.HopPlan` (the hop list as one device object) and all selected
hops are aggregated by ONE fused kernel launch that writes the stacked layout directly, so the ``tf.stack`` copy
(and the ``nnz*d > 2**31`` column split of ``_layers.py:65-74``) has no counterpart.
"""
from __future__ import annotations

import ctypes
import functools
import os
from dataclasses import dataclass, field
from typing import Iterable, Optional

import torch

from . import _capi
from .hops import HopPlan, RowSelection


class _HopSpMM(torch.autograd.Function):
    """forward: fused multi-hop SpMM; backward: adjoint SpMM on the plan's transposed operands (the gradient
    TF registers for SparseTensorDenseMatMul wrt its dense input).  The gradient wrt the adjacency values is
    :class:`_HopSpMMValues`, reached through ``hop_spmm(..., values=...)``."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, plan: HopPlan, hops):
        ctx.plan = plan
        ctx.hops = hops
        return plan.spmm(x, hops=hops)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        return ctx.plan.spmm_t(grad_out, hops=ctx.hops), None, None


class _HopSpMMValues(torch.autograd.Function):
    """The hop SpMM as a function of the dense input AND of the stored values of the hop matrices: forward -- install the given
    values in the plan (``set_values``), then the fused SpMM; backward -- the adjoint SpMM for the input and the SDDMM launch
    (``HopPlan.sddmm``) for the values of the hops that want a gradient (the other hops are not part of that launch)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, plan: HopPlan, hops, *values):
        for k, v in enumerate(values):
            if v is not None:
                plan.set_values(k, v.detach().contiguous())
        ctx.plan = plan
        ctx.hops = hops
        ctx.sel = tuple(range(plan.n_hops)) if hops is None else hops
        ctx.version = getattr(plan, "values_version", 0)
        ctx.save_for_backward(x)
        return plan.spmm(x, hops=hops)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        plan = ctx.plan
        if getattr(plan, "values_version", 0) != ctx.version:
            raise RuntimeError("the plan's values changed between the forward and the backward of hop_spmm(..., values=...) "
                               "(a set_values call, or another forward with values= on the same plan): the adjoint would run on "
                               "the wrong values.  Run the backward before the plan's values are replaced")
        (x,) = ctx.saved_tensors
        dx = plan.spmm_t(grad_out, hops=ctx.hops) if ctx.needs_input_grad[0] else None
        # values of hop k are argument 3 + k; only selected hops reach the output
        want = [k for k in ctx.sel if ctx.needs_input_grad[3 + k]]
        dvals = [None] * plan.n_hops
        if want:
            # the launch over the wanted hops reads their slots of the gradient: a strided view when some hop is left out
            pos = [ctx.sel.index(k) for k in want]
            g = _hop_slots(grad_out, pos)
            for k, dv in zip(want, plan.sddmm(g, x, hops=want)):
                dvals[k] = dv
        return (dx, None, None, *dvals)


def _hop_slots(grad: torch.Tensor, pos) -> torch.Tensor:
    """``grad[:, pos, :]`` for ascending hop slots ``pos``: a strided view when the slots are evenly spaced, else a copy."""
    steps = {b - a for a, b in zip(pos, pos[1:])}
    if len(steps) <= 1:
        return grad[:, pos[0]:pos[-1] + 1:(steps.pop() if steps else 1), :]
    return grad[:, list(pos), :]


def _check_values(adjhops: HopPlan, inputs: torch.Tensor, values) -> tuple:
    values = tuple(values)
    if len(values) != adjhops.n_hops:
        raise ValueError(f"values must have one entry per hop of the plan ({adjhops.n_hops}; None keeps a hop's current values), got {len(values)}")
    for k, v in enumerate(values):
        if v is None:
            continue
        nnz = adjhops.colidx[k].numel()
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != adjhops.device or tuple(v.shape) != (nnz,):
            what = f"{v.dtype} {tuple(v.shape)} on {v.device}" if isinstance(v, torch.Tensor) else type(v).__name__
            raise ValueError(f"values[{k}] must be a float32 [{nnz}] tensor on {adjhops.device} (one value per stored entry of hop {k}, "
                             f"in the order of colidx[{k}]), got {what}")
    if inputs.requires_grad and torch.is_grad_enabled() and adjhops.has_transpose and not adjhops.keep_permutation:
        raise ValueError("hop_spmm(..., values=...) with inputs that require a gradient: this plan holds transposed operands for the "
                         "adjoint but cannot refresh them for new values.  Build the plan with keep_permutation=True")
    return values


def hop_spmm(adjhops: HopPlan, inputs: torch.Tensor, hops: Optional[Iterable[int]] = None, values=None) -> torch.Tensor:
    """Functional form of :class:`GCNLayer`: ``[n_cols, d] -> [n_rows, H_sel, d]``, differentiable wrt ``inputs``.

    ``values``: optional sequence of ``n_hops`` entries -- per hop a float32 ``[nnz_k]`` tensor on the plan's device (the stored
    values of ``A_k`` in the order of ``colidx[k]``), or ``None`` to keep the plan's current values of that hop.  The result is
    then differentiable wrt these tensors too (learned or signed edge weights, attention coefficients, a per-edge gate): the
    backward computes ``d values[k][e] = sum_c grad[i, s, c] * inputs[j, c]`` over the stored entries with
    :meth:`HopPlan.sddmm`, for the hops whose values require a gradient.  The given values are installed with
    ``plan.set_values(k, values[k].detach().contiguous())``, and the plan KEEPS POINTING AT THEM afterwards, exactly as
    ``set_values`` documents: later launches of the plan use them until they are replaced.  Replacing them between this call
    and its backward raises a ``RuntimeError`` in the backward.  A plan with transposed operands must have been built with
    ``keep_permutation=True`` when ``inputs`` requires a gradient; row-partitioned operands (``ShardedHops``) are not covered.
    ``values=None`` is today's code path, untouched."""
    if values is not None and hasattr(adjhops, "aggregate"):
        raise ValueError("values= is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan, or set the "
                         "shards' values yourself")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    if values is not None:
        return _HopSpMMValues.apply(inputs, adjhops, sel, *_check_values(adjhops, inputs, values))
    if inputs.requires_grad and torch.is_grad_enabled():
        return _HopSpMM.apply(inputs, adjhops, sel)
    return adjhops.spmm(inputs, hops=sel)


class _HopSpMMLaunchValues(torch.autograd.Function):
    """The hop SpMM on values handed to the launch (``HopPlan.spmm_values``), a function of the dense input and of the values of
    the SELECTED hops: forward -- one launch, ``inputs`` and ``values`` saved, nothing installed in the plan; backward -- one
    ``spmm_values_t`` launch for the input, and for the values of the hops that want a gradient ONE ``HopPlan.sddmm_heads`` launch
    when there are heads (``HopPlan.sddmm`` once per head on that head's column slices -- the same bits -- on a library that
    predates it, and for a single head)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, plan: HopPlan, hops, *values):
        ctx.plan, ctx.hops = plan, hops
        ctx.save_for_backward(x, *values)
        return plan.spmm_values(x, values, hops=hops)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        plan = ctx.plan
        x, *values = ctx.saved_tensors
        dx = plan.spmm_values_t(grad_out, values, hops=ctx.hops) if ctx.needs_input_grad[0] else None
        sel = plan._selected(ctx.hops)
        pos = [s for s in range(len(sel)) if ctx.needs_input_grad[3 + s]]
        dvals = [None] * len(sel)
        if pos:
            want = [sel[s] for s in pos]
            g = _hop_slots(grad_out, pos)
            n_heads = 1 if values[0].dim() == 1 else values[0].shape[1]
            w = x.shape[1] // n_heads
            if n_heads > 1 and _capi.has("h2gcn_sddmm_hops_heads_f32"):
                for i, dv in enumerate(plan.sddmm_heads(g, x, n_heads, hops=want)):   # one launch, [nnz_k, K]: the same bits
                    dvals[pos[i]] = dv
                return (dx, None, None, *dvals)
            per_head = [plan.sddmm(g[:, :, h * w:(h + 1) * w], x[:, h * w:(h + 1) * w], hops=want) for h in range(n_heads)]
            for i, s in enumerate(pos):
                dvals[s] = per_head[0][i] if values[s].dim() == 1 else torch.stack([dv[i] for dv in per_head], dim=1)
        return (dx, None, None, *dvals)


def hop_spmm_values(adjhops: HopPlan, inputs: torch.Tensor, values, hops: Optional[Iterable[int]] = None) -> torch.Tensor:
    """The hop aggregation on values that are an ARGUMENT of the call: ``[n_cols, d] -> [n_rows, H_sel, d]`` with
    ``out[i, s, c] = sum_e values[s][e, h(c)] * inputs[j_e, c]`` over the stored entries of row ``i`` of selected hop ``s``,
    ``h(c) = c // (d // K)`` (head ``h`` owns columns ``h*d/K ..``: GAT's concat), differentiable wrt ``inputs`` and ``values``.

    ``values``: one float32 tensor per SELECTED hop -- what :func:`hop_softmax` returns -- each ``[nnz_k]`` or ``[nnz_k, K]`` with
    the same ``K``, in the entry order of ``colidx[k]``; any strides pass through (a ``[K, nnz_k]`` buffer as its ``.t()`` view is
    not copied).  ``K > 1`` needs ``d % K == 0`` and ``(d // K) % 4 == 0``.  Unlike ``hop_spmm(..., values=...)`` NOTHING is
    installed in the plan: its stored values are neither read nor replaced, so any number of such calls -- two attention layers,
    a ``GCNLayer`` between them -- can share one plan and be trained, and a training step can be captured in a hipGraph after one
    eager warm-up.  The bits are those of ``hop_spmm`` on a plan holding the values (per head on the head's column slice).

    Backward: one :meth:`HopPlan.spmm_values_t` launch for ``inputs`` (the plan needs ``build_transpose=True,
    keep_permutation=True``), and :meth:`HopPlan.sddmm` once per head for the values of the hops that want a gradient.
    fp32 only.  Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_spmm_values is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    if isinstance(values, torch.Tensor) or values is None:
        raise ValueError(f"values must be a sequence of {adjhops.n_selected(sel)} tensors (one per selected hop)")
    values = tuple(values)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (inputs, *values)):
        if inputs.requires_grad and not (adjhops.has_transpose and adjhops.keep_permutation):
            raise ValueError("hop_spmm_values with inputs that require a gradient: the adjoint reads the values through the permutation "
                             "of the plan's transposed operands.  Build the plan with HopPlan(..., build_transpose=True, "
                             "keep_permutation=True)")
        # (the argument checks of the launch run first either way: HopPlan.spmm_values refuses before any device work)
        return _HopSpMMLaunchValues.apply(inputs, adjhops, sel, *values)
    return adjhops.spmm_values(inputs, values, hops=sel)


class _HopSoftmax(torch.autograd.Function):
    """The row softmax over the hop pattern: forward -- ONE launch over the selected hops (``HopPlan.row_softmax``), ``alpha``
    saved; backward -- ONE launch over the selected hops (``HopPlan.row_softmax_backward``) on the contiguous incoming gradients
    (a hop nobody differentiated through enters as zeros), ``None`` for a hop whose scores do not require a gradient."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, *scores):
        alpha = plan.row_softmax(scores, hops=hops)
        ctx.plan, ctx.hops = plan, hops
        ctx.save_for_backward(*alpha)
        return tuple(alpha)

    @staticmethod
    def backward(ctx, *grads):
        alpha = ctx.saved_tensors
        if not any(ctx.needs_input_grad[2:]):
            return (None, None) + (None,) * len(alpha)
        grads = [torch.zeros_like(a) if g is None else g.contiguous() for g, a in zip(grads, alpha)]
        dscores = ctx.plan.row_softmax_backward(alpha, grads, hops=ctx.hops)
        return (None, None, *[d if need else None for d, need in zip(dscores, ctx.needs_input_grad[2:])])


def hop_softmax(adjhops: HopPlan, scores, hops: Optional[Iterable[int]] = None) -> tuple:
    """Attention coefficients over the hop pattern: per selected hop ``s`` and row ``i`` the softmax of ``scores[s]`` over the
    stored entries of row ``i`` -- ``alpha[s][e] = exp(scores[s][e] - max) / sum`` -- as a tuple of ``H_sel`` float32 ``[nnz_k]``
    tensors in the entry order of ``colidx[k]``, differentiable wrt ``scores`` (what ``hop_spmm(plan, x, values=list(alpha))``
    takes).  One softmax per hop and row; there is no joint softmax across hops.

    ``scores``: a sequence of ``H_sel`` contiguous float32 ``[nnz_k]`` tensors on the plan's device (bfloat16 scores are refused:
    the kernels are fp32 only).  ``hops``: the hop indices the scores belong to, default all.  Forward and backward are one
    launch each (:meth:`HopPlan.row_softmax` / :meth:`HopPlan.row_softmax_backward`); their bits are a function of each
    segment's own contents.  Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_softmax is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    if isinstance(scores, torch.Tensor) or scores is None:
        raise ValueError(f"scores must be a sequence of {adjhops.n_selected(sel)} tensors (one per selected hop)")
    scores = tuple(scores)
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in scores) and torch.is_grad_enabled():
        # (the argument checks of the launch run first either way: HopPlan.row_softmax refuses before any device work)
        return _HopSoftmax.apply(adjhops, sel, *scores)
    return tuple(adjhops.row_softmax(scores, hops=sel))


class _HopEdgeScores(torch.autograd.Function):
    """The additive edge scores on the hop pattern: forward -- ONE launch over the selected hops (``HopPlan.edge_scores``), ``l``
    and ``r`` saved (the backward recomputes ``pre``); backward -- ONE call (``HopPlan.edge_scores_backward``) on the contiguous
    incoming gradients (a hop nobody differentiated through enters as zeros), for the sides whose input requires a gradient."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, negative_slope: float, l: torch.Tensor, r: torch.Tensor):
        scores = plan.edge_scores(l, r, negative_slope, hops=hops)
        ctx.plan, ctx.hops, ctx.negative_slope = plan, hops, negative_slope
        ctx.save_for_backward(l, r)
        return tuple(scores)

    @staticmethod
    def backward(ctx, *grads):
        need_dl, need_dr = ctx.needs_input_grad[3:5]
        if not (need_dl or need_dr):
            return None, None, None, None, None
        l, r = ctx.saved_tensors
        plan = ctx.plan
        grads = [torch.zeros(plan.colidx[k].numel(), dtype=torch.float32, device=plan.device) if g is None else g.contiguous()
                 for g, k in zip(grads, plan._selected(ctx.hops))]
        dl, dr = plan.edge_scores_backward(l, r, grads, ctx.negative_slope, hops=ctx.hops, need_dl=need_dl, need_dr=need_dr)
        return None, None, None, dl, dr


def hop_edge_scores(adjhops: HopPlan, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2,
                    hops: Optional[Iterable[int]] = None) -> tuple:
    """Additive (GAT-style) attention scores over the hop pattern: ``scores[s][e] = leaky_relu(l[i, s] + r[j, s], negative_slope)``
    for every stored entry ``e = (i, j)`` of selected hop ``s``, as a tuple of ``H_sel`` float32 ``[nnz_k]`` tensors in the entry
    order of ``colidx[k]`` (what :func:`hop_softmax` takes), differentiable wrt ``l`` and ``r``.  There is no row-of-entry index,
    no gather and no ``index_add``: forward and backward are one call each (:meth:`HopPlan.edge_scores` /
    :meth:`HopPlan.edge_scores_backward`), and the backward is free of atomics -- its bits are reproducible.

    ``l`` ``[n_rows, H_sel]``, ``r`` ``[n_cols, H_sel]``: float32 on the plan's device (1-D when one hop is selected; bfloat16 is
    refused: the kernels are fp32 only).  The backward computes only the sides whose input requires a gradient.  A gradient for
    ``r`` sums over the columns of the hop matrices: the plan must have been built with ``build_transpose=True,
    keep_permutation=True`` (what ``hop_spmm(..., values=...)`` asks of a differentiable input already).  Row-partitioned
    operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_edge_scores is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    grads = [isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled() for t in (l, r)]
    if grads[1] and not (adjhops.has_transpose and adjhops.keep_permutation):
        raise ValueError("hop_edge_scores with an r that requires a gradient: that gradient sums over the columns of the hop matrices, "
                         "on the plan's transposed operands through their permutation.  Build the plan with "
                         "HopPlan(..., build_transpose=True, keep_permutation=True)")
    if any(grads):
        # (the argument checks of the launch run first either way: HopPlan.edge_scores refuses before any device work)
        return _HopEdgeScores.apply(adjhops, sel, float(negative_slope), l, r)
    return tuple(adjhops.edge_scores(l, r, negative_slope, hops=sel))


class _HopSoftmaxHeads(torch.autograd.Function):
    """:class:`_HopSoftmax` on entry-major ``[nnz_k, K]`` arrays: one launch forward (``HopPlan.row_softmax_heads``), one backward."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, *scores):
        alpha = plan.row_softmax_heads(scores, hops=hops)
        ctx.plan, ctx.hops = plan, hops
        ctx.save_for_backward(*alpha)
        return tuple(alpha)

    @staticmethod
    def backward(ctx, *grads):
        alpha = ctx.saved_tensors
        if not any(ctx.needs_input_grad[2:]):
            return (None, None) + (None,) * len(alpha)
        grads = [torch.zeros_like(a) if g is None else g.contiguous() for g, a in zip(grads, alpha)]
        dscores = ctx.plan.row_softmax_heads_backward(alpha, grads, hops=ctx.hops)
        return (None, None, *[d if need else None for d, need in zip(dscores, ctx.needs_input_grad[2:])])


def hop_softmax_heads(adjhops: HopPlan, scores, hops: Optional[Iterable[int]] = None) -> tuple:
    """:func:`hop_softmax` for ``K`` heads at once: ``scores`` is a sequence of ``H_sel`` contiguous float32 ``[nnz_k, K]`` tensors
    (entry-major: what :func:`hop_edge_scores_heads` returns), the result a tuple of ``[nnz_k, K]`` coefficients -- one softmax per
    hop, row and head -- that :func:`hop_spmm_values` takes as they are.  Forward and backward are one launch each
    (:meth:`HopPlan.row_softmax_heads` / :meth:`HopPlan.row_softmax_heads_backward`); per head the bits are those of
    :func:`hop_softmax` on that column.  fp32 only.  Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_softmax_heads is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    if isinstance(scores, torch.Tensor) or scores is None:
        raise ValueError(f"scores must be a sequence of {adjhops.n_selected(sel)} tensors (one per selected hop)")
    scores = tuple(scores)
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in scores) and torch.is_grad_enabled():
        # (the argument checks of the launch run first either way: HopPlan.row_softmax_heads refuses before any device work)
        return _HopSoftmaxHeads.apply(adjhops, sel, *scores)
    return tuple(adjhops.row_softmax_heads(scores, hops=sel))


class _HopEdgeScoresHeads(torch.autograd.Function):
    """:class:`_HopEdgeScores` with heads: one launch forward (``HopPlan.edge_scores_heads``), one call backward."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, negative_slope: float, l: torch.Tensor, r: torch.Tensor):
        scores = plan.edge_scores_heads(l, r, negative_slope, hops=hops)
        ctx.plan, ctx.hops, ctx.negative_slope = plan, hops, negative_slope
        ctx.save_for_backward(l, r)
        return tuple(scores)

    @staticmethod
    def backward(ctx, *grads):
        need_dl, need_dr = ctx.needs_input_grad[3:5]
        if not (need_dl or need_dr):
            return None, None, None, None, None
        l, r = ctx.saved_tensors
        plan = ctx.plan
        grads = [torch.zeros((plan.colidx[k].numel(), l.shape[2]), dtype=torch.float32, device=plan.device) if g is None
                 else g.contiguous() for g, k in zip(grads, plan._selected(ctx.hops))]
        dl, dr = plan.edge_scores_heads_backward(l, r, grads, ctx.negative_slope, hops=ctx.hops, need_dl=need_dl, need_dr=need_dr)
        return None, None, None, dl, dr


def hop_edge_scores_heads(adjhops: HopPlan, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2,
                          hops: Optional[Iterable[int]] = None) -> tuple:
    """:func:`hop_edge_scores` for ``K`` heads at once: ``scores[s][e, h] = leaky_relu(l[i, s, h] + r[j, s, h], negative_slope)`` as
    a tuple of ``H_sel`` contiguous float32 ``[nnz_k, K]`` tensors (what :func:`hop_softmax_heads` takes), differentiable wrt ``l``
    ``[n_rows, H_sel, K]`` and ``r`` ``[n_cols, H_sel, K]`` (float32; bfloat16 is refused).  Forward and backward are one call each
    (:meth:`HopPlan.edge_scores_heads` / :meth:`HopPlan.edge_scores_heads_backward`), free of atomics; per head the bits are those
    of :func:`hop_edge_scores` on ``l[:, :, h]``, ``r[:, :, h]``.  A gradient for ``r`` needs a plan built with
    ``build_transpose=True, keep_permutation=True``.  Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_edge_scores_heads is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    grads = [isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled() for t in (l, r)]
    if grads[1] and not (adjhops.has_transpose and adjhops.keep_permutation):
        raise ValueError("hop_edge_scores_heads with an r that requires a gradient: that gradient sums over the columns of the hop "
                         "matrices, on the plan's transposed operands through their permutation.  Build the plan with "
                         "HopPlan(..., build_transpose=True, keep_permutation=True)")
    if any(grads):
        # (the argument checks of the launch run first either way: HopPlan.edge_scores_heads refuses before any device work)
        return _HopEdgeScoresHeads.apply(adjhops, sel, float(negative_slope), l, r)
    return tuple(adjhops.edge_scores_heads(l, r, negative_slope, hops=sel))


class _HopEdgeScoresDynamic(torch.autograd.Function):
    """The dynamic (GATv2) edge scores: one launch forward (``HopPlan.edge_scores_dynamic``), one call backward.  ``u``, ``v``, ``a``
    are saved; ``u + v`` and its leaky_relu are recomputed per entry in the backward: nothing of size ``nnz x d`` is kept."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, heads: int, negative_slope: float, u: torch.Tensor, v: torch.Tensor, a: torch.Tensor):
        scores = plan.edge_scores_dynamic(u, v, a, heads, negative_slope, hops=hops)
        ctx.plan, ctx.hops, ctx.heads, ctx.negative_slope = plan, hops, heads, negative_slope
        ctx.save_for_backward(u, v, a)
        return tuple(scores)

    @staticmethod
    def backward(ctx, *grads):
        need_du, need_dv, need_da = ctx.needs_input_grad[4:7]
        if not (need_du or need_dv or need_da):
            return (None,) * 7
        u, v, a = ctx.saved_tensors
        plan = ctx.plan
        shape = (lambda k: (plan.colidx[k].numel(),) + (() if ctx.heads == 1 else (ctx.heads,)))
        # (a hop nobody differentiated through enters as zeros)
        grads = [torch.zeros(shape(k), dtype=torch.float32, device=plan.device) if g is None else g.contiguous()
                 for g, k in zip(grads, plan._selected(ctx.hops))]
        du, dv, da = plan.edge_scores_dynamic_backward(u, v, a, grads, ctx.heads, ctx.negative_slope, hops=ctx.hops, need_du=need_du,
                                                       need_dv=need_dv, need_da=need_da)
        return None, None, None, None, du, dv, None if da is None else da.view(a.shape)


def hop_edge_scores_dynamic(adjhops: HopPlan, u: torch.Tensor, v: torch.Tensor, a: torch.Tensor, heads: int = 1, negative_slope: float = 0.2,
                            hops: Optional[Iterable[int]] = None) -> tuple:
    """Dynamic (GATv2) attention scores: ``scores[s][e, h] = sum_{c in head h} a[s, c] * leaky_relu(u[i, c] + v[j, c], negative_slope)``
    for every stored entry ``e = (i, j)`` of selected hop ``s``, as a tuple of ``H_sel`` contiguous float32 ``[nnz_k, K]`` tensors
    (``[nnz_k]`` for ``heads == 1``: what :func:`hop_softmax_heads` / :func:`hop_softmax` take), differentiable wrt ``u``
    ``[n_rows, d]``, ``v`` ``[n_cols, d]`` and ``a`` ``[H_sel, d]`` (or ``[H_sel, K, d // K]``).  Where :func:`hop_edge_scores_heads`
    ranks the neighbours of every row by ``r[j]`` alone, here the ranking depends on the row.  Forward and backward are one call each
    (:meth:`HopPlan.edge_scores_dynamic` / :meth:`HopPlan.edge_scores_dynamic_backward`): ``u + v`` is recomputed per entry and no
    ``nnz x d`` array exists in either direction, which is why this is never run as a composite of torch operations; ``d > 256`` is
    a ``ValueError``.  A gradient for ``v`` needs a plan built with ``build_transpose=True, keep_permutation=True``.  float32 only.
    Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_edge_scores_dynamic is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    if isinstance(u, torch.Tensor) and u.dim() == 2 and u.shape[1] > HopPlan.EDGE_SCORES_DYNAMIC_MAX_WIDTH:
        raise ValueError(f"hop_edge_scores_dynamic serves widths up to EDGE_SCORES_DYNAMIC_MAX_WIDTH = {HopPlan.EDGE_SCORES_DYNAMIC_MAX_WIDTH}, "
                         f"got d = {u.shape[1]}")
    grads = [isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled() for t in (u, v, a)]
    if grads[1] and not (adjhops.has_transpose and adjhops.keep_permutation):
        raise ValueError("hop_edge_scores_dynamic with a v that requires a gradient: that gradient sums over the columns of the hop "
                         "matrices, on the plan's transposed operands through their permutation.  Build the plan with "
                         "HopPlan(..., build_transpose=True, keep_permutation=True)")
    if any(grads):
        # (the argument checks of the launch run first either way: HopPlan.edge_scores_dynamic refuses before any device work)
        return _HopEdgeScoresDynamic.apply(adjhops, sel, int(heads), float(negative_slope), u, v, a)
    return tuple(adjhops.edge_scores_dynamic(u, v, a, heads, negative_slope, hops=sel))


def hop_attention_heads(adjhops: HopPlan, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2,
                        hops: Optional[Iterable[int]] = None) -> torch.Tensor:
    """Multi-head attention over the hop pattern, scores to aggregation: ``[n_cols, d] -> [n_rows, H_sel, d]`` with
    ``out[i, s, c] = sum_e alpha_s[e, h(c)] * inputs[j_e, c]``, ``alpha_s[:, h]`` the softmax over row ``i`` of
    ``leaky_relu(l[i, s, h] + r[j, s, h], negative_slope)`` and ``h(c) = c // (d // K)`` -- what
    ``hop_spmm_values(plan, inputs, hop_softmax_heads(plan, hop_edge_scores_heads(plan, l, r, slope, hops), hops), hops)`` computes.

    When gradients are disabled, or none of ``inputs``, ``l``, ``r`` requires one, this is ONE launch
    (:meth:`HopPlan.attention_heads`) that allocates nothing but its result: the two ``[nnz_k, K]`` arrays per hop of the chain
    never exist.  Otherwise it IS the expression above, so the result is always differentiable, and it always has the same bits:
    the launch reproduces the chain's arithmetic bit for bit.  For the same reason ``K > 16`` (which the launch refuses) and a
    library that predates the launch take the chain as well, whatever the gradient mode.

    ``l`` ``[n_rows, H_sel, K]``, ``r`` ``[n_cols, H_sel, K]``, ``inputs`` ``[n_cols, d]``: float32 on the plan's device;
    ``K > 1`` needs ``d % K == 0`` and ``(d // K) % 4 == 0``.  Row-partitioned operands (``ShardedHops``) are not covered."""
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_attention_heads is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    wants_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (inputs, l, r))
    n_heads = int(l.shape[2]) if isinstance(l, torch.Tensor) and l.dim() == 3 else 1
    if isinstance(inputs, torch.Tensor) and inputs.dtype == torch.bfloat16:   # (bf16 embeddings: one launch, or a refusal)
        if wants_grad:
            raise ValueError("hop_attention_heads with bfloat16 inputs that need a gradient: the chain is float32 only -- call "
                             "hop_attention_recompute, whose training step has bf16 launches")
        _bf16_attention_limits("hop_attention_heads", inputs, n_heads, False)
        return adjhops.attention_heads_bf16(inputs, l, r, negative_slope, hops=sel)
    if wants_grad or n_heads > HopPlan.ATTENTION_FUSED_MAX_HEADS or not _capi.has("h2gcn_attention_hops_heads_f32"):
        scores = hop_edge_scores_heads(adjhops, l, r, negative_slope, sel)
        return hop_spmm_values(adjhops, inputs, hop_softmax_heads(adjhops, scores, sel), sel)
    return adjhops.attention_heads(inputs, l, r, negative_slope, hops=sel)


class _HopAttentionRecompute(torch.autograd.Function):
    """The attention over the hop pattern as TWO launches that keep no per-entry array: the forward stores ``y`` and the softmax
    statistics (``HopPlan.attention_heads_stats``), the backward computes every per-entry quantity again from ``x, l, r, stats, y``
    (``HopPlan.attention_heads_backward``)."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, negative_slope: float, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor,
                keep_prob: float = 1.0, seed: int = 0, step_dev: Optional[torch.Tensor] = None):
        if keep_prob >= 1.0:   # (without dropout: today's calls, argument for argument)
            y, stats = plan.attention_heads_stats(inputs, l, r, negative_slope, hops=hops)
        else:
            y, stats = plan.attention_heads_stats_dropout(inputs, l, r, float(keep_prob), int(seed), step_dev, negative_slope, hops=hops)
        ctx.plan, ctx.hops, ctx.negative_slope = plan, hops, negative_slope
        ctx.keep_prob, ctx.seed, ctx.has_step = float(keep_prob), int(seed), step_dev is not None
        # (the mask is not stored: the backward draws it again from the same (seed, step))
        ctx.save_for_backward(inputs, l, r, stats, y, _saved_step(step_dev, inputs.device))
        return y

    @staticmethod
    def backward(ctx, grad):
        need_dx, need_dl, need_dr = ctx.needs_input_grad[3:6]
        if not (need_dx or need_dl or need_dr):
            return None, None, None, None, None, None, None, None, None
        inputs, l, r, stats, y, step = ctx.saved_tensors
        if ctx.keep_prob >= 1.0:
            dl, dr, dx = ctx.plan.attention_heads_backward(inputs, l, r, stats, y, grad, ctx.negative_slope, hops=ctx.hops, need_dl=need_dl,
                                                           need_dr=need_dr, need_dx=need_dx)
        else:
            dl, dr, dx = ctx.plan.attention_heads_backward_dropout(inputs, l, r, stats, y, grad, ctx.keep_prob, ctx.seed,
                                                                   step if ctx.has_step else None, ctx.negative_slope, hops=ctx.hops,
                                                                   need_dl=need_dl, need_dr=need_dr, need_dx=need_dx)
        return None, None, None, dx, dl, dr, None, None, None


def _bf16_attention_limits(what: str, inputs: torch.Tensor, n_heads: int, wants_grad: bool) -> None:
    """What the bf16 attention launches do not cover is refused, never run in float32 instead (the model's rule for
    ``--embedding_dtype``): each a ``ValueError`` naming the limit."""
    d = int(inputs.shape[1]) if inputs.dim() == 2 else 1
    if n_heads > HopPlan.ATTENTION_FUSED_MAX_HEADS:
        raise ValueError(f"{what} with bfloat16 inputs serves at most K = {HopPlan.ATTENTION_FUSED_MAX_HEADS} heads, got K = {n_heads}: the "
                         "chain that serves more is float32 only")
    if wants_grad and d > HopPlan.ATTENTION_RECOMPUTE_MAX_WIDTH:
        raise ValueError(f"{what} with bfloat16 inputs that need a gradient serves at most d = {HopPlan.ATTENTION_RECOMPUTE_MAX_WIDTH} columns, "
                         f"got d = {d}: the chain that serves more is float32 only")
    if d % 2:
        raise ValueError(f"{what} with bfloat16 inputs needs an even width (a lane stores bf16 pairs), got d = {d}")
    missing = [s for s in HopPlan.BF16_ATTENTION_SYMBOLS if not _capi.has(s)]
    if missing:
        raise ValueError(f"{what} with bfloat16 inputs: {_capi.library_path()} predates the bf16 attention launches ({', '.join(missing)}): "
                         "rebuild it")


class _HopAttentionRecomputeBf16(torch.autograd.Function):
    """:class:`_HopAttentionRecompute` on bfloat16 embeddings: the forward stores a bfloat16 ``y`` and the float32 statistics
    (``HopPlan.attention_heads_stats_bf16``), the backward takes a bfloat16 ``grad`` and returns a bfloat16 ``dx`` and float32
    ``dl``, ``dr`` (``HopPlan.attention_heads_backward_bf16``).  What is kept for the backward -- ``x`` and ``y`` -- is 2-byte."""

    @staticmethod
    def forward(ctx, plan: HopPlan, hops, negative_slope: float, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor):
        y, stats = plan.attention_heads_stats_bf16(inputs, l, r, negative_slope, hops=hops)
        ctx.plan, ctx.hops, ctx.negative_slope = plan, hops, negative_slope
        ctx.save_for_backward(inputs, l, r, stats, y)
        return y

    @staticmethod
    def backward(ctx, grad):
        need_dx, need_dl, need_dr = ctx.needs_input_grad[3:6]
        if not (need_dx or need_dl or need_dr):
            return None, None, None, None, None, None
        inputs, l, r, stats, y = ctx.saved_tensors
        # (a grad of another layout is copied to the bf16 layout rule by the plan method)
        dl, dr, dx = ctx.plan.attention_heads_backward_bf16(inputs, l, r, stats, y, grad.to(torch.bfloat16), ctx.negative_slope, hops=ctx.hops,
                                                            need_dl=need_dl, need_dr=need_dr, need_dx=need_dx, dx_dtype=torch.bfloat16)
        return None, None, None, dx, dl, dr


def _dropped_chain(adjhops: HopPlan, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float, sel, keep_prob: float,
                   seed: int, step) -> torch.Tensor:
    """The chain of :func:`hop_attention_heads` with dropout on its coefficients: ``alpha_k * f_k``, ``f_k`` the factor arrays of
    :meth:`HopPlan.attention_dropout_factors` -- the mask the fused launches draw, and the forward bits of the fused launch."""
    n_heads = int(l.shape[2]) if isinstance(l, torch.Tensor) and l.dim() == 3 else 1
    if n_heads > HopPlan.ATTENTION_FUSED_MAX_HEADS:
        raise ValueError(f"attention dropout serves at most K = {HopPlan.ATTENTION_FUSED_MAX_HEADS} heads (the generator has one word per "
                         f"pair of heads, eight per entry), got K = {n_heads}")
    alpha = hop_softmax_heads(adjhops, hop_edge_scores_heads(adjhops, l, r, negative_slope, sel), sel)
    factors = adjhops.attention_dropout_factors(n_heads, keep_prob, seed, step, hops=sel)
    return hop_spmm_values(adjhops, inputs, [a * f for a, f in zip(alpha, factors)], sel)


def hop_attention_recompute(adjhops: HopPlan, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2,
                            hops: Optional[Iterable[int]] = None) -> torch.Tensor:
    """:func:`hop_attention_heads` whose TRAINING step keeps no per-entry array: what that function computes, ``[n_cols, d] ->
    [n_rows, H_sel, d]``, differentiable wrt ``inputs``, ``l`` and ``r``.

    With a gradient the forward is ONE launch that stores the result and the softmax statistics ``[n_rows, H_sel, 2, K]``
    (:meth:`HopPlan.attention_heads_stats`), the backward ONE call that computes the scores, coefficients and their gradients again
    per entry (:meth:`HopPlan.attention_heads_backward`): no ``[nnz_k, K]`` array is written, read or allocated in either.  The
    forward has the chain's bits; the gradients are deterministic but have summation orders of their own (include/h2gcn_hip.h), so
    they agree with the chain's to rounding, not bit for bit.  Without a gradient this is :meth:`HopPlan.attention_heads`.

    A gradient for ``inputs`` or ``r`` sums over the columns of the hop matrices: the plan needs ``build_transpose=True`` (no
    permutation: ``keep_permutation`` is not needed; a ``symmetric_pattern=True`` plan serves too).  ``K > 16``, ``d > 256`` and a
    library that predates the two launches take :func:`hop_attention_heads`, the chain.  fp32 only.  Row-partitioned operands
    (``ShardedHops``) are not covered.

    bfloat16 ``inputs`` (``l`` and ``r`` stay float32) run the bf16 launches (:meth:`HopPlan.attention_heads_stats_bf16`,
    :meth:`HopPlan.attention_heads_backward_bf16`; without a gradient :meth:`HopPlan.attention_heads_bf16`): the result and the
    gradient of ``inputs`` are bfloat16, the float32 launches' values on the upcast operands rounded once to nearest even.  What those
    launches do not cover -- ``K > 16``, ``d > 256`` under a gradient, an odd ``d``, a library without them -- is a ``ValueError``:
    bf16 embeddings are never run in float32 instead (the chain is float32 only).

    :func:`hop_attention_recompute_dropout` is this step with dropout on the attention coefficients."""
    return _hop_attention_recompute(adjhops, inputs, l, r, negative_slope, hops, 0.0, 0, None)


def hop_attention_recompute_dropout(adjhops: HopPlan, inputs: torch.Tensor, l: torch.Tensor, r: torch.Tensor, dropout: float, seed: int = 0,
                                    step: Optional[torch.Tensor] = None, negative_slope: float = 0.2,
                                    hops: Optional[Iterable[int]] = None) -> torch.Tensor:
    """:func:`hop_attention_recompute` with dropout on the attention coefficients; operands and limits as there.

    ``dropout`` in ``[0, 1)``: dropout on the attention coefficients (GAT's ``attn_drop``) -- every coefficient is kept with
    probability ``1 - dropout`` and scaled by ``1 / (1 - dropout)``.  The mask is a counter-based function of ``(seed, step, hop, row,
    column, head)`` drawn INSIDE the forward and backward kernels (include/h2gcn_hip.h): still no ``[nnz_k, K]`` array, and the
    backward redraws the forward's mask from the same ``(seed, step)``.  ``step``: a 1-element int64 tensor on the plan's device (read
    when the kernels run, so a replayed hipGraph that bumps it draws a fresh mask; it must not change between a forward and its
    backward -- pass a clone), or ``None`` for step 0.  It is applied whenever ``dropout > 0``, with or without a gradient: switching it
    off for evaluation is the caller's (the layers do it).  ``d > 256`` and a library that predates the fused launches run the chain on
    ``alpha_k * f_k`` with the factor arrays of :meth:`HopPlan.attention_dropout_factors`: the same mask, and the fused launch's forward
    bits; ``K > 16`` with dropout is refused.  ``dropout = 0`` is :func:`hop_attention_recompute`, call for call."""
    return _hop_attention_recompute(adjhops, inputs, l, r, negative_slope, hops, dropout, seed, step)


def _hop_attention_recompute(adjhops, inputs, l, r, negative_slope, hops, dropout, seed, step) -> torch.Tensor:
    dropout = float(dropout)
    if not 0.0 <= dropout < 1.0:
        raise ValueError(f"dropout = {dropout} outside [0, 1)")
    if hasattr(adjhops, "aggregate"):
        raise ValueError("hop_attention_recompute is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
    if not isinstance(adjhops, HopPlan):
        raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
    sel = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
    grads = [torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad for t in (inputs, l, r)]
    n_heads = int(l.shape[2]) if isinstance(l, torch.Tensor) and l.dim() == 3 else 1
    d = int(inputs.shape[1]) if isinstance(inputs, torch.Tensor) and inputs.dim() == 2 else 1
    if isinstance(inputs, torch.Tensor) and inputs.dtype == torch.bfloat16:   # (bf16 embeddings: the bf16 launches, or a refusal)
        if dropout > 0.0:
            raise ValueError(f"hop_attention_recompute_dropout(dropout={dropout}) with bfloat16 inputs: the attention dropout launches are "
                             "float32 only")
        _bf16_attention_limits("hop_attention_recompute", inputs, n_heads, any(grads))
        if not any(grads):
            return adjhops.attention_heads_bf16(inputs, l, r, negative_slope, hops=sel)
        if (grads[0] or grads[2]) and not adjhops.has_transpose:
            raise ValueError("hop_attention_recompute with inputs or an r that require a gradient: those gradients sum over the columns of the "
                             "hop matrices, on the plan's transposed operands (their permutation is not needed).  Build the plan with "
                             "HopPlan(..., build_transpose=True)")
        return _HopAttentionRecomputeBf16.apply(adjhops, sel, float(negative_slope), inputs, l, r)
    if (n_heads > HopPlan.ATTENTION_FUSED_MAX_HEADS or d > HopPlan.ATTENTION_RECOMPUTE_MAX_WIDTH
            or not all(_capi.has(s) for s in HopPlan._RECOMPUTE_SYMBOLS)):
        if dropout > 0.0:
            return _dropped_chain(adjhops, inputs, l, r, negative_slope, sel, 1.0 - dropout, seed, step)
        return hop_attention_heads(adjhops, inputs, l, r, negative_slope, sel)
    if not any(grads):
        if dropout > 0.0:   # (the mask applies without a gradient too: the statistics launch, its statistics dropped)
            return adjhops.attention_heads_stats_dropout(inputs, l, r, 1.0 - dropout, seed, step, negative_slope, hops=sel)[0]
        return adjhops.attention_heads(inputs, l, r, negative_slope, hops=sel)
    if (grads[0] or grads[2]) and not adjhops.has_transpose:
        raise ValueError("hop_attention_recompute with inputs or an r that require a gradient: those gradients sum over the columns of the "
                         "hop matrices, on the plan's transposed operands (their permutation is not needed).  Build the plan with "
                         "HopPlan(..., build_transpose=True)")
    # (the argument checks of the launch run first either way: HopPlan.attention_heads_stats refuses before any device work)
    if dropout > 0.0:
        return _HopAttentionRecompute.apply(adjhops, sel, float(negative_slope), inputs, l, r, 1.0 - dropout, int(seed), step)
    return _HopAttentionRecompute.apply(adjhops, sel, float(negative_slope), inputs, l, r)


class _StackHeads(torch.autograd.Function):
    """``torch.stack(per_head, dim=2)`` of ``K`` ``[N, H_sel]`` projections; the backward hands every head a CONTIGUOUS ``[N, H_sel]``
    gradient, the operand the per-head chain gave the projection's GEMMs (so they run as before, on the same bits)."""

    @staticmethod
    def forward(ctx, *per_head):
        return torch.stack(per_head, dim=2)

    @staticmethod
    def backward(ctx, grad):
        return tuple(grad[:, :, h].contiguous() for h in range(grad.shape[2]))


class HopAttention(torch.nn.Module):
    """``HopAttention(in_dim, hops=None, n_hops=2, negative_slope=0.2)(adjhops, inputs) -> [N, H_sel, d]``: the attention
    counterpart of :class:`GCNLayer` -- per selected hop ``s`` the rows of ``inputs`` are aggregated with coefficients

        ``alpha_s[i, j] = softmax_j( leaky_relu(inputs[i] . a_l[s] + inputs[j] . a_r[s]) )``   over the stored entries of row ``i``

    (single-head GAT attention over the 1-hop / 2-hop rings, one softmax per hop and row).  The chain is ``l = inputs @ a_l.T``,
    ``r = inputs @ a_r.T`` -> :func:`hop_edge_scores` -> :func:`hop_softmax` -> ``hop_spmm(adjhops, inputs, hops, values=alpha)``,
    every link one launch forward and one call backward, none of them atomic: two identical training steps give identical bits.

    ``a_l``, ``a_r``: parameters ``[H_sel, in_dim]``, Glorot-uniform.  ``hops``: the hop indices to attend over (``H_sel`` of
    them); ``None`` takes all ``n_hops`` hops of the plan.  Like ``hop_spmm(..., values=...)`` the layer INSTALLS the coefficients
    in the plan (``set_values``): the plan keeps pointing at them, and the stored values it was built with are not used.  It
    needs a square plan built with ``build_transpose=True, keep_permutation=True`` to be trained.  Row-partitioned operands
    (``ShardedHops``) are not covered."""

    SIGNATURE = ["adjhops", "inputs"]

    def __init__(self, in_dim: int, hops=None, n_hops: int = 2, negative_slope: float = 0.2):
        super().__init__()
        self.hops = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
        self.in_dim = int(in_dim)
        self.negative_slope = float(negative_slope)
        h_sel = int(n_hops) if self.hops is None else len(self.hops)
        if h_sel < 1 or self.in_dim < 1:
            raise ValueError(f"HopAttention needs at least one hop and one input column, got {h_sel} hops and in_dim = {in_dim}")
        self.a_l = torch.nn.Parameter(torch.empty(h_sel, self.in_dim))
        self.a_r = torch.nn.Parameter(torch.empty(h_sel, self.in_dim))
        torch.nn.init.xavier_uniform_(self.a_l)
        torch.nn.init.xavier_uniform_(self.a_r)

    def forward(self, adjhops: HopPlan, inputs: torch.Tensor) -> torch.Tensor:
        if hasattr(adjhops, "aggregate"):
            raise ValueError("HopAttention is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
        if not isinstance(adjhops, HopPlan):
            raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
        h_sel = self.a_l.shape[0]
        if adjhops.n_selected(self.hops) != h_sel:
            raise ValueError(f"HopAttention holds attention vectors for {h_sel} hops, the plan has {adjhops.n_hops}: pass hops= or n_hops=")
        if adjhops.n_rows != adjhops.n_cols:
            raise ValueError(f"HopAttention needs a square plan (the same nodes attend and are attended to), got {adjhops.n_rows} x {adjhops.n_cols}")
        if inputs.dim() != 2 or inputs.shape[1] != self.in_dim:
            raise ValueError(f"inputs must be [{adjhops.n_cols}, {self.in_dim}], got {tuple(inputs.shape)}")
        l, r = inputs @ self.a_l.t(), inputs @ self.a_r.t()
        alpha = hop_softmax(adjhops, hop_edge_scores(adjhops, l, r, self.negative_slope, self.hops), self.hops)
        values = [None] * adjhops.n_hops     # hop_spmm takes one entry per hop of the plan
        for s, k in enumerate(adjhops._selected(self.hops)):
            values[k] = alpha[s]
        return hop_spmm(adjhops, inputs, self.hops, values=values)

    def extra_repr(self) -> str:
        return f"in_dim={self.in_dim}, hops={None if self.hops is None else list(self.hops)}, negative_slope={self.negative_slope}"


class MultiHeadHopAttention(torch.nn.Module):
    """``MultiHeadHopAttention(in_dim, heads, hops=None, n_hops=2, negative_slope=0.2)(adjhops, inputs) -> [N, H_sel, in_dim]``:
    :class:`HopAttention` with ``K = heads`` heads and GAT's concat, on :func:`hop_spmm_values` -- NOTHING is installed in the plan.

    ``heads``: an integer ``K >= 1`` with ``in_dim % K == 0``, and ``(in_dim / K) % 4 == 0`` when ``K > 1``.  ``a_l``, ``a_r``:
    parameters ``[H_sel, K, in_dim / K]``, Glorot-uniform.  Head ``h`` scores with and aggregates columns ``h * in_dim / K ..`` of
    ``inputs``: ``l[n, s, h] = <inputs[n, head h], a_l[s, h]>``, ``r`` likewise, stacked to ``[N, H_sel, K]``; then
    :func:`hop_edge_scores_heads`, :func:`hop_softmax_heads` and ONE aggregation launch, every link one launch for all heads on
    entry-major ``[nnz_k, K]`` arrays (the layout the aggregation and its adjoint read fastest).  The bits are those of the
    per-head chain (:func:`hop_edge_scores`, :func:`hop_softmax` per head, stacked as ``[K, nnz_k].t()``), which a single head and
    a library that predates the head-batched calls still run.  Head ``h`` of the output is in columns ``h * in_dim / K ..``.

    Because the coefficients are an argument of the launch, such layers can be stacked on one plan (the K propagation rounds of
    H2GCN run on the same ``adj_hops``), share it with a ``GCNLayer``, and their training step can be captured in a hipGraph after
    one eager warm-up; the plan's stored values are neither read nor replaced.  ``heads=1`` computes what :class:`HopAttention`
    computes, bit for bit, without touching the plan.  Training needs a square plan built with ``build_transpose=True,
    keep_permutation=True``, as for :class:`HopAttention`.  Row-partitioned operands (``ShardedHops``) are not covered.

    The layer runs the chain in every gradient mode.  :func:`hop_attention_heads` computes the same bits in ONE launch without
    the per-entry arrays for a forward that needs no gradient; the layer is not routed to it because the launch is not faster
    than the chain at every measured shape: a caller short of memory calls it on the layer's projections."""

    SIGNATURE = ["adjhops", "inputs"]

    def __init__(self, in_dim: int, heads: int, hops=None, n_hops: int = 2, negative_slope: float = 0.2):
        super().__init__()
        self.hops = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
        self.in_dim, self.heads = int(in_dim), int(heads)
        self.negative_slope = float(negative_slope)
        h_sel = int(n_hops) if self.hops is None else len(self.hops)
        if h_sel < 1 or self.in_dim < 1:
            raise ValueError(f"MultiHeadHopAttention needs at least one hop and one input column, got {h_sel} hops and in_dim = {in_dim}")
        if self.heads < 1 or self.in_dim % self.heads:
            raise ValueError(f"MultiHeadHopAttention(heads={heads}) needs heads >= 1 and in_dim % heads == 0, got in_dim = {in_dim}")
        if self.heads > 1 and (self.in_dim // self.heads) % 4:
            raise ValueError(f"MultiHeadHopAttention(heads={heads}): the head width in_dim / heads = {self.in_dim // self.heads} must be "
                             "a multiple of 4")
        self.a_l = torch.nn.Parameter(torch.empty(h_sel, self.heads, self.in_dim // self.heads))
        self.a_r = torch.nn.Parameter(torch.empty(h_sel, self.heads, self.in_dim // self.heads))
        torch.nn.init.xavier_uniform_(self.a_l)
        torch.nn.init.xavier_uniform_(self.a_r)
        self.attn_dropout, self.seed = 0.0, None   # (see set_attention_dropout)

    def set_attention_dropout(self, attn_dropout: float, seed: Optional[int] = None) -> "MultiHeadHopAttention":
        """Dropout on the attention coefficients (GAT's ``attn_drop``) with rate ``attn_dropout`` in ``[0, 1)``, active in ``train()``
        only; returns ``self``: ``layer = RecomputeMultiHeadHopAttention(d, 8).set_attention_dropout(0.6)``.  (A method, not a
        constructor argument: the constructor, and with it the random numbers a model's construction consumes, stay as they are.)

        The mask is a pure function of ``(seed, step, hop, row, column, head)`` (include/h2gcn_hip.h): ``step`` lives in a
        non-persistent buffer ``_step`` bumped by a stream-ordered op per training forward (as :class:`DropoutDense` does), so the
        ``state_dict`` is unchanged and a replayed hipGraph draws a fresh mask per replay.  The step counters of a model's layers
        advance in lock step: a per-layer salt keeps two layers from drawing identical masks -- ``seed=None`` draws it from torch's
        generator HERE (and only for ``attn_dropout > 0``), an integer sets it.  :class:`RecomputeMultiHeadHopAttention` draws the
        mask inside its kernels; this class multiplies ``alpha`` by the factor arrays of :meth:`HopPlan.attention_dropout_factors`:
        with equal seeds and steps the two give ``torch.equal`` outputs.  At most 16 heads."""
        attn_dropout = float(attn_dropout)
        if not 0.0 <= attn_dropout < 1.0:
            raise ValueError(f"set_attention_dropout(attn_dropout={attn_dropout}) outside [0, 1)")
        if attn_dropout > 0.0 and self.heads > HopPlan.ATTENTION_FUSED_MAX_HEADS:
            raise ValueError(f"set_attention_dropout(attn_dropout={attn_dropout}) serves at most {HopPlan.ATTENTION_FUSED_MAX_HEADS} heads, "
                             f"got heads = {self.heads}")
        self.attn_dropout = attn_dropout
        if attn_dropout > 0.0:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
            if "_step" not in self._buffers:
                self.register_buffer("_step", torch.zeros(1, dtype=torch.int64, device=self.a_l.device), persistent=False)
        return self

    def _draw_step(self):
        """``(keep_prob, step)`` of one forward: in training with ``attn_dropout > 0`` the step counter advances (stream-ordered: a
        captured graph bumps it on every replay) and ``step`` is the value this forward and its backward use; else ``(1.0, None)``."""
        if not (self.training and self.attn_dropout > 0.0):
            return 1.0, None
        self._step += 1
        return 1.0 - self.attn_dropout, self._step.clone()

    def forward(self, adjhops: HopPlan, inputs: torch.Tensor) -> torch.Tensor:
        if hasattr(adjhops, "aggregate"):
            raise ValueError("MultiHeadHopAttention is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
        if not isinstance(adjhops, HopPlan):
            raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
        h_sel = self.a_l.shape[0]
        if adjhops.n_selected(self.hops) != h_sel:
            raise ValueError(f"MultiHeadHopAttention holds attention vectors for {h_sel} hops, the plan has {adjhops.n_hops}: pass hops= or n_hops=")
        if adjhops.n_rows != adjhops.n_cols:
            raise ValueError(f"MultiHeadHopAttention needs a square plan (the same nodes attend and are attended to), got {adjhops.n_rows} x {adjhops.n_cols}")
        if inputs.dim() != 2 or inputs.shape[1] != self.in_dim:
            raise ValueError(f"inputs must be [{adjhops.n_cols}, {self.in_dim}], got {tuple(inputs.shape)}")
        n_heads, w = self.heads, self.in_dim // self.heads
        keep_prob, step = self._draw_step()
        # (dropout: alpha times the factor arrays -- the mask RecomputeMultiHeadHopAttention draws inside its kernels for this seed and step)
        factors = None if step is None else adjhops.attention_dropout_factors(n_heads, keep_prob, self.seed, step, hops=self.hops)
        if n_heads > 1 and _capi.has("h2gcn_edge_scores_hops_heads_f32"):
            # one launch per link: the per-head projections as before, stacked to [N, H_sel, K]; entry-major [nnz_k, K] from there on
            ls, rs = [], []
            for h in range(n_heads):
                x_h = inputs[:, h * w:(h + 1) * w]
                l, r = x_h @ self.a_l[:, h, :].t(), x_h @ self.a_r[:, h, :].t()
                ls.append(l)
                rs.append(r)
            scores = hop_edge_scores_heads(adjhops, _StackHeads.apply(*ls), _StackHeads.apply(*rs), self.negative_slope, self.hops)
            alpha = hop_softmax_heads(adjhops, scores, self.hops)
            if factors is not None:
                alpha = [a * f for a, f in zip(alpha, factors)]
            return hop_spmm_values(adjhops, inputs, alpha, self.hops)
        alpha = []
        for h in range(n_heads):
            x_h = inputs if n_heads == 1 else inputs[:, h * w:(h + 1) * w]
            l, r = x_h @ self.a_l[:, h, :].t(), x_h @ self.a_r[:, h, :].t()
            alpha.append(hop_softmax(adjhops, hop_edge_scores(adjhops, l, r, self.negative_slope, self.hops), self.hops))
        values = [torch.stack([alpha[h][s] for h in range(n_heads)], dim=0).t() for s in range(h_sel)]
        if factors is not None:
            values = [v * f for v, f in zip(values, factors)]
        return hop_spmm_values(adjhops, inputs, values, self.hops)

    def extra_repr(self) -> str:
        return (f"in_dim={self.in_dim}, heads={self.heads}, hops={None if self.hops is None else list(self.hops)}, "
                f"negative_slope={self.negative_slope}" + (f", attn_dropout={self.attn_dropout}" if self.attn_dropout > 0.0 else ""))


class RecomputeMultiHeadHopAttention(MultiHeadHopAttention):
    """:class:`MultiHeadHopAttention` -- the same constructor, parameters and ``state_dict`` -- whose training step keeps no
    per-entry array: ``l`` and ``r`` are built exactly as the parent class builds them (per-head projections, stacked to ``[N, H_sel,
    K]``) and go to :func:`hop_attention_recompute`, one launch forward and one call backward.  The output has the parent's bits;
    the parameter gradients agree with the parent's to rounding (their summation orders differ) and are as deterministic.  Peak
    memory no longer grows with ``nnz * K``.  Training needs a square plan built with ``build_transpose=True`` (``keep_permutation``
    is not needed); such layers can be stacked on one plan, share it with a ``GCNLayer``, and their training step can be captured
    in a hipGraph after one eager warm-up.  ``heads > 16`` or ``in_dim > 256`` run the parent's chain.

    A bfloat16 ``inputs`` (an attention layer behind a bf16 propagation) runs the bf16 launches of :func:`hop_attention_recompute`:
    the per-head projections are computed in float32 from the upcast head slice (one ``[N, in_dim / heads]`` transient at a time),
    the output and ``inputs.grad`` are bfloat16, the parameters and their gradients float32.  What bf16 does not cover (more than 16
    heads, ``in_dim > 256`` under a gradient, attention dropout active in ``train()``) is a ``ValueError``."""

    def forward(self, adjhops: HopPlan, inputs: torch.Tensor) -> torch.Tensor:
        if hasattr(adjhops, "aggregate"):
            raise ValueError("RecomputeMultiHeadHopAttention is not supported on row-partitioned operands (ShardedHops): pass a single-GPU "
                             "HopPlan")
        if not isinstance(adjhops, HopPlan):
            raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
        h_sel = self.a_l.shape[0]
        if adjhops.n_selected(self.hops) != h_sel:
            raise ValueError(f"RecomputeMultiHeadHopAttention holds attention vectors for {h_sel} hops, the plan has {adjhops.n_hops}: pass "
                             "hops= or n_hops=")
        if adjhops.n_rows != adjhops.n_cols:
            raise ValueError("RecomputeMultiHeadHopAttention needs a square plan (the same nodes attend and are attended to), got "
                             f"{adjhops.n_rows} x {adjhops.n_cols}")
        if inputs.dim() != 2 or inputs.shape[1] != self.in_dim:
            raise ValueError(f"inputs must be [{adjhops.n_cols}, {self.in_dim}], got {tuple(inputs.shape)}")
        n_heads, w = self.heads, self.in_dim // self.heads
        if inputs.dtype == torch.bfloat16:
            # bf16 embeddings: the projections in fp32 from the upcast head slice (one [N, w] transient at a time), then the bf16
            # launches.  What they do not cover is refused by hop_attention_recompute, never run in float32 instead.
            if self.training and self.attn_dropout > 0.0:
                raise ValueError(f"RecomputeMultiHeadHopAttention(attn_dropout={self.attn_dropout}) in train() with bfloat16 inputs: the "
                                 "attention dropout launches are float32 only (eval(), or float32 inputs)")
            ls, rs = [], []
            for h in range(n_heads):
                x_h = (inputs if n_heads == 1 else inputs[:, h * w:(h + 1) * w]).float()
                ls.append(x_h @ self.a_l[:, h, :].t())
                rs.append(x_h @ self.a_r[:, h, :].t())
            return hop_attention_recompute(adjhops, inputs, _StackHeads.apply(*ls), _StackHeads.apply(*rs), self.negative_slope, self.hops)
        if (n_heads > HopPlan.ATTENTION_FUSED_MAX_HEADS or self.in_dim > HopPlan.ATTENTION_RECOMPUTE_MAX_WIDTH
                or not all(_capi.has(s) for s in HopPlan._RECOMPUTE_SYMBOLS)):
            return super().forward(adjhops, inputs)   # (the chain, on alpha * f under dropout: the same mask)
        ls, rs = [], []
        for h in range(n_heads):
            x_h = inputs if n_heads == 1 else inputs[:, h * w:(h + 1) * w]
            l, r = x_h @ self.a_l[:, h, :].t(), x_h @ self.a_r[:, h, :].t()
            ls.append(l)
            rs.append(r)
        keep_prob, step = self._draw_step()
        if step is None:
            return hop_attention_recompute(adjhops, inputs, _StackHeads.apply(*ls), _StackHeads.apply(*rs), self.negative_slope, self.hops)
        return hop_attention_recompute_dropout(adjhops, inputs, _StackHeads.apply(*ls), _StackHeads.apply(*rs), self.attn_dropout, self.seed,
                                               step, self.negative_slope, self.hops)


class DynamicHopAttention(torch.nn.Module):
    """``DynamicHopAttention(in_dim, heads, hops=None, n_hops=2, negative_slope=0.2, share_weights=False)(adjhops, inputs) ->
    [N, H_sel, in_dim]``: GATv2 (Brody et al.) on the hop rings.  :class:`MultiHeadHopAttention` scores an entry with
    ``leaky_relu(l[i] + r[j])``, which ranks the neighbours of EVERY row by ``r[j]`` alone (static attention); here

        ``u = inputs @ W_l``, ``v = inputs @ W_r``, ``score[s][e, h] = sum_{c in head h} a[s, h, c] * leaky_relu(u[i, c] + v[j, c])``

    so whom a node listens to depends on the node -- what heterophilous graphs ask for.  Then :func:`hop_softmax_heads`
    (:func:`hop_softmax` for one head) and ONE aggregation launch ``hop_spmm_values(adjhops, v, alpha)``: GATv2 aggregates the
    source projection.  Head ``h`` owns columns ``h * in_dim / K ..`` of ``u``, ``v`` and of the output.

    Parameters, Glorot-uniform and drawn in this order: ``W_l`` ``[in_dim, in_dim]``, ``W_r`` ``[in_dim, in_dim]`` (absent with
    ``share_weights=True``: ``v = u``, GATv2's ``share_weights``), ``a`` ``[H_sel, heads, in_dim // heads]``.  ``heads``: an
    integer ``K >= 1`` with ``in_dim % K == 0``, and ``(in_dim / K) % 4 == 0`` when ``K > 1``; ``in_dim <= 256``.

    The scores are one launch per direction (:func:`hop_edge_scores_dynamic`) without an ``nnz x in_dim`` array; nothing is
    installed in the plan, so such layers stack on one plan and their training step can be captured in a hipGraph after one eager
    warm-up.  Training needs a square plan built with ``build_transpose=True, keep_permutation=True``.  float32 only; no attention
    dropout.  Row-partitioned operands (``ShardedHops``) are not covered."""

    SIGNATURE = ["adjhops", "inputs"]

    def __init__(self, in_dim: int, heads: int, hops=None, n_hops: int = 2, negative_slope: float = 0.2, share_weights: bool = False):
        super().__init__()
        self.hops = None if hops is None else tuple(sorted(set(int(h) for h in hops)))
        self.in_dim, self.heads = int(in_dim), int(heads)
        self.negative_slope = float(negative_slope)
        self.share_weights = bool(share_weights)
        h_sel = int(n_hops) if self.hops is None else len(self.hops)
        if h_sel < 1 or self.in_dim < 1:
            raise ValueError(f"DynamicHopAttention needs at least one hop and one input column, got {h_sel} hops and in_dim = {in_dim}")
        if self.heads < 1 or self.in_dim % self.heads:
            raise ValueError(f"DynamicHopAttention(heads={heads}) needs heads >= 1 and in_dim % heads == 0, got in_dim = {in_dim}")
        if self.heads > 1 and (self.in_dim // self.heads) % 4:
            raise ValueError(f"DynamicHopAttention(heads={heads}): the head width in_dim / heads = {self.in_dim // self.heads} must be "
                             "a multiple of 4")
        if self.in_dim > HopPlan.EDGE_SCORES_DYNAMIC_MAX_WIDTH:
            raise ValueError(f"DynamicHopAttention(in_dim={in_dim}): the dynamic edge scores serve widths up to "
                             f"EDGE_SCORES_DYNAMIC_MAX_WIDTH = {HopPlan.EDGE_SCORES_DYNAMIC_MAX_WIDTH}")
        self.W_l = torch.nn.Parameter(torch.empty(self.in_dim, self.in_dim))
        torch.nn.init.xavier_uniform_(self.W_l)
        if not self.share_weights:
            self.W_r = torch.nn.Parameter(torch.empty(self.in_dim, self.in_dim))
            torch.nn.init.xavier_uniform_(self.W_r)
        self.a = torch.nn.Parameter(torch.empty(h_sel, self.heads, self.in_dim // self.heads))
        torch.nn.init.xavier_uniform_(self.a)

    def forward(self, adjhops: HopPlan, inputs: torch.Tensor) -> torch.Tensor:
        if hasattr(adjhops, "aggregate"):
            raise ValueError("DynamicHopAttention is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
        if not isinstance(adjhops, HopPlan):
            raise TypeError(f"adjhops must be a HopPlan, got {type(adjhops).__name__}")
        h_sel = self.a.shape[0]
        if adjhops.n_selected(self.hops) != h_sel:
            raise ValueError(f"DynamicHopAttention holds attention vectors for {h_sel} hops, the plan has {adjhops.n_hops}: pass hops= or n_hops=")
        if adjhops.n_rows != adjhops.n_cols:
            raise ValueError(f"DynamicHopAttention needs a square plan (the same nodes attend and are attended to), got {adjhops.n_rows} x {adjhops.n_cols}")
        if inputs.dim() != 2 or inputs.shape[1] != self.in_dim:
            raise ValueError(f"inputs must be [{adjhops.n_cols}, {self.in_dim}], got {tuple(inputs.shape)}")
        u = inputs @ self.W_l
        v = u if self.share_weights else inputs @ self.W_r
        scores = hop_edge_scores_dynamic(adjhops, u, v, self.a, self.heads, self.negative_slope, self.hops)
        alpha = hop_softmax(adjhops, scores, self.hops) if self.heads == 1 else hop_softmax_heads(adjhops, scores, self.hops)
        return hop_spmm_values(adjhops, v, alpha, self.hops)

    def extra_repr(self) -> str:
        return (f"in_dim={self.in_dim}, heads={self.heads}, hops={None if self.hops is None else list(self.hops)}, "
                f"negative_slope={self.negative_slope}, share_weights={self.share_weights}")


class GCNLayer(torch.nn.Module):
    """``GCNLayer(hops=None)(adjhops, inputs) -> [N, H_sel, d]`` (reference ``_layers.py:54-81``).

    ``hops``: optional set of hop indices to keep (the ``G0`` / ``G0_1`` forms of the network-setup DSL,
    ``h2gcn/models/__init__.py:88-95``); ``None`` keeps every hop of ``adjhops``.  Unknown indices are ignored
    like the reference's ``if ind in self.hops`` filter does -- unless nothing is left, which raises.
    ``forward(adjhops, inputs, values=None)``: ``values`` makes the stored values of the hop matrices differentiable inputs
    (see :func:`hop_spmm`).
    """

    SIGNATURE = ["adjhops", "inputs"]

    def __init__(self, hops=None):
        super().__init__()
        self.hops = None if hops is None else set(int(h) for h in hops)

    def forward(self, adjhops: HopPlan, inputs: torch.Tensor, values=None) -> torch.Tensor:
        sel = None
        if hasattr(adjhops, "aggregate"):  # partition.ShardedHops: all-gather + local SpMM (+ reduce-scatter backward)
            if values is not None:
                raise ValueError("values= is not supported on row-partitioned operands (ShardedHops): pass a single-GPU HopPlan")
            return adjhops.aggregate(inputs, None if self.hops is None else sorted(self.hops))
        if self.hops is not None:
            sel = [h for h in range(adjhops.n_hops) if h in self.hops]
            if not sel:
                raise ValueError(f"GCNLayer(hops={sorted(self.hops)}) selects none of the {adjhops.n_hops} hops")
        return hop_spmm(adjhops, inputs, sel, values)

    def extra_repr(self) -> str:
        return f"hops={None if self.hops is None else sorted(self.hops)}"


class SparseDropout(torch.nn.Module):
    """Dropout on the VALUES of the sparse feature operand (reference ``SparseDropout``, ``_layers.py:7-19``: mask =
    ``floor(keep_prob + U[0,1))`` per stored value, survivors divided by ``keep_prob``; reached when ``D`` precedes the
    first dense layer, ``H2GCN.py:250-257``).  The operand is a 1-hop :class:`HopPlan`; its pattern is static, so the
    layer writes the masked values into one persistent buffer (dropped entries as explicit zeros -- the same product as
    ``tf.sparse.retain``) and points the plan at it (``HopPlan.set_values``, which also refreshes the transposed
    operand the kernel gradient needs).

    Eval mode -- a DOCUMENTED DIVERGENCE from the reference: its ``SparseDropout.call(self, input)`` takes no
    ``training`` argument and ``H2GCN.call`` invokes ``layer(inputs)`` (``H2GCN.py:323``), so Keras never switches it
    off: the reference also drops sparse feature values during evaluation (its dense ``Dropout`` layers are switched
    off).  That looks unintended; here the layer is inactive in eval mode by default, like every other dropout.
    ``at_eval=True`` (CLI ``--sparse_dropout_at_eval``) reproduces the reference's behaviour.

    The plan is shared (``tensors["features"]``): :meth:`restore` puts the original values back; the training step calls
    it once the backward pass -- which still needs the dropped operand for ``dW = X_drop^T g`` -- is done, so nobody
    observes dropped values between steps."""

    def __init__(self, drop_prob: float, at_eval: bool = False):
        super().__init__()
        self.drop_prob = float(drop_prob)
        self.at_eval = bool(at_eval)
        self._buf = None
        self._plan = None

    def restore(self) -> None:
        """Point the plan back at its original values (no-op if they are in place)."""
        plan = self._plan
        if plan is None:
            return
        orig = getattr(plan, "_values_before_dropout", None)
        if orig is not None and plan.vals[0] is not orig:
            plan.set_values(0, orig)

    def forward(self, plan: HopPlan) -> HopPlan:
        if not isinstance(plan, HopPlan) or plan.n_hops != 1:
            raise TypeError("SparseDropout expects the sparse feature operand as a 1-hop HopPlan")
        self._plan = plan
        orig = getattr(plan, "_values_before_dropout", None)
        if not (self.training or self.at_eval) or self.drop_prob <= 0.0:
            self.restore()
            return plan
        if orig is None:
            orig = plan._values_before_dropout = plan.vals[0]
        if self._buf is None or self._buf.shape != orig.shape or self._buf.device != orig.device:
            self._buf = torch.empty_like(orig)
        keep = 1.0 - self.drop_prob
        mask = torch.floor(torch.rand_like(orig) + keep)
        torch.mul(orig, mask / keep, out=self._buf)
        plan.set_values(0, self._buf)
        return plan


class _SparseDenseFused(torch.autograd.Function):
    """``act(X_sp @ W + b)`` in ONE launch: bias and ReLU are the store epilogue of the hop kernel (reference
    ``SparseDense.call``, ``_layers.py:45-52``).  Backward: ``g = dY * (Y > 0)``; ``dW = X_sp^T g`` (adjoint launch),
    ``db = sum_rows g``."""

    @staticmethod
    def forward(ctx, kernel, bias, plan, relu):
        y = plan.spmm(kernel, bias=bias, relu=relu)[:, 0, :]
        ctx.plan, ctx.relu, ctx.has_bias = plan, relu, bias is not None
        ctx.save_for_backward(y if relu else torch.empty(0, device=y.device))
        return y

    @staticmethod
    def backward(ctx, grad):
        (y,) = ctx.saved_tensors
        g = grad * (y > 0) if ctx.relu else grad
        d_kernel = ctx.plan.spmm_t(g.contiguous().unsqueeze(1))
        return d_kernel, (g.sum(0) if ctx.has_bias else None), None, None


class SparseDense(torch.nn.Module):
    """Sparse features x dense kernel (reference ``SparseDense``, ``h2gcn/models/_layers.py:22-52``): the feature
    embedding ``X_sp[N, F] @ W[F, units]`` (+ bias, + activation).  The sparse operand is a 1-hop
    :class:`HopPlan` holding the feature matrix in CSR, so the product runs on the same HIP kernel as the hop
    aggregation; the kernel gradient ``X_sp^T @ dY`` is the plan's adjoint launch."""

    def __init__(self, input_dim: int, output_dim: int, use_bias: bool = False, activation=None):
        super().__init__()
        self.kernel = torch.nn.Parameter(torch.empty(input_dim, output_dim))
        torch.nn.init.xavier_uniform_(self.kernel)  # keras default: glorot_uniform
        self.bias = torch.nn.Parameter(torch.zeros(output_dim)) if use_bias else None
        self.activation = activation

    def forward(self, inputs: HopPlan) -> torch.Tensor:
        if not isinstance(inputs, HopPlan) or inputs.n_hops != 1:
            raise TypeError("SparseDense expects the sparse feature operand as a 1-hop HopPlan")
        if inputs.n_cols != self.kernel.shape[0]:
            raise ValueError(f"features have {inputs.n_cols} columns, kernel has {self.kernel.shape[0]} rows")
        relu = self.activation in ("relu", torch.relu, torch.nn.functional.relu) or isinstance(self.activation, torch.nn.ReLU)
        if self.bias is not None or relu:   # bias / ReLU fused into the store of the sparse product
            if inputs.has_transpose or not (self.kernel.requires_grad and torch.is_grad_enabled()):
                return _SparseDenseFused.apply(self.kernel, self.bias, inputs, relu)
        out = hop_spmm(inputs, self.kernel)[:, 0, :]
        if self.bias is not None:
            out = out + self.bias
        if self.activation is not None:
            out = torch.relu(out) if relu else self.activation(out)
        return out


class ConcatLayer(torch.nn.Module):
    """``concat([inputs] + [tagged[name] for name in tags])`` on the last axis (reference ``ConcatLayer``,
    ``_layers.py:83-96``).  Tagged outputs are taken in the order they were produced (the reference iterates the
    kwargs dict, i.e. insertion order), not in the order the tags are listed."""

    def __init__(self, tags, axis: int = -1, addInputs: bool = True):
        super().__init__()
        self.tags = list(tags)
        self.axis = axis
        self.addInputs = addInputs

    def forward(self, *args, **tagged) -> torch.Tensor:
        selected = [v for name, v in tagged.items() if name in self.tags]
        return torch.cat((list(args) if self.addInputs else []) + selected, dim=self.axis)


class SliceLayer(torch.nn.Module):
    """Column slice of the input or of a tagged output (reference ``SliceLayer``, ``_layers.py:107-116``)."""

    def __init__(self, loadTag, sliceObj, **_):
        super().__init__()
        self.tag = loadTag
        self.sliceObj = sliceObj

    def forward(self, inputs, **tagged):
        if self.tag:
            inputs = tagged[self.tag]
        return inputs[:, self.sliceObj]


@dataclass(frozen=True)
class ConcatLayout:
    """The column layout of the concat buffer ``[r_K | r_0 | r_1 | ... | r_{K-1}]`` of ``rounds = K`` aggregation rounds over
    ``n_hops = H`` hop matrices on an embedding of width ``w0``: round ``k`` is ``widths[k] = w0 * H**k`` columns wide and starts
    at column ``offsets[k]``.  The only place that knows the order of the slots."""

    w0: int
    n_hops: int
    rounds: int
    widths: tuple = field(init=False)
    offsets: tuple = field(init=False)
    total: int = field(init=False)

    def __post_init__(self):
        widths = tuple(self.w0 * self.n_hops ** k for k in range(self.rounds + 1))
        offsets = [0] * (self.rounds + 1)   # r_K first, then r_0 .. r_{K-1}
        pos = widths[self.rounds]
        for k in range(self.rounds):
            offsets[k] = pos
            pos += widths[k]
        for name, value in (("widths", widths), ("offsets", tuple(offsets)), ("total", pos)):
            object.__setattr__(self, name, value)

    def slot(self, t: torch.Tensor, k: int) -> torch.Tensor:
        """The columns of ``r_k`` in a ``[n, total]`` tensor (a view)."""
        return t[:, self.offsets[k]:self.offsets[k] + self.widths[k]]

    def hops(self, r_k: torch.Tensor, k: int) -> torch.Tensor:
        """``r_k [n, widths[k]]`` (``k >= 1``) as the ``[n, H, widths[k-1]]`` output of round ``k``'s hop launch (a view)."""
        return r_k.unflatten(1, (self.n_hops, self.widths[k - 1]))

    def hop_view(self, t: torch.Tensor, k: int) -> torch.Tensor:
        """``hops(slot(t, k), k)``: the slot of round ``k >= 1`` as ``[n, H, widths[k-1]]``."""
        return self.hops(self.slot(t, k), k)


#: ``concat_layout(w0, n_hops, rounds)``: the (immutable, hence shared) layout -- a training loop asks for the same one every step
concat_layout = functools.lru_cache(maxsize=64)(ConcatLayout)


def _propagate(layout: ConcatLayout, plan: HopPlan, r0: torch.Tensor, out: Optional[torch.Tensor], reuse: bool,
               dtype: torch.dtype) -> torch.Tensor:
    """The forward of the fused propagation (arguments checked by :func:`_check_propagation`): ``r0`` into its slot of ``out`` (or
    of a fresh buffer), then round ``k`` from slot ``k-1`` into slot ``k`` through the kernel's strides.  ``reuse``: nothing is
    computed."""
    n = r0.shape[0]
    # (out.view: a new tensor object on the caller's storage -- autograd marks IT as the node's output)
    buf = concat_buffer(n, layout.total, r0.device, dtype) if out is None else out.view(n, layout.total)
    if not reuse:
        layout.slot(buf, 0).copy_(r0)
        for k in range(1, layout.rounds + 1):
            plan.spmm(layout.slot(buf, k - 1), out=layout.hop_view(buf, k))
    return buf


def _backward_walk(layout: ConcatLayout, grad: torch.Tensor, adjoint, add_slot=None, bf16: bool = False, in_place=None) -> torch.Tensor:
    """The gradient of ``r_0`` from the gradient ``grad [n, total]`` of a concat buffer (full, or the compact rows of the
    rows-only path): the rounds in reverse, and THE statement of their order of operations (bf16: of roundings) --
    :class:`_FusedPropagation`, :class:`_PropagationClassifyRowsFn` and ``partition._ShardedFusedPropagation`` all walk here::

        t       = adjoint(k, g_k)                    accumulated and returned in fp32 (g_K = slot_K(grad), read in place)
        t      += slot_{k-1}(grad)                   a bf16 slot widened exactly to fp32
        g_{k-1} = t rounded to bf16 (nearest even)   for k > 1 of a bf16 walk
        g_{k-1} = t                                  otherwise: fp32 walks, and k = 1 of a bf16 walk (d r_0 stays fp32)

    ``adjoint(k, g, **kw)``: the adjoint of round ``k`` on ``g [n, H, widths[k-1]]``.  ``add_slot(t, slot)``: the second line
    where ``t`` and the slot differ in their rows (rows-only).  ``in_place(k)``: true where round ``k``
    may instead be ADDED to ``slot_{k-1}`` inside ``grad`` itself by the adjoint's store (``adjoint(k, g, out=slot,
    accumulate=True)``; fp32 only): the same sum, one pass and one tensor less."""
    g_k = layout.slot(grad, layout.rounds)
    for k in range(layout.rounds, 0, -1):
        slot = layout.slot(grad, k - 1)
        if in_place is not None and in_place(k):
            g_k = adjoint(k, layout.hops(g_k, k), out=slot, accumulate=True)
            continue
        t = adjoint(k, layout.hops(g_k, k))
        if add_slot is None:
            t += slot
        else:
            add_slot(t, slot)
        g_k = t.to(torch.bfloat16) if bf16 and k > 1 else t
    return g_k


class _FusedPropagation(torch.autograd.Function):
    """K rounds of hop aggregation written straight into the final concat buffer.

    H2GCN-K's representation is ``[r_K | r_0 | r_1 | ... | r_{K-1}]`` with ``r_k = flatten(GCNLayer(r_{k-1}))``
    (reference: ``G``/``V`` layers ``h2gcn/models/H2GCN.py:266-272,318-319`` followed by ``C<tag>`` concats,
    ``_layers.py:90-96``; concat order = running input first, then tags in production order).  The reference
    materialises every ``r_k`` (``tf.stack``), flattens, then copies everything twice more through ``ConcatV2``.
    Here one ``[N, W]`` buffer is allocated; each round's fused SpMM reads ``r_{k-1}`` from its column slot
    (row stride ``W``) and writes ``r_k`` into its own slot through the kernel's output strides -- no stack, no
    flatten, no concat copy.  Backward walks the rounds in reverse with the adjoint launch, reading the incoming
    gradient slots in place.

    ``dtype=torch.bfloat16``: the buffer is bf16.  ``r0`` (fp32) is rounded into its slot (nearest even) and every round is
    the bf16 -> bf16 launch (fp32 accumulation, one rounding at the store) from one slot to the next.  The backward receives
    the buffer's gradient in bf16 and walks the rounds ``k = K .. 1`` in the order of roundings that :func:`_backward_walk`
    specifies: one rounding per round on the way down and none on the last (the gradient handed to the embedding layer is
    fp32).  ``private_grad`` (the in-place accumulate) applies to fp32 only: a bf16 slot cannot be accumulated into.
    """

    @staticmethod
    def forward(ctx, r0: torch.Tensor, plan: HopPlan, layout: ConcatLayout, out: Optional[torch.Tensor], reuse: bool,
                private_grad: bool, dtype: torch.dtype):
        """``private_grad`` / ``out`` / ``reuse``: see :func:`fused_propagation` (the backward needs none of the forward's
        values: the rounds are linear)."""
        ctx.plan, ctx.layout = plan, layout
        ctx.private_grad = bool(private_grad) and dtype == torch.float32
        ctx.bf16 = dtype == torch.bfloat16
        return _propagate(layout, plan, r0, out, reuse, dtype)

    @staticmethod
    def backward(ctx, grad: torch.Tensor):
        plan, layout = ctx.plan, ctx.layout
        if ctx.bf16:   # the adjoint reads bf16 rows in dwords
            if grad.stride(1) != 1 or grad.stride(0) % 2 or grad.data_ptr() % 4:
                grad = grad.contiguous()
            d_r0 = _backward_walk(layout, grad, lambda k, g: plan.spmm_t(g, out_dtype=torch.float32), bf16=True)
            return d_r0, None, None, None, None, None, None
        # The adjoint of round k is ADDED to the slot of r_{k-1} inside the incoming gradient itself (the library's
        # accumulate flag: the `+=` rides on the adjoint's store) -- but ONLY when the caller has vouched that this tensor is a
        # temporary of its own (`private_grad`: models.H2GCN sets it when the buffer's sole consumer is a layer whose
        # backward allocates its input gradient, DropoutDense / Dense / Dropout).  Autograd itself gives no such guarantee
        # (a user-supplied `out.backward(G)`, a hook or `retain_grad` on the buffer, a gradient shared with another node),
        # so the default is a fresh tensor per round plus one `+=` pass.  Also needed: an ordinary dense gradient.
        dense = (ctx.private_grad and grad.is_contiguous() and isinstance(plan, HopPlan)
                 and os.environ.get("H2GCN_BACKWARD_IN_PLACE", "1") != "0")

        def in_place(k):
            # (not where the plain launch would run in the in-tile short-row mode -- short-throughout operands, where that mode is
            # worth more than the saved pass; list-driven / wave-walk launches lose nothing on the accumulating tile walk)
            return dense and plan.schedule(layout.widths[k - 1], ld_src=grad.stride(0), adjoint=True)["segment_walk"] != "lane group per segment (short rows)"

        return _backward_walk(layout, grad, lambda k, g, **kw: plan.spmm_t(g, **kw), in_place=in_place), None, None, None, None, None, None


def concat_buffer(n_rows: int, width: int, device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The ``[n_rows, width]`` concat buffer (fp32, or bf16 for a bf16 propagation), contiguous.  (Padding its row stride to a cache line was tried in round
    3 and dropped: the hop launches gain < 2 % -- the slots inside a row still start off-line, so they take the
    scratch-copy schedule either way -- while the stock dropout / classifier kernels that consume the buffer fall off
    their vectorised paths on a non-contiguous view: +2.8 ms per products-scale step at ``--hidden 100``,
    ``profiles/r03_train_step_hidden100.txt``.)"""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"concat_buffer: dtype must be float32 or bfloat16, got {dtype}")
    return torch.empty((n_rows, width), dtype=dtype, device=device)


def fused_propagation(plan: HopPlan, r0: torch.Tensor, rounds: int, out: Optional[torch.Tensor] = None,
                      reuse: bool = False, private_grad: bool = False, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``[r_K | r_0 | ... | r_{K-1}]`` for ``rounds = K`` aggregation rounds, without intermediate copies.

    ``out`` / ``reuse``: the propagation is a deterministic function of ``(plan, r0)``, and an epoch of the reference evaluates
    the model right after every update (``run_experiments.py:44-61``: ``train_step`` then ``test_step``) -- so the next
    epoch's training forward recomputes exactly the buffer the evaluation has just produced whenever nothing stochastic
    precedes the propagation (H2GCN's default setup: the only dropout sits behind it).  A caller that knows this
    (``models.H2GCN``) lets the evaluation fill a persistent buffer (``out=``) and hands the same buffer to the training
    forward with ``reuse=True``: same bits, one propagation per epoch instead of two.

    ``private_grad``: promise that the gradient arriving for the returned buffer is a temporary no one else holds; the
    backward then accumulates the rounds' adjoints into its slots in place (bit-identical, one pass and one tensor less per
    round).  Leave it off when the buffer's gradient may be observed (hooks, ``retain_grad``, an explicit ``backward(G)``).

    ``dtype``: ``None`` / ``torch.float32`` (default) or ``torch.bfloat16`` -- the dtype of the buffer; ``r0`` stays float32.
    With bfloat16 every hop launch moves half the bytes (fp32 accumulation, one rounding per slot); the gradient of the
    buffer is bfloat16 and the gradient returned for ``r0`` float32 (rounding order: :func:`_backward_walk`).  ``r0``
    needs an even width (bf16 rows are read in dwords)."""
    layout, dtype = _check_propagation("fused_propagation", plan, r0, rounds, out, reuse, dtype)
    if r0.requires_grad and torch.is_grad_enabled():
        return _FusedPropagation.apply(r0, plan, layout, out, reuse, private_grad, dtype)
    return _propagate(layout, plan, r0, out, reuse, dtype)


def _check_propagation(name: str, plan, r0: torch.Tensor, rounds: int, out: Optional[torch.Tensor], reuse: bool,
                       dtype: Optional[torch.dtype], rows_only: bool = False):
    """The argument checks of :func:`fused_propagation` and :func:`fused_propagation_classify_rows` (``name``: the caller, for
    the messages; ``rows_only``: the latter, whose ``r0`` is a float32 CUDA tensor whatever the buffer's dtype).  Returns the
    buffer's ``(layout, dtype)``."""
    if rounds < 1:
        raise ValueError("rounds must be >= 1")
    if dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"{name}: dtype must be float32 or bfloat16, got {dtype}")
    dtype = torch.float32 if dtype is None else dtype
    bf16 = dtype == torch.bfloat16
    if bf16 and not rows_only and r0.dtype != torch.float32:
        raise ValueError(f"{name}: r0 must be float32 (it is rounded into the bfloat16 buffer), got {r0.dtype}")
    square = r0.dim() == 2 and r0.shape[0] == plan.n_cols and plan.n_rows == plan.n_cols
    if rows_only and not (square and r0.is_cuda and r0.dtype == torch.float32):
        raise ValueError(f"r0 must be a float32 CUDA tensor [{plan.n_cols}, d] and the hop matrices square")
    if not square:
        raise ValueError(f"r0 must be [{plan.n_cols}, d] and the hop matrices square")
    if bf16 and r0.shape[1] % 2:
        raise ValueError(f"{name}: a bfloat16 buffer needs an even embedding width, got {r0.shape[1]}" + ("" if rows_only else
                         " (bf16 rows are read in dwords: pad the hidden width to an even number or use float32)"))
    if reuse and out is None:
        raise ValueError(f"{name}: reuse=True needs the buffer that holds the propagation (out=)")
    layout = concat_layout(r0.shape[1], plan.n_hops, rounds)
    _check_out(out, r0.shape[0], layout.total, dtype, r0.device)
    return layout, dtype


def _check_out(out: Optional[torch.Tensor], n: int, total: int, dtype: torch.dtype, device) -> None:
    """``out=`` of a fused propagation, single-GPU or row-partitioned: the whole ``[n, total]`` buffer or nothing."""
    if out is not None and (out.shape != (n, total) or out.dtype != dtype or out.device != device or not out.is_contiguous()):
        raise ValueError(f"fused_propagation: out must be a contiguous {str(dtype).replace('torch.', '')} [{n}, {total}] tensor on {device}")


# ---------------------------------------------------------------------------------------------------------------------
# Dropout + output Dense in one pass over the concat buffer (csrc/classifier.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _dd_workspace(n: int, k: int, c: int, device) -> torch.Tensor:
    nbytes = int(_capi.lib().h2gcn_dropout_dense_workspace_bytes(n, k, c))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _classifier_launch(stem: str, x, sel: Optional[RowSelection], rows_out: int, c: int, *args) -> None:
    """One call of ``<stem>[_rows]_{f32,bf16}``, the symbol picked from ``(x.dtype, sel is None)``.  ``args``: the arguments in
    front of ``(workspace, workspace_bytes, stream)``, which every symbol takes next (the workspace sized for ``rows_out`` rows);
    the row-selected symbols end in ``(rows, n_sel)``."""
    fn = getattr(_capi.lib(), stem + ("" if sel is None else "_rows") + ("_bf16" if x.dtype == torch.bfloat16 else "_f32"))
    ws = _dd_workspace(rows_out, x.shape[1], c, x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _capi.check(fn(*args, _ptr(ws), ws.numel(), ctypes.c_void_p(stream), *(() if sel is None else (_ptr(sel.rows), len(sel)))))


def _classifier_forward(x, w, bias, keep_prob, seed, step_dev, sel: Optional[RowSelection] = None) -> torch.Tensor:
    """``Z = (X .* M / keep) @ W + b`` on the library's kernels: ``[n, C]``, or -- ``sel`` -- the logits ``[len(sel), C]`` of rows
    ``sel.rows`` of ``x``.  ``x`` float32 or bfloat16, ``w`` contiguous."""
    n, k = x.shape
    c, m = w.shape[1], n if sel is None else len(sel)
    z = torch.empty((m, c), dtype=torch.float32, device=x.device)
    _classifier_launch("h2gcn_dropout_dense", x, sel, m, c,
                       _ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(bias), float(keep_prob), int(seed), _ptr(step_dev),
                       _ptr(z), z.stride(0))
    return z


def _classifier_backward(x, w, g, keep_prob, seed, step_dev, need_dx: bool, need_dw: bool, sel: Optional[RowSelection] = None):
    """``(dX in x's dtype, dW [K, C] float32)`` for the contiguous logit gradient ``g`` (either may be None: not computed).
    ``sel``: ``g`` and ``dX`` are compact, ``[len(sel), .]``."""
    n, k = x.shape
    c, m = w.shape[1], n if sel is None else len(sel)
    bf16 = x.dtype == torch.bfloat16
    # (a bf16 dX needs an even row stride: an odd K gets one padding column)
    dx = torch.empty((m, k + (k % 2 if bf16 else 0)), dtype=x.dtype, device=x.device)[:, :k] if need_dx else None
    dw = torch.empty((k, c), dtype=torch.float32, device=x.device) if need_dw else None
    if need_dx or need_dw:
        dx_dtype = (_capi.DTYPE_BF16,) if bf16 else ()   # an argument of the _bf16 symbols only
        _classifier_launch("h2gcn_dropout_dense_backward", x, sel, m, c,
                           _ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g), g.stride(0), float(keep_prob), int(seed), _ptr(step_dev),
                           *dx_dtype, _ptr(dx), dx.stride(0) if need_dx else k, _ptr(dw))
    return dx, dw


def _dd_rows_forward(x, w, bias, keep_prob, seed, step_dev, sel: RowSelection) -> torch.Tensor:
    """The row-selected forward under its earlier name and argument order (tests/test_special_values_gpu.py calls it)."""
    return _classifier_forward(x, w, bias, keep_prob, seed, step_dev, sel)


def _dd_rows_backward(x, w, g, keep_prob, seed, step_dev, sel: RowSelection, need_dx: bool, need_dw: bool):
    """The row-selected backward under its earlier name and argument order."""
    return _classifier_backward(x, w, g, keep_prob, seed, step_dev, need_dx, need_dw, sel)


def _saved_step(step_dev, device) -> torch.Tensor:
    return step_dev if step_dev is not None else torch.empty(0, device=device)


class _DropoutDenseFn(torch.autograd.Function):
    """``Z = (X .* M / keep) @ W + b`` and its gradients on the library's fp32-MFMA kernels; the mask ``M`` is a counter-based
    function of (seed, step, row, column), recomputed in the backward kernels instead of being stored.  ``X`` float32 or
    bfloat16 (the ``_bf16`` entry points: ``Z`` / ``dW`` float32 and bit-identical to the float32 call on ``X.float()``, ``dX``
    bfloat16)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, keep_prob, seed, step_dev):
        w = kernel.contiguous()
        ctx.save_for_backward(x, w, _saved_step(step_dev, x.device))
        ctx.keep_prob, ctx.seed, ctx.has_bias, ctx.has_step = float(keep_prob), int(seed), bias is not None, step_dev is not None
        return _classifier_forward(x, w, bias, keep_prob, seed, step_dev)

    @staticmethod
    def backward(ctx, g):
        x, w, step = ctx.saved_tensors
        g = g.contiguous()
        dx, dw = _classifier_backward(x, w, g, ctx.keep_prob, ctx.seed, step if ctx.has_step else None,
                                      ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None


def _rows_symbols() -> None:
    if not _capi.has("h2gcn_dropout_dense_rows_f32"):
        raise RuntimeError(f"{_capi.library_path()} predates the row-selected classifier (h2gcn_dropout_dense_rows_f32): rebuild it")


class _DropoutDenseRowsFn(torch.autograd.Function):
    """``DropoutDense(x, rows=sel)`` on its own: compact logits, gradients for ``kernel`` and ``bias`` only -- the compact
    ``dX`` has no place in an autograd graph whose node must return a gradient of ``x``'s shape (the training path that needs
    it is :func:`fused_propagation_classify_rows`)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, keep_prob, seed, step_dev, sel):
        w = kernel.contiguous()
        ctx.save_for_backward(x, w, _saved_step(step_dev, x.device))
        ctx.keep_prob, ctx.seed, ctx.has_bias, ctx.has_step, ctx.sel = float(keep_prob), int(seed), bias is not None, step_dev is not None, sel
        return _classifier_forward(x, w, bias, keep_prob, seed, step_dev, sel)

    @staticmethod
    def backward(ctx, g):
        x, w, step = ctx.saved_tensors
        g = g.contiguous()
        _, dw = _classifier_backward(x, w, g, ctx.keep_prob, ctx.seed, step if ctx.has_step else None, False, ctx.needs_input_grad[1], ctx.sel)
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return None, dw, db, None, None, None, None


class _PropagationClassifyRowsFn(torch.autograd.Function):
    """Propagation + classifier on selected rows as ONE autograd node: inputs ``r0``, ``kernel``, ``bias``; output the compact
    logits ``Z_c [m, C]``.  One node because the classifier's input gradient is compact (``[m, W]``: the rows of the concat
    buffer's gradient that are not zero) and a node boundary between the two would need it at the buffer's shape.

    Forward: the full ``[N, W]`` propagation exactly as :class:`_FusedPropagation` runs it (same buffer, ``out`` / ``reuse``,
    bfloat16), then the row-selected classifier forward.  Backward, with ``g_c = dX_c`` and ``rows = sel.rows``::

        round K:          t = sel.plan.spmm_t(g_c[:, slot_K])      [N, w_{K-1}]   (gathers m rows' gradient, not N)
                          t[rows] += g_c[:, slot_{K-1}]                           (rows are unique: deterministic)
        rounds K-1 .. 1:  t = plan.spmm_t(g_k);  t[rows] += g_c[:, slot_{k-1}]

    -- :func:`_backward_walk` over the compact gradient, with these two as its adjoint and its slot addition; bfloat16 rounds
    where that walk says."""

    @staticmethod
    def forward(ctx, r0, kernel, bias, plan, sel, layout, out, reuse, dtype, keep_prob, seed, step_dev):
        buf = _propagate(layout, plan, r0, out, reuse, dtype)
        w = kernel.contiguous()
        z = _classifier_forward(buf, w, bias, keep_prob, seed, step_dev, sel)
        ctx.save_for_backward(buf, w, _saved_step(step_dev, buf.device))
        ctx.plan, ctx.sel, ctx.layout = plan, sel, layout
        ctx.keep_prob, ctx.seed, ctx.has_bias, ctx.has_step = float(keep_prob), int(seed), bias is not None, step_dev is not None
        return z

    @staticmethod
    def backward(ctx, g):
        buf, w, step = ctx.saved_tensors
        plan, sel, layout = ctx.plan, ctx.sel, ctx.layout
        g = g.contiguous()
        need_r0 = ctx.needs_input_grad[0]
        g_c, dw = _classifier_backward(buf, w, g, ctx.keep_prob, ctx.seed, step if ctx.has_step else None, need_r0, ctx.needs_input_grad[1], sel)
        db = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        d_r0 = None
        if need_r0:
            bf16 = buf.dtype == torch.bfloat16
            d_r0 = _backward_walk(
                layout, g_c, bf16=bf16,
                # round K gathers through A_k[rows]^T, the others through A_k^T
                adjoint=lambda k, g_k: (sel.plan if k == layout.rounds else plan).spmm_t(g_k, out_dtype=torch.float32),
                add_slot=lambda t, slot: t.index_add_(0, sel.rows_long, slot.float() if bf16 else slot))
        return d_r0, dw, db, None, None, None, None, None, None, None, None, None


def fused_propagation_classify_rows(plan: HopPlan, sel: RowSelection, r0: torch.Tensor, rounds: int, dense_layer: "DropoutDense",
                                    out: Optional[torch.Tensor] = None, reuse: bool = False,
                                    dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``dense_layer(fused_propagation(plan, r0, rounds))[sel.rows]`` -- the logits of the selected rows, ``[m, units]`` -- with
    a backward that works on those rows only (:class:`_PropagationClassifyRowsFn`): a loss that lives on ``sel.rows`` has a
    zero logit gradient everywhere else, so the classifier's backward and the widest adjoint launch need ``m`` rows, not ``N``.

    ``sel = plan.select_rows(...)`` (with its transpose); ``out`` / ``reuse`` / ``dtype`` as in :func:`fused_propagation`.
    ``dense_layer`` is the :class:`DropoutDense` that consumes the buffer: its step counter advances exactly as in the full
    path, so with equal seeds both paths draw the same dropout mask, and the logits are bit-identical to the full path's rows.
    Gradients equal the full path's up to summation order."""
    if not isinstance(sel, RowSelection):
        raise TypeError(f"sel must be a RowSelection (HopPlan.select_rows), got {type(sel).__name__}")
    if not isinstance(plan, HopPlan):
        raise ValueError(f"fused_propagation_classify_rows: plan must be a HopPlan, got {type(plan).__name__} "
                         "(row-partitioned hops are not covered)")
    if sel.n_rows_full != plan.n_rows or sel.plan.n_cols != plan.n_cols or sel.plan.n_hops != plan.n_hops:
        raise ValueError("fused_propagation_classify_rows: sel was not taken from this plan")
    if not isinstance(dense_layer, DropoutDense):
        raise ValueError(f"fused_propagation_classify_rows: dense_layer must be a DropoutDense, got {type(dense_layer).__name__}")
    if dense_layer.kernel.shape[1] > 64:
        raise ValueError(f"fused_propagation_classify_rows: the classifier kernels cover units <= 64, got {dense_layer.kernel.shape[1]}")
    layout, dtype = _check_propagation("fused_propagation_classify_rows", plan, r0, rounds, out, reuse, dtype, rows_only=True)
    _rows_symbols()
    keep_prob, step = dense_layer._draw_step()
    if torch.is_grad_enabled() and (r0.requires_grad or dense_layer.kernel.requires_grad):
        if not sel.plan.has_transpose and r0.requires_grad:
            raise ValueError("fused_propagation_classify_rows: sel was built without its transpose (select_rows(build_transpose=True))")
        return _PropagationClassifyRowsFn.apply(r0, dense_layer.kernel, dense_layer.bias, plan, sel, layout, out, reuse, dtype,
                                                keep_prob, dense_layer.seed, step)
    buf = _propagate(layout, plan, r0, out, reuse, dtype)
    return _classifier_forward(buf, dense_layer.kernel.contiguous(), dense_layer.bias, keep_prob, dense_layer.seed, step, sel)


def _fused_classifier_covers(x: torch.Tensor, units: int) -> bool:
    """The layout rule of the classifier kernels: a 2-D float32 or bfloat16 CUDA tensor with unit column stride, at most 64
    units; bfloat16 rows are read in dwords (even row stride, 4-byte aligned base)."""
    return (x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16) and units <= 64
            and (x.shape[1] <= 1 or x.stride(1) == 1) and x.stride(0) >= x.shape[1]
            and (x.dtype != torch.bfloat16 or (x.stride(0) % 2 == 0 and x.data_ptr() % 4 == 0)))


class DropoutDense(torch.nn.Module):
    """keras ``Dropout(rate)`` followed by ``Dense(units)`` -- the ``D0.5-MO`` tail of the network setup (reference
    ``h2gcn/models/H2GCN.py:235-257``, called in order at ``:308-325``) -- as ONE pass over the ``[N, K]`` input per
    direction: the dropout mask is drawn from a counter-based generator inside the fp32-MFMA product kernels of
    ``csrc/classifier.hip`` (forward, ``dX``, ``dW``) instead of being materialised by a pass of its own.  Same parameters
    as the unfused pair (``kernel [K, units]``, optional ``bias``); in evaluation the mask is off and the layer is the plain
    product.  A bfloat16 input (the buffer of a bfloat16 propagation: CUDA, 2-D, even row stride) takes the ``_bf16`` entry
    points: float32 logits, float32 ``dW``, a bfloat16 ``dX``.  Inputs the kernels do not cover (CPU tensors, ``units > 64``,
    other dtypes or layouts) take the stock two-op path, upcast to float32 first -- correct, and the slow path.

    The mask stream differs from torch's (and from TensorFlow's, which nothing can reproduce): one mask per training
    forward, keyed by ``(seed, step)``; ``step`` lives in a device counter bumped by a stream-ordered op, so a replayed
    hipGraph draws a fresh mask every epoch."""

    def __init__(self, input_dim: int, units: int, use_bias: bool, drop_prob: float, seed: Optional[int] = None):
        super().__init__()
        self.kernel = torch.nn.Parameter(torch.empty(input_dim, units))
        torch.nn.init.xavier_uniform_(self.kernel)
        self.bias = torch.nn.Parameter(torch.zeros(units)) if use_bias else None
        self.drop_prob = float(drop_prob)
        if seed is None:
            # the mask is a pure function of (seed, step, row, column group) and every layer's step counter advances in
            # lock step: without a per-layer salt two DropoutDense layers of one model would draw IDENTICAL masks.  The
            # salt is drawn from torch's default generator right after the kernel's initialisation, like one more weight:
            # a pure function of torch.manual_seed and the construction order of THIS model -- never of what else the
            # process built before (repeated runs of run_experiments, one test after another).  H2GCN passes
            # seed = initial_seed + layer index explicitly.
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            # row-partitioned runs: the kernels index the mask by LOCAL row, so every rank gets its own stream (otherwise row i
            # of every shard would be dropped identically)
            self.seed = (self.seed ^ (torch.distributed.get_rank() * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF
        self.register_buffer("_step", torch.zeros(1, dtype=torch.int64), persistent=False)

    def _draw_step(self):
        """``(keep_prob, step)`` of one forward: in training the step counter advances (stream-ordered: a captured graph
        bumps it on every replay) and ``step`` is the value this forward and its backward use."""
        if not (self.training and self.drop_prob > 0.0):
            return 1.0, None
        self._step += 1
        return 1.0 - self.drop_prob, self._step.clone()

    def forward(self, x: torch.Tensor, rows: Optional[RowSelection] = None) -> torch.Tensor:
        """``rows``: a :class:`h2gcn_amd.hops.RowSelection` -- the logits of those rows only, ``[m, units]``, bit-identical to
        the same rows of the full result (the mask is keyed by the original row).  Meant for inference on a node subset
        (``torch.no_grad()``); with gradients enabled ``kernel`` and ``bias`` get theirs, ``x`` must not require one."""
        if rows is not None:
            return self._forward_rows(x, rows)
        if not _fused_classifier_covers(x, self.kernel.shape[1]):
            if x.dtype == torch.bfloat16:
                x = x.to(self.kernel.dtype)
            if self.training and self.drop_prob > 0.0:
                x = torch.nn.functional.dropout(x, self.drop_prob, True)
            y = x @ self.kernel
            return y if self.bias is None else y + self.bias
        if x.dtype == torch.bfloat16 and not _capi.has("h2gcn_dropout_dense_bf16"):
            raise RuntimeError(f"{_capi.library_path()} predates the bf16 classifier (h2gcn_dropout_dense_bf16): rebuild it")
        keep_prob, step = self._draw_step()
        return _DropoutDenseFn.apply(x, self.kernel, self.bias, keep_prob, self.seed, step)

    def _forward_rows(self, x: torch.Tensor, sel: RowSelection) -> torch.Tensor:
        if not isinstance(sel, RowSelection):
            raise TypeError(f"rows must be a RowSelection (HopPlan.select_rows), got {type(sel).__name__}")
        if not _fused_classifier_covers(x, self.kernel.shape[1]):   # no stock path here: it would draw another mask
            raise ValueError("DropoutDense(x, rows=...) runs on the row-selected classifier kernels only: x must be a 2-D float32 or "
                             "bfloat16 CUDA tensor with unit column stride (bfloat16: even row stride) and units <= 64")
        if x.shape[0] != sel.n_rows_full or sel.rows.device != x.device:
            raise ValueError(f"rows were selected from {sel.n_rows_full} rows on {sel.rows.device}, x has {x.shape[0]} rows on {x.device}")
        if x.requires_grad and torch.is_grad_enabled():
            raise ValueError("DropoutDense(x, rows=...) cannot return a gradient for x (it would be compact): train through "
                             "layers.fused_propagation_classify_rows, or detach x")
        _rows_symbols()
        keep_prob, step = self._draw_step()
        return _DropoutDenseRowsFn.apply(x, self.kernel, self.bias, keep_prob, self.seed, step, sel)

    def extra_repr(self) -> str:
        return f"in={self.kernel.shape[0]}, units={self.kernel.shape[1]}, bias={self.bias is not None}, drop={self.drop_prob}"
