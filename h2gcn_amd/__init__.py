"""h2gcn_amd -- MI355X-native hop aggregation for H2GCN (the GCNLayer path of GemsLab/H2GCN).

The package is a thin PyTorch-ROCm front end over ``libh2gcn_hip.so`` (hand-written gfx950 HIP behind the
C ABI of ``include/h2gcn_hip.h``).  It mirrors the reference's operator interface for this one path:

* :class:`h2gcn_amd.layers.GCNLayer` -- ``layer(adjhops, inputs) -> [N, H, d]``
  (reference ``h2gcn/models/_layers.py:54-81``);
* :func:`h2gcn_amd.layers.hop_softmax` -- softmax per (row, hop) segment of the pattern: attention coefficients for
  ``hop_spmm(..., values=...)`` (new; the reference's adjacency is constant);
* :func:`h2gcn_amd.layers.hop_edge_scores` / :class:`h2gcn_amd.layers.HopAttention` -- additive (GAT-style) scores on the
  pattern from per-node terms, differentiable back to the nodes without atomics, and the layer that chains scores, softmax and
  aggregation with the calling convention of ``GCNLayer`` (new);
* :func:`h2gcn_amd.layers.hop_spmm_values` -- the aggregation on values handed to the launch, with an optional head dimension:
  nothing is installed in the plan; :class:`h2gcn_amd.layers.MultiHeadHopAttention` is the multi-head attention layer on it, stackable
  on one plan (new);
* :func:`h2gcn_amd.layers.hop_edge_scores_heads` / :func:`h2gcn_amd.layers.hop_softmax_heads` -- scores and softmax for all heads
  in one launch each on entry-major ``[nnz_k, K]`` arrays, the links ``MultiHeadHopAttention`` chains (new);
* :func:`h2gcn_amd.layers.hop_attention_heads` -- scores, softmax and aggregation of all heads in ONE launch for every forward
  that needs no gradient (the chain's bits, no per-entry array) (new);
* :func:`h2gcn_amd.layers.hop_attention_recompute` / :class:`h2gcn_amd.layers.RecomputeMultiHeadHopAttention` -- the attention
  TRAINING step without per-entry arrays: a forward that stores the softmax statistics and a backward that recomputes per entry;
  :func:`h2gcn_amd.layers.hop_attention_recompute_dropout` / ``layer.set_attention_dropout(p)``: dropout on the attention
  coefficients, the mask drawn inside those kernels (new);
* :func:`h2gcn_amd.layers.hop_edge_scores_dynamic` / :class:`h2gcn_amd.layers.DynamicHopAttention` -- dynamic (GATv2) attention:
  ``a . leaky_relu(u[i] + v[j])`` per head in one launch per direction, without an ``nnz x d`` array (new);
* :class:`h2gcn_amd.hops.HopPlan` -- the device-resident ``adj_hops`` operand list
  (reference ``h2gcn/datasets/_dataset.py:559-576``);
* :mod:`h2gcn_amd.operands` -- construction of the normalised exact-k-hop matrices: on the device with the HIP ring
  kernels (``build_adj_norm_hops_device``) or on the host with scipy as the reference does
  (reference ``h2gcn/datasets/_dataset.py:102-158``);
* :mod:`h2gcn_amd.partition` -- row partitioning (equal or nnz-balanced blocks) + embedding exchange (RCCL all-gather or
  the library's IPC pulls) for 1..8 GPUs (new; the reference is single-device);
* :class:`h2gcn_amd.layers.DropoutDense` -- keras ``Dropout`` + output ``Dense`` (``D0.5-MO``) as one pass over the concat
  buffer per direction (reference ``h2gcn/models/H2GCN.py:235-257``);
* :meth:`h2gcn_amd.hops.HopPlan.select_rows` / :func:`h2gcn_amd.layers.fused_propagation_classify_rows` -- logits of, and the
  backward from, a subset of the nodes (the labelled rows a semi-supervised loss lives on; new, ``--train_rows_only``);
* :mod:`h2gcn_amd.metrics` -- masked softmax cross-entropy / accuracy in one pass over the logits
  (reference ``h2gcn/models/_metrics.py:8-25``);
* :class:`h2gcn_amd.optim.KerasAdam` -- the reference's optimizer step (Keras / TensorFlow Adam arithmetic) as one launch for
  all parameters (reference ``h2gcn/models/H2GCN.py:62-63, 73``).

Results of the aggregation are bit-reproducible functions of the operands (one canonical summation tree in every kernel):
any slicing, chunking or row partition gives the same bits.

There is no CPU fallback: every compute entry point raises if the HIP library or a GPU is missing.
"""

__version__ = "0.6.0"

from . import _capi  # noqa: F401  (does not load the library until first use)
from .hops import HopPlan, RowSelection  # noqa: F401
from .layers import (ConcatLayer, DropoutDense, DynamicHopAttention, GCNLayer, HopAttention, MultiHeadHopAttention, RecomputeMultiHeadHopAttention,  # noqa: F401
                     SliceLayer, SparseDense, SparseDropout, hop_attention_heads, hop_attention_recompute, hop_attention_recompute_dropout, hop_edge_scores,
                     hop_edge_scores_dynamic, hop_edge_scores_heads, hop_softmax, hop_softmax_heads, hop_spmm, hop_spmm_values)
