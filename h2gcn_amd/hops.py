"""HopPlan -- the device-resident ``adj_hops`` operand list of H2GCN and its launch plan.

Mirror of what the reference keeps in ``args.objects["tensors"]["adj_hops"]``: a Python list of H normalised
``tf.SparseTensor`` built once before training (reference ``h2gcn/models/H2GCN.py:46-54`` ->
``h2gcn/datasets/_dataset.py:559-576``, conversion ``sparse2Tensor`` ``:528-535``).  Here the list is one object:
CSR arrays on the GPU (int64 row pointers, int32 column ids in ascending order per row -- the canonical order
``tf.sparse.reorder`` establishes -- fp32 values) plus the opaque plan of ``libh2gcn_hip.so`` (the segment-class bins of the
CSR-adaptive schedule: lists of the long and of the short (row, hop) segments, see :meth:`HopPlan.segment_classes`;
optional transposed operands for the backward pass).
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import torch

from . import _capi


def _require(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _bf16_layout(name: str, t: torch.Tensor, d: int, strides) -> None:
    """The C ABI's rule for bf16 arrays: 4-byte aligned base, even strides (elements), even width."""
    _require(d % 2 == 0, f"bf16 {name}: the feature width d must be even (got {d})")
    _require(t.data_ptr() % 4 == 0, f"bf16 {name}: the base address must be 4-byte aligned")
    for st in strides:
        _require(st % 2 == 0, f"bf16 {name}: row / hop strides must be even (got {tuple(strides)} elements)")


def _bf16_symbols() -> None:
    _require(_capi.has("h2gcn_spmm_hops_bf16"), f"{_capi.library_path()} predates the bf16 launches (ABI 5)")


class HopPlan:
    """H hop matrices sharing one row space, resident on one GPU.

    Results are bit-reproducible functions of the operands: every launch builds the library's canonical per-row
    summation tree (``include/h2gcn_hip.h``), whatever slice width, scratch copy or segment walk the schedule picks.

    Embeddings / gradients may be float32 or bfloat16 (the gathered operand; adjacency values stay float32).  A bfloat16
    operand is widened exactly and summed in fp32 in the same tree: an fp32 result equals the launch on ``x.float()`` bit for
    bit, a bfloat16 result is that value ``.to(torch.bfloat16)``.  bfloat16 needs an even width and even strides.

    Parameters
    ----------
    rowptr, colidx, vals : sequences of H CUDA tensors (int64 ``[n_rows+1]``, int32 ``[nnz]``, float32 ``[nnz]``)
    n_cols : number of columns (rows of the dense operand ``X``)
    build_transpose : also build ``A_k^T`` on the device (needed for ``backward``)
    keep_permutation : with ``build_transpose``: remember where every transposed entry came from, so that :meth:`set_values`
        can refresh ``A_k^T`` (kept as the attribute ``keep_permutation``)
    long_row_threshold, rows_per_wave, variant, slice_cols : schedule tunables (0 = library default)
    validate : run the one-time column-range check (TensorFlow validates indices per call; this once)
    symmetric_pattern : the caller states that every ``A_k`` is square and stores ``(j, i)`` exactly when it stores ``(i, j)``
        (the adjacency rings of an undirected graph).  With ``build_transpose=True`` the backward then runs on these very
        arrays: no transposed copy is built or held (``H2GCN_PLAN_SYMMETRIC_PATTERN``).  The library verifies the statement
        on the device and refuses an operand that breaks it, naming the first entry without a mirror; results are bit for bit
        those of a plan with built transposes.  See :attr:`transpose_sharing` and :meth:`device_bytes`.
    """

    def __init__(self, rowptr: Sequence[torch.Tensor], colidx: Sequence[torch.Tensor],
                 vals: Sequence[torch.Tensor], n_cols: int, *, build_transpose: bool = False,
                 long_row_threshold: int = 0, rows_per_wave: int = 0, variant: int = 0,
                 slice_cols: int = 0, validate: bool = True, host_transpose: bool = False,
                 keep_permutation: bool = False, symmetric_pattern: bool = False):
        H = len(rowptr)
        _require(1 <= H <= _capi.MAX_HOPS, f"need 1..{_capi.MAX_HOPS} hop matrices, got {H}")
        _require(len(colidx) == H and len(vals) == H, "rowptr/colidx/vals lists differ in length")
        dev = rowptr[0].device
        _require(dev.type == "cuda", f"HopPlan operands must live on a GPU, got {dev} (no CPU fallback)")
        n_rows = rowptr[0].numel() - 1
        _require(n_rows >= 0, "rowptr must have n_rows+1 entries")
        for k in range(H):
            rp, ci, va = rowptr[k], colidx[k], vals[k]
            _require(rp.dtype == torch.int64 and ci.dtype == torch.int32 and va.dtype == torch.float32,
                     f"hop {k}: dtypes must be int64/int32/float32, got {rp.dtype}/{ci.dtype}/{va.dtype}")
            _require(rp.device == dev and ci.device == dev and va.device == dev, f"hop {k}: operands on different devices")
            _require(rp.dim() == 1 and rp.numel() == n_rows + 1, f"hop {k}: rowptr has {rp.numel()} entries, expected {n_rows + 1}")
            _require(ci.dim() == 1 and va.dim() == 1 and ci.numel() == va.numel(), f"hop {k}: colidx/vals sizes differ")
            _require(rp.is_contiguous() and ci.is_contiguous() and va.is_contiguous(), f"hop {k}: operands must be contiguous")
        if symmetric_pattern:
            _require(build_transpose, "symmetric_pattern=True modifies build_transpose=True, which is not set")
            _require(not host_transpose, "symmetric_pattern=True builds no transpose: it cannot be combined with host_transpose=True")
            _require(n_rows == int(n_cols), f"symmetric_pattern=True needs square operands, got {n_rows} x {int(n_cols)}")
            if not _capi.has("h2gcn_plan_transpose_sharing"):   # (it would ignore the unknown flag bit silently)
                raise RuntimeError(f"{_capi.library_path()} predates symmetric plans (H2GCN_PLAN_SYMMETRIC_PATTERN)")
        # the schedule tunables, so that select_rows can build its sub-plan the same way
        self._tunables = dict(long_row_threshold=long_row_threshold, rows_per_wave=rows_per_wave, variant=variant, slice_cols=slice_cols)
        self.n_hops = H
        self.n_rows = int(n_rows)
        self.n_cols = int(n_cols)
        self.device = dev
        self.has_transpose = bool(build_transpose)
        #: the plan can refresh its transposed operands when :meth:`set_values` brings new values
        self.keep_permutation = bool(keep_permutation and build_transpose)
        # the plan borrows these arrays: keep them alive
        self.rowptr = list(rowptr)
        self.colidx = list(colidx)
        self.vals = list(vals)
        self._handle = C.c_void_p()
        #: let launches use scratch memory for the slice-major copy of X (see h2gcn_spmm_workspace_bytes)
        self.use_workspace = True
        #: narrowest feature chunk a pipeline may cut: any width gives the same bits (one canonical summation tree in every
        #: kernel); below 16 columns a chunk is just not worth its extra pass over the indices
        self.min_chunk_cols = 16

        L = _capi.lib()
        arr_t = C.c_void_p * H
        rp_a = arr_t(*[t.data_ptr() for t in self.rowptr])
        ci_a = arr_t(*[t.data_ptr() for t in self.colidx])
        va_a = arr_t(*[t.data_ptr() for t in self.vals])
        opts = _capi.PlanOpts()
        opts.struct_size = C.sizeof(_capi.PlanOpts)
        opts.flags = ((_capi.PLAN_BUILD_TRANSPOSE if build_transpose else 0) | (0 if validate else _capi.PLAN_SKIP_VALIDATION)
                      | (_capi.PLAN_HOST_TRANSPOSE if host_transpose else 0)
                      | (_capi.PLAN_KEEP_PERMUTATION if keep_permutation and build_transpose else 0)
                      | (_capi.PLAN_SYMMETRIC_PATTERN if symmetric_pattern else 0))
        opts.long_row_threshold = int(long_row_threshold)
        opts.rows_per_wave = int(rows_per_wave)
        opts.variant = int(variant)
        opts.slice_cols = int(slice_cols)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            st = L.h2gcn_plan_create(H, self.n_rows, self.n_cols, rp_a, ci_a, va_a, C.byref(opts),
                                     C.c_void_p(stream), C.byref(self._handle))
        _capi.check(st)

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_scipy(cls, mats: Iterable, device, **kw) -> "HopPlan":
        """Upload a list of scipy sparse matrices (any format; cast to fp32 CSR with sorted indices -- the
        same cast/ordering ``sparse2Tensor`` applies, reference ``h2gcn/datasets/_dataset.py:528-535``)."""
        import numpy as np
        import scipy.sparse as sp

        rowptr, colidx, vals = [], [], []
        n_cols = None
        n_rows = None
        for m in mats:
            m = sp.csr_matrix(m)
            m.sum_duplicates()
            m.sort_indices()
            _require(n_cols in (None, m.shape[1]) and n_rows in (None, m.shape[0]), "hop matrices differ in shape")
            n_rows, n_cols = m.shape
            rowptr.append(torch.from_numpy(m.indptr.astype(np.int64)).to(device))
            colidx.append(torch.from_numpy(m.indices.astype(np.int32)).to(device))
            vals.append(torch.from_numpy(m.data.astype(np.float32)).to(device))
        _require(n_cols is not None, "empty hop list")
        return cls(rowptr, colidx, vals, n_cols, **kw)

    def set_values(self, hop: int, vals: torch.Tensor) -> None:
        """New values for hop ``hop`` (same pattern); the transposed operand is refreshed too (plans built with
        ``keep_permutation=True``).  ``vals`` is borrowed like the original arrays.  See ``h2gcn_plan_set_values``."""
        _require(vals.dtype == torch.float32 and vals.device == self.device and vals.is_contiguous()
                 and vals.numel() == self.colidx[hop].numel(), "vals must be a contiguous float32 array of the hop's nnz")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _capi.check(_capi.lib().h2gcn_plan_set_values(self._handle, int(hop), C.c_void_p(vals.data_ptr()), C.c_void_p(stream)))
        self.vals[hop] = vals
        self.values_version = getattr(self, "values_version", 0) + 1   # anything cached as a function of the values is stale

    def select_rows(self, rows, build_transpose: bool = True) -> "RowSelection":
        """The hop matrices restricted to a set of rows: ``RowSelection(rows, plan, n_rows_full)`` with ``plan`` a
        :class:`HopPlan` of ``A_k[rows, :]`` (shape ``[m, n_cols]``) -- what the backward of a loss that lives on these rows
        needs (``sel.plan.spmm_t`` gathers a COMPACT ``[m, H, d]`` gradient through ``A_k[rows]^T``), and what
        ``DropoutDense(x, rows=sel)`` takes for logits of a node subset.

        ``rows``: a bool mask ``[n_rows]`` or an integer index tensor / sequence (any order; it is sorted).  Duplicates,
        indices outside ``[0, n_rows)`` and an empty selection raise ``ValueError``.  ``sel.rows`` is int32, ascending and
        unique, on the plan's device.

        The sub-CSR is built on the device with torch ops (row-length gather, cumsum, segmented index arithmetic); it keeps
        the per-row column order and the values of this plan, so its launches give the bits of a plan built from the same
        sub-matrices.  ``A_k[rows, :]`` is not square: the sub-plan of a ``symmetric_pattern`` plan builds its own transpose like
        any other.  One-off set-up (it synchronises: the checks and the sub-matrix sizes are read back) -- call it before
        any hipGraph capture, never inside one.

        Memory: the sub-plan holds its own copy of the selected rows' column ids and values, and of their transpose when
        ``build_transpose`` -- about ``2 * m / n_rows`` of this operand's bytes for a selection of average row length
        (``m / n_rows`` without the transpose), plus two ``[m]`` index arrays."""
        _require(self.device.type == "cuda", f"select_rows: the plan must live on a GPU, got {self.device} (no CPU fallback)")
        t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows)
        if t.dtype == torch.bool:
            _require(t.dim() == 1 and t.numel() == self.n_rows, f"select_rows: a bool mask must have shape [{self.n_rows}], got {tuple(t.shape)}")
            idx = torch.nonzero(t.to(self.device)).flatten()
            _require(idx.numel() > 0, "select_rows: empty selection")
        else:
            _require(not (t.is_floating_point() or t.is_complex()), f"select_rows: rows must be a bool mask or integer indices, got {t.dtype}")
            _require(t.dim() == 1, f"select_rows: an index tensor must be one-dimensional, got shape {tuple(t.shape)}")
            _require(t.numel() > 0, "select_rows: empty selection")
            idx = torch.sort(t.to(self.device, torch.int64)).values
            lo, hi = int(idx[0]), int(idx[-1])
            _require(lo >= 0 and hi < self.n_rows, f"select_rows: row index {lo if lo < 0 else hi} outside [0, {self.n_rows})")
            _require(not bool((idx[1:] == idx[:-1]).any()), "select_rows: duplicate row indices")
        m = int(idx.numel())
        rowptr, colidx, vals = [], [], []
        for k in range(self.n_hops):
            rp = self.rowptr[k]
            begin = rp[idx]
            lens = rp[idx + 1] - begin
            sub_rp = torch.zeros(m + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(lens, 0, out=sub_rp[1:])
            nnz = int(sub_rp[-1])
            # entry e of the sub-matrix, in row i, is entry begin[i] + (e - sub_rp[i]) of the parent
            src = torch.arange(nnz, dtype=torch.int64, device=self.device) + torch.repeat_interleave(begin - sub_rp[:-1], lens, output_size=nnz)
            rowptr.append(sub_rp)
            colidx.append(self.colidx[k][src].contiguous())
            vals.append(self.vals[k][src].contiguous())
        plan = HopPlan(rowptr, colidx, vals, self.n_cols, build_transpose=build_transpose, validate=False, **self._tunables)
        return RowSelection(idx.to(torch.int32), plan, self.n_rows)

    # ------------------------------------------------------------------ introspection
    @property
    def nnz(self) -> list:
        return [int(t.numel()) for t in self.colidx]

    def info(self, hop: int) -> dict:
        L = _capi.lib()
        n_rows, n_cols, nnz, n_long = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        has_t = C.c_int32()
        _capi.check(L.h2gcn_plan_info(self._handle, hop, C.byref(n_rows), C.byref(n_cols), C.byref(nnz),
                                      C.byref(n_long), C.byref(has_t)))
        return dict(n_rows=n_rows.value, n_cols=n_cols.value, nnz=nnz.value, n_long_segments=n_long.value,
                    has_transpose=bool(has_t.value))

    @property
    def transpose_sharing(self) -> list:
        """Per hop, what the backward's operand shares with the forward arrays: ``"none"`` (a built transpose, or no transpose),
        ``"indices"`` or ``"indices+values"`` (``symmetric_pattern`` plans; the values are shared when they are bit-symmetric and
        ``keep_permutation`` is off)."""
        if not _capi.has("h2gcn_plan_transpose_sharing"):
            return ["none"] * self.n_hops
        L = _capi.lib()
        out = []
        for k in range(self.n_hops):
            v = L.h2gcn_plan_transpose_sharing(self._handle, k)
            _capi.check(v)
            out.append(("none", "indices", "indices+values")[v])
        return out

    @property
    def row_constant(self) -> list:
        """Per hop, 1 when every stored value of each row carries the bits of the row's first one (established at plan creation,
        cleared by :meth:`set_values`), else 0: forward launches whose selected hops are all row-constant do not read the value
        arrays (``h2gcn_plan_row_constant``)."""
        if not _capi.has("h2gcn_plan_row_constant"):
            return [0] * self.n_hops
        L = _capi.lib()
        out = []
        for k in range(self.n_hops):
            v = L.h2gcn_plan_row_constant(self._handle, k)
            _capi.check(v)
            out.append(int(v))
        return out

    def device_bytes(self) -> int:
        """Device memory the plan owns now, in bytes: transposed arrays, permutations, a symmetric plan's transposed values, and
        the row lists built so far -- never the operand arrays it borrows (``h2gcn_plan_device_bytes``)."""
        if not _capi.has("h2gcn_plan_device_bytes"):
            raise RuntimeError(f"{_capi.library_path()} predates h2gcn_plan_device_bytes")
        return int(_capi.lib().h2gcn_plan_device_bytes(self._handle))

    def schedule(self, d: int, ld_src: Optional[int] = None, hops=None, adjoint: bool = False) -> dict:
        """What a launch at feature width ``d`` (source row stride ``ld_src``, default contiguous) would do."""
        L = _capi.lib()
        sc, ns, pf, cp = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        ld = int(ld_src) if ld_src is not None else (self.n_selected(hops) * d if adjoint else d)
        _capi.check(L.h2gcn_plan_schedule(self._handle, self._mask(hops), 1 if adjoint else 0, ld, int(d),
                                          C.byref(sc), C.byref(ns), C.byref(pf), C.byref(cp)))
        return dict(slice_cols=sc.value, n_slices=ns.value,
                    segment_walk={0: "wave per segment", 1: "wave per segment + index prefetch",
                                  2: "lane group per segment (short rows)",
                                  3: "lane group per segment (binned short segments) + wave per segment"}[pf.value],
                    scratch_copy=bool(cp.value) and self.use_workspace)

    def segment_classes(self, d: int, ld_src: Optional[int] = None, hops=None, adjoint: bool = False) -> dict:
        """CSR-adaptive dispatch of a launch at width ``d``: per selected hop the number of short (<= 16 nonzeros) / medium /
        long (>= long_row_threshold) segments and their nonzeros, which walk serves each class, and how many segments the
        launch takes from the binned short list (``listed``; 0 = the wave walk serves the short class too, -1 = in-tile
        short-row mode: rounds of consecutive short rows are grouped on the fly)."""
        L = _capi.lib()
        if not _capi.has("h2gcn_plan_segment_classes"):
            raise RuntimeError(f"{_capi.library_path()} predates h2gcn_plan_segment_classes (ABI 4)")
        h_sel = self.n_selected(hops)
        seg, nnz, listed = (C.c_int64 * (3 * h_sel))(), (C.c_int64 * (3 * h_sel))(), C.c_int64()
        ld = int(ld_src) if ld_src is not None else (h_sel * d if adjoint else d)
        _capi.check(L.h2gcn_plan_segment_classes(self._handle, self._mask(hops), 1 if adjoint else 0, ld, int(d), seg, nnz, C.byref(listed)))
        sel = self._selected(hops)
        short_walk = ("lane group per segment (binned list)" if listed.value > 0 else
                      "lane group per segment (rounds of consecutive short rows)" if listed.value < 0 else "wave per segment")
        per_hop = [dict(hop=sel[s], segments=dict(short=seg[3 * s], medium=seg[3 * s + 1], long=seg[3 * s + 2]),
                        nonzeros=dict(short=nnz[3 * s], medium=nnz[3 * s + 1], long=nnz[3 * s + 2])) for s in range(h_sel)]
        return dict(per_hop=per_hop, listed=listed.value,
                    walks=dict(short=short_walk, medium="wave per segment", long="workgroup per segment (4 waves, LDS-staged)"))

    def _mask(self, hops) -> int:
        if hops is None:
            return 0
        mask = 0
        for h in hops:
            _require(0 <= int(h) < self.n_hops, f"hop index {h} outside 0..{self.n_hops - 1}")
            mask |= 1 << int(h)
        _require(mask != 0, "empty hop selection")
        return mask

    def _selected(self, hops) -> list:
        """The selected hop indices in ascending order: slot ``s`` of a launch is hop ``_selected(hops)[s]``."""
        return list(range(self.n_hops)) if hops is None else sorted({int(h) for h in hops})

    def n_selected(self, hops) -> int:
        return self.n_hops if hops is None else bin(self._mask(hops)).count("1")

    # ------------------------------------------------------------------ launches
    def spmm(self, x: torch.Tensor, hops=None, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
             relu: bool = False, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """``out[i, s, :] = act(sum_j A_s[i, j] * x[j, :] + bias)`` for the selected hops -> ``[n_rows, H_sel, d]``
        (``bias`` [d] and ``relu`` are the optional fused epilogue of the store; default: the plain sum).

        ``x``: float32 or bfloat16.  The result's dtype is ``out.dtype``, else ``out_dtype``, else ``x.dtype``: float32 ->
        float32, bfloat16 -> float32 or bfloat16 (see the class docstring; float32 -> bfloat16 does not exist).  ``bias`` is
        float32 and the epilogue runs before the rounding to bfloat16.
        ``out`` may be any tensor view of shape ``[n_rows, H_sel, d]`` whose last dim is contiguous
        (e.g. a column slice of a wider concat buffer)."""
        _require(x.dim() == 2, f"inputs must be [n_cols, d], got shape {tuple(x.shape)}")
        _require(x.dtype in (torch.float32, torch.bfloat16), f"inputs must be float32 or bfloat16, got {x.dtype}")
        _require(x.device == self.device, f"inputs on {x.device}, plan on {self.device}")
        _require(x.shape[0] == self.n_cols, f"inputs have {x.shape[0]} rows, hop matrices have {self.n_cols} columns")
        d = int(x.shape[1])
        _require(d >= 1, "inputs need at least one column")
        bf16 = x.dtype == torch.bfloat16
        if out_dtype is None:
            out_dtype = out.dtype if out is not None else x.dtype
        _require(out_dtype in (torch.float32, torch.bfloat16), f"outputs must be float32 or bfloat16, got {out_dtype}")
        _require(bf16 or out_dtype == torch.float32, "float32 inputs give float32 outputs (float32 -> bfloat16 is not supported)")
        if x.stride(1) != 1:
            x = x.contiguous()
        h_sel = self.n_selected(hops)
        if out is None:
            out = torch.empty((self.n_rows, h_sel, d), dtype=out_dtype, device=self.device)
        else:
            _require(out.dtype == out_dtype and out.device == self.device, f"out must be {out_dtype} on the plan's device")
            _require(tuple(out.shape) == (self.n_rows, h_sel, d), f"out has shape {tuple(out.shape)}, expected {(self.n_rows, h_sel, d)}")
            _require(d == 1 or out.stride(2) == 1, "out's last dimension must be contiguous")
        if bf16:
            _bf16_symbols()
            _bf16_layout("inputs", x, d, (x.stride(0),))
            if out_dtype == torch.bfloat16:
                _bf16_layout("out", out, d, (out.stride(0), out.stride(1) if h_sel > 1 else d))
        if self.n_rows == 0:
            return out
        if bias is not None:
            _require(bias.dtype == torch.float32 and bias.device == self.device and bias.numel() == d and bias.is_contiguous(),
                     f"bias must be a contiguous float32 [{d}] tensor on the plan's device")
        L = _capi.lib()
        mask = self._mask(hops)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            # scratch for the slice-major copy of X the library wants when X's row stride is a multiple of 1 KiB, when
            # its rows are wide and not line-aligned, or when d % 4 != 0 / X is not 16-byte addressable (0 bytes
            # otherwise); a torch allocation, so it is stream-ordered and capturable in a hipGraph.  bf16 launches gather
            # in place (no scratch copy)
            ws_bytes = (int(L.h2gcn_spmm_workspace_bytes(self._handle, mask, 0, C.c_void_p(x.data_ptr()), x.stride(0), 0, d))
                        if self.use_workspace and not bf16 else 0)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device) if ws_bytes else None
            opts = None
            if ws is not None or bias is not None or relu:
                opts = _capi.LaunchOpts(struct_size=C.sizeof(_capi.LaunchOpts), flags=_capi.LAUNCH_RELU if relu else 0,
                                        workspace=ws.data_ptr() if ws is not None else None, workspace_bytes=ws_bytes,
                                        bias=bias.data_ptr() if bias is not None else None)
            fn, y_dtype = ((L.h2gcn_spmm_hops_bf16, (_capi.DTYPE_BF16 if out_dtype == torch.bfloat16 else _capi.DTYPE_F32,))
                           if bf16 else (L.h2gcn_spmm_hops_opts_f32, ()))
            st = fn(self._handle, mask, C.c_void_p(x.data_ptr()), x.stride(0), d, *y_dtype,
                    C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1) if h_sel > 1 else d,
                    C.byref(opts) if opts is not None else None, C.c_void_p(stream))
        _capi.check(st)
        return out

    def spmm_t(self, grad: torch.Tensor, hops=None, out: torch.Tensor = None, accumulate: bool = False,
               out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """Adjoint: ``dx[j, :] = sum_s sum_i A_s[i, j] * grad[i, s, :]`` -> ``[n_cols, d]``.  ``out``: write into this
        ``[n_cols, d]`` tensor (unit column stride, any row stride) instead of a new one; ``accumulate=True`` ADDS the
        result to what ``out`` holds (``H2GCN_LAUNCH_ACCUMULATE``: the `+=` of a gradient slot fused into the store).
        ``grad``: float32 or bfloat16; the dtype of ``dx`` is ``out.dtype``, else ``out_dtype``, else ``grad.dtype`` (as in
        :meth:`spmm`).  ``accumulate=True`` needs a float32 ``out``."""
        _require(self.has_transpose, "plan was built without build_transpose=True; backward is unavailable")
        h_sel = self.n_selected(hops)
        _require(grad.dim() == 3 and grad.shape[0] == self.n_rows and grad.shape[1] == h_sel,
                 f"grad must be [{self.n_rows}, {h_sel}, d], got {tuple(grad.shape)}")
        _require(grad.dtype in (torch.float32, torch.bfloat16) and grad.device == self.device,
                 "grad must be float32 or bfloat16 on the plan's device")
        d = int(grad.shape[2])
        bf16 = grad.dtype == torch.bfloat16
        if out_dtype is None:
            out_dtype = out.dtype if out is not None else grad.dtype
        _require(out_dtype in (torch.float32, torch.bfloat16), f"dx must be float32 or bfloat16, got {out_dtype}")
        _require(bf16 or out_dtype == torch.float32, "a float32 grad gives a float32 dx (float32 -> bfloat16 is not supported)")
        _require(not (accumulate and out_dtype == torch.bfloat16), "accumulate=True needs a float32 out (a bfloat16 dx cannot be accumulated into)")
        if grad.stride(2) != 1 or grad.stride(0) < d or (h_sel > 1 and grad.stride(1) < d):
            grad = grad.contiguous()  # e.g. an expanded (stride-0) gradient coming out of a reduction
        if out is None:
            _require(not accumulate, "accumulate=True needs the tensor to accumulate into (out=)")
            dx = torch.empty((self.n_cols, d), dtype=out_dtype, device=self.device)
        else:
            _require(out.shape == (self.n_cols, d) and out.dtype == out_dtype and out.device == self.device
                     and (out.stride(1) == 1 or d == 1) and (out.stride(0) >= d or self.n_cols <= 1),
                     f"out must be {out_dtype} [{self.n_cols}, {d}] on the plan's device with unit column stride")
            dx = out
        if bf16:
            _bf16_symbols()
            _bf16_layout("grad", grad, d, (grad.stride(0) if self.n_rows > 0 else h_sel * d, grad.stride(1) if h_sel > 1 else d))
            if out_dtype == torch.bfloat16:
                _bf16_layout("dx", dx, d, (dx.stride(0) if self.n_cols > 1 else d,))
        if self.n_cols == 0:
            return dx
        L = _capi.lib()
        mask = self._mask(hops)
        # (a single hop's stride is only checked for its sign and, bf16, its parity: pass d)
        ld_row, ld_hop = (grad.stride(0) if self.n_rows > 0 else h_sel * d), (grad.stride(1) if h_sel > 1 else d)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            # scratch: slice-major copy of the stacked gradient (same rules as the forward launch; fp32 only)
            ws_bytes = (int(L.h2gcn_spmm_workspace_bytes(self._handle, mask, 1, C.c_void_p(grad.data_ptr()), ld_row, ld_hop, d))
                        if self.use_workspace and not bf16 else 0)
            opts = None
            if ws_bytes or accumulate:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device) if ws_bytes else None
                opts = _capi.LaunchOpts(struct_size=C.sizeof(_capi.LaunchOpts), flags=_capi.LAUNCH_ACCUMULATE if accumulate else 0,
                                        workspace=ws.data_ptr() if ws is not None else None, workspace_bytes=ws_bytes, bias=None)
            fn, dx_dtype = ((L.h2gcn_spmm_hops_T_bf16, (_capi.DTYPE_BF16 if out_dtype == torch.bfloat16 else _capi.DTYPE_F32,))
                            if bf16 else (L.h2gcn_spmm_hops_T_opts_f32, ()))
            st = fn(self._handle, mask, C.c_void_p(grad.data_ptr()), ld_row, ld_hop, d, *dx_dtype,
                    C.c_void_p(dx.data_ptr()), dx.stride(0) if self.n_cols > 1 else d,
                    C.byref(opts) if opts is not None else None, C.c_void_p(stream))
        _capi.check(st)
        return dx

    def sddmm(self, grad: torch.Tensor, x: torch.Tensor, hops=None, out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """Gradient wrt the stored values: ``dvals[s][e] = sum_c grad[i, s, c] * x[j, c]`` for every stored entry ``e = (i, j)``
        of selected hop ``s`` -> one contiguous float32 ``[nnz_k]`` tensor per selected hop, in the entry order of
        ``colidx[k]`` (``h2gcn_sddmm_hops_*``).  The pattern decides: the plan's current values are not read, and no
        transposed operand is needed.

        ``grad`` ``[n_rows, H_sel, d]`` and ``x`` ``[n_cols, d]`` are both float32 or both bfloat16 (widened exactly; fp32
        arithmetic and result, bit-identical to the launch on ``.float()`` operands).  Views with a row / hop stride pass
        through (a slot of a concat buffer); a non-unit last stride is made contiguous.  ``out``: a list of ``H_sel``
        contiguous float32 ``[nnz_k]`` tensors to overwrite."""
        h_sel = self.n_selected(hops)
        _require(grad.dim() == 3 and grad.shape[0] == self.n_rows and grad.shape[1] == h_sel,
                 f"grad must be [{self.n_rows}, {h_sel}, d], got {tuple(grad.shape)}")
        d = int(grad.shape[2])
        _require(d >= 1, "grad needs at least one column")
        _require(x.dim() == 2 and tuple(x.shape) == (self.n_cols, d), f"x must be [{self.n_cols}, {d}], got {tuple(x.shape)}")
        _require(grad.dtype in (torch.float32, torch.bfloat16), f"grad must be float32 or bfloat16, got {grad.dtype}")
        _require(x.dtype == grad.dtype, f"grad and x must have the same dtype (both float32 or both bfloat16), got {grad.dtype} and {x.dtype}")
        _require(grad.device == self.device and x.device == self.device, f"grad on {grad.device}, x on {x.device}, plan on {self.device}")
        bf16 = grad.dtype == torch.bfloat16
        if grad.stride(2) != 1 or grad.stride(0) < d or (h_sel > 1 and grad.stride(1) < d):
            grad = grad.contiguous()  # e.g. an expanded (stride-0) gradient coming out of a reduction
        if x.stride(1) != 1 or x.stride(0) < d:
            x = x.contiguous()
        mask, sel = self._mask(hops), self._selected(hops)
        out = self._segment_outputs("values gradient", out, sel)
        ld_row, ld_hop = (grad.stride(0) if self.n_rows > 1 else h_sel * d), (grad.stride(1) if h_sel > 1 else d)
        ldx = x.stride(0) if self.n_cols > 1 else d
        if bf16:
            _bf16_layout("grad", grad, d, (ld_row, ld_hop))
            _bf16_layout("x", x, d, (ldx,))
        _require(_capi.has("h2gcn_sddmm_hops_f32"), f"{_capi.library_path()} predates the values gradient (h2gcn_sddmm_hops_*)")
        L = _capi.lib()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            fn = L.h2gcn_sddmm_hops_bf16 if bf16 else L.h2gcn_sddmm_hops_f32
            st = fn(self._handle, mask, C.c_void_p(grad.data_ptr()), ld_row, ld_hop, C.c_void_p(x.data_ptr()), ldx, d,
                    *self._segment_ptrs(out), C.c_void_p(stream))
        _capi.check(st)
        return out

    @staticmethod
    def _head_width(d: int, n_heads: int) -> None:
        """``K`` heads share ``d`` columns evenly, and a lane's four columns lie in one head."""
        _require(d % n_heads == 0, f"the width d = {d} is not a multiple of the number of heads K = {n_heads}")
        _require(n_heads == 1 or (d // n_heads) % 4 == 0,
                 f"with K = {n_heads} > 1 heads the head width d / K = {d // n_heads} must be a multiple of 4")

    def _launch_values(self, values, sel, d: int):
        """The ``values`` of :meth:`spmm_values` / :meth:`spmm_values_t`, checked -> ``(tensors, K, pointer table, ldv_entry,
        ldv_head)``.  Strides pass through as they are: nothing is made contiguous."""
        _require(not isinstance(values, torch.Tensor) and values is not None,
                 f"values must be a sequence of {len(sel)} tensors (one per selected hop)")
        values = list(values)
        _require(len(values) == len(sel), f"values must list {len(sel)} tensors (one per selected hop), got {len(values)}")
        n_heads = None
        for s, k in enumerate(sel):
            t, nnz = values[s], self.colidx[k].numel()
            _require(isinstance(t, torch.Tensor), f"values[{s}] must be a tensor, got {type(t).__name__}")
            _require(t.dtype == torch.float32, f"values[{s}] must be float32 (the launch is fp32 only), got {t.dtype}")
            _require(t.device == self.device, f"values[{s}] on {t.device}, plan on {self.device}")
            _require(t.dim() in (1, 2) and t.shape[0] == nnz and (t.dim() == 1 or t.shape[1] >= 1),
                     f"values[{s}] must have shape [{nnz}] or [{nnz}, K] (one value per stored entry of hop {k} and head), got {tuple(t.shape)}")
            heads = 1 if t.dim() == 1 else int(t.shape[1])
            _require(n_heads in (None, heads), f"values[{s}] has {heads} heads, values[0] has {n_heads}: every hop needs the same K")
            n_heads = heads
        self._head_width(d, n_heads)
        ptrs = (C.c_void_p * len(sel))(*[t.data_ptr() if t.numel() else None for t in values])
        ldv_entry = (C.c_int64 * len(sel))(*[t.stride(0) if t.shape[0] > 1 else 1 for t in values])
        ldv_head = (C.c_int64 * len(sel))(*[t.stride(1) if t.dim() == 2 and t.shape[1] > 1 else 0 for t in values])
        return values, n_heads, ptrs, ldv_entry, ldv_head

    @staticmethod
    def _values_symbols() -> None:
        if not _capi.has("h2gcn_spmm_hops_values_f32"):
            raise RuntimeError(f"{_capi.library_path()} predates the launches on per-launch values "
                               "(h2gcn_spmm_hops_values_f32 / h2gcn_spmm_hops_T_values_f32): rebuild it")

    @staticmethod
    def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
        """Do the memory extents of two tensors intersect?"""
        def extent(t):
            if t.numel() == 0:
                return 0, 0
            return t.data_ptr(), t.data_ptr() + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()
        (a0, a1), (b0, b1) = extent(a), extent(b)
        return a0 < b1 and b0 < a1

    def _dense_inputs(self, x, what: str) -> int:
        """The gathered operand ``x`` of :meth:`spmm_values` / :meth:`attention_heads`, checked -> its width ``d``."""
        _require(isinstance(x, torch.Tensor) and x.dim() == 2, f"inputs must be [n_cols, d], got shape {tuple(getattr(x, 'shape', ()))}")
        _require(x.dtype == torch.float32, f"inputs must be float32 (the {what} is fp32 only), got {x.dtype}")
        _require(x.device == self.device, f"inputs on {x.device}, plan on {self.device}")
        _require(x.shape[0] == self.n_cols, f"inputs have {x.shape[0]} rows, hop matrices have {self.n_cols} columns")
        _require(x.shape[1] >= 1, "inputs need at least one column")
        return int(x.shape[1])

    def _dense_output(self, out, h_sel: int, d: int) -> None:
        """The caller's ``out`` of the same two calls: float32 ``[n_rows, h_sel, d]`` whose rows and hop slots do not overlap."""
        _require(isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == self.device,
                 "out must be float32 on the plan's device")
        _require(tuple(out.shape) == (self.n_rows, h_sel, d), f"out has shape {tuple(out.shape)}, expected {(self.n_rows, h_sel, d)}")
        _require(d == 1 or out.stride(2) == 1, "out's last dimension must be contiguous")
        _require((self.n_rows <= 1 or out.stride(0) >= d) and (h_sel == 1 or out.stride(1) >= d), "out's rows / hop slots overlap")

    def spmm_values(self, x: torch.Tensor, values: Sequence[torch.Tensor], hops=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The hop SpMM on values that are an argument of the launch: ``out[i, s, c] = sum_e values[s][e, h(c)] * x[j_e, c]`` over
        the stored entries ``e = (i, j_e)`` of selected hop ``s``, ``h(c) = c // (d // K)`` -> ``[n_rows, H_sel, d]``
        (``h2gcn_spmm_hops_values_f32``, one launch).  The plan gives the pattern only: its stored values are not read and nothing
        in it changes, so launches with different values can share one plan.  The bits are those of :meth:`spmm` on a plan
        holding these values (per head: on that head's column slice).

        ``values``: ``H_sel`` float32 tensors on the plan's device, one per SELECTED hop (what ``hop_softmax`` returns), each
        ``[nnz_k]`` or ``[nnz_k, K]`` with one ``K`` for all; any strides pass through (``[K, nnz_k].t()`` is legal, nothing is
        copied).  ``K > 1`` needs ``d % K == 0`` and ``(d // K) % 4 == 0``.  ``x``: float32 ``[n_cols, d]`` (a row stride passes
        through); ``out``: float32 ``[n_rows, H_sel, d]`` with a contiguous last dimension (a view into a wider buffer is
        fine) that does not overlap ``x``.  fp32 only; no transposed operand is needed."""
        d = self._dense_inputs(x, "launch on per-launch values")
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        values, n_heads, ptrs, ldv_entry, ldv_head = self._launch_values(values, sel, d)
        if (d > 1 and x.stride(1) != 1) or (self.n_cols > 1 and x.stride(0) < d):
            x = x.contiguous()
        if out is None:
            out = torch.empty((self.n_rows, h_sel, d), dtype=torch.float32, device=self.device)
        else:
            self._dense_output(out, h_sel, d)
            _require(not self._overlap(out, x), "out overlaps the inputs: the launch gathers rows of x while it stores rows of out")
        self._values_symbols()
        if self.n_rows == 0:
            return out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_spmm_hops_values_f32(
                self._handle, mask, ptrs, ldv_entry, ldv_head, n_heads, C.c_void_p(x.data_ptr()), x.stride(0) if self.n_cols > 1 else d, d,
                C.c_void_p(out.data_ptr()), out.stride(0) if self.n_rows > 1 else h_sel * d, out.stride(1) if h_sel > 1 else d,
                C.c_void_p(stream))
        _capi.check(st)
        return out

    def spmm_values_t(self, grad: torch.Tensor, values: Sequence[torch.Tensor], hops=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The adjoint of :meth:`spmm_values`: ``dx[j, c] = sum_s sum_i values[s][e(i, j), h(c)] * grad[i, s, c]`` -> ``[n_cols, d]``
        (``h2gcn_spmm_hops_T_values_f32``, one launch).  ``values`` as in :meth:`spmm_values`, in FORWARD entry order: the launch
        walks the plan's transposed pattern and reads them through its permutation, so the plan must have been built with
        ``build_transpose=True, keep_permutation=True`` (``symmetric_pattern=True`` serves it on the forward arrays).  The plan's
        stored and transposed values are not read.  ``grad``: float32 ``[n_rows, H_sel, d]`` (row / hop strides pass through);
        ``out``: float32 ``[n_cols, d]`` with unit column stride.  The bits are those of :meth:`spmm_t` on a plan holding these
        values."""
        _require(self.has_transpose, "plan was built without build_transpose=True; backward is unavailable")
        _require(self.keep_permutation, "spmm_values_t reads the values through the permutation of the plan's transposed operands: "
                 "build the plan with HopPlan(..., build_transpose=True, keep_permutation=True)")
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        _require(isinstance(grad, torch.Tensor) and grad.dim() == 3 and grad.shape[0] == self.n_rows and grad.shape[1] == h_sel,
                 f"grad must be [{self.n_rows}, {h_sel}, d], got {tuple(getattr(grad, 'shape', ()))}")
        _require(grad.dtype == torch.float32, f"grad must be float32 (the launch on per-launch values is fp32 only), got {grad.dtype}")
        _require(grad.device == self.device, f"grad on {grad.device}, plan on {self.device}")
        d = int(grad.shape[2])
        _require(d >= 1, "grad needs at least one column")
        values, n_heads, ptrs, ldv_entry, ldv_head = self._launch_values(values, sel, d)
        if (d > 1 and grad.stride(2) != 1) or (self.n_rows > 1 and grad.stride(0) < d) or (h_sel > 1 and grad.stride(1) < d):
            grad = grad.contiguous()  # e.g. an expanded (stride-0) gradient coming out of a reduction
        if out is None:
            out = torch.empty((self.n_cols, d), dtype=torch.float32, device=self.device)
        else:
            _require(isinstance(out, torch.Tensor) and tuple(out.shape) == (self.n_cols, d) and out.dtype == torch.float32
                     and out.device == self.device and (out.stride(1) == 1 or d == 1) and (out.stride(0) >= d or self.n_cols <= 1),
                     f"out must be float32 [{self.n_cols}, {d}] on the plan's device with unit column stride")
            _require(not self._overlap(out, grad), "out overlaps grad: the launch gathers rows of grad while it stores rows of out")
        self._values_symbols()
        if self.n_cols == 0:
            return out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_spmm_hops_T_values_f32(
                self._handle, mask, ptrs, ldv_entry, ldv_head, n_heads, C.c_void_p(grad.data_ptr()),
                grad.stride(0) if self.n_rows > 1 else h_sel * d, grad.stride(1) if h_sel > 1 else d, d,
                C.c_void_p(out.data_ptr()), out.stride(0) if self.n_cols > 1 else d, C.c_void_p(stream))
        _capi.check(st)
        return out

    def _segment_tensors(self, op: str, name: str, tensors, sel, heads: Optional[int] = None) -> tuple:
        """``tensors`` as a list of one contiguous float32 tensor per selected hop -> ``(list, K)``; ``op`` names the operation.
        ``heads`` None: ``[nnz_k]`` tensors; 0: entry-major ``[nnz_k, K]`` tensors, one ``K`` for all; ``K > 0``: that ``K``."""
        _require(not isinstance(tensors, torch.Tensor) and tensors is not None, f"{name} must be a sequence of {len(sel)} tensors (one per selected hop)")
        tensors = list(tensors)
        _require(len(tensors) == len(sel), f"{name} must list {len(sel)} tensors (one per selected hop), got {len(tensors)}")
        for s, k in enumerate(sel):
            t, nnz = tensors[s], self.colidx[k].numel()
            _require(isinstance(t, torch.Tensor), f"{name}[{s}] must be a tensor, got {type(t).__name__}")
            _require(t.dtype == torch.float32, f"{name}[{s}] must be float32 (the {op} is fp32 only), got {t.dtype}")
            _require(t.device == self.device, f"{name}[{s}] on {t.device}, plan on {self.device}")
            if heads is None:
                _require(tuple(t.shape) == (nnz,), f"{name}[{s}] must have shape [{nnz}] (one value per stored entry of hop {k}), got {tuple(t.shape)}")
                _require(t.is_contiguous(), f"{name}[{s}] must be contiguous")
                continue
            _require(t.dim() == 2 and t.shape[0] == nnz and t.shape[1] >= 1,
                     f"{name}[{s}] must have shape [{nnz}, K] (one value per stored entry of hop {k} and head), got {tuple(t.shape)}")
            _require(heads in (0, int(t.shape[1])),
                     f"{name}[{s}] has {int(t.shape[1])} heads where {heads} are expected: every per-entry array needs the same K")
            heads = int(t.shape[1])
            _require(t.is_contiguous(), f"{name}[{s}] must be contiguous (entry-major: element (e, h) at e * K + h)")
        return tensors, heads

    def _segment_outputs(self, op: str, out, sel, heads: Optional[int] = None) -> list:
        """The caller's ``out`` list, checked, or new tensors (``heads`` as in :meth:`_segment_tensors`, but not 0)."""
        if out is not None:
            return self._segment_tensors(op, "out", out, sel, heads)[0]
        return [torch.empty((self.colidx[k].numel(),) + (() if heads is None else (heads,)), dtype=torch.float32, device=self.device)
                for k in sel]

    @staticmethod
    def _segment_ptrs(*tables) -> list:
        """Per table the C ABI's array of one device pointer per selected hop (NULL for a hop without entries)."""
        arr_t = C.c_void_p * len(tables[0])
        return [arr_t(*[t.data_ptr() if t.numel() else None for t in ts]) for ts in tables]

    def _row_softmax_launch(self, symbol: str, hops, inputs: dict, out, heads: Optional[int] = None) -> list:
        """The four row-softmax calls; ``heads`` as in :meth:`_segment_tensors` (0: the head-batched symbols, which take ``K``)."""
        mask, sel = self._mask(hops), self._selected(hops)
        tables = []
        for name, ts in inputs.items():
            ts, heads = self._segment_tensors("row softmax", name, ts, sel, heads)
            tables.append(ts)
        out = self._segment_outputs("row softmax", out, sel, heads)
        if heads is not None:
            self._heads_symbols()
        elif not _capi.has(symbol):
            raise RuntimeError(f"{_capi.library_path()} predates the row softmax (h2gcn_row_softmax_hops_f32 / _backward_hops_f32): rebuild it")
        ptrs = self._segment_ptrs(*tables, out)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = getattr(_capi.lib(), symbol)(self._handle, mask, *ptrs, *(() if heads is None else (heads,)), C.c_void_p(stream))
        _capi.check(st)
        return out

    def row_softmax(self, scores: Sequence[torch.Tensor], hops=None, out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """Softmax over every (row, hop) segment of the pattern: ``alpha[s][e] = exp(scores[s][e] - m) / S`` with ``m`` / ``S`` the
        maximum / the sum of exponentials over the entries of ``e``'s row in selected hop ``s`` -> one contiguous float32
        ``[nnz_k]`` tensor per selected hop, in the entry order of ``colidx[k]`` (``h2gcn_row_softmax_hops_f32``: one launch for
        all selected hops, one softmax per hop and row -- not a joint one across hops).

        ``scores``: a sequence of ``H_sel`` contiguous float32 CUDA tensors ``[nnz_k]``.  ``out``: the tensors to overwrite; it
        may be the ``scores`` tensors themselves.  The bits are a function of each segment's own scores (``include/h2gcn_hip.h``);
        non-finite scores behave as in ``torch.softmax`` on the segment."""
        return self._row_softmax_launch("h2gcn_row_softmax_hops_f32", hops, {"scores": scores}, out)

    def row_softmax_backward(self, alpha: Sequence[torch.Tensor], grad: Sequence[torch.Tensor], hops=None,
                             out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """The backward of :meth:`row_softmax`: ``dscores[s][e] = alpha[s][e] * (grad[s][e] - D)`` with ``D`` the sum of
        ``alpha * grad`` over the entries of ``e``'s row in hop ``s`` (``h2gcn_row_softmax_backward_hops_f32``, one launch).
        ``alpha`` (the forward's result) and ``grad`` as ``scores`` above; ``out`` may be the ``grad`` tensors themselves."""
        return self._row_softmax_launch("h2gcn_row_softmax_backward_hops_f32", hops, {"alpha": alpha, "grad": grad}, out)

    def _node_operand(self, name: str, t, n: int, h_sel: int):
        """``t`` as the C ABI takes a per-node operand of the edge scores: float32 ``[n, h_sel]`` with unit column stride (a row
        stride passes through; 1-D when ``h_sel == 1``) -> ``(tensor, row stride in elements)``."""
        _require(isinstance(t, torch.Tensor), f"{name} must be a tensor, got {type(t).__name__}")
        _require(t.dtype == torch.float32, f"{name} must be float32 (the edge scores are fp32 only), got {t.dtype}")
        _require(t.device == self.device, f"{name} on {t.device}, plan on {self.device}")
        if t.dim() == 1 and h_sel == 1:
            t = t.unsqueeze(1)
        _require(t.dim() == 2 and tuple(t.shape) == (n, h_sel),
                 f"{name} must have shape [{n}, {h_sel}] (one column per selected hop{'; or [' + str(n) + ']' if h_sel == 1 else ''}), got {tuple(t.shape)}")
        if (h_sel > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < h_sel):
            t = t.contiguous()
        return t, (t.stride(0) if n > 1 else h_sel)

    def _column_side(self, need_dr: bool) -> None:
        """What ``dr`` of the edge-score backwards needs of the plan."""
        _require(not need_dr or (self.has_transpose and self.keep_permutation),
                 "the gradient wrt r sums over the COLUMNS of the hop matrices: it walks the plan's transposed operands through their "
                 "permutation.  Build the plan with HopPlan(..., build_transpose=True, keep_permutation=True)"
                 + ("" if self.has_transpose else " (this plan has no transposed operands)"))

    @staticmethod
    def _edge_scores_symbols() -> None:
        if not _capi.has("h2gcn_edge_scores_hops_f32"):
            raise RuntimeError(f"{_capi.library_path()} predates the edge scores (h2gcn_edge_scores_hops_f32 / _backward_hops_f32): rebuild it")

    def edge_scores(self, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                    out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """Additive (GAT-style) attention scores on the pattern: ``score[s][e] = leaky_relu(l[i, s] + r[j, s], negative_slope)`` for
        every stored entry ``e = (i, j)`` of selected hop ``s`` -> one contiguous float32 ``[nnz_k]`` tensor per selected hop, in
        the entry order of ``colidx[k]`` (``h2gcn_edge_scores_hops_f32``: one launch, no row-of-entry index) -- what
        :meth:`row_softmax` takes.  The bits are those of ``torch.nn.functional.leaky_relu(l[row, s] + r[col, s], slope)``.

        ``l`` ``[n_rows, H_sel]`` and ``r`` ``[n_cols, H_sel]``: float32 on the plan's device (1-D when ``H_sel == 1``); a row
        stride passes through (column slices of a wider tensor), a non-unit column stride is made contiguous.  ``out``: a list of
        ``H_sel`` contiguous float32 ``[nnz_k]`` tensors to overwrite.  Only the forward pattern is read: no transposed operand
        is needed."""
        mask, sel = self._mask(hops), self._selected(hops)
        l, ldl = self._node_operand("l", l, self.n_rows, len(sel))
        r, ldr = self._node_operand("r", r, self.n_cols, len(sel))
        out = self._segment_outputs("edge scores", out, sel)
        self._edge_scores_symbols()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_hops_f32(self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr,
                                                        float(negative_slope), *self._segment_ptrs(out), C.c_void_p(stream))
        _capi.check(st)
        return out

    def edge_scores_backward(self, l: torch.Tensor, r: torch.Tensor, grad: Sequence[torch.Tensor], negative_slope: float = 0.2,
                             hops=None, need_dl: bool = True, need_dr: bool = True) -> tuple:
        """The backward of :meth:`edge_scores` -> ``(dl, dr)``: with ``t[e] = grad[s][e]`` where ``l[i, s] + r[j, s] > 0`` and
        ``grad[s][e] * negative_slope`` elsewhere, ``dl[i, s]`` is the sum of ``t`` over row ``i`` and ``dr[j, s]`` the sum over
        column ``j`` of selected hop ``s`` (``h2gcn_edge_scores_backward_hops_f32``).  No atomics: one fixed summation order per
        row / column (``include/h2gcn_hip.h``), so the bits are reproducible and do not depend on the plan's tunables.  Every
        element is written; a row / column without entries gets ``+0``.

        ``l``, ``r`` as in :meth:`edge_scores`; ``grad``: ``H_sel`` contiguous float32 ``[nnz_k]`` tensors.  ``need_dl`` /
        ``need_dr``: compute only that side (``None`` for the other; both ``False`` is refused).  ``dr`` walks the plan's
        transposed operands through their permutation: the plan must have been built with ``build_transpose=True,
        keep_permutation=True`` (``symmetric_pattern=True`` serves it on the forward arrays); ``dl`` needs neither."""
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        _require(need_dl or need_dr, "need_dl and need_dr are both False: nothing to compute")
        shapes = (l.shape if isinstance(l, torch.Tensor) else None, r.shape if isinstance(r, torch.Tensor) else None)
        l, ldl = self._node_operand("l", l, self.n_rows, h_sel)
        r, ldr = self._node_operand("r", r, self.n_cols, h_sel)
        grad, _ = self._segment_tensors("edge scores", "grad", grad, sel)
        self._column_side(need_dr)
        self._edge_scores_symbols()
        dl = torch.empty((self.n_rows, h_sel), dtype=torch.float32, device=self.device) if need_dl else None
        dr = torch.empty((self.n_cols, h_sel), dtype=torch.float32, device=self.device) if need_dr else None
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_backward_hops_f32(
                self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr, float(negative_slope),
                *self._segment_ptrs(grad), C.c_void_p(dl.data_ptr()) if need_dl else None, h_sel,
                C.c_void_p(dr.data_ptr()) if need_dr else None, h_sel, C.c_void_p(stream))
        _capi.check(st)
        return (dl.view(shapes[0]) if need_dl else None, dr.view(shapes[1]) if need_dr else None)

    # ---- the head dimension of sddmm / row_softmax / edge_scores: entry-major [nnz_k, K] arrays, one launch for all heads
    _HEADS_SYMBOLS = ("h2gcn_sddmm_hops_heads_f32", "h2gcn_row_softmax_hops_heads_f32", "h2gcn_row_softmax_backward_hops_heads_f32",
                      "h2gcn_edge_scores_hops_heads_f32", "h2gcn_edge_scores_backward_hops_heads_f32")

    @classmethod
    def _heads_symbols(cls) -> None:
        if not all(_capi.has(s) for s in cls._HEADS_SYMBOLS):
            raise RuntimeError(f"{_capi.library_path()} predates the head-batched attention calls ({', '.join(cls._HEADS_SYMBOLS)}): rebuild it")

    def sddmm_heads(self, grad: torch.Tensor, x: torch.Tensor, heads: int, hops=None,
                    out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """:meth:`sddmm` for ``K = heads`` heads in one launch: ``dvals[s][e, h] = sum_{c in head h} grad[i, s, c] * x[j, c]``, head
        ``h`` owning columns ``h * d / K ..`` -> one contiguous float32 ``[nnz_k, K]`` tensor per selected hop
        (``h2gcn_sddmm_hops_heads_f32``).  Per head the bits are those of :meth:`sddmm` on the head's column slices.

        ``grad`` ``[n_rows, H_sel, d]`` and ``x`` ``[n_cols, d]``: float32 (bfloat16 is refused); row / hop strides pass through.
        ``heads >= 1`` with ``d % heads == 0`` and, for ``heads > 1``, ``(d // heads) % 4 == 0``.  ``out``: a list of ``H_sel``
        contiguous float32 ``[nnz_k, K]`` tensors to overwrite."""
        h_sel = self.n_selected(hops)
        _require(isinstance(grad, torch.Tensor) and grad.dim() == 3 and grad.shape[0] == self.n_rows and grad.shape[1] == h_sel,
                 f"grad must be [{self.n_rows}, {h_sel}, d], got {tuple(getattr(grad, 'shape', ()))}")
        d = int(grad.shape[2])
        _require(d >= 1, "grad needs at least one column")
        _require(isinstance(x, torch.Tensor) and x.dim() == 2 and tuple(x.shape) == (self.n_cols, d),
                 f"x must be [{self.n_cols}, {d}], got {tuple(getattr(x, 'shape', ()))}")
        _require(grad.dtype == torch.float32 and x.dtype == torch.float32,
                 f"grad and x must be float32 (the values gradient with heads is fp32 only), got {grad.dtype} and {x.dtype}")
        _require(grad.device == self.device and x.device == self.device, f"grad on {grad.device}, x on {x.device}, plan on {self.device}")
        n_heads = int(heads)
        _require(n_heads >= 1, f"heads = {heads} < 1")
        self._head_width(d, n_heads)
        if grad.stride(2) != 1 or grad.stride(0) < d or (h_sel > 1 and grad.stride(1) < d):
            grad = grad.contiguous()
        if x.stride(1) != 1 or x.stride(0) < d:
            x = x.contiguous()
        mask, sel = self._mask(hops), self._selected(hops)
        out = self._segment_outputs("values gradient", out, sel, n_heads)
        ld_row, ld_hop = (grad.stride(0) if self.n_rows > 1 else h_sel * d), (grad.stride(1) if h_sel > 1 else d)
        ldx = x.stride(0) if self.n_cols > 1 else d
        self._heads_symbols()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_sddmm_hops_heads_f32(self._handle, mask, C.c_void_p(grad.data_ptr()), ld_row, ld_hop,
                                                        C.c_void_p(x.data_ptr()), ldx, d, n_heads, *self._segment_ptrs(out),
                                                        C.c_void_p(stream))
        _capi.check(st)
        return out

    def row_softmax_heads(self, scores: Sequence[torch.Tensor], hops=None, out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """:meth:`row_softmax` for ``K`` heads in one launch: one softmax per (row, hop, head) over contiguous float32
        ``[nnz_k, K]`` scores -> ``[nnz_k, K]`` coefficients per selected hop (``h2gcn_row_softmax_hops_heads_f32``) -- the layout
        :meth:`spmm_values` reads fastest.  Per head the bits are those of :meth:`row_softmax` on a contiguous copy of that
        column.  ``out`` may be the ``scores`` tensors themselves."""
        return self._row_softmax_launch("h2gcn_row_softmax_hops_heads_f32", hops, {"scores": scores}, out, heads=0)

    def row_softmax_heads_backward(self, alpha: Sequence[torch.Tensor], grad: Sequence[torch.Tensor], hops=None,
                                   out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """The backward of :meth:`row_softmax_heads` (``h2gcn_row_softmax_backward_hops_heads_f32``, one launch): ``alpha`` and
        ``grad`` contiguous float32 ``[nnz_k, K]``; ``out`` may be the ``grad`` tensors themselves."""
        return self._row_softmax_launch("h2gcn_row_softmax_backward_hops_heads_f32", hops, {"alpha": alpha, "grad": grad}, out, heads=0)

    def _node_heads_operand(self, name: str, t, n: int, h_sel: int, n_heads: Optional[int] = None):
        """A per-node operand of the edge scores with heads: float32 ``[n, h_sel, K]`` whose last two dimensions are contiguous (a
        row stride passes through) -> ``(tensor, row stride in elements, K)``."""
        _require(isinstance(t, torch.Tensor), f"{name} must be a tensor, got {type(t).__name__}")
        _require(t.dtype == torch.float32, f"{name} must be float32 (the edge scores are fp32 only), got {t.dtype}")
        _require(t.device == self.device, f"{name} on {t.device}, plan on {self.device}")
        _require(t.dim() == 3 and t.shape[0] == n and t.shape[1] == h_sel and t.shape[2] >= 1 and n_heads in (None, int(t.shape[2])),
                 f"{name} must have shape [{n}, {h_sel}, {'K' if n_heads is None else n_heads}] (node, selected hop, head), got {tuple(t.shape)}")
        k = int(t.shape[2])
        if (k > 1 and t.stride(2) != 1) or (h_sel > 1 and t.stride(1) != k) or (n > 1 and t.stride(0) < h_sel * k):
            t = t.contiguous()
        return t, (t.stride(0) if n > 1 else h_sel * k), k

    def edge_scores_heads(self, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                          out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """:meth:`edge_scores` for ``K`` heads in one launch: ``score[s][e, h] = leaky_relu(l[i, s, h] + r[j, s, h])`` -> one
        contiguous float32 ``[nnz_k, K]`` tensor per selected hop (``h2gcn_edge_scores_hops_heads_f32``).  ``l`` ``[n_rows, H_sel,
        K]``, ``r`` ``[n_cols, H_sel, K]``: float32; a row stride passes through.  Per head the bits are those of
        :meth:`edge_scores` on ``l[:, :, h]``, ``r[:, :, h]``."""
        mask, sel = self._mask(hops), self._selected(hops)
        l, ldl, n_heads = self._node_heads_operand("l", l, self.n_rows, len(sel))
        r, ldr, _ = self._node_heads_operand("r", r, self.n_cols, len(sel), n_heads)
        out = self._segment_outputs("edge scores", out, sel, n_heads)
        self._heads_symbols()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_hops_heads_f32(self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()),
                                                              ldr, n_heads, float(negative_slope), *self._segment_ptrs(out),
                                                              C.c_void_p(stream))
        _capi.check(st)
        return out

    def edge_scores_heads_backward(self, l: torch.Tensor, r: torch.Tensor, grad: Sequence[torch.Tensor], negative_slope: float = 0.2,
                                   hops=None, need_dl: bool = True, need_dr: bool = True) -> tuple:
        """The backward of :meth:`edge_scores_heads` -> ``(dl, dr)``, ``[n_rows, H_sel, K]`` and ``[n_cols, H_sel, K]``
        (``h2gcn_edge_scores_backward_hops_heads_f32``): per head the row / column sums of :meth:`edge_scores_backward`, the same
        bits.  ``grad``: ``H_sel`` contiguous float32 ``[nnz_k, K]`` tensors.  ``need_dl`` / ``need_dr`` and the plan requirements
        of the column side as in :meth:`edge_scores_backward`."""
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        _require(need_dl or need_dr, "need_dl and need_dr are both False: nothing to compute")
        l, ldl, n_heads = self._node_heads_operand("l", l, self.n_rows, h_sel)
        r, ldr, _ = self._node_heads_operand("r", r, self.n_cols, h_sel, n_heads)
        grad, _ = self._segment_tensors("edge scores", "grad", grad, sel, n_heads)
        self._column_side(need_dr)
        self._heads_symbols()
        dl = torch.empty((self.n_rows, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dl else None
        dr = torch.empty((self.n_cols, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dr else None
        if all(t is None or t.numel() == 0 for t in (dl, dr)):   # (no node on the requested sides: nothing to write)
            return dl, dr
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_backward_hops_heads_f32(
                self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr, n_heads, float(negative_slope),
                *self._segment_ptrs(grad), C.c_void_p(dl.data_ptr()) if need_dl else None, h_sel * n_heads,
                C.c_void_p(dr.data_ptr()) if need_dr else None, h_sel * n_heads, C.c_void_p(stream))
        _capi.check(st)
        return dl, dr

    # ---- dynamic (GATv2) edge scores: the nonlinearity between the gather and the reduction over a head's columns
    #: the widest ``u`` / ``v`` the dynamic edge scores serve (a node row stays in registers)
    EDGE_SCORES_DYNAMIC_MAX_WIDTH = 256
    _DYNAMIC_SYMBOLS = ("h2gcn_edge_scores_dynamic_workspace_bytes", "h2gcn_edge_scores_dynamic_hops_f32",
                        "h2gcn_edge_scores_dynamic_backward_hops_f32")

    @classmethod
    def _dynamic_symbols(cls) -> None:
        if not all(_capi.has(s) for s in cls._DYNAMIC_SYMBOLS):
            raise RuntimeError(f"{_capi.library_path()} predates the dynamic edge scores ({', '.join(cls._DYNAMIC_SYMBOLS)}): rebuild it")

    def _dynamic_operands(self, u, v, a, heads, h_sel: int):
        """``u`` ``[n_rows, d]``, ``v`` ``[n_cols, d]`` and ``a`` ``[H_sel, d]`` (or ``[H_sel, K, d / K]``) of the dynamic edge scores,
        checked -> ``(u, ldu, v, ldv, a, lda, d, K)``.  Row strides pass through; a non-unit column stride is made contiguous."""
        for name, t in (("u", u), ("v", v), ("a", a)):
            _require(isinstance(t, torch.Tensor), f"{name} must be a tensor, got {type(t).__name__}")
            _require(t.dtype == torch.float32, f"{name} must be float32 (the dynamic edge scores are fp32 only), got {t.dtype}")
            _require(t.device == self.device, f"{name} on {t.device}, plan on {self.device}")
        _require(u.dim() == 2 and u.shape[0] == self.n_rows and u.shape[1] >= 1, f"u must be [{self.n_rows}, d], got {tuple(u.shape)}")
        d = int(u.shape[1])
        _require(tuple(v.shape) == (self.n_cols, d), f"v must be [{self.n_cols}, {d}], got {tuple(v.shape)}")
        n_heads = int(heads)
        _require(n_heads >= 1, f"heads = {heads} < 1")
        self._head_width(d, n_heads)
        _require(d <= self.EDGE_SCORES_DYNAMIC_MAX_WIDTH,
                 f"the width d = {d} exceeds EDGE_SCORES_DYNAMIC_MAX_WIDTH = {self.EDGE_SCORES_DYNAMIC_MAX_WIDTH} (a node row stays in registers)")
        if a.dim() == 3 and tuple(a.shape) == (h_sel, n_heads, d // n_heads):
            a = a.reshape(h_sel, d)
        _require(tuple(a.shape) == (h_sel, d),
                 f"a must be [{h_sel}, {d}] or [{h_sel}, {n_heads}, {d // n_heads}] (one row per selected hop), got {tuple(a.shape)}")
        out = []
        for t, n in ((u, self.n_rows), (v, self.n_cols), (a, h_sel)):
            if (d > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < d):
                t = t.contiguous()
            out += [t, t.stride(0) if n > 1 else d]
        return (*out, d, n_heads)

    def edge_scores_dynamic(self, u: torch.Tensor, v: torch.Tensor, a: torch.Tensor, heads: int = 1, negative_slope: float = 0.2,
                            hops=None, out: Optional[Sequence[torch.Tensor]] = None) -> list:
        """Dynamic (GATv2) attention scores on the pattern: ``score[s][e, h] = sum_{c in head h} a[s, c] * leaky_relu(u[i, c] + v[j, c])``
        for every stored entry ``e = (i, j)`` of selected hop ``s`` -> one contiguous float32 ``[nnz_k, K]`` tensor per selected hop
        (``[nnz_k]`` for ``heads == 1``), in the entry order of ``colidx[k]`` (``h2gcn_edge_scores_dynamic_hops_f32``: one launch,
        nothing of size ``nnz x d``).  Unlike :meth:`edge_scores_heads` the ranking of a row's neighbours depends on the row.

        ``u`` ``[n_rows, d]``, ``v`` ``[n_cols, d]``, ``a`` ``[H_sel, d]`` (or ``[H_sel, K, d // K]``): float32; ``d <= 256``,
        ``d % heads == 0`` and, for ``heads > 1``, ``(d // heads) % 4 == 0``.  Row strides pass through.  The bits are a function of
        ``a[s]``, ``u[i]``, ``v[j]``, ``d``, ``K`` and the slope alone (``include/h2gcn_hip.h``).  Only the forward pattern is read."""
        mask, sel = self._mask(hops), self._selected(hops)
        u, ldu, v, ldv, a, lda, d, n_heads = self._dynamic_operands(u, v, a, heads, len(sel))
        out = self._segment_outputs("dynamic edge scores", out, sel, None if n_heads == 1 else n_heads)
        self._dynamic_symbols()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_dynamic_hops_f32(
                self._handle, mask, C.c_void_p(u.data_ptr()), ldu, C.c_void_p(v.data_ptr()), ldv, C.c_void_p(a.data_ptr()), lda, d, n_heads,
                float(negative_slope), *self._segment_ptrs(out), C.c_void_p(stream))
        _capi.check(st)
        return out

    def edge_scores_dynamic_backward(self, u: torch.Tensor, v: torch.Tensor, a: torch.Tensor, grad: Sequence[torch.Tensor], heads: int = 1,
                                     negative_slope: float = 0.2, hops=None, need_du: bool = True, need_dv: bool = True,
                                     need_da: bool = True) -> tuple:
        """The backward of :meth:`edge_scores_dynamic` -> ``(du, dv, da)``, ``[n_rows, d]``, ``[n_cols, d]`` and ``[H_sel, d]``
        (``h2gcn_edge_scores_dynamic_backward_hops_f32``): ``u + v`` and its leaky_relu are recomputed per entry, nothing of size
        ``nnz x d`` is stored.  No float atomics: fixed summation orders (``include/h2gcn_hip.h``), ``du`` / ``dv`` independent of
        ``rows_per_wave`` and of which outputs were asked for.  Every element is written; a node without entries gets ``+0``.

        ``grad``: ``H_sel`` contiguous float32 ``[nnz_k, K]`` tensors (``[nnz_k]`` for one head).  ``need_*``: compute only those
        (``None`` for the others; all ``False`` is refused).  ``dv`` walks the plan's transposed operands through their permutation:
        ``build_transpose=True, keep_permutation=True`` (``symmetric_pattern=True`` serves it on the forward arrays).  The workspace
        of ``da`` is allocated per call."""
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        _require(need_du or need_dv or need_da, "need_du, need_dv and need_da are all False: nothing to compute")
        u, ldu, v, ldv, a, lda, d, n_heads = self._dynamic_operands(u, v, a, heads, h_sel)
        grad, _ = self._segment_tensors("dynamic edge scores", "grad", grad, sel, None if n_heads == 1 else n_heads)
        self._column_side(need_dv)
        self._dynamic_symbols()
        du = torch.empty((self.n_rows, d), dtype=torch.float32, device=self.device) if need_du else None
        dv = torch.empty((self.n_cols, d), dtype=torch.float32, device=self.device) if need_dv else None
        da = torch.empty((h_sel, d), dtype=torch.float32, device=self.device) if need_da else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            ws = None
            if need_da:
                nbytes = int(_capi.lib().h2gcn_edge_scores_dynamic_workspace_bytes(self._handle, mask, d))
                ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_edge_scores_dynamic_backward_hops_f32(
                self._handle, mask, C.c_void_p(u.data_ptr()), ldu, C.c_void_p(v.data_ptr()), ldv, C.c_void_p(a.data_ptr()), lda, d, n_heads,
                float(negative_slope), *self._segment_ptrs(grad), ptr(du), d, ptr(dv), d, ptr(da), d, ptr(ws),
                0 if ws is None else ws.numel(), C.c_void_p(stream))
        _capi.check(st)
        return du, dv, da

    #: the largest K the fused attention forward serves (``h2gcn_attention_hops_heads_f32``); beyond it the chain is the way
    ATTENTION_FUSED_MAX_HEADS = 16

    def attention_heads(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The attention forward in ONE launch: ``out[i, s, c] = sum_e alpha_s[e, h(c)] * x[j_e, c]`` with ``alpha_s[:, h]`` the
        softmax over row ``i`` of ``leaky_relu(l[i, s, h] + r[j, s, h], negative_slope)`` -> ``[n_rows, H_sel, d]``
        (``h2gcn_attention_hops_heads_f32``).  The bits are those of :meth:`edge_scores_heads` -> :meth:`row_softmax_heads` ->
        :meth:`spmm_values` on the same operands, but no ``[nnz_k, K]`` array exists: the launch allocates nothing and writes only
        ``out``.  Forward only (no gradient flows through it); only the forward pattern is read, the plan's values are not.

        ``l`` ``[n_rows, H_sel, K]``, ``r`` ``[n_cols, H_sel, K]``, ``x`` ``[n_cols, d]``: float32 on the plan's device; row strides
        pass through.  ``1 <= K <= 16``; ``K > 1`` needs ``d % K == 0`` and ``(d // K) % 4 == 0``.  ``out``: float32 ``[n_rows,
        H_sel, d]`` with a contiguous last dimension (a view into a wider buffer is fine: its strides pass through) that overlaps
        none of the inputs."""
        d = self._dense_inputs(x, "fused attention forward")
        mask, sel = self._mask(hops), self._selected(hops)
        h_sel = len(sel)
        l, ldl, n_heads = self._node_heads_operand("l", l, self.n_rows, h_sel)
        r, ldr, _ = self._node_heads_operand("r", r, self.n_cols, h_sel, n_heads)
        _require(n_heads <= self.ATTENTION_FUSED_MAX_HEADS,
                 f"the fused attention forward serves at most K = {self.ATTENTION_FUSED_MAX_HEADS} heads, got K = {n_heads}: run the chain "
                 "(edge_scores_heads, row_softmax_heads, spmm_values)")
        self._head_width(d, n_heads)
        if (d > 1 and x.stride(1) != 1) or (self.n_cols > 1 and x.stride(0) < d):
            x = x.contiguous()
        if out is not None:
            self._dense_output(out, h_sel, d)
            for name, t in (("the inputs", x), ("l", l), ("r", r)):
                _require(not self._overlap(out, t), f"out overlaps {name}: the launch gathers rows of x and r while it stores rows of out")
        if not _capi.has("h2gcn_attention_hops_heads_f32"):
            raise RuntimeError(f"{_capi.library_path()} predates the fused attention forward (h2gcn_attention_hops_heads_f32): rebuild it")
        if out is None:
            out = torch.empty((self.n_rows, h_sel, d), dtype=torch.float32, device=self.device)
        if self.n_rows == 0:
            return out
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_attention_hops_heads_f32(
                self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr, n_heads, float(negative_slope),
                C.c_void_p(x.data_ptr()), x.stride(0) if self.n_cols > 1 else d, d, C.c_void_p(out.data_ptr()),
                out.stride(0) if self.n_rows > 1 else h_sel * d, out.stride(1) if h_sel > 1 else d, C.c_void_p(stream))
        _capi.check(st)
        return out

    #: the widest ``d`` the recomputing attention backward serves (``h2gcn_attention_hops_heads_backward_f32``)
    ATTENTION_RECOMPUTE_MAX_WIDTH = 256
    _RECOMPUTE_SYMBOLS = ("h2gcn_attention_hops_heads_stats_f32", "h2gcn_attention_hops_heads_backward_f32")

    def _attention_operands(self, what: str, x, l, r, hops):
        """``x``, ``l``, ``r`` of the attention launches, checked as :meth:`attention_heads` checks them -> ``(x, l, ldl, r, ldr, K, d,
        mask, H_sel)``."""
        d = self._dense_inputs(x, what)
        mask, h_sel = self._mask(hops), len(self._selected(hops))
        l, ldl, n_heads = self._node_heads_operand("l", l, self.n_rows, h_sel)
        r, ldr, _ = self._node_heads_operand("r", r, self.n_cols, h_sel, n_heads)
        _require(n_heads <= self.ATTENTION_FUSED_MAX_HEADS,
                 f"the {what} serves at most K = {self.ATTENTION_FUSED_MAX_HEADS} heads, got K = {n_heads}: run the chain "
                 "(edge_scores_heads, row_softmax_heads, spmm_values)")
        self._head_width(d, n_heads)
        if (d > 1 and x.stride(1) != 1) or (self.n_cols > 1 and x.stride(0) < d):
            x = x.contiguous()
        return x, l, ldl, r, ldr, n_heads, d, mask, h_sel

    @classmethod
    def _recompute_symbol(cls, name: str) -> None:
        if not _capi.has(name):
            raise RuntimeError(f"{_capi.library_path()} predates the recomputing attention backward ({name}): rebuild it")

    _DROPOUT_SYMBOLS = ("h2gcn_attention_hops_heads_stats_dropout_f32", "h2gcn_attention_hops_heads_backward_dropout_f32",
                        "h2gcn_attention_dropout_factors_hops_f32")

    def _mask_args(self, keep_prob, seed, step, symbol: str):
        """``keep_prob``, ``seed``, ``step`` of an attention-dropout launch, checked -> the C ABI's ``(keep_prob, seed, step_dev)``, or
        ``None`` for ``keep_prob == 1`` (today's call, argument for argument)."""
        keep_prob = float(keep_prob)
        _require(0.0 < keep_prob <= 1.0, f"keep_prob = {keep_prob} outside (0, 1]")
        if keep_prob == 1.0:
            return None
        if step is not None:
            _require(isinstance(step, torch.Tensor) and step.dtype == torch.int64 and step.numel() == 1 and step.device == self.device,
                     f"step must be a 1-element int64 tensor on {self.device} (the device counter the kernels read), or None for step 0")
        if not _capi.has(symbol):
            raise RuntimeError(f"{_capi.library_path()} predates the attention dropout ({symbol}): rebuild it")
        return (C.c_float(keep_prob), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_void_p(step.data_ptr()) if step is not None else None)

    def attention_dropout_factors(self, n_heads: int, keep_prob: float, seed: int, step: Optional[torch.Tensor] = None, hops=None) -> list:
        """The dropout factors of the attention coefficients, per selected hop float32 ``[nnz_k, n_heads]`` with elements in
        ``{0, 1 / keep_prob}`` (``h2gcn_attention_dropout_factors_hops_f32``): the mask :meth:`attention_heads_stats_dropout` and
        :meth:`attention_heads_backward_dropout` draw inside their kernels for the same ``(keep_prob, seed, step)``, a function of the
        entry's hop, row, column and head alone (include/h2gcn_hip.h).  For a chain that multiplies its ``alpha`` by them, and for
        tests; ``1 <= n_heads <= 16``.  ``step``: a 1-element int64 tensor on the plan's device, or ``None`` for step 0."""
        n_heads = int(n_heads)
        _require(1 <= n_heads <= self.ATTENTION_FUSED_MAX_HEADS, f"n_heads = {n_heads} outside 1..{self.ATTENTION_FUSED_MAX_HEADS}")
        mask, sel = self._mask(hops), self._selected(hops)
        keep_prob = float(keep_prob)
        margs = self._mask_args(keep_prob, seed, step, self._DROPOUT_SYMBOLS[2])
        nnz = self.nnz
        if margs is None:
            return [torch.ones((nnz[k], n_heads), dtype=torch.float32, device=self.device) for k in sel]
        out = [torch.empty((nnz[k], n_heads), dtype=torch.float32, device=self.device) for k in sel]
        ld = (C.c_int64 * len(sel))(*[n_heads] * len(sel))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_attention_dropout_factors_hops_f32(self._handle, mask, n_heads, *margs, *self._segment_ptrs(out), ld,
                                                                      C.c_void_p(stream))
        _capi.check(st)
        return out

    def attention_heads_stats(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                              out: Optional[torch.Tensor] = None) -> tuple:
        """:meth:`attention_heads` that also returns the softmax statistics -> ``(y, stats)``
        (``h2gcn_attention_hops_heads_stats_f32``, one launch).  ``y`` has the bits of :meth:`attention_heads`; ``stats`` is float32
        ``[n_rows, H_sel, 2, K]``: ``stats[i, s, 0, h]`` the maximum score of the segment, ``stats[i, s, 1, h]`` the reciprocal of
        its sum of exponentials -- ``(+0, +0)`` for an empty segment.  With ``x, l, r, stats, y`` :meth:`attention_heads_backward`
        computes the gradients without any ``[nnz_k, K]`` array.  Operands and ``out`` as in :meth:`attention_heads`."""
        return self._attention_heads_stats(x, l, r, negative_slope, hops, out, 1.0, 0, None)

    def attention_heads_stats_dropout(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, keep_prob: float, seed: int,
                                      step: Optional[torch.Tensor] = None, negative_slope: float = 0.2, hops=None,
                                      out: Optional[torch.Tensor] = None) -> tuple:
        """:meth:`attention_heads_stats` with dropout on the coefficients, the mask drawn inside the kernel from ``(seed, step)``
        (``h2gcn_attention_hops_heads_stats_dropout_f32``; :meth:`attention_dropout_factors` returns the factors) -> ``(y, stats)``:
        ``y`` has the bits of ``spmm_values(x, [alpha_k * f_k])``, ``stats`` are those without dropout.  ``keep_prob`` in ``(0, 1]``
        (1: the launch without dropout); ``step``: a 1-element int64 tensor on the plan's device, read when the kernel runs, or
        ``None`` for step 0.  :meth:`attention_heads_backward_dropout` with the same three computes the gradients."""
        return self._attention_heads_stats(x, l, r, negative_slope, hops, out, keep_prob, seed, step)

    def _attention_heads_stats(self, x, l, r, negative_slope, hops, out, keep_prob, seed, step) -> tuple:
        x, l, ldl, r, ldr, n_heads, d, mask, h_sel = self._attention_operands("fused attention forward", x, l, r, hops)
        margs = self._mask_args(keep_prob, seed, step, self._DROPOUT_SYMBOLS[0])
        if out is not None:
            self._dense_output(out, h_sel, d)
            for name, t in (("the inputs", x), ("l", l), ("r", r)):
                _require(not self._overlap(out, t), f"out overlaps {name}: the launch gathers rows of x and r while it stores rows of out")
        self._recompute_symbol(self._RECOMPUTE_SYMBOLS[0])
        if out is None:
            out = torch.empty((self.n_rows, h_sel, d), dtype=torch.float32, device=self.device)
        stats = torch.empty((self.n_rows, h_sel, 2, n_heads), dtype=torch.float32, device=self.device)
        if self.n_rows == 0:
            return out, stats
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            fn = _capi.lib().h2gcn_attention_hops_heads_stats_f32 if margs is None else _capi.lib().h2gcn_attention_hops_heads_stats_dropout_f32
            st = fn(
                self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr, n_heads, float(negative_slope),
                C.c_void_p(x.data_ptr()), x.stride(0) if self.n_cols > 1 else d, d, C.c_void_p(out.data_ptr()),
                out.stride(0) if self.n_rows > 1 else h_sel * d, out.stride(1) if h_sel > 1 else d, C.c_void_p(stats.data_ptr()),
                h_sel * 2 * n_heads, *(margs or ()), C.c_void_p(stream))
        _capi.check(st)
        return out, stats

    def attention_heads_backward(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, stats: torch.Tensor, y: torch.Tensor,
                                 grad: torch.Tensor, negative_slope: float = 0.2, hops=None, need_dl: bool = True, need_dr: bool = True,
                                 need_dx: bool = True) -> tuple:
        """The backward of :meth:`attention_heads_stats` -> ``(dl, dr, dx)``, ``[n_rows, H_sel, K]``, ``[n_cols, H_sel, K]`` and
        ``[n_cols, d]`` (``h2gcn_attention_hops_heads_backward_f32``): every per-entry quantity is computed again from the node
        operands and ``stats``, so nothing of size ``nnz`` is read, written or allocated -- the launch allocates its results and one
        ``[n_rows, H_sel, K]`` buffer.  ``x``, ``l``, ``r``, ``stats``, ``y`` are the forward's operands and results, ``grad`` the
        gradient of ``y`` (float32 ``[n_rows, H_sel, d]``; row and hop strides pass through).  An unwanted side is ``None``.

        The gradients are deterministic; they are NOT the chain's bits (include/h2gcn_hip.h has the orders).  ``dr`` and ``dx`` walk
        the plan's transposed operands WITHOUT their permutation: ``build_transpose=True`` (or ``symmetric_pattern=True``) is
        enough.  ``d <= 256``."""
        return self._attention_heads_backward(x, l, r, stats, y, grad, negative_slope, hops, need_dl, need_dr, need_dx, 1.0, 0, None)

    def attention_heads_backward_dropout(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, stats: torch.Tensor, y: torch.Tensor,
                                         grad: torch.Tensor, keep_prob: float, seed: int, step: Optional[torch.Tensor] = None,
                                         negative_slope: float = 0.2, hops=None, need_dl: bool = True, need_dr: bool = True,
                                         need_dx: bool = True) -> tuple:
        """The backward of :meth:`attention_heads_stats_dropout` (``h2gcn_attention_hops_heads_backward_dropout_f32``):
        :meth:`attention_heads_backward` whose kernels draw the forward's mask again from the forward's ``(keep_prob, seed, step)``
        -- still nothing of size ``nnz``, and no permutation: the factor is keyed by the entry's row and column."""
        return self._attention_heads_backward(x, l, r, stats, y, grad, negative_slope, hops, need_dl, need_dr, need_dx, keep_prob, seed, step)

    def _attention_heads_backward(self, x, l, r, stats, y, grad, negative_slope, hops, need_dl, need_dr, need_dx, keep_prob, seed, step) -> tuple:
        x, l, ldl, r, ldr, n_heads, d, mask, h_sel = self._attention_operands("recomputing attention backward", x, l, r, hops)
        margs = self._mask_args(keep_prob, seed, step, self._DROPOUT_SYMBOLS[1])
        _require(need_dl or need_dr or need_dx, "need_dl, need_dr and need_dx are all False: nothing to compute")
        _require(d <= self.ATTENTION_RECOMPUTE_MAX_WIDTH,
                 f"the recomputing attention backward serves at most d = {self.ATTENTION_RECOMPUTE_MAX_WIDTH} columns, got d = {d}: run the chain")
        for name, t, shape in (("stats", stats, (self.n_rows, h_sel, 2, n_heads)), ("y", y, (self.n_rows, h_sel, d)),
                               ("grad", grad, (self.n_rows, h_sel, d))):
            _require(isinstance(t, torch.Tensor) and tuple(t.shape) == shape, f"{name} must be {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
            _require(t.dtype == torch.float32, f"{name} must be float32 (the recomputing attention backward is fp32 only), got {t.dtype}")
            _require(t.device == self.device, f"{name} on {t.device}, plan on {self.device}")
        stats = stats.contiguous()
        if (d > 1 and y.stride(2) != 1) or (self.n_rows > 1 and y.stride(0) < d) or (h_sel > 1 and y.stride(1) < d):
            y = y.contiguous()
        if (d > 1 and grad.stride(2) != 1) or (self.n_rows > 1 and grad.stride(0) < d) or (h_sel > 1 and grad.stride(1) < d):
            grad = grad.contiguous()
        _require(not (need_dr or need_dx) or self.has_transpose,
                 "the gradients wrt r and the inputs sum over the COLUMNS of the hop matrices: they walk the plan's transposed operands "
                 "(no permutation is needed).  Build the plan with HopPlan(..., build_transpose=True)")
        self._recompute_symbol(self._RECOMPUTE_SYMBOLS[1])
        dl = torch.empty((self.n_rows, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dl else None
        dr = torch.empty((self.n_cols, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dr else None
        dx = torch.empty((self.n_cols, d), dtype=torch.float32, device=self.device) if need_dx else None
        if all(t is None or t.numel() == 0 for t in (dl, dr, dx)):   # (no node on the requested sides: nothing to write)
            return dl, dr, dx
        delta = torch.empty((self.n_rows, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dr or need_dx else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            fn = (_capi.lib().h2gcn_attention_hops_heads_backward_f32 if margs is None
                  else _capi.lib().h2gcn_attention_hops_heads_backward_dropout_f32)
            st = fn(
                self._handle, mask, ptr(l), ldl, ptr(r), ldr, n_heads, float(negative_slope), ptr(x), x.stride(0) if self.n_cols > 1 else d, d,
                ptr(stats), h_sel * 2 * n_heads, ptr(y), y.stride(0) if self.n_rows > 1 else h_sel * d, y.stride(1) if h_sel > 1 else d,
                ptr(grad), grad.stride(0) if self.n_rows > 1 else h_sel * d, grad.stride(1) if h_sel > 1 else d,
                ptr(delta), h_sel * n_heads, ptr(dl), h_sel * n_heads, ptr(dr), h_sel * n_heads, ptr(dx), d, *(margs or ()), C.c_void_p(stream))
        _capi.check(st)
        return dl, dr, dx

    # ---- the recomputing attention on bf16 embeddings (csrc/attention_bf16.hip): widen exactly, the fp32 kernels' operations in
    # their order, one rounding to nearest even at the store.  l, r, stats and the K-wide gradients stay float32.
    BF16_ATTENTION_SYMBOLS = ("h2gcn_attention_hops_heads_bf16", "h2gcn_attention_hops_heads_stats_bf16",
                              "h2gcn_attention_hops_heads_backward_bf16")

    @classmethod
    def _bf16_attention_symbol(cls, name: str) -> None:
        _require(_capi.has(name), f"{_capi.library_path()} predates the bf16 attention launches ({name}): rebuild it "
                 "(bfloat16 embeddings are never run in float32 instead)")

    def _attention_operands_bf16(self, what: str, x, l, r, hops):
        """``x`` (bfloat16), ``l``, ``r`` (float32) of the bf16 attention launches -> what :meth:`_attention_operands` returns."""
        _require(isinstance(x, torch.Tensor) and x.dim() == 2, f"inputs must be [n_cols, d], got shape {tuple(getattr(x, 'shape', ()))}")
        _require(x.dtype == torch.bfloat16, f"inputs must be bfloat16 (the {what} takes bf16 embeddings), got {x.dtype}")
        _require(x.device == self.device, f"inputs on {x.device}, plan on {self.device}")
        _require(x.shape[0] == self.n_cols, f"inputs have {x.shape[0]} rows, hop matrices have {self.n_cols} columns")
        _require(x.shape[1] >= 1, "inputs need at least one column")
        d = int(x.shape[1])
        mask, h_sel = self._mask(hops), len(self._selected(hops))
        l, ldl, n_heads = self._node_heads_operand("l", l, self.n_rows, h_sel)
        r, ldr, _ = self._node_heads_operand("r", r, self.n_cols, h_sel, n_heads)
        _require(n_heads <= self.ATTENTION_FUSED_MAX_HEADS,
                 f"the {what} serves at most K = {self.ATTENTION_FUSED_MAX_HEADS} heads, got K = {n_heads} (the chain is float32 only)")
        self._head_width(d, n_heads)
        if x.stride(1) != 1 or (self.n_cols > 1 and x.stride(0) < d):
            x = x.contiguous()
        _bf16_layout("inputs", x, d, (x.stride(0),) if self.n_cols > 1 else ())
        return x, l, ldl, r, ldr, n_heads, d, mask, h_sel

    def _dense_output_bf16(self, out, out_dtype, h_sel: int, d: int, inputs):
        """The result dtype (``out.dtype``, else ``out_dtype``, else bfloat16) and the caller's ``out``, checked."""
        if out_dtype is None:
            out_dtype = out.dtype if out is not None else torch.bfloat16
        _require(out_dtype in (torch.float32, torch.bfloat16), f"outputs must be float32 or bfloat16, got {out_dtype}")
        if out is not None:
            _require(isinstance(out, torch.Tensor) and out.dtype == out_dtype and out.device == self.device,
                     f"out must be {out_dtype} on the plan's device")
            _require(tuple(out.shape) == (self.n_rows, h_sel, d), f"out has shape {tuple(out.shape)}, expected {(self.n_rows, h_sel, d)}")
            _require(d == 1 or out.stride(2) == 1, "out's last dimension must be contiguous")
            _require((self.n_rows <= 1 or out.stride(0) >= d) and (h_sel == 1 or out.stride(1) >= d), "out's rows / hop slots overlap")
            if out_dtype == torch.bfloat16:
                _bf16_layout("out", out, d, [out.stride(i) for i, n in ((0, self.n_rows), (1, h_sel)) if n > 1])
            for name, t in inputs:
                _require(not self._overlap(out, t), f"out overlaps {name}: the launch gathers rows of x and r while it stores rows of out")
        return out_dtype

    def attention_heads_bf16(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                             out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """:meth:`attention_heads` on bfloat16 ``x`` (``h2gcn_attention_hops_heads_bf16``): every element of ``x`` is widened
        exactly, the fp32 launch's operations run in fp32 in its order, and the result is rounded once, to nearest even, where it is
        stored.  A float32 result has the bits of ``attention_heads(x.float(), l, r)``, a bfloat16 result is that
        ``.to(torch.bfloat16)``.  ``l``, ``r``: float32.  The result's dtype is ``out.dtype``, else ``out_dtype``, else bfloat16 (as
        in :meth:`spmm`).  ``d`` even; the other limits are :meth:`attention_heads`'s."""
        return self._attention_heads_bf16(False, x, l, r, negative_slope, hops, out, out_dtype)[0]

    def attention_heads_stats_bf16(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, negative_slope: float = 0.2, hops=None,
                                   out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> tuple:
        """:meth:`attention_heads_stats` on bfloat16 ``x`` -> ``(y, stats)`` (``h2gcn_attention_hops_heads_stats_bf16``): ``y`` as
        :meth:`attention_heads_bf16` gives it, ``stats`` float32 with the bits of ``attention_heads_stats(x.float(), l, r)``."""
        return self._attention_heads_bf16(True, x, l, r, negative_slope, hops, out, out_dtype)

    def _attention_heads_bf16(self, with_stats, x, l, r, negative_slope, hops, out, out_dtype) -> tuple:
        x, l, ldl, r, ldr, n_heads, d, mask, h_sel = self._attention_operands_bf16("bf16 fused attention forward", x, l, r, hops)
        out_dtype = self._dense_output_bf16(out, out_dtype, h_sel, d, (("the inputs", x), ("l", l), ("r", r)))
        self._bf16_attention_symbol(self.BF16_ATTENTION_SYMBOLS[1 if with_stats else 0])
        if out is None:
            out = torch.empty((self.n_rows, h_sel, d), dtype=out_dtype, device=self.device)
        stats = torch.empty((self.n_rows, h_sel, 2, n_heads), dtype=torch.float32, device=self.device) if with_stats else None
        if self.n_rows == 0:
            return out, stats
        y_dtype = _capi.DTYPE_BF16 if out_dtype == torch.bfloat16 else _capi.DTYPE_F32
        args = (self._handle, mask, C.c_void_p(l.data_ptr()), ldl, C.c_void_p(r.data_ptr()), ldr, n_heads, float(negative_slope),
                C.c_void_p(x.data_ptr()), x.stride(0) if self.n_cols > 1 else d, d, y_dtype, C.c_void_p(out.data_ptr()),
                out.stride(0) if self.n_rows > 1 else h_sel * d, out.stride(1) if h_sel > 1 else d)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if with_stats:
                st = _capi.lib().h2gcn_attention_hops_heads_stats_bf16(*args, C.c_void_p(stats.data_ptr()), h_sel * 2 * n_heads,
                                                                       C.c_void_p(stream))
            else:
                st = _capi.lib().h2gcn_attention_hops_heads_bf16(*args, C.c_void_p(stream))
        _capi.check(st)
        return out, stats

    def attention_heads_backward_bf16(self, x: torch.Tensor, l: torch.Tensor, r: torch.Tensor, stats: torch.Tensor, y: torch.Tensor,
                                      grad: torch.Tensor, negative_slope: float = 0.2, hops=None, need_dl: bool = True,
                                      need_dr: bool = True, need_dx: bool = True, dx_dtype: Optional[torch.dtype] = None) -> tuple:
        """:meth:`attention_heads_backward` on bfloat16 ``x``, ``y`` and ``grad`` -> ``(dl, dr, dx)``
        (``h2gcn_attention_hops_heads_backward_bf16``).  ``y`` is the bfloat16 result of :meth:`attention_heads_stats_bf16`: ``delta =
        <grad, y>`` is taken on it.  ``dl``, ``dr`` (float32) and a float32 ``dx`` have the bits of ``attention_heads_backward(x.float(),
        l, r, stats, y.float(), grad.float())``; a bfloat16 ``dx`` (``dx_dtype``, the default) is that rounded once, after the sum
        over the hops.  ``d`` even and ``<= 256``."""
        x, l, ldl, r, ldr, n_heads, d, mask, h_sel = self._attention_operands_bf16("bf16 recomputing attention backward", x, l, r, hops)
        _require(need_dl or need_dr or need_dx, "need_dl, need_dr and need_dx are all False: nothing to compute")
        _require(d <= self.ATTENTION_RECOMPUTE_MAX_WIDTH,
                 f"the bf16 recomputing attention backward serves at most d = {self.ATTENTION_RECOMPUTE_MAX_WIDTH} columns, got d = {d} "
                 "(the chain is float32 only)")
        if dx_dtype is None:
            dx_dtype = torch.bfloat16
        _require(dx_dtype in (torch.float32, torch.bfloat16), f"dx must be float32 or bfloat16, got {dx_dtype}")
        for name, t, shape, dtype in (("stats", stats, (self.n_rows, h_sel, 2, n_heads), torch.float32),
                                      ("y", y, (self.n_rows, h_sel, d), torch.bfloat16), ("grad", grad, (self.n_rows, h_sel, d), torch.bfloat16)):
            _require(isinstance(t, torch.Tensor) and tuple(t.shape) == shape, f"{name} must be {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
            _require(t.dtype == dtype, f"{name} must be {str(dtype).replace('torch.', '')} (the bf16 recomputing attention backward), got {t.dtype}")
            _require(t.device == self.device, f"{name} on {t.device}, plan on {self.device}")
        stats = stats.contiguous()

        def wide(t):   # the layout rule of a bf16 [n_rows, H_sel, d] array; anything else is copied
            bad = (t.stride(2) != 1 or (self.n_rows > 1 and (t.stride(0) < d or t.stride(0) % 2))
                   or (h_sel > 1 and (t.stride(1) < d or t.stride(1) % 2)) or t.data_ptr() % 4)
            return t.contiguous() if bad else t
        y, grad = wide(y), wide(grad)
        _require(not (need_dr or need_dx) or self.has_transpose,
                 "the gradients wrt r and the inputs sum over the COLUMNS of the hop matrices: they walk the plan's transposed operands "
                 "(no permutation is needed).  Build the plan with HopPlan(..., build_transpose=True)")
        self._bf16_attention_symbol(self.BF16_ATTENTION_SYMBOLS[2])
        dl = torch.empty((self.n_rows, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dl else None
        dr = torch.empty((self.n_cols, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dr else None
        dx = torch.empty((self.n_cols, d), dtype=dx_dtype, device=self.device) if need_dx else None
        if all(t is None or t.numel() == 0 for t in (dl, dr, dx)):   # (no node on the requested sides: nothing to write)
            return dl, dr, dx
        delta = torch.empty((self.n_rows, h_sel, n_heads), dtype=torch.float32, device=self.device) if need_dr or need_dx else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            st = _capi.lib().h2gcn_attention_hops_heads_backward_bf16(
                self._handle, mask, ptr(l), ldl, ptr(r), ldr, n_heads, float(negative_slope), ptr(x), x.stride(0) if self.n_cols > 1 else d, d,
                ptr(stats), h_sel * 2 * n_heads, ptr(y), y.stride(0) if self.n_rows > 1 else h_sel * d, y.stride(1) if h_sel > 1 else d,
                ptr(grad), grad.stride(0) if self.n_rows > 1 else h_sel * d, grad.stride(1) if h_sel > 1 else d,
                ptr(delta), h_sel * n_heads, ptr(dl), h_sel * n_heads, ptr(dr), h_sel * n_heads,
                _capi.DTYPE_BF16 if dx_dtype == torch.bfloat16 else _capi.DTYPE_F32, ptr(dx), d, C.c_void_p(stream))
        _capi.check(st)
        return dl, dr, dx

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _capi.lib().h2gcn_plan_destroy(h)
            except Exception:
                pass
            self._handle = C.c_void_p()


class RowSelection:
    """A set of rows of a :class:`HopPlan` (see :meth:`HopPlan.select_rows`).

    ``rows``: int32 ``[m]``, ascending and unique, on the plan's device; ``plan``: the :class:`HopPlan` of ``A_k[rows, :]``;
    ``n_rows_full``: the row count of the plan the selection was taken from.  ``rows_long`` is the same list as int64 (what
    torch's indexing ops take)."""

    def __init__(self, rows: torch.Tensor, plan: HopPlan, n_rows_full: int):
        self.rows = rows
        self.rows_long = rows.to(torch.int64)
        self.plan = plan
        self.n_rows_full = int(n_rows_full)

    def __len__(self) -> int:
        return int(self.rows.numel())
