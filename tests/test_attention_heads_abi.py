"""CPU suite: the head dimension of the SDDMM, the row softmax and the edge scores (h2gcn_*_hops_heads_f32, added within ABI 5) --
the five entry points are declared with their contract, bound and exported consistently, refuse a NULL plan before any device
work, and the front end has the new names and refuses what it can without a GPU."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
SDDMM = "h2gcn_sddmm_hops_heads_f32"
SOFTMAX, SOFTMAX_BWD = "h2gcn_row_softmax_hops_heads_f32", "h2gcn_row_softmax_backward_hops_heads_f32"
SCORES, SCORES_BWD = "h2gcn_edge_scores_hops_heads_f32", "h2gcn_edge_scores_backward_hops_heads_f32"
ALL = (SDDMM, SOFTMAX, SOFTMAX_BWD, SCORES, SCORES_BWD)


def test_header_declares_the_five_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    head = r"\(const h2gcn_plan_t\* plan, uint32_t hop_mask, "
    protos = {
        SDDMM: r"const float\* dY_dev, int64_t ldg_row, int64_t ldg_hop, const float\* X_dev, int64_t ldx, int32_t d, "
               r"int32_t n_heads, float\* const\* dvals_dev, void\* stream\);",
        SOFTMAX: r"const float\* const\* scores_dev, float\* const\* alpha_dev, int32_t n_heads, void\* stream\);",
        SOFTMAX_BWD: r"const float\* const\* alpha_dev, const float\* const\* dalpha_dev, float\* const\* dscores_dev, "
                     r"int32_t n_heads, void\* stream\);",
        SCORES: r"const float\* l_dev, int64_t ldl, const float\* r_dev, int64_t ldr, int32_t n_heads, float negative_slope, "
                r"float\* const\* scores_dev, void\* stream\);",
        SCORES_BWD: r"const float\* l_dev, int64_t ldl, const float\* r_dev, int64_t ldr, int32_t n_heads, float negative_slope, "
                    r"const float\* const\* dscores_dev, float\* dl_dev, int64_t lddl, float\* dr_dev, int64_t lddr, void\* stream\);",
    }
    for name, rest in protos.items():
        assert re.search(rf"int {name}{head}{rest}", code), name


def test_header_states_the_contract_next_to_the_prototypes():
    at = HEADER.index(f"int {SDDMM}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("added within ABI 5", "CONTIGUOUS ENTRY-MAJOR", "e * K + h", "fp32 only", "d % K == 0", "w % 4 == 0",
                   "K == 1 takes any d", "i*ldl + s*K + h", "ldl >= H_sel*K", "NOTHING NEW",
                   "the bits equal those of the single-head entry point applied to head h alone",
                   "h2gcn_sddmm_hops_f32 with d := w", "a contiguous copy of column h", "l[:, :, h] and r[:, :, h]",
                   "long_row_threshold, rows_per_wave, variant, the hop selection", "gamma_w",
                   "a NaN in head h never changes a bit of another head", "write nothing (softmax) or +0 (dl, dr)",
                   "No atomics, no workspace, all offsets 64-bit", "hipGraph capture", "H2GCN_ERR_NO_TRANSPOSE",
                   "H2GCN_PLAN_KEEP_PERMUTATION", '"plan is NULL"', "n_heads < 1", "dl and dr both NULL"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in ALL:
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5


def test_capi_declares_the_prototypes():
    L, C = _capi.lib(), ctypes
    tbl = C.POINTER(C.c_void_p)
    want = {
        SDDMM: [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, tbl, C.c_void_p],
        SOFTMAX: [C.c_void_p, C.c_uint32, tbl, tbl, C.c_int32, C.c_void_p],
        SOFTMAX_BWD: [C.c_void_p, C.c_uint32, tbl, tbl, tbl, C.c_int32, C.c_void_p],
        SCORES: [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, tbl, C.c_void_p],
        SCORES_BWD: [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, tbl,
                     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    tab = (ctypes.c_void_p * 1)(None)
    calls = (
        lambda: L.h2gcn_sddmm_hops_heads_f32(None, 0, None, 8, 8, None, 8, 8, 2, tab, None),
        lambda: L.h2gcn_row_softmax_hops_heads_f32(None, 0, tab, tab, 2, None),
        lambda: L.h2gcn_row_softmax_backward_hops_heads_f32(None, 0, tab, tab, tab, 2, None),
        lambda: L.h2gcn_edge_scores_hops_heads_f32(None, 0, None, 2, None, 2, 2, 0.2, tab, None),
        lambda: L.h2gcn_edge_scores_backward_hops_heads_f32(None, 0, None, 2, None, 2, 2, 0.2, tab, None, 2, None, 2, None),
    )
    for call in calls:
        assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
        assert call() == _capi.ERR_INVALID_ARGUMENT
        assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import MultiHeadHopAttention, hop_edge_scores_heads, hop_softmax_heads

    assert h2gcn_amd.hop_edge_scores_heads is hop_edge_scores_heads and h2gcn_amd.hop_softmax_heads is hop_softmax_heads
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = {
        hop_softmax_heads: ["adjhops", "scores", "hops"],
        hop_edge_scores_heads: ["adjhops", "l", "r", "negative_slope", "hops"],
        HopPlan.sddmm_heads: ["self", "grad", "x", "heads", "hops", "out"],
        HopPlan.row_softmax_heads: ["self", "scores", "hops", "out"],
        HopPlan.row_softmax_heads_backward: ["self", "alpha", "grad", "hops", "out"],
        HopPlan.edge_scores_heads: ["self", "l", "r", "negative_slope", "hops", "out"],
        HopPlan.edge_scores_heads_backward: ["self", "l", "r", "grad", "negative_slope", "hops", "need_dl", "need_dr"],
    }
    defaults = {"hops": None, "out": None, "negative_slope": 0.2, "need_dl": True, "need_dr": True}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults:
                assert p[name].default == defaults[name], (fn, name)
            else:
                assert p[name].default is inspect.Parameter.empty, (fn, name)
    # the layer keeps its pinned signatures
    assert list(inspect.signature(MultiHeadHopAttention.__init__).parameters) == ["self", "in_dim", "heads", "hops", "n_hops", "negative_slope"]
    assert list(inspect.signature(MultiHeadHopAttention.forward).parameters) == ["self", "adjhops", "inputs"]


def _stand_in_plan(nnz=(5, 3), n_rows=4, n_cols=6, transpose=True, perm=True):
    """A HopPlan that never reached the library: what the argument checks read, on the CPU.  Any launch on it would fail, so a
    test that passes has been refused before the library was called."""
    from h2gcn_amd import HopPlan

    plan = object.__new__(HopPlan)
    plan._handle = None
    plan.n_hops, plan.n_rows, plan.n_cols = len(nnz), n_rows, n_cols
    plan.device = torch.device("cpu")
    plan.colidx = [torch.zeros(n, dtype=torch.int32) for n in nnz]
    plan.has_transpose, plan.keep_permutation = transpose, transpose and perm
    return plan


def test_python_side_refusals_need_no_device():
    from h2gcn_amd.layers import hop_edge_scores_heads, hop_softmax_heads

    plan = _stand_in_plan()
    g, x = torch.zeros(4, 2, 8), torch.zeros(6, 8)
    v = [torch.zeros(5, 2), torch.zeros(3, 2)]
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    bf = torch.bfloat16
    bad = [
        # sddmm_heads
        ("grad must be", lambda: plan.sddmm_heads(torch.zeros(4, 1, 8), x, 2)),
        ("x must be", lambda: plan.sddmm_heads(g, torch.zeros(5, 8), 2)),
        ("must be float32", lambda: plan.sddmm_heads(g.to(bf), x.to(bf), 2)),
        ("must be float32", lambda: plan.sddmm_heads(g, x.double(), 2)),
        ("heads = 0 < 1", lambda: plan.sddmm_heads(g, x, 0)),
        ("not a multiple of the number of heads", lambda: plan.sddmm_heads(g, x, 3)),
        ("must be a multiple of 4", lambda: plan.sddmm_heads(g, x, 4)),
        ("one per selected hop", lambda: plan.sddmm_heads(g, x, 2, out=v[:1])),
        ("must have shape", lambda: plan.sddmm_heads(g, x, 2, out=[v[0], torch.zeros(3)])),
        ("2 are expected", lambda: plan.sddmm_heads(g, x, 2, out=[v[0], torch.zeros(3, 4)])),
        ("must be contiguous", lambda: plan.sddmm_heads(g, x, 2, out=[torch.zeros(2, 5).t(), v[1]])),
        # softmax
        ("one per selected hop", lambda: plan.row_softmax_heads(v[:1])),
        ("one per selected hop", lambda: plan.row_softmax_heads(v[0])),
        ("one per selected hop", lambda: plan.row_softmax_heads(v, hops=[1])),
        ("must be float32", lambda: plan.row_softmax_heads([v[0].to(bf), v[1]])),
        ("must have shape", lambda: plan.row_softmax_heads([v[0], torch.zeros(3)])),
        ("must have shape", lambda: plan.row_softmax_heads([v[0], torch.zeros(4, 2)])),
        ("same K", lambda: plan.row_softmax_heads([v[0], torch.zeros(3, 4)])),
        ("must be contiguous", lambda: plan.row_softmax_heads([torch.zeros(2, 5).t(), v[1]])),
        ("must be contiguous", lambda: plan.row_softmax_heads([torch.zeros(5, 4)[:, ::2], v[1]])),
        ("same K", lambda: plan.row_softmax_heads_backward(v, [torch.zeros(5, 3), torch.zeros(3, 3)])),
        ("must be float32", lambda: plan.row_softmax_heads_backward(v, [v[0], v[1].double()])),
        ("same K", lambda: plan.row_softmax_heads(v, out=[torch.zeros(5, 1), torch.zeros(3, 1)])),
        ("one per selected hop", lambda: hop_softmax_heads(plan, v[0])),
        # edge scores
        ("l must have shape", lambda: plan.edge_scores_heads(torch.zeros(4, 2), r)),
        ("l must have shape", lambda: plan.edge_scores_heads(torch.zeros(5, 2, 2), r)),
        ("r must have shape", lambda: plan.edge_scores_heads(l, torch.zeros(6, 2, 3))),
        ("r must have shape", lambda: plan.edge_scores_heads(l, torch.zeros(6, 1, 2))),
        ("must be float32", lambda: plan.edge_scores_heads(l.to(bf), r.to(bf))),
        ("must have shape", lambda: plan.edge_scores_heads(l, r, out=[v[0], torch.zeros(3)])),
        ("both False", lambda: plan.edge_scores_heads_backward(l, r, v, need_dl=False, need_dr=False)),
        ("same K", lambda: plan.edge_scores_heads_backward(l, r, [torch.zeros(5, 3), torch.zeros(3, 3)])),
        ("must be contiguous", lambda: plan.edge_scores_heads_backward(l, r, [torch.zeros(2, 5).t(), v[1]])),
        ("keep_permutation=True", lambda: _stand_in_plan(perm=False).edge_scores_heads_backward(l, r, v)),
        ("no transposed operands", lambda: _stand_in_plan(transpose=False).edge_scores_heads_backward(l, r, v)),
        ("keep_permutation=True", lambda: hop_edge_scores_heads(_stand_in_plan(perm=False), l, r.clone().requires_grad_())),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_a_row_partitioned_operand_is_refused_before_any_device_work():
    from h2gcn_amd.layers import hop_edge_scores_heads, hop_softmax_heads

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_edge_scores_heads(Sharded(), None, None)
    with pytest.raises(ValueError, match="row-partitioned"):
        hop_softmax_heads(Sharded(), None, hops=[0])
    with pytest.raises(TypeError, match="HopPlan"):
        hop_softmax_heads(object(), [])


def test_a_library_without_the_symbols_is_named(monkeypatch):
    plan = _stand_in_plan()
    monkeypatch.setattr(_capi, "has", lambda name: not name.endswith("_heads_f32"))
    with pytest.raises(RuntimeError, match="h2gcn_row_softmax_hops_heads_f32"):
        plan.row_softmax_heads([torch.zeros(5, 2), torch.zeros(3, 2)])
    with pytest.raises(RuntimeError, match="h2gcn_sddmm_hops_heads_f32"):
        plan.sddmm_heads(torch.zeros(4, 2, 8), torch.zeros(6, 8), 2)
