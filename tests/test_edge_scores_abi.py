"""CPU suite: the additive edge scores on the hop pattern (h2gcn_edge_scores_hops_f32 / h2gcn_edge_scores_backward_hops_f32,
added within ABI 5) -- both entry points are declared, bound and exported consistently, refuse a NULL plan before any device
work, and the front end has the new entry points (no GPU in the build container)."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
FWD, BWD = "h2gcn_edge_scores_hops_f32", "h2gcn_edge_scores_backward_hops_f32"


def test_header_declares_both_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"int {FWD}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* l_dev, int64_t ldl, "
                     r"const float\* r_dev, int64_t ldr, float negative_slope, float\* const\* scores_dev, void\* stream\);", code)
    assert re.search(rf"int {BWD}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* l_dev, int64_t ldl, "
                     r"const float\* r_dev, int64_t ldr, float negative_slope, const float\* const\* dscores_dev, "
                     r"float\* dl_dev, int64_t lddl, float\* dr_dev, int64_t lddr, void\* stream\);", code)


def test_built_library_exports_both_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (FWD, BWD):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5


def test_capi_declares_the_prototypes():
    L = _capi.lib()
    C = ctypes
    head = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.POINTER(C.c_void_p)]
    fwd, bwd = getattr(L, FWD), getattr(L, BWD)
    assert fwd.restype is C.c_int and bwd.restype is C.c_int
    assert list(fwd.argtypes) == head + [C.c_void_p]
    assert list(bwd.argtypes) == head + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    tab = (ctypes.c_void_p * 1)(None)
    assert L.h2gcn_edge_scores_hops_f32(None, 0, None, 1, None, 1, 0.2, tab, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
    assert L.h2gcn_edge_scores_backward_hops_f32(None, 0, None, 1, None, 1, 0.2, tab, None, 1, None, 1, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import GCNLayer, HopAttention, hop_edge_scores

    assert h2gcn_amd.hop_edge_scores is hop_edge_scores and h2gcn_amd.HopAttention is HopAttention
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    p = inspect.signature(hop_edge_scores).parameters
    assert list(p) == ["adjhops", "l", "r", "negative_slope", "hops"] and all(v.kind is kw for v in p.values())
    assert p["negative_slope"].default == 0.2 and p["hops"].default is None
    f = inspect.signature(HopPlan.edge_scores).parameters
    assert list(f) == ["self", "l", "r", "negative_slope", "hops", "out"]
    assert f["negative_slope"].default == 0.2 and f["hops"].default is None and f["out"].default is None
    b = inspect.signature(HopPlan.edge_scores_backward).parameters
    assert list(b) == ["self", "l", "r", "grad", "negative_slope", "hops", "need_dl", "need_dr"]
    assert b["negative_slope"].default == 0.2 and b["hops"].default is None and b["need_dl"].default is True and b["need_dr"].default is True
    assert all(v.kind is kw for v in list(f.values()) + list(b.values()))
    c = inspect.signature(HopAttention.__init__).parameters
    assert list(c) == ["self", "in_dim", "hops", "n_hops", "negative_slope"]
    assert c["hops"].default is None and c["n_hops"].default == 2 and c["negative_slope"].default == 0.2
    # the calling convention of GCNLayer
    assert HopAttention.SIGNATURE == GCNLayer.SIGNATURE
    assert list(inspect.signature(HopAttention.forward).parameters) == ["self", "adjhops", "inputs"]


def test_hop_attention_parameters():
    import torch

    from h2gcn_amd import HopAttention

    torch.manual_seed(0)
    layer = HopAttention(24)
    assert tuple(layer.a_l.shape) == (2, 24) and tuple(layer.a_r.shape) == (2, 24)
    bound = (6.0 / (2 + 24)) ** 0.5                                          # Glorot uniform
    for a in (layer.a_l, layer.a_r):
        assert a.requires_grad and 0.5 * bound < float(a.detach().abs().max()) <= bound
    assert not torch.equal(layer.a_l, layer.a_r)
    assert tuple(HopAttention(7, hops=[1]).a_l.shape) == (1, 7) and tuple(HopAttention(7, n_hops=3).a_r.shape) == (3, 7)


def test_a_row_partitioned_operand_is_refused_before_any_device_work():
    """A stand-in with `aggregate` is what the layers take for ShardedHops."""
    from h2gcn_amd.layers import HopAttention, hop_edge_scores

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_edge_scores(Sharded(), None, None)
    with pytest.raises(ValueError, match="row-partitioned"):
        hop_edge_scores(Sharded(), None, None, 0.2, hops=[0])
    with pytest.raises(ValueError, match="row-partitioned"):
        HopAttention(4)(Sharded(), None)
