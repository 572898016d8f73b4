"""CPU suite: the row softmax over the hop pattern (h2gcn_row_softmax_hops_f32 / h2gcn_row_softmax_backward_hops_f32, added
within ABI 5) -- both entry points are declared, bound and exported consistently, refuse a NULL plan before any device work,
and the front end has the three new entry points (no GPU in the build container)."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
FWD, BWD = "h2gcn_row_softmax_hops_f32", "h2gcn_row_softmax_backward_hops_f32"


def test_header_declares_both_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"int {FWD}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* const\* scores_dev, "
                     r"float\* const\* alpha_dev, void\* stream\);", code)
    assert re.search(rf"int {BWD}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* const\* alpha_dev, "
                     r"const float\* const\* dalpha_dev, float\* const\* dscores_dev, void\* stream\);", code)


def test_built_library_exports_both_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (FWD, BWD):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5


def test_capi_declares_the_prototypes():
    L = _capi.lib()
    table = ctypes.POINTER(ctypes.c_void_p)
    for name, n_tables in ((FWD, 2), (BWD, 3)):
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_uint32] + [table] * n_tables + [ctypes.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    tab = (ctypes.c_void_p * 1)(None)
    assert L.h2gcn_row_softmax_hops_f32(None, 0, tab, tab, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
    assert L.h2gcn_row_softmax_backward_hops_f32(None, 0, tab, tab, tab, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_softmax

    assert h2gcn_amd.hop_softmax is hop_softmax
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    p = inspect.signature(hop_softmax).parameters
    assert list(p) == ["adjhops", "scores", "hops"] and p["hops"].default is None and all(v.kind is kw for v in p.values())
    f = inspect.signature(HopPlan.row_softmax).parameters
    assert list(f) == ["self", "scores", "hops", "out"] and f["hops"].default is None and f["out"].default is None
    b = inspect.signature(HopPlan.row_softmax_backward).parameters
    assert list(b) == ["self", "alpha", "grad", "hops", "out"] and b["hops"].default is None and b["out"].default is None
    assert all(v.kind is kw for v in list(f.values()) + list(b.values()))


def test_a_row_partitioned_operand_is_refused_before_any_device_work():
    """A stand-in with `aggregate` is what the layers take for ShardedHops."""
    from h2gcn_amd.layers import hop_softmax

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_softmax(Sharded(), [None])
    with pytest.raises(ValueError, match="row-partitioned"):
        hop_softmax(Sharded(), [None], hops=[0])
