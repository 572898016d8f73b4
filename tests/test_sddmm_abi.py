"""CPU suite: the values gradient of the hop SpMM (h2gcn_sddmm_hops_f32 / _bf16, added within ABI 5) -- both entry points are
declared, bound and exported consistently, refuse a NULL plan before any device work, and the front end takes the new optional
argument (no GPU in the build container)."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
NEW = ("h2gcn_sddmm_hops_f32", "h2gcn_sddmm_hops_bf16")


def test_header_declares_both_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    for name, elem in (("h2gcn_sddmm_hops_f32", "float"), ("h2gcn_sddmm_hops_bf16", "uint16_t")):
        proto = (rf"int {name}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const {elem}\* dY_dev, int64_t ldg_row, "
                 rf"int64_t ldg_hop, const {elem}\* X_dev, int64_t ldx, int32_t d, float\* const\* dvals_dev, void\* stream\);")
        assert re.search(proto, code), name


def test_built_library_exports_both_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5


def test_capi_declares_the_prototypes():
    L = _capi.lib()
    want = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
            ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want


@pytest.mark.parametrize("name", NEW)
def test_null_plan_is_refused_without_a_device(name):
    L = _capi.lib()
    tab = (ctypes.c_void_p * 1)(None)
    assert getattr(L, name)(None, 0, None, 4, 4, None, 4, 4, tab, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_takes_the_optional_values_argument():
    from h2gcn_amd import GCNLayer, HopPlan
    from h2gcn_amd.layers import hop_spmm

    p = inspect.signature(hop_spmm).parameters
    assert list(p) == ["adjhops", "inputs", "hops", "values"] and p["values"].default is None
    assert p["values"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    q = inspect.signature(GCNLayer.forward).parameters
    assert list(q) == ["self", "adjhops", "inputs", "values"] and q["values"].default is None
    assert q["values"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    s = inspect.signature(HopPlan.sddmm).parameters
    assert list(s) == ["self", "grad", "x", "hops", "out"] and s["hops"].default is None and s["out"].default is None


def test_values_on_a_row_partitioned_operand_are_refused_before_any_device_work():
    """A stand-in with `aggregate` is what GCNLayer takes for ShardedHops."""
    from h2gcn_amd import GCNLayer
    from h2gcn_amd.layers import hop_spmm

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_spmm(Sharded(), None, None, [None])
    with pytest.raises(ValueError, match="row-partitioned"):
        GCNLayer()(Sharded(), None, values=[None])
