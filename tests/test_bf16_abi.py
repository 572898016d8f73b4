"""CPU suite: the bf16 launches of ABI 5 (h2gcn_spmm_hops_bf16 / h2gcn_spmm_hops_T_bf16) are declared, bound and exported
consistently, and reject a NULL plan / an unknown dtype code before touching the device (no GPU in the build container)."""
import ctypes
import re
from pathlib import Path

import pytest

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
NEW = ("h2gcn_spmm_hops_bf16", "h2gcn_spmm_hops_T_bf16")


def test_abi_5_in_header_binding_and_library():
    assert _capi.ABI_VERSION == 5
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    assert _capi.lib().h2gcn_abi_version() == 5


def test_bf16_symbols_are_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
        assert getattr(_capi.lib(), name).argtypes is not None   # prototypes declared by the binding


def test_dtype_codes_agree():
    for name, val in (("H2GCN_DTYPE_F32", _capi.DTYPE_F32), ("H2GCN_DTYPE_BF16", _capi.DTYPE_BF16)):
        assert int(re.search(rf"#define {name}\s+(\d+)", HEADER).group(1)) == val
    assert (_capi.DTYPE_F32, _capi.DTYPE_BF16) == (0, 1)


@pytest.mark.parametrize("out_dtype", [_capi.DTYPE_F32, _capi.DTYPE_BF16])
def test_null_plan_is_an_error_not_a_crash(out_dtype):
    L = _capi.lib()
    assert L.h2gcn_spmm_hops_bf16(None, 0, None, 128, 128, out_dtype, None, 256, 128, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_spmm_hops_T_bf16(None, 0, None, 256, 128, 128, out_dtype, None, 128, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


@pytest.mark.parametrize("bad", [-1, 2, 7])
def test_bad_dtype_code_is_rejected_before_the_device(bad):
    L = _capi.lib()
    assert L.h2gcn_spmm_hops_bf16(None, 0, None, 128, 128, bad, None, 256, 128, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"y_dtype" in L.h2gcn_last_error() and b"H2GCN_DTYPE_BF16" in L.h2gcn_last_error()
    assert L.h2gcn_spmm_hops_T_bf16(None, 0, None, 256, 128, 128, bad, None, 128, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"dx_dtype" in L.h2gcn_last_error()
    with pytest.raises(_capi.H2GCNError):
        _capi.check(L.h2gcn_spmm_hops_bf16(None, 0, None, 128, 128, bad, None, 256, 128, None, None))


def test_bf16_dx_with_accumulate_is_rejected_before_the_device():
    L = _capi.lib()
    opts = _capi.LaunchOpts(struct_size=ctypes.sizeof(_capi.LaunchOpts), flags=_capi.LAUNCH_ACCUMULATE)
    st = L.h2gcn_spmm_hops_T_bf16(None, 0, None, 256, 128, 128, _capi.DTYPE_BF16, None, 128, ctypes.byref(opts), None)
    assert st == _capi.ERR_INVALID_ARGUMENT
    assert b"ACCUMULATE" in L.h2gcn_last_error()
