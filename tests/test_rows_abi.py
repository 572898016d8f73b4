"""CPU suite: the row-selected classifier entry points (h2gcn_dropout_dense_rows_* / _backward_rows_*, added within ABI 5) are
declared, bound and exported consistently and validate their arguments before touching the device; HopPlan.select_rows and
the train_rows_only model switch refuse what they do not cover with the documented messages (no GPU in the build container)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
NEW = ("h2gcn_dropout_dense_rows_f32", "h2gcn_dropout_dense_rows_bf16",
       "h2gcn_dropout_dense_backward_rows_f32", "h2gcn_dropout_dense_backward_rows_bf16")
FULL = {"h2gcn_dropout_dense_rows_f32": "h2gcn_dropout_dense_f32", "h2gcn_dropout_dense_rows_bf16": "h2gcn_dropout_dense_bf16",
        "h2gcn_dropout_dense_backward_rows_f32": "h2gcn_dropout_dense_backward_f32",
        "h2gcn_dropout_dense_backward_rows_bf16": "h2gcn_dropout_dense_backward_bf16"}


def test_abi_version_stays_5():
    assert _capi.ABI_VERSION == 5
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    assert _capi.lib().h2gcn_abi_version() == 5


def test_rows_symbols_are_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in NEW:
        decl = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", code)
        assert decl, name
        assert re.search(r"const int32_t\*\s*rows_dev,\s*int64_t\s+n_sel\s*$", decl.group(1).strip()), name   # the two trailing arguments
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
        # the full call's signature followed by (rows_dev, n_sel)
        assert list(getattr(_capi.lib(), name).argtypes) == list(getattr(_capi.lib(), FULL[name]).argtypes) + [ctypes.c_void_p, ctypes.c_int64]
        assert getattr(_capi.lib(), name).restype is ctypes.c_int


def _fwd(L, name, *, x=16, ldx=8, n_rows=10, w=16, z=16, rows=16, n_sel=2):
    return getattr(L, name)(x, ldx, n_rows, 8, w, 3, None, 1.0, 0, None, z, 3, 16, 1 << 20, None, rows, n_sel)


def _bwd(L, name, *, x=16, ldx=8, n_rows=10, w=16, g=16, rows=16, n_sel=2, dx_dtype=_capi.DTYPE_BF16):
    extra = (dx_dtype,) if name.endswith("bf16") else ()
    return getattr(L, name)(x, ldx, n_rows, 8, w, 3, g, 3, 1.0, 0, None, *extra, 16, 8, 16, 16, 1 << 20, None, rows, n_sel)


@pytest.mark.parametrize("name", NEW)
def test_arguments_are_validated_before_the_device(name):
    """(the pointers are small fake addresses: a call that got past validation would fault, so every case must be refused)"""
    L = _capi.lib()
    call = _bwd if "backward" in name else _fwd
    for kw, word in ((dict(rows=None), b"rows_dev is NULL"), (dict(n_sel=-1), b"n_sel"), (dict(n_sel=11), b"n_sel"),
                     (dict(n_rows=-1), b"n_rows"), (dict(x=None), b"X_dev is NULL"), (dict(w=None), b"W_dev is NULL")):
        assert call(L, name, **kw) == _capi.ERR_INVALID_ARGUMENT, kw
        assert word in L.h2gcn_last_error(), (kw, L.h2gcn_last_error())
    if "backward" in name:
        assert call(L, name, g=None) == _capi.ERR_INVALID_ARGUMENT and b"G_dev is NULL" in L.h2gcn_last_error()
    else:
        assert call(L, name, z=None) == _capi.ERR_INVALID_ARGUMENT and b"Z_dev is NULL" in L.h2gcn_last_error()
    if name.endswith("bf16"):   # the layout rules of the bf16 calls
        assert call(L, name, ldx=9) == _capi.ERR_INVALID_ARGUMENT and b"ldx" in L.h2gcn_last_error()
        assert call(L, name, x=18) == _capi.ERR_INVALID_ARGUMENT and b"X_dev must be 4-byte aligned" in L.h2gcn_last_error()
    if name == "h2gcn_dropout_dense_backward_rows_bf16":
        assert call(L, name, dx_dtype=7) == _capi.ERR_INVALID_ARGUMENT and b"dx_dtype" in L.h2gcn_last_error()
    with pytest.raises(_capi.H2GCNError):
        _capi.check(call(L, name, rows=None))


def _cpu_plan(n_rows=6):
    from h2gcn_amd import HopPlan
    plan = object.__new__(HopPlan)   # a HopPlan cannot be constructed off the GPU: the fields select_rows looks at first
    plan.device, plan.n_rows, plan.n_cols, plan.n_hops = torch.device("cpu"), n_rows, n_rows, 1
    return plan


def test_select_rows_refuses_a_cpu_plan():
    with pytest.raises(ValueError, match="select_rows: the plan must live on a GPU"):
        _cpu_plan().select_rows([0, 1])


def test_select_rows_refuses_bad_input():
    class _Gpu:
        type = "cuda"
    plan = _cpu_plan()
    plan.device = _Gpu()      # past the device check: every case below is refused before anything is computed
    with pytest.raises(ValueError, match=r"a bool mask must have shape \[6\]"):
        plan.select_rows(torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="must be a bool mask or integer indices"):
        plan.select_rows(torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="must be one-dimensional"):
        plan.select_rows(torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="empty selection"):
        plan.select_rows(torch.zeros(0, dtype=torch.int64))


def test_model_refuses_what_train_rows_only_does_not_cover():
    from h2gcn_amd.models import parse_network_setup
    from h2gcn_amd.models.H2GCN import H2GCN

    ok = H2GCN(parse_network_setup("M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", 7), input_dim=10, train_rows_only=True)
    assert ok.train_rows_only
    with pytest.raises(ValueError, match="--no_fused_classifier"):
        H2GCN(parse_network_setup("M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", 7), input_dim=10, fused_classifier=False, train_rows_only=True)
    with pytest.raises(ValueError, match="units > 64"):
        H2GCN(parse_network_setup("M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", 100), input_dim=10, train_rows_only=True)
    with pytest.raises(ValueError, match="needs the fused propagation block"):
        H2GCN(parse_network_setup("M64-R-D0.5-MO", 7), input_dim=10, train_rows_only=True)
    off = H2GCN(parse_network_setup("M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", 7), input_dim=10)
    with pytest.raises(ValueError, match="train_rows_only=True"):
        off(None, None, None, rows=object())


def test_cli_flag_exists_and_defaults_off():
    import argparse

    import importlib
    plugin = importlib.import_module("h2gcn_amd.models.H2GCN")
    p = argparse.ArgumentParser()
    p.function_hooks = {"argparse": []}
    plugin.add_subparser_args(p)
    assert p.parse_args([]).train_rows_only is False
    assert p.parse_args(["--train_rows_only"]).train_rows_only is True
