"""CPU suite: symmetric hop plans (H2GCN_PLAN_SYMMETRIC_PATTERN, added within ABI 5) -- the flag and the two introspection
functions are declared, bound and exported consistently; the front end refuses what the mode does not cover before any device
work (no GPU in the build container)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
NEW = ("h2gcn_plan_transpose_sharing", "h2gcn_plan_device_bytes")


def test_header_defines_the_flag_and_declares_both_functions():
    assert int(re.search(r"#define H2GCN_PLAN_SYMMETRIC_PATTERN\s+(0x[0-9a-fA-F]+)u", HEADER).group(1), 16) == 0x10
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+h2gcn_plan_transpose_sharing\s*\(\s*const h2gcn_plan_t\*\s*plan,\s*int\s+hop\s*\)\s*;", code)
    assert re.search(r"\bsize_t\s+h2gcn_plan_device_bytes\s*\(\s*const h2gcn_plan_t\*\s*plan\s*\)\s*;", code)


def test_capi_carries_the_same_constant_and_prototypes():
    assert _capi.PLAN_SYMMETRIC_PATTERN == 0x10
    # one bit of its own
    others = (_capi.PLAN_BUILD_TRANSPOSE, _capi.PLAN_SKIP_VALIDATION, _capi.PLAN_HOST_TRANSPOSE, _capi.PLAN_KEEP_PERMUTATION)
    assert all(_capi.PLAN_SYMMETRIC_PATTERN & o == 0 for o in others)
    L = _capi.lib()
    assert L.h2gcn_plan_transpose_sharing.restype is ctypes.c_int
    assert list(L.h2gcn_plan_transpose_sharing.argtypes) == [ctypes.c_void_p, ctypes.c_int]
    assert L.h2gcn_plan_device_bytes.restype is ctypes.c_size_t
    assert list(L.h2gcn_plan_device_bytes.argtypes) == [ctypes.c_void_p]


def test_built_library_exports_both_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5


def test_introspection_validates_its_arguments():
    L = _capi.lib()
    assert L.h2gcn_plan_transpose_sharing(None, 0) == _capi.ERR_INVALID_ARGUMENT and b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_plan_device_bytes(None) == 0


def test_plan_create_refuses_bad_flag_combinations_before_the_device():
    """(the operand tables are NULL-filled: a call that got past the flag checks would be refused for them, with another message)"""
    L = _capi.lib()
    tab = (ctypes.c_void_p * 1)(None)
    handle = ctypes.c_void_p()

    def create(flags, n_rows=4, n_cols=4):
        opts = _capi.PlanOpts()
        opts.struct_size = ctypes.sizeof(_capi.PlanOpts)
        opts.flags = flags
        return L.h2gcn_plan_create(1, n_rows, n_cols, tab, tab, tab, ctypes.byref(opts), None, ctypes.byref(handle))

    S, T, HOST = _capi.PLAN_SYMMETRIC_PATTERN, _capi.PLAN_BUILD_TRANSPOSE, _capi.PLAN_HOST_TRANSPOSE
    assert create(S) == _capi.ERR_INVALID_ARGUMENT and b"H2GCN_PLAN_BUILD_TRANSPOSE" in L.h2gcn_last_error()
    assert create(S | T | HOST) == _capi.ERR_INVALID_ARGUMENT and b"H2GCN_PLAN_HOST_TRANSPOSE" in L.h2gcn_last_error()
    assert create(S | T, n_rows=3) == _capi.ERR_INVALID_ARGUMENT and b"square" in L.h2gcn_last_error()
    assert not handle.value


def test_cli_flag_exists_and_defaults_off():
    import argparse
    import importlib

    plugin = importlib.import_module("h2gcn_amd.models.H2GCN")
    p = argparse.ArgumentParser()
    p.function_hooks = {"argparse": []}
    plugin.add_subparser_args(p)
    assert p.parse_args([]).symmetric_hops is False
    assert p.parse_args(["--symmetric_hops"]).symmetric_hops is True


def test_get_tensors_refuses_a_row_partitioned_symmetric_plan():
    """Raised before any device work: the dataset object is bare and the device does not exist."""
    from h2gcn_amd.datasets._dataset import PlanetoidData
    from h2gcn_amd.datasets.synthetic import SyntheticShapeData

    data = object.__new__(PlanetoidData)
    with pytest.raises(ValueError, match=r"symmetric_hops covers one-GPU plans \(a row block of a symmetric matrix is not square\)"):
        data.get_tensors(torch.device("cuda:0"), adj_norm_hops=["1", "2"], shard=(0, 2), symmetric_hops=True)
    syn = object.__new__(SyntheticShapeData)
    with pytest.raises(ValueError, match="symmetric_hops covers one-GPU plans"):
        syn.get_tensors(torch.device("cuda:0"), shard=(0, 2), symmetric_hops=True)


def test_hop_plan_refuses_before_the_library_is_called():
    """The keyword's own preconditions come after the operand checks, which already need GPU tensors: check the order of the
    statements in the constructor instead (every refusal stands before the plan_create call)."""
    import inspect

    from h2gcn_amd import HopPlan

    src = inspect.getsource(HopPlan.__init__)
    call = src.index("h2gcn_plan_create")
    for word in ("symmetric_pattern=True modifies build_transpose=True", "cannot be combined with host_transpose=True",
                 "needs square operands", "predates symmetric plans"):
        assert 0 <= src.index(word) < call, word
    assert "symmetric_pattern" in inspect.signature(HopPlan.__init__).parameters
    assert inspect.signature(HopPlan.__init__).parameters["symmetric_pattern"].default is False
