"""CPU suite: the bf16 classifier entry points (h2gcn_dropout_dense_bf16 / h2gcn_dropout_dense_backward_bf16, an additive
extension of ABI 5) are declared, bound and exported consistently and validate their arguments before touching the device (no
GPU in the build container); the bf16 classifier kernels compile for gfx950 without scratch; `--embedding_dtype` parses, the
model refuses what bfloat16 mode does not cover, and default arguments build the layers they built before."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
NEW = ("h2gcn_dropout_dense_bf16", "h2gcn_dropout_dense_backward_bf16")
H2GCN2 = "M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO"


def test_symbols_are_declared_bound_and_exported_and_the_abi_is_still_5():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
        assert getattr(_capi.lib(), name).argtypes is not None   # prototypes declared by the binding
    assert len(_capi.lib().h2gcn_dropout_dense_backward_bf16.argtypes) == len(_capi.lib().h2gcn_dropout_dense_backward_f32.argtypes) + 1
    assert _capi.ABI_VERSION == 5
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    assert _capi.lib().h2gcn_abi_version() == 5


# fake, suitably aligned device addresses: every call below is rejected before anything is dereferenced or launched
P = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1002)


def _fwd(x=P, ldx=448, w=P, z=P):
    return _capi.lib().h2gcn_dropout_dense_bf16(x, ldx, 100, 448, w, 7, None, 0.5, 1, None, z, 7, P, 1 << 30, None)


def _bwd(x=P, ldx=448, w=P, g=P, dx_dtype=_capi.DTYPE_BF16, dx=P, lddx=448):
    return _capi.lib().h2gcn_dropout_dense_backward_bf16(x, ldx, 100, 448, w, 7, g, 7, 0.5, 1, None, dx_dtype, dx, lddx, P, P, 1 << 30, None)


@pytest.mark.parametrize("call,kwargs,named", [
    (_fwd, dict(x=None), b"X_dev"), (_fwd, dict(w=None), b"W_dev"), (_fwd, dict(z=None), b"Z_dev"),
    (_bwd, dict(x=None), b"X_dev"), (_bwd, dict(w=None), b"W_dev"), (_bwd, dict(g=None), b"G_dev"),
])
def test_null_operands_are_rejected_before_the_device(call, kwargs, named):
    assert call(**kwargs) == _capi.ERR_INVALID_ARGUMENT
    msg = _capi.lib().h2gcn_last_error()
    assert named in msg and b"NULL" in msg, msg


@pytest.mark.parametrize("bad", [-1, 2, 7])
def test_bad_dx_dtype_is_rejected_before_the_device(bad):
    assert _bwd(dx_dtype=bad) == _capi.ERR_INVALID_ARGUMENT
    msg = _capi.lib().h2gcn_last_error()
    assert b"dx_dtype" in msg and b"H2GCN_DTYPE_BF16" in msg, msg
    with pytest.raises(_capi.H2GCNError):
        _capi.check(_bwd(dx_dtype=bad))


def test_odd_strides_and_misaligned_bases_are_rejected_before_the_device():
    L = _capi.lib()
    assert _fwd(ldx=449) == _capi.ERR_INVALID_ARGUMENT and b"ldx" in L.h2gcn_last_error() and b"even" in L.h2gcn_last_error()
    assert _bwd(ldx=449) == _capi.ERR_INVALID_ARGUMENT and b"ldx" in L.h2gcn_last_error()
    assert _bwd(lddx=449) == _capi.ERR_INVALID_ARGUMENT and b"lddx" in L.h2gcn_last_error() and b"even" in L.h2gcn_last_error()
    assert _fwd(x=ODD) == _capi.ERR_INVALID_ARGUMENT and b"X_dev" in L.h2gcn_last_error() and b"aligned" in L.h2gcn_last_error()
    assert _bwd(dx=ODD) == _capi.ERR_INVALID_ARGUMENT and b"dX_dev" in L.h2gcn_last_error()
    # an fp32 dX has no parity rule: an odd lddx passes the layout checks; the call is then stopped by the workspace check (0 bytes
    # handed in), still before the device
    st = L.h2gcn_dropout_dense_backward_bf16(P, 448, 100, 448, P, 7, P, 7, 0.5, 1, None, _capi.DTYPE_F32, P, 449, P, P, 0, None)
    assert st == _capi.ERR_INVALID_ARGUMENT and b"workspace" in L.h2gcn_last_error()


def test_bf16_classifier_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 on the bf16 translation unit: no error, and the compiler's resource remarks report
    0 bytes of scratch for every kernel in it."""
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        import shutil
        found = shutil.which("hipcc")
        assert found, "hipcc not found"
        hipcc = Path(found)
    src = ROOT / "h2gcn_amd" / "csrc" / "classifier_bf16.hip"
    r = subprocess.run([str(hipcc), "-O3", "-std=c++17", "-fPIC", f"-I{ROOT}/include", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "k.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "error:" not in r.stderr
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    bf16_kernels = [b for b in blocks if "bf16" in b.split("\n")[0]]
    # forward / dW / small forward on a bf16 X, dX / small dX to a bf16 dX: 3 + 12 + 12 + 3 + 12 instantiations
    assert len(bf16_kernels) == 42, len(bf16_kernels)
    for b in blocks:
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
        assert m and int(m.group(1)) == 0, b.split("\n")[0]


# ---- CLI and construction ----------------------------------------------------------------------------------------------------
def _parser():
    from h2gcn_amd import run_experiments
    from h2gcn_amd.models import H2GCN as H2GCN_mod

    parser = run_experiments.build_parser()
    H2GCN_mod.add_subparser_args(parser)
    return parser


def test_cli_flag_parses():
    assert _parser().parse_args([]).embedding_dtype == "float32"
    assert _parser().parse_args(["--embedding_dtype", "bfloat16"]).embedding_dtype == "bfloat16"
    with pytest.raises(SystemExit):
        _parser().parse_args(["--embedding_dtype", "float16"])


def _model(network=H2GCN2, hidden=64, **kw):
    from h2gcn_amd.models import parse_network_setup
    from h2gcn_amd.models.H2GCN import H2GCN

    setup = parse_network_setup(network, 7, _dense_units=hidden, _dropout_rate=0.5)
    torch.manual_seed(0)
    return H2GCN(setup, input_dim=1433, n_hops=2, l2_regularize_weight=5e-4, **kw)


def test_default_arguments_build_the_same_layers_as_before():
    from h2gcn_amd import layers as L

    m = _model()
    assert m.embedding_dtype == torch.float32
    assert [type(l).__name__ for l in m.layer_objs] == ["SparseDense", "Identity", "GCNLayer", "Flatten", "GCNLayer", "Flatten",
                                                         "ConcatLayer", "ConcatLayer", "Identity", "DropoutDense"]
    assert m.fused == (2, 8, 2, ["1", "2"]) and m.reuse_propagation
    b = _model(embedding_dtype=torch.bfloat16)
    assert [type(l).__name__ for l in b.layer_objs] == [type(l).__name__ for l in m.layer_objs]
    assert b.embedding_dtype == torch.bfloat16 and b.fused == m.fused and b.reuse_propagation
    assert all(p.dtype == torch.float32 for p in b.parameters())            # parameters stay float32
    for p, q in zip(m.parameters(), b.parameters()):                        # and are initialised identically
        assert torch.equal(p, q)
    assert isinstance(b.layer_objs[-1], L.DropoutDense)


def test_bfloat16_refuses_what_it_does_not_cover(monkeypatch):
    from h2gcn_amd.models import H2GCN as H2GCN_mod

    with pytest.raises(ValueError, match="fused propagation block.*float32"):
        _model("M64-R-D-MO", embedding_dtype=torch.bfloat16)                       # no propagation at all
    with pytest.raises(ValueError, match="fused propagation block"):
        _model("M64-R-T1-G0-V-C1-D0.5-MO", embedding_dtype=torch.bfloat16)          # a filtered G: generic interpreter
    with pytest.raises(ValueError, match="even.*--hidden"):
        _model("M-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", hidden=63, embedding_dtype=torch.bfloat16)
    _model("M-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", hidden=63)                           # float32: any width
    monkeypatch.setattr(H2GCN_mod, "_is_sharded", lambda: True)
    with pytest.raises(ValueError, match="row-partitioned.*float32"):
        _model(embedding_dtype=torch.bfloat16)
    _model()                                                                        # float32 row-partitioned runs are untouched
    monkeypatch.undo()
    with pytest.raises(ValueError, match="embedding_dtype"):
        _model(embedding_dtype=torch.float16)

    class FakeShardedHops:
        n_hops = 2

        def fused_propagation(self, *a, **k):
            raise AssertionError("must not be reached")

    m = _model(embedding_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="row-partitioned"):                       # the first forward handed a ShardedHops
        m(None, torch.zeros(4, 64), FakeShardedHops(), execute_after=m.fused[0])


def test_front_end_rejects_odd_widths_and_wrong_buffers():
    from h2gcn_amd import layers as L

    class Plan:
        n_rows = n_cols = 5
        n_hops = 2

    with pytest.raises(ValueError, match="even embedding width"):
        L.fused_propagation(Plan(), torch.zeros(5, 3), 1, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):
        L.fused_propagation(Plan(), torch.zeros(5, 2), 1, out=torch.zeros(5, 6), dtype=torch.bfloat16)   # out of the wrong dtype
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        L.fused_propagation(Plan(), torch.zeros(5, 2), 1, dtype=torch.float16)
    assert L.concat_buffer(3, 4, "cpu").dtype == torch.float32
    assert L.concat_buffer(3, 4, "cpu", torch.bfloat16).dtype == torch.bfloat16
