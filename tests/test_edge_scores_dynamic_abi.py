"""CPU suite: the dynamic (GATv2) edge scores (h2gcn_edge_scores_dynamic_workspace_bytes, h2gcn_edge_scores_dynamic_hops_f32 and
h2gcn_edge_scores_dynamic_backward_hops_f32, added within ABI 5; h2gcn_amd/csrc/edge_scores_dynamic.hip) -- the three entry points
are declared with their contract, bound and exported consistently and refuse a NULL plan before any device work; the front end
(HopPlan.edge_scores_dynamic / edge_scores_dynamic_backward, hop_edge_scores_dynamic, DynamicHopAttention) has the documented
signatures, parameters and refusals, all of them before a launch."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi
from test_attention_fused_abi import _stand_in_plan

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
WORKSPACE = "h2gcn_edge_scores_dynamic_workspace_bytes"
FORWARD = "h2gcn_edge_scores_dynamic_hops_f32"
BACKWARD = "h2gcn_edge_scores_dynamic_backward_hops_f32"
NODE_ARGS = (r"const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* u_dev, int64_t ldu, const float\* v_dev, int64_t ldv, "
             r"const float\* a_dev, int64_t lda, int32_t d, int32_t n_heads, float negative_slope, ")


def test_header_declares_the_three_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"size_t {WORKSPACE}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, int32_t d\);", code)
    assert re.search(rf"int {FORWARD}\({NODE_ARGS}float\* const\* scores_dev, void\* stream\);", code)
    assert re.search(rf"int {BACKWARD}\({NODE_ARGS}const float\* const\* dscores_dev, float\* du_dev, int64_t lddu, float\* dv_dev, "
                     r"int64_t lddv, float\* da_dev, int64_t ldda, void\* workspace_dev, size_t workspace_bytes, void\* stream\);", code)


def test_header_states_the_arithmetic_next_to_the_prototypes():
    at = HEADER.index(f"size_t {WORKSPACE}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("added within ABI 5", "a NaN p takes the slope branch", "d <= 256", "d % n_heads == 0", "w % 4 == 0 when n_heads > 1",
                   "the order of h2gcn_sddmm_hops_heads_f32", "of h2gcn_sddmm_hops_f32", "fma(a1, q1, t)", "gamma_{w+2}",
                   "contraction off", "P[m mod 4]", "(P0 + P1) + (P2 + P3)", "((T0 + T1) + T2) + T3", "ascending order",
                   "never of rows_per_wave", "gamma_{n+2}", "ONE partial row per selected hop", "a function of G alone", "never on the run",
                   "gamma_{nnz_s+3}", "No float atomics", "H2GCN_ERR_NO_TRANSPOSE", "H2GCN_PLAN_KEEP_PERMUTATION", "writes +0",
                   "zeroes the requested outputs without a launch", "hipGraph capture", "du, dv and da all NULL", "d > 256"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbols_and_the_unit_is_built():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (WORKSPACE, FORWARD, BACKWARD):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5
    makefile = (ROOT / "h2gcn_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()
    assert "edge_scores_dynamic.hip" in srcs
    assert (ROOT / "h2gcn_amd" / "csrc" / "edge_scores_dynamic.hip").is_file()


def test_capi_declares_the_prototypes():
    L, C = _capi.lib(), ctypes
    node = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float,
            C.POINTER(C.c_void_p)]
    fn = getattr(L, WORKSPACE)
    assert fn.restype is C.c_size_t and list(fn.argtypes) == [C.c_void_p, C.c_uint32, C.c_int32]
    fn = getattr(L, FORWARD)
    assert fn.restype is C.c_int and list(fn.argtypes) == node + [C.c_void_p]
    fn = getattr(L, BACKWARD)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    assert L.h2gcn_edge_scores_dynamic_workspace_bytes(None, 3, 128) == 0
    assert L.h2gcn_edge_scores_dynamic_hops_f32(None, 3, None, 8, None, 8, None, 8, 8, 2, 0.2, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_edge_scores_dynamic_backward_hops_f32(None, 3, None, 8, None, 8, None, 8, 8, 2, 0.2, None, None, 8, None, 8, None, 8, None, 0,
                                                         None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import DynamicHopAttention, HopPlan, hop_edge_scores_dynamic
    from h2gcn_amd.layers import MultiHeadHopAttention

    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = {
        HopPlan.edge_scores_dynamic: ["self", "u", "v", "a", "heads", "negative_slope", "hops", "out"],
        HopPlan.edge_scores_dynamic_backward: ["self", "u", "v", "a", "grad", "heads", "negative_slope", "hops", "need_du", "need_dv", "need_da"],
        hop_edge_scores_dynamic: ["adjhops", "u", "v", "a", "heads", "negative_slope", "hops"],
        DynamicHopAttention.__init__: ["self", "in_dim", "heads", "hops", "n_hops", "negative_slope", "share_weights"],
        DynamicHopAttention.forward: ["self", "adjhops", "inputs"],
    }
    defaults = {"heads": 1, "negative_slope": 0.2, "hops": None, "out": None, "need_du": True, "need_dv": True, "need_da": True, "n_hops": 2,
                "share_weights": False}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults and not (fn is DynamicHopAttention.__init__ and name == "heads"):
                assert p[name].default == defaults[name], (fn, name)
            else:
                assert p[name].default is inspect.Parameter.empty, (fn, name)
    assert HopPlan.EDGE_SCORES_DYNAMIC_MAX_WIDTH == 256
    assert DynamicHopAttention.SIGNATURE == MultiHeadHopAttention.SIGNATURE == ["adjhops", "inputs"]
    assert h2gcn_amd.DynamicHopAttention is DynamicHopAttention and h2gcn_amd.hop_edge_scores_dynamic is hop_edge_scores_dynamic


def test_layer_constructor_parameters_and_generator_order():
    from h2gcn_amd import DynamicHopAttention

    for bad, match in (((30, 4), "in_dim % heads == 0"), ((24, 4), "must be a multiple of 4"), ((8, 0), "heads >= 1"),
                       ((260, 1), "EDGE_SCORES_DYNAMIC_MAX_WIDTH = 256")):
        with pytest.raises(ValueError, match=match):
            DynamicHopAttention(*bad)
    with pytest.raises(ValueError, match="at least one hop"):
        DynamicHopAttention(8, 2, hops=[])
    DynamicHopAttention(22, 1)      # (one head takes any width)
    layer = DynamicHopAttention(32, 8)
    assert [(k, tuple(v.shape)) for k, v in layer.state_dict().items()] == [("W_l", (32, 32)), ("W_r", (32, 32)), ("a", (2, 8, 4))]
    shared = DynamicHopAttention(32, 8, hops=[1], share_weights=True)
    assert [(k, tuple(v.shape)) for k, v in shared.state_dict().items()] == [("W_l", (32, 32)), ("a", (1, 8, 4))]
    assert DynamicHopAttention(32, 8, n_hops=3).a.shape == (3, 8, 4)
    # Glorot-uniform, drawn in the order W_l, W_r, a
    for share in (False, True):
        torch.manual_seed(11)
        layer = DynamicHopAttention(32, 8, share_weights=share)
        torch.manual_seed(11)
        for name, shape in (("W_l", (32, 32)),) + ((("W_r", (32, 32)),) if not share else ()) + (("a", (2, 8, 4)),):
            want = torch.nn.init.xavier_uniform_(torch.empty(shape))
            assert torch.equal(getattr(layer, name).detach(), want), name
        follow = torch.rand(3)
        torch.manual_seed(11)
        DynamicHopAttention(32, 8, share_weights=share)
        assert torch.equal(torch.rand(3), follow)
    assert "share_weights=True" in repr(shared)


def _forbid_launches(monkeypatch):
    from h2gcn_amd import HopPlan

    def forbidden(name):
        def fn(self, *args, **kwargs):
            raise AssertionError(f"{name} was launched")
        return fn

    for name in ("edge_scores_dynamic", "edge_scores_dynamic_backward", "edge_scores_heads", "edge_scores", "row_softmax_heads", "row_softmax",
                 "spmm_values", "sddmm_heads"):
        monkeypatch.setattr(HopPlan, name, forbidden(name))


def test_plan_methods_refuse_without_a_device():
    plan = _stand_in_plan()
    z = lambda *shape: torch.zeros(*shape)     # noqa: E731
    u, v, a = z(4, 8), z(6, 8), z(2, 8)
    g = [z(5, 2), z(3, 2)]
    fwd, bwd = plan.edge_scores_dynamic, plan.edge_scores_dynamic_backward
    bad = []
    for f in (lambda *args, **kw: fwd(*args, **kw), lambda uu, vv, aa, *args, **kw: bwd(uu, vv, aa, kw.pop("grad", g), *args, **kw)):
        bad += [
            ("u must be a tensor", lambda f=f: f(None, v, a, 2)),
            ("u must be float32", lambda f=f: f(u.to(torch.bfloat16), v, a, 2)),
            ("v must be float32", lambda f=f: f(u, v.double(), a, 2)),
            (r"u must be \[4, d\]", lambda f=f: f(z(5, 8), v, a, 2)),
            (r"u must be \[4, d\]", lambda f=f: f(z(4), v, a, 2)),
            (r"v must be \[6, 8\]", lambda f=f: f(u, z(6, 12), a, 2)),
            (r"v must be \[6, 8\]", lambda f=f: f(u, z(4, 8), a, 2)),
            ("heads = 0 < 1", lambda f=f: f(u, v, a, 0)),
            ("not a multiple of the number of heads", lambda f=f: f(u, v, a, 3)),
            ("must be a multiple of 4", lambda f=f: f(z(4, 12), z(6, 12), z(2, 12), 2)),
            ("exceeds EDGE_SCORES_DYNAMIC_MAX_WIDTH = 256", lambda f=f: f(z(4, 260), z(6, 260), z(2, 260), 1)),
            (r"a must be \[2, 8\] or \[2, 2, 4\]", lambda f=f: f(u, v, z(1, 8), 2)),
            (r"a must be \[1, 8\]", lambda f=f: f(u, v, a, 2, hops=[1])),
            (r"a must be \[2, 8\] or \[2, 2, 4\]", lambda f=f: f(u, v, z(2, 4, 2), 2)),
        ]
    bad += [
        ("out must list 2 tensors", lambda: fwd(u, v, a, 2, out=[z(5, 2)])),
        (r"out\[0\] must have shape \[5, K\]", lambda: fwd(u, v, a, 2, out=[z(5), z(3)])),
        (r"out\[1\] must have shape \[3\]", lambda: fwd(u, v, a, 1, out=[z(5), z(3, 1)])),
        (r"out\[0\] must be contiguous", lambda: fwd(u, v, a, 2, out=[z(5, 4)[:, ::2], z(3, 2)])),
        ("grad must list 2 tensors", lambda: bwd(u, v, a, g[:1], 2)),
        (r"grad\[0\] has 2 heads where 4 are expected", lambda: bwd(z(4, 16), z(6, 16), z(2, 16), g, 4)),
        (r"grad\[1\] must have shape \[3\]", lambda: bwd(u, v, a, [z(5), z(3, 1)], 1)),
        ("grad must be a sequence", lambda: bwd(u, v, a, z(5, 2), 2)),
        ("all False", lambda: bwd(u, v, a, g, 2, need_du=False, need_dv=False, need_da=False)),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()
    bare = _stand_in_plan()
    bare.has_transpose = bare.keep_permutation = False
    for needs in ({}, {"need_du": False, "need_da": False}):
        with pytest.raises(ValueError, match=r"build_transpose=True, keep_permutation=True\)"):
            bare.edge_scores_dynamic_backward(u, v, a, g, 2, **needs)
    noperm = _stand_in_plan()
    noperm.keep_permutation = False
    with pytest.raises(ValueError, match="keep_permutation=True"):
        noperm.edge_scores_dynamic_backward(u, v, a, g, 2)


def test_a_library_without_the_symbols_says_rebuild_it(monkeypatch):
    plan = _stand_in_plan()
    u, v, a = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(2, 8)
    g = [torch.zeros(5, 2), torch.zeros(3, 2)]
    for gone in (WORKSPACE, FORWARD, BACKWARD):
        monkeypatch.setattr(_capi, "has", lambda name, gone=gone: name != gone)
        for call in (lambda: plan.edge_scores_dynamic(u, v, a, 2), lambda: plan.edge_scores_dynamic_backward(u, v, a, g, 2)):
            with pytest.raises(RuntimeError, match=f"predates the dynamic edge scores.*{gone}.*rebuild it"):
                call()


def test_function_and_layer_refusals_reach_no_launch(monkeypatch):
    from h2gcn_amd import DynamicHopAttention, hop_edge_scores_dynamic

    _forbid_launches(monkeypatch)
    plan = _stand_in_plan(n_rows=6)
    z = lambda *shape: torch.zeros(*shape)     # noqa: E731
    u, v, a = z(6, 8), z(6, 8), z(2, 8)

    class Sharded:
        def aggregate(self):
            pass

    with pytest.raises(ValueError, match=r"hop_edge_scores_dynamic is not supported on row-partitioned operands \(ShardedHops\)"):
        hop_edge_scores_dynamic(Sharded(), u, v, a, 2)
    with pytest.raises(TypeError, match="adjhops must be a HopPlan"):
        hop_edge_scores_dynamic(object(), u, v, a, 2)
    with pytest.raises(ValueError, match="EDGE_SCORES_DYNAMIC_MAX_WIDTH = 256, got d = 260"):
        hop_edge_scores_dynamic(plan, z(6, 260).requires_grad_(), z(6, 260), z(2, 260), 1)
    noperm = _stand_in_plan(n_rows=6)
    noperm.keep_permutation = False
    with pytest.raises(ValueError, match=r"hop_edge_scores_dynamic with a v that requires a gradient.*keep_permutation=True\)"):
        hop_edge_scores_dynamic(noperm, u, v.clone().requires_grad_(), a, 2)
    with pytest.raises(AssertionError, match="edge_scores_dynamic was launched"):      # (u alone needs no transposes: it goes on to the launch)
        hop_edge_scores_dynamic(noperm, u.clone().requires_grad_(), v, a, 2)
    layer = DynamicHopAttention(8, 2)
    with pytest.raises(ValueError, match=r"DynamicHopAttention is not supported on row-partitioned operands \(ShardedHops\)"):
        layer(Sharded(), u)
    with pytest.raises(TypeError, match="adjhops must be a HopPlan"):
        layer(object(), u)
    with pytest.raises(ValueError, match="holds attention vectors for 2 hops"):
        DynamicHopAttention(8, 2, n_hops=2)(_stand_in_plan(nnz=(5,), n_rows=6), u)
    with pytest.raises(ValueError, match="needs a square plan"):
        layer(_stand_in_plan(), z(6, 8))
    with pytest.raises(ValueError, match=r"inputs must be \[6, 8\]"):
        layer(plan, z(6, 12))
    with pytest.raises(ValueError, match="keep_permutation=True"):          # training on a plan without the permutation
        layer(noperm, u)
