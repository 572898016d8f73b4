"""CPU suite: bf16 embeddings in the recomputing hop attention (h2gcn_attention_hops_heads_bf16, ..._stats_bf16 and
..._backward_bf16, added within ABI 5; h2gcn_amd/csrc/attention_bf16.hip) -- the three entry points are declared with their
contract, bound and exported consistently and refuse a NULL plan before any device work; the front end
(HopPlan.attention_heads_bf16 / attention_heads_stats_bf16 / attention_heads_backward_bf16, hop_attention_heads,
hop_attention_recompute, RecomputeMultiHeadHopAttention) refuses what bf16 does not cover instead of running it in float32, reaches
only the bf16 calls on a bfloat16 input and only the fp32 calls on a float32 one."""
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
FORWARD = "h2gcn_attention_hops_heads_bf16"
STATS = "h2gcn_attention_hops_heads_stats_bf16"
BACKWARD = "h2gcn_attention_hops_heads_backward_bf16"
NODE_ARGS = (r"const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* l_dev, int64_t ldl, const float\* r_dev, int64_t ldr, "
             r"int32_t n_heads, float negative_slope, const uint16_t\* X_dev, int64_t ldx, int32_t d, ")
BF = torch.bfloat16


def test_header_declares_the_three_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"int {FORWARD}\({NODE_ARGS}int y_dtype, void\* Y_dev, int64_t ldy_row, int64_t ldy_hop, void\* stream\);", code)
    assert re.search(rf"int {STATS}\({NODE_ARGS}int y_dtype, void\* Y_dev, int64_t ldy_row, int64_t ldy_hop, float\* stats_dev, "
                     r"int64_t ldstats, void\* stream\);", code)
    assert re.search(rf"int {BACKWARD}\({NODE_ARGS}const float\* stats_dev, int64_t ldstats, const uint16_t\* Y_dev, int64_t ldy_row, "
                     r"int64_t ldy_hop, const uint16_t\* G_dev, int64_t ldg_row, int64_t ldg_hop, float\* delta_dev, int64_t lddelta, "
                     r"float\* dl_dev, int64_t lddl, float\* dr_dev, int64_t lddr, int dx_dtype, void\* dX_dev, int64_t lddx, "
                     r"void\* stream\);", code)


def test_header_states_the_contract_next_to_the_prototypes():
    at = HEADER.index(f"int {FORWARD}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("added within ABI 5", "h2gcn_spmm_hops_bf16", "WIDENED EXACTLY", "EVERY OPERATION OF THE FP32 KERNEL RUNS IN FP32 IN THE DOCUMENTED ORDER",
                   "ROUNDED ONCE, TO NEAREST EVEN, AT THE FINAL STORE", "bit-identical to the fp32 launch on the upcast operands",
                   "a bf16 output is that value rounded to nearest even", "l, r, stats, delta, dl and dr stay fp32", "K wide, not d wide",
                   "THE SUMMATION ORDERS are those of the fp32 launches", "dX is rounded once, after the sum over the hops",
                   "H2GCN_DTYPE_F32 or H2GCN_DTYPE_BF16", "in ELEMENTS",
                   "In the backward X, Y and G are all bf16: delta = <G, Y> is taken on the bf16 Y that the forward stored.",
                   "K <= 16", "d % K == 0", "(d / K) % 4 == 0", "the backward needs d <= 256", "the forward takes any even d",
                   "in their order and with their messages", "a 4-byte aligned base, even row / hop strides and an even d",
                   "a memset of the outputs in the element size of each", "hipGraph capture"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbols_and_the_unit_is_built():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (FORWARD, STATS, BACKWARD):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5
    makefile = (ROOT / "h2gcn_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()
    assert "attention_bf16.hip" in srcs
    assert (ROOT / "h2gcn_amd" / "csrc" / "attention_bf16.hip").is_file()


def test_capi_declares_the_prototypes():
    L, C = _capi.lib(), ctypes
    node = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int32]
    fn = getattr(L, FORWARD)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    fn = getattr(L, STATS)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    fn = getattr(L, BACKWARD)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                        C.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    quiet = lambda: L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1)     # noqa: E731 (a call that leaves the error channel alone)
    assert quiet() == 0
    assert L.h2gcn_attention_hops_heads_bf16(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, _capi.DTYPE_BF16, None, 8, 8,
                                             None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert quiet() == 0
    assert L.h2gcn_attention_hops_heads_stats_bf16(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, _capi.DTYPE_F32, None, 8, 8, None, 8,
                                                   None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert quiet() == 0
    assert L.h2gcn_attention_hops_heads_backward_bf16(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, None, 8, 8, None, 8, 8, None, 4,
                                                      None, 4, None, 4, _capi.DTYPE_BF16, None, 8, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures_and_the_pinned_ones():
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import (MultiHeadHopAttention, RecomputeMultiHeadHopAttention, hop_attention_heads, hop_attention_recompute,
                                  hop_attention_recompute_dropout)

    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = {
        HopPlan.attention_heads_bf16: ["self", "x", "l", "r", "negative_slope", "hops", "out", "out_dtype"],
        HopPlan.attention_heads_stats_bf16: ["self", "x", "l", "r", "negative_slope", "hops", "out", "out_dtype"],
        HopPlan.attention_heads_backward_bf16: ["self", "x", "l", "r", "stats", "y", "grad", "negative_slope", "hops", "need_dl", "need_dr",
                                                "need_dx", "dx_dtype"],
    }
    defaults = {"hops": None, "out": None, "out_dtype": None, "dx_dtype": None, "negative_slope": 0.2, "need_dl": True, "need_dr": True,
                "need_dx": True}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults:
                assert p[name].default == defaults[name], (fn, name)
            else:
                assert p[name].default is inspect.Parameter.empty, (fn, name)
    assert HopPlan.BF16_ATTENTION_SYMBOLS == (FORWARD, STATS, BACKWARD)
    # the existing methods and functions keep their pinned signatures
    assert list(inspect.signature(HopPlan.attention_heads).parameters) == ["self", "x", "l", "r", "negative_slope", "hops", "out"]
    assert list(inspect.signature(HopPlan.attention_heads_stats).parameters) == ["self", "x", "l", "r", "negative_slope", "hops", "out"]
    assert list(inspect.signature(HopPlan.attention_heads_backward).parameters) == [
        "self", "x", "l", "r", "stats", "y", "grad", "negative_slope", "hops", "need_dl", "need_dr", "need_dx"]
    assert list(inspect.signature(hop_attention_heads).parameters) == ["adjhops", "inputs", "l", "r", "negative_slope", "hops"]
    assert list(inspect.signature(hop_attention_recompute).parameters) == ["adjhops", "inputs", "l", "r", "negative_slope", "hops"]
    assert list(inspect.signature(hop_attention_recompute_dropout).parameters) == [
        "adjhops", "inputs", "l", "r", "dropout", "seed", "step", "negative_slope", "hops"]
    assert list(inspect.signature(RecomputeMultiHeadHopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    assert RecomputeMultiHeadHopAttention.__init__ is MultiHeadHopAttention.__init__


def test_plan_methods_refuse_without_a_device():
    plan = _stand_in_plan()
    x = torch.zeros(6, 8, dtype=BF)
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    stats, y, g = torch.zeros(4, 2, 2, 2), torch.zeros(4, 2, 8, dtype=BF), torch.zeros(4, 2, 8, dtype=BF)
    wide, rows = torch.zeros(6, 2 * 8 + 8, dtype=BF), torch.zeros(4, 2 * 2 + 2 * 8)
    fwd, sts, bwd = plan.attention_heads_bf16, plan.attention_heads_stats_bf16, plan.attention_heads_backward_bf16
    bad = []
    for f in (fwd, sts):
        bad += [
            ("inputs must be", lambda f=f: f(torch.zeros(6, dtype=BF), l, r)),
            ("inputs have 5 rows", lambda f=f: f(torch.zeros(5, 8, dtype=BF), l, r)),
            ("inputs must be bfloat16", lambda f=f: f(x.float(), l, r)),
            ("l must have shape", lambda f=f: f(x, torch.zeros(4, 2), r)),
            ("l must have shape", lambda f=f: f(x, l, r, hops=[1])),
            ("r must have shape", lambda f=f: f(x, l, torch.zeros(6, 2, 3))),
            ("must be float32", lambda f=f: f(x, l.to(BF), r.to(BF))),
            ("at most K = 16 heads, got K = 17", lambda f=f: f(torch.zeros(6, 68, dtype=BF), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17))),
            ("not a multiple of the number of heads", lambda f=f: f(x, torch.zeros(4, 2, 3), torch.zeros(6, 2, 3))),
            ("must be a multiple of 4", lambda f=f: f(x, torch.zeros(4, 2, 4), torch.zeros(6, 2, 4))),
            ("the feature width d must be even \\(got 7\\)", lambda f=f: f(torch.zeros(6, 7, dtype=BF), l[:, :, :1], r[:, :, :1])),
            ("row / hop strides must be even", lambda f=f: f(torch.zeros(6, 9, dtype=BF)[:, :8], l, r)),
            ("4-byte aligned", lambda f=f: f(torch.zeros(6 * 8 + 1, dtype=BF)[1:].view(6, 8), l, r)),
            ("outputs must be float32 or bfloat16", lambda f=f: f(x, l, r, out_dtype=torch.float16)),
            ("out has shape", lambda f=f: f(x, l, r, out=torch.zeros(4, 1, 8, dtype=BF))),
            ("out must be torch.float32", lambda f=f: f(x, l, r, out=torch.zeros(4, 2, 8, dtype=BF), out_dtype=torch.float32)),
            ("last dimension must be contiguous", lambda f=f: f(x, l, r, out=torch.zeros(4, 2, 16, dtype=BF)[:, :, ::2])),
            ("bf16 out: row / hop strides must be even", lambda f=f: f(x, l, r, out=torch.zeros(4, 2, 9, dtype=BF)[:, :, :8])),
            ("out overlaps the inputs", lambda f=f: f(wide[:, :8], l, r, out=wide[:4, 8:].view(4, 2, 8))),
            ("out overlaps l", lambda f=f: f(x, rows[:, :4].view(4, 2, 2), r, out=rows[:, 4:].view(4, 2, 8))),
        ]
    bad += [
        ("inputs must be bfloat16", lambda: bwd(x.float(), l, r, stats, y, g)),
        ("inputs have 5 rows", lambda: bwd(torch.zeros(5, 8, dtype=BF), l, r, stats, y, g)),
        ("l must have shape", lambda: bwd(x, torch.zeros(5, 2, 2), r, stats, y, g)),
        ("at most K = 16 heads, got K = 17", lambda: bwd(torch.zeros(6, 68, dtype=BF), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17), stats, y, g)),
        ("must be a multiple of 4", lambda: bwd(x, torch.zeros(4, 2, 4), torch.zeros(6, 2, 4), stats, y, g)),
        ("the feature width d must be even", lambda: bwd(torch.zeros(6, 7, dtype=BF), l[:, :, :1], r[:, :, :1], stats, y, g)),
        ("all False", lambda: bwd(x, l, r, stats, y, g, need_dl=False, need_dr=False, need_dx=False)),
        ("at most d = 256 columns, got d = 260", lambda: bwd(torch.zeros(6, 260, dtype=BF), l[:, :, :1], r[:, :, :1], stats, y, g)),
        ("dx must be float32 or bfloat16", lambda: bwd(x, l, r, stats, y, g, dx_dtype=torch.float16)),
        ("stats must be", lambda: bwd(x, l, r, torch.zeros(4, 2, 2), y, g)),
        ("stats must be float32", lambda: bwd(x, l, r, stats.to(BF), y, g)),
        ("y must be", lambda: bwd(x, l, r, stats, torch.zeros(4, 2, 4, dtype=BF), g)),
        ("y must be bfloat16", lambda: bwd(x, l, r, stats, y.float(), g)),
        ("grad must be", lambda: bwd(x, l, r, stats, y, torch.zeros(4, 1, 8, dtype=BF))),
        ("grad must be bfloat16", lambda: bwd(x, l, r, stats, y, g.float())),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()
    bare = _stand_in_plan()
    bare.has_transpose = bare.keep_permutation = False
    for needs in ({"need_dl": False, "need_dx": False}, {"need_dl": False, "need_dr": False}, {}):
        with pytest.raises(ValueError, match=r"build_transpose=True\)"):
            bare.attention_heads_backward_bf16(x, l, r, stats, y, g, **needs)
    # the existing methods keep their refusal of a bfloat16 x
    for call in (lambda: plan.attention_heads(x, l, r), lambda: plan.attention_heads_stats(x, l, r),
                 lambda: plan.attention_heads_backward(x, l, r, stats, y.float(), g.float())):
        with pytest.raises(ValueError, match="inputs must be float32"):
            call()


def test_what_bf16_does_not_cover_is_refused_never_run_in_float32(monkeypatch):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import (RecomputeMultiHeadHopAttention, hop_attention_heads, hop_attention_recompute,
                                  hop_attention_recompute_dropout)

    def forbidden(name):
        def fn(self, *args, **kwargs):
            raise AssertionError(f"{name} was launched")
        return fn

    for name in ("edge_scores_heads", "row_softmax_heads", "spmm_values", "attention_heads", "attention_heads_stats", "attention_heads_backward",
                 "attention_heads_stats_dropout", "attention_heads_backward_dropout", "attention_heads_bf16", "attention_heads_stats_bf16",
                 "attention_heads_backward_bf16"):
        monkeypatch.setattr(HopPlan, name, forbidden(name))
    plan = _stand_in_plan(n_rows=6)
    z = lambda *shape: torch.zeros(*shape)     # noqa: E731
    x, l, r = z(6, 8).to(BF), z(6, 2, 2), z(6, 2, 2)
    with pytest.raises(ValueError, match="at most K = 16 heads, got K = 17"):
        hop_attention_recompute(plan, z(6, 68).to(BF), z(6, 2, 17), z(6, 2, 17))
    with pytest.raises(ValueError, match="at most K = 16 heads, got K = 17"):
        hop_attention_heads(plan, z(6, 68).to(BF), z(6, 2, 17), z(6, 2, 17))
    with pytest.raises(ValueError, match="at most d = 256 columns, got d = 260"):
        hop_attention_recompute(plan, z(6, 260).to(BF), z(6, 2, 1).requires_grad_(), z(6, 2, 1))
    for fn in (hop_attention_recompute, hop_attention_heads):
        with pytest.raises(ValueError, match="needs an even width .* got d = 7"):
            fn(plan, z(6, 7).to(BF), z(6, 2, 1), z(6, 2, 1))
    with pytest.raises(ValueError, match=r"hop_attention_recompute_dropout\(dropout=0.5\) with bfloat16 inputs"):
        hop_attention_recompute_dropout(plan, x, l, r, 0.5)
    with pytest.raises(ValueError, match="hop_attention_heads with bfloat16 inputs that need a gradient.*hop_attention_recompute"):
        hop_attention_heads(plan, x, l.clone().requires_grad_(), r)
    layer = RecomputeMultiHeadHopAttention(8, 2).set_attention_dropout(0.5, seed=1)
    layer.train()
    with pytest.raises(ValueError, match=r"attn_dropout=0.5\) in train\(\) with bfloat16 inputs"):
        layer(plan, x)
    wide = RecomputeMultiHeadHopAttention(260, 1)
    with pytest.raises(ValueError, match="at most d = 256 columns, got d = 260"):
        wide(plan, z(6, 260).to(BF))
    many = RecomputeMultiHeadHopAttention(68, 17)
    with pytest.raises(ValueError, match="at most K = 16 heads, got K = 17"):
        many(plan, z(6, 68).to(BF))
    # a library without the three symbols
    for gone in (FORWARD, STATS, BACKWARD):
        monkeypatch.setattr(_capi, "has", lambda name, gone=gone: name != gone)
        for call in (lambda: hop_attention_recompute(plan, x, l, r), lambda: hop_attention_heads(plan, x, l, r),
                     lambda: hop_attention_recompute(plan, x, l.clone().requires_grad_(), r)):
            with pytest.raises(ValueError, match=f"predates the bf16 attention launches.*{gone}"):
                call()
    monkeypatch.undo()
    monkeypatch.setattr(_capi, "has", lambda name: name not in (FORWARD, STATS, BACKWARD))
    stats, y = z(6, 2, 2, 2), z(6, 2, 8).to(BF)
    for name, call in ((FORWARD, lambda: plan.attention_heads_bf16(x, l, r)), (STATS, lambda: plan.attention_heads_stats_bf16(x, l, r)),
                       (BACKWARD, lambda: plan.attention_heads_backward_bf16(x, l, r, stats, y, y))):
        with pytest.raises(ValueError, match=name):
            call()


def _recording(monkeypatch, n=6):
    """HopPlan with every launch the front end could reach replaced by a recorder; the links of the chain raise."""
    from h2gcn_amd import HopPlan

    calls = []

    def forbidden(name):
        def fn(self, *args, **kwargs):
            raise AssertionError(f"{name}: a link of the chain was launched")
        return fn

    for name in ("edge_scores_heads", "row_softmax_heads", "spmm_values"):
        monkeypatch.setattr(HopPlan, name, forbidden(name))

    def forward(name, dtype, with_stats):
        def fn(self, x, l, r, negative_slope=0.2, hops=None, out=None, **kwargs):
            calls.append((name, x.dtype, dict(kwargs)))
            y = torch.zeros(n, 2, x.shape[1], dtype=dtype)
            return (y, torch.zeros(n, 2, 2, l.shape[2])) if with_stats else y
        return fn

    def backward(name):
        def fn(self, x, l, r, stats, y, grad, negative_slope=0.2, hops=None, need_dl=True, need_dr=True, need_dx=True, **kwargs):
            calls.append((name, x.dtype, dict(kwargs, y=y.dtype, grad=grad.dtype, needs=(need_dl, need_dr, need_dx))))
            dx = torch.ones_like(x, dtype=kwargs.get("dx_dtype") or x.dtype) if need_dx else None
            return torch.ones_like(l) if need_dl else None, torch.ones_like(r) if need_dr else None, dx
        return fn

    monkeypatch.setattr(HopPlan, "attention_heads", forward("fused", torch.float32, False))
    monkeypatch.setattr(HopPlan, "attention_heads_stats", forward("stats", torch.float32, True))
    monkeypatch.setattr(HopPlan, "attention_heads_backward", backward("backward"))
    monkeypatch.setattr(HopPlan, "attention_heads_bf16", forward("fused_bf16", BF, False))
    monkeypatch.setattr(HopPlan, "attention_heads_stats_bf16", forward("stats_bf16", BF, True))
    monkeypatch.setattr(HopPlan, "attention_heads_backward_bf16", backward("backward_bf16"))
    return calls


def test_a_bf16_input_reaches_only_the_bf16_calls_and_a_float32_input_only_the_fp32_calls(monkeypatch):
    from h2gcn_amd.layers import RecomputeMultiHeadHopAttention, hop_attention_heads, hop_attention_recompute

    plan = _stand_in_plan(n_rows=6)
    calls = _recording(monkeypatch)
    x32, l, r = torch.zeros(6, 8), torch.zeros(6, 2, 2), torch.zeros(6, 2, 2)
    for dtype, names in ((BF, ["stats_bf16", "backward_bf16"]), (torch.float32, ["stats", "backward"])):
        for wanted in ((True, True, True), (False, True, False), (True, False, False), (False, False, True)):
            del calls[:]
            a, b, c = (t.clone().requires_grad_(w) for t, w in zip((x32.to(dtype), l, r), wanted))
            y = hop_attention_recompute(plan, a, b, c)
            assert y.requires_grad and y.dtype == dtype and [name for name, _, _ in calls] == names[:1]
            y.sum().backward()
            assert [name for name, _, _ in calls] == names and all(dt == dtype for _, dt, _ in calls)
            assert calls[1][2]["needs"] == (wanted[1], wanted[2], wanted[0])
            assert calls[1][2]["y"] == dtype and calls[1][2]["grad"] == dtype
            if dtype == BF:
                assert calls[1][2]["dx_dtype"] == BF
            for t, w in zip((a, b, c), wanted):
                assert (t.grad is not None) == w
                assert t.grad is None or t.grad.dtype == t.dtype
        # without a gradient: the one forward launch, from either function
        del calls[:]
        hop_attention_recompute(plan, x32.to(dtype), l, r)
        hop_attention_heads(plan, x32.to(dtype), l, r)
        with torch.no_grad():
            hop_attention_recompute(plan, x32.to(dtype).requires_grad_(), l, r)
        assert [name for name, _, _ in calls] == ["fused_bf16" if dtype == BF else "fused"] * 3
    # the layer: fp32 projections of the upcast head slices, then the bf16 calls; x.grad is bfloat16
    torch.manual_seed(0)
    layer = RecomputeMultiHeadHopAttention(8, 2)
    for dtype, names in ((BF, ["stats_bf16", "backward_bf16"]), (torch.float32, ["stats", "backward"])):
        del calls[:]
        layer.zero_grad()
        x = torch.ones(6, 8, dtype=dtype).requires_grad_()
        layer(plan, x).sum().backward()
        assert [name for name, _, _ in calls] == names
        assert x.grad.dtype == dtype and layer.a_l.grad.dtype == torch.float32 and layer.a_l.grad.abs().sum() > 0
    # a non-contiguous bf16 grad reaches the backward as bfloat16
    del calls[:]
    a = x32.to(BF).requires_grad_()
    y = hop_attention_recompute(plan, a, l, r)
    y.transpose(0, 1).contiguous().transpose(0, 1).sum().backward()
    assert calls[-1][0] == "backward_bf16" and calls[-1][2]["grad"] == BF
