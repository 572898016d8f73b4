"""CPU suite: attention training without per-entry arrays (h2gcn_attention_hops_heads_stats_f32 and
h2gcn_attention_hops_heads_backward_f32, added within ABI 5) -- both entry points are declared with their contract, bound and
exported consistently, refuse a NULL plan before any device work, and the front end has the new names
(HopPlan.attention_heads_stats / attention_heads_backward, hop_attention_recompute, RecomputeMultiHeadHopAttention), refuses what it
can without a GPU and reaches only the two new calls under a gradient."""
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
STATS = "h2gcn_attention_hops_heads_stats_f32"
BACKWARD = "h2gcn_attention_hops_heads_backward_f32"
NODE_ARGS = (r"const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* l_dev, int64_t ldl, const float\* r_dev, int64_t ldr, "
             r"int32_t n_heads, float negative_slope, const float\* X_dev, int64_t ldx, int32_t d, ")


def test_header_declares_both_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"int {STATS}\({NODE_ARGS}float\* Y_dev, int64_t ldy_row, int64_t ldy_hop, float\* stats_dev, int64_t ldstats, "
                     r"void\* stream\);", code)
    assert re.search(rf"int {BACKWARD}\({NODE_ARGS}const float\* stats_dev, int64_t ldstats, const float\* Y_dev, int64_t ldy_row, "
                     r"int64_t ldy_hop, const float\* G_dev, int64_t ldg_row, int64_t ldg_hop, float\* delta_dev, int64_t lddelta, "
                     r"float\* dl_dev, int64_t lddl, float\* dr_dev, int64_t lddr, float\* dX_dev, int64_t lddx, void\* stream\);", code)


def test_header_states_the_contract_next_to_the_prototypes():
    at = HEADER.index(f"int {STATS}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("added within ABI 5", "ALSO STORES THE SOFTMAX STATISTICS", "RECOMPUTING BACKWARD", "Nothing of size nnz is read, written or allocated",
                   "no workspace, no atomics", "all offsets 64-bit", "fp32 only", "[n_rows, H_sel, 2, K]", "ldstats >= H_sel*2*K",
                   "i*ldstats + s*2*K + h", "i*ldstats + s*2*K + K + h", "bit for bit", "an empty segment stores (+0, +0)",
                   "a stats that IS Y, X, l or r", "K <= 16", "dalpha[e,h] = sum_c G[i,s,c] * X[j,c]", "delta[i,s,h] = sum_c G[i,s,c] * Y[i,s,c]",
                   "dscore = alpha * (dalpha - delta)", "a NaN pre: the slope branch", "each optional", "at least one must be wanted",
                   "the ROW SIDE fills and the COLUMN SIDE reads", "THE COLUMN SIDE READS t_rowptr / t_colidx ONLY, never the permutation",
                   "without H2GCN_PLAN_KEEP_PERMUTATION is served", "a symmetric plan on its forward arrays", "H2GCN_ERR_NO_TRANSPOSE",
                   "K == 1 takes any d up to 256", "d % K == 0", "(d / K) % 4 == 0", "d > 256 is refused with a message naming the limit",
                   "DETERMINISTIC BUT NOT THE CHAIN'S BITS", "delta comes from <G, Y>", "THE SUMMATION ORDERS", "the SDDMM's order",
                   "the row-softmax tree over the WALKED segment", "256 partials P[t mod 256]", "(W_0 + W_1) + (W_2 + W_3)",
                   "the canonical aggregation tree", "P[jj & 3]", "(P0 + P1) + (P2 + P3)", "((T0 + T1) + T2) + T3", "ascending hop order",
                   "long_row_threshold, rows_per_wave", "hipGraph capture", "one eager warm-up", "a memset of the outputs", '"plan is NULL"',
                   "n_heads < 1", "n_heads > 16", "no output wanted", "a NULL delta when dr or dX is wanted",
                   "an output that IS an input or another output"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (STATS, BACKWARD):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5
    makefile = (ROOT / "h2gcn_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()
    assert "attention_backward.hip" in srcs and "attention_fused.hip" in srcs


def test_capi_declares_the_prototypes():
    L, C = _capi.lib(), ctypes
    node = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int32]
    fn = getattr(L, STATS)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    fn = getattr(L, BACKWARD)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == node + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
    assert L.h2gcn_attention_hops_heads_stats_f32(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, 8, None, 8,
                                                  None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()
    assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0
    assert L.h2gcn_attention_hops_heads_backward_f32(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, None, 8, 8, None, 8, 8, None, 4,
                                                     None, 4, None, 4, None, 8, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import (HopAttention, MultiHeadHopAttention, RecomputeMultiHeadHopAttention, hop_attention_heads,
                                  hop_attention_recompute)

    assert h2gcn_amd.hop_attention_recompute is hop_attention_recompute
    assert h2gcn_amd.RecomputeMultiHeadHopAttention is RecomputeMultiHeadHopAttention
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = {
        hop_attention_recompute: ["adjhops", "inputs", "l", "r", "negative_slope", "hops"],
        HopPlan.attention_heads_stats: ["self", "x", "l", "r", "negative_slope", "hops", "out"],
        HopPlan.attention_heads_backward: ["self", "x", "l", "r", "stats", "y", "grad", "negative_slope", "hops", "need_dl", "need_dr",
                                           "need_dx"],
    }
    defaults = {"hops": None, "out": None, "negative_slope": 0.2, "need_dl": True, "need_dr": True, "need_dx": True}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults:
                assert p[name].default == defaults[name], (fn, name)
            else:
                assert p[name].default is inspect.Parameter.empty, (fn, name)
    assert HopPlan.ATTENTION_FUSED_MAX_HEADS == 16 and HopPlan.ATTENTION_RECOMPUTE_MAX_WIDTH == 256
    # the new layer is the old one with another forward: the same constructor, parameters and state_dict
    assert issubclass(RecomputeMultiHeadHopAttention, MultiHeadHopAttention)
    assert RecomputeMultiHeadHopAttention.__init__ is MultiHeadHopAttention.__init__
    torch.manual_seed(0)
    old, new = MultiHeadHopAttention(32, 8), RecomputeMultiHeadHopAttention(32, 8)
    assert list(old.state_dict()) == list(new.state_dict()) == ["a_l", "a_r"]
    new.load_state_dict(old.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(old.parameters(), new.parameters()))
    # the old layers and functions keep their pinned signatures
    assert list(inspect.signature(MultiHeadHopAttention.__init__).parameters) == ["self", "in_dim", "heads", "hops", "n_hops", "negative_slope"]
    assert list(inspect.signature(MultiHeadHopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    assert list(inspect.signature(RecomputeMultiHeadHopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    assert list(inspect.signature(HopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    assert list(inspect.signature(hop_attention_heads).parameters) == ["adjhops", "inputs", "l", "r", "negative_slope", "hops"]
    assert list(inspect.signature(HopPlan.attention_heads).parameters) == ["self", "x", "l", "r", "negative_slope", "hops", "out"]
    doc = re.sub(r"\s+", " ", hop_attention_recompute.__doc__)
    assert "K > 16" in doc and "d > 256" in doc and "predates the two launches" in doc and "the chain" in doc and "build_transpose=True" in doc


def test_python_side_refusals_need_no_device():
    plan = _stand_in_plan()
    x = torch.zeros(6, 8)
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    out = torch.zeros(4, 2, 8)
    stats, y, g = torch.zeros(4, 2, 2, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8)
    bf = torch.bfloat16
    wide, rows = torch.zeros(6, 2 * 8 + 8), torch.zeros(4, 2 * 2 + 2 * 8)
    fwd, bwd = plan.attention_heads_stats, plan.attention_heads_backward
    bad = [
        ("inputs must be", lambda: fwd(torch.zeros(6), l, r)),
        ("inputs have 5 rows", lambda: fwd(torch.zeros(5, 8), l, r)),
        ("inputs must be float32", lambda: fwd(x.to(bf), l, r)),
        ("l must have shape", lambda: fwd(x, torch.zeros(4, 2), r)),
        ("l must have shape", lambda: fwd(x, l, r, hops=[1])),
        ("r must have shape", lambda: fwd(x, l, torch.zeros(6, 2, 3))),
        ("must be float32", lambda: fwd(x, l.to(bf), r.to(bf))),
        ("must be a tensor", lambda: fwd(x, None, r)),
        ("at most K = 16 heads, got K = 17", lambda: fwd(torch.zeros(6, 68), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17))),
        ("not a multiple of the number of heads", lambda: fwd(x, torch.zeros(4, 2, 3), torch.zeros(6, 2, 3))),
        ("must be a multiple of 4", lambda: fwd(x, torch.zeros(4, 2, 4), torch.zeros(6, 2, 4))),
        ("out has shape", lambda: fwd(x, l, r, out=torch.zeros(4, 1, 8))),
        ("out must be float32", lambda: fwd(x, l, r, out=out.double())),
        ("last dimension must be contiguous", lambda: fwd(x, l, r, out=torch.zeros(4, 2, 16)[:, :, ::2])),
        ("out overlaps the inputs", lambda: fwd(wide[:, :8], l, r, out=wide[:4, 8:].view(4, 2, 8))),
        ("out overlaps l", lambda: fwd(x, rows[:, :4].view(4, 2, 2), r, out=rows[:, 4:].view(4, 2, 8))),
        ("out overlaps r", lambda: fwd(x, l, wide[:, 8:12].view(6, 2, 2), out=wide[:4, 8:].view(4, 2, 8))),
        ("inputs must be float32", lambda: bwd(x.to(bf), l, r, stats, y, g)),
        ("inputs have 5 rows", lambda: bwd(torch.zeros(5, 8), l, r, stats, y, g)),
        ("l must have shape", lambda: bwd(x, torch.zeros(5, 2, 2), r, stats, y, g)),
        ("r must have shape", lambda: bwd(x, l, torch.zeros(4, 2, 2), stats, y, g)),
        ("at most K = 16 heads, got K = 17", lambda: bwd(torch.zeros(6, 68), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17), stats, y, g)),
        ("must be a multiple of 4", lambda: bwd(x, torch.zeros(4, 2, 4), torch.zeros(6, 2, 4), stats, y, g)),
        ("all False", lambda: bwd(x, l, r, stats, y, g, need_dl=False, need_dr=False, need_dx=False)),
        ("at most d = 256 columns, got d = 260", lambda: bwd(torch.zeros(6, 260), l[:, :, :1], r[:, :, :1], stats, y, g)),
        ("stats must be", lambda: bwd(x, l, r, torch.zeros(4, 2, 2), y, g)),
        ("stats must be float32", lambda: bwd(x, l, r, stats.double(), y, g)),
        ("y must be", lambda: bwd(x, l, r, stats, torch.zeros(4, 2, 4), g)),
        ("grad must be", lambda: bwd(x, l, r, stats, y, torch.zeros(4, 1, 8))),
        ("grad must be float32", lambda: bwd(x, l, r, stats, y, g.to(bf))),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()
    bare = _stand_in_plan()
    bare.has_transpose = bare.keep_permutation = False
    for needs in ({"need_dl": False, "need_dx": False}, {"need_dl": False, "need_dr": False}, {}):
        with pytest.raises(ValueError, match=r"build_transpose=True\)"):
            bare.attention_heads_backward(x, l, r, stats, y, g, **needs)


def test_a_row_partitioned_operand_is_refused_before_any_device_work():
    from h2gcn_amd.layers import RecomputeMultiHeadHopAttention, hop_attention_recompute

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="hop_attention_recompute is not supported on row-partitioned operands \\(ShardedHops\\)"):
        hop_attention_recompute(Sharded(), None, None, None)
    with pytest.raises(TypeError, match="HopPlan"):
        hop_attention_recompute(object(), None, None, None)
    layer = RecomputeMultiHeadHopAttention(8, 2)
    with pytest.raises(ValueError, match="RecomputeMultiHeadHopAttention is not supported on row-partitioned operands \\(ShardedHops\\)"):
        layer(Sharded(), torch.zeros(6, 8))
    with pytest.raises(TypeError, match="HopPlan"):
        layer(object(), torch.zeros(6, 8))


def _recording(monkeypatch, n=6):
    """HopPlan with every launch the front end could reach replaced by a recorder; the links of the chain raise."""
    from h2gcn_amd import HopPlan

    calls = []

    def link(name, result):
        def fn(self, *args, **kwargs):
            calls.append((name, kwargs))
            return result() if callable(result) else result
        return fn

    def forbidden(name):
        def fn(self, *args, **kwargs):
            raise AssertionError(f"{name}: a link of the chain was launched")
        return fn

    for name in ("edge_scores_heads", "row_softmax_heads", "spmm_values"):
        monkeypatch.setattr(HopPlan, name, forbidden(name))
    monkeypatch.setattr(HopPlan, "attention_heads", link("fused", torch.zeros(n, 2, 8)))
    monkeypatch.setattr(HopPlan, "attention_heads_stats", link("stats", lambda: (torch.zeros(n, 2, 8), torch.zeros(n, 2, 2, 2))))

    def backward(self, x, l, r, stats, y, grad, negative_slope=0.2, hops=None, need_dl=True, need_dr=True, need_dx=True):
        calls.append(("backward", {"need_dl": need_dl, "need_dr": need_dr, "need_dx": need_dx}))
        return (torch.ones_like(l) if need_dl else None, torch.ones_like(r) if need_dr else None, torch.ones_like(x) if need_dx else None)

    monkeypatch.setattr(HopPlan, "attention_heads_backward", backward)
    return calls


def test_under_a_gradient_only_the_two_new_calls_are_reached(monkeypatch):
    from h2gcn_amd.layers import hop_attention_recompute

    plan = _stand_in_plan(n_rows=6)
    calls = _recording(monkeypatch)
    x, l, r = torch.zeros(6, 8), torch.zeros(6, 2, 2), torch.zeros(6, 2, 2)
    for wanted in ((True, True, True), (False, True, False), (True, False, False), (False, False, True)):
        del calls[:]
        a, b, c = (t.clone().requires_grad_(w) for t, w in zip((x, l, r), wanted))
        y = hop_attention_recompute(plan, a, b, c)
        assert y.requires_grad and [name for name, _ in calls] == ["stats"]
        y.sum().backward()
        assert [name for name, _ in calls] == ["stats", "backward"]
        assert calls[1][1] == {"need_dx": wanted[0], "need_dl": wanted[1], "need_dr": wanted[2]}
        for t, w in zip((a, b, c), wanted):
            assert (t.grad is not None) == w
    # without a gradient: the one forward launch
    del calls[:]
    hop_attention_recompute(plan, x, l, r)
    with torch.no_grad():
        hop_attention_recompute(plan, x.clone().requires_grad_(), l, r)
    assert [name for name, _ in calls] == ["fused", "fused"]


def test_a_plan_without_transposes_is_told_what_to_build(monkeypatch):
    from h2gcn_amd.layers import hop_attention_recompute

    plan = _stand_in_plan(n_rows=6)
    plan.has_transpose = plan.keep_permutation = False
    calls = _recording(monkeypatch)
    x, l, r = torch.zeros(6, 8), torch.zeros(6, 2, 2), torch.zeros(6, 2, 2)
    for wanted in ((True, False, False), (False, False, True)):
        a, b, c = (t.clone().requires_grad_(w) for t, w in zip((x, l, r), wanted))
        with pytest.raises(ValueError, match=r"Build the plan with HopPlan\(\.\.\., build_transpose=True\)"):
            hop_attention_recompute(plan, a, b, c)
    assert calls == []
    y = hop_attention_recompute(plan, x, l.clone().requires_grad_(), r)               # dl alone needs no transposes
    y.sum().backward()
    assert [name for name, _ in calls] == ["stats", "backward"]


def test_an_old_library_many_heads_or_a_wide_input_take_the_chain(monkeypatch):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_attention_recompute

    plan = _stand_in_plan(n_rows=6)
    x, l, r = torch.zeros(6, 8), torch.zeros(6, 2, 2), torch.zeros(6, 2, 2)
    monkeypatch.setattr(_capi, "has", lambda name: name not in (STATS, BACKWARD))
    for name, call in ((STATS, lambda: plan.attention_heads_stats(x, l, r)),
                       (BACKWARD, lambda: plan.attention_heads_backward(x, l, r, torch.zeros(6, 2, 2, 2), torch.zeros(6, 2, 8), torch.zeros(6, 2, 8)))):
        with pytest.raises(RuntimeError, match=name):
            call()
    calls = []

    def link(name, result):
        def fn(self, *args, **kwargs):
            calls.append(name)
            return result
        return fn

    monkeypatch.setattr(HopPlan, "edge_scores_heads", link("scores", [torch.zeros(5, 2), torch.zeros(3, 2)]))
    monkeypatch.setattr(HopPlan, "row_softmax_heads", link("softmax", [torch.zeros(5, 2), torch.zeros(3, 2)]))
    monkeypatch.setattr(HopPlan, "spmm_values", link("spmm", torch.zeros(6, 2, 8)))
    monkeypatch.setattr(HopPlan, "attention_heads", link("fused", torch.zeros(6, 2, 8)))
    monkeypatch.setattr(HopPlan, "attention_heads_stats", link("stats", None))
    with torch.no_grad():
        hop_attention_recompute(plan, x, l, r)                                        # an old library that has the fused forward
    assert calls == ["fused"]
    del calls[:]
    monkeypatch.setattr(_capi, "has", lambda name: name not in (STATS, BACKWARD, "h2gcn_attention_hops_heads_f32"))
    hop_attention_recompute(plan, x, l, r)
    assert calls == ["scores", "softmax", "spmm"]
    monkeypatch.setattr(_capi, "has", lambda name: True)
    for shape in (((6, 68), 17), ((6, 260), 1)):                                      # K > 16, d > 256
        del calls[:]
        with torch.no_grad():
            hop_attention_recompute(plan, torch.zeros(shape[0]), torch.zeros(6, 2, shape[1]), torch.zeros(6, 2, shape[1]))
        assert calls in (["scores", "softmax", "spmm"], ["fused"]) and "stats" not in calls
    del calls[:]
    hop_attention_recompute(plan, torch.zeros(6, 68), torch.zeros(6, 2, 17), torch.zeros(6, 2, 17))
    assert calls == ["scores", "softmax", "spmm"]
