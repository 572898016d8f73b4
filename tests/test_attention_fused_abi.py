"""CPU suite: the fused attention forward (h2gcn_attention_hops_heads_f32, added within ABI 5) -- the entry point is declared
with its contract, bound and exported consistently, refuses a NULL plan before any device work, and the front end has the new
names (HopPlan.attention_heads, hop_attention_heads) and refuses what it can without a GPU."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
FUSED = "h2gcn_attention_hops_heads_f32"


def test_header_declares_the_entry_point_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    proto = (rf"int {FUSED}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, const float\* l_dev, int64_t ldl, const float\* r_dev, "
             r"int64_t ldr, int32_t n_heads, float negative_slope, const float\* X_dev, int64_t ldx, int32_t d, float\* Y_dev, "
             r"int64_t ldy_row, int64_t ldy_hop, void\* stream\);")
    assert re.search(proto, code)


def test_header_states_the_contract_next_to_the_prototype():
    at = HEADER.index(f"int {FUSED}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("added within ABI 5", "ONE launch", "i*ldl + s*K + h", "ldl >= H_sel*K", "ldy_row / ldy_hop",
                   "K == 1 takes any d", "d % K == 0", "(d / K) % 4 == 0", "K <= 16 is served", "naming the limit",
                   "reads only rowptr / colidx", "n_rows != n_cols is legal", "stored values are never read",
                   "No workspace, no atomics, no allocation", "all offsets 64-bit", "fp32 only", "an empty segment stores +0",
                   "Forward only", "THE CONTRACT IS THE CHAIN'S BITS", "h2gcn_edge_scores_hops_heads_f32",
                   "h2gcn_row_softmax_hops_heads_f32", "h2gcn_spmm_hops_values_f32", "ldv_entry = K, ldv_head = 1",
                   "one fp32 addition", "a NaN pre takes the slope branch", "the one hardware exponential",
                   "256 partials P[j mod 256]", "S = (W_0 + W_1) + (W_2 + W_3)", "one correctly rounded 1/S per segment",
                   "alpha_j = e_j * (1/S)", "defined on the partial's index", "a segment of -inf only is NaN throughout",
                   "gives exactly +0", "a head that holds a NaN never changes a bit of another head", "P[jj & 3]",
                   "(P0 + P1) + (P2 + P3)", "((T0 + T1) + T2) + T3", "long_row_threshold, rows_per_wave", "hipGraph capture",
                   "a memset of the output", '"plan is NULL"', "n_heads < 1", "n_heads > 16", "a Y that IS X, l or r"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbol():
    lib = ctypes.CDLL(str(_capi.library_path()))
    assert FUSED in _capi.EXPORTED_SYMBOLS
    assert hasattr(lib, FUSED)
    assert _capi.has(FUSED)
    assert _capi.lib().h2gcn_abi_version() == 5
    makefile = (ROOT / "h2gcn_amd" / "csrc" / "Makefile").read_text()
    assert "attention_fused.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()


def test_capi_declares_the_prototype():
    L, C = _capi.lib(), ctypes
    fn = getattr(L, FUSED)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                 C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
    assert L.h2gcn_attention_hops_heads_f32(None, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, 8, None) == _capi.ERR_INVALID_ARGUMENT
    assert b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import HopAttention, MultiHeadHopAttention, hop_attention_heads

    assert h2gcn_amd.hop_attention_heads is hop_attention_heads
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    want = {
        hop_attention_heads: ["adjhops", "inputs", "l", "r", "negative_slope", "hops"],
        HopPlan.attention_heads: ["self", "x", "l", "r", "negative_slope", "hops", "out"],
    }
    defaults = {"hops": None, "out": None, "negative_slope": 0.2}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults:
                assert p[name].default == defaults[name], (fn, name)
            else:
                assert p[name].default is inspect.Parameter.empty, (fn, name)
    assert HopPlan.ATTENTION_FUSED_MAX_HEADS == 16
    # the layers keep their pinned signatures
    assert list(inspect.signature(MultiHeadHopAttention.__init__).parameters) == ["self", "in_dim", "heads", "hops", "n_hops", "negative_slope"]
    assert list(inspect.signature(MultiHeadHopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    assert list(inspect.signature(HopAttention.forward).parameters) == ["self", "adjhops", "inputs"]
    # the docstring says which calls take the chain
    doc = re.sub(r"\s+", " ", hop_attention_heads.__doc__)
    assert "K > 16" in doc and "predates the launch" in doc and "take the chain" in doc


def _stand_in_plan(nnz=(5, 3), n_rows=4, n_cols=6):
    """A HopPlan that never reached the library: what the argument checks read, on the CPU.  Any launch on it would fail, so a
    test that passes has been refused before the library was called."""
    from h2gcn_amd import HopPlan

    plan = object.__new__(HopPlan)
    plan._handle = None
    plan.n_hops, plan.n_rows, plan.n_cols = len(nnz), n_rows, n_cols
    plan.device = torch.device("cpu")
    plan.colidx = [torch.zeros(n, dtype=torch.int32) for n in nnz]
    plan.has_transpose, plan.keep_permutation = True, True
    return plan


def test_python_side_refusals_need_no_device():
    plan = _stand_in_plan()
    x = torch.zeros(6, 8)
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    out = torch.zeros(4, 2, 8)
    bf = torch.bfloat16
    wide, rows = torch.zeros(6, 2 * 8 + 8), torch.zeros(4, 2 * 2 + 2 * 8)
    bad = [
        ("inputs must be", lambda: plan.attention_heads(torch.zeros(6), l, r)),
        ("inputs have 5 rows", lambda: plan.attention_heads(torch.zeros(5, 8), l, r)),
        ("inputs must be float32", lambda: plan.attention_heads(x.to(bf), l, r)),
        ("inputs must be float32", lambda: plan.attention_heads(x.double(), l, r)),
        ("l must have shape", lambda: plan.attention_heads(x, torch.zeros(4, 2), r)),
        ("l must have shape", lambda: plan.attention_heads(x, torch.zeros(5, 2, 2), r)),
        ("l must have shape", lambda: plan.attention_heads(x, l, r, hops=[1])),
        ("r must have shape", lambda: plan.attention_heads(x, l, torch.zeros(6, 2, 3))),
        ("r must have shape", lambda: plan.attention_heads(x, l, torch.zeros(4, 2, 2))),
        ("must be float32", lambda: plan.attention_heads(x, l.to(bf), r.to(bf))),
        ("must be a tensor", lambda: plan.attention_heads(x, None, r)),
        ("at most K = 16 heads, got K = 17", lambda: plan.attention_heads(torch.zeros(6, 68), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17))),
        ("not a multiple of the number of heads", lambda: plan.attention_heads(x, torch.zeros(4, 2, 3), torch.zeros(6, 2, 3))),
        ("must be a multiple of 4", lambda: plan.attention_heads(x, torch.zeros(4, 2, 4), torch.zeros(6, 2, 4))),
        ("out has shape", lambda: plan.attention_heads(x, l, r, out=torch.zeros(4, 1, 8))),
        ("out must be float32", lambda: plan.attention_heads(x, l, r, out=out.double())),
        ("last dimension must be contiguous", lambda: plan.attention_heads(x, l, r, out=torch.zeros(4, 2, 16)[:, :, ::2])),
        ("rows / hop slots overlap", lambda: plan.attention_heads(x, l, r, out=torch.zeros(4, 1, 8).expand(4, 2, 8))),
        ("out overlaps the inputs", lambda: plan.attention_heads(wide[:, :8], l, r, out=wide[:4, 8:].view(4, 2, 8))),
        ("out overlaps l", lambda: plan.attention_heads(x, rows[:, :4].view(4, 2, 2), r, out=rows[:, 4:].view(4, 2, 8))),
        ("out overlaps r", lambda: plan.attention_heads(x, l, wide[:, 8:12].view(6, 2, 2), out=wide[:4, 8:].view(4, 2, 8))),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_a_row_partitioned_operand_is_refused_before_any_device_work():
    from h2gcn_amd.layers import hop_attention_heads

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="hop_attention_heads is not supported on row-partitioned"):
        hop_attention_heads(Sharded(), None, None, None)
    with pytest.raises(TypeError, match="HopPlan"):
        hop_attention_heads(object(), None, None, None)


def test_a_library_without_the_symbol_is_named_and_the_front_end_takes_the_chain(monkeypatch):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_attention_heads

    plan = _stand_in_plan()
    x, l, r = torch.zeros(6, 8), torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    monkeypatch.setattr(_capi, "has", lambda name: name != FUSED)
    with pytest.raises(RuntimeError, match=FUSED):
        plan.attention_heads(x, l, r)
    # hop_attention_heads: the chain, not the launch, on such a library -- and for K > 16 and when a gradient is wanted
    calls = []

    def link(name, result):
        def fn(self, *args, **kwargs):
            calls.append(name)
            return result
        return fn

    monkeypatch.setattr(HopPlan, "edge_scores_heads", link("scores", [torch.zeros(5, 2), torch.zeros(3, 2)]))
    monkeypatch.setattr(HopPlan, "row_softmax_heads", link("softmax", [torch.zeros(5, 2), torch.zeros(3, 2)]))
    monkeypatch.setattr(HopPlan, "spmm_values", link("spmm", torch.zeros(4, 2, 8)))
    monkeypatch.setattr(HopPlan, "attention_heads", link("fused", torch.zeros(4, 2, 8)))
    hop_attention_heads(plan, x, l, r)
    assert calls == ["scores", "softmax", "spmm"]
    monkeypatch.setattr(_capi, "has", lambda name: True)
    del calls[:]
    hop_attention_heads(plan, x, l, r)
    assert calls == ["fused"]
    del calls[:]
    with torch.no_grad():
        hop_attention_heads(plan, x.clone().requires_grad_(), l, r)
    assert calls == ["fused"]
    del calls[:]
    hop_attention_heads(plan, torch.zeros(6, 68), torch.zeros(4, 2, 17), torch.zeros(6, 2, 17))
    assert calls == ["scores", "softmax", "spmm"]
