"""CPU suite: attention dropout drawn in the kernels (h2gcn_attention_hops_heads_stats_dropout_f32,
h2gcn_attention_hops_heads_backward_dropout_f32 and h2gcn_attention_dropout_factors_hops_f32, added within ABI 5) -- the entry
points are declared with the generator and their contract, bound and exported consistently, refuse a bad keep_prob and a NULL plan
before any device work, and the front end has the new names next to the unchanged ones, refuses what it can without a GPU and makes
today's calls without dropout."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from h2gcn_amd import _capi
from test_attention_fused_abi import _stand_in_plan
from test_attention_recompute_abi import NODE_ARGS, _recording

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "h2gcn_hip.h").read_text()
STATS = "h2gcn_attention_hops_heads_stats_dropout_f32"
BACKWARD = "h2gcn_attention_hops_heads_backward_dropout_f32"
FACTORS = "h2gcn_attention_dropout_factors_hops_f32"
MASK_ARGS = r"float keep_prob, uint64_t seed, const int64_t\* step_dev, "


def test_header_declares_the_entry_points_within_abi_5():
    assert int(re.search(r"#define H2GCN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 5
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(rf"int {STATS}\({NODE_ARGS}float\* Y_dev, int64_t ldy_row, int64_t ldy_hop, float\* stats_dev, int64_t ldstats, "
                     rf"{MASK_ARGS}void\* stream\);", code)
    assert re.search(rf"int {BACKWARD}\({NODE_ARGS}const float\* stats_dev, int64_t ldstats, const float\* Y_dev, int64_t ldy_row, "
                     r"int64_t ldy_hop, const float\* G_dev, int64_t ldg_row, int64_t ldg_hop, float\* delta_dev, int64_t lddelta, "
                     rf"float\* dl_dev, int64_t lddl, float\* dr_dev, int64_t lddr, float\* dX_dev, int64_t lddx, {MASK_ARGS}void\* stream\);",
                     code)
    assert re.search(rf"int {FACTORS}\(const h2gcn_plan_t\* plan, uint32_t hop_mask, int32_t n_heads, {MASK_ARGS}"
                     r"float\* const\* f_dev, const int64_t\* ldf_entry, void\* stream\);", code)


def test_header_states_the_generator_and_where_the_factor_enters():
    at = HEADER.index(f"int {STATS}(")
    comment = re.sub(r"\s*\n \*\s*", " ", HEADER[HEADER.rindex("/*", 0, at):at])
    for phrase in ("Added within ABI 5", "DRAWN IN THE KERNELS", "nothing of size nnz holds it", "THE GENERATOR",
                   "a pure function of (seed, step, k, i, j, h)", "the PLAN's hop index", "It does not depend on the entry's position in colidx or t_colidx",
                   "long_row_threshold or rows_per_wave", "which hops are selected", "a symmetric plan's forward arrays",
                   "x *= 0x7FEB352D", "x *= 0x846CA68B", "0x9E3779B9", "0x85EBCA6B", "step = step_dev ? *step_dev : 0",
                   "gid = ((uint64(i) * n_cols + j) * n_hops_of_plan + k) * 8 + (h >> 1)", "one word per PAIR of heads",
                   "rot16(hi32(gid))", "field = (w >> 16 * (h & 1)) & 0xFFFF", "kept iff field < thr", "thr = floor(keep_prob * 65536)",
                   "inv_keep = 1.f / keep_prob, one fp32 division on the host", "WHERE f ENTERS", "ONE fp32 multiply",
                   "A dropped entry STILL multiplies", "stats are those of the launch without dropout, bit for bit",
                   "dalpha[e,h] = f[e,h] * <G[i,s], X[j]>_h", "delta = <G, Y>_h unchanged", "the UNDROPPED alpha",
                   "dX[j,c] += (alpha * f) * G[i,s,c]", "K <= 16; backward d <= 256", "keep_prob == 1 dispatches to the launches without dropout",
                   "keep_prob outside (0, 1] (NaN included) is refused FIRST", "all before the device is touched", "hipGraph capture",
                   "draws a fresh mask", "f_dev[s][e * ldf_entry[s] + h]", "reads rowptr / colidx only", "ldf_entry[s] < n_heads"):
        assert phrase in comment, phrase


def test_built_library_exports_the_symbols():
    lib = ctypes.CDLL(str(_capi.library_path()))
    for name in (STATS, BACKWARD, FACTORS):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert _capi.has(name)
    assert _capi.lib().h2gcn_abi_version() == 5
    makefile = (ROOT / "h2gcn_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=\s*(.*)$", makefile, flags=re.M).group(1).split()
    assert "attention_dropout.hip" in srcs and "attention_dropout_backward.hip" in srcs
    assert "attention_dropout.hip.h" in hdrs and "attention_backward.hip.h" in hdrs


def test_capi_declares_the_prototypes():
    L, C = _capi.lib(), ctypes
    mask = [C.c_float, C.c_uint64, C.c_void_p]
    for new, old in ((STATS, "h2gcn_attention_hops_heads_stats_f32"), (BACKWARD, "h2gcn_attention_hops_heads_backward_f32")):
        fn = getattr(L, new)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == list(getattr(L, old).argtypes)[:-1] + mask + [C.c_void_p]
    fn = getattr(L, FACTORS)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32, C.c_int32] + mask + [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]


def _stats(plan, keep):
    return _capi.lib().h2gcn_attention_hops_heads_stats_dropout_f32(plan, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, 8, None, 8,
                                                                    keep, 1, None, None)


def _backward(plan, keep):
    return _capi.lib().h2gcn_attention_hops_heads_backward_dropout_f32(plan, 0, None, 2, None, 2, 2, 0.2, None, 8, 8, None, 8, None, 8, 8, None,
                                                                       8, 8, None, 4, None, 4, None, 4, None, 8, keep, 1, None, None)


def _factors(plan, keep, n_heads=2):
    return _capi.lib().h2gcn_attention_dropout_factors_hops_f32(plan, 0, n_heads, keep, 1, None, None, None, None)


@pytest.mark.parametrize("keep", (0.0, -0.5, 1.5, float("nan"), float("inf")))
def test_a_bad_keep_prob_is_refused_first_and_without_a_device(keep):
    L = _capi.lib()
    for call in (_stats, _backward):
        assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0     # (any call that leaves the error channel alone)
        assert call(None, keep) == _capi.ERR_INVALID_ARGUMENT
        msg = L.h2gcn_last_error()
        assert b"keep_prob = " in msg and b"outside (0, 1]" in msg and b"plan" not in msg


def test_null_plan_is_refused_without_a_device():
    L = _capi.lib()
    for keep in (0.5, 1.0):                                                     # (1.0: the dispatch to the launch without dropout)
        for call in (_stats, _backward, _factors):
            assert L.h2gcn_spmm_workspace_bytes(None, 0, 0, None, 1, 0, 1) == 0
            assert call(None, keep) == _capi.ERR_INVALID_ARGUMENT
            assert b"plan is NULL" in L.h2gcn_last_error()
    # the factors: the plan comes first, as in every pattern launch
    assert _factors(None, float("nan")) == _capi.ERR_INVALID_ARGUMENT and b"plan is NULL" in L.h2gcn_last_error()


def test_front_end_signatures_and_defaults():
    import h2gcn_amd
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import MultiHeadHopAttention, RecomputeMultiHeadHopAttention, hop_attention_recompute, hop_attention_recompute_dropout

    assert h2gcn_amd.hop_attention_recompute_dropout is hop_attention_recompute_dropout
    kw = inspect.Parameter.POSITIONAL_OR_KEYWORD
    empty = inspect.Parameter.empty
    want = {
        HopPlan.attention_dropout_factors: ["self", "n_heads", "keep_prob", "seed", "step", "hops"],
        HopPlan.attention_heads_stats_dropout: ["self", "x", "l", "r", "keep_prob", "seed", "step", "negative_slope", "hops", "out"],
        HopPlan.attention_heads_backward_dropout: ["self", "x", "l", "r", "stats", "y", "grad", "keep_prob", "seed", "step", "negative_slope",
                                                   "hops", "need_dl", "need_dr", "need_dx"],
        hop_attention_recompute_dropout: ["adjhops", "inputs", "l", "r", "dropout", "seed", "step", "negative_slope", "hops"],
        MultiHeadHopAttention.set_attention_dropout: ["self", "attn_dropout", "seed"],
    }
    defaults = {"step": None, "hops": None, "out": None, "negative_slope": 0.2, "need_dl": True, "need_dr": True, "need_dx": True}
    for fn, names in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == names and all(v.kind is kw for v in p.values()), fn
        for name in names:
            if name in defaults:
                assert p[name].default == defaults[name], (fn, name)
    assert inspect.signature(hop_attention_recompute_dropout).parameters["dropout"].default is empty
    assert inspect.signature(hop_attention_recompute_dropout).parameters["seed"].default == 0
    assert inspect.signature(MultiHeadHopAttention.set_attention_dropout).parameters["seed"].default is None
    assert inspect.signature(HopPlan.attention_heads_stats_dropout).parameters["keep_prob"].default is empty
    # what exists keeps its signature: dropout has names of its own
    assert list(inspect.signature(hop_attention_recompute).parameters) == ["adjhops", "inputs", "l", "r", "negative_slope", "hops"]
    assert list(inspect.signature(HopPlan.attention_heads_stats).parameters) == ["self", "x", "l", "r", "negative_slope", "hops", "out"]
    assert list(inspect.signature(MultiHeadHopAttention.__init__).parameters) == ["self", "in_dim", "heads", "hops", "n_hops", "negative_slope"]
    assert RecomputeMultiHeadHopAttention.__init__ is MultiHeadHopAttention.__init__
    assert RecomputeMultiHeadHopAttention.set_attention_dropout is MultiHeadHopAttention.set_attention_dropout
    # the layer without dropout is today's: no buffer, no seed, the same repr
    plain = MultiHeadHopAttention(32, 8)
    assert list(plain.buffers()) == [] and plain.seed is None and plain.attn_dropout == 0.0 and "attn_dropout" not in repr(plain)
    drop = RecomputeMultiHeadHopAttention(32, 8)
    assert drop.set_attention_dropout(0.6, seed=2 ** 63 + 5) is drop
    assert [n for n, _ in drop.named_buffers()] == ["_step"] and list(drop.state_dict()) == ["a_l", "a_r"]
    assert drop.seed == 5 and "attn_dropout=0.6" in repr(drop)
    assert drop._draw_step()[0] == pytest.approx(0.4) and int(drop._step) == 1
    drop.eval()
    assert drop._draw_step() == (1.0, None) and int(drop._step) == 1
    drop.train()
    drop.set_attention_dropout(0.0)                                              # off again: the counter rests, the repr is the plain one
    assert drop._draw_step() == (1.0, None) and "attn_dropout" not in repr(drop) and list(drop.state_dict()) == ["a_l", "a_r"]
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="attn_dropout"):
            MultiHeadHopAttention(32, 8).set_attention_dropout(bad)
    with pytest.raises(ValueError, match="at most 16 heads"):
        MultiHeadHopAttention(136, 34).set_attention_dropout(0.5)
    # the salt is drawn by the method, never by the constructor
    torch.manual_seed(3)
    MultiHeadHopAttention(32, 8)
    state = torch.get_rng_state()
    torch.manual_seed(3)
    layer = MultiHeadHopAttention(32, 8)
    assert torch.equal(torch.get_rng_state(), state)
    layer.set_attention_dropout(0.5, seed=1)
    assert torch.equal(torch.get_rng_state(), state)
    layer.set_attention_dropout(0.5)
    assert not torch.equal(torch.get_rng_state(), state)
    doc = re.sub(r"\s+", " ", hop_attention_recompute_dropout.__doc__)
    for phrase in ("GAT's ``attn_drop``", "drawn INSIDE the forward and backward kernels", "still no ``[nnz_k, K]`` array", "pass a clone",
                   "with or without a gradient", "the same mask", "``K > 16`` with dropout is refused", "call for call"):
        assert phrase in doc, phrase


def test_python_side_refusals_need_no_device():
    from h2gcn_amd.layers import hop_attention_recompute_dropout

    plan = _stand_in_plan()
    x = torch.zeros(6, 8)
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    stats, y, g = torch.zeros(4, 2, 2, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8)
    fwd, bwd, fac = plan.attention_heads_stats_dropout, plan.attention_heads_backward_dropout, plan.attention_dropout_factors
    bad = [
        (r"keep_prob = 0.0 outside \(0, 1\]", lambda: fwd(x, l, r, 0.0, 1)),
        (r"keep_prob = -1.0 outside \(0, 1\]", lambda: fwd(x, l, r, -1.0, 1)),
        (r"keep_prob = 1.5 outside \(0, 1\]", lambda: bwd(x, l, r, stats, y, g, 1.5, 1)),
        (r"keep_prob = nan outside \(0, 1\]", lambda: bwd(x, l, r, stats, y, g, float("nan"), 1)),
        (r"keep_prob = 0.0 outside \(0, 1\]", lambda: fac(2, 0.0, 1)),
        ("n_heads = 17 outside 1..16", lambda: fac(17, 0.5, 1)),
        ("n_heads = 0 outside 1..16", lambda: fac(0, 0.5, 1)),
        ("step must be a 1-element int64 tensor", lambda: fwd(x, l, r, 0.5, 1, 3)),
        ("step must be a 1-element int64 tensor", lambda: fwd(x, l, r, 0.5, 1, torch.zeros(1, dtype=torch.int32))),
        ("step must be a 1-element int64 tensor", lambda: bwd(x, l, r, stats, y, g, 0.5, 1, torch.zeros(2, dtype=torch.int64))),
        ("step must be a 1-element int64 tensor", lambda: fac(2, 0.5, 1, step=torch.zeros(1))),
        ("inputs have 5 rows", lambda: fwd(torch.zeros(5, 8), l, r, 0.5, 1)),                # (the operand checks come first)
        ("all False", lambda: bwd(x, l, r, stats, y, g, 0.5, 1, need_dl=False, need_dr=False, need_dx=False)),
        (r"dropout = 1.0 outside \[0, 1\)", lambda: hop_attention_recompute_dropout(plan, x, l, r, 1.0)),
        (r"dropout = -0.5 outside \[0, 1\)", lambda: hop_attention_recompute_dropout(plan, x, l, r, -0.5)),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_without_dropout_todays_calls_and_with_it_the_new_ones(monkeypatch):
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import RecomputeMultiHeadHopAttention, hop_attention_recompute, hop_attention_recompute_dropout

    plan = _stand_in_plan(n_rows=6)
    calls = _recording(monkeypatch)                                              # (today's stats and backward, recorded)
    seen = []

    def stats_dropout(self, x, l, r, keep_prob, seed, step=None, negative_slope=0.2, hops=None, out=None):
        calls.append(("stats_dropout", dict(keep_prob=keep_prob, seed=seed, step=step)))
        return torch.zeros(6, 2, 8), torch.zeros(6, 2, 2, 2)

    def backward_dropout(self, x, l, r, stats, y, grad, keep_prob, seed, step=None, negative_slope=0.2, hops=None, need_dl=True, need_dr=True,
                         need_dx=True):
        seen.append(dict(keep_prob=keep_prob, seed=seed, step=step))
        return None, None, torch.ones_like(x)

    monkeypatch.setattr(HopPlan, "attention_heads_stats_dropout", stats_dropout)
    monkeypatch.setattr(HopPlan, "attention_heads_backward_dropout", backward_dropout)
    x, l, r = torch.zeros(6, 8), torch.zeros(6, 2, 2), torch.zeros(6, 2, 2)
    a = x.clone().requires_grad_()
    hop_attention_recompute(plan, a, l, r).sum().backward()
    hop_attention_recompute_dropout(plan, a, l, r, 0.0, seed=9).sum().backward()  # no dropout: today's two calls
    assert [name for name, _ in calls] == ["stats", "backward"] * 2 and seen == []
    assert all(set(kw) == {"hops"} for name, kw in calls if name == "stats")
    # with dropout: the dropout launch gets (keep_prob, seed, step), with or without a gradient; its backward the same three
    del calls[:]
    step = torch.tensor([4])
    hop_attention_recompute_dropout(plan, a, l, r, 0.25, seed=9, step=step).sum().backward()
    with torch.no_grad():
        hop_attention_recompute_dropout(plan, a, l, r, 0.25, seed=9, step=step)
    assert [name for name, _ in calls] == ["stats_dropout", "stats_dropout"]
    for _, kw in calls:
        assert kw["keep_prob"] == 0.75 and kw["seed"] == 9 and kw["step"] is step
    assert len(seen) == 1 and seen[0]["keep_prob"] == 0.75 and seen[0]["seed"] == 9 and torch.equal(seen[0]["step"], step)
    # the layer: one step per training forward, the same value for the forward and its backward; none in eval()
    layer = RecomputeMultiHeadHopAttention(8, 2).set_attention_dropout(0.5, seed=3)
    del calls[:], seen[:]
    layer(plan, a).sum().backward()
    assert calls[0][1]["seed"] == 3 and int(calls[0][1]["step"]) == 1 and int(seen[0]["step"]) == 1 and seen[0]["keep_prob"] == 0.5
    layer(plan, a)
    assert int(calls[1][1]["step"]) == 2 and int(calls[0][1]["step"]) == 1, "the step of the first forward moved"
    layer.eval()
    del calls[:]
    layer(plan, a)
    assert [name for name, _ in calls] == ["stats"] and set(calls[0][1]) == {"hops"}


def test_a_library_without_the_symbols_is_named_only_under_dropout(monkeypatch):
    plan = _stand_in_plan()
    x = torch.zeros(6, 8)
    l, r = torch.zeros(4, 2, 2), torch.zeros(6, 2, 2)
    stats, y, g = torch.zeros(4, 2, 2, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8)
    monkeypatch.setattr(_capi, "has", lambda name: name not in (STATS, BACKWARD, FACTORS))
    for name, call in ((STATS, lambda: plan.attention_heads_stats_dropout(x, l, r, 0.5, 1)),
                       (BACKWARD, lambda: plan.attention_heads_backward_dropout(x, l, r, stats, y, g, 0.5, 1)),
                       (FACTORS, lambda: plan.attention_dropout_factors(2, 0.5, 1))):
        with pytest.raises(RuntimeError, match=rf"predates the attention dropout \({name}\): rebuild it"):
            call()
