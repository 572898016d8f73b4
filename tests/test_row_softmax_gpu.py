"""GPU suite: the row softmax over the hop pattern -- HopPlan.row_softmax / row_softmax_backward (h2gcn_row_softmax_hops_f32 /
h2gcn_row_softmax_backward_hops_f32, csrc/row_softmax.hip) and layers.hop_softmax on top of them.

Operands (fixed seeds):
  * a crafted 322 x 400 operand, 3 hops, segment lengths cycling through 0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 400
    (every lane-group, wave and 256-partial boundary; each hop shifts the cycle), planned with long_row_threshold = 32 (segments
    of 63+ entries take the 4-wave workgroups) and 256 (16-lane groups, one wave in registers up to 256, workgroups from 256);
    the schedule sweep adds 1024, where the segments of 257+ entries run on one wave in passes;
  * Cora's hop1_sym / hop2_sym from tests/golden/cora_operands.npz;
  * scores 4 * N(0, 1), clipped per segment to within 32 of the segment's maximum (every exp is a normal number); g ~ U(-1, 1).

Accuracy is judged against fp64 with the bounds of include/h2gcn_hip.h, asserted without any extra factor (u = 2^-24, T the
largest |score - m| of the segment, n its length):
    forward    |alpha - alpha64| <= (6T + n + 6) * u * alpha64
               (3T: the subtraction and the scaled argument, for each of the term and the sum; 2: a 1-ulp exp; n: the sum in any
               order; 3: the reciprocal and the multiplication)
    backward   |ds - exact| <= alpha * gamma_{n+2} * (|g| + sum_j |alpha_j g_j|) + 2^-149   (exact: fp64 on the same fp32 alpha)
Worst error / bound measured on the MI355X: forward 0.25 (crafted) / 0.27 (Cora), backward 0.38 / 0.52 -- see DESIGN.md.
Everything else is torch.equal: the bits are a function of the segment's own contents.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_planetoid_golden
from test_sddmm_gpu import TUNABLES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 400)
N_ROWS, N_COLS = 23 * len(LENGTHS), 400
THRESHOLDS = (32, 256)


def gamma(n):
    return n * U / (1.0 - n * U)


def _pattern(lengths, n_cols, rng):
    """CSR matrix whose row i has lengths[i] entries (ascending random columns, values 1)."""
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, size=n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((np.ones(len(indices), np.float32), indices.astype(np.int32), indptr), shape=(len(lengths), n_cols))


def _crafted_hops():
    rng = np.random.default_rng(14)
    return [_pattern([LENGTHS[(i + 3 * k) % len(LENGTHS)] for i in range(N_ROWS)], N_COLS, rng) for k in range(3)]


def seg_reduce(ufunc, x, indptr, empty=0.0):
    """ufunc-reduction of every segment of x (float64 [n_rows]; `empty` for a segment without entries)."""
    lens = np.diff(indptr)
    out = np.full(len(lens), empty, dtype=np.float64)
    if x.size:
        out[lens > 0] = ufunc.reduceat(x.astype(np.float64), indptr[:-1][lens > 0])
    return out


def spread(per_row, indptr):
    return np.repeat(per_row, np.diff(indptr))


def make_scores(indptr, rng):
    s = (4.0 * rng.standard_normal(int(indptr[-1]))).astype(np.float32)
    m = spread(seg_reduce(np.maximum, s, indptr), indptr).astype(np.float32)
    return np.maximum(s, m - np.float32(32.0)).astype(np.float32)


def forward64(s, indptr):
    """(alpha64, bound factor (6T + n + 6) * u per entry) of fp32 scores s."""
    s64 = s.astype(np.float64)
    t = s64 - spread(seg_reduce(np.maximum, s64, indptr), indptr)
    e = np.exp(t)
    alpha = e / spread(seg_reduce(np.add, e, indptr), indptr)
    T = spread(seg_reduce(np.maximum, np.abs(t), indptr), indptr)
    n = spread(np.diff(indptr).astype(np.float64), indptr)
    return alpha, (6.0 * T + n + 6.0) * U


def backward64(alpha, g, indptr):
    """(exact dscore in fp64 from the fp32 alpha, bound per entry)."""
    a, g = alpha.astype(np.float64), g.astype(np.float64)
    D = spread(seg_reduce(np.add, a * g, indptr), indptr)
    A = spread(seg_reduce(np.add, np.abs(a * g), indptr), indptr)
    n = spread(np.diff(indptr).astype(np.float64), indptr)
    return a * (g - D), a * gamma(n + 2.0) * (np.abs(g) + A) + 2.0 ** -149


class Operand:
    """Hop matrices, their scores / gradients (host and device) and the fp64 references, computed once and never changed."""

    def __init__(self, name, mats, seed):
        rng = np.random.default_rng(seed)
        self.name, self.mats = name, mats
        self.indptr = [m.indptr.astype(np.int64) for m in mats]
        self.scores = [make_scores(p, rng) for p in self.indptr]
        self.grads = [rng.uniform(-1, 1, int(p[-1])).astype(np.float32) for p in self.indptr]
        self.scores_dev = [torch.from_numpy(s).to(DEV) for s in self.scores]
        self.grads_dev = [torch.from_numpy(g).to(DEV) for g in self.grads]
        self.fwd64 = [forward64(s, p) for s, p in zip(self.scores, self.indptr)]
        self._plans = {}

    def plan(self, **kw):
        from h2gcn_amd import HopPlan

        key = tuple(sorted(kw.items()))
        if key not in self._plans:
            self._plans[key] = HopPlan.from_scipy(self.mats, DEV, **kw)
        return self._plans[key]


@pytest.fixture(scope="module")
def crafted():
    return Operand("crafted", _crafted_hops(), 100)


@pytest.fixture(scope="module")
def cora():
    g = load_planetoid_golden("cora")
    return Operand("cora", [sp.csr_matrix(g["hop1_sym"]), sp.csr_matrix(g["hop2_sym"])], 101)


def operands_and_plans(crafted, cora):
    for thr in THRESHOLDS:
        yield crafted, crafted.plan(long_row_threshold=thr, rows_per_wave=4), f"crafted thr={thr}"
    yield cora, cora.plan(), "cora"


def equal_lists(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------ 1. forward accuracy against fp64
def test_forward_accuracy(crafted, cora):
    n_long = [crafted.plan(long_row_threshold=thr, rows_per_wave=4).info(0)["n_long_segments"] for thr in THRESHOLDS]
    assert n_long[0] > n_long[1] > 0
    for op, plan, what in operands_and_plans(crafted, cora):
        alpha = plan.row_softmax(op.scores_dev)
        for s, (got, (want, factor)) in enumerate(zip(alpha, op.fwd64)):
            assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want.shape
            err, bound = np.abs(got.cpu().numpy().astype(np.float64) - want), factor * want
            print(f"forward {what} hop {s}: worst err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (what, s, float((err / bound).max()))


# ------------------------------------------------------------------ 2. backward accuracy against fp64 (from the same fp32 alpha)
def test_backward_accuracy(crafted, cora):
    for op, plan, what in operands_and_plans(crafted, cora):
        alpha = plan.row_softmax(op.scores_dev)
        ds = plan.row_softmax_backward(alpha, op.grads_dev)
        for s in range(len(alpha)):
            exact, bound = backward64(alpha[s].cpu().numpy(), op.grads[s], op.indptr[s])
            err = np.abs(ds[s].cpu().numpy().astype(np.float64) - exact)
            print(f"backward {what} hop {s}: worst err / bound {float((err / bound).max()):.3f}")
            assert ds[s].dtype == torch.float32 and (err <= bound).all(), (what, s, float((err / bound).max()))


# ------------------------------------------------------------------ 3. invariants
def test_invariants(crafted, cora):
    for op, plan, what in operands_and_plans(crafted, cora):
        alpha = plan.row_softmax(op.scores_dev)
        ds = plan.row_softmax_backward(alpha, op.grads_dev)
        for s, p in enumerate(op.indptr):
            nonempty = np.diff(p) > 0
            a = alpha[s].cpu().numpy()
            factor = seg_reduce(np.maximum, op.fwd64[s][1], p)            # (6T + n + 6) u: constant within a segment
            total = seg_reduce(np.add, a, p)
            assert (np.abs(total - 1.0)[nonempty] <= factor[nonempty]).all(), (what, s)
            _, bound = backward64(a, op.grads[s], p)
            assert (np.abs(seg_reduce(np.add, ds[s].cpu().numpy(), p)) <= seg_reduce(np.add, bound, p)).all(), (what, s)


# ------------------------------------------------------------------ 4. the bits do not depend on the schedule
def both(plan, scores, grads, hops=None):
    alpha = plan.row_softmax(scores, hops=hops)
    return alpha, plan.row_softmax_backward(alpha, grads, hops=hops)


@pytest.mark.parametrize("build_transpose", (True, False))
def test_bits_do_not_depend_on_plan_tunables(crafted, cora, build_transpose):
    """(build_transpose=False: the launches need no transposed operand -- the forward row pointers only)"""
    for op in (crafted, cora):
        want = both(op.plan(long_row_threshold=32), op.scores_dev, op.grads_dev)
        for kw in TUNABLES + (dict(long_row_threshold=1024), dict(long_row_threshold=1024, rows_per_wave=3), dict(long_row_threshold=256, rows_per_wave=4)):
            got = both(op.plan(build_transpose=build_transpose, **kw), op.scores_dev, op.grads_dev)
            assert equal_lists(got[0], want[0]) and equal_lists(got[1], want[1]), (op.name, kw)


def test_bits_hop_alone_vs_all_hops_and_repeated_launches(crafted):
    plan = crafted.plan(long_row_threshold=32)
    want = both(plan, crafted.scores_dev, crafted.grads_dev)
    again = both(plan, crafted.scores_dev, crafted.grads_dev)           # two launches in a row
    assert equal_lists(again[0], want[0]) and equal_lists(again[1], want[1])
    for k in range(3):
        a, d = both(plan, crafted.scores_dev[k:k + 1], crafted.grads_dev[k:k + 1], hops=[k])
        assert torch.equal(a[0], want[0][k]) and torch.equal(d[0], want[1][k]), k
    a, d = both(plan, crafted.scores_dev[::2], crafted.grads_dev[::2], hops=[0, 2])
    assert equal_lists(a, want[0][::2]) and equal_lists(d, want[1][::2])


def test_bits_row_selected_sub_plan(crafted):
    plan = crafted.plan(long_row_threshold=32)
    want = both(plan, crafted.scores_dev, crafted.grads_dev)
    rows = [0, 3, 6, 7, 8, 9, 10, 11, 12, 13, 17, 18, 29, 40, 150, 321]
    sel = plan.select_rows(rows, build_transpose=False)
    assert sel.plan.n_rows == len(rows) and sel.plan.n_cols == N_COLS
    entries = [torch.from_numpy(np.concatenate([np.arange(p[r], p[r + 1]) for r in rows])).to(DEV) for p in crafted.indptr]
    got = both(sel.plan, [t[e] for t, e in zip(crafted.scores_dev, entries)], [t[e] for t, e in zip(crafted.grads_dev, entries)])
    for s in range(3):
        assert torch.equal(got[0][s], want[0][s][entries[s]]) and torch.equal(got[1][s], want[1][s][entries[s]]), s


# ------------------------------------------------------------------ 5. the bits depend on the segment only
def test_bits_depend_on_the_segment_only(crafted):
    """The same score segments in other rows, other hops and at other offsets: row r of hop (k + 1) % 3 of the second operand is
    row order[r] of hop k of the first."""
    from h2gcn_amd import HopPlan

    order = np.random.default_rng(5).permutation(N_ROWS)
    mats, src = [None] * 3, [None] * 3
    for k, m in enumerate(crafted.mats):
        p = crafted.indptr[k]
        lens = np.diff(p)[order]
        new_p = np.concatenate([[0], np.cumsum(lens)])
        mats[(k + 1) % 3] = m[order, :]
        src[(k + 1) % 3] = torch.from_numpy(np.repeat(p[order] - new_p[:-1], lens) + np.arange(int(new_p[-1]))).to(DEV)
        assert (src[(k + 1) % 3].cpu().numpy() % 4 != np.arange(int(new_p[-1])) % 4).any()      # other alignments of the entries
    for thr_a, thr_b in ((32, 32), (32, 256), (256, 1024)):
        want = both(crafted.plan(long_row_threshold=thr_a), crafted.scores_dev, crafted.grads_dev)
        moved = HopPlan.from_scipy(mats, DEV, long_row_threshold=thr_b)
        got = both(moved, [crafted.scores_dev[(j - 1) % 3][src[j]] for j in range(3)], [crafted.grads_dev[(j - 1) % 3][src[j]] for j in range(3)])
        for j in range(3):
            assert torch.equal(got[0][j], want[0][(j - 1) % 3][src[j]]) and torch.equal(got[1][j], want[1][(j - 1) % 3][src[j]]), (thr_a, thr_b, j)


# ------------------------------------------------------------------ 6. in place
def test_in_place(crafted, cora):
    for op, plan, what in operands_and_plans(crafted, cora):
        want = both(plan, op.scores_dev, op.grads_dev)
        buf = [t.clone() for t in op.scores_dev]
        res = plan.row_softmax(buf, out=buf)
        assert all(r is b for r, b in zip(res, buf)) and equal_lists(buf, want[0]), what
        gbuf = [t.clone() for t in op.grads_dev]
        res = plan.row_softmax_backward(buf, gbuf, out=gbuf)
        assert all(r is b for r, b in zip(res, gbuf)) and equal_lists(gbuf, want[1]), what
        out = [torch.full_like(t, float("nan")) for t in op.scores_dev]      # out=: overwritten
        assert equal_lists(plan.row_softmax(op.scores_dev, out=out), want[0]), what


# ------------------------------------------------------------------ 7. non-finite scores
SPECIAL_LENGTHS = (1, 3, 17, 70, 300)
KINDS = ("nan", "+inf", "only -inf", "-inf among finite")


def _special_operand():
    """One hop; per length 12 special rows (kind x position of the special value) alternating with 12 plain neighbours of the
    same length, so that four consecutive rows share a length (the tile walk then serves them on one mapping)."""
    lengths, cases = [], []
    for n in SPECIAL_LENGTHS:
        for kind in KINDS:
            for pos in (0, n // 2, n - 1):
                if not (kind == "-inf among finite" and n == 1):      # (a segment of one entry has no finite neighbour)
                    cases.append((len(lengths), n, kind, pos))
                lengths += [n, n]                                     # the special row and a neighbour
    return _pattern(lengths, N_COLS, np.random.default_rng(7)), cases


def test_non_finite_scores_follow_torch_softmax():
    from h2gcn_amd import HopPlan

    mat, cases = _special_operand()
    p = mat.indptr.astype(np.int64)
    base = make_scores(p, np.random.default_rng(8))
    special = base.copy()
    for row, n, kind, pos in cases:
        seg = special[p[row]:p[row + 1]]
        if kind == "nan":
            seg[pos] = np.nan
        elif kind == "+inf":
            seg[pos] = np.inf
        elif kind == "only -inf":
            seg[:] = -np.inf
        else:
            seg[pos] = -np.inf
            if n == 3:
                seg[(pos + 1) % 3] = -np.inf                          # two of the three
    touched = np.zeros(len(base), bool)
    for row, *_ in cases:
        touched[p[row]:p[row + 1]] = True
    keep = torch.from_numpy(~touched).to(DEV)
    for thr in THRESHOLDS + (1024,):
        plan = HopPlan.from_scipy([mat], DEV, long_row_threshold=thr, rows_per_wave=4)
        plain = plan.row_softmax([torch.from_numpy(base).to(DEV)])[0]
        got_dev = plan.row_softmax([torch.from_numpy(special).to(DEV)])[0]
        assert torch.equal(got_dev[keep], plain[keep]), thr         # the neighbours: bit-unchanged
        got = got_dev.cpu().numpy()
        for row, n, kind, pos in cases:
            seg = special[p[row]:p[row + 1]]
            want = torch.softmax(torch.from_numpy(seg).double(), 0).numpy()
            have = got[p[row]:p[row + 1]]
            assert np.array_equal(np.isnan(have), np.isnan(want)), (thr, n, kind, pos)
            assert np.array_equal(have == 0.0, want == 0.0) and not np.signbit(have[have == 0.0]).any(), (thr, n, kind, pos)
            if kind == "-inf among finite":
                fin = np.isfinite(seg)
                T = np.abs(seg[fin].astype(np.float64) - seg[fin].max()).max()
                assert (np.abs(have - want) <= (6.0 * T + n + 6.0) * U * want).all(), (thr, n, kind, pos)
            else:
                assert np.isnan(have).all(), (thr, n, kind, pos)


# ------------------------------------------------------------------ 8. refusals
def test_refusals(crafted, monkeypatch):
    from h2gcn_amd import HopPlan, _capi
    from h2gcn_amd.layers import hop_softmax

    plan = crafted.plan(long_row_threshold=32)
    L = _capi.lib()
    calls = []
    real = {n: getattr(L, n) for n in ("h2gcn_row_softmax_hops_f32", "h2gcn_row_softmax_backward_hops_f32")}
    for n in real:
        monkeypatch.setattr(L, n, lambda *a, _n=n: calls.append(_n) or real[_n](*a))
    sc, gr = crafted.scores_dev, crafted.grads_dev

    class Sharded:
        def aggregate(self, inputs, hops):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="row-partitioned"):
        hop_softmax(Sharded(), sc)
    bad = {
        "must list 3 tensors": sc[:2],
        "fp32 only": [sc[0].to(torch.bfloat16), sc[1], sc[2]],
        "must be float32": [sc[0].double(), sc[1], sc[2]],
        "plan on": [sc[0].cpu(), sc[1], sc[2]],
        "must have shape": [sc[0], sc[1][:-1], sc[2]],
        "must be contiguous": [sc[0], sc[1], torch.cat([sc[2], sc[2]])[::2]],
        "must be a sequence": sc[0],
    }
    for match, arg in bad.items():
        with pytest.raises(ValueError, match=match):
            plan.row_softmax(arg)
        with pytest.raises(ValueError, match=match):
            hop_softmax(plan, arg)
        with pytest.raises(ValueError, match=match):
            plan.row_softmax_backward(sc, arg)
        with pytest.raises(ValueError, match=match):
            plan.row_softmax_backward(arg, gr)
        if not isinstance(arg, torch.Tensor):
            with pytest.raises(ValueError, match=match):
                plan.row_softmax(sc, out=arg)
    with pytest.raises(ValueError, match="must list 1 tensors"):
        plan.row_softmax(sc, hops=[1])
    with pytest.raises(ValueError, match="hop index 3 outside"):
        plan.row_softmax(sc[:1], hops=[3])
    assert calls == []
    monkeypatch.setattr(_capi, "has", lambda name: "row_softmax" not in name)      # a library that predates the symbols
    with pytest.raises(RuntimeError, match="predates the row softmax"):
        plan.row_softmax(sc)
    with pytest.raises(RuntimeError, match="predates the row softmax"):
        plan.row_softmax_backward(sc, gr)
    monkeypatch.undo()
    assert calls == []

    # the C calls: a NULL entry of a hop that has nonzeros, a NULL table, a mask outside the plan -- all before any launch
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in sc])
    holed = (ctypes.c_void_p * 3)(sc[0].data_ptr(), None, sc[2].data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # (evaluated one at a time: the error channel holds the last message)
    for fn, args, needle in ((L.h2gcn_row_softmax_hops_f32, (0, holed, ptrs), b"scores[1] is NULL"),
                             (L.h2gcn_row_softmax_hops_f32, (0, ptrs, holed), b"alpha[1] is NULL"),
                             (L.h2gcn_row_softmax_backward_hops_f32, (0, ptrs, holed, ptrs), b"dalpha[1] is NULL"),
                             (L.h2gcn_row_softmax_backward_hops_f32, (0, ptrs, ptrs, holed), b"dscores[1] is NULL"),
                             (L.h2gcn_row_softmax_hops_f32, (0, None, ptrs), b"scores is NULL"),
                             (L.h2gcn_row_softmax_backward_hops_f32, (0, ptrs, None, ptrs), b"dalpha is NULL"),
                             (L.h2gcn_row_softmax_hops_f32, (1 << 3, ptrs, ptrs), b"hop")):
        assert fn(plan._handle, *args, stream) == _capi.ERR_INVALID_ARGUMENT, needle
        assert needle in L.h2gcn_last_error(), (needle, L.h2gcn_last_error())

    # a launch that would have to build a long-segment list under capture: refused with the forward launch's advice
    fresh = HopPlan.from_scipy(crafted.mats, DEV, long_row_threshold=32)
    out = [torch.empty_like(sc[1])]
    errors = []
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for fn in (lambda: fresh.row_softmax(sc[1:2], hops=[1], out=out), lambda: fresh.row_softmax_backward(sc[1:2], gr[1:2], hops=[1], out=out)):
            try:
                fn()
            except _capi.H2GCNError as e:
                errors.append(str(e))
    assert len(errors) == 2 and all("captured" in e and "warm-up" in e for e in errors), errors


# ------------------------------------------------------------------ 9. hipGraph
def test_hipgraph_replay_equals_eager(crafted):
    plan = crafted.plan(long_row_threshold=32)
    s_static = [t.clone() for t in crafted.scores_dev]
    g_static = [t.clone() for t in crafted.grads_dev]
    alpha = [torch.empty_like(t) for t in s_static]
    ds = [torch.empty_like(t) for t in s_static]
    plan.row_softmax(s_static, out=alpha)                                   # one eager launch
    first = [t.clone() for t in plan.row_softmax_backward(alpha, g_static, out=ds)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.row_softmax(s_static, out=alpha)
        plan.row_softmax_backward(alpha, g_static, out=ds)
    for s, g in zip(s_static, g_static):                                    # fresh contents of the static inputs
        s.copy_(s.flip(0) * 0.5)
        g.copy_(g.flip(0))
    for t in alpha + ds:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want = both(plan, [t.clone() for t in s_static], [t.clone() for t in g_static])
    assert equal_lists(alpha, want[0]) and equal_lists(ds, want[1]) and not equal_lists(ds, first)


# ------------------------------------------------------------------ 10. autograd end to end
def test_autograd_end_to_end_against_dense_replicas(cora):
    """Test 10 of the row-softmax issue: GAT-style scores on Cora through hop_softmax and hop_spmm(values=...), the parameter
    gradients against a dense fp64 replica (masked dense torch.softmax, A @ h) under torch's own autograd; the figure
    max|g - g64| / max|g64| may be at most max(8 x the same figure of the dense fp32 replica on the same device, 1e-5).
    Measured on the MI355X: W 6.8e-7 (replica 7.9e-7), a_l 6.3e-7 (4.6e-7), a_r 5.4e-7 (4.9e-7)."""
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import hop_softmax, hop_spmm

    mats = cora.mats
    n, f, d = mats[0].shape[0], 48, 16
    plan = HopPlan.from_scipy(mats, DEV, build_transpose=True, keep_permutation=True)
    gen = torch.Generator().manual_seed(10)
    X0 = (torch.rand((n, f), generator=gen) * 2 - 1).to(DEV)
    R = (torch.rand((n, 2, d), generator=gen) * 2 - 1).to(DEV)
    init = [((torch.rand(shape, generator=gen) * 2 - 1) * scale).to(DEV) for shape, scale in (((f, d), 0.3), ((d,), 1.0), ((d,), 1.0))]
    rows = [torch.from_numpy(np.repeat(np.arange(n), np.diff(m.indptr))).to(DEV) for m in mats]
    cols = [torch.from_numpy(m.indices.astype(np.int64)).to(DEV) for m in mats]

    # the library's path
    W, a_l, a_r = (t.clone().requires_grad_(True) for t in init)
    h = X0 @ W
    scores = [torch.nn.functional.leaky_relu((h @ a_l)[r] + (h @ a_r)[c], 0.2) for r, c in zip(rows, cols)]
    alpha = hop_softmax(plan, scores)
    assert isinstance(alpha, tuple) and len(alpha) == 2
    y = hop_spmm(plan, h, values=list(alpha))
    loss = (y * R).sum()
    dalpha = torch.autograd.grad(loss, alpha, retain_graph=True)
    dscores = torch.autograd.grad(alpha, scores, dalpha, retain_graph=True)
    want = plan.row_softmax_backward([a.detach() for a in alpha], [g.contiguous() for g in dalpha])
    assert equal_lists(list(dscores), want)              # hop_softmax's backward IS the launch
    loss.backward()
    got = [W.grad, a_l.grad, a_r.grad]
    # only hop 1's scores require a gradient: still one launch over the selected hops, and hop 1's result is that launch's
    s0, s1 = scores[0].detach(), scores[1].detach().requires_grad_(True)
    al2 = hop_softmax(plan, [s0, s1])
    assert torch.equal(al2[0], alpha[0].detach()) and torch.equal(al2[1], alpha[1].detach())
    (al2[1] * dalpha[1]).sum().backward()
    assert torch.equal(s1.grad, plan.row_softmax_backward([a.detach() for a in alpha], [torch.zeros_like(dalpha[0]), dalpha[1]])[1])
    assert not hop_softmax(plan, [s0, scores[1].detach()])[0].requires_grad

    def replica(dtype):
        Wd, ld, rd = (t.to(dtype).clone().requires_grad_(True) for t in init)
        hd = X0.to(dtype) @ Wd
        ys = []
        for r, c in zip(rows, cols):
            e = torch.nn.functional.leaky_relu((hd @ ld)[:, None] + (hd @ rd)[None, :], 0.2)
            mask = torch.zeros((n, n), dtype=torch.bool, device=DEV).index_put((r, c), torch.ones((), dtype=torch.bool, device=DEV))
            # (a row without entries keeps its finite scores: an all -inf row would be NaN, also in the backward; it is zeroed next)
            A = torch.softmax(e.masked_fill(~mask & mask.any(dim=1, keepdim=True), float("-inf")), dim=1)
            A = torch.where(mask, A, torch.zeros((), dtype=dtype, device=DEV))
            ys.append(A @ hd)
        (torch.stack(ys, dim=1) * R.to(dtype)).sum().backward()
        return [Wd.grad, ld.grad, rd.grad]

    g64, g32 = replica(torch.float64), replica(torch.float32)
    for name, g, r64, r32 in zip(("W", "a_l", "a_r"), got, g64, g32):
        scale = float(r64.abs().max())
        ours, theirs = float((g.double() - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
        print(f"d{name}: max|g - g64| / max|g64| = {ours:.3e}; dense fp32 replica {theirs:.3e}")
        assert ours <= max(8.0 * theirs, 1e-5), (name, ours, theirs)
