"""GPU suite: the additive edge scores on the hop pattern -- HopPlan.edge_scores / edge_scores_backward
(h2gcn_edge_scores_hops_f32 / h2gcn_edge_scores_backward_hops_f32, csrc/edge_scores.hip), layers.hop_edge_scores and
layers.HopAttention on top of them.

Operands (fixed seeds):
  * the crafted 322 x 400, 3-hop operand of test_row_softmax_gpu.py (segment lengths on every lane-group / wave / 256-partial
    boundary; its transpose has ragged lengths of its own), planned with build_transpose=True, keep_permutation=True at
    long_row_threshold = 32 and 256;
  * Cora's hop1_sym / hop2_sym from tests/golden/cora_operands.npz;
  * l, r ~ N(0, 1), g ~ U(-1, 1).

The forward is torch.equal with torch's own leaky_relu(l[row] + r[col]).  The backward is compared BIT FOR BIT with a numpy fp32
restatement of the documented tree (256 partials, four 64-lane xor butterflies, (W0 + W1) + (W2 + W3)) over the rows of A_k and
of a scipy-transposed A_k, and against fp64 with the bound of include/h2gcn_hip.h asserted without any factor (u = 2^-24, n the
segment length, t the terms):
    |dl - exact| <= gamma_{n+1} * sum |t| + (n + 1) * 2^-149        and the same for dr
Worst error / bound measured on the MI355X: crafted dl 0.38, dr 0.007; Cora dl 0.51, dr 0.47.  HopAttention on Cora against the
dense fp64 replica, max|g - g64| / max|g64| (dense fp32 replica in brackets): W 5.4e-7 (5.1e-7), a_l 5.3e-7 (2.2e-7), a_r 6.0e-7
(6.0e-7); max|y - y64| 6.7e-7 at max|y64| 2.9 (replica 6.7e-7) -- see DESIGN.md.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_planetoid_golden
from test_row_softmax_gpu import _crafted_hops, seg_reduce
from test_sddmm_gpu import TUNABLES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
THRESHOLDS = (32, 256)
ADJ = dict(build_transpose=True, keep_permutation=True)
F32 = np.float32


def gamma(n):
    return n * U / (1.0 - n * U)


def tree_sum(t):
    """The documented summation tree on the fp32 terms of one segment, in numpy fp32."""
    P = np.zeros(256, F32)
    for start in range(0, len(t), 256):                     # ascending position within every partial
        chunk = t[start:start + 256]
        P[:len(chunk)] = P[:len(chunk)] + chunk
    W = []
    lanes = np.arange(64)
    for w in range(4):
        v = P[64 * w:64 * w + 64].copy()
        for dist in (1, 2, 4, 8, 16, 32):
            v = v + v[lanes ^ dist]
        W.append(v[0])
    return (W[0] + W[1]) + (W[2] + W[3])


def tree_rows(t, indptr):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([tree_sum(t[indptr[i]:indptr[i + 1]]) for i in range(len(indptr) - 1)], F32)


class Operand:
    """Hop matrices, their transposes, node terms and entry gradients (host and device): computed once, never changed."""

    def __init__(self, name, mats, seed):
        rng = np.random.default_rng(seed)
        self.name, self.mats, self.H = name, mats, len(mats)
        self.n_rows, self.n_cols = mats[0].shape
        self.indptr = [m.indptr.astype(np.int64) for m in mats]
        self.rows = [np.repeat(np.arange(self.n_rows), np.diff(p)) for p in self.indptr]
        self.cols = [m.indices.astype(np.int64) for m in mats]
        # A_k^T in canonical CSR order; perm[e'] = forward entry behind transposed entry e'
        self.t_indptr, self.perm = [], []
        for m in mats:
            t = sp.csr_matrix((np.arange(1, m.nnz + 1, dtype=np.int64), m.indices, m.indptr), shape=m.shape).T.tocsr()
            t.sort_indices()
            self.t_indptr.append(t.indptr.astype(np.int64))
            self.perm.append(t.data.astype(np.int64) - 1)
        self.l = rng.standard_normal((self.n_rows, self.H)).astype(F32)
        self.r = rng.standard_normal((self.n_cols, self.H)).astype(F32)
        self.g = [rng.uniform(-1, 1, m.nnz).astype(F32) for m in mats]
        self.l_dev, self.r_dev = torch.from_numpy(self.l).to(DEV), torch.from_numpy(self.r).to(DEV)
        self.g_dev = [torch.from_numpy(g).to(DEV) for g in self.g]
        self.rows_dev = [torch.from_numpy(x).to(DEV) for x in self.rows]
        self.cols_dev = [torch.from_numpy(x).to(DEV) for x in self.cols]
        self._plans, self._bits = {}, {}

    def plan(self, **kw):
        from h2gcn_amd import HopPlan

        key = tuple(sorted(kw.items()))
        if key not in self._plans:
            self._plans[key] = HopPlan.from_scipy(self.mats, DEV, **kw)
        return self._plans[key]

    def terms(self, s, slope, l=None, r=None, g=None, k=None):
        """fp32 t of hop k (column s of l / r), forward entry order: the arithmetic of the header."""
        k = s if k is None else k
        l, r, g = (self.l if l is None else l), (self.r if r is None else r), (self.g[k] if g is None else g)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            pre = l[self.rows[k], s] + r[self.cols[k], s]
            return np.where(pre > 0, g, g * F32(slope)).astype(F32), pre

    def tree_bits(self, slope, l=None, r=None, g=None):
        """(dl, dr) of the documented tree in numpy fp32 (cached for the default operands)."""
        key = slope if l is None and r is None and g is None else None
        if key is not None and key in self._bits:
            return self._bits[key]
        dl, dr = np.zeros((self.n_rows, self.H), F32), np.zeros((self.n_cols, self.H), F32)
        for s in range(self.H):
            t, _ = self.terms(s, slope, l, r, None if g is None else g[s])
            dl[:, s] = tree_rows(t, self.indptr[s])
            dr[:, s] = tree_rows(t[self.perm[s]], self.t_indptr[s])
        if key is not None:
            self._bits[key] = (dl, dr)
        return dl, dr

    def composite(self, l, r, slope, hops=None):
        """What a caller writes in torch today: gathers through a row-of-entry index and leaky_relu."""
        hops = range(self.H) if hops is None else hops
        return [torch.nn.functional.leaky_relu(l[self.rows_dev[k], s] + r[self.cols_dev[k], s], slope) for s, k in enumerate(hops)]


@pytest.fixture(scope="module")
def crafted():
    return Operand("crafted", _crafted_hops(), 200)


@pytest.fixture(scope="module")
def cora():
    g = load_planetoid_golden("cora")
    return Operand("cora", [sp.csr_matrix(g["hop1_sym"]), sp.csr_matrix(g["hop2_sym"])], 201)


def operands_and_plans(crafted, cora):
    for thr in THRESHOLDS:
        yield crafted, crafted.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ), f"crafted thr={thr}"
    yield cora, cora.plan(**ADJ), "cora"


def equal_lists(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def same_bits(dev_tensor, host_array):
    """Bit equality, the sign of a zero included (NaNs: both NaN)."""
    got = dev_tensor.cpu().numpy()
    nan = np.isnan(host_array)
    return got.shape == host_array.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], host_array.view(np.int32)[~nan])


# ------------------------------------------------------------------ 1. forward bits
def test_forward_bits_equal_torch(crafted, cora):
    n_long = [crafted.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ).info(0)["n_long_segments"] for thr in THRESHOLDS]
    assert n_long[0] > n_long[1] > 0
    for op, plan, what in operands_and_plans(crafted, cora):
        for slope in (0.2, 0.0):
            got = plan.edge_scores(op.l_dev, op.r_dev, slope)
            assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == (m.nnz,) for t, m in zip(got, op.mats))
            assert equal_lists(got, op.composite(op.l_dev, op.r_dev, slope)), (what, slope)
        assert equal_lists(plan.edge_scores(op.l_dev, op.r_dev), op.composite(op.l_dev, op.r_dev, 0.2)), what     # the default slope
        want = op.composite(op.l_dev, op.r_dev, 0.2)
        # hop subsets: column s of l / r belongs to the s-th selected hop
        for hops in ([op.H - 1], [0, op.H - 1]):
            l, r = op.l_dev[:, :len(hops)], op.r_dev[:, :len(hops)]                 # (row stride H: passes through)
            assert l.stride(0) == op.H
            assert equal_lists(plan.edge_scores(l, r, hops=hops), op.composite(l, r, 0.2, hops)), (what, hops)
        # one hop, 1-D operands (a strided 1-D view included)
        k = op.H - 1
        assert torch.equal(plan.edge_scores(op.l_dev[:, k].contiguous(), op.r_dev[:, k], hops=[k])[0], want[k]), what
        # strided column slices of a wider tensor; out= is overwritten
        wide_l, wide_r = torch.zeros((op.n_rows, op.H + 3), device=DEV), torch.zeros((op.n_cols, op.H + 5), device=DEV)
        wide_l[:, 1:1 + op.H], wide_r[:, 2:2 + op.H] = op.l_dev, op.r_dev
        out = [torch.full_like(t, float("nan")) for t in want]
        res = plan.edge_scores(wide_l[:, 1:1 + op.H], wide_r[:, 2:2 + op.H], out=out)
        assert all(a is b for a, b in zip(res, out)) and equal_lists(out, want), what
        # a non-unit column stride is made contiguous
        assert equal_lists(plan.edge_scores(op.l_dev.t().contiguous().t(), op.r_dev.t().contiguous().t()), want), what


# ------------------------------------------------------------------ 2. backward bits against the tree
@pytest.mark.parametrize("slope", (0.2, 0.0))
def test_backward_bits_equal_the_documented_tree(crafted, slope):
    """(slope 0 with negative g makes terms of -0: the partials start at +0, so an all -0 segment still sums to +0)"""
    want_dl, want_dr = crafted.tree_bits(slope)
    for thr in THRESHOLDS + (1024,):
        plan = crafted.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ)
        dl, dr = plan.edge_scores_backward(crafted.l_dev, crafted.r_dev, crafted.g_dev, slope)
        assert dl.dtype == torch.float32 and tuple(dl.shape) == (crafted.n_rows, 3) and tuple(dr.shape) == (crafted.n_cols, 3)
        assert same_bits(dl, want_dl), (thr, "dl")
        assert same_bits(dr, want_dr), (thr, "dr")
    assert (np.diff(crafted.indptr[0]) == 0).any()                              # empty rows: +0


def test_backward_bits_with_empty_columns(crafted):
    """The crafted operand without its entries in the columns 380 .. 399: every column of A_k^T beyond 379 is an empty segment
    and gets +0, after (and next to) non-empty ones."""
    mats = []
    for m in crafted.mats:
        m = m.copy()
        m.data[m.indices >= 380] = 0
        m.eliminate_zeros()
        mats.append(m)
    op = Operand("crafted, 20 empty columns", mats, 202)
    assert op.n_cols == 400 and all((np.diff(p)[380:] == 0).all() and (np.diff(p)[:380] > 0).all() for p in op.t_indptr)
    want_dl, want_dr = op.tree_bits(0.2)
    assert not want_dr[380:].any() and not np.signbit(want_dr[380:]).any()
    for thr in THRESHOLDS:
        dl, dr = op.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ).edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
        assert same_bits(dl, want_dl) and same_bits(dr, want_dr), thr


# ------------------------------------------------------------------ 3. backward accuracy against fp64, without a factor
def test_backward_accuracy(crafted, cora):
    """Worst error / bound measured on the MI355X: crafted dl 0.38, dr 0.007; Cora dl 0.51, dr 0.47."""
    for op, plan, what in operands_and_plans(crafted, cora):
        dl, dr = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev, 0.2)
        for s in range(op.H):
            t32, pre = op.terms(s, 0.2)
            t64 = np.where(pre > 0, op.g[s].astype(np.float64), op.g[s].astype(np.float64) * float(F32(0.2)))
            for name, got, t, p in (("dl", dl, t64, op.indptr[s]), ("dr", dr, t64[op.perm[s]], op.t_indptr[s])):
                n = np.diff(p).astype(np.float64)
                exact, mag = seg_reduce(np.add, t, p), seg_reduce(np.add, np.abs(t), p)
                bound = gamma(n + 1.0) * mag + (n + 1.0) * 2.0 ** -149
                err = np.abs(got[:, s].cpu().numpy().astype(np.float64) - exact)
                print(f"backward {what} hop {s} {name}: worst err / bound {float((err / bound).max()):.3f}")
                assert (err <= bound).all(), (what, s, name, float((err / bound).max()))


# ------------------------------------------------------------------ 4. the bits do not depend on the schedule
def test_bits_do_not_depend_on_plan_tunables(crafted, cora):
    for op in (crafted, cora):
        ref = op.plan(long_row_threshold=32, **ADJ)
        want = ref.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
        want_s = ref.edge_scores(op.l_dev, op.r_dev)
        for kw in TUNABLES + (dict(long_row_threshold=1024), dict(long_row_threshold=1024, rows_per_wave=3), dict(variant=2)):
            plan = op.plan(**kw, **ADJ)
            got = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (op.name, kw)
            assert equal_lists(plan.edge_scores(op.l_dev, op.r_dev), want_s), (op.name, kw)


def test_bits_hop_alone_repeated_launches_and_single_sides(crafted):
    for thr in THRESHOLDS:
        plan = crafted.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ)
        l, r, g = crafted.l_dev, crafted.r_dev, crafted.g_dev
        want = plan.edge_scores_backward(l, r, g)
        again = plan.edge_scores_backward(l, r, g)                                   # two launches in a row: no atomics
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
        for k in range(3):
            dl, dr = plan.edge_scores_backward(l[:, k], r[:, k], g[k:k + 1], hops=[k])
            assert dl.shape == (crafted.n_rows,) and dr.shape == (crafted.n_cols,)   # 1-D in, 1-D out
            assert torch.equal(dl, want[0][:, k]) and torch.equal(dr, want[1][:, k]), (thr, k)
        dl, dr = plan.edge_scores_backward(l[:, ::2], r[:, ::2], g[::2], hops=[0, 2])
        assert torch.equal(dl, want[0][:, ::2]) and torch.equal(dr, want[1][:, ::2]), thr
        only_l = plan.edge_scores_backward(l, r, g, need_dr=False)
        only_r = plan.edge_scores_backward(l, r, g, need_dl=False)
        assert only_l[1] is None and only_r[0] is None
        assert torch.equal(only_l[0], want[0]) and torch.equal(only_r[1], want[1]), thr


def test_eight_hops(crafted):
    """Every lane of the row-pointer load in use (8 hops x 7 rows per wave): the forward against torch, the backward against
    one-hop launches."""
    op = Operand("crafted x 8 hops", [crafted.mats[k % 3] for k in range(8)], 203)
    plan = op.plan(long_row_threshold=32, **ADJ)
    assert equal_lists(plan.edge_scores(op.l_dev, op.r_dev), op.composite(op.l_dev, op.r_dev, 0.2))
    dl, dr = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
    for k in range(8):
        one = plan.edge_scores_backward(op.l_dev[:, k], op.r_dev[:, k], op.g_dev[k:k + 1], hops=[k])
        assert torch.equal(dl[:, k], one[0]) and torch.equal(dr[:, k], one[1]), k


# ------------------------------------------------------------------ 5. symmetric plan
def test_symmetric_plan_equals_built_transposes(cora):
    built = cora.plan(**ADJ)
    shared = cora.plan(symmetric_pattern=True, **ADJ)
    assert shared.transpose_sharing == ["indices", "indices"] and built.transpose_sharing == ["none", "none"]
    want = built.edge_scores_backward(cora.l_dev, cora.r_dev, cora.g_dev)
    got = shared.edge_scores_backward(cora.l_dev, cora.r_dev, cora.g_dev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert equal_lists(shared.edge_scores(cora.l_dev, cora.r_dev), built.edge_scores(cora.l_dev, cora.r_dev))
    one = shared.edge_scores_backward(cora.l_dev[:, 1], cora.r_dev[:, 1], cora.g_dev[1:], hops=[1], need_dl=False)
    assert torch.equal(one[1], want[1][:, 1])


# ------------------------------------------------------------------ 6. non-finite and extreme inputs
def test_non_finite_and_extreme_node_terms(crafted):
    """NaN, +inf + -inf, -inf, subnormals and 1e38 magnitudes in l / r: the forward is torch's, bit for bit; in the backward they
    only choose the branch (a NaN pre takes the slope branch), so the touched rows / columns follow the tree on the same inputs
    and every other element keeps the bits of the clean run."""
    op = crafted
    l, r = op.l.copy(), op.r.copy()
    m0 = op.mats[0]
    i_inf = 2                                                       # (rows of at most 65 entries in every hop: most columns stay clean)
    j_inf = int(m0.indices[m0.indptr[i_inf]])                       # (i_inf, j_inf) is stored in hop 0: -inf + +inf there
    special_rows = {14: np.nan, i_inf: -np.inf, 15: 1e-45, 16: 3e38, 28: -3e38, 29: np.inf}
    special_cols = {j_inf: np.inf, 7: np.nan, 8: -np.inf, 9: 1e-40, 10: 3e38, 11: -3e38}
    for i, v in special_rows.items():
        l[i, :] = v
    for j, v in special_cols.items():
        r[j, :] = v
    l_dev, r_dev = torch.from_numpy(l).to(DEV), torch.from_numpy(r).to(DEV)
    sr, sc = np.array(sorted(special_rows)), np.array(sorted(special_cols))
    want_dl, want_dr = op.tree_bits(0.2, l, r)
    for thr in THRESHOLDS:
        plan = op.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ)
        got = plan.edge_scores(l_dev, r_dev)
        want = op.composite(l_dev, r_dev, 0.2)
        assert any(torch.isnan(t).any() for t in got) and any(torch.isinf(t).any() for t in got)
        for a, b in zip(got, want):
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), thr
        clean = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
        dl, dr = plan.edge_scores_backward(l_dev, r_dev, op.g_dev)
        assert same_bits(dl, want_dl) and same_bits(dr, want_dr), thr
        assert torch.isfinite(dl).all() and torch.isfinite(dr).all()            # g is finite: so is every sum
        for s in range(op.H):
            touched_r = np.isin(np.arange(op.n_rows), sr) | (seg_reduce(np.add, np.isin(op.cols[s], sc).astype(np.float64), op.indptr[s]) > 0)
            touched_c = np.isin(np.arange(op.n_cols), sc) | (seg_reduce(np.add, np.isin(op.rows[s], sr)[op.perm[s]].astype(np.float64), op.t_indptr[s]) > 0)
            assert touched_r.any() and not touched_r.all() and touched_c.any() and not touched_c.all()
            keep_r, keep_c = torch.from_numpy(~touched_r).to(DEV), torch.from_numpy(~touched_c).to(DEV)
            assert torch.equal(dl[keep_r, s], clean[0][keep_r, s]) and torch.equal(dr[keep_c, s], clean[1][keep_c, s]), (thr, s)


def test_non_finite_and_extreme_gradients(crafted):
    """NaN, +inf, -inf, +inf next to -inf, 3e38 + 3e38 and subnormals in g: only the rows / columns whose segments contain such an
    entry change -- they follow the tree on the same inputs, non-finite where the arithmetic says so -- and every other element
    keeps the bits of the clean run."""
    op = crafted
    g = [x.copy() for x in op.g]
    hit = []                                                                     # (hop, entry)
    for s, p in enumerate(op.indptr):
        long_rows = np.flatnonzero(np.diff(p) >= 65)
        short_rows = np.flatnonzero((np.diff(p) >= 2) & (np.diff(p) <= 16))
        for row, vals in ((long_rows[0], (np.nan,)), (long_rows[1], (np.inf, -np.inf)), (long_rows[2], (3e38, 3e38)), (long_rows[3], (-np.inf,)),
                          (short_rows[0], (np.nan,)), (short_rows[1], (np.inf,)), (short_rows[2], (1e-45, -1e-40))):
            for off, v in enumerate(vals):
                e = p[row] + (off * 7) % (p[row + 1] - p[row])
                g[s][e] = v
                hit.append((s, int(e)))
    g_dev = [torch.from_numpy(x).to(DEV) for x in g]
    want_dl, want_dr = op.tree_bits(0.2, g=g)
    for thr in THRESHOLDS:
        plan = op.plan(long_row_threshold=thr, rows_per_wave=4, **ADJ)
        clean = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
        dl, dr = plan.edge_scores_backward(op.l_dev, op.r_dev, g_dev)
        assert same_bits(dl, want_dl) and same_bits(dr, want_dr), thr
        for s in range(op.H):
            entries = np.array([e for k, e in hit if k == s])
            touched_r, touched_c = np.zeros(op.n_rows, bool), np.zeros(op.n_cols, bool)
            touched_r[op.rows[s][entries]] = True
            touched_c[op.cols[s][entries]] = True
            bad = entries[~np.isfinite(g[s][entries])]
            bad_r, bad_c = torch.from_numpy(np.unique(op.rows[s][bad])).to(DEV), torch.from_numpy(np.unique(op.cols[s][bad])).to(DEV)
            assert not torch.isfinite(dl[bad_r, s]).any() and not torch.isfinite(dr[bad_c, s]).any(), (thr, s)
            keep_r, keep_c = torch.from_numpy(~touched_r).to(DEV), torch.from_numpy(~touched_c).to(DEV)
            assert torch.isfinite(dl[keep_r, s]).all() and torch.isfinite(dr[keep_c, s]).all()
            assert torch.equal(dl[keep_r, s], clean[0][keep_r, s]) and torch.equal(dr[keep_c, s], clean[1][keep_c, s]), (thr, s)


# ------------------------------------------------------------------ 7. refusals
def test_refusals(crafted, monkeypatch):
    from h2gcn_amd import _capi
    from h2gcn_amd.layers import hop_edge_scores

    op = crafted
    plan = op.plan(long_row_threshold=32, **ADJ)
    L = _capi.lib()
    calls = []
    real = {n: getattr(L, n) for n in ("h2gcn_edge_scores_hops_f32", "h2gcn_edge_scores_backward_hops_f32")}
    for n in real:
        monkeypatch.setattr(L, n, lambda *a, _n=n: calls.append(_n) or real[_n](*a))
    l, r, g = op.l_dev, op.r_dev, op.g_dev
    bad_nodes = {
        "fp32 only": l.to(torch.bfloat16),
        "must be float32": l.double(),
        "plan on": l.cpu(),
        "must have shape": l[:, :2],
        "must be a tensor": [l],
    }
    for match, arg in bad_nodes.items():
        for fn in (lambda a: plan.edge_scores(a, r), lambda a: plan.edge_scores(l, a), lambda a: hop_edge_scores(plan, a, r),
                   lambda a: plan.edge_scores_backward(a, r, g), lambda a: plan.edge_scores_backward(l, a, g)):
            with pytest.raises(ValueError, match=match):
                fn(arg)
    with pytest.raises(ValueError, match="must have shape"):
        plan.edge_scores(l[:, 0], r[:, 0])                                       # 1-D needs a single selected hop
    with pytest.raises(ValueError, match="must have shape"):
        plan.edge_scores(r, l)                                                   # n_rows != n_cols: swapped operands
    bad_grads = {
        "must list 3 tensors": g[:2],
        "fp32 only": [g[0].to(torch.bfloat16), g[1], g[2]],
        "must have shape": [g[0], g[1][:-1], g[2]],
        "plan on": [g[0].cpu(), g[1], g[2]],
        "must be a sequence": g[0],
    }
    for match, arg in bad_grads.items():
        with pytest.raises(ValueError, match=match):
            plan.edge_scores_backward(l, r, arg)
        if not isinstance(arg, torch.Tensor):
            with pytest.raises(ValueError, match=match):
                plan.edge_scores(l, r, out=arg)
    with pytest.raises(ValueError, match="both False"):
        plan.edge_scores_backward(l, r, g, need_dl=False, need_dr=False)
    with pytest.raises(ValueError, match="hop index 3 outside"):
        plan.edge_scores(l[:, :1], r[:, :1], hops=[3])
    # the column side needs the transposed operands and their permutation; the row side needs neither
    no_perm, no_t = op.plan(long_row_threshold=32, build_transpose=True), op.plan(long_row_threshold=32)
    for p in (no_perm, no_t):
        with pytest.raises(ValueError, match="keep_permutation=True"):
            p.edge_scores_backward(l, r, g)
        with pytest.raises(ValueError, match="keep_permutation=True"):
            hop_edge_scores(p, l, r.clone().requires_grad_(True))
    assert calls == []
    monkeypatch.setattr(_capi, "has", lambda name: "edge_scores" not in name)      # a library that predates the symbols
    with pytest.raises(RuntimeError, match="predates the edge scores"):
        plan.edge_scores(l, r)
    with pytest.raises(RuntimeError, match="predates the edge scores"):
        plan.edge_scores_backward(l, r, g)
    monkeypatch.undo()
    assert calls == []
    want = plan.edge_scores_backward(l, r, g)
    for p in (no_perm, no_t):
        assert equal_lists(p.edge_scores(l, r), plan.edge_scores(l, r))
        dl, dr = p.edge_scores_backward(l, r, g, need_dr=False)
        assert dr is None and torch.equal(dl, want[0])

    # the C calls, all refused before any launch (evaluated one at a time: the error channel holds the last message)
    C = ctypes
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in g])
    holed = (C.c_void_p * 3)(g[0].data_ptr(), None, g[2].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lp, rp = C.c_void_p(l.data_ptr()), C.c_void_p(r.data_ptr())
    dl = torch.full((op.n_rows, 3), 7.0, device=DEV)
    dr = torch.full((op.n_cols, 3), 7.0, device=DEV)
    dlp, drp = C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr())
    fwd, bwd = L.h2gcn_edge_scores_hops_f32, L.h2gcn_edge_scores_backward_hops_f32
    INV, NOT = _capi.ERR_INVALID_ARGUMENT, _capi.ERR_NO_TRANSPOSE
    for fn, handle, args, status, needle in (
            (fwd, plan, (0, lp, 2, rp, 3, 0.2, ptrs), INV, b"ldl"),
            (fwd, plan, (0, lp, 3, rp, 2, 0.2, ptrs), INV, b"ldr"),
            (fwd, plan, (0, None, 3, rp, 3, 0.2, ptrs), INV, b"l is NULL"),
            (fwd, plan, (0, lp, 3, None, 3, 0.2, ptrs), INV, b"r is NULL"),
            (fwd, plan, (0, lp, 3, rp, 3, 0.2, holed), INV, b"scores[1] is NULL"),
            (fwd, plan, (0, lp, 3, rp, 3, 0.2, None), INV, b"scores is NULL"),
            (fwd, plan, (1 << 3, lp, 3, rp, 3, 0.2, ptrs), INV, b"hop"),
            (bwd, plan, (0, lp, 3, rp, 3, 0.2, holed, dlp, 3, drp, 3), INV, b"dscores[1] is NULL"),
            (bwd, plan, (0, lp, 3, rp, 3, 0.2, None, dlp, 3, drp, 3), INV, b"dscores is NULL"),
            (bwd, plan, (0, lp, 3, rp, 3, 0.2, ptrs, None, 3, None, 3), INV, b"dl and dr are both NULL"),
            (bwd, plan, (0, lp, 3, rp, 3, 0.2, ptrs, dlp, 2, drp, 3), INV, b"lddl"),
            (bwd, plan, (0, lp, 3, rp, 3, 0.2, ptrs, dlp, 3, drp, 2), INV, b"lddr"),
            (bwd, plan, (0, lp, 1, rp, 3, 0.2, ptrs, dlp, 3, drp, 3), INV, b"ldl"),
            (bwd, no_perm, (0, lp, 3, rp, 3, 0.2, ptrs, dlp, 3, drp, 3), INV, b"H2GCN_PLAN_KEEP_PERMUTATION"),
            (bwd, no_t, (0, lp, 3, rp, 3, 0.2, ptrs, dlp, 3, drp, 3), NOT, b"H2GCN_PLAN_BUILD_TRANSPOSE")):
        assert fn(handle._handle, *args, stream) == status, needle
        assert needle in L.h2gcn_last_error(), (needle, L.h2gcn_last_error())
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()) and bool((dr == 7.0).all())                   # ... and before the row side ran


# ------------------------------------------------------------------ 8. hipGraph
def test_hipgraph_replay_equals_eager(crafted):
    plan = crafted.plan(long_row_threshold=32, **ADJ)
    l, r = crafted.l_dev.clone(), crafted.r_dev.clone()
    g = [t.clone() for t in crafted.g_dev]
    scores = [torch.empty_like(t) for t in g]
    plan.edge_scores(l, r, out=scores)                                           # one eager launch of each
    first = [t.clone() for t in plan.edge_scores_backward(l, r, g)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.edge_scores(l, r, out=scores)
        dl, dr = plan.edge_scores_backward(l, r, g)
    l.copy_(l.flip(0) * 0.5)                                                     # fresh contents of the static inputs
    r.copy_(r.flip(0) - 0.25)
    for t in g:
        t.copy_(t.flip(0))
    for t in scores + [dl, dr]:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    want_s = plan.edge_scores(l.clone(), r.clone())
    want = plan.edge_scores_backward(l.clone(), r.clone(), [t.clone() for t in g])
    assert equal_lists(scores, want_s) and torch.equal(dl, want[0]) and torch.equal(dr, want[1])
    assert not torch.equal(dl, first[0]) and not torch.equal(dr, first[1])


# ------------------------------------------------------------------ 9. autograd
def test_autograd_is_the_backward_call(crafted, cora, monkeypatch):
    from h2gcn_amd.layers import hop_edge_scores

    for op, plan, what in operands_and_plans(crafted, cora):
        l, r = op.l_dev.clone().requires_grad_(True), op.r_dev.clone().requires_grad_(True)
        scores = hop_edge_scores(plan, l, r)
        assert isinstance(scores, tuple) and len(scores) == op.H and all(s.requires_grad for s in scores)
        assert equal_lists([s.detach() for s in scores], plan.edge_scores(op.l_dev, op.r_dev)), what
        sum((s * g).sum() for s, g in zip(scores, op.g_dev)).backward()
        want = plan.edge_scores_backward(op.l_dev, op.r_dev, op.g_dev)
        assert torch.equal(l.grad, want[0]) and torch.equal(r.grad, want[1]), what
        # the torch composite's own autograd (index_add: atomic, any order) within the bound of the backward's accuracy test
        lc, rc = op.l_dev.clone().requires_grad_(True), op.r_dev.clone().requires_grad_(True)
        sum((s * g).sum() for s, g in zip(op.composite(lc, rc, 0.2), op.g_dev)).backward()
        for s in range(op.H):
            mag = np.abs(op.terms(s, 0.2)[0].astype(np.float64))
            for ours, theirs, t, p in ((l.grad, lc.grad, mag, op.indptr[s]), (r.grad, rc.grad, mag[op.perm[s]], op.t_indptr[s])):
                n = np.diff(p).astype(np.float64)
                bound = gamma(n + 1.0) * seg_reduce(np.add, t, p) + (n + 1.0) * 2.0 ** -149
                assert (np.abs(ours[:, s].double().cpu().numpy() - theirs[:, s].double().cpu().numpy()) <= bound).all(), (what, s)
    # only l (only r) requires a gradient: the other side is not asked for -- None for it; dl needs no transposed operand
    plain, full = crafted.plan(long_row_threshold=32), crafted.plan(long_row_threshold=32, **ADJ)
    want = full.edge_scores_backward(crafted.l_dev, crafted.r_dev, crafted.g_dev)
    asked = []
    for p in (plain, full):
        monkeypatch.setattr(p, "edge_scores_backward", lambda *a, _p=p, **kw: asked.append((kw["need_dl"], kw["need_dr"])) or type(_p).edge_scores_backward(_p, *a, **kw))
    l = crafted.l_dev.clone().requires_grad_(True)
    grads = torch.autograd.grad(hop_edge_scores(plain, l, crafted.r_dev), [l], crafted.g_dev)
    assert torch.equal(grads[0], want[0]) and asked == [(True, False)]
    r = crafted.r_dev.clone().requires_grad_(True)
    grads = torch.autograd.grad(hop_edge_scores(full, crafted.l_dev, r), [r], crafted.g_dev)
    assert torch.equal(grads[0], want[1]) and asked[1:] == [(False, True)]
    monkeypatch.undo()
    # only hop 1 is differentiated through: the others enter as zeros; nothing requires a gradient: a plain launch
    l = crafted.l_dev.clone().requires_grad_(True)
    hop_edge_scores(plain, l, crafted.r_dev)[1].backward(crafted.g_dev[1])
    zeros = [torch.zeros_like(crafted.g_dev[0]), crafted.g_dev[1], torch.zeros_like(crafted.g_dev[2])]
    assert torch.equal(l.grad, plain.edge_scores_backward(crafted.l_dev, crafted.r_dev, zeros, need_dr=False)[0])
    assert not hop_edge_scores(plain, crafted.l_dev, crafted.r_dev)[0].requires_grad


# ------------------------------------------------------------------ 10. HopAttention end to end
def test_hop_attention_end_to_end_on_cora(cora):
    """HopAttention on Cora behind a dense W, the gradients of W, a_l, a_r against a dense fp64 replica (masked dense
    torch.softmax, A @ h) under torch's own autograd: per parameter max|g - g64| / max|g64| may be at most
    max(8 x the same figure of the dense fp32 replica on the same device, 1e-5), and y is within 1e-5 of the replica.  Two
    identical training steps from the same seed give bit-equal parameters (no atomics anywhere in the chain).
    Measured on the MI355X: W 5.4e-7 (replica 5.1e-7), a_l 5.3e-7 (2.2e-7), a_r 6.0e-7 (6.0e-7); max|y - y64| 6.7e-7."""
    from h2gcn_amd import HopAttention

    mats = cora.mats
    n, f, d = mats[0].shape[0], 48, 16
    plan = cora.plan(**ADJ)
    gen = torch.Generator().manual_seed(10)
    X0 = (torch.rand((n, f), generator=gen) * 2 - 1).to(DEV)
    R = (torch.rand((n, 2, d), generator=gen) * 2 - 1).to(DEV)
    W0 = ((torch.rand((f, d), generator=gen) * 2 - 1) * 0.3).to(DEV)
    torch.manual_seed(11)
    layer = HopAttention(d).to(DEV)
    assert tuple(layer.a_l.shape) == (2, d) and layer.a_l.device.type == "cuda"
    init = [W0, layer.a_l.detach().clone(), layer.a_r.detach().clone()]

    W = W0.clone().requires_grad_(True)
    y = layer(plan, X0 @ W)
    assert tuple(y.shape) == (n, 2, d)
    (y * R).sum().backward()
    got = [W.grad, layer.a_l.grad, layer.a_r.grad]

    def replica(dtype):
        Wd, ld, rd = (t.to(dtype).clone().requires_grad_(True) for t in init)
        hd = X0.to(dtype) @ Wd
        ys = []
        for s, (r, c) in enumerate(zip(cora.rows_dev, cora.cols_dev)):
            e = torch.nn.functional.leaky_relu((hd @ ld[s])[:, None] + (hd @ rd[s])[None, :], 0.2)
            mask = torch.zeros((n, n), dtype=torch.bool, device=DEV).index_put((r, c), torch.ones((), dtype=torch.bool, device=DEV))
            # (a row without entries keeps its finite scores: an all -inf row would be NaN, also in the backward; it is zeroed next)
            A = torch.softmax(e.masked_fill(~mask & mask.any(dim=1, keepdim=True), float("-inf")), dim=1)
            A = torch.where(mask, A, torch.zeros((), dtype=dtype, device=DEV))
            ys.append(A @ hd)
        yd = torch.stack(ys, dim=1)
        (yd * R.to(dtype)).sum().backward()
        return yd.detach(), [Wd.grad, ld.grad, rd.grad]

    (y64, g64), (y32, g32) = replica(torch.float64), replica(torch.float32)
    err_y = float((y.detach().double() - y64).abs().max())
    print(f"y: max|y - y64| = {err_y:.3e} (max|y64| = {float(y64.abs().max()):.3f}); dense fp32 replica {float((y32.double() - y64).abs().max()):.3e}")
    assert err_y <= 1e-5
    for name, g, r64, r32 in zip(("W", "a_l", "a_r"), got, g64, g32):
        scale = float(r64.abs().max())
        ours, theirs = float((g.double() - r64).abs().max()) / scale, float((r32.double() - r64).abs().max()) / scale
        print(f"d{name}: max|g - g64| / max|g64| = {ours:.3e}; dense fp32 replica {theirs:.3e}")
        assert ours <= max(8.0 * theirs, 1e-5), (name, ours, theirs)

    def train():
        torch.manual_seed(11)
        net = HopAttention(d).to(DEV)
        Wt = W0.clone().requires_grad_(True)
        opt = torch.optim.SGD([Wt, *net.parameters()], lr=0.05)
        for _ in range(2):
            opt.zero_grad()
            (net(plan, X0 @ Wt) * R).sum().backward()
            opt.step()
        return [Wt.detach().clone()] + [p.detach().clone() for p in net.parameters()]

    a, b = train(), train()
    assert all(not torch.equal(p, q) for p, q in zip(a, init))                    # the steps moved every parameter
    assert all(torch.equal(p, q) for p, q in zip(a, b))

    # a hop subset: the layer's single hop is hop 1 of the plan
    torch.manual_seed(12)
    one = HopAttention(d, hops=[1]).to(DEV)
    h = (X0 @ W0).requires_grad_(True)
    y1 = one(plan, h)
    assert tuple(y1.shape) == (n, 1, d)
    y1.sum().backward()
    assert one.a_l.grad is not None and one.a_r.grad is not None and h.grad is not None
    with pytest.raises(ValueError, match="hops"):
        HopAttention(d, n_hops=3)(plan, h)
    with pytest.raises(ValueError, match="keep_permutation=True"):
        layer(cora.plan(build_transpose=True), h)
