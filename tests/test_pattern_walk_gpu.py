"""GPU suite: the frame shared by the kernels that walk the CSR pattern of the selected hops (csrc/pattern_walk.hip.h: the
block -> long segment / row tile map, the wave-wide row-pointer load, the launch geometry), driven through both of them --
HopPlan.sddmm (d = 4 and d = 130) and HopPlan.row_softmax / row_softmax_backward.  The per-kernel suites reach it with 3 hops;
here are its edges:

  * H2GCN_MAX_HOPS = 8 hops at rows_per_wave = 7: (7 + 1) * 8 = 64, every lane of the row-pointer load in use; n_rows = 29 is one
    full tile of 28 rows plus one row (the clamp at n_rows), and 2 tiles on 8 XCDs leave most blocks of the tile map empty.
    Segment lengths cycle through 0, 1, 16, 17, 64, 65, each hop one step further, so with long_row_threshold = 32 every row
    holds long and regular segments;
  * a plan whose every non-empty segment is long (long_row_threshold = 1): the tile walk writes nothing, the long blocks
    everything;
  * n_rows = 1, one selected hop of a three-hop plan (a long segment, an empty hop, a single entry).

No tolerance anywhere: both kernels document that their bits do not depend on the schedule, so every result is torch.equal to the
same hops launched ONE AT A TIME, each from a plan of its own at rows_per_wave = 1.  Outputs start as NaN: an entry nobody wrote
fails the comparison.  That the crafted patterns build (n_cols >= 65, distinct ascending columns) is checked without a GPU.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

DEV = "cuda:0"
LENGTHS = (0, 1, 16, 17, 64, 65)
N_COLS = 80
WIDTHS = (4, 130)


def crafted_hops(n_hops, n_rows, first, seed):
    """n_hops CSR matrices [n_rows, N_COLS]: row i of hop k has LENGTHS[(first + i + k) % 6] entries in distinct ascending columns."""
    assert N_COLS >= max(LENGTHS)
    rng = np.random.default_rng(seed)
    mats = []
    for k in range(n_hops):
        lens = [LENGTHS[(first + i + k) % len(LENGTHS)] for i in range(n_rows)]
        rows = [np.sort(rng.choice(N_COLS, size=n, replace=False)) for n in lens]
        assert all(bool((np.diff(r) > 0).all()) for r in rows)
        indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        mats.append(sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_rows, N_COLS)))
    return mats


class Case:
    """Hop matrices, the operands of both kernels and the reference, computed once and never changed."""

    def __init__(self, n_hops, n_rows, first, seed):
        from h2gcn_amd import HopPlan

        self.mats = crafted_hops(n_hops, n_rows, first, seed)
        self.lens = [np.diff(m.indptr) for m in self.mats]
        gen = torch.Generator().manual_seed(seed)
        nnz = [m.nnz for m in self.mats]
        self.g = {d: (torch.rand((n_rows, n_hops, d), generator=gen) * 2 - 1).to(DEV) for d in WIDTHS}
        self.x = {d: (torch.rand((N_COLS, d), generator=gen) * 2 - 1).to(DEV) for d in WIDTHS}
        self.scores = [(4.0 * torch.randn(z, generator=gen)).to(DEV) for z in nnz]
        self.grads = [(torch.rand(z, generator=gen) * 2 - 1).to(DEV) for z in nnz]
        alone = [self.run(HopPlan.from_scipy([m], DEV, long_row_threshold=32, rows_per_wave=1), [k], alone=True)
                 for k, m in enumerate(self.mats)]
        self.ref = {name: [r[name][0] for r in alone] for name in alone[0]}

    def plan(self, **kw):
        from h2gcn_amd import HopPlan

        return HopPlan.from_scipy(self.mats, DEV, **kw)

    def run(self, plan, hops, alone=False):
        """Every pattern kernel on hops `hops` of the case (alone: `plan` holds just that hop) -> name -> one [nnz_k] tensor per hop."""
        sel = None if alone else hops

        def blank():
            return [torch.full((self.mats[k].nnz,), float("nan"), device=DEV) for k in hops]

        res = {f"sddmm d={d}": plan.sddmm(self.g[d][:, hops, :], self.x[d], hops=sel, out=blank()) for d in WIDTHS}
        res["softmax"] = plan.row_softmax([self.scores[k] for k in hops], hops=sel, out=blank())
        res["softmax backward"] = plan.row_softmax_backward(res["softmax"], [self.grads[k] for k in hops], hops=sel, out=blank())
        torch.cuda.synchronize()
        return res

    def assert_equal(self, res, hops, what):
        for name, tensors in res.items():
            for s, k in enumerate(hops):
                assert torch.equal(tensors[s], self.ref[name][k]), (what, name, f"hop {k}")


def test_crafted_patterns_build():
    for n_hops, n_rows, first, seed in ((8, 29, 0, 15), (3, 1, 5, 16)):      # the cases of the GPU tests below
        for k, m in enumerate(crafted_hops(n_hops, n_rows, first, seed)):
            assert m.shape == (n_rows, N_COLS) and N_COLS >= 65 and m.has_canonical_format
            assert np.diff(m.indptr).tolist() == [LENGTHS[(first + i + k) % 6] for i in range(n_rows)]


@pytest.fixture(scope="module")
def eight():
    return Case(8, 29, 0, 15)


@pytest.mark.gpu
def test_full_lane_row_pointer_load(eight):
    hops = list(range(8))
    plan = eight.plan(long_row_threshold=32, rows_per_wave=7)
    for k in hops:      # long and regular segments in every hop
        n_long = int((eight.lens[k] >= 32).sum())
        assert plan.info(k)["n_long_segments"] == n_long and 0 < n_long < int((eight.lens[k] > 0).sum())
    eight.assert_equal(eight.run(plan, hops), hops, "8 hops, rows_per_wave=7")
    for k in hops:      # (the reference is not empty-handed: a softmax over one entry is exactly 1)
        single = torch.from_numpy(np.repeat(eight.lens[k] == 1, eight.lens[k])).to(DEV)
        assert bool(single.any()) and bool((eight.ref["softmax"][k][single] == 1.0).all())


@pytest.mark.gpu
def test_every_segment_long(eight):
    hops = list(range(8))
    all_long, none_long = eight.plan(long_row_threshold=1, rows_per_wave=7), eight.plan()
    for k in hops:
        assert all_long.info(k)["n_long_segments"] == int((eight.lens[k] > 0).sum())
        assert none_long.info(k)["n_long_segments"] == 0
    res_long, res_none = eight.run(all_long, hops), eight.run(none_long, hops)
    for name in res_long:
        for k in hops:
            assert torch.equal(res_long[name][k], res_none[name][k]), (name, f"hop {k}")
    eight.assert_equal(res_long, hops, "every segment long")


@pytest.mark.gpu
def test_one_row_one_selected_hop():
    case = Case(3, 1, 5, 16)
    assert [int(n[0]) for n in case.lens] == [65, 0, 1]
    for kw in (dict(), dict(long_row_threshold=32), dict(long_row_threshold=32, rows_per_wave=7)):
        plan = case.plan(**kw)
        for k in range(3):
            case.assert_equal(case.run(plan, [k]), [k], f"n_rows = 1, {kw}")
