"""GPU suite: HopPlan.select_rows -- the hop matrices restricted to a set of rows, built on the device.

Operand: two hop matrices of 203 rows with empty rows (rows 5, 100 and the last row have no nonzero in either hop, rows 0 and 50..59
none in hop 1).  Every selection holds an empty row, row 0 and the last row; one selection has no nonzero at all in hop 1.

Tolerances: the sub-plan's launches are torch.equal to those of a plan built from scipy's A_k[rows] (same operands -> same
canonical summation tree); against the fp64 scipy product the adjoint is within the 1e-5 the spmm suite asserts for inputs
in [-1, 1]; in bf16 the fp32 result equals the launch on the upcast operand bit for bit (the bf16 suite's rule)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 203


def _hops():
    hops = []
    for k, dens in enumerate((0.02, 0.08)):
        m = sp.random(N, N, dens, format="lil", random_state=10 + k, dtype=np.float32)
        for r in (5, 100, N - 1):
            m[r, :] = 0
        if k == 1:
            m[50:60, :] = 0
        m = sp.csr_matrix(m)
        m.eliminate_zeros()
        m.sort_indices()
        hops.append(m.astype(np.float32))
    return hops


def _selections(hops):
    rng = np.random.default_rng(0)
    some = np.sort(np.concatenate([[0, 5, N - 1], rng.choice(np.setdiff1d(np.arange(1, N - 1), [5]), 40, replace=False)]))
    mask = np.zeros(N, dtype=bool)
    mask[some] = True
    return {"index list": some, "bool mask": mask, "everything": np.arange(N), "no nonzero in hop 1": None}


@pytest.fixture(scope="module")
def operand():
    from h2gcn_amd import HopPlan
    hops = _hops()
    # the selection without a nonzero in hop 1: empty rows of hop 1 only (row 0 and the last row included, so empty them there too)
    h1 = sp.lil_matrix(hops[1])
    h1[0, :] = 0
    hops[1] = sp.csr_matrix(h1)
    hops[1].eliminate_zeros()
    plan = HopPlan.from_scipy(hops, DEV, build_transpose=True)
    return hops, plan


def _rows_of(name, sel_np):
    if name == "no nonzero in hop 1":
        return np.array([0, 5] + list(range(50, 60)) + [100, N - 1])
    return np.flatnonzero(sel_np) if sel_np.dtype == bool else sel_np


@pytest.mark.parametrize("name", ["index list", "bool mask", "everything", "no nonzero in hop 1"])
def test_sub_plan_equals_a_plan_built_from_the_sub_matrices(operand, name):
    from h2gcn_amd import HopPlan
    hops, plan = operand
    sel_np = _selections(hops)[name]
    rows = _rows_of(name, sel_np)
    arg = torch.from_numpy(sel_np).to(DEV) if name == "bool mask" else torch.from_numpy(rows[::-1].copy())   # unsorted input is sorted
    sel = plan.select_rows(arg, build_transpose=True)
    m = len(rows)
    assert sel.rows.dtype == torch.int32 and sel.rows.device.type == "cuda" and np.array_equal(sel.rows.cpu().numpy(), rows)
    assert sel.n_rows_full == N and len(sel) == m
    assert (sel.plan.n_rows, sel.plan.n_cols, sel.plan.n_hops, sel.plan.has_transpose) == (m, N, 2, True)
    subs = [sp.csr_matrix(h[rows]) for h in hops]
    if name == "no nonzero in hop 1":
        assert subs[1].nnz == 0 and subs[0].nnz > 0
    for k, sub in enumerate(subs):   # indptr, indices, data: bit for bit
        assert np.array_equal(sel.plan.rowptr[k].cpu().numpy(), sub.indptr.astype(np.int64))
        assert np.array_equal(sel.plan.colidx[k].cpu().numpy(), sub.indices.astype(np.int32))
        assert np.array_equal(sel.plan.vals[k].cpu().numpy().view(np.int32), sub.data.astype(np.float32).view(np.int32))
    ref = HopPlan.from_scipy(subs, DEV, build_transpose=True)
    rng = np.random.default_rng(1)
    for d in (64, 7):
        x = torch.from_numpy(rng.uniform(-1, 1, (N, d)).astype(np.float32)).to(DEV)
        g = torch.from_numpy(rng.uniform(-1, 1, (m, 2, d)).astype(np.float32)).to(DEV)
        assert torch.equal(sel.plan.spmm(x), ref.spmm(x))
        got_t = sel.plan.spmm_t(g)
        assert torch.equal(got_t, ref.spmm_t(g))
        gn = g.cpu().numpy().astype(np.float64)
        want = sum(subs[k].astype(np.float64).T @ gn[:, k, :] for k in range(2))
        assert np.abs(got_t.cpu().numpy() - want).max() <= 1e-5
    # bf16: an fp32 result equals the launch on the upcast operand bit for bit
    gb = torch.from_numpy(rng.uniform(-1, 1, (m, 2, 64)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    got_b = sel.plan.spmm_t(gb, out_dtype=torch.float32)
    assert torch.equal(got_b, sel.plan.spmm_t(gb.float()))
    want = sum(subs[k].astype(np.float64).T @ gb.float().cpu().numpy().astype(np.float64)[:, k, :] for k in range(2))
    assert np.abs(got_b.cpu().numpy() - want).max() <= 1e-5
    xb = torch.from_numpy(rng.uniform(-1, 1, (N, 64)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    assert torch.equal(sel.plan.spmm(xb, out_dtype=torch.float32), sel.plan.spmm(xb.float()))


def test_refusals_and_no_transpose(operand):
    _, plan = operand
    with pytest.raises(ValueError, match="duplicate row indices"):
        plan.select_rows(torch.tensor([3, 7, 3]))
    with pytest.raises(ValueError, match=r"outside \[0, 203\)"):
        plan.select_rows(torch.tensor([0, N]))
    with pytest.raises(ValueError, match=r"outside \[0, 203\)"):
        plan.select_rows(torch.tensor([-1, 4]))
    with pytest.raises(ValueError, match="empty selection"):
        plan.select_rows(torch.zeros(N, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="empty selection"):
        plan.select_rows(torch.zeros(0, dtype=torch.int64))
    sel = plan.select_rows([1, 2], build_transpose=False)
    assert not sel.plan.has_transpose
    with pytest.raises(ValueError, match="build_transpose"):
        sel.plan.spmm_t(torch.zeros((2, 2, 8), device=DEV))
