"""GPU suite: symmetric hop plans -- HopPlan(build_transpose=True, symmetric_pattern=True) runs the adjoint on the forward arrays
(H2GCN_PLAN_SYMMETRIC_PATTERN; the mirror pass of csrc/symmetric.hip verifies the pattern and produces the transposed values).

Everything is compared with the plan that builds its transposes, with torch.equal: the adjoint's arrays must hold exactly what
the radix transposition produces, so no tolerance applies.  Operand sets:
  (a) Cora's exact-1-hop / exact-2-hop rings, SYM values (bit-symmetric: indices and values are shared);
  (b) the same patterns with the RW values (pattern-symmetric only: indices are shared);
  (c) a synthetic symmetrised pattern, n = 1500, 3 hops: ~10 % empty rows, rows of length 1, diagonal entries (an entry that is
      its own mirror), hubs longer than long_row_threshold = 32 (the 4-wave LDS path and the binned lists both occur), nnz not a
      multiple of 256, signed non-symmetric values; hops 0 / 1 average < 32 nonzeros per row and hop 2 more, so both lane-group
      widths of the mirror kernel run.
"""
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_planetoid_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SYN = 1500
LONG = 32


def _synthetic_hop(rng, n, mean_deg, n_hubs):
    """One symmetric pattern with the properties listed in the module docstring; values signed and not symmetric."""
    perm = rng.permutation(n)
    empty, pendant, hubs, lone_diag = perm[:150], perm[150:260], perm[260:260 + n_hubs], perm[270:290]
    rest = perm[290:]
    m = sp.random(n, n, density=mean_deg / (2.0 * n), random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="coo")
    a = sp.csr_matrix((np.ones(m.nnz), (m.row, m.col)), shape=(n, n))
    a = sp.lil_matrix(((a + a.T) > 0).astype(np.float32))
    for group in (empty, pendant, lone_diag):
        a[group, :] = 0
        a[:, group] = 0
    for h in hubs:                                       # rows (and columns) well beyond the long-row threshold
        nb = rng.choice(rest, size=int(rng.integers(LONG + 8, 5 * LONG)), replace=False)
        a[h, nb] = 1
        a[nb, h] = 1
    for p in pendant:                                    # rows of length 1: one off-diagonal entry
        q = int(rng.choice(rest))
        a[p, q] = 1
        a[q, p] = 1
    for i in lone_diag:                                  # rows of length 1: the diagonal entry alone
        a[i, i] = 1
    for i in rest[:40]:                                  # diagonal entries inside ordinary rows
        a[i, i] = 1
    a = sp.csr_matrix(a)
    a.eliminate_zeros()
    if a.nnz % 256 == 0:
        a = sp.lil_matrix(a)
        a[rest[41], rest[41]] = 1
        a = sp.csr_matrix(a)
    a.sort_indices()
    a.data = rng.standard_normal(a.nnz).astype(np.float32)
    a.data[a.data == 0] = 1.0
    return a


@pytest.fixture(scope="module")
def operand_sets():
    g = load_planetoid_golden("cora")
    rng = np.random.default_rng(20)
    syn = [_synthetic_hop(rng, N_SYN, 6, 4), _synthetic_hop(rng, N_SYN, 14, 6), _synthetic_hop(rng, N_SYN, 64, 5)]
    for k, a in enumerate(syn):
        lens = np.diff(a.indptr)
        pat = sp.csr_matrix((np.ones(a.nnz, np.int8), a.indices, a.indptr), shape=a.shape)
        assert (pat != pat.T).nnz == 0 and (a != a.T).nnz > 0                # symmetric in pattern, not in value
        assert 0.08 * N_SYN <= (lens == 0).sum() <= 0.12 * N_SYN and (lens == 1).sum() >= 50 and (lens > LONG).sum() >= 4
        assert a.diagonal().astype(bool).sum() >= 40 and a.nnz % 256 != 0
        assert (a.nnz < 32 * N_SYN) == (k < 2)                               # hops 0, 1: 16-lane groups; hop 2: whole waves
    return {"a": [g["hop1_sym"], g["hop2_sym"]], "b": [g["hop1_rw"], g["hop2_rw"]], "c": syn}


def _plans(mats, **kw):
    from h2gcn_amd import HopPlan
    sym = HopPlan.from_scipy(mats, DEV, build_transpose=True, symmetric_pattern=True, **kw)
    ref = HopPlan.from_scipy(mats, DEV, build_transpose=True, **kw)
    return sym, ref


def _kw(name):
    return dict(long_row_threshold=LONG) if name == "c" else {}


def _rand(shape, seed, dtype=torch.float32):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=gen) * 2 - 1).to(DEV).to(dtype)


def _sharing_bound(mats, per_nnz):
    return sum(per_nnz * m.nnz + 8 * (m.shape[0] + 1) for m in mats)


# ---------------------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("variant", [0, 3, 6])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_adjoint_and_forward_bits_equal_the_transposed_plan(operand_sets, name, variant):
    mats = operand_sets[name]
    P, T = _plans(mats, variant=variant, **_kw(name))
    n, H = P.n_rows, P.n_hops
    assert P.info(0)["has_transpose"] and P.has_transpose
    subsets = [[0], [1]] + ([[0, 2]] if H > 2 else [])
    for d in (1, 7, 64, 130):
        g = _rand((n, H, d), 100 + d)
        assert torch.equal(P.spmm_t(g), T.spmm_t(g)), (name, variant, d)
        assert P.schedule(d, adjoint=True) == T.schedule(d, adjoint=True), d
        assert P.segment_classes(d, adjoint=True) == T.segment_classes(d, adjoint=True), d
        for hops in subsets:
            gs = _rand((n, len(hops), d), 200 + d)
            assert torch.equal(P.spmm_t(gs, hops=hops), T.spmm_t(gs, hops=hops)), (name, variant, d, hops)
            assert P.schedule(d, hops=hops, adjoint=True) == T.schedule(d, hops=hops, adjoint=True)
            assert P.segment_classes(d, hops=hops, adjoint=True) == T.segment_classes(d, hops=hops, adjoint=True)
        x = _rand((n, d), 300 + d)
        assert torch.equal(P.spmm(x), T.spmm(x)), (name, variant, d)
        # a strided gradient (a slice of a wider buffer) and the accumulating store
        wide = _rand((n, H, d + 8), 400 + d)
        gv = wide[:, :, :d]
        assert torch.equal(P.spmm_t(gv), T.spmm_t(gv)), (name, variant, d)
        base = _rand((n, d), 500 + d)
        out_p, out_t = base.clone(), base.clone()
        P.spmm_t(g, out=out_p, accumulate=True)
        T.spmm_t(g, out=out_t, accumulate=True)
        assert torch.equal(out_p, out_t), (name, variant, d)
    for d in (2, 64, 130):
        g = _rand((n, H, d), 600 + d, torch.bfloat16)
        for out_dtype in (torch.float32, torch.bfloat16):
            assert torch.equal(P.spmm_t(g, out_dtype=out_dtype), T.spmm_t(g, out_dtype=out_dtype)), (name, variant, d, out_dtype)
            for hops in subsets:
                gs = g[:, :len(hops)].contiguous()
                assert torch.equal(P.spmm_t(gs, hops=hops, out_dtype=out_dtype), T.spmm_t(gs, hops=hops, out_dtype=out_dtype))
        x = _rand((n, d), 700 + d, torch.bfloat16)
        assert torch.equal(P.spmm(x, out_dtype=torch.float32), T.spmm(x, out_dtype=torch.float32))


def test_the_synthetic_operand_takes_the_long_and_the_listed_paths(operand_sets):
    P, _ = _plans(operand_sets["c"], **_kw("c"))
    cls = P.segment_classes(64, adjoint=True)
    assert all(h["segments"]["long"] >= 4 for h in cls["per_hop"])
    assert P.schedule(64, adjoint=True)["segment_walk"].startswith("lane group per segment (binned")


# ------------------------------------------------------------------------------------------------- 2. sharing and memory
def test_sharing_and_owned_bytes(operand_sets):
    a, b, c = operand_sets["a"], operand_sets["b"], operand_sets["c"]
    P, T = _plans(a)
    assert P.transpose_sharing == ["indices+values"] * 2 and T.transpose_sharing == ["none"] * 2
    print(f"(a) device_bytes: transposed {T.device_bytes()}  symmetric {P.device_bytes()}  bound {_sharing_bound(a, 8)}")
    assert T.device_bytes() - P.device_bytes() >= _sharing_bound(a, 8)
    for name, mats in (("b", b), ("c", c)):
        P, T = _plans(mats, **_kw(name))
        assert P.transpose_sharing == ["indices"] * len(mats), name
        print(f"({name}) device_bytes: transposed {T.device_bytes()}  symmetric {P.device_bytes()}  bound {_sharing_bound(mats, 4)}")
        assert T.device_bytes() - P.device_bytes() >= _sharing_bound(mats, 4), name
    P, T = _plans(a, keep_permutation=True)
    assert P.transpose_sharing == ["indices"] * 2
    assert T.device_bytes() - P.device_bytes() >= _sharing_bound(a, 4)           # both keep 8 B per nonzero: t_vals and perm
    # a plan without transposes owns no transposed bytes and shares nothing
    from h2gcn_amd import HopPlan
    assert HopPlan.from_scipy(a, DEV).transpose_sharing == ["none"] * 2


@pytest.mark.parametrize("hop", [0, 1])
def test_one_ulp_on_one_side_of_a_pair_unshares_the_values_of_that_hop_only(operand_sets, hop):
    mats = [m.copy() for m in operand_sets["a"]]
    m = mats[hop]
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    e = int(np.flatnonzero(rows != m.indices)[len(m.data) // 3])                 # an off-diagonal entry
    m.data[e] = np.nextafter(m.data[e], np.float32(np.inf), dtype=np.float32)
    P, T = _plans(mats)
    want = ["indices+values"] * 2
    want[hop] = "indices"
    assert P.transpose_sharing == want
    g = _rand((P.n_rows, 2, 64), 11)
    assert torch.equal(P.spmm_t(g), T.spmm_t(g))
    assert not torch.equal(P.spmm_t(g), _plans(operand_sets["a"])[0].spmm_t(g))   # (the ulp is visible in the result)


# ------------------------------------------------------------------------------------------------------- 3. set_values
def test_set_values(operand_sets):
    from h2gcn_amd import _capi
    a = operand_sets["a"]
    P, T = _plans(a, keep_permutation=True)
    g = _rand((P.n_rows, 2, 64), 12)
    assert torch.equal(P.spmm_t(g), T.spmm_t(g))
    new = _rand((a[1].nnz,), 13)                                                  # signed, not symmetric
    P.set_values(1, new)
    T.set_values(1, new)
    assert P.transpose_sharing == ["indices"] * 2
    assert torch.equal(P.spmm_t(g), T.spmm_t(g))
    assert torch.equal(P.spmm_t(g[:, 1:].contiguous(), hops=[1]), T.spmm_t(g[:, 1:].contiguous(), hops=[1]))
    x = _rand((P.n_rows, 64), 14)
    assert torch.equal(P.spmm(x), T.spmm(x))
    # without the permutation: refused exactly as on a plan with built transposes
    P2, T2 = _plans(a)
    msgs = []
    for plan in (P2, T2):
        with pytest.raises(_capi.H2GCNError) as ei:
            plan.set_values(1, new)
        assert ei.value.status == _capi.ERR_INVALID_ARGUMENT
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] and "H2GCN_PLAN_KEEP_PERMUTATION" in msgs[0]
    assert torch.equal(P2.spmm_t(g), T2.spmm_t(g))                                # ... and left as it was


# --------------------------------------------------------------------------------------------------------- 4. refusals
def _drop_mirror(m, which):
    """Remove entry (c, r), the mirror of the `which`-th off-diagonal entry (r, c); returns the matrix and (r, c)."""
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    e = int(np.flatnonzero(rows != m.indices)[which])
    r, c = int(rows[e]), int(m.indices[e])
    out = sp.lil_matrix(m)
    out[c, r] = 0
    out = sp.csr_matrix(out)
    out.eliminate_zeros()
    out.sort_indices()
    assert out.nnz == m.nnz - 1
    return out, (r, c)


def _first_unmirrored(m):
    """The (row, col) that comes first in (row, col) order among the stored entries whose mirror is not stored (CPU)."""
    pat = sp.csr_matrix((np.ones(m.nnz, np.int8), m.indices, m.indptr), shape=m.shape)
    lone = sp.coo_matrix(pat - pat.multiply(pat.T))
    lone.eliminate_zeros()
    return min(zip(lone.row.tolist(), lone.col.tolist()))


def test_a_missing_mirror_is_refused_with_the_first_offending_entry(operand_sets):
    from h2gcn_amd import HopPlan, _capi
    c = operand_sets["c"]
    broken1, rc1 = _drop_mirror(c[1], 5000)
    twice1, rc1b = _drop_mirror(broken1, 700)           # two lone entries in hop 1: the earlier one is named
    broken2, _ = _drop_mirror(c[2], 10)                 # (an earlier (row, col) than hop 1's, in a later hop)
    assert _first_unmirrored(broken1) == rc1 and _first_unmirrored(twice1) == min(rc1, rc1b) == rc1b
    for mats, want in (([c[0], broken1, c[2]], rc1), ([c[0], broken1, broken2], rc1), ([c[0], twice1, broken2], rc1b)):
        with pytest.raises(_capi.H2GCNError) as ei:
            HopPlan.from_scipy(mats, DEV, build_transpose=True, symmetric_pattern=True, long_row_threshold=LONG)
        assert ei.value.status == _capi.ERR_BAD_INDEX
        got = re.search(r"hop (\d+): entry \((\d+), (\d+)\) has no mirror entry \((\d+), (\d+)\): pattern not symmetric", str(ei.value))
        assert got, str(ei.value)
        assert tuple(int(v) for v in got.groups()) == (1, want[0], want[1], want[1], want[0])
    # nothing is left behind: a valid creation and its launches follow
    P, T = _plans(c, **_kw("c"))
    g = _rand((N_SYN, 3, 64), 15)
    assert torch.equal(P.spmm_t(g), T.spmm_t(g))
    # the transposed plan takes the broken operand as before
    assert HopPlan.from_scipy([c[0], broken1, c[2]], DEV, build_transpose=True).transpose_sharing == ["none"] * 3


def test_unsupported_combinations_are_refused(operand_sets):
    from h2gcn_amd import HopPlan
    a = operand_sets["a"]
    with pytest.raises(ValueError, match="square"):
        HopPlan.from_scipy([m[:100, :] for m in a], DEV, build_transpose=True, symmetric_pattern=True)
    with pytest.raises(ValueError, match="host_transpose"):
        HopPlan.from_scipy(a, DEV, build_transpose=True, host_transpose=True, symmetric_pattern=True)
    with pytest.raises(ValueError, match="build_transpose"):
        HopPlan.from_scipy(a, DEV, symmetric_pattern=True)
    P, T = _plans(a)
    g = _rand((P.n_rows, 2, 7), 16)
    assert torch.equal(P.spmm_t(g), T.spmm_t(g))


def test_unsorted_columns_are_refused(operand_sets):
    """The mirror search relies on ascending columns: an operand whose rows are not in that order is refused, not searched."""
    from h2gcn_amd import HopPlan, _capi
    m = operand_sets["a"][0]
    lens = np.diff(m.indptr)
    r = int(np.flatnonzero(lens >= 2)[0])
    ci = m.indices.astype(np.int32).copy()
    b = int(m.indptr[r])
    ci[b], ci[b + 1] = ci[b + 1], ci[b]
    t = [torch.from_numpy(v).to(DEV) for v in (m.indptr.astype(np.int64), ci, m.data.astype(np.float32))]
    with pytest.raises(_capi.H2GCNError, match="not strictly ascending") as ei:
        HopPlan([t[0]], [t[1]], [t[2]], m.shape[1], build_transpose=True, symmetric_pattern=True)
    assert ei.value.status == _capi.ERR_BAD_INDEX


# ------------------------------------------------------------------------------------------------------ 5. select_rows
def test_select_rows_builds_its_own_transpose(operand_sets):
    P, T = _plans(operand_sets["a"])
    rows = torch.arange(0, P.n_rows, 19, device=DEV)
    sel_p, sel_t = P.select_rows(rows), T.select_rows(rows)
    assert sel_p.plan.transpose_sharing == ["none"] * 2
    assert sel_p.plan.device_bytes() == sel_t.plan.device_bytes() > 0
    g = _rand((len(sel_p), 2, 64), 17)
    assert torch.equal(sel_p.plan.spmm_t(g), sel_t.plan.spmm_t(g))
