"""GPU suite: boundary sweep of the ring set kernels and the pattern normalisation (csrc/rings.hip) against Python sets, through
tests/ring_driver.py -- a 0xFF scratch before every call, sentinels around every output, out-of-range entries behind every input,
every call pair made twice.  Integers: every comparison is exact.

Wide mode (level 0 of the bitmap in global slabs, rows <= 1024 candidates on the sorted-candidate kernel) needs n >= 131073 but no
nonzeros to speak of, and the row-window entry points evaluate only the rows they are given: every boundary is a hand-built window
of a few hundred rows over a nearly empty A.  tests/test_ring_driver.py asserts on the CPU that the lists contain what they claim."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import ring_driver as rd
from h2gcn_amd import _capi
from h2gcn_amd import operands as po
from oracle import operands as oo

pytestmark = pytest.mark.gpu
DEV = rd.DEV


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ a. candidate counts, wide mode
@pytest.mark.parametrize("add_diag", [False, True])
@pytest.mark.parametrize("at_end", [False, True])
def test_candidate_count_edges_wide(at_end, add_diag):
    """n = 131073; ONE window holds every row shape of ring_driver.WIDE_SHAPES x duplicate structure -- sorted-kernel rows of every
    sort size and bitmap-kernel rows (the device-built big_rows list) in one launch -- with no SUB, a SUB that removes the first,
    last and a middle survivor, a SUB that removes everything, and sub_diag where the diagonal is a candidate and where it is not;
    the window at row 0 and ending at row n - 1."""
    for case in rd.wide_cases(at_end, add_diag):
        rd.run(case)


# ------------------------------------------------------------------------------------------------ b. the kernel hand-over
@pytest.mark.parametrize("builder", ["add", "frontier"])
@pytest.mark.parametrize("lo", [1023, 1024])
def test_kernel_hand_over_1024_1025(lo, builder):
    """The same final set from c = lo, lo + 1, lo + 2 candidates (one more duplicate each): 1024 is the last row of the sorted
    kernel, 1025 the first of the bitmap kernel; identical output rows."""
    case = rd.hand_over_case(rd.WIDE_N, lo, builder)
    assert rd.candidates(case) == [lo, lo + 1, lo + 2]
    rowptr, colidx = rd.run(case)
    rows = [colidx[rowptr[i]:rowptr[i + 1]].tolist() for i in range(3)]
    assert rows[0] == rows[1] == rows[2] and len(rows[0]) == 700


# ------------------------------------------------------------------------------------------------ c. bitmap edges
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1023, 1024, 1025, 131071, 131072])
def test_bitmap_edges_lds(n):
    """Level 0 in LDS: n at word and level-1-word edges; see ring_driver.lds_shapes for the rows (the full row among them)."""
    for at_end in (False, True):
        for case in rd.lds_cases(n, at_end=at_end):
            rd.run(case)


@pytest.mark.parametrize("n", [rd.WIDE_N, 140_000])
def test_bitmap_edges_full_rows_global_slabs(n):
    """The full row and the full row minus every second column beyond the LDS bitmap: the bitmap kernel on global slabs, three
    level-1 words per thread.  n = 131073: the last word of both levels holds one valid bit, 129 level-1 words = 43 full threads;
    n = 140000: 137 level-1 words, the last thread's range is cut short."""
    shapes = [s for s in rd.lds_shapes(n) if s[0].startswith("full") or s[0].startswith("SUB of")]
    assert len(shapes) == 4
    for at_end in (False, True):
        (case,) = rd.lds_cases(n, shapes, at_end=at_end)
        assert min(rd.candidates(case)) > rd.SORT_CAP
        rd.run(case)


# ------------------------------------------------------------------------------------------------ d. the mode switch
def _caterpillar(n):
    """40 spine nodes in a path, 65 .. 200 leaves each, up to two leaf-leaf edges per leaf (leaf degree <= 5), two hubs of degree
    1500 whose neighbours are otherwise isolated; node ids scattered over 0 .. n - 1 with n - 1 in use; everything else isolated."""
    rng = np.random.default_rng(11)
    ids = rng.permutation(n - 1)[:12000].tolist()
    spine = [n - 1] + ids[:39]
    nxt = 39
    edges = list(zip(spine, spine[1:]))
    for s in spine:
        k = int(rng.integers(65, 201))
        leaves = ids[nxt:nxt + k]
        nxt += k
        edges += [(s, v) for v in leaves]
        half = len(leaves) // 2
        edges += [(leaves[t], leaves[half + t]) for t in range(0, half, 2)]
        edges += [(leaves[t], leaves[(t + 7) % half]) for t in range(0, half, 5) if t != (t + 7) % half]
    for _ in range(2):
        hub = ids[nxt]
        edges += [(hub, v) for v in ids[nxt + 1:nxt + 1501]]
        nxt += 1501
    assert nxt <= len(ids)
    r, c = np.array(edges, dtype=np.int64).T
    a = sp.csr_matrix((np.ones(2 * len(r), dtype=np.float32), (np.r_[r, c], np.r_[c, r])), shape=(n, n))
    a.sum_duplicates()
    a.data[:] = 1
    a.sort_indices()
    return a, spine


def _sorted_csr(m):
    m = sp.csr_matrix(m)
    m.eliminate_zeros()
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


def test_mode_switch_131072_131073():
    """One graph through exact_hop_rings_device for 3 hops at n = 131072 (bitmap in LDS) and at n = 131073 with one isolated node
    added (sorted-candidate kernel + global slabs): rings 1 .. 3 equal between the two and equal to oracle.nhood_split."""
    n = rd.LDS_BITMAP_COLS
    a, spine = _caterpillar(n)
    deg = np.diff(a.indptr)
    leaf = np.ones(n, dtype=bool)
    leaf[spine] = False
    assert deg[leaf & (deg < 1000)].max() <= 5 and (deg == 1500).sum() == 2
    c2 = a @ deg                                 # candidates of the ring-2 call: degrees summed over the frontier ring 1 = A
    assert ((deg > 64) & (c2 <= rd.SORT_CAP)).sum() >= 10 and (c2 > rd.SORT_CAP).sum() >= 2
    want = [_sorted_csr(h) for h in oo.nhood_split(a, 3)]
    assert len(want) == 4
    got = {}
    for m in (n, n + 1):
        rp = np.r_[a.indptr, [a.indptr[-1]] * (m - n)].astype(np.int64)
        pat = (torch.from_numpy(rp).to(DEV), torch.from_numpy(a.indices.astype(np.int32)).to(DEV))
        rings = po.exact_hop_rings_device(pat[0], pat[1], m, 3)
        assert len(rings) == 4
        got[m] = [(r[0].cpu().numpy(), r[1].cpu().numpy()) for r in rings]
        # ring 1 the header's other way: F = I with A as the expansion operand
        other = po.ring_set_device(m, torch.device(DEV), a=pat, frontier=po.identity_pattern(m, DEV), sub_diag=True)
        assert np.array_equal(other[0].cpu().numpy(), got[m][1][0]) and np.array_equal(other[1].cpu().numpy(), got[m][1][1])
    for k in (1, 2, 3):
        assert np.array_equal(got[n][k][0], want[k][0]) and np.array_equal(got[n][k][1], want[k][1]), k
        assert np.array_equal(got[n + 1][k][0], np.r_[want[k][0], want[k][0][-1]]) and np.array_equal(got[n + 1][k][1], want[k][1]), k


# ------------------------------------------------------------------------------------------------ e. slab / LDS reuse
def _reuse(n, rows, with_sub):
    """`rows` rows whose frontier is one of 7 hubs (degree 1025 .. 1100, pairwise overlapping, unequal column sets) in turn.
    with_sub: SUB takes, per hub, its columns in every second level-0 word -- whole words go to zero under a set level-1 bit."""
    rng = np.random.default_rng(23)
    universe = np.unique(np.r_[rng.integers(0, n, 1500), n - 1])
    hubs = sorted(rng.choice(n, 7, replace=False).tolist())
    cols = [np.sort(np.r_[rng.choice(universe[:-1], 1025 + 12 * h + (h == 6) * 3 - 1, replace=False), n - 1]).astype(np.int32) for h in range(7)]
    assert [len(c) for c in cols] == [1025, 1037, 1049, 1061, 1073, 1085, 1100]
    for x in range(7):
        for y in range(x):
            assert len(np.intersect1d(cols[x], cols[y])) > 0 and not np.array_equal(cols[x], cols[y])
    a = {hubs[h]: cols[h].tolist() for h in range(7)}
    turn = np.arange(rows) % 7
    f = (np.arange(rows + 1, dtype=np.int64), np.asarray(hubs, dtype=np.int32)[turn])
    subs, want = [], cols
    if with_sub:
        sub_cols = [c[(c >> 5) % 2 == 0] for c in cols]
        want = [c[(c >> 5) % 2 == 1] for c in cols]
        lens = np.array([len(s) for s in sub_cols], dtype=np.int64)[turn]
        rp = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum(lens, out=rp[1:])
        block = np.concatenate(sub_cols)
        ci = np.concatenate([np.tile(block, rows // 7)] + [sub_cols[h] for h in range(rows % 7)])
        subs = [(rp, ci)]
    case = rd.Case(n, n - rows if rows < n else 0, rows, a=a, f=f, sub=subs)
    rowptr, colidx = rd.execute(case)
    lens = np.array([len(w) for w in want], dtype=np.int64)
    assert np.array_equal(np.diff(rowptr), lens[turn])
    block = np.concatenate(want)
    whole = rows // 7
    assert np.array_equal(colidx[:whole * len(block)].reshape(whole, len(block)), np.broadcast_to(block, (whole, len(block))))
    assert np.array_equal(colidx[whole * len(block):], np.concatenate([want[h] for h in range(rows % 7)] + [np.zeros(0, np.int32)]))
    print(f"n = {n}: {rows} rows, {len(colidx)} columns written")


def test_slab_reuse_global_mode():
    """More rows than level-0 bitmaps (CUs * 32 slabs at n = 131073, CUs * 8 workgroups with LDS bitmaps at n = 4096), every one
    for the bitmap kernel: at least 2048 rows are served by a workgroup that has served another hub's row before, so a bit -- or,
    with the SUB, a level-1 bit over a zeroed word -- left behind shows in the next row."""
    _reuse(rd.WIDE_N, _cus() * 32 + 2048, with_sub=False)
    _reuse(4096, _cus() * 8 + 2048, with_sub=True)


# ------------------------------------------------------------------------------------------------ f. pattern table, window edges
def _small_rows_case(n, rows, row_begin, n_add, n_sub, seed, **flags):
    """ADD rows of 1 .. 4 drawn columns (any order, repeats); a SUB_q row holds two drawn columns and the first column of the same
    row of ADD_q, ascending."""
    rng = np.random.default_rng(seed)
    add = [[rng.integers(0, n, size=int(rng.integers(1, 5))).tolist() for _ in range(rows)] for _ in range(n_add)]
    sub = []
    for q in range(n_sub):
        hit = add[q % n_add] if n_add else None
        sub.append([sorted(set(rng.integers(0, n, size=2).tolist() + ([hit[i][0]] if hit else []))) for i in range(rows)])
    return rd.Case(n, row_begin, rows, add=add, sub=sub, **flags)


@pytest.mark.parametrize("n", [1025, rd.WIDE_N])
def test_pattern_table_limits(n):
    """8 ADD and 8 SUB patterns at once (kMaxPatterns), all non-empty; 9 of either is H2GCN_ERR_INVALID_ARGUMENT with nothing
    written; windows of 0, 1, 2 and 3 rows, one row at n - 1 with add_diag, and a window past the sorted kernel's grid cap."""
    most = rd.MAX_PATTERNS
    case = _small_rows_case(n, 37, n - 37, most, most, seed=1, add_diag=True, sub_diag=True)
    rd.run(case)
    for n_add, n_sub in ((most + 1, 0), (0, most + 1), (most + 1, most + 1)):
        call = rd.Call(_small_rows_case(n, 5, 0, n_add, n_sub, seed=2))
        st, rp_h, rp_dev, nnz = call.count()
        assert st == _capi.ERR_INVALID_ARGUMENT and f"at most {most}" in call.error()
        assert (rp_h == rd.SENT64).all() and nnz == rd.SENT64
        st, ci_h = call.fill(rp_dev, 16)
        assert st == _capi.ERR_INVALID_ARGUMENT and (ci_h == rd.SENT32).all()
        assert (rp_dev.cpu().numpy() == rd.SENT64).all()
    for row_begin, rows in ((n - 4, 5), (n, 1), (-1, 2)):          # a window that leaves 0 .. n: an error, nothing written
        call = rd.Call(_small_rows_case(n, rows, row_begin, 1, 1, seed=3))
        st, rp_h, rp_dev, nnz = call.count()
        assert st == _capi.ERR_INVALID_ARGUMENT and "row window" in call.error() and (rp_h == rd.SENT64).all() and nnz == rd.SENT64
        st, ci_h = call.fill(rp_dev, 16)
        assert st == _capi.ERR_INVALID_ARGUMENT and (ci_h == rd.SENT32).all()
    rowptr, colidx = rd.run(rd.Case(n, n // 2, 0, add=[[]], add_diag=True))
    assert rowptr.tolist() == [0] and colidx.size == 0
    rowptr, colidx = rd.run(rd.Case(n, n - 1, 1, add_diag=True))
    assert colidx.tolist() == [n - 1]
    for rows in (1, 2, 3):
        rd.run(_small_rows_case(n, rows, n - rows, 2, 1, seed=3 + rows, sub_diag=True))
    rows = 4 * _cus() * 8 + 3          # the sorted kernel's grid is capped at CUs * 8 workgroups of 4 waves: its row loop strides
    assert rows <= n or n <= rd.LDS_BITMAP_COLS
    rows = min(rows, n)
    rd.run(_small_rows_case(n, rows, n - rows, 2, 1, seed=9, add_diag=True))


# ------------------------------------------------------------------------------------------------ g. drawn cases
_STREAM = []


def _side_stream():
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


@settings(max_examples=int(os.environ.get("H2GCN_FUZZ_EXAMPLES", "100")), deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow])
@given(seed=st.integers(0, 2 ** 31 - 1), n=st.sampled_from([33, 1024, 4097, 131072, 131073, 140000]), n_rows=st.integers(1, 300),
       pos=st.floats(0.0, 1.0), has_f=st.booleans(), n_add=st.integers(0, 8), n_sub=st.integers(0, 8), add_diag=st.booleans(),
       sub_diag=st.booleans(), dense=st.booleans(), side_stream=st.booleans())
def test_random_set_algebra(seed, n, n_rows, pos, has_f, n_add, n_sub, add_diag, sub_diag, dense, side_stream):
    """Property-based sweep over n (both modes and their edge), window position and length, frontier or none, 0 .. 8 ADD and SUB
    patterns, both diagonal flags, row densities (a few rows beyond 1024 candidates) and the stream (the default one or another);
    the checks of ring_driver.run.  100 examples by default (H2GCN_FUZZ_EXAMPLES sets another count), the same ones on every run."""
    case = rd.random_case(seed, n, n_rows, pos, has_f, n_add, n_sub, add_diag, sub_diag, dense)
    if side_stream:
        with torch.cuda.stream(_side_stream()):
            rd.run(case)
    else:
        rd.run(case)


# ------------------------------------------------------------------------------------------------ h. normalisation
def _normalize(rowptr, colidx, mode, table, table_len, col_len=None):
    """h2gcn_hop_normalize_rows on NaN-filled values with a NaN guard behind; -> (status, values)."""
    nnz = int(rowptr[-1])
    vals = torch.full((nnz + 8,), float("nan"), dtype=torch.float32, device=DEV)
    rp, ci = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(colidx).to(DEV)
    cl = torch.from_numpy(col_len).to(DEV) if col_len is not None else None
    st = _capi.lib().h2gcn_hop_normalize_rows(len(rowptr) - 1, C.c_void_p(rp.data_ptr()), C.c_void_p(ci.data_ptr()), mode,
                                              C.c_void_p(table.data_ptr()) if table is not None else None, table_len,
                                              C.c_void_p(cl.data_ptr()) if cl is not None else None, C.c_void_p(vals.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = vals.cpu().numpy()
    assert np.isnan(out[nnz:]).all()
    return st, out[:nnz]


def _table(norm, length):
    """k^-1/2 / k^-1 for k = 0 .. length - 1, inf -> 0: the reference's numpy expression; a slice of a longer device array."""
    with np.errstate(divide="ignore"):
        s = np.power(np.arange(length + 8, dtype=np.float64), -0.5 if norm == oo.SYM else -1.0)
    s[np.isinf(s)] = 0.0
    return torch.from_numpy(s).to(DEV)


def test_normalize_table_and_windows():
    """Row lengths 0, 1, 63, 64, 65 (the lane loop strides by 64) and 40 000 rows of length 1 in one call (more rows than the
    32 768 waves of the capped grid: the wave loop strides); SYM and RW bit-equal to oracle.normalize cast to fp32, ORDINARY all
    ones; a row window with col_len equals the rows of the whole call; a table one entry short is an error."""
    n = 40_005
    rng = np.random.default_rng(2)
    lens = np.r_[[0, 1, 63, 64, 65], np.ones(40_000, dtype=np.int64)]
    rows = [np.sort(rng.choice(np.arange(1, n), size=k, replace=False)) for k in lens[:5]]      # no column 0: row 0 is empty and
    cols = np.r_[np.concatenate(rows), rng.integers(1, n, size=40_000)].astype(np.int32)          # scipy drops a product that is 0
    rowptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    m = sp.csr_matrix((np.ones(len(cols)), cols, rowptr), shape=(n, n))
    longest = int(lens.max())
    whole = {}
    for norm, mode in ((oo.SYM, 1), (oo.RW, 2), (oo.ORDINARY, 0)):
        ref = sp.csr_matrix(oo.normalize(m, norm))
        ref.sort_indices()
        assert np.array_equal(ref.indptr, rowptr) and np.array_equal(ref.indices, cols)
        tab = _table(norm, longest + 1) if mode else None
        st, vals = _normalize(rowptr, cols, mode, tab, longest + 1 if mode else 0)          # s_table_len = max row length + 1
        assert st == 0, _capi.lib().h2gcn_last_error()
        assert np.array_equal(vals, ref.data.astype(np.float32)), norm
        assert mode != 0 or (vals == 1).all()
        whole[norm] = vals
        if mode:
            st, _ = _normalize(rowptr, cols, mode, tab, longest)                           # the longest row is past the table
            assert st == _capi.ERR_INVALID_ARGUMENT and b"scaling table" in _capi.lib().h2gcn_last_error(), norm
            # row windows, the whole matrix's row lengths in col_len
            for r0, r1 in ((0, 5), (2, 4), (3, 20_000), (39_990, n)):
                lo, hi = rowptr[r0], rowptr[r1]
                st, part = _normalize(rowptr[r0:r1 + 1] - lo, cols[lo:hi], mode, tab, longest + 1, col_len=lens.astype(np.int64))
                assert st == 0 and np.array_equal(part, whole[norm][lo:hi]), (norm, r0, r1)
    # a COLUMN's length decides under SYM with col_len: rows of length 1, column 7 has 500 entries in the whole matrix
    col_len = np.ones(64, dtype=np.int64)
    col_len[7] = 500
    rp, ci = np.arange(4, dtype=np.int64), np.array([3, 7, 9], dtype=np.int32)
    tab = _table(oo.SYM, 501)
    st, vals = _normalize(rp, ci, 1, tab, 501, col_len=col_len)
    assert st == 0 and np.array_equal(vals, np.array([1.0, np.power(np.float64(500), -0.5), 1.0]).astype(np.float32))
    st, _ = _normalize(rp, ci, 1, tab, 500, col_len=col_len)
    assert st == _capi.ERR_INVALID_ARGUMENT and b"scaling table" in _capi.lib().h2gcn_last_error()
    st, vals = _normalize(rp, ci, 2, _table(oo.RW, 2), 2, col_len=col_len)                 # RW never looks at the column
    assert st == 0 and (vals == 1).all()
