"""CPU suite: the Python-set reference of tests/ring_driver.py against the restatement of the reference's nhoodSplit
(oracle/operands.nhood_split) -- the reference is checked before it judges the kernels -- and the COVERAGE of the case lists the GPU
sweep (tests/test_rings_sweep_gpu.py) runs: a later edit of the lists that loses a boundary fails here, without a GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import ring_driver as rd
from oracle import operands as oo


def _graph(name):
    if name == "path":
        n, edges = 7, [(i, i + 1) for i in range(6)]
    elif name == "star":
        n, edges = 9, [(0, i) for i in range(1, 9)]
    elif name == "pendant triangle":
        n, edges = 6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 3)]
    else:
        n = 200
        rng = np.random.default_rng(5)
        edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 260), rng.integers(0, n, 260)) if u != v]
    a = {}
    for u, v in edges:
        a.setdefault(u, set()).add(v)
        a.setdefault(v, set()).add(u)
    return n, {j: sorted(s) for j, s in a.items()}


@pytest.mark.parametrize("name", ["path", "star", "pendant triangle", "random 200"])
def test_set_reference_equals_nhood_split(name):
    n, a = _graph(name)
    m = sp.lil_matrix((n, n), dtype=np.float64)
    for j, row in a.items():
        m[j, row] = 1
    want = oo.nhood_split(m.tocsr(), 3)
    assert len(want) == (3 if name == "star" else 4)        # like the reference, the list ends once reachability stops growing
    rings = rd.hop_rings_by_sets(a, n, 3)
    for k in (1, 2, 3):
        if k >= len(want):
            assert not any(rings[k - 1])
            continue
        h = sp.csr_matrix(want[k])
        h.eliminate_zeros()
        h.sort_indices()
        assert [h.indices[h.indptr[i]:h.indptr[i + 1]].tolist() for i in range(n)] == rings[k - 1], k
    # a row window of the expression is the rows of the whole
    r0, r1 = n // 3, n - 1
    win = rd.hop_rings_by_sets(a, n, 3, rows=(r0, r1))
    assert all(win[k] == rings[k][r0:r1] for k in range(3))


def test_candidates_and_expected_on_a_hand_case():
    a = {0: [5, 5, 2], 4: [], 6: [1]}
    case = rd.Case(8, 3, 2, a=a, f=[[0, 4], [6]], add=[[[7, 2], []], [[], [3, 3]]], sub=[[[2], [6]]], add_diag=True, sub_diag=False)
    assert rd.candidates(case) == [3 + 0 + 2 + 0 + 1, 1 + 0 + 2 + 1]
    assert rd.expected(case) == [[3, 5, 7], [1, 3, 4]]
    case.sub_diag = True
    assert rd.expected(case) == [[5, 7], [1, 3]]
    assert [rd.sort_size(c) for c in (0, 64, 65, 128, 129, 1024)] == [64, 64, 128, 128, 256, 1024]


def test_builders_make_what_they_claim():
    rng = np.random.default_rng(0)
    for k in (1, 2, 64, 65, 128, 129, 1025):
        for dup in rd.DUPS:
            cand = rd.make_candidates(rd.WIDE_N, k, dup, rng, include=77)
            assert len(cand) == k and 77 in cand and all(0 <= v < rd.WIDE_N for v in cand)
            s = sorted(cand)
            if dup == "distinct":
                assert len(set(cand)) == k
            if dup == "same":
                assert len(set(cand)) == 1
            if dup == "seam":
                assert (k <= 64 or s[63] == s[64]) and (k <= 128 or s[127] == s[128])
                assert len(set(cand)) == k - (k > 64) - (k > 128)
            assert 123 not in rd.make_candidates(rd.WIDE_N, k, dup, rng, exclude=123)
    degs = rd.split_degrees(1024, 200, zero_chunk=True)
    assert sum(degs) == 1024 and len(degs) == 200 and not any(degs[64:128]) and any(degs[:64]) and any(degs[128:]) and 0 in degs[:64]
    assert rd.split_degrees(0, 1) == [0] and rd.split_degrees(5, 1) == [5] and sum(rd.split_degrees(3, 129)) == 3


@pytest.mark.parametrize("at_end", [False, True])
def test_wide_case_list_covers_every_boundary(at_end):
    """A condition on the lists, not a measurement: with the single-ADD build and with the frontier build each, every candidate
    count on either side of every power of two up to the kernel hand-over, every frontier length around the 64-node gather step,
    every sort size -- and rows for the bitmap kernel in the same window."""
    assert rd.WIDE_N == rd.LDS_BITMAP_COLS + 1
    cases = rd.wide_cases(at_end, add_diag=False)
    assert len(cases) == 6 and {(bool(c.sub), c.sub_diag) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    for case in cases:
        assert case.n == rd.WIDE_N and case.row_begin == (case.n - case.n_rows if at_end else 0)
        cand = rd.candidates(case)
        f_len = [len(r) for r in case.f]
        for build in ("add", "frontier"):
            mine = [i for i, t in enumerate(case.tags) if t.startswith(build + " ")]
            assert {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026, 4096} <= {cand[i] for i in mine}
            assert {rd.sort_size(cand[i]) for i in mine if cand[i] <= rd.SORT_CAP} == {64, 128, 256, 512, 1024}
            for dup in rd.DUPS:     # both sides of the hand-over with every duplicate structure
                assert {1023, 1024, 1025} <= {cand[i] for i in mine if case.tags[i].endswith(dup)}
        front = [i for i, t in enumerate(case.tags) if t.startswith("frontier ")]
        assert {1, 63, 64, 65, 128, 129, 200} <= {f_len[i] for i in front if cand[i] <= rd.SORT_CAP}
        assert all(f_len[i] == 0 for i, t in enumerate(case.tags) if t.startswith("add "))
        # a multi-step gather with an all-zero middle step, at the cap
        assert any(cand[i] == 1024 and f_len[i] == 200 and not any(len(case.a.get(j, ())) for j in case.f[i][64:128]) for i in front)
        assert any(t.startswith("mixed ") for t in case.tags)
        # the contract: F and SUB strictly ascending, columns in range
        for pat in [case.f] + case.sub:
            assert all(x < y for row in pat for x, y in zip(row, row[1:]))
        assert all(0 <= v < case.n for pat in case.add + case.sub + [list(case.a.values())] for row in pat for v in row)
        g = [case.row_begin + i for i in range(case.n_rows)]
        unsubtracted = rd.expected(rd.Case(case.n, case.row_begin, case.n_rows, a=case.a, f=case.f, add=case.add))
        has_diag = [g[i] in set(unsubtracted[i]) for i in range(case.n_rows)]
        assert any(has_diag) and not all(has_diag)
    assert at_end is False or cases[0].row_begin + cases[0].n_rows == rd.WIDE_N
    everything = [c for c in cases if c.sub and not any(rd.expected(c))]
    assert len(everything) == 2                                            # the SUB-removes-everything windows
    with_diag = rd.wide_cases(at_end, add_diag=True)
    assert all(c.add_diag and min(rd.candidates(c)) == 1 and {1024, 1025} <= set(rd.candidates(c)) for c in with_diag)


def test_lds_shapes_and_hand_over_cases():
    for n in (1, 31, 32, 33, 1023, 1024, 1025, 131071, 131072):
        shapes = rd.lds_shapes(n)
        by_name = {s[0]: s for s in shapes}
        assert by_name["full"][1] == list(range(n)) and by_name["{n-1}"][1] == [n - 1]
        edges = set(by_name["32 / 1024 edges"][1])
        assert all(m - 1 in edges and m in edges for m in range(32, n, 32)) and (n <= 32) == (not edges)
        assert all(x < y for s in shapes for x, y in zip(s[2], s[2][1:]))
        assert all(c.n_rows <= n for c in rd.lds_cases(n)) and sum(c.n_rows for c in rd.lds_cases(n)) == len(shapes)
    for lo in (1023, 1024):
        for builder in ("add", "frontier"):
            case = rd.hand_over_case(rd.WIDE_N, lo, builder)
            assert rd.candidates(case) == [lo, lo + 1, lo + 2]
            want = rd.expected(case)
            assert want[0] == want[1] == want[2] and len(want[0]) == 700
