"""Test driver for the ring set kernels (h2gcn_ring_count_rows / h2gcn_ring_fill_rows; csrc/rings.hip, include/h2gcn_hip.h).

A `Case` is a plain description of ONE call: n, the row window, the window's rows of F / ADD_p / SUB_q as Python lists, A as a
dict of rows, the two diagonal flags.  `expected` evaluates the header's set expression with Python sets (no SpGEMM anywhere),
`candidates` restates the kernel's candidate count, and `run` makes the call pair through ctypes on buffers the test owns:

  scratch      h2gcn_ring_scratch_bytes(n) bytes, EVERY byte 0xFF before each of the two calls (one tensor per n, reused)
  out_rowptr   sentinel-filled, guard entries before and after
  out_colidx   nnz entries between two sentinel-filled guard bands
  inputs       every array is followed by out-of-range entries (row pointers -1, columns n): a kernel that reads one entry too
               far produces a wrong row instead of leaving the allocation

and checks: both statuses 0, rowptr[0] == 0, rowptr[-1] == nnz_out, every row == sorted(expected), guards intact, the same
arrays when the pair is repeated on the same buffers, and the row pointers of ring_set_device(count_only=True).

The builders below compose a row with a PRESCRIBED candidate count c (the quantity the dispatch and the sort size depend on) from
one ADD row, from a frontier of a given length (zero-degree nodes, an all-zero 64-node chunk between two non-empty ones) or from
frontier + two ADD rows, with a duplicate structure chosen separately; `wide_cases` / `WIDE_SHAPES` is the list the wide-mode
sweep runs and tests/test_ring_driver.py asserts the coverage of.

Operand contract the inputs respect (include/h2gcn_hip.h): F and SUB rows strictly ascending; ADD and A rows in any order, with
duplicates; every column in [0, n)."""
import ctypes as C
from dataclasses import dataclass, field
from itertools import chain

import numpy as np

DEV = "cuda:0"
SENT64 = -0x0123_4567_89AB_CDEF
SENT32 = -0x0246_8ACE
RP_GUARD = 8          # sentinel row pointers on either side of out_rowptr
CI_GUARD = 2048       # sentinel columns on either side of out_colidx: twice kSortCap, so even a row that emitted every
                      # candidate of a sorted-kernel row on top of its own would stay inside the band
PAD = 32              # out-of-range entries behind every input array

# constants of csrc/rings.hip the case lists are built around
LDS_BITMAP_COLS = 1 << 17     # kLdsBitmapCols: level 0 in LDS up to this n
SORT_CAP = 1024               # kSortCap: candidates the sorted-candidate kernel takes
MAX_PATTERNS = 8              # kMaxPatterns
WIDE_N = LDS_BITMAP_COLS + 1  # the first n with level 0 in global slabs: l0_words = 4097, l1_words = 129, one valid bit in the last


@dataclass
class Case:
    n: int
    row_begin: int
    n_rows: int
    a: object = None          # dict node -> list of columns (absent = empty row), or a CSR pair (rowptr, colidx) of n rows
    f: object = None          # None = no expansion; else n_rows rows (lists) or a CSR pair
    add: list = field(default_factory=list)     # patterns: n_rows rows each, or CSR pairs
    sub: list = field(default_factory=list)
    add_diag: bool = False
    sub_diag: bool = False
    tags: list = None         # per row: the builder that made it (coverage assertion)


# ------------------------------------------------------------------------------------------------ reference (Python sets)
def _rows(pat, n_rows):
    if isinstance(pat, tuple):
        rp, ci = pat
        return [ci[rp[i]:rp[i + 1]].tolist() for i in range(n_rows)]
    assert len(pat) == n_rows
    return pat


def _a_row(a, j):
    if isinstance(a, tuple):
        return a[1][a[0][j]:a[0][j + 1]].tolist()
    return a.get(j, ())


def expected(case):
    """out[i] = (U_{j in F[i]} A[j]  U  U_p ADD_p[i]  U  {g}?)  \\  (U_q SUB_q[i]  U  {g}?),  g = row_begin + i; sorted lists."""
    f = _rows(case.f, case.n_rows) if case.f is not None else None
    add = [_rows(p, case.n_rows) for p in case.add]
    sub = [_rows(p, case.n_rows) for p in case.sub]
    out = []
    for i in range(case.n_rows):
        g = case.row_begin + i
        s = set()
        if f is not None:
            for j in f[i]:
                s.update(_a_row(case.a, j))
        for p in add:
            s.update(p[i])
        if case.add_diag:
            s.add(g)
        for q in sub:
            s.difference_update(q[i])
        if case.sub_diag:
            s.discard(g)
        out.append(sorted(s))
    return out


def candidates(case):
    """c per row as `candidate_count` of rings.hip defines it: A-row lengths summed over the frontier + ADD row lengths + 1 for
    add_diag (duplicates count)."""
    f = _rows(case.f, case.n_rows) if case.f is not None else None
    add = [_rows(p, case.n_rows) for p in case.add]
    out = []
    for i in range(case.n_rows):
        c = sum(len(_a_row(case.a, j)) for j in f[i]) if f is not None else 0
        out.append(c + sum(len(p[i]) for p in add) + (1 if case.add_diag else 0))
    return out


def sort_size(c):
    """P of the bitonic sort: the next power of two >= max(64, c)."""
    p = 64
    while p < c:
        p <<= 1
    return p


def hop_rings_by_sets(a, n, hops, rows=None):
    """Exact-k-hop rings 1 .. hops as the header spells them (ring_1: ADD = {A}, sub_diag; ring_k: F = ring_{k-1}, SUB = ring_1 ..
    ring_{k-1}, sub_diag), each evaluated by `expected`; lists of rows of the window `rows` (default: all)."""
    r0, r1 = rows if rows is not None else (0, n)
    rings = [expected(Case(n, r0, r1 - r0, add=[[list(a.get(i, ())) for i in range(r0, r1)]], sub_diag=True))]
    for _ in range(2, hops + 1):
        rings.append(expected(Case(n, r0, r1 - r0, a=a, f=rings[-1], sub=list(rings), sub_diag=True)))
    return rings


# ------------------------------------------------------------------------------------------------ arrays
def _csr(pat, n_rows):
    if isinstance(pat, tuple):
        return np.asarray(pat[0], dtype=np.int64), np.asarray(pat[1], dtype=np.int32)
    assert len(pat) == n_rows
    rp = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(r) for r in pat), dtype=np.int64, count=n_rows), out=rp[1:])
    return rp, np.fromiter(chain.from_iterable(pat), dtype=np.int32, count=int(rp[-1]))


def _a_csr(a, n):
    if isinstance(a, tuple):
        return _csr(a, n)
    rp = np.zeros(n + 1, dtype=np.int64)
    keys = sorted(a)
    if keys:
        rp[np.asarray(keys, dtype=np.int64) + 1] = [len(a[j]) for j in keys]
    np.cumsum(rp, out=rp)
    return rp, np.fromiter(chain.from_iterable(a[j] for j in keys), dtype=np.int32, count=int(rp[-1]))


def flatten(rows):
    """(rowptr, colidx) numpy arrays of a list of rows."""
    return _csr(rows, len(rows))


_SCRATCH = {}
STATS = {"calls": 0, "rows": 0}       # call pairs made and rows compared since the import (a figure for reports)


def _scratch(n):
    import torch

    from h2gcn_amd import _capi
    if n not in _SCRATCH:
        if len(_SCRATCH) >= 3:       # the wide ones are ~130 MB each
            _SCRATCH.clear()
        _SCRATCH[n] = torch.empty(int(_capi.lib().h2gcn_ring_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    return _SCRATCH[n]


def _upload(pair, n):
    """(rowptr, colidx) device tensors, each followed by PAD out-of-range entries."""
    import torch
    rp, ci = pair
    rp = np.concatenate([rp, np.full(PAD, -1, dtype=np.int64)])
    ci = np.concatenate([ci, np.full(PAD, n, dtype=np.int32)])
    return torch.from_numpy(rp).to(DEV), torch.from_numpy(ci).to(DEV)


def _ptr_array(tensors):
    arr_t = C.c_void_p * max(len(tensors), 1)
    return arr_t(*[t.data_ptr() for t in tensors])


class Call:
    """The device-side arguments of one case; `count` / `fill` make ONE API call each on sentinel-prepared outputs."""

    def __init__(self, case):
        import torch

        from h2gcn_amd import _capi
        self.case, self.L = case, _capi.lib()
        n, rows = case.n, case.n_rows
        self.a = _upload(_a_csr(case.a, n), n) if case.a is not None else None
        self.f = _upload(_csr(case.f, rows), n) if case.f is not None else None
        self.add = [_upload(_csr(p, rows), n) for p in case.add]
        self.sub = [_upload(_csr(p, rows), n) for p in case.sub]
        self.scratch = _scratch(n)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        a_rp, a_ci = self.a if self.a is not None else (None, None)
        f_rp, f_ci = self.f if self.f is not None else (None, None)
        self._keep = (_ptr_array([p[0] for p in self.add]), _ptr_array([p[1] for p in self.add]),
                      _ptr_array([p[0] for p in self.sub]), _ptr_array([p[1] for p in self.sub]))
        self.common = (n, case.row_begin, rows, ptr(a_rp), ptr(a_ci), ptr(f_rp), ptr(f_ci),
                       len(self.add), self._keep[0], self._keep[1], int(case.add_diag),
                       len(self.sub), self._keep[2], self._keep[3], int(case.sub_diag))

    def count(self):
        """-> (status, out_rowptr buffer with its guards as numpy, device buffer, nnz_out)."""
        import torch
        rows = self.case.n_rows
        buf = torch.full((rows + 1 + 2 * RP_GUARD,), SENT64, dtype=torch.int64, device=DEV)
        nnz = C.c_int64(SENT64)
        self.scratch.fill_(0xFF)
        st = self.L.h2gcn_ring_count_rows(*self.common, C.c_void_p(buf.data_ptr() + 8 * RP_GUARD), C.byref(nnz),
                                          C.c_void_p(self.scratch.data_ptr()), self.scratch.numel(), self.stream)
        torch.cuda.synchronize()
        return st, buf.cpu().numpy(), buf, nnz.value

    def fill(self, rp_buf, nnz):
        """-> (status, out_colidx buffer with its guard bands as numpy)."""
        import torch
        buf = torch.full((nnz + 2 * CI_GUARD,), SENT32, dtype=torch.int32, device=DEV)
        self.scratch.fill_(0xFF)
        st = self.L.h2gcn_ring_fill_rows(*self.common, C.c_void_p(rp_buf.data_ptr() + 8 * RP_GUARD), C.c_void_p(buf.data_ptr() + 4 * CI_GUARD),
                                         C.c_void_p(self.scratch.data_ptr()), self.scratch.numel(), self.stream)
        torch.cuda.synchronize()
        return st, buf.cpu().numpy()

    def error(self):
        return self.L.h2gcn_last_error().decode()


def execute(case, check=None):
    """The call pair, twice, on owned buffers, with every check that needs no reference (`check(result)`, if given, judges the
    first round before the two are compared); -> (rowptr, colidx) numpy."""
    import torch

    from h2gcn_amd import operands as po
    call = Call(case)
    rows = case.n_rows
    STATS["calls"] += 1
    STATS["rows"] += rows
    outs = []
    for rnd in range(2):
        st, rp_h, rp_dev, nnz = call.count()
        assert st == 0, (rnd, call.error())
        assert (rp_h[:RP_GUARD] == SENT64).all() and (rp_h[RP_GUARD + rows + 1:] == SENT64).all(), "out_rowptr guard touched"
        rowptr = rp_h[RP_GUARD:RP_GUARD + rows + 1].copy()
        assert rowptr[0] == 0 and rowptr[-1] == nnz, (rnd, rowptr[0], rowptr[-1], nnz)
        assert (np.diff(rowptr) >= 0).all(), rnd
        st, ci_h = call.fill(rp_dev, nnz)
        assert st == 0, (rnd, call.error())
        assert (ci_h[:CI_GUARD] == SENT32).all(), "guard band before out_colidx touched"
        assert (ci_h[CI_GUARD + nnz:] == SENT32).all(), "guard band behind out_colidx touched"
        assert np.array_equal(rp_dev.cpu().numpy(), rp_h), "the fill pass changed out_rowptr"
        outs.append((rowptr, ci_h[CI_GUARD:CI_GUARD + nnz].copy()))
        if check is not None and rnd == 0:
            check(outs[0])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "second round differs"
    rp2, _ = po.ring_set_device(case.n, torch.device(DEV), a=call.a, frontier=call.f, add=call.add, add_diag=case.add_diag,
                                sub=call.sub, sub_diag=case.sub_diag, rows=(case.row_begin, case.row_begin + rows), count_only=True)
    assert np.array_equal(rp2.cpu().numpy(), outs[0][0]), "ring_set_device(count_only=True) counts differently"
    return outs[0]


def compare(case, got, want_rows):
    rowptr, colidx = got
    want_rp, want_ci = flatten(want_rows)
    if np.array_equal(rowptr, want_rp) and np.array_equal(colidx, want_ci):
        return
    cand = None
    for i, want in enumerate(want_rows):
        row = colidx[rowptr[i]:rowptr[i + 1]].tolist()
        if row != want:
            cand = cand or candidates(case)
            extra, missing = sorted(set(row) - set(want)), sorted(set(want) - set(row))
            raise AssertionError(f"row {i} (global {case.row_begin + i}, {case.tags[i] if case.tags else 'untagged'}, c = {cand[i]}, n = "
                                 f"{case.n}): {len(row)} columns, want {len(want)}; extra {extra[:8]}, missing {missing[:8]}, "
                                 f"ascending and distinct: {all(x < y for x, y in zip(row, row[1:]))}")
    raise AssertionError("row pointers differ although every row matches")


def run(case):
    """execute + every row against the Python-set reference; -> (rowptr, colidx) numpy."""
    want = expected(case)
    return execute(case, check=lambda got: compare(case, got, want))


# ------------------------------------------------------------------------------------------------ builders
DUPS = ("distinct", "same", "half", "seam")


def distinct_columns(n, d, rng, include=None, exclude=None):
    """d distinct columns of [0, n) in random order; `include` among them, `exclude` not; 0 and n - 1 from d = 3 on."""
    if d == 0:
        return []
    if n <= 4 * d + 64:
        pool = rng.permutation(n)
    else:
        pool = np.unique(rng.integers(0, n, size=2 * d + 16))
        rng.shuffle(pool)
    forced = ([include] if include is not None else []) + ([0, n - 1] if d >= 3 else [])
    forced = [v for v in dict.fromkeys(forced) if v != exclude]
    taken = set(forced)
    out = (forced + [v for v in pool.tolist() if v != exclude and v not in taken])[:d]
    assert len(out) == d and len(set(out)) == d
    return out


def make_candidates(n, k, dup, rng, include=None, exclude=None):
    """k candidate columns (a multiset, shuffled) with the duplicate structure `dup`:
    distinct / same (one column k times) / half (about half of them a second copy) / seam (two equal values on the SORTED
    positions 63 | 64 and 127 | 128 -- the seams of the sorted kernel's 64-lane emit chunks -- everything else distinct)."""
    if k == 0:
        return []
    if dup == "distinct":
        cand = distinct_columns(n, k, rng, include, exclude)
    elif dup == "same":
        cand = distinct_columns(n, 1, rng, include, exclude) * k
    elif dup == "half":
        vals = distinct_columns(n, (k + 1) // 2, rng, include, exclude)
        cand = vals + vals[:k - len(vals)]
    elif dup == "seam":
        vals = sorted(distinct_columns(n, k - (k > 64) - (k > 128), rng, include, exclude))
        cand = []
        for v in vals:
            cand.append(v)
            if len(cand) in (64, 128) and len(cand) < k:
                cand.append(v)
        s = sorted(cand)
        assert (k <= 64 or s[63] == s[64]) and (k <= 128 or s[127] == s[128])
    else:
        raise ValueError(dup)
    assert len(cand) == k
    return [cand[t] for t in rng.permutation(k)]


def split_degrees(k, f, zero_chunk=False):
    """Degrees of f frontier nodes summing to k.  From f = 3 on every third node has degree 0; `zero_chunk`: the nodes 64 .. 127
    (one whole 64-node gather step) all have degree 0, with non-empty steps before and after (f > 128)."""
    assert f >= 1 and not (zero_chunk and f <= 128)
    slots = [t for t in range(f) if not (zero_chunk and 64 <= t < 128) and not (f > 2 and t % 3 == 1)]
    degs = [0] * f
    q, r = divmod(k, len(slots))
    for idx, t in enumerate(slots):
        degs[t] = q + (1 if idx < r else 0)
    return degs


C_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026, 4096)
F_EDGES = (1, 63, 64, 65, 128, 129, 200)
# (builder, c, frontier length, all-zero middle chunk)
WIDE_SHAPES = (
    [("add", c, 0, False) for c in C_EDGES]
    + [("frontier", c, F_EDGES[t % len(F_EDGES)], False) for t, c in enumerate(C_EDGES)]
    + [("frontier", 1024, 200, True), ("frontier", 1024, 64, False), ("frontier", 1024, 129, False), ("frontier", 1023, 128, False),
       ("frontier", 700, 200, True), ("frontier", 1025, 200, True), ("frontier", 257, 1, False), ("frontier", 513, 65, False)]
    + [("mixed", c, f, z) for c, f, z in ((5, 1, False), (64, 63, False), (300, 65, False), (1024, 129, True), (1025, 64, False),
                                          (2000, 200, True))]
)
SUB_VARIANTS = ("none", "first-last-middle", "all")


def build_window(n, shapes, row_begin=None, add_diag=False, sub_variant="none", sub_diag=False, dups=DUPS, seed=0):
    """One window with a row per (shape, duplicate structure).  `row_begin` None: the window ends at row n - 1.  Rows with an even
    local index hold their own global id among the candidates, odd ones do not (sub_diag where the diagonal is a candidate and where
    it is not).  SUB: nothing / the first, last and middle survivor (two patterns, and a column that is no candidate) / everything."""
    specs = [(b, c, f, z, d) for (b, c, f, z) in shapes for d in dups if c - int(add_diag) >= 0]
    rows = len(specs)
    if row_begin is None:
        row_begin = n - rows
    rng = np.random.default_rng(seed)
    a, top = {}, n               # frontier nodes are handed out from n - 1 downwards, a fresh block per row
    f_rows, add0, add1, sub0, sub1, tags = [], [], [], [], [], []
    for i, (build, c, f, zero_chunk, dup) in enumerate(specs):
        g = row_begin + i
        k = c - int(add_diag)
        cand = make_candidates(n, k, dup, rng, include=g if i % 2 == 0 else None, exclude=None if i % 2 == 0 else g)
        k_f = {"add": 0, "frontier": k, "mixed": k // 2}[build]
        k_0 = {"add": k, "frontier": 0, "mixed": k // 4}[build]
        nodes = []
        if build != "add":
            nodes = list(range(top - f, top))
            top -= f
            pos = 0
            for j, deg in zip(nodes, split_degrees(k_f, f, zero_chunk)):
                a[j] = cand[pos:pos + deg]
                pos += deg
        f_rows.append(nodes)
        add0.append(cand[k_f:k_f + k_0])
        add1.append(cand[k_f + k_0:])
        surv = sorted(set(cand) | ({g} if add_diag else set()))
        if sub_variant == "first-last-middle" and surv:
            in_row = set(surv)
            other = next(v for v in range(n) if v not in in_row)
            sub0.append(sorted({surv[0], surv[-1], other}))
            sub1.append([surv[len(surv) // 2]])
        elif sub_variant == "all":
            sub0.append(surv[::2])
            sub1.append(surv[1::2])
        else:
            sub0.append([])
            sub1.append([])
        tags.append(f"{build} c={c} f={f}{' zero-chunk' if zero_chunk else ''} {dup}")
    assert top > 0
    return Case(n, row_begin, rows, a=a, f=f_rows, add=[add0, add1], sub=[] if sub_variant == "none" else [sub0, sub1],
                add_diag=add_diag, sub_diag=sub_diag, tags=tags)


def wide_cases(at_end, add_diag, n=WIDE_N, shapes=WIDE_SHAPES):
    """The windows of the wide-mode sweep at one window position and one add_diag: every SUB variant x sub_diag."""
    return [build_window(n, shapes, row_begin=None if at_end else 0, add_diag=add_diag, sub_variant=sv, sub_diag=sd,
                         seed=17 + 2 * t + int(sd))
            for t, sv in enumerate(SUB_VARIANTS) for sd in (False, True)]


def hand_over_case(n, lo, builder, seed=0):
    """Three rows with the SAME final set (700 distinct columns) built with c = lo, lo + 1 and lo + 2 candidates -- each one more
    copy of a column -- by `builder` ("add" or "frontier": 200 nodes, an all-zero middle chunk)."""
    rng = np.random.default_rng(seed)
    final = distinct_columns(n, 700, rng)
    a, top, f_rows, add0, tags = {}, n, [], [], []
    for c in (lo, lo + 1, lo + 2):
        cand = final + [final[t % 700] for t in range(c - 700)]
        cand = [cand[t] for t in rng.permutation(c)]
        if builder == "add":
            f_rows.append([])
            add0.append(cand)
        else:
            nodes = list(range(top - 200, top))
            top -= 200
            pos = 0
            for j, deg in zip(nodes, split_degrees(c, 200, True)):
                a[j] = cand[pos:pos + deg]
                pos += deg
            f_rows.append(nodes)
            add0.append([])
        tags.append(f"{builder} c={c}")
    return Case(n, 5, 3, a=a, f=f_rows, add=[add0], tags=tags)


def lds_shapes(n):
    """(name, ADD row, SUB row) of the bitmap edge sweep at n columns; SUB rows ascending."""
    edges = sorted({c for step in (32, 1024) for m in range(step, n, step) for c in (m - 1, m)})
    every32 = list(range(0, n, 32))
    full = list(range(n))
    # columns 32k (every level-0 word) and 32k + 5 (every third word); SUB takes every 32k -- two thirds of the marked words become
    # zero while their level-1 bit stays set -- and 32k + 7, which is never a candidate
    part = sorted(every32 + [c + 5 for c in every32[::3] if c + 5 < n])
    sub = sorted(every32 + [c + 7 for c in every32 if c + 7 < n])
    return [("empty", [], []), ("{0}", [0], []), ("{n-1}", [n - 1], []), ("32 / 1024 edges", edges, []),
            ("every 32nd", every32, []), ("full", full, []), ("full minus every second", full, full[::2]),
            ("full minus the odd columns", full, full[1::2]), ("SUB of non-candidates and whole words", part, sub),
            ("SUB only", [], every32)]


def lds_cases(n, shapes=None, at_end=False):
    """The shapes in windows of at most n rows (n = 1: one row per call)."""
    shapes = lds_shapes(n) if shapes is None else shapes
    out = []
    for s in range(0, len(shapes), n):
        chunk = shapes[s:s + n]
        out.append(Case(n, n - len(chunk) if at_end else 0, len(chunk), add=[[list(x[1]) for x in chunk]], sub=[[list(x[2]) for x in chunk]],
                        tags=[x[0] for x in chunk]))
    return out


def random_case(seed, n, n_rows, pos, has_f, n_add, n_sub, add_diag, sub_diag, dense):
    """A drawn case: A has up to 300 non-empty rows (degree up to 40, a few up to 700 when `dense`), F rows name them (up to 12
    nodes, a few up to 150), ADD rows have up to 30 entries (a few beyond 1024 when `dense`) in any order with duplicates, SUB
    rows are ascending samples of the candidates and of other columns."""
    rng = np.random.default_rng(seed)
    n_rows = min(n_rows, n)
    row_begin = int(round(pos * (n - n_rows)))
    active = np.unique(rng.integers(0, n, size=min(n, 300))).tolist()
    a = {}
    for j in active:
        deg = int(rng.integers(0, 41)) if not (dense and rng.random() < 0.03) else int(rng.integers(300, 701))
        a[j] = rng.integers(0, n, size=deg).tolist()
    f_rows = None
    if has_f:
        f_rows = []
        for _ in range(n_rows):
            ln = int(rng.integers(0, 13)) if rng.random() < 0.95 else int(rng.integers(60, 151))
            f_rows.append(sorted(set(rng.choice(active, size=min(ln, len(active)), replace=False).tolist())))
    add = []
    for _ in range(n_add):
        pat = []
        for _ in range(n_rows):
            ln = int(rng.integers(0, 31)) if not (dense and rng.random() < 0.02) else int(rng.integers(1000, 1300))
            pat.append(rng.integers(0, n, size=ln).tolist())
        add.append(pat)
    case = Case(n, row_begin, n_rows, a=a if has_f else None, f=f_rows, add=add, add_diag=add_diag, sub_diag=sub_diag)
    full = expected(case)
    for _ in range(n_sub):
        pat = []
        for i in range(n_rows):
            row = set(rng.integers(0, n, size=int(rng.integers(0, 6))).tolist())
            if full[i]:
                row.update(np.asarray(full[i])[rng.random(len(full[i])) < rng.choice([0.0, 0.2, 1.0])].tolist())
            pat.append(sorted(row))
        case.sub.append(pat)
    return case
