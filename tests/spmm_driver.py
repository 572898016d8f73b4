"""Test driver for the CSR-adaptive walks of the fused hop SpMM (h2gcn_amd/csrc/spmm_kernels.hip.h: short_list_blocks,
medium_list_blocks, their interleave in groups of kNumXcd workgroups, in_tile_short_rows; host side: launch() in h2gcn_capi.hip).

A `Case` is ONE plan plus the launches made on it: hop matrices built from PRESCRIBED per-row segment lengths (`hop_from_lengths`,
`hop_with_transposed_lengths` for the adjoint, whose classes are those of the transposed operand), the schedule tunables, the hop
selections, and the claims its name makes.  `reach` restates on the CPU what such a launch does -- the class counts, the walk the
schedule picks, and `work_split`, a plain-Python copy of launch()'s split into entries per wave, workgroups per hop, chunk-major
padding and groups of 8 -- so that `check_claims` can assert that a case reaches what it says BEFORE any GPU is involved
(tests/test_spmm_driver.py asserts the coverage of every family's case list with it).  `run_case` then makes the launches:

  outputs      views with 4 guard columns on either side into buffers filled with a NaN sentinel, passed through out=: a row no
               walk served keeps the sentinel, a store outside the row hits a guard
  forward      all hops, the hop subsets, twice each (second call bit for bit the first)
  adjoint      the same through spmm_t
  compared     BIT FOR BIT with oracle.gcn_layer.gcn_layer_tree / gcn_layer_grad_tree at the case's long threshold, and within
               1e-5 * max(1, sum |a||x|) of the fp64-accumulated product
  path         plan.schedule(d)["segment_walk"] and plan.segment_classes(d)["listed"] equal the restatement's

The last column of a forward-built hop is never referenced and X's last row is NaN: POISON for the `views` cases, whose colidx /
vals are views at element offsets into buffers of that column id and of Inf (the technique of tests/test_index_window_gpu.py).

`python -m tests.spmm_driver --family NAME` runs one family in this process and exits 0 or 1, one line per case; the `knobs` family
is run that way in child processes, because H2GCN_SHORT_HOP_MAJOR / H2GCN_SHORT_PER_WAVE / H2GCN_MED_PER_WAVE are read once per
process.  Importing this module needs no GPU.  (The tests import it as `spmm_driver`, like the sibling drivers; `-m tests.spmm_driver`
from the repository root resolves `tests` as a namespace package -- there is no tests/__init__.py -- and is the same module.)"""
import argparse
import os
import re
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
_CSRC = ROOT / "h2gcn_amd" / "csrc"


def _constant(file_name, name):
    m = re.search(rf"constexpr (?:int|int64_t) {name} = (\d+);", (_CSRC / file_name).read_text())
    if not m:
        raise RuntimeError(f"{file_name}: no `constexpr int {name} = <n>;` -- the driver's restatement is built around it")
    return int(m.group(1))


SHORT_MAX = _constant("spmm_kernels.hip.h", "kShortMax")
SHORT_SUM_HOPS = _constant("spmm_kernels.hip.h", "kShortSumHops")
WAVES_PER_BLOCK = _constant("spmm_kernels.hip.h", "kWavesPerBlock")
NUM_XCD = _constant("spmm_kernels.hip.h", "kNumXcd")
WF = _constant("h2gcn_capi.hip", "kWavesToFill")
WAVE = 64
DEFAULT_THR = 256
KNOBS = ("H2GCN_SHORT_HOP_MAJOR", "H2GCN_SHORT_PER_WAVE", "H2GCN_MED_PER_WAVE")
WALKS = {"tile": "wave per segment", "pipe": "wave per segment + index prefetch", "in_tile": "lane group per segment (short rows)",
         "lists": "lane group per segment (binned short segments) + wave per segment"}
GUARD = 4     # sentinel columns on either side of every output row
ATOL = 1e-5

# the lengths family A cycles through (plus thr - 2 .. thr + 1 of the case's threshold)
LEN_SHORT = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16)
LEN_MEDIUM = (17, 18, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255)
LEN_LONG = (256, 257, 319, 320, 321, 511, 512, 513)
THRESHOLDS = (0, 17, 16, 9, 2, 1, 512)          # 0 = the default, 256
WIDTHS = ((64, 0), (128, 0), (128, 64), (100, 0), (20, 0))     # (d, slice_cols): 100 / 20 run on a masked 128 / 64-column slice
COUNTS_SHORT = (0, 1, 3, 4, 5, 15, 16, 17, 127, 128, 129, 255, 257)
COUNTS_MEDIUM = (0, 1, 3, 4, 5, 31, 32, 33)
RATIOS = {"n:0": (257, 0, 0), "1:n": (1, 100, 1), "1:1": (100, 20, 0), "1:5": (128, 133, 3), "5:1": (520, 32, 0), "3:2": (257, 33, 1)}


# ---------------------------------------------------------------------------------------------------------- graph builders
def hop_from_lengths(lengths, n_cols, seed, cover_residues=None):
    """CSR [len(lengths), n_cols] whose row r has exactly lengths[r] entries: distinct ascending columns (an arithmetic run of
    random start and stride inside [0, n_cols - 1): the LAST column is never referenced), values uniform in (-1, 1).
    cover_residues=(lo, hi): the segments of lo..hi entries must start on every residue of the element index mod 32."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n, usable = len(lengths), int(n_cols) - 1
    assert lengths.min(initial=0) >= 0 and lengths.max(initial=0) <= usable, "a row cannot hold more distinct columns than there are"
    rng = np.random.default_rng(seed)
    steps = np.maximum(lengths - 1, 1)
    stride = 1 + rng.integers(0, 1 << 30, n) % np.minimum(np.maximum((usable - 1) // steps, 1), 7)
    stride[lengths <= 1] = 1
    span = np.maximum(lengths - 1, 0) * stride
    start = rng.integers(0, 1 << 62, n) % (usable - span)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    nnz = int(indptr[-1])
    j = np.arange(nnz, dtype=np.int64) - np.repeat(indptr[:-1], lengths)
    cols = np.repeat(start, lengths) + np.repeat(stride, lengths) * j
    assert nnz == 0 or (0 <= cols.min() and cols.max() < usable)
    vals = rng.uniform(-1, 1, nnz).astype(np.float32)
    vals[np.abs(vals) >= 1] = 0.5
    m = sp.csr_matrix((vals, cols.astype(np.int32), indptr), shape=(n, int(n_cols)))
    m.has_sorted_indices = True
    assert np.array_equal(np.diff(m.indptr), lengths)
    inner = np.ones(nnz, dtype=bool)
    inner[indptr[:-1][lengths > 0]] = False          # first entry of each row
    assert (np.diff(cols, prepend=-1)[inner] > 0).all(), "columns ascend inside every row"
    if cover_residues is not None:
        lo, hi = cover_residues
        sel = (lengths >= lo) & (lengths <= hi)
        got = set((indptr[:-1][sel] % 32).tolist())
        assert len(got) == 32, f"segment starts of the {lo}..{hi}-entry rows miss residues {sorted(set(range(32)) - got)} mod 32"
    return m


def hop_with_transposed_lengths(lengths, n_rows, seed, cover_residues=None):
    """A [n_rows, len(lengths)] such that row j of A^T -- output row j of the adjoint -- has exactly lengths[j] entries, in the
    order the plan's stable transposition gives them."""
    a = hop_from_lengths(lengths, n_rows, seed, cover_residues).T.tocsr()
    a.sort_indices()
    assert np.array_equal(transposed_lengths(a), np.asarray(lengths))
    return a


def row_lengths(m):
    return np.diff(m.indptr).astype(np.int64)


def transposed_lengths(m):
    return np.bincount(m.indices, minlength=m.shape[1]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- restatement
def short_max_of(thr):
    return min(SHORT_MAX, thr - 1)


def classes(lengths, thr):
    """0 short / 1 medium / 2 long per segment (h2gcn_capi.hip: short <= short_max < medium < long_threshold <= long)"""
    lengths = np.asarray(lengths)
    return np.where(lengths <= short_max_of(thr), 0, np.where(lengths >= thr, 2, 1))


def class_counts(sel_lengths, thr, adjoint):
    """Forward: (short, medium, long) per selected hop.  Adjoint: ONE (short, medium, long) -- the rows short in every selected
    hop, the rows owned by the long path (any long segment), the rest."""
    cls = [classes(l, thr) for l in sel_lengths]
    if not adjoint:
        return [tuple(int((c == k).sum()) for k in range(3)) for c in cls]
    c = np.stack(cls)
    all_short, any_long = (c == 0).all(0), (c == 2).any(0)
    return [(int(all_short.sum()), int((~all_short & ~any_long).sum()), int(any_long.sum()))]


def work_split(short_counts, med_counts, n_sel, adjoint, env=None):
    """launch()'s split of a list-driven launch, restated: entries per wave (spw, mpw), list workgroups per hop, chunk-major
    padding, groups of kNumXcd workgroups.  `env`: the three knobs (strings, as in os.environ)."""
    env = env or {}
    knob = lambda k, dflt: int(env[k]) if env.get(k) not in (None, "") else dflt  # noqa: E731
    n_listed, n_med, longest = sum(short_counts), sum(med_counts), max(short_counts)
    mpw_max = max(1, min(4, WAVE // n_sel)) if adjoint else 8
    mpw = max(1, min(n_med // WF, mpw_max))
    e = knob("H2GCN_MED_PER_WAVE", 0)
    if e >= 1 and e * n_sel <= WAVE:
        mpw = e
    spw = 4
    while spw < 64 and n_listed // (2 * spw) >= WF:
        spw *= 2
    e = knob("H2GCN_SHORT_PER_WAVE", 0)
    if 4 <= e <= 64 and e % 4 == 0:
        spw = e
    major = knob("H2GCN_SHORT_HOP_MAJOR", -1)
    hop_major = major if major >= 0 else 0
    s_per_block, m_per_block = WAVES_PER_BLOCK * spw, WAVES_PER_BLOCK * mpw
    short_blocks = [-(-c // s_per_block) for c in short_counts]
    med_blocks = [-(-c // m_per_block) for c in med_counts]
    sblocks, mblocks = sum(short_blocks), sum(med_blocks)
    padded = not adjoint and not hop_major
    if padded:
        sblocks = -(-longest // s_per_block) * len(short_counts)
    return dict(spw=spw, mpw=mpw, hop_major=bool(hop_major), padded=padded, short_blocks=short_blocks, med_blocks=med_blocks,
                short_end=list(np.cumsum(short_blocks)), med_end=list(np.cumsum(med_blocks)), sblocks=sblocks, mblocks=mblocks,
                short_groups=-(-sblocks // NUM_XCD), med_groups=-(-mblocks // NUM_XCD))


def slice_of(d, slice_cols):
    """pick_slice_cols for the small operands of this sweep (nothing here is cache-sized)"""
    if slice_cols:
        return slice_cols
    if d < 64:
        return 64
    for w in (256, 128, 64):
        if d % w == 0:
            return w
    w = 64
    while w < d:
        w *= 2
    return w


def reach(case, hops, sel, adjoint, env=None):
    """What the launch of `case` on the hop selection `sel` (None = all) does, from the lengths alone."""
    H = len(hops)
    sel = list(range(H)) if sel is None else sorted(sel)
    thr = case.thr or DEFAULT_THR
    lens = [(transposed_lengths if adjoint else row_lengths)(hops[k]) for k in sel]
    n_sel, n_out = len(sel), len(lens[0])
    nnz_sel = int(sum(l.sum() for l in lens))
    counts = class_counts(lens, thr, adjoint)
    n_short = sum(c[0] for c in counts) if (not adjoint or n_sel <= SHORT_SUM_HOPS) else 0
    frac = n_short / (float(n_out) * (1 if adjoint else n_sel))
    avg = nnz_sel / (float(n_out) * n_sel)
    sl = slice_of(case.d, case.slice_cols)
    assert case.d % 4 == 0 and case.d >= 4, "the sweep stays on the plain-store kernels"
    grouped_ok = sl in (64, 128)
    v = case.variant
    in_tile = grouped_ok and (v == 5 or (v == 0 and avg < 16.0 and n_out >= 4 * WF))
    lists = grouped_ok and not in_tile and n_short > 0 and (v == 6 or (v == 0 and frac >= 0.05))
    pipe = (v == 2 or (v == 0 and avg < 16.0)) and not in_tile and not lists
    out = dict(walk="in_tile" if in_tile else "lists" if lists else "pipe" if pipe else "tile", listed=-1 if in_tile else n_short if lists else 0,
               counts=counts, n_sel=n_sel, n_out=n_out, slice=sl, G=WAVE // (sl // 4), n_long=sum(c[2] for c in counts))
    if lists:
        out.update(work_split([c[0] for c in counts], [c[1] for c in counts], n_sel, adjoint, env))
    return out


# ---------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    make: object                  # () -> list of scipy CSR hop matrices [n_rows, n_cols]
    d: int
    variant: int = 6
    thr: int = 0                  # long_row_threshold (0 = default)
    rpw: int = 0
    slice_cols: int = 0
    fwd: tuple = (None,)          # forward hop selections (None = all hops)
    adj: tuple = ()               # adjoint hop selections; () = the plan is built without the transpose
    bf16: bool = False            # bf16 source, fp32 and bf16 outputs
    views: object = None          # (per-hop (colidx offset, vals offset), tail): poisoned buffers around the hop arrays
    claims: tuple = ()            # ("fwd" | "adj", selection, key, value or predicate): what the case's name says it reaches
    tags: dict = field(default_factory=dict)


def check_claims(case, hops, env=None):
    """Assert every claim of the case against the restatement; returns {(direction, selection): reach}."""
    seen = {}
    for direction, sel, key, want in case.claims:
        k = (direction, None if sel is None else tuple(sel))
        if k not in seen:
            seen[k] = reach(case, hops, sel, direction == "adj", env)
        got = seen[k].get(key)
        ok = want(got) if callable(want) else got == want
        assert ok, f"{case.name}: {direction} {sel}: {key} = {got}, the case claims {want if not callable(want) else 'otherwise'}"
    return seen


def _pad4(values):
    values = list(dict.fromkeys(values))
    extra = iter((1, 17, 0, 16))
    while len(values) % 4:
        values.append(next(extra))         # a repeat: the cycle length must be a multiple of 4 (see edges_graph)
    return values


def edge_lengths(thr):
    t = thr or DEFAULT_THR
    return _pad4(list(LEN_SHORT) + list(LEN_MEDIUM) + list(LEN_LONG) + [x for x in (t - 2, t - 1, t, t + 1) if x >= 0])


N_COLS_A = 1200
ROUND_EDGES = (15, 16, 17, 31, 32, 33)     # LPR - 1 / LPR / LPR + 1 of the 64- and 128-column geometries


def edges_lengths_2hops(thr, rpw, rot):
    """Per-row lengths of the two hops of family A.  With Ls the edge lengths (m of them, m % 4 == 0):
    hop 0  row q*m + i holds Ls[(i + q) % m]: every length at every row position mod 4;
    hop 1  another rotation, then every length LAST in a tile of 4*rpw rows (row k*T - 1) and FIRST in one (row k*T);
    both   a region of rows of 3 entries in which each of ROUND_EDGES and one long row sit at every position of a wave's
           rpw rows (hence of a round of G rows), alone among short rows; row n - 1 holds Ls[rot], Ls[rot + m/2];
    n is no multiple of rpw, so the last wave has rows_here < rpw."""
    Ls = edge_lengths(thr)
    m, T, w = len(Ls), 4 * max(rpw, 1), max(rpw, 1)
    n_main = max(700, T * (m + 1))
    r = np.arange(n_main)
    q, i = r // m, r % m
    h0 = np.array(Ls)[(i + q) % m]
    h1 = np.array(Ls)[(i + 3 * q + m // 2) % m]
    for k in range(1, m + 1):
        h1[k * T - 1] = Ls[k - 1]
        h1[k * T] = Ls[(k - 1 + m // 2) % m]
    region = []
    for x in ROUND_EDGES + ((thr or DEFAULT_THR),):
        blk = np.full(w * (w + 1) + 1, 3)
        blk[1 + np.arange(w) * (w + 1)] = x      # every position mod w, rows of 3 entries on either side
        region.append(blk)
    # 32 consecutive LISTED (short) segments of an odd length start on every residue mod 32, whatever precedes them
    region.append(np.full(34, 3 if short_max_of(thr or DEFAULT_THR) >= 3 else 1))
    region = np.concatenate(region)
    tail = np.full(1 + int(w > 1 and (n_main + len(region) + 1) % w == 0), 2)
    h0 = np.concatenate([h0, region, tail])
    h1 = np.concatenate([h1, np.roll(region, 1), tail])
    h0[-1], h1[-1] = Ls[rot % m], Ls[(rot + m // 2) % m]
    assert w == 1 or len(h0) % w != 0
    return h0, h1


def edges_graph(thr, rpw, rot):
    h0, h1 = edges_lengths_2hops(thr, rpw, rot)
    sm = short_max_of(thr or DEFAULT_THR)
    cover = (1, sm) if sm >= 1 else None       # the listed lengths; thr = 1 lists empty rows only
    return [hop_from_lengths(h0, N_COLS_A, 1000 + rot, cover_residues=cover), hop_from_lengths(h1, N_COLS_A, 2000 + rot, cover_residues=cover)]


def family_edges(thr):
    """A, forward-built: every class edge x 7 thresholds x variants 6 / 5 / 0 x 5 widths; the in-tile mode with rows_per_wave
    0 / 1 / 3 / 7 at EVERY width (a round holds more than one row only for rows_per_wave > 1); bf16 at every width (thr 256)."""
    cases, rot = [], 0
    combos = [(v, 0, d, sc) for v in (6, 5, 0) for d, sc in WIDTHS] + [(5, rpw, d, sc) for rpw in (1, 3, 7) for d, sc in WIDTHS]
    for v, rpw, d, sc in combos:
        walk = {6: "lists", 5: "in_tile"}.get(v)
        claims = [("fwd", None, "walk", walk), ("adj", None, "walk", walk)] if walk else []
        if v == 6:
            claims += [("fwd", None, "spw", 4), ("fwd", None, "mpw", 1)]
        cases.append(Case(f"edges thr={thr} v={v} rpw={rpw} d={d}/{sc}", (lambda t=thr, w=rpw, r=rot: edges_graph(t, w, r)), d, variant=v, thr=thr,
                          rpw=rpw, slice_cols=sc, fwd=(None, [0], [1]), adj=(None, [1]), claims=tuple(claims),
                          tags=dict(thr=thr, rpw=rpw, rot=rot)))
        rot += 1
    if thr == 0:
        for v in (6, 5, 0):
            for d, sc in WIDTHS:
                rpw = 3 if v == 5 else 0
                cases.append(Case(f"edges bf16 v={v} rpw={rpw} d={d}/{sc}", (lambda w=rpw, r=rot: edges_graph(0, w, r)), d, variant=v, rpw=rpw, slice_cols=sc,
                                  fwd=(None, [1]), adj=(None,), bf16=True, tags=dict(thr=0, rpw=rpw, rot=rot)))
                rot += 1
    return cases


ADJ_SELECTIONS = ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3], None)
N_SRC_ADJ = 1100


def adjoint_base_lengths(thr, n_out=704):
    """Base sequence b of the adjoint graph; hop k holds b shifted by 3k rows, so every hop has the SAME nonzero count and an
    output row is medium in at most one hop: rows short in every hop, rows short in all but one, and -- around the long
    entries -- rows with one long segment.  The same ROUND_EDGES / long placements as family A sit in the sequence."""
    t = thr or DEFAULT_THR
    shorts = [x for x in LEN_SHORT + (t - 2, t - 1) if 0 <= x <= short_max_of(t)]
    mediums = [x for x in LEN_MEDIUM + (t - 2, t - 1, 33) if short_max_of(t) < x < t] or [short_max_of(t)]
    longs = [x for x in LEN_LONG + (t, t + 1) if x >= t]
    r = np.arange(n_out)
    b = np.array(shorts)[(r - r // len(shorts)) % len(shorts)]
    med_rows = r[r % 16 == 0]
    b[med_rows] = np.array(mediums)[np.arange(len(med_rows)) % len(mediums)]
    long_rows = r[r % 113 == 56]       # 113 is prime: the long-owned rows take every position of a wave's rows and rounds
    b[long_rows] = np.array(longs)[np.arange(len(long_rows)) % len(longs)]
    return b


def adjoint_graph(thr, seed=0):
    b = adjoint_base_lengths(thr)
    return [hop_with_transposed_lengths(np.roll(b, 3 * k), N_SRC_ADJ, 3000 + 10 * seed + k) for k in range(5)]


def family_edges_adjoint(thr):
    """A, transposed-built, per threshold: the adjoint's classes prescribed, selections of 1..5 hops (5: no lists, tile walk), at
    every width; variants 6 and 0 and the in-tile mode with rows_per_wave 3 and 7, so that SUM rounds hold G = 2 / 4 rows --
    all short, one row too wide, one long-owned row at every position; bf16 at every width (thr 256)."""
    cases = []
    for v, rpw in ((6, 0), (0, 0), (5, 3), (5, 7)):
        for d, sc in WIDTHS:
            claims = []
            if v == 6:
                claims = [("adj", s, "walk", "lists") for s in ADJ_SELECTIONS[:4]] + [("adj", None, "walk", "tile"), ("adj", None, "listed", 0)]
                has_medium = (thr or DEFAULT_THR) > SHORT_MAX + 1
                claims += [("adj", s, "counts", lambda c, hm=has_medium: c[0][0] > 0 and (c[0][1] > 0) == hm and c[0][2] > 0) for s in ADJ_SELECTIONS[1:4]]
            if v == 5:
                claims = [("adj", s, "walk", "in_tile") for s in ADJ_SELECTIONS]
            cases.append(Case(f"edges adjoint thr={thr} v={v} rpw={rpw} d={d}/{sc}", (lambda t=thr: adjoint_graph(t)), d, variant=v, thr=thr, slice_cols=sc,
                              rpw=rpw, fwd=(None,), adj=ADJ_SELECTIONS, claims=tuple(claims), tags=dict(thr=thr)))
    if thr == 0:
        for i, (d, sc) in enumerate(WIDTHS):
            v, rpw = ((6, 0), (5, 3), (5, 7))[i % 3]
            cases.append(Case(f"edges adjoint bf16 v={v} rpw={rpw} d={d}/{sc}", (lambda: adjoint_graph(0)), d, variant=v, rpw=rpw, slice_cols=sc,
                              adj=([0, 1, 2], None), fwd=(), bf16=True, tags=dict(thr=0)))
    return cases


def lengths_for_counts(n_short, n_med, n_long, seed):
    """A shuffled sequence with exactly these class counts at the default threshold: short 0..16, medium 17..80, long 256..300."""
    rng = np.random.default_rng(seed)
    l = np.concatenate([np.arange(n_short) % (SHORT_MAX + 1), 17 + np.arange(n_med) % 64, 256 + np.arange(n_long) % 45]).astype(np.int64)
    rng.shuffle(l)
    return l


N_COLS_B = 600


def family_counts():
    """B: prescribed list counts at spw = 4 (16 entries per workgroup, 128 per group of 8) and mpw = 1."""
    cases = []
    singles = [(s, COUNTS_MEDIUM[i % len(COUNTS_MEDIUM)], (0, 1, 3)[i % 3]) for i, s in enumerate(COUNTS_SHORT)]
    singles += [(5, 0, 0), (17, 1, 0), (16, 32, 0), (1, 5, 1)]      # the medium counts the pairing above leaves out ...
    singles += list(RATIOS.values())
    for j, (s, m, l) in enumerate(singles):
        if s + m + l == 0:
            m = 1
        for d in (64, 128):
            lists = s > 0
            claims = [("fwd", None, "walk", "lists" if lists else "tile"), ("fwd", None, "counts", [(s, m, l)]), ("fwd", None, "listed", s)]
            if lists:
                claims += [("fwd", None, "spw", 4), ("fwd", None, "mpw", 1)]
            cases.append(Case(f"counts fwd s={s} m={m} l={l} d={d}", (lambda a=(s, m, l), k=j: [hop_from_lengths(lengths_for_counts(*a, k), N_COLS_B, 4000 + k)]),
                              d, claims=tuple(claims), tags=dict(counts=(s, m, l))))
            aclaims = [("adj", None, k_, v_) for _, _, k_, v_ in claims]
            cases.append(Case(f"counts adj s={s} m={m} l={l} d={d}",
                              (lambda a=(s, m, l), k=j: [hop_with_transposed_lengths(lengths_for_counts(*a, k), N_COLS_B, 5000 + k)]),
                              d, fwd=(), adj=(None,), claims=tuple(aclaims), tags=dict(counts=(s, m, l))))
    # the adjoint's single list with two hops: both hops hold the same length sequence, so a row has one class
    for j, (s, m, l) in enumerate([(257, 33, 1), (17, 5, 0), (129, 0, 3), (1, 100, 1)]):
        claims = (("adj", None, "walk", "lists"), ("adj", None, "counts", [(s, m, l)]), ("adj", None, "spw", 4), ("adj", None, "mpw", 1))
        cases.append(Case(f"counts adj 2 hops s={s} m={m} l={l}",
                          (lambda a=(s, m, l), k=j: [hop_with_transposed_lengths(lengths_for_counts(*a, 77 + k), N_COLS_B, 6000 + 2 * k + h) for h in range(2)]),
                          64 if j % 2 else 128, fwd=(), adj=(None,), claims=claims, tags=dict(counts=(s, m, l))))
    # unequal lists across 2 and 3 hops; an empty short list beside one of 257 (the chunk-major padding)
    for j, per_hop in enumerate([((257, 43, 0), (0, 297, 3)), ((129, 170, 1), (17, 283, 0), (5, 292, 3)), ((257, 43, 0), (0, 300, 0), (17, 280, 3))]):
        H = len(per_hop)
        sels = (None,) + tuple([a, b] for a in range(H) for b in range(a + 1, H) if H > 2)
        claims = [("fwd", None, "walk", "lists"), ("fwd", None, "counts", list(per_hop)), ("fwd", None, "padded", True),
                  ("fwd", None, "short_blocks", lambda sb: len(set(sb)) == len(sb))]
        for d in (64, 128):
            cases.append(Case(f"counts fwd {H} hops {[c[0] for c in per_hop]} d={d}",
                              (lambda p=per_hop, k=j: [hop_from_lengths(lengths_for_counts(*c, 90 + 10 * k + h), N_COLS_B, 7000 + 10 * k + h) for h, c in enumerate(p)]),
                              d, fwd=sels, claims=tuple(claims), tags=dict(per_hop=per_hop)))
    return cases


def _cycle(n, lo, hi, shift=0):
    return lo + (np.arange(n, dtype=np.int64) + shift) % (hi - lo + 1)


def steps_adjoint_lengths():
    """4 hops of equal nonzero count (hop k = the base sequence shifted by k rows): 8*WF + 9 rows short in every hop, then rows
    whose hop r % 4 holds 17..40 entries -- medium for every selection that contains that hop."""
    n_s, n_m = 8 * WF + 9, 8 * WF + 41     # 2*WF + 11 medium rows per hop: no multiple of a wave's or a workgroup's entries
    b = np.concatenate([_cycle(n_s, 0, SHORT_MAX), _cycle(n_m, 0, SHORT_MAX, 5)])
    med = n_s + np.arange(0, n_m, 4)
    b[med] = _cycle(len(med), 17, 40)
    return [np.roll(b, k) for k in range(4)]


def family_steps():
    """C: the per-wave steps.  d = 8: one masked 64-column slice, G = 4."""
    cases = []
    for mult, plus, spw in ((8, -1, 4), (8, 1, 8), (16, 3, 16), (32, 5, 32), (64, 7, 64)):
        n = mult * WF + plus
        cases.append(Case(f"steps fwd short n={mult}*WF{plus:+d} spw={spw}", (lambda n=n: [hop_from_lengths(_cycle(n, 0, SHORT_MAX), 4096, n)]), 8,
                          claims=(("fwd", None, "walk", "lists"), ("fwd", None, "spw", spw), ("fwd", None, "listed", n), ("fwd", None, "G", 4),
                                  ("fwd", None, "short_blocks", lambda sb, n=n, spw=spw: n % (4 * spw) != 0 and n % 4 != 0)),
                          tags=dict(spw=spw)))
    n = 8 * WF + 1
    cases.append(Case("steps fwd short spw=8 d=128", (lambda n=n: [hop_from_lengths(_cycle(n, 0, SHORT_MAX), 2048, n + 1)]), 128,
                      claims=(("fwd", None, "spw", 8), ("fwd", None, "G", 2)), tags=dict(spw=8)))
    for mult, plus, mpw in ((2, 1, 2), (5, 3, 5), (8, 1, 8)):
        n = mult * WF + plus
        cases.append(Case(f"steps fwd medium n={mult}*WF+{plus} mpw={mpw}",
                          (lambda n=n: [hop_from_lengths(np.concatenate([_cycle(n, 17, 40), [0, 3, 16, 1, 9]]), 4096, n)]), 8,
                          claims=(("fwd", None, "walk", "lists"), ("fwd", None, "mpw", mpw), ("fwd", None, "counts", [(5, n, 0)])), tags=dict(mpw=mpw)))
    sels = ([0, 1], [0, 1, 2], None)
    claims = []
    for s in sels:
        claims += [("adj", s, "walk", "lists"), ("adj", s, "mpw", 4), ("adj", s, "spw", lambda v: v >= 8),
                   ("adj", s, "counts", lambda c: c[0][1] >= 4 * WF + 1)]
    cases.append(Case("steps adj NS=2,3,4 mpw=4 spw>=8", (lambda: [hop_with_transposed_lengths(l, 4096, 8000 + k) for k, l in enumerate(steps_adjoint_lengths())]),
                      8, fwd=(), adj=sels, claims=tuple(claims), tags=dict(mpw=4, ns=(2, 3, 4))))
    return cases


def family_views():
    """E: colidx / vals as views at element offsets into poisoned buffers; tail 0 = the views end where the buffers end."""
    cases = []
    k = 0
    for off in (0, 1, 15, 31):
        other = {0: 31, 1: 0, 15: 1, 31: 15}[off]
        for tail in (64, 0):
            for v in (6, 5):
                d, sc = WIDTHS[(k // 2 + k) % 2]
                k += 1
                cases.append(Case(f"views off={off}/{other} tail={tail} v={v} d={d}", (lambda: edges_graph(0, 0, 5)), d, variant=v, slice_cols=sc,
                                  fwd=(None, [1]), views=(((off, other), (other, off)), tail),
                                  claims=(("fwd", None, "walk", "lists" if v == 6 else "in_tile"),), tags=dict(off=off, tail=tail)))
    return cases


def family_knobs():
    """D: the small graphs of A and B under the three once-per-process knobs (run in child processes): forward selections of 3
    hops with unequal short lists (short_end[] matters in the hop-major order), adjoint selections of 1..4 hops on hops of equal
    nonzero count."""
    cases = [c for c in family_edges(0) if c.variant == 6 and not c.bf16]
    for c in cases:
        c.adj, c.claims = (), ()
    for c in family_counts():
        multi = "per_hop" in c.tags
        if multi or c.tags.get("counts") in RATIOS.values() or "2 hops" in c.name:
            c.claims = ()
            cases.append(c)
    for d, sc in WIDTHS[:2]:
        cases.append(Case(f"knobs adjoint d={d}", (lambda: adjoint_graph(0)), d, slice_cols=sc, fwd=(None, [0, 2, 4]), adj=ADJ_SELECTIONS[:4]))
    return cases


def knob_claims(cases_with_hops, env):
    """What a knob setting must reach on the knobs family (asserted by the child before it touches the GPU)."""
    reached = []
    for case, hops in cases_with_hops:
        for direction, sels in (("fwd", case.fwd), ("adj", case.adj)):
            for sel in sels:
                r = reach(case, hops, sel, direction == "adj", env)
                if r["walk"] == "lists":
                    reached.append((direction, r))
    if env.get("H2GCN_SHORT_HOP_MAJOR"):
        # (a later hop's workgroups find their list only through short_end[hop - 1] > 0)
        assert any(d == "fwd" and r["hop_major"] and r["n_sel"] >= 3 and len({c[0] for c in r["counts"]}) == r["n_sel"] and r["short_end"][0] > 0
                   and r["counts"][-1][0] > 0 for d, r in reached), "no 3-hop forward launch with unequal short lists"
    if env.get("H2GCN_SHORT_PER_WAVE"):
        assert all(r["spw"] == int(env["H2GCN_SHORT_PER_WAVE"]) for _, r in reached)
    if env.get("H2GCN_MED_PER_WAVE"):
        assert all(r["mpw"] == int(env["H2GCN_MED_PER_WAVE"]) for _, r in reached)
        assert all(any(d == "adj" and r["n_sel"] == ns and r["counts"][0][1] > r["mpw"] for d, r in reached) for ns in (2, 3, 4))
    return reached


FAMILIES = {"edges": lambda: [c for t in THRESHOLDS for c in family_edges(t)], "edges_adjoint": lambda: [c for t in THRESHOLDS for c in family_edges_adjoint(t)], "counts": family_counts,
            "steps": family_steps, "views": family_views, "knobs": family_knobs}


# ---------------------------------------------------------------------------------------------------------- runner
def _bits_equal(t, want):
    import torch

    want = torch.from_numpy(np.ascontiguousarray(want))
    if t.dtype == torch.bfloat16:
        return torch.equal(t.cpu().contiguous().view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    return torch.equal(t.cpu().contiguous().view(torch.int32), want.view(torch.int32))


def _bf16_round(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def _make_plan(case, hops, dev):
    import torch

    from h2gcn_amd import HopPlan

    n_cols = hops[0].shape[1]
    offsets, tail = case.views if case.views else (((0, 0),) * len(hops), 0)
    rp, ci, va = [], [], []
    for m, (oc, ov) in zip(hops, offsets):
        nnz = m.nnz
        cbuf = torch.full((oc + nnz + tail,), n_cols - 1, dtype=torch.int32, device=dev)
        vbuf = torch.full((ov + nnz + tail,), float("inf"), dtype=torch.float32, device=dev)
        cbuf[oc:oc + nnz] = torch.from_numpy(m.indices.astype(np.int32)).to(dev)
        vbuf[ov:ov + nnz] = torch.from_numpy(m.data.astype(np.float32)).to(dev)
        rp.append(torch.from_numpy(m.indptr.astype(np.int64)).to(dev))
        ci.append(cbuf[oc:oc + nnz])
        va.append(vbuf[ov:ov + nnz])
    return HopPlan(rp, ci, va, n_cols, build_transpose=bool(case.adj), long_row_threshold=case.thr, rows_per_wave=case.rpw, variant=case.variant,
                   slice_cols=case.slice_cols)


def _guarded(shape, dtype, dev):
    """(buffer, view): the view is `shape` with GUARD sentinel columns on either side of every row; all NaN"""
    import torch

    buf = torch.full(tuple(shape[:-1]) + (shape[-1] + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[..., GUARD:GUARD + shape[-1]]


def _launch_twice(fn, shape, dtype, dev, where):
    import torch

    outs = []
    for _ in range(2):
        buf, view = _guarded(shape, dtype, dev)
        fn(view)
        assert bool(torch.isnan(buf[..., :GUARD]).all()) and bool(torch.isnan(buf[..., GUARD + shape[-1]:]).all()), f"{where}: a guard column was written"
        outs.append(view)
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(outs[0].contiguous().view(it), outs[1].contiguous().view(it)), f"{where}: the second call differs from the first"
    return outs[0]


def _assert_bound(y, want64, mag, where):
    bad = ~(np.abs(y.astype(np.float64) - want64) <= ATOL * np.maximum(1.0, mag))
    assert not bad.any(), f"{where}: {int(bad.sum())} elements beyond {ATOL} * max(1, magnitude) of the fp64 product"


def run_case(case, dev, env=None, hops=None):
    """Build the plan, make every launch of the case, assert bits, bound and path.  `env`: the knob settings of THIS process
    (default: none, and then the case's claims are asserted too)."""
    import torch

    from oracle import gcn_layer as og

    env = {k: v for k, v in (os.environ if env is None else env).items() if k in KNOBS}
    hops = case.make() if hops is None else hops
    if not env:
        check_claims(case, hops)
    H, (n_rows, n_cols), d, thr = len(hops), hops[0].shape, case.d, case.thr or DEFAULT_THR
    plan = _make_plan(case, hops, dev)
    rng = np.random.default_rng(len(case.name) + d)
    BF = torch.bfloat16

    def check_path(sel, adjoint, where):
        want = reach(case, hops, sel, adjoint, env)
        got = plan.schedule(d, hops=sel, adjoint=adjoint)["segment_walk"], plan.segment_classes(d, hops=sel, adjoint=adjoint)["listed"]
        assert got == (WALKS[want["walk"]], want["listed"]), f"{where}: the plan reports {got}, the restatement {WALKS[want['walk']], want['listed']}"

    if case.fwd:
        x = rng.uniform(-1, 1, (n_cols, d)).astype(np.float32)
        if case.bf16:
            x = _bf16_round(x)
        poisoned = all(m.nnz == 0 or m.indices.max() < n_cols - 1 for m in hops)
        assert poisoned or not case.views
        xt = torch.from_numpy(x).to(dev)
        if poisoned:
            xt[n_cols - 1] = float("nan")
        tree = og.gcn_layer_tree(hops, x, long_threshold=thr)
        want64 = og.gcn_layer_f64acc(hops, x)
        mag = og.gcn_layer_f64acc([abs(m) for m in hops], np.abs(x))
        for sel in case.fwd:
            idx = list(range(H)) if sel is None else sorted(sel)
            where = f"{case.name}: forward hops={sel}"
            check_path(sel, False, where)
            src = xt.to(BF) if case.bf16 else xt
            y = _launch_twice(lambda out: plan.spmm(src, hops=sel, out=out), (n_rows, len(idx), d), torch.float32, dev, where)
            assert _bits_equal(y, tree[:, idx]), f"{where}: bits differ from the canonical tree"
            _assert_bound(y.cpu().numpy(), want64[:, idx], mag[:, idx], where)
            if case.bf16:
                yb = _launch_twice(lambda out: plan.spmm(src, hops=sel, out=out), (n_rows, len(idx), d), BF, dev, where + " bf16 out")
                assert _bits_equal(yb, tree[:, idx]), f"{where}: bf16 output is not the rounded tree"
    if case.adj:
        w = rng.uniform(-1, 1, (n_rows, H, d)).astype(np.float32)
        if case.bf16:
            w = _bf16_round(w)
        wt = torch.from_numpy(w).to(dev)
        for sel in case.adj:
            idx = list(range(H)) if sel is None else sorted(sel)
            where = f"{case.name}: adjoint hops={sel}"
            check_path(sel, True, where)
            hs, ws = [hops[k] for k in idx], np.ascontiguousarray(w[:, idx])
            tree_t = og.gcn_layer_grad_tree(hs, ws, n_cols, long_threshold=thr)
            want64 = sum(h.T.astype(np.float64) @ ws[:, k].astype(np.float64) for k, h in enumerate(hs))
            mag = sum(abs(h).T.astype(np.float64) @ np.abs(ws[:, k]).astype(np.float64) for k, h in enumerate(hs))
            g = wt[:, idx].contiguous()
            g = g.to(BF) if case.bf16 else g
            dx = _launch_twice(lambda out: plan.spmm_t(g, hops=sel, out=out), (n_cols, d), torch.float32, dev, where)
            assert _bits_equal(dx, tree_t), f"{where}: bits differ from the canonical tree"
            _assert_bound(dx.cpu().numpy(), np.asarray(want64), np.asarray(mag), where)
            if case.bf16:
                db = _launch_twice(lambda out: plan.spmm_t(g, hops=sel, out=out), (n_cols, d), BF, dev, where + " bf16 out")
                assert _bits_equal(db, tree_t), f"{where}: bf16 output is not the rounded tree"
    torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    args = ap.parse_args(argv)
    import torch

    env = {k: os.environ[k] for k in KNOBS if os.environ.get(k)}
    built = [(c, c.make()) for c in FAMILIES[args.family]()]
    if args.family == "knobs":
        knob_claims(built, env)
    if not torch.cuda.is_available():
        print("no GPU")
        return 1
    dev = torch.device("cuda:0")
    failed = 0
    for case, hops in built:
        try:
            run_case(case, dev, env, hops)
            print(f"ok   {case.name}")
        except AssertionError as e:
            failed += 1
            print(f"FAIL {case.name}: {e}")
    print(f"{len(built) - failed} of {len(built)} cases passed ({' '.join(f'{k}={v}' for k, v in env.items()) or 'no knobs'})")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
