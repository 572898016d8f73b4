"""GPU suite: every kernel on the values the other files never feed it -- NaN, +-Inf, subnormals, -0.0, logits of large
magnitude, fp32 products that overflow -- in places the kernel actually READS, against the promises of include/h2gcn_hip.h:

  1. hop SpMM, forward and adjoint, fp32 and bf16: bit identity with the canonical summation tree (oracle.gcn_layer), stored
     zeros ("the pattern decides": 0 * Inf = NaN), the bf16 store's rounding of special values;
  2. the fused bias / ReLU epilogue: NaN propagates (np.maximum / torch.relu), -Inf -> 0, +Inf stays;
  3. masked metrics and the logit gradient: accurate at ANY offset of the logits (softmax cross-entropy is shift-invariant), and
     the documented contract for non-finite rows;
  4. dropout + Dense, both kernel families, f32 and bf16 X, full and row-selected: the dropout mask is a SELECT;
  5. the SDDMM's ONE documented order, restated on the CPU (oracle_sddmm_order_f32), bit for bit;
  6. Keras Adam on gradients whose squares underflow and overflow.

Shapes are the smallest that still reach every kernel path (row lengths 0 .. 130 around the short / medium / long classes, widths
around the 4-column vectors and the 64-column slices).  Bit comparisons go through assert_same_bits_nan_aware: identical NaN
positions, identical bits everywhere else (sign of zero, which infinity); NaN payload and sign are not compared.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import classifier as oc
from oracle import gcn_layer as og
from oracle import h2gcn_model as om
from oracle import keras_adam as ok

from test_sddmm_gpu import LENGTHS, N_COLS, N_ROWS, WIDTHS, _crafted_hops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
BF_MAX = float(torch.finfo(BF).max)            # (2 - 2^-7) * 2^127
SUB_MIN32, SUB_MIN_BF, NORM_MIN = 2.0 ** -149, 2.0 ** -133, 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- helper
def _host(t):
    """(values as float32 numpy, bit patterns as unsigned numpy) of a float32 / bfloat16 tensor or a float32 array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        if t.dtype == BF:
            return t.float().numpy(), t.view(torch.int16).numpy().view(np.uint16)
        assert t.dtype == torch.float32, t.dtype
        t = t.numpy()
    t = np.ascontiguousarray(t)
    assert t.dtype == np.float32, t.dtype
    return t, t.view(np.uint32)


def special_counts(v):
    a = np.abs(v)
    return dict(nan=int(np.isnan(v).sum()), inf=int(np.isinf(v).sum()), subnormal=int(((a > 0) & (a < NORM_MIN)).sum()),
                negative_zero=int(((v == 0) & np.signbit(v)).sum()))


def assert_same_bits_nan_aware(got, want, what=""):
    """NaN exactly where `want` has NaN; everywhere else the same BITS (sign of zero and which infinity included).  NaN payload
    and NaN sign are not compared.  Prints the special-value census of `want`."""
    gv, gb = _host(got)
    wv, wb = _host(want)
    assert gv.shape == wv.shape and gb.dtype == wb.dtype, (what, gv.shape, wv.shape, gb.dtype, wb.dtype)
    c = special_counts(wv)
    print(f"{what}: {wv.size} elements, want holds {c['nan']} NaN, {c['inf']} Inf, {c['subnormal']} subnormal, {c['negative_zero']} -0.0")
    gn, wn = np.isnan(gv), np.isnan(wv)
    assert np.array_equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()), np.argwhere(gn != wn)[:4].tolist())
    bad = (gb != wb) & ~wn
    if bad.any():
        idx = np.argwhere(bad)
        where_sub = (np.abs(wv[bad]) < NORM_MIN) | (np.abs(gv[bad]) < NORM_MIN)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in bits ({int(where_sub.sum())} of them where got or want is "
                             f"zero / subnormal); first at {idx[0].tolist()}: got {gv[tuple(idx[0])]!r} want {wv[tuple(idx[0])]!r}")


def _bits_equal_where_not_nan(a, b):
    (av, ab), (bv, bb) = _host(a), _host(b)
    return np.array_equal(np.isnan(av), np.isnan(bv)) and np.array_equal(ab[~np.isnan(bv)], bb[~np.isnan(bv)])


def rne(a):
    """fp32 numpy -> bf16 the way torch rounds on the CPU (nearest even, overflow to inf, NaN stays NaN)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF)


# ------------------------------------------------------------------------------------------------ 1. the 300 x 300 operand
N = 300


def _symmetric_pattern(lengths, shift, rng):
    """A symmetric 0/1 pattern (no diagonal) whose row i has lengths[(i + shift) % 10] entries: Havel-Hakimi -- a vertex takes
    the neighbours with the most entries still to place -- with random tie-breaking."""
    target = np.array([lengths[(i + shift) % len(lengths)] for i in range(N)])
    rem = target.copy()
    adj = np.zeros((N, N), bool)
    key = rng.random(N)
    for v in sorted(range(N), key=lambda u: (-target[u], key[u])):
        if rem[v] == 0:
            continue
        cand = sorted((u for u in range(N) if u != v and rem[u] > 0 and not adj[v, u]), key=lambda u: (-rem[u], key[u]))
        for u in cand[:rem[v]]:
            adj[v, u] = adj[u, v] = True
            rem[u] -= 1
        rem[v] = 0
    return adj


def _hops(case):
    """Two hops, symmetric in pattern (so that the adjoint can run through a built transpose AND on the forward arrays), every
    length of LENGTHS in each.  Values: U(-1, 1) with explicit zeros; `extremes` adds -0.0, 2^-100 and +-1e30."""
    mats = []
    for k in range(2):
        rng = np.random.default_rng(100 + k)
        m = sp.csr_matrix(_symmetric_pattern(LENGTHS, 3 * k, rng).astype(np.float32))
        m.sort_indices()
        assert (m != m.T).nnz == 0 and set(LENGTHS) <= set(np.diff(m.indptr).tolist())
        data = rng.uniform(-1, 1, m.nnz).astype(np.float32)
        data[::7] = 0.0                                    # stored entries whose value is an explicit zero
        if case == "extremes":
            data[3::7] = -0.0
            data[5::11] = 2.0 ** -100
            data[1::29] = 1e30
            data[2::31] = -1e30
        m.data = data
        mats.append(m)
    return mats


_POOL32 = np.array([0.0, -0.0, SUB_MIN32, -SUB_MIN32, 2.0 ** -127, -2.0 ** -127, NORM_MIN, -NORM_MIN, 1e30, -1e30, FLT_MAX, -FLT_MAX], np.float32)
# the bf16-representable members of the pool; the three that are not (2^-149, 1e30, FLT_MAX) are replaced by their bf16
# neighbours: the smallest bf16 subnormal, bf16(1e30) and the largest finite bf16
_POOLBF = np.array([0.0, -0.0, SUB_MIN_BF, -SUB_MIN_BF, 2.0 ** -127, -2.0 ** -127, NORM_MIN, -NORM_MIN,
                    float(rne(np.float32(1e30)).float()), -float(rne(np.float32(1e30)).float()), BF_MAX, -BF_MAX], np.float32)


def plant_extremes(a, rng, bf16=False, frac=0.02):
    """2 % of the elements of `a` (in place, flat order) take values of the finite-extremes pool."""
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, max(1, int(round(frac * flat.size))), replace=False)
    flat[idx] = (_POOLBF if bf16 else _POOL32)[rng.integers(0, 12, idx.size)]
    return a


def _background(shape, rng, bf16, scale=1.0):
    a = (rng.uniform(-1, 1, shape) * scale).astype(np.float32)
    return rne(a).float().numpy() if bf16 else a


def _poison_rows(a, rows):
    """a [rows, ..., d]: row q gets +Inf, -Inf and NaN at different columns (column 0 always; then every third column, the kind
    rotating with q), the rest of the row stays finite."""
    d = a.shape[-1]
    kinds = (np.inf, -np.inf, np.nan)
    for t, q in enumerate(rows):
        for c in range(0, d, 3):
            a[q, ..., c] = kinds[(t + c // 3) % 3]
    return a


# the "tiny" case: sources U(-1, 1) * 2^-140 -- every source element, product, partial sum and result of the fp32 launches is
# subnormal (or zero; 260 terms stay below 2^-131).  bf16 sources: * 2^-128, so that they keep a few bits on bf16's subnormal
# grid of 2^-133; most results are subnormal, the longest rows' may reach the smallest normals
TINY = {False: 2.0 ** -140, True: 2.0 ** -128}
Q_ROWS = (17, 41, 258)       # chosen on the CPU (with the seeds above): 5 % .. 60 % of the oracle's output rows are non-finite


def _x_of(case, d, bf16):
    """The gather source of the forward launch, [N, d] float32 (bf16: values that bf16 holds exactly)."""
    rng = np.random.default_rng(7000 + d + (500 if bf16 else 0))
    x = _background((N, d), rng, bf16, TINY[bf16] if case == "tiny" else 1.0)
    if case == "extremes":
        plant_extremes(x, rng, bf16)
        big = float(rne(np.float32(1e30)).float()) if bf16 else 1e30
        hop = _hops_cached(case)[0]
        lens = np.diff(hop.indptr)
        # deterministic plants, so that every width yields a subnormal, a NaN, a +Inf and a -Inf (the random 2 % cannot promise
        # that at d = 3): three rows whose neighbour sets are disjoint.  The rows' VALUES are set to match in _hops_cached.
        ra, rb, rc = _plant_rows(hop, lens)
        x[hop.indices[hop.indptr[ra]], 0] = NORM_MIN                    # 0.5 * 2^-126 = 2^-127: a subnormal sum
        j0, j1 = hop.indices[hop.indptr[rb]], hop.indices[hop.indptr[rb] + 1]
        x[j0, 1], x[j1, 1] = big, big                                   # 1e30 * big + (-1e30) * big = inf - inf = NaN
        x[j0, 2], x[j1, 2] = big, 0.5                                   # +inf + finite = +Inf
        x[hop.indices[hop.indptr[rc]], 0] = big                         # -1e30 * big = -Inf
    elif case == "poisoned":
        _poison_rows(x, Q_ROWS)
    return x


def _plant_rows(hop, lens):
    """(a row of one entry, two rows of two entries) of hop 0 whose neighbour sets are pairwise disjoint."""
    ones, twos = np.flatnonzero(lens == 1), np.flatnonzero(lens == 2)
    nb = lambda r: set(hop.indices[hop.indptr[r]:hop.indptr[r + 1]].tolist())
    for ra in ones:
        for rb in twos:
            for rc in twos:
                if rb != rc and not (nb(ra) & nb(rb)) and not (nb(ra) & nb(rc)) and not (nb(rb) & nb(rc)):
                    return int(ra), int(rb), int(rc)
    raise AssertionError("no three rows with disjoint neighbour sets")


_HOPS = {}


def _hops_cached(case):
    if case not in _HOPS:
        mats = _hops(case)
        if case == "extremes":
            hop = mats[0]
            ra, rb, rc = _plant_rows(hop, np.diff(hop.indptr))
            hop.data[hop.indptr[ra]] = 0.5
            hop.data[hop.indptr[rb]:hop.indptr[rb] + 2] = (1e30, -1e30)
            hop.data[hop.indptr[rc]:hop.indptr[rc] + 2] = (-1e30, 1.0)
        _HOPS[case] = mats
    return _HOPS[case]


def _dy_of(case, d, bf16):
    """The gather source of the adjoint, [N, 2, d]."""
    rng = np.random.default_rng(9000 + d + (500 if bf16 else 0))
    g = _background((N, 2, d), rng, bf16, TINY[bf16] if case == "tiny" else 1.0)
    if case == "extremes":
        plant_extremes(g, rng, bf16)
    elif case == "poisoned":
        _poison_rows(g, Q_ROWS)
    return g


def _old_dx(d, scale=1.0):
    """What the accumulate launch adds to: U(-1, 1) * scale holding special values of its own."""
    rng = np.random.default_rng(300 + d)
    a = (rng.uniform(-1, 1, (N, d)) * scale).astype(np.float32)
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, max(6, flat.size // 20), replace=False)
    flat[idx] = np.array([np.inf, -np.inf, np.nan, -0.0, SUB_MIN32, -NORM_MIN, FLT_MAX, -FLT_MAX], np.float32)[rng.integers(0, 8, idx.size)]
    return a


_PLANS = {}


def _plan(case, thr, variant, symmetric):
    from h2gcn_amd import HopPlan

    key = (case, thr, variant, symmetric)
    if key not in _PLANS:
        _PLANS[key] = HopPlan.from_scipy(_hops_cached(case), DEV, build_transpose=True, long_row_threshold=thr, variant=variant,
                                         symmetric_pattern=symmetric)
    return _PLANS[key]


_TREES = {}


def _trees(case, d, thr, bf16):
    """(x, dy, forward tree, adjoint tree) -- the oracle's values, computed once per (case, width, threshold, source dtype)."""
    key = (case, d, thr, bf16)
    if key not in _TREES:
        hops = _hops_cached(case)
        x, dy = _x_of(case, d, bf16), _dy_of(case, d, bf16)
        with np.errstate(all="ignore"):
            _TREES[key] = (x, dy, og.gcn_layer_tree(hops, x, long_threshold=thr), og.gcn_layer_grad_tree(hops, dy, N, long_threshold=thr))
    return _TREES[key]


def _check_degenerate(case, d, x, dy, tree, tree_t, bf16=False):
    """The guards of the value cases, on the ORACLE's output alone."""
    hops = _hops_cached(case)
    if case == "extremes":
        c = special_counts(tree)
        assert c["subnormal"] >= 1 and c["nan"] >= 1 and (tree == np.inf).any() and (tree == -np.inf).any(), (d, c)
    elif case == "tiny":
        assert special_counts(x)["subnormal"] == int((x != 0).sum()) and special_counts(dy)["subnormal"] == int((dy != 0).sum())
        for t in (tree, tree_t):                       # fp32 sources: nothing but subnormals and the zeros of the empty rows
            n_sub, n_nz = special_counts(t)["subnormal"], int((t != 0).sum())
            assert n_nz >= 0.7 * t.size and (n_sub >= 0.5 * n_nz if bf16 else n_sub == n_nz), (d, n_sub, n_nz, t.size)
    else:
        frac = float((~np.isfinite(tree)).any(axis=(1, 2)).mean())
        frac_t = float((~np.isfinite(tree_t)).any(axis=1).mean())
        print(f"poisoned d={d}: {frac:.1%} of the forward's rows and {frac_t:.1%} of the adjoint's are non-finite")
        assert 0.05 <= frac <= 0.60 and 0.05 <= frac_t <= 0.60, (frac, frac_t)
        # the structural fact on its own: (i, k, c) is non-finite iff row i of A_k stores an entry whose column is in Q and
        # X[that row, c] is non-finite -- whatever the entry's value, an explicit zero included (0 * Inf = NaN)
        bad_x, bad_g = ~np.isfinite(x), ~np.isfinite(dy)
        zero_into_q = 0
        want_t = np.zeros((N, d), bool)
        for k, m in enumerate(hops):
            pat = sp.csr_matrix((np.ones(m.nnz, np.float32), m.indices, m.indptr), shape=m.shape)
            want = (pat @ bad_x.astype(np.float32)) > 0
            assert np.array_equal(~np.isfinite(tree[:, k, :]), want), (d, k)
            want_t |= (pat.T @ bad_g[:, k, :].astype(np.float32)) > 0
            zero_into_q += int(((m.data == 0) & np.isin(m.indices, Q_ROWS)).sum())
        assert np.array_equal(~np.isfinite(tree_t), want_t), d
        assert zero_into_q >= 1
        return want, want_t
    return None


F32_WIDTHS = (3, 4, 7, 64, 100, 128, 200)      # 3: the generic column-tiled kernel; the others: the float4 gather kernels
BF16_WIDTHS = (6, 64, 128)
_WALK = {5: "lane group per segment (short rows)", 6: "lane group per segment (binned"}


@pytest.mark.parametrize("thr", (32, 256))
@pytest.mark.parametrize("case", ("extremes", "poisoned", "tiny"))
def test_hop_spmm_bits_on_special_values(case, thr):
    """Forward, adjoint, adjoint with accumulate, fp32 and bf16 sources, fp32 and bf16 outputs == the canonical tree, through
    variants 0 / 5 / 6 and through a built transpose as well as symmetric=True.  `tiny` (sources U(-1, 1) * 2^-140) keeps every
    operand, product, partial sum and result in the subnormal range: what the build does with fp32 subnormals in its
    multiply-adds and in the bf16 conversion of the store is measured by it, not assumed."""
    for symmetric in (False, True):
        for variant in (0, 5, 6):
            plan = _plan(case, thr, variant, symmetric)
            assert plan.has_transpose and (plan.info(0)["n_long_segments"] > 0) == (thr == 32)
            if symmetric:
                assert all(s != "none" for s in plan.transpose_sharing)
            for d in F32_WIDTHS:
                x, dy, tree, tree_t = _trees(case, d, thr, False)
                if variant == 0 and not symmetric:
                    _check_degenerate(case, d, x, dy, tree, tree_t)
                if variant in _WALK and d in (64, 128):            # the forced walk really is the one that runs
                    assert plan.schedule(d)["segment_walk"].startswith(_WALK[variant]), (variant, d, plan.schedule(d))
                tag = f"{case} thr={thr} variant={variant} symmetric={symmetric} d={d}"
                xt, gt = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
                assert_same_bits_nan_aware(plan.spmm(xt), tree, tag + " forward")
                assert_same_bits_nan_aware(plan.spmm_t(gt), tree_t, tag + " adjoint")
                old = _old_dx(d, TINY[False] if case == "tiny" else 1.0)
                with np.errstate(all="ignore"):
                    want = old + tree_t                                # each element is `old + sum`, one fp32 addition
                buf = torch.from_numpy(old).to(DEV)
                plan.spmm_t(gt, out=buf, accumulate=True)
                assert_same_bits_nan_aware(buf, want, tag + " adjoint accumulate")
            for d in BF16_WIDTHS:
                x, dy, tree, tree_t = _trees(case, d, thr, True)
                if variant == 0 and not symmetric:
                    _check_degenerate(case, d, x, dy, tree, tree_t, bf16=True)
                tag = f"{case} thr={thr} variant={variant} symmetric={symmetric} d={d} bf16"
                xb, gb = rne(x).to(DEV), rne(dy).to(DEV)
                assert _bits_equal_where_not_nan(xb.float(), x) and _bits_equal_where_not_nan(gb.float(), dy)   # bf16 holds the sources exactly
                assert_same_bits_nan_aware(plan.spmm(xb, out_dtype=torch.float32), tree, tag + " -> fp32 forward")
                assert_same_bits_nan_aware(plan.spmm(xb), rne(tree), tag + " -> bf16 forward")
                assert_same_bits_nan_aware(plan.spmm_t(gb, out_dtype=torch.float32), tree_t, tag + " -> fp32 adjoint")
                assert_same_bits_nan_aware(plan.spmm_t(gb), rne(tree_t), tag + " -> bf16 adjoint")
                old = _old_dx(d, TINY[False] if case == "tiny" else 1.0)
                with np.errstate(all="ignore"):
                    want = old + tree_t
                buf = torch.from_numpy(old).to(DEV)
                plan.spmm_t(gb, out=buf, accumulate=True)
                assert_same_bits_nan_aware(buf, want, tag + " -> fp32 adjoint accumulate")


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def test_bf16_store_rounds_special_values_like_torch():
    """A crafted plan whose values are powers of two and whose sources are bf16, so every product and every sum is exact in fp32
    and the fp32 value that reaches the store is known by construction.  Two entries per row (they land in the tree's partials
    P0 and P1, the element is P0 + P1); the last row has three: the largest fp32 that still rounds to the largest finite bf16,
    0x7F7F7FFF, has 15 significant bits below the bf16 field and cannot be written as two bf16 values times powers of two.
    An fp32 SUM of -0.0 does not exist (every partial starts from +0 and +0 + -0 = +0); the bf16 -0.0 is reached from a negative
    sum below half the smallest bf16 subnormal."""
    from h2gcn_amd import HopPlan

    p = lambda e: 2.0 ** e
    nan, inf = float("nan"), float("inf")
    # (a, x, b, y, the fp32 sum a*x + b*y as bits -- None: NaN)
    rows = [
        (1.0, nan, 1.0, 1.0, None),                                      # NaN stays NaN (not Inf, not zero)
        (1.0, 1.0, p(-3), nan, None),
        (1.0, inf, 1.0, 1.0, 0x7F800000),                                # +Inf
        (1.0, -inf, 1.0, 1.0, 0xFF800000),                               # -Inf
        (1.0, inf, 1.0, -inf, None),                                     # Inf - Inf
        (0.0, inf, 1.0, 1.0, None),                                      # a stored zero times Inf: the pattern decides
        (p(-20), -p(-126), 1.0, 0.0, 0x80000008),                        # -2^-146, below half the smallest bf16 subnormal -> bf16 -0.0
        (1.0, 8 * p(-133), p(-8), p(-126), 0x00080000 + 0x8000),         # 8 ulp_bf16 + half: an exact tie, to the even 8
        (1.0, 9 * p(-133), p(-8), p(-126), 0x00090000 + 0x8000),         # 9 ulp_bf16 + half: an exact tie, to the even 10
        (1.0, 8 * p(-133), p(-9), 1.984375 * p(-126), 0x00080000 + 0x7F00),    # just below the tie (by 2^-141): down
        (1.0, 8 * p(-133), p(-8), (1 + p(-7)) * p(-126), 0x00080000 + 0x8100),  # just above the tie (by 2^-141): up
        (1.0, p(-133), p(-8), p(-126), 0x00010000 + 0x8000),             # the smallest bf16 subnormal + half: tie, to the even 2
        (1.0, 127 * p(-133), p(-8), p(-126), 0x007F0000 + 0x8000),       # the largest bf16 subnormal + half: tie, up to 2^-126
        (p(-8), p(-126), 0.0, 1.0, 0x00008000),                          # half the smallest bf16 subnormal: tie, to zero
        (1.0, BF_MAX, p(119), 1.0, 0x7F7F8000),                          # bf16 max + half an ulp: tie, to the even Inf
        (-1.0, BF_MAX, -p(119), 1.0, 0xFF7F8000),
    ]
    indptr, indices, data, xs = [0], [], [], []
    for a, x, b, y, _ in rows:
        indices += [len(xs), len(xs) + 1]
        data += [a, b]
        xs += [x, y]
        indptr.append(len(indices))
    # the three-entry row: bf16 max + 0xFF * 2^111 + 0x7F * 2^104 = 0x7F7F7FFF, the largest fp32 below the tie
    indices += [len(xs), len(xs) + 1, len(xs) + 2]
    data += [1.0, p(104), p(98)]
    xs += [BF_MAX, 255.0 * p(7), 127.0 * p(6)]
    indptr.append(len(indices))
    want_bits = [r[4] for r in rows] + [0x7F7F7FFF]
    d = 6
    m = sp.csr_matrix((np.array(data, np.float32), np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(len(want_bits), len(xs)))
    x = np.repeat(np.array(xs, np.float32)[:, None], d, axis=1)
    assert np.array_equal(rne(x).float().numpy().view(np.uint32)[~np.isnan(x)], x.view(np.uint32)[~np.isnan(x)])   # bf16 holds every source exactly
    with np.errstate(all="ignore"):
        tree = og.gcn_layer_tree([m], x)                                  # [rows, 1, d]
    for i, bits in enumerate(want_bits):                                  # the crafted sums are what the comments say
        if bits is None:
            assert np.isnan(tree[i]).all(), i
        else:
            assert (tree[i].view(np.uint32) == bits).all(), (i, hex(bits), tree[i, 0, 0])
    want_bf = rne(tree)
    wb = want_bf.view(torch.int16).numpy().view(np.uint16)[:, 0, 0].tolist()
    assert [hex(b) for b in wb[2:4] + wb[6:]] == [hex(b) for b in (0x7F80, 0xFF80, 0x8000, 0x0008, 0x000A, 0x0008, 0x0009, 0x0002, 0x0080,
                                                                     0x0000, 0x7F80, 0xFF80, 0x7F7F)]
    xb = rne(x).to(DEV)
    plan = HopPlan.from_scipy([m], DEV, build_transpose=True)
    assert_same_bits_nan_aware(plan.spmm(xb, out_dtype=torch.float32), tree, "crafted bf16 -> fp32")
    assert_same_bits_nan_aware(plan.spmm(xb), want_bf, "crafted bf16 -> bf16")
    # the adjoint's store: the same matrix reached as the transpose of its transpose
    plan_t = HopPlan.from_scipy([sp.csr_matrix(m.T)], DEV, build_transpose=True)
    assert_same_bits_nan_aware(plan_t.spmm_t(xb.view(len(xs), 1, d), out_dtype=torch.float32), tree[:, 0, :], "crafted bf16 -> fp32 adjoint")
    assert_same_bits_nan_aware(plan_t.spmm_t(xb.view(len(xs), 1, d)), want_bf[:, 0, :], "crafted bf16 -> bf16 adjoint")


# ------------------------------------------------------------------------------------------------ 2. fused bias / ReLU
def _assert_same_values_nan_aware(got, want, what):
    """NaN exactly where `want` has it; equal VALUES elsewhere (zeros compare equal whatever their sign; +Inf != -Inf)."""
    gv, _ = _host(got)
    wv, _ = _host(want)
    c = special_counts(wv)
    print(f"{what}: want holds {c['nan']} NaN, {c['inf']} Inf, {int((wv == 0).sum())} zeros")
    assert np.array_equal(np.isnan(gv), np.isnan(wv)), (what, "NaN positions differ", int((np.isnan(gv) != np.isnan(wv)).sum()))
    ok_ = np.isnan(wv) | (gv == wv)
    assert ok_.all(), (what, int((~ok_).sum()), gv[~ok_][:4], wv[~ok_][:4])


@pytest.mark.parametrize("thr", (32, 256))
@pytest.mark.parametrize("d", (4, 7, 64, 128))
def test_fused_bias_relu_epilogue_propagates_nan(d, thr):
    """Y = relu(A X + b) in one launch == np.maximum(tree + b, 0): a NaN sum stays NaN (C's fmaxf would store 0), -Inf becomes
    0, +Inf stays -- fp32, bf16 -> fp32 and bf16 -> bf16 (the epilogue runs on the fp32 value, before the rounding)."""
    plan = _plan("poisoned", thr, 0, False)
    rng = np.random.default_rng(40 + d)
    bias = rng.uniform(-0.5, 0.5, d).astype(np.float32)
    bt = torch.from_numpy(bias).to(DEV)
    for bf16 in ((False, True) if d % 2 == 0 else (False,)):
        x, _, tree, _ = _trees("poisoned", d, thr, bf16)
        with np.errstate(all="ignore"):
            pre = tree + bias
            want = np.maximum(pre, np.float32(0))
        assert np.isnan(pre).any() and (pre == np.inf).any() and (pre == -np.inf).any()       # all three reach the epilogue
        assert np.isnan(want).sum() == np.isnan(pre).sum() and not (want == -np.inf).any()
        tag = f"relu epilogue d={d} thr={thr} bf16={bf16}"
        if not bf16:
            _assert_same_values_nan_aware(plan.spmm(torch.from_numpy(x).to(DEV), bias=bt, relu=True), want, tag)
            _assert_same_values_nan_aware(plan.spmm(torch.from_numpy(x).to(DEV), relu=True), np.maximum(tree, np.float32(0)), tag + " no bias")
        else:
            xb = rne(x).to(DEV)
            _assert_same_values_nan_aware(plan.spmm(xb, bias=bt, relu=True, out_dtype=torch.float32), want, tag + " -> fp32")
            _assert_same_values_nan_aware(plan.spmm(xb, bias=bt, relu=True), rne(want), tag + " -> bf16")


def test_sparse_dense_fused_relu_keeps_a_diverged_kernel_visible():
    """SparseDense(activation="relu") on a plan with a transpose is the fused launch (the training configuration): with one NaN
    column in the kernel the embedding is NaN exactly where the unfused composition's is."""
    from h2gcn_amd import HopPlan
    from h2gcn_amd.layers import SparseDense

    feats = _hops_cached("poisoned")[0]
    plan = HopPlan.from_scipy([feats], DEV, build_transpose=True)
    torch.manual_seed(0)
    layer = SparseDense(N, 64, use_bias=True, activation="relu").to(DEV)
    with torch.no_grad():
        layer.bias.uniform_(-0.1, 0.1)
        layer.kernel[:, 5] = float("nan")
    y = layer(plan)
    ref = torch.relu(plan.spmm(layer.kernel.detach())[:, 0, :] + layer.bias.detach())
    lens = np.diff(feats.indptr)
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert bool(torch.isnan(y[:, 5]).cpu()[lens > 0].all()) and int(torch.isnan(y).sum()) == int((lens > 0).sum())
    finite = ~torch.isnan(ref)
    assert torch.equal(y[finite], ref[finite])


# ------------------------------------------------------------------------------------------------ 3. masked metrics
def _labels(n, c, seed, frac):
    rng = np.random.default_rng(seed)
    y = np.zeros((n, c), np.float32)
    y[np.arange(n), rng.integers(0, c, n)] = 1.0
    if n > 4:
        y[rng.choice(n, max(1, n // 10), replace=False)] = 0.0           # unlabelled rows
    mask = rng.random(n) < frac
    mask[0] = True
    return y, mask


def _ce_grad64(z, y, w):
    z64 = z.astype(np.float64)
    zs = z64 - z64.max(1, keepdims=True)
    logp = zs - np.log(np.exp(zs).sum(1, keepdims=True))
    y64 = y.astype(np.float64)
    return w.astype(np.float64)[:, None] * (np.exp(logp) * y64.sum(1, keepdims=True) - y64)


OFFSETS = (("N(0,2)", 0.0), ("N(0,2)+30", 30.0), ("N(0,2)-30", -30.0), ("N(0,2)+1e3", 1e3), ("N(0,2)-1e3", -1e3), ("N(0,2)+1e4", 1e4),
           ("N(0,2)-1e4", -1e4), ("N(0,2)+1e6", 1e6), ("N(0,50)", None))


@pytest.mark.parametrize("n,c", [(5, 3), (64, 7), (257, 47), (1000, 64)])
def test_metrics_and_logit_gradient_are_accurate_at_any_offset(n, c):
    """Loss, accuracy and dZ against the fp64 restatement on the SAME fp32 logits, with the tolerances of test_metrics_gpu.py
    unchanged, for logits N(0, 2) + offset and N(0, 50): three ordinary sets, and four sets whose weight is one-hot on a single
    row each (loss[m] is then that row's cross-entropy: averaging over rows cannot hide a per-row error)."""
    from h2gcn_amd import metrics

    rng = np.random.default_rng(1000 * n + c)
    base = rng.normal(0, 2.0, (n, c))
    wide = rng.normal(0, 50.0, (n, c))
    sets = [_labels(n, c, 1, 0.3), _labels(n, c, 2, 0.6), _labels(n, c, 3, 0.05)]
    y1 = sets[0][0]
    labelled = np.flatnonzero(y1.sum(1) > 0)
    singles = [labelled[0], labelled[len(labelled) // 3], labelled[2 * len(labelled) // 3], labelled[-1]]
    single_sets = []
    for r in singles:
        mk = np.zeros(n, bool)
        mk[r] = True
        single_sets.append((y1, mk))
    all_failures = []
    for name, off in OFFSETS:
        z = (wide if off is None else base + off).astype(np.float32)
        z64 = z.astype(np.float64)
        zt = torch.from_numpy(z).to(DEV)
        worst = dict(loss=0.0, acc=0.0, grad=0.0)
        failures = []
        for kind, group in (("sets", sets), ("one-hot rows", single_sets)):
            ys = [torch.from_numpy(y).to(DEV) for y, _ in group]
            ws_h = [(m / m.sum()).astype(np.float32) for _, m in group]
            ws = [torch.from_numpy(w).to(DEV) for w in ws_h]
            loss, acc = metrics.masked_metrics(zt, ys, ws)
            loss, acc = loss.cpu().numpy(), acc.cpu().numpy()
            for k, (y, m) in enumerate(group):
                ref_l = om.masked_softmax_cross_entropy(z64, y.astype(np.float64), m)
                ref_a = om.masked_accuracy(z64, y.astype(np.float64), m)
                rl = abs(loss[k] - ref_l) / (2e-6 * max(1.0, abs(ref_l)))
                ra = abs(acc[k] - ref_a) / (1e-6 * max(1.0, n ** 0.5))
                worst["loss"], worst["acc"] = max(worst["loss"], rl), max(worst["acc"], ra)
                if not (rl <= 1.0 and ra <= 1.0):
                    failures.append((kind, k, "loss", float(loss[k]), ref_l, "acc", float(acc[k]), ref_a))
            for k in (0, len(group) - 1):                                   # the gradient of the first and the last set
                za = zt.clone().requires_grad_(True)
                metrics.masked_cross_entropy(za, ys[k], ws[k]).backward()
                want = _ce_grad64(z, group[k][0], ws_h[k])
                tol = 3e-6 * max(1e-3, np.abs(want).max()) + 2.5e-7 * float(ws_h[k].max()) + 1e-12
                rg = float(np.abs(za.grad.cpu().numpy() - want).max() / tol)
                worst["grad"] = max(worst["grad"], rg)
                if not rg <= 1.0:
                    failures.append((kind, k, "grad err / tol", rg))
        print(f"metrics n={n} c={c} {name:>11}: worst error / tolerance  loss {worst['loss']:.3f}  accuracy {worst['acc']:.3f}  gradient {worst['grad']:.3f}")
        all_failures += [(name,) + f for f in failures]
    assert not all_failures, (len(all_failures), all_failures[:4])            # (after the loop: the table above is always complete)


def _bits_equal(a, b):
    return np.array_equal(_host(a)[1], _host(b)[1])


def test_metrics_non_finite_rows_follow_the_documented_contract():
    """include/h2gcn_hip.h: rows whose weight is zero in every set are not read -- NaN / Inf there change nothing, their dZ rows
    are exact zeros; a NaN logit in a row a set COVERS makes that set's loss and that dZ row NaN and leaves the other sets'
    bits alone.  (The accuracy of a set that covers a NaN row is not asserted: the reference's argmax on NaN is unspecified.)"""
    from h2gcn_amd import metrics

    n, c = 200, 7
    rng = np.random.default_rng(5)
    z = rng.normal(0, 2.0, (n, c)).astype(np.float32)
    sets = [_labels(n, c, 11, 0.3), _labels(n, c, 12, 0.5), _labels(n, c, 13, 0.1)]
    covered = sets[0][1] | sets[1][1] | sets[2][1]
    free = np.flatnonzero(~covered)
    assert len(free) >= 9
    ys = [torch.from_numpy(y).to(DEV) for y, _ in sets]
    ws = [torch.from_numpy((m / m.sum()).astype(np.float32)).to(DEV) for _, m in sets]

    def run(zz):
        zt = torch.from_numpy(zz).to(DEV)
        loss, acc = metrics.masked_metrics(zt, ys, ws)
        grads = []
        for k in range(3):
            za = zt.clone().requires_grad_(True)
            metrics.masked_cross_entropy(za, ys[k], ws[k]).backward()
            grads.append(za.grad)
        return loss, acc, grads

    zeroed = z.copy()
    zeroed[free] = 0.0
    poisoned = zeroed.copy()
    for t, r in enumerate(free):
        poisoned[r, t % c] = (np.nan, np.inf, -np.inf)[t % 3]
        if t % 4 == 0:
            poisoned[r, :] = (np.nan, np.inf, -np.inf)[(t // 4) % 3]
    l0, a0, g0 = run(zeroed)
    l1, a1, g1 = run(poisoned)
    assert torch.isfinite(l0).all() and _bits_equal(l0, l1) and _bits_equal(a0, a1)
    for k in range(3):
        assert _bits_equal(g0[k], g1[k]), k
        assert bool((g1[k][torch.from_numpy(free).to(DEV)] == 0).all()) and not bool(torch.signbit(g1[k][torch.from_numpy(free).to(DEV)]).any())
    # one NaN logit in a row that set 0 covers and sets 1 and 2 do not
    only0 = np.flatnonzero(sets[0][1] & ~sets[1][1] & ~sets[2][1] & (sets[0][0].sum(1) > 0))
    r = int(only0[0])
    hit = zeroed.copy()
    hit[r, 3] = np.nan
    l2, a2, g2 = run(hit)
    assert bool(torch.isnan(l2[0])), l2
    assert _bits_equal(l2[1:], l0[1:]) and _bits_equal(a2[1:], a0[1:])
    assert bool(torch.isnan(g2[0][r]).all())
    others = np.setdiff1d(np.arange(n), [r])
    assert _bits_equal(g2[0][others], g0[0][others]) and _bits_equal(g2[1], g0[1]) and _bits_equal(g2[2], g0[2])


# ------------------------------------------------------------------------------------------------ 4. dropout + Dense
@pytest.fixture(params=["matrix-core kernels", "small-operand kernels"])
def kernel_family(request):
    """As in test_classifier_gpu.py: the small-operand kernels switched off (every call on the fp32-MFMA kernels) / the shipped
    rule (<= 12288 rows, <= 16 classes, K <= 512: the plain kernels -- both shapes below qualify)."""
    from h2gcn_amd import _capi
    L = _capi.lib()
    old = L.h2gcn_dropout_dense_small_rows(0 if request.param.startswith("matrix") else 12288)
    yield request.param
    L.h2gcn_dropout_dense_small_rows(old)


SEED, STEP = 0x1234_5678_9ABC, 41


def _dd_calls(x, w, b, g, keep, rows):
    """(Z, dX, dW) as numpy float32 through the library: the full call, or -- rows: an ascending int array -- the row-selected
    one (Z, G and dX compact).  x: float32 or bfloat16 on the device."""
    from h2gcn_amd.hops import RowSelection
    from h2gcn_amd.layers import _DropoutDenseFn, _dd_rows_backward, _dd_rows_forward

    step = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    if rows is None:
        xa = x.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        z = _DropoutDenseFn.apply(xa, wa, b, keep, SEED, step)
        z.backward(g)
        dx, dw = xa.grad, wa.grad
    else:
        sel = RowSelection(torch.from_numpy(rows.astype(np.int32)).to(DEV), None, x.shape[0])
        z = _dd_rows_forward(x, w, b, keep, SEED, step, sel)
        dx, dw = _dd_rows_backward(x, w, g, keep, SEED, step, sel, True, True)
    torch.cuda.synchronize()
    return z.detach().cpu().numpy(), dx.float().cpu().numpy(), dw.cpu().numpy()


@pytest.mark.parametrize("keep", (0.5, 0.9))
@pytest.mark.parametrize("n,k,c", [(129, 130, 7), (513, 448, 16)])
def test_dropout_dense_mask_is_a_select(kernel_family, n, k, c, keep):
    """NaN / Inf in X at DROPPED positions never reach Z, dW or dX; one NaN at a KEPT position reaches exactly its row of Z and
    its row of dW; an Inf in one row of G makes that row of dX non-finite at the kept positions and exactly 0 at the dropped
    ones -- in both kernel families, for f32 and bf16 X, in the full and in the row-selected call."""
    rng = np.random.default_rng(n + k + c)
    m = oc.keep_mask(n, k, keep, SEED, STEP)
    w = rng.uniform(-0.3, 0.3, (k, c)).astype(np.float32)
    w[np.abs(w) < 1e-3] = 0.01                                          # no product with G's Inf is 0 * Inf
    b = rng.uniform(-0.5, 0.5, c).astype(np.float32)
    g_full = rng.uniform(-1, 1, (n, c)).astype(np.float32)
    g_full[np.abs(g_full) < 1e-3] = 0.01
    x0 = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    dropped = np.argwhere(~m)
    kept = np.argwhere(m)
    r, q = (int(v) for v in kept[len(kept) // 2])                        # the kept position that gets the NaN
    rows = np.union1d(np.arange(0, n, 2), [r])                          # the selection of the row-selected calls (holds r)
    wt, bt = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    for bf16 in (False, True):
        xbase = rne(x0).float().numpy() if bf16 else x0
        to_dev = lambda a: (rne(a) if bf16 else torch.from_numpy(a)).to(DEV)
        for sel in (None, rows):
            tag = f"{kernel_family} n={n} k={k} c={c} keep={keep} bf16={bf16} rows={'all' if sel is None else len(sel)}"
            idx = np.arange(n) if sel is None else sel
            g = g_full[idx]
            g_scat = np.zeros_like(g_full)
            g_scat[idx] = g
            gt = torch.from_numpy(g).to(DEV)
            # (a) non-finite X at dropped positions only
            xa = xbase.copy()
            pick = dropped[::3]
            xa[pick[:, 0], pick[:, 1]] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(pick)) % 3]
            z, dx, dw = _dd_calls(to_dev(xa), wt, bt, gt, keep, sel)
            with np.errstate(all="ignore"):
                xd = np.where(m, xa.astype(np.float64) / keep, 0.0)
                z_w = oc.dropout_dense(xa, w, b, keep, SEED, STEP)[idx]
                dx_w, dw_w, _ = oc.dropout_dense_grad(xa, w, g_scat, keep, SEED, STEP)
            assert np.isfinite(z_w).all() and np.isfinite(dw_w).all() and np.isfinite(dx_w).all()
            assert np.isfinite(z).all() and np.isfinite(dw).all() and np.isfinite(dx).all(), tag
            assert (np.abs(z - z_w) <= 2e-6 * np.maximum((np.abs(xd) @ np.abs(w) + np.abs(b))[idx], 1.0)).all(), tag
            assert (np.abs(dw - dw_w) <= 2e-6 * np.maximum(np.abs(xd).T @ np.abs(g_scat), 1.0)).all(), tag
            assert (dx[~m[idx]] == 0).all(), tag                          # exactly zero where dropped
            if not bf16:
                assert (np.abs(dx - dx_w[idx]) <= 2e-6 * np.maximum((np.abs(g) @ np.abs(w).T) / keep, 1.0)).all(), tag
            # (b) one NaN at a kept position (r, q)
            xb_ = xbase.copy()
            xb_[r, q] = np.nan
            z, dx, dw = _dd_calls(to_dev(xb_), wt, bt, gt, keep, sel)
            zr = int(np.flatnonzero(idx == r)[0])
            assert np.isnan(z[zr]).all() and np.isfinite(np.delete(z, zr, axis=0)).all(), tag
            assert np.isnan(dw[q]).all() and np.isfinite(np.delete(dw, q, axis=0)).all(), tag
            assert np.isfinite(dx).all(), tag
            # (c) an Inf in row r of G
            gi = g.copy()
            gi[zr, 0] = np.inf
            z, dx, dw = _dd_calls(to_dev(xbase), wt, bt, torch.from_numpy(gi).to(DEV), keep, sel)
            assert (dx[zr][~m[r]] == 0).all(), (tag, "dropped positions of the Inf row must be exactly 0", dx[zr][~m[r]][:8])
            assert (~np.isfinite(dx[zr][m[r]])).all(), tag
            assert np.isfinite(np.delete(dx, zr, axis=0)).all() and (np.delete(dx, zr, axis=0)[~np.delete(m[idx], zr, axis=0)] == 0).all(), tag


# ------------------------------------------------------------------------------------------------ 5. SDDMM
_SDDMM_PLANS = {}


def _sddmm_plan(thr):
    from h2gcn_amd import HopPlan

    if thr not in _SDDMM_PLANS:
        _SDDMM_PLANS[thr] = HopPlan.from_scipy(_crafted_hops(), DEV, long_row_threshold=thr)
    return _SDDMM_PLANS[thr]


def _sddmm_operands(d, kind, bf16):
    rng = np.random.default_rng(2000 + d + (500 if bf16 else 0))
    scale = 2.0 ** -70 if kind == "tiny" else 1.0     # tiny: every product (~2^-140) and every sum is subnormal
    g = _background((N_ROWS, 3, d), rng, bf16, scale)
    x = _background((N_COLS, d), rng, bf16, scale)
    if kind == "extremes":
        plant_extremes(g, rng, bf16)
        plant_extremes(x, rng, bf16)
    elif kind == "poisoned":
        _poison_rows(x, (SDDMM_QX,))
        _poison_rows(g, (SDDMM_QG,))
    return g, x


SDDMM_QX, SDDMM_QG = 57, 9          # a row of X that entries reference, a row of dY that has entries (asserted below)


@pytest.mark.parametrize("d", WIDTHS)
def test_sddmm_bits_are_the_documented_order(d):
    """plan.sddmm == oracle_sddmm_order_f32 bit for bit: thresholds 32 (long segments: one workgroup each) and 256, fp32 at every
    width of test_sddmm_gpu.WIDTHS and bf16 (widened exactly) at the even ones; on U(-1, 1), on the finite-extremes pool, with
    a poisoned row of X and of dY -- there dvals[e] is non-finite iff entry e touches one of them at a column < d -- and on
    operands of magnitude 2^-70, whose products, fma chains, butterfly sums and results are all subnormal."""
    hops = _crafted_hops()
    for kind in ("plain", "extremes", "poisoned", "tiny"):
        for bf16 in ((False, True) if d % 2 == 0 else (False,)):
            g, x = _sddmm_operands(d, kind, bf16)
            with np.errstate(all="ignore"):
                want = og.sddmm_order(hops, g, x)
            if kind == "poisoned":
                touched = 0
                for s, mat in enumerate(hops):
                    rows = np.repeat(np.arange(N_ROWS), np.diff(mat.indptr))
                    hit = (rows == SDDMM_QG) | (mat.indices == SDDMM_QX)
                    assert np.array_equal(~np.isfinite(want[s]), hit), (d, s)
                    touched += int(hit.sum())
                assert touched >= 10
            if kind == "tiny":
                assert all(special_counts(v)["subnormal"] >= 0.9 * v.size for v in want), d
            cvt = (lambda a: rne(a).to(DEV)) if bf16 else (lambda a: torch.from_numpy(a).to(DEV))
            # X as a column slot of a wider NaN-filled buffer: nothing at a column >= d may leak in
            wide = torch.full((N_COLS, d + 6), float("nan"), device=DEV, dtype=BF if bf16 else torch.float32)
            wide[:, :d] = cvt(x)
            for thr in (32, 256):
                plan = _sddmm_plan(thr)
                assert (plan.info(0)["n_long_segments"] > 0) == (thr == 32)
                got = plan.sddmm(cvt(g), wide[:, :d])
                for s in range(3):
                    assert_same_bits_nan_aware(got[s], want[s], f"sddmm {kind} d={d} bf16={bf16} thr={thr} hop {s}")


# ------------------------------------------------------------------------------------------------ 6. Adam
def test_adam_on_gradients_whose_squares_underflow_and_overflow():
    """One tensor of 64 elements, 3 steps, gradients from {0, +-2^-149, +-1e-30, +-1e30, NaN}: g*g underflows to 0, overflows to
    Inf, and inf - inf turns up in v.  NaN exactly where the restatement has it, 2e-6 * max(1, |h|) elsewhere; an element whose
    gradient is always 0 does not move."""
    from h2gcn_amd.optim import KerasAdam

    pool = np.array([0.0, SUB_MIN32, -SUB_MIN32, 1e-30, -1e-30, 1e30, -1e30, np.nan], np.float32)
    rng = np.random.default_rng(8)
    h = rng.normal(size=64).astype(np.float32)
    start = h.copy()
    p = torch.nn.Parameter(torch.from_numpy(h.copy()).to(DEV))
    opt = KerasAdam([p], lr=0.01)
    m, v = np.zeros_like(h), np.zeros_like(h)
    still = np.arange(0, 8)                                               # elements whose gradient is 0 at every step
    for t in range(1, 4):
        g = pool[rng.integers(0, len(pool), 64)]
        g[8:15] = pool[1:]                                                # every member at least once per step ...
        g[16:24] = np.roll(pool, t)                                       # ... and followed by every other one
        g[still] = 0.0
        p.grad = torch.from_numpy(g.copy()).to(DEV)
        opt.step()
        with np.errstate(all="ignore"):
            h, m, v = ok.keras_adam_step(h, g, m, v, t, lr=0.01)
    got = p.detach().cpu().numpy()
    c = special_counts(h)
    print(f"adam: restatement holds {c['nan']} NaN, {c['inf']} Inf; v holds {int(np.isnan(v).sum())} NaN, {int(np.isinf(v).sum())} Inf")
    assert np.isnan(v).any() and np.isinf(v).any()                        # the cases the test is about did occur
    assert np.array_equal(np.isnan(got), np.isnan(h)), (np.flatnonzero(np.isnan(got) != np.isnan(h)), got, h)
    fin = np.isfinite(h)
    assert np.array_equal(got[~fin & ~np.isnan(h)], h[~fin & ~np.isnan(h)])
    assert (np.abs(got[fin] - h[fin]) <= 2e-6 * np.maximum(1.0, np.abs(h[fin]))).all(), np.abs(got[fin] - h[fin]).max()
    assert np.array_equal(got[still].view(np.uint32), start[still].view(np.uint32))
