"""GPU suite: the dynamic (GATv2) edge scores (h2gcn_amd/csrc/edge_scores_dynamic.hip) over EVERY kernel geometry of its dispatch
-- forward(), launch_side() and the coef launch of backward(), restated below and asserted -- against the fp64 restatement
tests/edge_scores_dynamic_ref.py.

Operands: attention_backward_ref.sweep_hops, 371-node hops whose row AND column lengths take 0 .. 340 around every chunk, set and
threshold edge, under the plans (long_row_threshold, rows_per_wave) = (32, 1), (256, 3), (1024, 7).  Every input of a raw launch is a
view with NaN between its rows (u, v, a) or NaN elements before and after the array (each ds[s]): an over-read that is consumed shows
as a NaN.  Outputs are guarded and every launch is made twice (raw_scores / raw_backward of test_edge_scores_dynamic_gpu).  Per shape:
 (a) random operands: scores, du, dv, da within the four bounds of include/h2gcn_hip.h (Reference.*_bound: derived, not measured);
 (b) EXACT operands: u, v multiples of 1/8 in [-2, 2], a multiples of 1/4 in [-2, 2], ds in {-2, -1, 1, 2}, slope 0.5 -- every product
     and every partial sum is an integer multiple of 1/64 below 2^24 units (asserted on the host from the reference's magnitude arrays:
     a condition on the inputs, not a tolerance), so fp32 is exact in ANY order and all four outputs must have the bits of the fp64
     reference cast to fp32.  A lost, doubled or misattributed term cannot hide behind the order of summation;
 (c) the bits of the scores across the three plans, of du / dv across rows_per_wave 1, 3, 7 at long_row_threshold 32 and 256;
 (d) the first and the last head of a K > 1 launch against the K = 1 launch on that head's column slice, bit for bit;
 (e) the six need-flag combinations, (f) the hop selections [0], [1], [0, 1] -- at one shape per geometry.
Beside the sweep: eight hops (rows whose first long segment lies in a later hop) and the partition of the da launch (8, 64, 72, 2040
and 2048 partial rows, with and without the stride loop)."""
import functools
import re

import numpy as np
import pytest
import torch

import attention_backward_ref as sweep
import edge_scores_dynamic_ref as ref
import spmm_driver as drv
from test_edge_scores_dynamic_gpu import G, per_entry, raw_backward, raw_scores, same, uniform
from test_spmm_values_gpu import DEV, make_plan, strided_rows

pytestmark = pytest.mark.gpu

KNOBS = ((32, 1), (256, 3), (1024, 7))        # (long_row_threshold, rows_per_wave); the last: no long segment
MAX_HOPS = int(re.search(r"#define\s+H2GCN_MAX_HOPS\s+(\d+)", (drv.ROOT / "include" / "h2gcn_hip.h").read_text()).group(1))
N_HOPS_MANY = min(8, MAX_HOPS)
SLOPE, SLOPE_EXACT = 0.2, 0.5
NAMES = ("scores", "du", "dv", "da")

# forward geometry (L, NB) -> shapes (d, K).  Packed forms: one pass, several full passes, a part-filled last pass.
SHAPES = {
    (1, 1): [(8, 2), (20, 5), (64, 16), (68, 17), (128, 32), (256, 64)],                     # packed, w = 4: 64 columns per pass
    (2, 2): [(16, 2), (72, 9), (128, 16), (136, 17), (256, 32)],                             # w = 8: 128 columns per pass
    (4, 2): [(48, 3), (128, 8), (144, 9), (256, 16)],                                        # w = 16
    (8, 2): [(64, 2), (96, 3), (128, 4), (160, 5), (256, 8)],                                # w = 32
    (0, 1): [(1, 1), (3, 1), (4, 1), (5, 1), (22, 1), (63, 1), (64, 1),                      # head-aligned, w <= 64
             (24, 2), (48, 2), (60, 3), (252, 7), (240, 4), (256, 4)],                       # (w = 12, 24, 20, 36, 60, 64)
    (0, 2): [(65, 1), (100, 1), (127, 1), (128, 1), (136, 2), (192, 2), (248, 2), (256, 2)],  # 64 < w <= 128 (w = 68, 96, 124, 128)
    (0, 4): [(129, 1), (200, 1), (255, 1), (256, 1)],                                        # w > 128 with d <= 256 forces K = 1
}
GRID = [shape for shapes in SHAPES.values() for shape in shapes]
NEED_FLAGS = [(20, 5), (100, 1), (256, 64)]                                                  # (e): one shape per backward NB
HOP_SELECTION = [(68, 17), (136, 17), (144, 9), (160, 5), (252, 7), (248, 2), (200, 1)]      # (f): one shape per forward geometry
MANY_HOPS = [(64, 16), (100, 1), (256, 32)]                                                  # eight hops: one shape per backward NB


def forward_geometry(d, k):
    """forward() of edge_scores_dynamic.hip -> (L, NB, passes of walk_chunk_packed's column loop)."""
    w = d // k
    if k > 1 and w in (4, 8, 16, 32):
        nb = 1 if w == 4 else 2
        return w // 4, nb, -(-d // (64 * nb))
    return 0, 1 if w <= 64 else 2 if w <= 128 else 4, 1


def backward_nb(d):
    """launch_side() and the coef launch of backward(): the row side, the column side and the da partials alike."""
    return 1 if d <= 64 else 2 if d <= 128 else 4


def legal(d, k):
    """check_operands"""
    return d >= 1 and k >= 1 and d % k == 0 and (k == 1 or (d // k) % 4 == 0) and d <= 256


def coef_blocks(n_rows, rpw):
    """coef_blocks of edge_scores_dynamic.hip: workgroups of the da launch = partial rows per selected hop (n_part)."""
    tiles = -(-n_rows // (4 * rpw))
    return min(2048, -(-tiles // 8) * 8) if n_rows > 0 else 0


def virtual_blocks(hops, rpw, thr):
    """launch_geometry of pattern_walk.hip.h: the blocks of the forward walk the da workgroups stride over (n_virtual)."""
    n_long = sum(int((np.diff(m.indptr) >= thr).sum()) for m in hops)
    tiles = -(-hops[0].shape[0] // (4 * rpw))
    return n_long + -(-tiles // 8) * 8


# (n_rows, rows_per_wave, long_row_threshold).  The last case has no long segment: the only way to n_virtual == n_part.
PARTITION_CASES = [(n, 1, 32) for n in (1, 29, 253, 257, 8160, 8192, 8200, 20000)] + [(24600, 3, 32), (8192, 1, 256)]
PARTITION_SHAPES = {20: (1, 5), 128: (1, 8), 256: (1, 4)}      # d -> the K of the case (at d = 20 neither 4 nor 8 heads are legal: w = 4)
LONG = 40


@functools.lru_cache(maxsize=None)
def partition_hops(n_rows, rpw):
    """Two hops [n_rows, 64]: row lengths cycle 0, 1, 2, 5 (hop 1: 1, 2, 5, 0); rows of 40 entries at row 0, at the last row and at a
    row beyond 8192 * rows_per_wave (the second round of the stride loop at its cap) in hop 0, and one in hop 1 only."""
    lens = [np.tile(np.array(c, dtype=np.int64), n_rows // 4 + 1)[:n_rows].copy() for c in ((0, 1, 2, 5), (1, 2, 5, 0))]
    lens[0][0] = lens[0][n_rows - 1] = LONG
    if 8192 * rpw + 5 < n_rows:
        lens[0][8192 * rpw + 5] = LONG
    if n_rows > 2:
        lens[1][n_rows // 2] = LONG
    return tuple(drv.hop_from_lengths(l, 64, seed=91 + k) for k, l in enumerate(lens))


def test_every_geometry_is_reached_and_the_partition_cases_are_what_they_claim():
    """Needs no GPU work: the dispatch restated above against the shape table and the partition cases."""
    reached, by_nb = {}, {1: [], 2: [], 4: []}
    for d, k in GRID:
        assert legal(d, k), (d, k)
        geom = forward_geometry(d, k)
        reached.setdefault(geom[:2], []).append((d, k, geom[2]))
        by_nb[backward_nb(d)].append((d, k))
    assert set(reached) == set(SHAPES) == {(1, 1), (2, 2), (4, 2), (8, 2), (0, 1), (0, 2), (0, 4)}
    assert len(set(GRID)) == len(GRID) and all(len(v) >= 3 for v in reached.values()), reached
    assert all(forward_geometry(d, k)[:2] == geom for geom, shapes in SHAPES.items() for d, k in shapes), "a shape is filed under another geometry"
    for geom, shapes in reached.items():
        if geom[0] == 0:
            continue
        cols = 64 * geom[1]
        assert any(p == 1 for _, _, p in shapes), f"{geom}: no shape with one pass"
        assert any(p > 1 and d % cols == 0 for d, _, p in shapes), f"{geom}: no shape with several full passes"
        assert any(p > 1 and d % cols != 0 for d, _, p in shapes), f"{geom}: no shape whose last pass is part-filled"
    widths = {d // k for d, k in SHAPES[(0, 1)] + SHAPES[(0, 2)] if k > 1}
    assert widths >= {12, 20, 24, 36, 60, 64, 68, 96, 124, 128}
    assert sum(k > 1 for _, k in SHAPES[(0, 1)]) >= 4 and sum(k > 1 for _, k in SHAPES[(0, 2)]) >= 4
    assert {d for d, k in GRID if k == 1} >= {1, 3, 4, 5, 22, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256}
    assert all(k == 1 for _, k in SHAPES[(0, 4)]), "w > 128 with d <= 256 forces K = 1"
    assert max(k for _, k in GRID) == 64 and {(128, 32), (256, 32), (256, 64)} <= set(GRID)
    for nb, shapes in by_nb.items():
        assert sum(k == 1 for _, k in shapes) >= 3 and sum(k > 1 for _, k in shapes) >= 3, f"backward NB {nb}: {shapes}"
    for table in (NEED_FLAGS, MANY_HOPS):
        assert set(table) <= set(GRID) and sorted(backward_nb(d) for d, _ in table) == [1, 2, 4]
    assert set(HOP_SELECTION) <= set(GRID) and sorted(forward_geometry(*s)[:2] for s in HOP_SELECTION) == sorted(SHAPES)
    assert sorted(backward_nb(d) for d in PARTITION_SHAPES) == [1, 2, 4] and all(legal(d, k) for d, ks in PARTITION_SHAPES.items() for k in ks)
    # the da partition
    parts = {case: (coef_blocks(case[0], case[1]), virtual_blocks(partition_hops(case[0], case[1]), case[1], case[2])) for case in PARTITION_CASES}
    n_parts = {p for p, _ in parts.values()}
    assert {8, 64, 2048} <= n_parts, n_parts
    assert any(64 < p < 2048 and p % 64 for p in n_parts), n_parts
    assert any(p == 2048 and v == p for p, v in parts.values()), "2048 partial rows, every workgroup with one block"
    assert any(p == 2048 and v > 2 * p for p, v in parts.values()), "2048 partial rows, the stride loop run more than twice"
    assert any(p < 2048 and v > p for p, v in parts.values()) and all(v >= p for p, v in parts.values())
    for (n_rows, rpw, thr), (p, v) in parts.items():
        lens = [np.diff(m.indptr) for m in partition_hops(n_rows, rpw)]
        assert lens[0][0] == LONG and lens[0][-1] == LONG and max(int(l.max()) for l in lens) == LONG
        if n_rows > 2:
            only = int(np.flatnonzero(lens[1] == LONG)[0])
            assert lens[0][only] < 32, "a row that is long in hop 1 only"
        if n_rows > 8192 * rpw + 5:
            assert lens[0][8192 * rpw + 5] == LONG
    assert any(n > 8192 * rpw + 5 for n, rpw, _ in PARTITION_CASES)
    # eight hops at long_row_threshold 32: rows that are long in a later hop only, rows long in several, a first long segment beyond hop 0
    lengths = np.stack([np.diff(m.indptr) for m in sweep.sweep_hops(N_HOPS_MANY)])
    is_long = lengths >= KNOBS[0][0]
    first = np.argmax(is_long, axis=0)
    assert (is_long.any(axis=0) & (first >= 1)).any(), "no row whose first long segment is in hop >= 1"
    assert (~is_long[0] & is_long[1:].any(axis=0)).any(), "no row that is long in a later hop only"
    assert (is_long.sum(axis=0) >= 2).any(), "no row that is long in several hops"
    for sel in ([N_HOPS_MANY - 1], [1, N_HOPS_MANY - 2]):
        assert is_long[sel].any(), f"the selection {sel} has no long segment"
    assert (~is_long[1] & is_long[N_HOPS_MANY - 2]).any(), "the selection of two hops has no row that is long in its second hop only"


# ------------------------------------------------------------------ operands
def exact_operands(hops, d, k, seed):
    """(u, v, a, ds) of check (b), with exact zeros and entries with u + v == 0 (asserted)."""
    rng = np.random.default_rng(seed)
    n_rows, n_cols = hops[0].shape
    u = (rng.integers(-16, 17, (n_rows, d)) / 8).astype(np.float32)
    v = (rng.integers(-16, 17, (n_cols, d)) / 8).astype(np.float32)
    a = (rng.integers(-8, 9, (len(hops), d)) / 4).astype(np.float32)
    ds = tuple(rng.choice(np.array([-2, -1, 1, 2], dtype=np.float32), (m.nnz, k)) for m in hops)
    u[n_rows // 2, d // 2] = v[n_cols // 2, 0] = 0
    if d > 1:
        a[0, d // 2] = 0
    rows, cols = ref.entries(hops[0])
    first = hops[0].indptr[:-1][np.diff(hops[0].indptr) > 0][::3]        # the first entry of every third non-empty row of hop 0 ...
    _, keep = np.unique(cols[first], return_index=True)                  # ... one row per column: p = 0 in every column of the entry
    v[cols[first[keep]]] = -u[rows[first[keep]]]
    assert (u == 0).any() and (hops[0].nnz == 0 or ((u[rows] + v[cols] == 0).all(axis=1)).any())
    return u, v, a, ds


def random_operands(hops, d, k, seed):
    rng = np.random.default_rng(seed)
    n_rows, n_cols = hops[0].shape
    return uniform(rng, (n_rows, d)), uniform(rng, (n_cols, d)), uniform(rng, (len(hops), d)), tuple(uniform(rng, (m.nnz, k)) for m in hops)


def exact_condition(want):
    """64 * magnitude < 2^24 for every element of every output: every partial sum, in any order, is an fp32 number."""
    mags = list(want.mag_scores) + [want.mag_du, want.mag_dv, want.mag_da]
    return all((64.0 * m < 2.0 ** 24).all() and (np.round(64.0 * m) == 64.0 * m).all() for m in mags)


def reference(hops, host, k, exact, sel=None):
    u, v, a, ds = host
    sel_ = list(range(len(hops))) if sel is None else sel
    want = ref.Reference(hops, u, v, a[sel_], k, SLOPE_EXACT if exact else SLOPE, ds=[ds[s] for s in sel_], sel=sel)
    if exact:
        assert exact_condition(want), "the exact operands leave the range in which fp32 adds them exactly"
    return want


def guarded_entries(t, k):
    """A per-entry array as the launch takes it ([nnz, K]; K = 1: [nnz]) with G NaN elements before and after it."""
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32).reshape(-1))
    buf = torch.full((t.numel() + 2 * G,), float("nan"), dtype=torch.float32, device=DEV)
    buf[G:G + t.numel()] = t.to(DEV)
    return per_entry(buf[G:G + t.numel()], k)


def device_operands(host, k, sel=None):
    u, v, a, ds = host
    sel = list(range(len(ds))) if sel is None else sel
    return strided_rows(u), strided_rows(v), strided_rows(a[sel]), [guarded_entries(ds[s], k) for s in sel]


def plan_of(hops, thr, rpw):
    return make_plan(hops, build_transpose=True, keep_permutation=True, long_row_threshold=thr, rows_per_wave=rpw)


def launch(plan, ops, k, exact, hops=None, needs=(True, True, True), where=""):
    """-> (scores per selected hop, du, dv, da)"""
    u, v, a, ds = ops
    slope = SLOPE_EXACT if exact else SLOPE
    sc = raw_scores(plan, u, v, a, k, slope, hops=hops, where=where)
    return (sc,) + raw_backward(plan, u, v, a, k, ds, needs=needs, slope=slope, hops=hops, where=where)


def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def compare(got, want, k, exact, where, failures, worst):
    """(a): every element within the header's bound; (b): every element has the bits of the fp64 reference cast to fp32 (+0 for a
    zero: every sum of the kernels starts from +0)."""
    sc, du, dv, da = got
    items = [(f"scores[{s}]", host(t).reshape(-1, k), want.scores[s], want.score_bound(s)) for s, t in enumerate(sc)]
    items += [(n, host(t), w, b) for n, t, w, b in (("du", du, want.du, want.du_bound()), ("dv", dv, want.dv, want.dv_bound()),
                                                  ("da", da, want.da, want.da_bound())) if t is not None]
    for name, g, w, bound in items:
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        if exact:
            bad = g.view(np.int32) != (w + 0.0).astype(np.float32).view(np.int32)
            if bad.any():
                at = tuple(int(i) for i in np.argwhere(bad)[0])
                failures.append(f"{where}: (b) {name} differs from the exact result in {int(bad.sum())} of {bad.size} elements, first at {at}: "
                                f"got {g[at]!r}, exact {w[at]!r}")
        else:
            err = np.abs(g.astype(np.float64) - w)
            ratio = float(np.nan_to_num(err / bound, nan=np.inf).max()) if err.size else 0.0
            key = name.split("[")[0]
            worst[key] = max(worst.get(key, 0.0), ratio)
            if not ratio <= 1.0:
                at = tuple(int(i) for i in np.argwhere(~(err <= bound))[0])
                failures.append(f"{where}: (a) {name}: {int((~(err <= bound)).sum())} of {err.size} elements beyond the bound of include/h2gcn_hip.h, "
                                f"worst error / bound {ratio:.3e}, first at {at} (NaNs {int(np.isnan(g).sum())})")


def same_bits(a, b, what, failures):
    if not same(a, b):
        failures.append(f"{what}: the bits differ")


def report(where, worst):
    print(f"{where} worst error / bound: " + "  ".join(f"{n} {worst[n]:.4f}" for n in NAMES if n in worst))


# ------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("d,k", GRID)
def test_sweep(d, k):
    hops = sweep.sweep_hops()
    w = d // k
    where = f"d {d} K {k}"
    failures, worst = [], {}
    plans = [plan_of(hops, thr, rpw) for thr, rpw in KNOBS]
    results = {}
    for exact in (False, True):
        data = (exact_operands if exact else random_operands)(hops, d, k, seed=1000 + 17 * d + k)
        want = reference(hops, data, k, exact)
        ops = device_operands(data, k)
        assert ops[0].stride(0) == d + 4 and ops[2].stride(0) == d + 4
        res = [launch(plan, ops, k, exact, where=f"{where} knob {knob}") for plan, knob in zip(plans, KNOBS)]
        for got, knob in zip(res, KNOBS):                                                    # (a) / (b), all three plans
            compare(got, want, k, exact, f"{where} thr {knob[0]} rpw {knob[1]}", failures, worst)
        for got, knob in zip(res[1:], KNOBS[1:]):                                            # (c) scores: a function of w alone
            for s in range(len(hops)):
                same_bits(got[0][s], res[0][0][s], f"{where} exact {exact}: (c) scores of hop {s} at knob {knob} against knob {KNOBS[0]}", failures)
        for base, thr in ((res[0], 32), (res[1], 256)):                                      # (c) du / dv: never of rows_per_wave
            for rpw in (1, 3, 7):
                if (thr, rpw) in KNOBS:
                    continue
                _, du, dv, _ = launch(plan_of(hops, thr, rpw), ops, k, exact, needs=(True, True, False), where=f"{where} thr {thr} rpw {rpw}")
                same_bits(du, base[1], f"{where} exact {exact}: (c) du at thr {thr}, rows_per_wave {rpw}", failures)
                same_bits(dv, base[2], f"{where} exact {exact}: (c) dv at thr {thr}, rows_per_wave {rpw}", failures)
        results[exact] = (data, want, ops, res)

    data, want, ops, res = results[False]
    u, v, a, _ = ops
    # ---- (d) a head of the launch has the bits of the K = 1 launch on its column slice
    for h in sorted({0, k - 1}) if k > 1 else ():
        cs = slice(h * w, (h + 1) * w)
        one = launch(plans[0], (u[:, cs], v[:, cs], a[:, cs], [guarded_entries(t[:, h], 1) for t in data[3]]), 1, False, where=f"{where} head {h}")
        for s in range(len(hops)):
            same_bits(one[0][s], res[0][0][s][:, h], f"{where}: (d) scores of hop {s}, head {h} against the K = 1 launch on its columns", failures)
        for n, name in ((1, "du"), (2, "dv"), (3, "da")):
            same_bits(one[n], res[0][n][:, cs], f"{where}: (d) {name} of head {h} against the K = 1 launch on its columns", failures)

    # ---- (e) need flags
    if (d, k) in NEED_FLAGS:
        for needs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            got = launch(plans[1], ops, k, False, needs=tuple(bool(x) for x in needs))
            for need, x, y, name in zip(needs, got[1:], res[1][1:], NAMES[1:]):
                assert (x is None) == (not need)
                if need:
                    same_bits(x, y, f"{where}: (e) {name} under the need flags {needs}", failures)

    # ---- (f) hop selection: the slots of the full launch for the scores, the reference for the gradients
    if (d, k) in HOP_SELECTION:
        for sel in ([0], [1], [0, 1]):
            got = launch(plans[0], device_operands(data, k, sel), k, False, hops=sel, where=f"{where} hops {sel}")
            for slot, s in enumerate(sel):
                same_bits(got[0][slot], res[0][0][s], f"{where}: (f) scores of hop {s} under the selection {sel}", failures)
            compare(got, reference(hops, data, k, False, sel), k, False, f"{where} hops {sel}", failures, worst)

    report(f"{where} {forward_geometry(d, k)} backward NB {backward_nb(d)}", worst)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ eight hops
@pytest.mark.parametrize("d,k", MANY_HOPS)
def test_many_hops(d, k):
    """The long list packs the hop into e & 15; the row side's "first long segment serves the row" looks at the earlier hops."""
    n = N_HOPS_MANY
    hops = sweep.sweep_hops(n)
    plan = plan_of(hops, *KNOBS[0])
    where = f"{n} hops d {d} K {k}"
    failures, worst = [], {}
    for exact in (False, True):
        data = (exact_operands if exact else random_operands)(hops, d, k, seed=2000 + 17 * d + k)
        full = launch(plan, device_operands(data, k), k, exact, where=where)
        compare(full, reference(hops, data, k, exact), k, exact, where, failures, worst)
        for sel in ([n - 1], [1, n - 2]):
            got = launch(plan, device_operands(data, k, sel), k, exact, hops=sel, where=f"{where} hops {sel}")
            for slot, s in enumerate(sel):
                same_bits(got[0][slot], full[0][s], f"{where} exact {exact}: scores of hop {s} under the selection {sel}", failures)
            compare(got, reference(hops, data, k, exact, sel), k, exact, f"{where} hops {sel}", failures, worst)
    report(where, worst)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ the da partition
@pytest.mark.parametrize("d", list(PARTITION_SHAPES))
@pytest.mark.parametrize("n_rows,rpw,thr", PARTITION_CASES)
def test_da_partition(n_rows, rpw, thr, d):
    from h2gcn_amd import _capi

    hops = partition_hops(n_rows, rpw)
    plan = plan_of(hops, thr, rpw)
    n_part = coef_blocks(n_rows, rpw)
    got_bytes = int(_capi.lib().h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, 0, d))
    assert got_bytes == n_part * len(hops) * d * 4, f"workspace {got_bytes} bytes, the restatement has {n_part} partial rows"
    assert int(_capi.lib().h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, 2, d)) == n_part * d * 4
    failures, worst = [], {}
    for k in PARTITION_SHAPES[d]:
        where = f"n_rows {n_rows} rpw {rpw} thr {thr} (n_part {n_part}, n_virtual {virtual_blocks(hops, rpw, thr)}) d {d} K {k}"
        for exact in (True, False):
            data = (exact_operands if exact else random_operands)(hops, d, k, seed=3000 + d + k + n_rows)
            got = launch(plan, device_operands(data, k), k, exact, where=where)      # (the workspace: 0xFF between guard bytes)
            compare(got, reference(hops, data, k, exact), k, exact, where, failures, worst)
    report(f"n_rows {n_rows} rpw {rpw} thr {thr} d {d}", worst)
    assert not failures, "\n".join(failures)
