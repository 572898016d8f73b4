"""CPU suite of tests/spmm_driver.py: the graph builders, the restatement of launch()'s work split at its thresholds, and the
COVERAGE of the case lists the GPU sweep (tests/test_spmm_classes_sweep_gpu.py) runs -- every claim of every case is checked
against the restatement here, and every family must contain the (spw, mpw, NS, list count, group ratio, class edge, threshold)
its docstring names.  A case list that stops reaching a path fails here, without a GPU."""
import numpy as np
import pytest

import spmm_driver as sd

WF = sd.WF


def test_constants_come_from_the_sources():
    assert (sd.SHORT_MAX, sd.SHORT_SUM_HOPS, sd.WAVES_PER_BLOCK, sd.NUM_XCD) == (16, 4, 4, 8) and WF == 12288
    with pytest.raises(RuntimeError):
        sd._constant("spmm_kernels.hip.h", "kNoSuchConstant")


def test_builders_give_the_prescribed_lengths():
    lengths = np.concatenate([np.array([0, 1, 16, 17, 0, 255, 256, 513, 3, 0, 64, 65]) + (k % 2) * (np.arange(12) % 3) for k in range(12)])
    m = sd.hop_from_lengths(lengths, 700, 1, cover_residues=(1, 255))
    assert m.shape == (len(lengths), 700) and np.array_equal(sd.row_lengths(m), lengths)
    assert m.indices.max() < 699 and (np.abs(m.data) < 1).all()
    for r in range(m.shape[0]):
        c = m.indices[m.indptr[r]:m.indptr[r + 1]]
        assert (np.diff(c) > 0).all()
    a = sd.hop_with_transposed_lengths(lengths, 700, 2)
    assert a.shape == (700, len(lengths)) and np.array_equal(sd.transposed_lengths(a), lengths)
    assert np.array_equal(sd.row_lengths(a.T.tocsr()), lengths) and a.has_sorted_indices
    with pytest.raises(AssertionError):
        sd.hop_from_lengths([5, 5, 5, 5], 700, 3, cover_residues=(1, 255))     # 4 segments cannot start on 32 residues
    with pytest.raises(AssertionError):
        sd.hop_from_lengths([700], 700, 3)


def test_classes_and_counts():
    l = np.array([0, 15, 16, 17, 255, 256, 8, 9])
    assert sd.classes(l, 256).tolist() == [0, 0, 0, 1, 1, 2, 0, 0]
    assert sd.classes(l, 17).tolist() == [0, 0, 0, 2, 2, 2, 0, 0]          # short_max = 16: no medium class
    assert sd.classes(l, 9).tolist() == [0, 2, 2, 2, 2, 2, 0, 2]
    assert sd.classes(l, 1).tolist() == [0, 2, 2, 2, 2, 2, 2, 2]           # only empty rows are short
    assert sd.classes(l, 512).tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
    assert sd.class_counts([l, l[::-1]], 256, False) == [(5, 2, 1), (5, 2, 1)]
    assert sd.class_counts([l, l[::-1]], 256, True) == [(4, 2, 2)]


def test_work_split_at_the_thresholds():
    spw = lambda n, **kw: sd.work_split([n], [0], 1, False, **kw)["spw"]  # noqa: E731
    assert [spw(n) for n in (1, 8 * WF - 1, 8 * WF, 16 * WF - 1, 16 * WF, 32 * WF - 1, 32 * WF, 64 * WF - 1, 64 * WF, 640 * WF)] == \
        [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert sd.work_split([4 * WF, 4 * WF], [0, 0], 2, False)["spw"] == 8              # the lists of a launch are pooled
    mpw = lambda n, n_sel, adj, **kw: sd.work_split([1], [n], n_sel, adj, **kw)["mpw"]  # noqa: E731
    assert [mpw(n, 1, False) for n in (0, WF - 1, 2 * WF - 1, 2 * WF, 5 * WF + 3, 8 * WF, 100 * WF)] == [1, 1, 1, 2, 5, 8, 8]
    for n_sel in (1, 2, 3, 4):
        assert [mpw(n, n_sel, True) for n in (0, 2 * WF, 4 * WF - 1, 4 * WF + 1, 100 * WF)] == [1, 2, 3, 4, 4]
    # the knobs: taken only inside their valid ranges
    assert spw(5, env={"H2GCN_SHORT_PER_WAVE": "64"}) == 64 and spw(5, env={"H2GCN_SHORT_PER_WAVE": "6"}) == 4
    assert spw(5, env={"H2GCN_SHORT_PER_WAVE": "68"}) == 4 and spw(5, env={"H2GCN_SHORT_PER_WAVE": "0"}) == 4
    assert mpw(5, 4, True, env={"H2GCN_MED_PER_WAVE": "8"}) == 8 and mpw(5, 4, True, env={"H2GCN_MED_PER_WAVE": "17"}) == 1
    assert mpw(5, 1, False, env={"H2GCN_MED_PER_WAVE": "64"}) == 64
    # workgroups: chunk-major pads every hop to the longest list, hop-major does not; groups of 8
    w = sd.work_split([257, 0, 17], [43, 300, 280], 3, False)
    assert (w["short_blocks"], w["sblocks"], w["short_groups"], w["padded"]) == ([17, 0, 2], 51, 7, True)
    assert (w["med_blocks"], w["med_end"], w["med_groups"]) == ([11, 75, 70], [11, 86, 156], 20)
    w = sd.work_split([257, 0, 17], [43, 300, 280], 3, False, env={"H2GCN_SHORT_HOP_MAJOR": "1"})
    assert (w["sblocks"], w["short_end"], w["short_groups"], w["hop_major"]) == (19, [17, 17, 19], 3, True)
    w = sd.work_split([257], [33], 2, True)
    assert (w["sblocks"], w["short_groups"], w["med_groups"], w["padded"]) == (17, 3, 2, False)


def _built(cases):
    for c in cases:
        hops = c.make()
        yield c, hops, sd.check_claims(c, hops)


def _round_kinds(lengths, rpw, G, lpr, thr):
    """kinds of in-tile rounds a wave walk of rows_per_wave = rpw makes over `lengths` (G rows per round inside a wave's rows)"""
    kinds = set()
    for row0 in range(0, len(lengths), rpw):
        rows = lengths[row0:row0 + rpw]
        for b in range(0, len(rows), G):
            r = rows[b:b + G]
            if len(rows) < rpw:
                kinds.add("partial last wave")
            elif (r <= lpr).all():
                kinds.add("all short")
            elif (r == lpr + 1).sum() == 1 and (r <= lpr + 1).all():
                kinds.add(("one LPR+1", int(np.flatnonzero(r == lpr + 1)[0])))
            elif (r >= thr).sum() == 1 and (r[r < thr] <= lpr).all():
                kinds.add(("one long", int(np.flatnonzero(r >= thr)[0])))
    return kinds


@pytest.mark.parametrize("thr", sd.THRESHOLDS)
def test_coverage_class_edges(thr):
    t = thr or sd.DEFAULT_THR
    Ls = sd.edge_lengths(thr)
    assert set(sd.LEN_SHORT + sd.LEN_MEDIUM + sd.LEN_LONG + (t - 1, t, t + 1)) <= set(Ls)
    cases = sd.family_edges(thr)
    assert {(c.variant, c.d, c.slice_cols) for c in cases if not c.bf16} >= {(v, d, s) for v in (6, 5, 0) for d, s in sd.WIDTHS}
    assert {(c.rpw, c.d, c.slice_cols) for c in cases if c.variant == 5 and not c.bf16} == {(w, d, s) for w in (0, 1, 3, 7) for d, s in sd.WIDTHS}
    last = set()
    for c, hops, seen in _built(cases):
        h0, h1 = (sd.row_lengths(m) for m in hops)
        n, w = len(h0), max(c.rpw, 1)
        T = 4 * w
        last |= {int(h0[-1]), int(h1[-1])}
        assert w == 1 or n % w != 0                                   # a last wave with rows_here < rows_per_wave
        for L in set(Ls) - {int(h0[-1])}:
            assert set((np.flatnonzero(h0 == L) % 4).tolist()) == {0, 1, 2, 3}, (c.name, L)
            rows = np.flatnonzero(h1 == L)
            assert (rows % T == 0).any() and (rows % T == T - 1).any(), (c.name, L)
        for x in sd.ROUND_EDGES + (t,):
            for h in (h0, h1):
                alone = np.flatnonzero((h == x) & (np.roll(h, 1) == 3) & (np.roll(h, -1) == 3))
                assert set((alone % w).tolist()) == set(range(w)), (c.name, x)
        if c.variant == 5 and c.rpw in (3, 7) and t > 33:
            lpr, G = (16, 4) if sd.slice_of(c.d, c.slice_cols) == 64 else (32, 2)
            want = {"all short", "partial last wave"} | {(k, p) for k in ("one LPR+1", "one long") for p in range(min(G, c.rpw))}
            for h in (h0, h1):
                kinds = _round_kinds(h, c.rpw, G, lpr, t)
                assert want <= kinds, (c.name, want - kinds)
        if c.variant == 6 and not c.bf16:
            cnt = seen[("fwd", None)]["counts"]
            assert all(s > 0 and l > 0 for s, _, l in cnt) and all((m > 0) == (t > 17) for _, m, _ in cnt), (c.name, cnt)
    assert set(Ls) <= last, sorted(set(Ls) - last)                    # every edge length closes some graph (row n - 1)
    if thr == 0:
        assert {(c.variant, c.d, c.slice_cols) for c in cases if c.bf16} == {(v, d, s) for v in (6, 5, 0) for d, s in sd.WIDTHS}
        assert all(c.rpw == 3 for c in cases if c.bf16 and c.variant == 5)


def _sum_round_kinds(lens, rpw, G, lpr, thr):
    """kinds of in-tile SUM rounds over the selected hops' lengths `lens` [n_sel, n]: a row is long-owned if any of its segments
    is long, wide if one is longer than a lane group takes (min(LPR, thr - 1)), short otherwise"""
    owned, wide = (lens >= thr).any(0), (lens > min(lpr, thr - 1)).any(0)
    kinds = set()
    for row0 in range(0, lens.shape[1], rpw):
        n_rows = min(rpw, lens.shape[1] - row0)
        for b in range(0, n_rows, G):
            o, w = owned[row0 + b:row0 + min(b + G, n_rows)], wide[row0 + b:row0 + min(b + G, n_rows)]
            if n_rows < rpw:
                kinds.add("partial last wave")
            elif not w.any():
                kinds.add("all short")
            elif o.sum() == 1:
                kinds.add(("long-owned", int(np.flatnonzero(o)[0])))
            elif not o.any() and w.sum() == 1:
                kinds.add(("wide", int(np.flatnonzero(w)[0])))
    return kinds


@pytest.mark.parametrize("thr", sd.THRESHOLDS)
def test_coverage_class_edges_adjoint(thr):
    t = thr or sd.DEFAULT_THR
    cases = sd.family_edges_adjoint(thr)
    assert {(c.variant, c.rpw, c.d, c.slice_cols) for c in cases if not c.bf16} == \
        {(v, w, d, s) for v, w in ((6, 0), (0, 0), (5, 3), (5, 7)) for d, s in sd.WIDTHS}
    if thr == 0:
        assert {(c.d, c.slice_cols) for c in cases if c.bf16} == set(sd.WIDTHS) and {c.variant for c in cases if c.bf16} == {6, 5}
    for c, hops, seen in _built(cases):
        assert len({m.nnz for m in hops}) == 1                        # hops of equal nonzero count
        if c.variant == 6 and not c.bf16:
            assert [len(s) if s else 5 for s in c.adj] == [1, 2, 3, 4, 5]
            for ns in (2, 3, 4):
                r = seen[("adj", tuple(range(ns)))]
                s, m, l = r["counts"][0]
                assert r["walk"] == "lists" and r["listed"] == s and min(s, l) > 0 and (m > 0) == (t > 17)
                if thr == 0:
                    assert m >= ns * 40 and l >= ns * 5               # short in all but ONE hop; one long segment
            assert seen[("adj", None)]["listed"] == 0
        if c.variant == 5:
            # SUM rounds of G rows at this width: all short, a long-owned row / a row too wide at every position of a round
            lpr, G = (16, 4) if sd.slice_of(c.d, c.slice_cols) == 64 else (32, 2)
            assert c.rpw >= 3 and min(G, c.rpw) >= 2
            lens = np.stack([sd.transposed_lengths(m) for m in hops])
            for sel in c.adj:
                kinds = _sum_round_kinds(lens[list(range(5)) if sel is None else sel], c.rpw, G, lpr, t)
                want = {"all short", "partial last wave"} | {("long-owned", p) for p in range(min(G, c.rpw))}
                if t > lpr + 1:
                    want |= {("wide", p) for p in range(min(G, c.rpw))}
                assert want <= kinds, (c.name, sel, want - kinds)


def test_coverage_list_counts():
    built = list(_built(sd.family_counts()))
    for direction in ("fwd", "adj"):
        single = [(c, seen[(direction, None)]) for c, _, seen in built if (direction, None) in seen and "counts" in c.tags]
        single = [(c, r) for c, r in single if r["n_sel"] == 1]
        assert {c.d for c, _ in single} == {64, 128}
        for d in (64, 128):
            got = [r["counts"][0] for c, r in single if c.d == d]
            assert {s for s, _, _ in got} >= set(sd.COUNTS_SHORT) and {m for _, m, _ in got} >= set(sd.COUNTS_MEDIUM)
            assert {l for _, _, l in got} >= {0, 1, 3}
            assert {s % 16 for s, _, _ in got} >= {0, 1, 15} and {s % 128 for s, _, _ in got if s >= 127} >= {127, 0, 1}
        assert all(r["spw"] == 4 and r["mpw"] == 1 for _, r in single if r["walk"] == "lists")
        ratio = {c.tags["counts"]: (r["short_groups"], r["med_groups"]) for c, r in single if r["walk"] == "lists"}
        want = {"n:0": (3, 0), "1:n": (1, 4), "1:1": (1, 1), "1:5": (1, 5), "5:1": (5, 1), "3:2": (3, 2)}
        assert {k: ratio[v] for k, v in sd.RATIOS.items()} == want and sd.RATIOS["1:n"][0] == 1
    two = [seen[("adj", None)] for c, _, seen in built if "adj 2 hops" in c.name]
    assert len(two) == 4 and all(r["n_sel"] == 2 and r["walk"] == "lists" for r in two)
    multi = [(c, seen[("fwd", None)]) for c, _, seen in built if "per_hop" in c.tags]
    assert {r["n_sel"] for _, r in multi} == {2, 3} and {c.d for c, _ in multi} == {64, 128}
    assert any(sorted(x[0] for x in r["counts"])[:1] == [0] and max(x[0] for x in r["counts"]) == 257 for _, r in multi)
    for _, r in multi:
        assert r["padded"] and r["sblocks"] == max(r["short_blocks"]) * r["n_sel"] > sum(r["short_blocks"])


def test_coverage_per_wave_steps():
    fwd_spw, fwd_mpw, adj = {}, set(), None
    for c, hops, seen in _built(sd.family_steps()):
        if ("fwd", None) in seen:
            r = seen[("fwd", None)]
            fwd_spw.setdefault(r["spw"], set()).add(r["G"])
            fwd_mpw.add(r["mpw"])
            if c.d == 8 and r["spw"] > 4 or "spw=4" in c.name:
                n = r["listed"]
                assert n % (4 * r["spw"]) and n % r["spw"] and n % 4          # partial last workgroup, wave and round
        else:
            adj = seen
            assert len({m.nnz for m in hops}) == 1
    assert set(fwd_spw) == {4, 8, 16, 32, 64} and fwd_spw[8] == {2, 4} and fwd_mpw >= {1, 2, 5, 8}
    assert {r["n_sel"] for r in adj.values()} == {2, 3, 4}
    for r in adj.values():
        assert r["mpw"] == 4 and r["spw"] >= 8 and r["counts"][0][1] >= 4 * WF + 1 and r["counts"][0][1] % 16


def test_coverage_views_and_knobs():
    views = sd.family_views()
    assert {(c.tags["off"], c.tags["tail"]) for c in views} == {(o, t) for o in (0, 1, 15, 31) for t in (64, 0)}
    assert {(c.variant, c.d) for c in views} == {(v, d) for v in (6, 5) for d in (64, 128)}
    assert all(c.views[0][0][0] != c.views[0][0][1] for c in views)         # colidx and vals at different offsets
    list(_built(views))
    built = [(c, c.make()) for c in sd.family_knobs()]
    for env in ({"H2GCN_SHORT_HOP_MAJOR": "1", "H2GCN_SHORT_PER_WAVE": "8", "H2GCN_MED_PER_WAVE": "2"}, {"H2GCN_SHORT_HOP_MAJOR": "1"},
                {"H2GCN_SHORT_PER_WAVE": "64", "H2GCN_MED_PER_WAVE": "8"}):
        reached = sd.knob_claims(built, env)
        assert {d for d, _ in reached} == {"fwd", "adj"}
        assert all(r["hop_major"] == ("H2GCN_SHORT_HOP_MAJOR" in env) for _, r in reached)
