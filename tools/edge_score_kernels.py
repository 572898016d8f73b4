"""Times of the edge-score launches (HopPlan.edge_scores / edge_scores_backward: h2gcn_edge_scores_hops_f32 /
h2gcn_edge_scores_backward_hops_f32, csrc/edge_scores.hip) on the synthetic operands of h2gcn_amd/synth.py, both hops in one
launch, next to what a caller has without the kernels: the torch composite over a row-of-entry index per hop,
    forward    pre = l_s[row] + r_s[col];  score = leaky_relu(pre)
    backward   t = leaky_relu_backward(g, pre);  dl_s = index_add(row, t);  dr_s = index_add(col, t)
(the int64 row and column indices -- 8 B per nonzero each -- and the per-hop contiguous l_s / r_s are built once, outside the
timed region, and the composite's backward reads the pre its forward saved instead of recomputing it).
usage: python tools/edge_score_kernels.py [--shapes arxiv,products] [--reps R] [--rounds Q]
The measuring loop is tools/_launch_timing.py: a figure is the median of R launches (default 12); Q rounds (default 2), whose
spread is the noise.  "of 8 TB/s": the byte model of the launch, node = (n_rows + 1) * 8 * H + (n_rows + n_cols) * 4 * H,
    forward, backward row side    sum_k nnz_k * 12 + node        backward column side    sum_k nnz_k * 16 + node
(both sides: the sum of the two), over the time, as a fraction of 8e12 B/s (the composite is rated on the same bytes: what the
result needs, not what it moves)."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from _launch_timing import print_bandwidth, round_medians, warm_up
from h2gcn_amd import HopPlan, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="arxiv,products")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
SLOPE = 0.2


def composite_forward(rows, cols, lt, rt, pre, out):
    for s, (r, c) in enumerate(zip(rows, cols)):
        torch.add(lt[s][r], rt[s][c], out=pre[s])
        torch.ops.aten.leaky_relu.out(pre[s], SLOPE, out=out[s])
    return out


def composite_backward(rows, cols, n, pre, grad, col_side):
    dl, dr = torch.zeros((len(rows), n), device=dev), torch.zeros((len(rows), n), device=dev) if col_side else None
    for s, (r, c) in enumerate(zip(rows, cols)):
        t = torch.ops.aten.leaky_relu_backward(grad[s], pre[s], SLOPE, False)
        dl[s].index_add_(0, r, t)
        if col_side:
            dr[s].index_add_(0, c, t)
    return dl, dr


for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n, build_transpose=True, keep_permutation=True)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(16)
    l, r = torch.randn((n, H), device=dev, generator=gen), torch.randn((n, H), device=dev, generator=gen)
    grad = [torch.rand(z, device=dev, generator=gen) * 2 - 1 for z in nnz]
    rows = [torch.repeat_interleave(torch.arange(n, device=dev), c[0][1:] - c[0][:-1]) for c in csr]   # built once, not timed
    cols = [c[1].to(torch.int64) for c in csr]
    lt, rt = l.t().contiguous(), r.t().contiguous()
    scores, scores_c, pre = ([torch.empty(z, device=dev) for z in nnz] for _ in range(3))
    composite_forward(rows, cols, lt, rt, pre, scores_c)
    configs = {
        "edge_scores forward": (lambda: plan.edge_scores(l, r, SLOPE, out=scores), 12),
        "torch composite forward": (lambda: composite_forward(rows, cols, lt, rt, pre, scores_c), 12),
        "edge_scores backward dl": (lambda: plan.edge_scores_backward(l, r, grad, SLOPE, need_dr=False), 12),
        "torch composite backward dl": (lambda: composite_backward(rows, cols, n, pre, grad, False), 12),
        "edge_scores backward dl+dr": (lambda: plan.edge_scores_backward(l, r, grad, SLOPE), 28),
        "torch composite backward dl+dr": (lambda: composite_backward(rows, cols, n, pre, grad, True), 28),
    }
    seg = plan.segment_classes(128)["per_hop"]
    print(f"== {shape}: n = {n}, nonzeros per hop {nnz}, segments per hop (short <= 16 / medium / long): "
          + ", ".join(f"{h['segments']['short']} / {h['segments']['medium']} / {h['segments']['long']}" for h in seg))
    fns = {k: fn for k, (fn, _) in configs.items()}
    warm_up(fns)
    # the forward has one order: the same bits; the backward's order of summation is torch's (atomic), so compare with a tolerance
    dl, dr = plan.edge_scores_backward(l, r, grad, SLOPE)
    dl_c, dr_c = composite_backward(rows, cols, n, pre, grad, True)
    print(f"   forward bits equal the composite's: {all(torch.equal(p, q) for p, q in zip(scores, scores_c))};  "
          f"max |kernel - composite|: dl {float((dl - dl_c.t()).abs().max()):.3e}, dr {float((dr - dr_c.t()).abs().max()):.3e}")
    med = round_medians(fns, a.reps, a.rounds)
    node = (n + 1) * 8 * H + 2 * n * 4 * H
    for k, (_, per_nnz) in configs.items():
        nbytes = sum(z * per_nnz for z in nnz) + node * (2 if per_nnz == 28 else 1)
        print_bandwidth(k, 31, med[k], nbytes)
    for d in ("forward", "backward dl", "backward dl+dr"):
        ratio = [p / q for p, q in zip(med[f"torch composite {d}"], med[f"edge_scores {d}"])]
        print(f"   torch composite / edge_scores {d}: " + "  ".join(f"{v:.2f}" for v in ratio))
    del plan, csr, l, r, grad, rows, cols, lt, rt, scores, scores_c, pre, configs, fns, dl, dr, dl_c, dr_c
    torch.cuda.empty_cache()
