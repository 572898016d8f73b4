"""Times of the row-softmax launches (HopPlan.row_softmax / row_softmax_backward: h2gcn_row_softmax_hops_f32 /
h2gcn_row_softmax_backward_hops_f32, csrc/row_softmax.hip) on the synthetic operands of h2gcn_amd/synth.py, both hops in one launch,
next to what a caller had before the kernels existed: the torch composite over a row-of-entry index per hop,
    forward    m = scatter_reduce(amax);  e = exp(s - m[row]);  S = index_add(e);  alpha = e / S[row]
    backward   D = index_add(alpha * g);  ds = alpha * (g - D[row])
(the row index -- repeat_interleave, 8 B per nonzero -- is built once, outside the timed region).
usage: python tools/row_softmax_kernels.py [--shapes arxiv,products] [--reps R] [--rounds Q]
The measuring loop is tools/_launch_timing.py: a figure is the median of R launches (default 12); Q rounds (default 2), whose
spread is the noise.  "of 8 TB/s": the byte model of the launch,
    forward    sum_k nnz_k * 8  + (n_rows + 1) * 8 * H          backward   sum_k nnz_k * 12 + (n_rows + 1) * 8 * H,
over the time, as a fraction of 8e12 B/s (the composite is rated on the same bytes: what the result needs, not what it moves)."""
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


def composite_forward(rows, n, scores, out):
    for s, r in enumerate(rows):
        m = torch.full((n,), float("-inf"), device=dev).scatter_reduce(0, r, scores[s], "amax")
        e = torch.exp(scores[s] - m[r])
        total = torch.zeros(n, device=dev).index_add_(0, r, e)
        torch.div(e, total[r], out=out[s])
    return out


def composite_backward(rows, n, alpha, grad, out):
    for s, r in enumerate(rows):
        dot = torch.zeros(n, device=dev).index_add_(0, r, alpha[s] * grad[s])
        torch.mul(alpha[s], grad[s] - dot[r], out=out[s])
    return out


for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(14)
    scores = [4.0 * torch.randn(z, device=dev, generator=gen) for z in nnz]
    grad = [torch.rand(z, device=dev, generator=gen) * 2 - 1 for z in nnz]
    rows = [torch.repeat_interleave(torch.arange(n, device=dev), c[0][1:] - c[0][:-1]) for c in csr]   # built once, not timed
    alpha, ds = [torch.empty(z, device=dev) for z in nnz], [torch.empty(z, device=dev) for z in nnz]
    alpha_c, ds_c = [torch.empty(z, device=dev) for z in nnz], [torch.empty(z, device=dev) for z in nnz]
    plan.row_softmax(scores, out=alpha)
    configs = {
        "row_softmax forward": (lambda: plan.row_softmax(scores, out=alpha), 8),
        "torch composite forward": (lambda: composite_forward(rows, n, scores, alpha_c), 8),
        "row_softmax backward": (lambda: plan.row_softmax_backward(alpha, grad, out=ds), 12),
        "torch composite backward": (lambda: composite_backward(rows, n, alpha, grad, ds_c), 12),
    }
    seg = plan.segment_classes(128)["per_hop"]
    print(f"== {shape}: n = {n}, nonzeros per hop {nnz}, segments per hop (short <= 16 / medium / long): "
          + ", ".join(f"{h['segments']['short']} / {h['segments']['medium']} / {h['segments']['long']}" for h in seg))
    fns = {k: fn for k, (fn, _) in configs.items()}
    warm_up(fns)
    # same quantities: the composite's exp and order of summation are torch's, so compare with a tolerance
    print(f"   max |kernel - composite|: forward {max(float((p - q).abs().max()) for p, q in zip(alpha, alpha_c)):.3e}, "
          f"backward {max(float((p - q).abs().max()) for p, q in zip(ds, ds_c)):.3e}")
    med = round_medians(fns, a.reps, a.rounds)
    for k, (_, per_nnz) in configs.items():
        nbytes = sum(z * per_nnz for z in nnz) + (n + 1) * 8 * H
        print_bandwidth(k, 26, med[k], nbytes)
    for d in ("forward", "backward"):
        r = [p / q for p, q in zip(med[f"torch composite {d}"], med[f"row_softmax {d}"])]
        print(f"   torch composite / row_softmax {d}: " + "  ".join(f"{v:.2f}" for v in r))
    del plan, csr, scores, grad, rows, alpha, ds, alpha_c, ds_c, configs, fns
    torch.cuda.empty_cache()
