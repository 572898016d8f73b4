"""Times of the values-gradient launch (HopPlan.sddmm: h2gcn_sddmm_hops_f32 / _bf16, csrc/sddmm.hip) next to the forward launch
of the same plan and width (HopPlan.spmm), on the synthetic operands of h2gcn_amd/synth.py, and -- on shapes of at most
--composite-max-nnz nonzeros per hop -- next to what a caller had before the kernel existed: the chunked torch composite
(grad[row_of_entry, s] * x[col]).sum(-1), chunks of 2^20 entries.
usage: python tools/sddmm_kernels.py [--shapes arxiv,products] [--d 128] [--reps R] [--rounds Q] [--composite-max-nnz N]
The measuring loop is tools/_launch_timing.py: a figure is the median of R launches (default 12); Q rounds (default 2), whose
spread is the noise.  "of 8 TB/s": the algorithmic bytes of the launch,
    sum_k nnz_k * (4 + 4 + d*s) + n_rows * H * d*s + (n_rows + 1) * 8 * H        (s = bytes per element of grad / x),
over the time, as a fraction of 8e12 B/s -- the same count for the forward launch, which moves nearly the same bytes."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from _launch_timing import print_bandwidth, round_medians, warm_up
from h2gcn_amd import HopPlan, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="arxiv,products")
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--composite-max-nnz", type=int, default=2_000_000)
a = ap.parse_args()
dev = torch.device("cuda:0")
CHUNK = 1 << 20


def composite(rows, cols, grad, x, out):
    """The torch composite, chunked by hand: it materialises chunk x d products per hop."""
    for s in range(len(cols)):
        for lo in range(0, cols[s].numel(), CHUNK):
            r, c = rows[s][lo:lo + CHUNK], cols[s][lo:lo + CHUNK]
            out[s][lo:lo + CHUNK] = (grad[r, s, :] * x[c, :]).sum(-1)
    return out


for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n, d = cfg["n"], a.d
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n)
    H, nnz = plan.n_hops, plan.nnz
    x32 = synth.synth_features(d, synth.SEED_X, 0, n, dev)
    g32 = synth.synth_features(H * d, synth.SEED_X + 1, 0, n, dev).view(n, H, d)
    ops = {"f32": (g32, x32), "bf16": (g32.to(torch.bfloat16), x32.to(torch.bfloat16))}
    dv = [torch.empty(z, device=dev) for z in nnz]
    y = {"f32": torch.empty((n, H, d), device=dev), "bf16": torch.empty((n, H, d), device=dev, dtype=torch.bfloat16)}
    configs = {}
    for name, (g, x) in ops.items():
        configs[f"sddmm {name}"] = (lambda g=g, x=x: plan.sddmm(g, x, out=dv), 4 if name == "f32" else 2)
        configs[f"spmm  {name}"] = (lambda x=x, name=name: plan.spmm(x, out=y[name]), 4 if name == "f32" else 2)
    with_composite = max(nnz) <= a.composite_max_nnz
    if with_composite:
        rows = [torch.repeat_interleave(torch.arange(n, device=dev), c[0][1:] - c[0][:-1]) for c in csr]
        cols = [c[1].long() for c in csr]
        dv_c = [torch.empty(z, device=dev) for z in nnz]
        configs["torch composite f32"] = (lambda: composite(rows, cols, g32, x32, dv_c), 4)
    print(f"== {shape}: n = {n}, nonzeros per hop {nnz}, d = {d}, schedule of the forward launch: {plan.schedule(d)}")
    fns = {k: fn for k, (fn, _) in configs.items()}
    warm_up(fns)
    if with_composite:      # same quantity: the composite's order of summation is torch's, so compare with a tolerance
        plan.sddmm(g32, x32, out=dv)
        err = max(float((p - q).abs().max()) for p, q in zip(dv, dv_c))
        print(f"   max |kernel - composite| = {err:.3e}")
    med = round_medians(fns, a.reps, a.rounds)
    for k, (_, s) in configs.items():
        nbytes = sum(z * (4 + 4 + d * s) for z in nnz) + n * H * d * s + (n + 1) * 8 * H
        print_bandwidth(k, 22, med[k], nbytes)
    for name in ops:
        r = [p / q for p, q in zip(med[f"sddmm {name}"], med[f"spmm  {name}"])]
        print(f"   sddmm / spmm {name}: " + "  ".join(f"{v:.3f}" for v in r))
    if with_composite:
        r = [p / q for p, q in zip(med["torch composite f32"], med["sddmm f32"])]
        print("   torch composite / sddmm f32: " + "  ".join(f"{v:.2f}" for v in r))
    del plan, csr, ops, configs, fns, x32, g32, dv, y
    torch.cuda.empty_cache()
