"""Time of one MultiHeadHopAttention training step (forward + backward, device events) on the synthetic operands of
h2gcn_amd/synth.py, d = 128, K = 8 heads, both hops; operands built as tools/spmm_values_kernels.py builds them (transposes and
the permutation kept).  The step uses the public layer API only, so this file also runs from a checkout that predates the
head-batched calls (csrc/attention_heads.hip): there it times the per-head chain and prints no per-launch table.
usage: python tools/attention_heads_step.py [--shapes arxiv,products] [--d D] [--heads K] [--reps R] [--rounds Q] [--no-kernels]
The measuring loop is tools/_launch_timing.py: a figure is the median of R launches (default 12); Q rounds (default 2), whose
spread is the noise.

With the head-batched calls present, the same process then times the five new launches one by one next to the K single-head
launches they replace.  "of 8 TB/s": the byte model below over the time, as a fraction of 8e12 B/s (both rows of a pair are rated
on the bytes of the head-batched launch: what the result needs, not what K launches move):
    scores forward      sum_k nnz_k * (4 + 4K + 4K)           colidx, the gathered r row, the scores       + n * H * K * 4
    softmax forward     sum_k nnz_k * 8K                      scores in, alpha out
    softmax backward    sum_k nnz_k * 12K                     alpha, dalpha in, dscores out
    scores backward     sum_k nnz_k * (4 + 8K) + nnz_k * (8 + 8K)   row side; column side with perm        + 2 * n * H * K * 4
    sddmm               sum_k nnz_k * (4 + 4d + 4K) + n * H * d * 4
every one + (n + 1) * 8 * H for the row pointers."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from _launch_timing import print_bandwidth, round_medians, warm_up
from h2gcn_amd import HopPlan, MultiHeadHopAttention, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="arxiv,products")
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--no-kernels", action="store_true", help="the step only, no per-launch table")
a = ap.parse_args()
dev = torch.device("cuda:0")
d, K = a.d, a.heads
w = d // K
batched = hasattr(HopPlan, "sddmm_heads")
print(f"head-batched calls: {'present' if batched else 'absent (the per-head chain)'}")

for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2].clone() for c in csr], n, build_transpose=True, keep_permutation=True)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(21)
    x = (torch.rand((n, d), device=dev, generator=gen) * 2 - 1).requires_grad_(True)
    weight = torch.rand((n, H, d), device=dev, generator=gen) * 2 - 1
    torch.manual_seed(22)
    layer = MultiHeadHopAttention(d, K).to(dev)

    def step():
        x.grad = None
        for p in layer.parameters():
            p.grad = None
        (layer(plan, x) * weight).sum().backward()

    print(f"== {shape}: n = {n}, d = {d}, K = {K}, nonzeros per hop {nnz}")
    fns = {"step (forward + backward)": step}
    warm_up(fns)
    med = round_medians(fns, a.reps, a.rounds)
    print("   step (forward + backward)  " + "  ".join(f"round {r}: {t:9.4f} ms" for r, t in enumerate(med["step (forward + backward)"])))
    print(f"   checksum dx {float(x.grad.double().sum()):.9e}  da_l {float(layer.a_l.grad.double().sum()):.9e}")
    x.grad = None
    if batched and not a.no_kernels:
        with torch.no_grad():
            xd = x.detach()
            l, r = torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1, torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1
            lh, rh = [l[:, :, h].contiguous() for h in range(K)], [r[:, :, h].contiguous() for h in range(K)]
            sc = plan.edge_scores_heads(l, r)
            al = plan.row_softmax_heads(sc)
            gr = [torch.rand((z, K), device=dev, generator=gen) for z in nnz]
            sc_h, al_h, gr_h = ([[t[:, h].contiguous() for t in ts] for h in range(K)] for ts in (sc, al, gr))
            out, out_h = [torch.empty_like(t) for t in sc], [torch.empty_like(t) for t in sc_h[0]]
            rows = (n + 1) * 8 * H
            S = sum(nnz)
            pairs = [
                ("scores forward", lambda: plan.edge_scores_heads(l, r, out=out),
                 lambda: [plan.edge_scores(lh[h], rh[h], out=out_h) for h in range(K)], S * (4 + 8 * K) + n * H * K * 4),
                ("softmax forward", lambda: plan.row_softmax_heads(sc, out=out),
                 lambda: [plan.row_softmax(sc_h[h], out=out_h) for h in range(K)], S * 8 * K),
                ("softmax backward", lambda: plan.row_softmax_heads_backward(al, gr, out=out),
                 lambda: [plan.row_softmax_backward(al_h[h], gr_h[h], out=out_h) for h in range(K)], S * 12 * K),
                ("scores backward", lambda: plan.edge_scores_heads_backward(l, r, gr),
                 lambda: [plan.edge_scores_backward(lh[h], rh[h], gr_h[h]) for h in range(K)], S * (12 + 16 * K) + 2 * n * H * K * 4),
                ("sddmm", lambda: plan.sddmm_heads(weight, xd, K, out=out),
                 lambda: [plan.sddmm(weight[:, :, h * w:(h + 1) * w], xd[:, h * w:(h + 1) * w], out=out_h) for h in range(K)],
                 S * (4 + 4 * d + 4 * K) + n * H * d * 4),
            ]
            fns, nbytes = {}, {}
            for name, one, per_head, b in pairs:
                fns[f"{name}: 1 launch [nnz,K]"], fns[f"{name}: {K} single-head launches"] = one, per_head
                nbytes[f"{name}: 1 launch [nnz,K]"] = nbytes[f"{name}: {K} single-head launches"] = b + rows
            warm_up(fns)
            med = round_medians(fns, a.reps, a.rounds)
            width = max(len(k) for k in fns)
            for k in fns:
                print_bandwidth(k, width, med[k], nbytes[k])
            for name, *_ in pairs:
                p, q = med[f"{name}: {K} single-head launches"], med[f"{name}: 1 launch [nnz,K]"]
                print(f"   {name}: {K} launches / 1 launch: " + "  ".join(f"{u / v:.2f}" for u, v in zip(p, q)))
            del l, r, lh, rh, sc, al, gr, sc_h, al_h, gr_h, out, out_h, pairs, fns
    del plan, csr, x, weight, layer
    torch.cuda.empty_cache()
