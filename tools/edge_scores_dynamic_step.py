"""The dynamic (GATv2) edge scores against the launches they share a gather stream with, in ONE process, on the synthetic operands of
h2gcn_amd/synth.py (built as tools/attention_recompute_step.py builds them), d = 128, K = 8 heads, both hops.
usage: python tools/edge_scores_dynamic_step.py [--shapes arxiv,products] [--d D] [--heads K] [--reps R] [--rounds Q]
The measuring loop is tools/_launch_timing.py: a figure is the median of R launches (default 12) between device events after warm-up;
Q rounds (default 2), whose spread is the noise; the candidates take turns.

The launches one by one, each with its own algorithmic bytes over the time as a fraction of 8e12 B/s (S = sum_k nnz_k, H hops, n nodes,
rows = (n + 1) * 8 * H for the row pointers; a node row that every entry of a segment shares is counted once per segment):
    sddmm_heads (the yardstick)     S * (4 + 4d + 4K)        colidx, the gathered x row, the K results        + n * H * d * 4 + rows
    dynamic scores, forward         S * (4 + 4d + 4K)        colidx, the gathered v row, the K scores         + n * d * 4 + H * d * 4 + rows
    dynamic backward, row side (du) S * (4 + 4d + 4K)        colidx, the gathered v row, ds of the entry      + n * d * 8 + rows
    spmm_values_t (the yardstick)   S * (4 + 4 + 4K + 4d)    t_colidx, perm, the values through it, the gathered dY row     + n * d * 4 + rows
    dynamic backward, column (dv)   S * (4 + 4 + 4K + 4d)    t_colidx, perm, ds through it, the gathered u row              + n * d * 8 + rows
    dynamic backward, da            S * (4 + 4d + 4K)        the row side's stream again                      + n * d * 4 + G * H * d * 8 + rows
(du / dv / da alone are the backward with one need flag; G: the partial rows of the workspace.)

Then one training step (forward + backward) and its peak memory (torch.cuda.max_memory_allocated above what is allocated before it)
of DynamicHopAttention against MultiHeadHopAttention on the same plan and inputs."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from _launch_timing import print_bandwidth, round_medians, warm_up
from h2gcn_amd import DynamicHopAttention, HopPlan, MultiHeadHopAttention, _capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="arxiv,products")
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
d, K = a.d, a.heads
if K < 2:
    ap.error("--heads: the yardstick sddmm_heads and the [nnz, K] arrays of this tool need K >= 2")

for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2].clone() for c in csr], n, build_transpose=True, keep_permutation=True)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(21)
    rand = lambda *s: torch.rand(s, device=dev, generator=gen) * 2 - 1     # noqa: E731
    print(f"== {shape}: n = {n}, d = {d}, K = {K}, nonzeros per hop {nnz}")
    with torch.no_grad():
        u, v, att, gy = rand(n, d), rand(n, d), rand(H, d), rand(n, H, d)
        ds = [rand(m, K) if K > 1 else rand(m) for m in nnz]
        out = [torch.empty_like(t) for t in ds]
        ydx = torch.empty((n, d), device=dev)
        S, rows = sum(nnz), (n + 1) * 8 * H
        G = int(_capi.lib().h2gcn_edge_scores_dynamic_workspace_bytes(plan._handle, plan._mask(None), d)) // (H * d * 4)
        bwd = lambda **needs: plan.edge_scores_dynamic_backward(u, v, att, ds, K, **needs)     # noqa: E731
        fns = {
            "sddmm_heads": lambda: plan.sddmm_heads(gy, v, K, out=out),
            "dynamic scores, forward": lambda: plan.edge_scores_dynamic(u, v, att, K, out=out),
            "dynamic backward, row side (du)": lambda: bwd(need_dv=False, need_da=False),
            "spmm_values_t": lambda: plan.spmm_values_t(gy, ds, out=ydx),
            "dynamic backward, column side (dv)": lambda: bwd(need_du=False, need_da=False),
            "dynamic backward, da": lambda: bwd(need_du=False, need_dv=False),
            "dynamic backward, all three": lambda: bwd(),
        }
        row_stream, col_stream = S * (4 + 4 * d + 4 * K), S * (8 + 4 * K + 4 * d)
        nbytes = {
            "sddmm_heads": row_stream + n * H * d * 4 + rows,
            "dynamic scores, forward": row_stream + n * d * 4 + H * d * 4 + rows,
            "dynamic backward, row side (du)": row_stream + n * d * 8 + rows,
            "spmm_values_t": col_stream + n * d * 4 + rows,
            "dynamic backward, column side (dv)": col_stream + n * d * 8 + rows,
            "dynamic backward, da": row_stream + n * d * 4 + G * H * d * 8 + rows,
        }
        nbytes["dynamic backward, all three"] = sum(nbytes[k] for k in fns if k.startswith("dynamic backward,") and k in nbytes)
        warm_up(fns)
        med = round_medians(fns, a.reps, a.rounds)
        width = max(len(k) for k in fns) + 2
        for k in fns:
            print_bandwidth(k, width, med[k], nbytes[k])
        for name, base in (("dynamic scores, forward", "sddmm_heads"), ("dynamic backward, row side (du)", "sddmm_heads"),
                           ("dynamic backward, column side (dv)", "spmm_values_t")):
            print(f"   {name} / {base}: " + "  ".join(f"{x / y:.3f}" for x, y in zip(med[name], med[base])))
        print(f"   workspace of da: {G} partial rows per hop, {G * H * d * 4 / 2 ** 20:.2f} MiB")
        del fns, ds, out, u, v, gy, ydx
    # one training step of the two layers on the same plan and inputs
    x = rand(n, d).requires_grad_(True)
    weight = rand(n, H, d)
    torch.manual_seed(22)
    layers = {"MultiHeadHopAttention": MultiHeadHopAttention(d, K).to(dev), "DynamicHopAttention": DynamicHopAttention(d, K).to(dev)}

    def step_of(layer):
        def step():
            x.grad = None
            for p in layer.parameters():
                p.grad = None
            (layer(plan, x) * weight).sum().backward()
        return step

    fns = {name: step_of(layer) for name, layer in layers.items()}
    warm_up(fns)
    med = round_medians(fns, a.reps, a.rounds)
    for name in fns:
        print(f"   step, {name:22s} " + "  ".join(f"round {r}: {t:9.4f} ms" for r, t in enumerate(med[name])))
    print("   dynamic / static: " + "  ".join(f"{x_ / y_:.2f}" for x_, y_ in zip(med["DynamicHopAttention"], med["MultiHeadHopAttention"])))
    for name, fn in fns.items():
        torch.cuda.synchronize()
        x.grad = None
        for p in layers[name].parameters():
            p.grad = None
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        print(f"   peak memory of one step above its start, {name:22s} {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:10.1f} MiB   "
              f"checksum dx {float(x.grad.double().sum()):.9e}")
    del plan, csr, x, weight, layers, fns
    torch.cuda.empty_cache()
