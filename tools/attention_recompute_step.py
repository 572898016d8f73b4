"""One attention training step (forward + backward, device events), the chain against the recomputing path, in ONE process:
MultiHeadHopAttention and RecomputeMultiHeadHopAttention (the same parameters) take turns on the synthetic operands of
h2gcn_amd/synth.py, d = 128, K = 8 heads, both hops; operands built as tools/attention_heads_step.py builds them.
usage: python tools/attention_recompute_step.py [--shapes arxiv,products] [--d D] [--heads K] [--reps R] [--rounds Q] [--attn_dropout P]
       [--embedding_dtype {float32,bfloat16}]
The measuring loop is tools/_launch_timing.py: a figure is the median of R steps (default 12); Q rounds (default 2), whose spread
is the noise.  Peak memory: torch.cuda.max_memory_allocated over one step of each layer, above what is allocated before it.

Then the three launches of the recomputing step one by one.  "of 8 TB/s": the byte model below over the time, as a fraction of
8e12 B/s (the node terms: the rows a launch reads or writes once):
    forward + stats     sum_k nnz_k * (4 + 4K + 4d)     colidx, the gathered r and x rows     + n * H * (d + 3K) * 4 + n * d * 4
    backward, row side  sum_k nnz_k * (4 + 4K + 4d)     colidx, the gathered r and x rows     + n * H * (2d + 5K) * 4
    backward, col side  sum_k nnz_k * (4 + 16K + 4d)    t_colidx, the gathered g row and l, m, 1/S, delta of row i
                                                                                              + n * d * 8 + n * H * K * 8
every one + (n + 1) * 8 * H for the row pointers.  The row side alone is the backward with need_dl only; the column side is the
full backward minus the row side.

--attn_dropout P (P > 0): the layers that take turns are instead (a) the recomputing layer WITHOUT dropout -- the kernels of the
line above, the baseline -- (b) the recomputing layer with attention dropout P, its mask drawn inside the kernels, and (c) the chain
layer with the same dropout, on alpha * f with the factor arrays; and the launches one by one are timed with and without the mask
(the byte model is unchanged: the factor costs no bytes).  (b) and (c) draw the same mask per step (equal seeds).

--embedding_dtype bfloat16: the layers that take turns are the recomputing layer on float32 embeddings and the same layer on
bfloat16 embeddings (csrc/attention_bf16.hip), the same operands rounded to bf16; then the three launches of each, the bf16 ones on
the byte model above with 2 bytes per element of the d-wide arrays (2d for 4d; y, g, x and dx rows at 2 bytes)."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from _launch_timing import print_bandwidth, round_medians, warm_up
from h2gcn_amd import HopPlan, MultiHeadHopAttention, RecomputeMultiHeadHopAttention, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="arxiv,products")
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--attn_dropout", type=float, default=0.0)
ap.add_argument("--embedding_dtype", choices=("float32", "bfloat16"), default="float32")
a = ap.parse_args()
dev = torch.device("cuda:0")
d, K = a.d, a.heads
if a.embedding_dtype == "bfloat16" and a.attn_dropout > 0:
    ap.error("--embedding_dtype bfloat16 has no attention dropout: the dropout launches are float32 only")


def bf16_shape(shape):
    """--embedding_dtype bfloat16: the fp32 recomputing layer and the bf16 one take turns on the same operands rounded to bf16 (x16,
    and x16.float()), then the three launches of each one by one -- the fp32 ones with the byte model of the docstring, the bf16 ones
    with its 4d terms (and the d-wide node rows) at 2 bytes per element."""
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2].clone() for c in csr], n, build_transpose=True)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(21)
    x16 = (torch.rand((n, d), device=dev, generator=gen) * 2 - 1).to(torch.bfloat16)
    w16 = (torch.rand((n, H, d), device=dev, generator=gen) * 2 - 1).to(torch.bfloat16)
    xs = {"recompute, fp32": x16.float().requires_grad_(True), "recompute, bf16": x16.clone().requires_grad_(True)}
    ws = {"recompute, fp32": w16.float(), "recompute, bf16": w16}
    torch.manual_seed(22)
    layer = RecomputeMultiHeadHopAttention(d, K).to(dev)

    def step_of(name):
        def step():
            xs[name].grad = None
            for p in layer.parameters():
                p.grad = None
            (layer(plan, xs[name]) * ws[name]).sum().backward()
        return step

    print(f"== {shape}: n = {n}, d = {d}, K = {K}, nonzeros per hop {nnz}, embeddings rounded to bfloat16")
    fns = {name: step_of(name) for name in xs}
    warm_up(fns)
    med = round_medians(fns, a.reps, a.rounds)
    for name in fns:
        print(f"   step, {name:18s} " + "  ".join(f"round {r}: {t:9.4f} ms" for r, t in enumerate(med[name])))
    print("   fp32 / bf16: " + "  ".join(f"{u / v:.3f}" for u, v in zip(med["recompute, fp32"], med["recompute, bf16"])))
    for name, fn in fns.items():
        torch.cuda.synchronize()
        for t in xs.values():
            t.grad = None
        for p in layer.parameters():
            p.grad = None
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        print(f"   peak memory of one step above its start, {name:18s} {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:10.1f} MiB   "
              f"checksum dx {float(xs[name].grad.double().sum()):.9e}  da_l {float(layer.a_l.grad.double().sum()):.9e}")
    with torch.no_grad():
        x32, w32 = x16.float(), w16.float()
        l, r = torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1, torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1
        y32, stats = plan.attention_heads_stats(x32, l, r)
        y16 = plan.attention_heads_stats_bf16(x16, l, r)[0]
        o32, o16 = torch.empty_like(y32), torch.empty_like(y16)
        S, rows = sum(nnz), (n + 1) * 8 * H
        fns = {
            "fp32 forward + stats": lambda: plan.attention_heads_stats(x32, l, r, out=o32),
            "bf16 forward + stats": lambda: plan.attention_heads_stats_bf16(x16, l, r, out=o16),
            "fp32 backward, row side (dl only)": lambda: plan.attention_heads_backward(x32, l, r, stats, y32, w32, need_dr=False, need_dx=False),
            "bf16 backward, row side (dl only)": lambda: plan.attention_heads_backward_bf16(x16, l, r, stats, y16, w16, need_dr=False, need_dx=False),
            "fp32 backward, both sides": lambda: plan.attention_heads_backward(x32, l, r, stats, y32, w32),
            "bf16 backward, both sides": lambda: plan.attention_heads_backward_bf16(x16, l, r, stats, y16, w16),
        }
        nbytes, cols = {}, {}
        for tag, e in (("fp32", 4), ("bf16", 2)):   # e: bytes per element of the d-wide arrays
            gather = S * (4 + 4 * K + e * d)
            row_bytes = gather + n * H * (2 * d * e + 5 * K * 4) + rows
            cols[tag] = S * (4 + 16 * K + e * d) + n * d * 2 * e + n * H * K * 8 + rows
            nbytes[f"{tag} forward + stats"] = gather + n * H * (d * e + 3 * K * 4) + n * d * e + rows
            nbytes[f"{tag} backward, row side (dl only)"] = row_bytes
            nbytes[f"{tag} backward, both sides"] = row_bytes + cols[tag]
        warm_up(fns)
        med = round_medians(fns, a.reps, a.rounds)
        width = max(len(k) for k in fns) + 6
        for k in fns:
            print_bandwidth(k, width, med[k], nbytes[k])
        for tag in ("fp32", "bf16"):
            col = [b - c for b, c in zip(med[f"{tag} backward, both sides"], med[f"{tag} backward, row side (dl only)"])]
            print_bandwidth(f"{tag} backward, column side (both - row)", width, col, cols[tag])
    del plan, csr, xs, ws, layer, fns
    torch.cuda.empty_cache()


for shape in a.shapes.split(","):
    if a.embedding_dtype == "bfloat16":
        bf16_shape(shape)
        continue
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
    P = a.attn_dropout
    if P > 0:
        layers = {"recompute, P = 0": RecomputeMultiHeadHopAttention(d, K).to(dev),
                  "recompute, dropout": RecomputeMultiHeadHopAttention(d, K).set_attention_dropout(P, seed=23).to(dev),
                  "chain, dropout": MultiHeadHopAttention(d, K).set_attention_dropout(P, seed=23).to(dev)}
    else:
        layers = {"chain": MultiHeadHopAttention(d, K).to(dev), "recompute": RecomputeMultiHeadHopAttention(d, K).to(dev)}
    first = next(iter(layers.values()))
    for layer in layers.values():
        layer.load_state_dict(first.state_dict())

    def step_of(layer):
        def step():
            x.grad = None
            for p in layer.parameters():
                p.grad = None
            (layer(plan, x) * weight).sum().backward()
        return step

    print(f"== {shape}: n = {n}, d = {d}, K = {K}, nonzeros per hop {nnz}" + (f", attention dropout {P}" if P > 0 else ""))
    fns = {name: step_of(layer) for name, layer in layers.items()}
    warm_up(fns)
    med = round_medians(fns, a.reps, a.rounds)
    for name in fns:
        print(f"   step, {name:18s} " + "  ".join(f"round {r}: {t:9.4f} ms" for r, t in enumerate(med[name])))
    if P > 0:
        for name in ("recompute, P = 0", "chain, dropout"):
            print(f"   {name} / recompute, dropout: " + "  ".join(f"{u / v:.3f}" for u, v in zip(med[name], med["recompute, dropout"])))
    else:
        print("   chain / recompute: " + "  ".join(f"{u / v:.2f}" for u, v in zip(med["chain"], med["recompute"])))
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
        print(f"   peak memory of one step above its start, {name:18s} {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:10.1f} MiB   "
              f"checksum dx {float(x.grad.double().sum()):.9e}  da_l {float(layers[name].a_l.grad.double().sum()):.9e}")
    x.grad = None
    with torch.no_grad():
        xd = x.detach()
        l, r = torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1, torch.rand((n, H, K), device=dev, generator=gen) * 2 - 1
        y, stats = plan.attention_heads_stats(xd, l, r)
        out = torch.empty_like(y)
        S, rows = sum(nnz), (n + 1) * 8 * H
        gather = S * (4 + 4 * K + 4 * d)
        fns = {
            "forward + stats": lambda: plan.attention_heads_stats(xd, l, r, out=out),
            "forward (no stats)": lambda: plan.attention_heads(xd, l, r, out=out),
            "backward, row side (dl only)": lambda: plan.attention_heads_backward(xd, l, r, stats, y, weight, need_dr=False, need_dx=False),
            "backward, both sides": lambda: plan.attention_heads_backward(xd, l, r, stats, y, weight),
        }
        if P > 0:
            mask = (1.0 - P, 23, torch.ones(1, dtype=torch.int64, device=dev))   # keep_prob, seed, step
            yd = plan.attention_heads_stats_dropout(xd, l, r, *mask)[0]
            fns["forward + stats, dropout"] = lambda: plan.attention_heads_stats_dropout(xd, l, r, *mask, out=out)
            fns["backward, row side, dropout"] = lambda: plan.attention_heads_backward_dropout(xd, l, r, stats, yd, weight, *mask,
                                                                                               need_dr=False, need_dx=False)
            fns["backward, both sides, dropout"] = lambda: plan.attention_heads_backward_dropout(xd, l, r, stats, yd, weight, *mask)
            fns["the factor arrays"] = lambda: plan.attention_dropout_factors(K, *mask)
        row_bytes = gather + n * H * (2 * d + 5 * K) * 4 + rows
        col_bytes = S * (4 + 16 * K + 4 * d) + n * d * 8 + n * H * K * 8 + rows
        nbytes = {"forward + stats": gather + n * H * (d + 3 * K) * 4 + n * d * 4 + rows,
                  "forward (no stats)": gather + n * H * (d + K) * 4 + n * d * 4 + rows,
                  "backward, row side (dl only)": row_bytes, "backward, both sides": row_bytes + col_bytes}
        nbytes.update({"forward + stats, dropout": nbytes["forward + stats"], "backward, row side, dropout": row_bytes,
                       "backward, both sides, dropout": row_bytes + col_bytes, "the factor arrays": S * (4 + 4 * K) + rows})
        warm_up(fns)
        med = round_medians(fns, a.reps, a.rounds)
        width = max(len(k) for k in fns) + 2
        for k in fns:
            print_bandwidth(k, width, med[k], nbytes[k])
        col = [b - c for b, c in zip(med["backward, both sides"], med["backward, row side (dl only)"])]
        print_bandwidth("backward, column side (both - row)", width, col, col_bytes)
        del l, r, y, stats, out, fns
    del plan, csr, x, weight, layers
    torch.cuda.empty_cache()
