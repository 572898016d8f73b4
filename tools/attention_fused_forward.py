"""The attention forward without a gradient, chain against fused launch (HopPlan.attention_heads: h2gcn_attention_hops_heads_f32,
csrc/attention_fused.hip), on the synthetic operands of h2gcn_amd/synth.py, both hops, width d (default 128), K heads (default 8):
    (a) the three-launch chain under no_grad     edge_scores_heads -> row_softmax_heads -> spmm_values, [nnz_k, K] arrays between
    (b) the fused launch                         nothing between
Both write a preallocated Y.  Per shape the tool prints the extra device memory each allocates (torch.cuda.max_memory_allocated
over the level before the call), a checksum of Y for both (the fp64 sum and the exact integer sum of all words: they must agree
to every digit) and the times.
usage: python tools/attention_fused_forward.py [--shapes arxiv,products] [--d D] [--heads K] [--reps R] [--rounds Q]
The measuring loop is tools/_launch_timing.py: 3 warm-ups, every launch between its own events, a figure is the median of R
launches (default 12); Q rounds (default 2), the configurations taking turns; the spread between the rounds is the noise.
"of 8 TB/s": the byte model of the FUSED launch for both rows,
    sum_k nnz_k * (4 + 4K + 4d) + n * H * (2K + d) * 4 + (n + 1) * 8 * H
(what the result needs: the chain moves sum_k nnz_k * 16K more, its two per-entry arrays written and read back)."""
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
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
d, K = a.d, a.heads
torch.set_grad_enabled(False)


def extra_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def checksum(t):
    words = int(torch.sum(t.view(torch.int32), dtype=torch.int64))          # exact: every bit of every word counts
    return f"fp64 sum {float(torch.sum(t, dtype=torch.float64))!r}  sum of the words {words}"


for shape in a.shapes.split(","):
    cfg = synth.SHAPES[shape]
    n = cfg["n"]
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, dev) for k in range(2)]
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n)
    H, nnz = plan.n_hops, plan.nnz
    gen = torch.Generator(device=dev).manual_seed(21)
    x = torch.rand((n, d), device=dev, generator=gen) * 2 - 1
    l = torch.rand((n, H, K), device=dev, generator=gen) * 4 - 2
    r = torch.rand((n, H, K), device=dev, generator=gen) * 4 - 2
    y_chain, y_fused = torch.empty((n, H, d), device=dev), torch.empty((n, H, d), device=dev)

    def chain():
        plan.spmm_values(x, plan.row_softmax_heads(plan.edge_scores_heads(l, r, 0.2)), out=y_chain)

    def fused():
        plan.attention_heads(x, l, r, 0.2, out=y_fused)

    fns = {"(a) chain: scores, softmax, aggregation": chain, "(b) fused launch": fused}
    print(f"== {shape}: n = {n}, d = {d}, K = {K}, nonzeros per hop {nnz}; one [nnz_k, K] fp32 array per hop: "
          + ", ".join(f"{z * K * 4 / 2**20:.1f} MiB" for z in nnz))
    warm_up(fns)
    for name, fn in fns.items():
        print(f"   {name}: extra device memory {extra_memory(fn) / 2**20:10.1f} MiB")
        torch.cuda.empty_cache()
    sums = [checksum(y_chain), checksum(y_fused)]
    print(f"   checksum of Y  (a) {sums[0]}\n                  (b) {sums[1]}\n   equal: {sums[0] == sums[1] and torch.equal(y_chain.view(torch.int32), y_fused.view(torch.int32))}")
    med = round_medians(fns, a.reps, a.rounds)
    width = max(len(k) for k in fns)
    nbytes = sum(z * (4 + 4 * K + 4 * d) for z in nnz) + n * H * (2 * K + d) * 4 + (n + 1) * 8 * H
    for k in fns:
        print_bandwidth(k, width, med[k], nbytes)
    names = list(fns)
    print("   (a) / (b): " + "  ".join(f"{p / q:.2f}" for p, q in zip(med[names[0]], med[names[1]])))
    del plan, csr, x, l, r, y_chain, y_fused, fns
    torch.cuda.empty_cache()
