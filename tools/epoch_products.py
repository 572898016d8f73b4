"""One full-batch H2GCN-2 training step at the products shape on ONE GPU (synthetic labels/features): forward
(dense embedding -> concat-free propagation -> classifier), masked CE + L2, backward (adjoint SpMMs), Adam.
usage: python tools/epoch_products.py [hidden] [--dtype f32|bf16] [--steps S] [--stock-classifier] [--train_rows_only]
  --dtype bf16: the model's embedding_dtype=bfloat16 (bf16 concat buffer, bf16 hop launches, bf16 classifier input).
  --train_rows_only: classifier and backward pass on the labelled rows only (the model's train_rows_only=True; the row selection
      is built once, outside the timed steps)."""
import sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from h2gcn_amd import HopPlan, synth
from h2gcn_amd.models import parse_network_setup
from h2gcn_amd.models.H2GCN import H2GCN, make_optimizer
from h2gcn_amd.models._metrics import masked_softmax_cross_entropy
cfg = synth.SHAPES["products"]; n = cfg["n"]; F, C = 100, 47
HIDDEN = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 64
def _opt(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default
ROWS_ONLY = "--train_rows_only" in sys.argv
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}[_opt("--dtype", "f32")]
STEPS = int(_opt("--steps", "20"))
dev = torch.device("cuda:0")
degs = [synth.synth_degrees(n, cfg["nnz_per_hop"], s, n) for s in (123, 124)]
csr = [synth.synth_hop_rows(degs[k], n, (123, 124)[k], 0, n, dev) for k in range(2)]
t0 = time.perf_counter()
plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n, build_transpose=True)
torch.cuda.synchronize(); print(f"plan with device-built transposes: {time.perf_counter() - t0:.2f} s")
feats = synth.synth_features(F, 5, 0, n, dev)
labels = torch.nn.functional.one_hot(torch.randint(0, C, (n,), device=dev), C).float()
mask = torch.rand(n, device=dev) < 0.1
model = H2GCN(parse_network_setup(f"M{HIDDEN}-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", C), input_dim=F, n_hops=2, sparse_input=False,
              l2_regularize_weight=5e-4, fused_classifier="--stock-classifier" not in sys.argv, embedding_dtype=DTYPE,
              train_rows_only=ROWS_ONLY).to(dev)
opt = make_optimizer("adam", model.parameters(), 0.01)
if ROWS_ONLY:
    t0 = time.perf_counter()
    sel = plan.select_rows(mask); labels_c = labels[sel.rows_long].contiguous(); ones = torch.ones(len(sel), device=dev)
    torch.cuda.synchronize(); print(f"row selection ({len(sel)} of {n} rows, sub-plan with its transpose): {time.perf_counter() - t0:.2f} s")
def step():
    model.train(); opt.zero_grad(set_to_none=True)
    if ROWS_ONLY:
        loss = masked_softmax_cross_entropy(model(None, feats, plan, rows=sel), labels_c, ones) + model.regularization_loss()
    else:
        loss = model.loss(model(None, feats, plan), labels, mask)
    loss.backward(); opt.step(); return loss
for _ in range(2): step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(STEPS): l = step()
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / STEPS * 1e3
edges = sum(plan.nnz)
print(f"hidden {HIDDEN} {_opt('--dtype', 'f32')}{' train_rows_only' if ROWS_ONLY else ''}: {STEPS} timed steps; train step {dt:.1f} ms  (loss {l.item():.4f}); 2 G-layers fwd + 2 adjoints = {4 * edges} edge visits -> {4 * edges / dt / 1e6:.2f}e9 edges/s; peak mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
