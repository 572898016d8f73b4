"""One full-batch H2GCN-2 training step at the products shape on ONE GPU (synthetic labels/features): forward
(dense embedding -> concat-free propagation -> classifier), masked CE + L2, backward (adjoint SpMMs), Adam.
usage: python tools/epoch_products.py [hidden] [--dtype f32|bf16] [--steps S] [--stock-classifier] [--train_rows_only] [--symmetric]
  --dtype bf16: the model's embedding_dtype=bfloat16 (bf16 concat buffer, bf16 hop launches, bf16 classifier input).
  --train_rows_only: classifier and backward pass on the labelled rows only (the model's train_rows_only=True; the row selection
      is built once, outside the timed steps).
  --symmetric: symmetric hop plans (HopPlan(symmetric_pattern=True)) next to plans with built transposes, in ONE process: the two
      synthetic patterns are generated at half the products nonzeros and symmetrised (A + A^T, so the operands keep the products
      size), with SYM values from h2gcn_hop_normalize (bit-symmetric: indices and values are shared).  Prints each plan's
      construction time (host clock around a device synchronise; three constructions of each kind, taking turns), device_bytes() and the device's free memory before / after,
      then times the training steps with the two plans taking turns (one step each, device events) and the peak memory of each."""
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
def symmetric_main():
    from h2gcn_amd import operands
    GiB = 2.0 ** 30
    csr = []
    for k, seed in enumerate((123, 124)):
        rp, ci, _ = synth.synth_hop_rows(synth.synth_degrees(n, cfg["nnz_per_hop"] // 2, seed, n), n, seed, 0, n, dev)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
        key = torch.unique(torch.cat([rows * n + ci.long(), ci.long() * n + rows]))        # A + A^T pattern
        del rows, rp, ci
        r, c = torch.div(key, n, rounding_mode="floor"), (key % n).to(torch.int32).contiguous()
        del key
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
        del r
        csr.append((rowptr, c, operands.normalize_pattern_device((rowptr, c), n, operands.SYM_NORMALIZED)))
    torch.cuda.empty_cache()
    print(f"symmetrised operands: n = {n}, nonzeros per hop {[int(c[1].numel()) for c in csr]}")
    plans = {}
    for rnd in range(3):   # the first construction of each kind also loads its kernels: the repeats are the steady state
        for name, kw in (("transposed", {}), ("symmetric", dict(symmetric_pattern=True))):
            torch.cuda.synchronize(); free0 = torch.cuda.mem_get_info()[0]; t0 = time.perf_counter()
            plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n, build_transpose=True, **kw)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0; free1 = torch.cuda.mem_get_info()[0]
            print(f"{name} plan, construction {rnd + 1}: {dt:.3f} s; device_bytes {plan.device_bytes() / GiB:.3f} GiB; device memory free "
                  f"{free0 / GiB:.2f} -> {free1 / GiB:.2f} GiB; sharing {plan.transpose_sharing}")
            plans.setdefault(name, plan)   # (the steps below run on the first pair; a repeat is released right away)
            del plan
    feats = synth.synth_features(F, 5, 0, n, dev)
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (n,), device=dev), C).float()
    mask = torch.rand(n, device=dev) < 0.1
    model = H2GCN(parse_network_setup(f"M{HIDDEN}-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", C), input_dim=F, n_hops=2, sparse_input=False,
                  l2_regularize_weight=5e-4, fused_classifier="--stock-classifier" not in sys.argv, embedding_dtype=DTYPE,
                  train_rows_only=ROWS_ONLY).to(dev)
    opt = make_optimizer("adam", model.parameters(), 0.01)
    sels = {name: plan.select_rows(mask) for name, plan in plans.items()} if ROWS_ONLY else {}
    if ROWS_ONLY:
        any_sel = sels["transposed"]; labels_c = labels[any_sel.rows_long].contiguous(); ones = torch.ones(len(any_sel), device=dev)
    def step(name):
        model.train(); opt.zero_grad(set_to_none=True)
        if ROWS_ONLY:
            loss = masked_softmax_cross_entropy(model(None, feats, plans[name], rows=sels[name]), labels_c, ones) + model.regularization_loss()
        else:
            loss = model.loss(model(None, feats, plans[name]), labels, mask)
        loss.backward(); opt.step(); return loss
    for name in plans:
        for _ in range(2): step(name)
    ms = {name: [] for name in plans}
    for _ in range(STEPS):
        for name in plans:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); l = step(name); e1.record(); e1.synchronize(); ms[name].append(e0.elapsed_time(e1))
    tag = f"hidden {HIDDEN} {_opt('--dtype', 'f32')}{' train_rows_only' if ROWS_ONLY else ''}"
    for name in plans:
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); step(name); torch.cuda.synchronize()
        v = sorted(ms[name])
        print(f"{tag}, {name} plan: {STEPS} timed steps (alternating); train step mean {sum(v) / len(v):.2f} ms, median {v[len(v) // 2]:.2f} ms, "
              f"min {v[0]:.2f} ms; peak mem {torch.cuda.max_memory_allocated() / GiB:.2f} GiB (allocator) + {plans[name].device_bytes() / GiB:.2f} GiB "
              f"(plan) = {(torch.cuda.max_memory_allocated() + plans[name].device_bytes()) / GiB:.2f} GiB  (loss {l.item():.4f})")
if "--symmetric" in sys.argv:
    symmetric_main(); sys.exit(0)
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
