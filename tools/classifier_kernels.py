"""Per-entry-point times of the dropout + dense kernels (csrc/classifier.hip, classifier_bf16.hip) at the products shape, through
the C ABI: forward, backward-data only, backward-weights only.
usage: python tools/classifier_kernels.py [K] [C] [N] [keep_prob] [--dtype f32|bf16|both] [--against OTHER_LIB.so] [--reps R] [--rounds Q]
                                          [--rows-frac F]
  --dtype    element type of X and dX (default f32; `both`: fp32 and bf16 take turns in one process)
  --against  also time the fp32 entry points of another build of the library (e.g. build/ab/lib_parent.so from
             tools/build_ab_lib.sh), taking turns with this one in the same process
  --rows-frac  also time the row-selected entry points (h2gcn_dropout_dense_rows_* / _backward_rows_*) on a random selection of
             F * N rows, taking turns with the full passes ("rows" in the build column; GB/s and TFLOP/s count the selected rows)
Every configuration is timed in Q rounds (default 2; the spread between the rounds of one configuration is the noise) of R
launches (default 12), each launch between its own pair of device events, after 3 warm-up launches; the median per round is
printed."""
import argparse
import ctypes as C
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from h2gcn_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", default=[])
ap.add_argument("--dtype", choices=["f32", "bf16", "both"], default="f32")
ap.add_argument("--against", default=None)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--rows-frac", type=float, default=None)
a = ap.parse_args()
k = int(a.shape[0]) if len(a.shape) > 0 else 448
c = int(a.shape[1]) if len(a.shape) > 1 else 47
n = int(a.shape[2]) if len(a.shape) > 2 else 2_400_000
keep = float(a.shape[3]) if len(a.shape) > 3 else 0.5
dev = torch.device("cuda:0")
lib = _capi.lib()
libs = {"this build": lib}
if a.against:
    other = C.CDLL(a.against)
    for name in ("h2gcn_dropout_dense_f32", "h2gcn_dropout_dense_backward_f32", "h2gcn_dropout_dense_small_rows"):
        getattr(other, name).restype = getattr(lib, name).restype
        getattr(other, name).argtypes = getattr(lib, name).argtypes
    libs[Path(a.against).name] = other
if os.environ.get("H2GCN_CLS_SMALL_ROWS") is not None:      # rows at or below which the small-operand kernels serve the call (0: never)
    for L in libs.values():
        L.h2gcn_dropout_dense_small_rows(int(os.environ["H2GCN_CLS_SMALL_ROWS"]))
dtypes = {"f32": ["f32"], "bf16": ["bf16"], "both": ["f32", "bf16"]}[a.dtype]
tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
x32 = torch.randn((n, k), device=dev)
x = {d: (x32 if d == "f32" else x32.to(torch.bfloat16)) for d in set(dtypes) | ({"f32"} if a.against else set())}
dx = {d: torch.empty((n, k), device=dev, dtype=tdt[d]) for d in x}
w = torch.randn((k, c), device=dev) * 0.05
b = torch.randn((c,), device=dev)
g = torch.randn((n, c), device=dev)
z = torch.empty((n, c), device=dev)
dw = torch.empty((k, c), device=dev)
ws = torch.empty(int(lib.h2gcn_dropout_dense_workspace_bytes(n, k, c)), dtype=torch.uint8, device=dev)
step = torch.zeros((), dtype=torch.int64, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
m = 0
if a.rows_frac is not None:
    rows = torch.sort(torch.randperm(n, device=dev)[:max(1, int(a.rows_frac * n))]).values.to(torch.int32)
    m = rows.numel()
    g_c, z_c = g[:m].contiguous(), torch.empty((m, c), device=dev)
    dx_c = {d: torch.empty((m, k), device=dev, dtype=tdt[d]) for d in x}


def fwd(L, d, sel=False):
    if sel:
        fn = L.h2gcn_dropout_dense_rows_bf16 if d == "bf16" else L.h2gcn_dropout_dense_rows_f32
        return _capi.check(fn(P(x[d]), k, n, k, P(w), c, P(b), keep, 7, P(step), P(z_c), c, P(ws), ws.numel(), stream, P(rows), m))
    fn = L.h2gcn_dropout_dense_bf16 if d == "bf16" else L.h2gcn_dropout_dense_f32
    _capi.check(fn(P(x[d]), k, n, k, P(w), c, P(b), keep, 7, P(step), P(z), c, P(ws), ws.numel(), stream))


def bwd(L, d, want_dx, want_dw, sel=False):
    if sel:
        fn, extra = (L.h2gcn_dropout_dense_backward_rows_bf16, (_capi.DTYPE_BF16,)) if d == "bf16" else (L.h2gcn_dropout_dense_backward_rows_f32, ())
        return _capi.check(fn(P(x[d]), k, n, k, P(w), c, P(g_c), c, keep, 7, P(step), *extra, P(dx_c[d]) if want_dx else None, k,
                              P(dw) if want_dw else None, P(ws), ws.numel(), stream, P(rows), m))
    fn, extra = (L.h2gcn_dropout_dense_backward_bf16, (_capi.DTYPE_BF16,)) if d == "bf16" else (L.h2gcn_dropout_dense_backward_f32, ())
    _capi.check(fn(P(x[d]), k, n, k, P(w), c, P(g), c, keep, 7, P(step), *extra, P(dx[d]) if want_dx else None, k,
                   P(dw) if want_dw else None, P(ws), ws.numel(), stream))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev)


configs = [("this build", d) for d in dtypes] + ([(Path(a.against).name, "f32")] if a.against else [])
if a.against and ("this build", "f32") not in configs:
    configs.insert(0, ("this build", "f32"))
if m:
    configs += [(f"rows {m}", d) for d in dtypes]
    libs[f"rows {m}"] = lib
reps = a.reps if n > 200_000 else max(a.reps, 200)
for name, call in (("forward", lambda L, d, s: fwd(L, d, s)), ("backward dX", lambda L, d, s: bwd(L, d, True, False, s)),
                   ("backward dW (+ reduction)", lambda L, d, s: bwd(L, d, False, True, s))):
    for rnd in range(a.rounds):            # the configurations take turns
        for which, d in configs:
            sel = which.startswith("rows ")
            nn = m if sel else n
            t = timed(lambda: call(libs[which], d, sel), reps)
            flop = 2.0 * nn * k * ((c + 15) // 16 * 16)
            gb = nn * k * (4 if d == "f32" else 2) / 1e9
            print(f"N={n} K={k} C={c} keep={keep}  {name:26s} {d:4s} {which:18s} round {rnd}  {t:7.3f} ms (median of {reps})   "
                  f"{gb / t * 1e3:6.0f} GB/s of the [N, K] operand   {flop / t / 1e9:6.1f} TFLOP/s fp32 MFMA", flush=True)
