"""Test driver for the eight classifier entry points (h2gcn_dropout_dense_{,backward_}{,rows_}{f32,bf16}; include/h2gcn_hip.h).

`Driver.call` makes ONE configuration -- element types of X / dX, full-matrix or row-selected, dX only / dW only / both, bias or
none -- through ctypes, on buffers in which everything the kernels must not touch is adversarial:

  X          a column slot of a wider buffer whose other columns are NaN, two NaN rows after the last one; fp32: odd row stride,
             slot one element in (rows only 4-byte aligned); bf16: even stride, 4-byte aligned base.  Row-selected calls: every
             UNSELECTED row of X is NaN, and the row list is followed by entries that name a NaN row
  G          ldg = C + 3, NaN padding, two NaN rows after the last one
  Z, dX, dW  slots with guard rows / columns / elements of a sentinel value, which must be intact afterwards
  workspace  only 16-byte aligned, h2gcn_dropout_dense_workspace_bytes(...) bytes + a 256-byte tail, EVERY byte 0xFF (stale
             contents read as NaN) before each of the two API calls; head and tail must be intact afterwards

and makes it TWICE: the two rounds must leave the same bits in every output buffer.  `reference` is the fp64 restatement
(oracle/classifier.py: the mask bit for bit from keep_mask, the products as dropout_dense / dropout_dense_grad spell them --
tests/test_oracle_tree_and_classifier.py pins that equality) for any row subset, `check` compares one call with it, and
`run_shape` runs every assertion the classifier sweep makes at one shape.

Tolerances (tests/test_classifier_gpu.py): an fp32 output is an exact-fp32 multiply-add chain, so against fp64
|got - want| <= 2e-6 * max(sum |terms|, 1) =: b;  a bf16 dX adds one rounding to an 8-bit significand: b + 2^-8 (|want| + b)."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import classifier as oc

DEV = "cuda:0"
BF = torch.bfloat16
VARIANTS = (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"))     # (X, dX) element types
TOL = 2e-6
# the keep values, steps and seeds of the sweep (tests/test_classifier_sweep_gpu.py; the CPU suite runs the generator over them too)
KEEPS = (1 / 256, 0.25, 0.75, 255 / 256, 0.999, 65534 / 65536)
STEPS = (0, 41, 2 ** 32 + 41, (7 << 40) + 3, 2 ** 63 - 1)
SEEDS = (0, 0x9ABC, 0x1234 << 32, 2 ** 64 - 1)
SEED, STEP = 0x1234_5678_9ABC, 41
Z_GUARD, DX_GUARD, DW_GUARD = 9.0, 5.0, 7.0
WS_TAIL = 256

# largest |err| / bound seen per output kind since the last reset (the tests print it; a figure, not an assertion)
RATIOS = {"Z": 0.0, "dX f32": 0.0, "dX bf16": 0.0, "dW": 0.0}


def bf16_bits(a32: np.ndarray) -> np.ndarray:
    """uint16 bits of a32 rounded to bf16, nearest even (torch's CPU conversion)."""
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(BF).view(torch.int16).numpy().view(np.uint16)


def bf16_widen(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def selection(n: int, m: int, rng) -> np.ndarray:
    """m ascending unique rows of n, always row 0 and row n - 1 (m >= 2)."""
    if m >= n:
        return np.arange(n)
    inner = rng.choice(np.arange(1, n - 1), size=m - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], inner])).astype(np.int64)


@dataclass
class Inputs:
    n: int
    k: int
    c: int
    x32: np.ndarray        # [n, k] fp32
    xbf_bits: np.ndarray   # [n, k] uint16: x32 rounded to bf16
    xbf: np.ndarray        # ... widened back to fp32: what the oracle gets for a bf16 X
    w: np.ndarray
    b: np.ndarray
    g: np.ndarray          # [n, c]; a row-selected call gets g[rows]


def make_inputs(n: int, k: int, c: int, data_seed: int) -> Inputs:
    """X, G uniform(-1, 1), W uniform(-0.3, 0.3): no kept element has an exactly zero product sum."""
    rng = np.random.default_rng(data_seed)
    x32 = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    bits = bf16_bits(x32)
    return Inputs(n, k, c, x32, bits, bf16_widen(bits), rng.uniform(-0.3, 0.3, (k, c)).astype(np.float32),
                  rng.uniform(-0.5, 0.5, c).astype(np.float32), rng.uniform(-1, 1, (n, c)).astype(np.float32))


@dataclass
class Reference:
    mask: np.ndarray
    xd: np.ndarray         # fp64 [n, k]: kept ? x / keep : 0
    g: np.ndarray          # fp64
    z: np.ndarray
    z_mag: np.ndarray      # sum |terms| of z
    dx: np.ndarray
    dx_mag: np.ndarray

    def dw(self, sel):
        """(dW, sum |terms|) over the rows `sel` (slice or index array)."""
        xd, g = self.xd[sel], self.g[sel]
        return xd.T @ g, np.abs(xd).T @ np.abs(g)


def reference(x, w, b, g, keep, seed, step) -> Reference:
    """fp64, every row of x; the formulas of oracle.classifier.dropout_dense / dropout_dense_grad on ONE keep_mask."""
    f = np.float64
    m = oc.keep_mask(x.shape[0], x.shape[1], keep, seed, step)
    xd = np.where(m, x.astype(f) / f(keep), f(0))
    w64, g64 = w.astype(f), g.astype(f)
    z = xd @ w64
    z_mag = np.abs(xd) @ np.abs(w64)
    if b is not None:
        z = z + b.astype(f)
        z_mag = z_mag + np.abs(b.astype(f))
    dx = np.where(m, (g64 @ w64.T) / f(keep), f(0))
    return Reference(m, xd, g64, z, z_mag, dx, (np.abs(g64) @ np.abs(w64).T) / f(keep))


@dataclass
class Result:
    variant: tuple
    z: np.ndarray
    dx: np.ndarray = None        # fp32 (a bf16 dX widened), or None when not requested
    dx_bits: np.ndarray = None   # uint16 bits of a bf16 dX
    dw: np.ndarray = None


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _int_view(t):
    return t.view(torch.int16 if t.dtype == BF else (torch.int32 if t.dtype == torch.float32 else torch.uint8))


@dataclass
class Driver:
    inp: Inputs
    keep: float
    seed: int
    step: int
    bias: bool = True
    x_off: int = 1     # column offsets of the slots in elements (bf16 arrays: twice that, their base must stay 4-byte aligned)
    z_off: int = 2
    dx_off: int = 1
    _xcache: dict = field(default_factory=dict)

    def __post_init__(self):
        from h2gcn_amd import _capi
        self.capi = _capi
        self.L = _capi.lib()
        self.w = torch.from_numpy(self.inp.w).to(DEV)
        self.b = torch.from_numpy(self.inp.b).to(DEV) if self.bias else None
        self.st = torch.tensor([self.step], dtype=torch.int64, device=DEV)

    def _x(self, tx, rows, n, x):
        """(device buffer, byte offset of the slot, ldx) of the X a call reads: rows [0, n) of the data, NaN around them and,
        for a row-selected call, in every row that `rows` does not name."""
        key = (tx, None if rows is None else rows.tobytes(), n, None if x is None else id(x))
        if key not in self._xcache:
            k = self.inp.k
            if tx == "f32":
                data = (self.inp.x32 if x is None else x)[:n]
                off, ld = self.x_off, (k + 2 * self.x_off + 3) | 1
                host = np.full((n + 2, ld), np.nan, dtype=np.float32)
            else:
                assert x is None
                data = self.inp.xbf_bits[:n]
                off, ld = 2 * self.x_off, k + k % 2 + 4 * self.x_off + 2
                ld += 2 if ld % 4 == 0 else 0          # rows alternate between 8-byte aligned and not
                host = np.full((n + 2, ld), 0xFFFF, dtype=np.uint16)
            if rows is None:
                host[:n, off:off + k] = data
            else:
                host[rows, off:off + k] = data[rows]
            t = torch.from_numpy(host.view(np.int16) if tx == "bf16" else host).to(DEV)
            self._xcache = {key: (t.view(BF) if tx == "bf16" else t, off * t.element_size(), ld)}   # one buffer at a time
        return self._xcache[key]

    def call(self, variant, rows=None, n=None, outputs="both", x=None) -> Result:
        """Forward + backward of one configuration, twice.  rows: ascending original rows (row-selected entry points; X keeps
        all inp.n rows); otherwise the full-matrix call on the first n rows (default: all).  outputs: "both", "dx" or "dw".
        x: an fp32 [n, k] array to use instead of inp.x32."""
        tx, td = variant
        L, inp = self.L, self.inp
        k, c = inp.k, inp.c
        n_x = inp.n if (rows is not None or n is None) else n
        m = n_x if rows is None else len(rows)
        xbuf, x_byte, ldx = self._x(tx, rows, n_x, x)
        ghost = np.full((m + 2, c + 3), np.nan, dtype=np.float32)
        ghost[:m, :c] = inp.g[:m] if rows is None else inp.g[rows]
        g = torch.from_numpy(ghost).to(DEV)
        rows_dev = None
        if rows is not None:   # entries past the list name the first NaN row after X: an over-read shows, and stays in bounds
            rows_dev = torch.from_numpy(np.concatenate([rows, np.full(64, n_x)]).astype(np.int32)).to(DEV)
        dmul = 2 if td == "bf16" else 1
        zo, do = self.z_off, dmul * self.dx_off
        zbuf = torch.empty((m + 2, c + 3 + zo), device=DEV)
        lddx = k + do + 2 + ((k + do) % 2 if td == "bf16" else 0)
        dxbuf = torch.empty((m + 2, lddx), device=DEV, dtype=BF if td == "bf16" else torch.float32)
        dwbuf = torch.empty(k * c + 8, device=DEV)
        ws_bytes = int(L.h2gcn_dropout_dense_workspace_bytes(m, k, c))
        wsbuf = torch.empty(16 + ws_bytes + WS_TAIL, dtype=torch.uint8, device=DEV)
        assert wsbuf.data_ptr() % 32 == 0
        zslot, dxslot, dwslot = zbuf[1:1 + m, zo:zo + c], dxbuf[1:1 + m, do:do + k], dwbuf[4:4 + k * c]
        want_dx, want_dw = outputs != "dw", outputs != "dx"
        base = (_ptr(xbuf, x_byte), ldx, n_x, k, _ptr(self.w), c)
        keyargs = (C.c_float(self.keep), C.c_uint64(self.seed), _ptr(self.st))
        ws_args = (_ptr(wsbuf, 16), ws_bytes, None)
        tail = () if rows is None else (_ptr(rows_dev), m)
        fwd = getattr(L, f"h2gcn_dropout_dense_{'rows_' if rows is not None else ''}{tx}")
        bwd = getattr(L, f"h2gcn_dropout_dense_backward_{'rows_' if rows is not None else ''}{tx}")
        dt = () if tx == "f32" else (self.capi.DTYPE_BF16 if td == "bf16" else self.capi.DTYPE_F32,)
        assert not (tx == "f32" and td == "bf16")
        first = None
        for _ in range(2):
            zbuf.fill_(Z_GUARD)
            dxbuf.fill_(DX_GUARD)
            dwbuf.fill_(DW_GUARD)
            wsbuf.fill_(0xFF)
            self.capi.check(fwd(*base, _ptr(self.b), *keyargs, _ptr(zslot), zbuf.stride(0), *ws_args, *tail))
            torch.cuda.synchronize()
            assert bool((wsbuf[:16] == 0xFF).all()) and bool((wsbuf[16 + ws_bytes:] == 0xFF).all()), "forward wrote outside its workspace"
            wsbuf.fill_(0xFF)
            self.capi.check(bwd(*base, _ptr(g), g.stride(0), *keyargs, *dt, _ptr(dxslot) if want_dx else None, dxbuf.stride(0),
                                _ptr(dwslot) if want_dw else None, *ws_args, *tail))
            torch.cuda.synchronize()
            assert bool((wsbuf[:16] == 0xFF).all()) and bool((wsbuf[16 + ws_bytes:] == 0xFF).all()), "backward wrote outside its workspace"
            # guards: everything outside the slots (and a slot that was not requested) still holds its sentinel
            for buf, slot, guard, written in ((zbuf, zslot, Z_GUARD, True), (dxbuf, dxslot, DX_GUARD, want_dx), (dwbuf, dwslot, DW_GUARD, want_dw)):
                chk = buf.clone()
                if written:
                    (chk[1:1 + m, zo:zo + c] if buf is zbuf else chk[1:1 + m, do:do + k] if buf is dxbuf else chk[4:4 + k * c]).fill_(guard)
                assert bool((chk == guard).all()), f"sentinel overwritten ({'Z' if buf is zbuf else 'dX' if buf is dxbuf else 'dW'})"
            now = [_int_view(t).clone() for t in (zbuf, dxbuf, dwbuf)]
            if first is None:
                first = now
            else:
                assert all(torch.equal(a, b) for a, b in zip(first, now)), "two identical calls, different bits"
        res = Result(variant, zslot.cpu().numpy())
        if want_dx:
            if td == "bf16":
                res.dx_bits = dxslot.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
                res.dx = bf16_widen(res.dx_bits)
            else:
                res.dx = dxslot.cpu().numpy()
        if want_dw:
            res.dw = dwslot.cpu().numpy().reshape(k, c)
        return res


def _ratio(kind, err, bound):
    r = float((err / bound).max())
    RATIOS[kind] = max(RATIOS[kind], r)
    return r


def check(res: Result, ref: Reference, sel, what):
    """One call against the fp64 restatement; sel: the original row behind each output row (slice or index array)."""
    b = TOL * np.maximum(ref.z_mag[sel], 1.0)
    err = np.abs(res.z - ref.z[sel])
    r = _ratio("Z", err, b)
    assert (err <= b).all(), (what, "Z", r)
    if res.dx is not None:
        want = ref.dx[sel]
        b = TOL * np.maximum(ref.dx_mag[sel], 1.0)
        kind = "dX f32"
        if res.dx_bits is not None:
            b = b + 2.0 ** -8 * (np.abs(want) + b)
            kind = "dX bf16"
        err = np.abs(res.dx - want)
        r = _ratio(kind, err, b)
        assert (err <= b).all(), (what, kind, r)
        assert np.array_equal(res.dx == 0, ~ref.mask[sel] | (want == 0)), (what, "zero pattern of dX")
    if res.dw is not None:
        want, mag = ref.dw(sel)
        b = TOL * np.maximum(mag, 1.0)
        err = np.abs(res.dw - want)
        r = _ratio("dW", err, b)
        assert (err <= b).all(), (what, "dW", r)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))


def run_shape(inp: Inputs, keep, seed, step, *, n=None, selections=(), variants=VARIANTS, bias=True, partial_outputs=True,
              offsets=(1, 2, 1), tag=""):
    """Everything the sweep asserts at one shape.  Full-matrix calls on the first n rows of inp (default: all), row-selected
    calls on each list of `selections` (rows of all inp.n; the unselected ones are NaN on the device).  Returns the Results of
    the full calls by variant."""
    n = inp.n if n is None else n
    drv = Driver(inp, keep, seed, step, bias, *offsets)
    b = inp.b if bias else None
    refs = {}

    def ref_of(tx):
        if tx not in refs:
            refs.clear()                                     # one at a time: they are the large arrays
            refs[tx] = reference(inp.x32 if tx == "f32" else inp.xbf, inp.w, b, inp.g, keep, seed, step)
        return refs[tx]

    full = {}
    for variant in sorted(variants, key=lambda v: (v[0] != "bf16", v[1] != "f32")):   # (bf16, f32), (bf16, bf16), (f32, f32): each reference is built once
        tx, td = variant
        what = (tag, inp.n, inp.k, inp.c, keep, hex(seed), step, variant)
        ref = ref_of(tx)
        res = full[variant] = drv.call(variant, n=n)
        check(res, ref, slice(0, n), what + ("full",))
        if tx == "bf16":
            # from the widening on the kernels ARE the fp32 ones: Z, dW (and an fp32 dX) have the bits of the fp32 call on X.float()
            up = drv.call(("f32", "f32"), n=n, x=inp.xbf)
            assert same_bits(res.z, up.z) and same_bits(res.dw, up.dw), what + ("bf16 X vs fp32 call on the upcast X",)
            wide = res if td == "f32" else (full.get(("bf16", "f32")) or drv.call(("bf16", "f32"), n=n, outputs="dx"))
            assert same_bits(wide.dx, up.dx), what + ("fp32 dX of a bf16 X vs fp32 call",)
            if td == "bf16":                                 # the bits of round-to-nearest-even of the fp32-dX launch
                assert np.array_equal(res.dx_bits, bf16_bits(wide.dx)), what + ("bf16 dX is not RNE(fp32 dX)",)
        if partial_outputs:
            only_dx, only_dw = drv.call(variant, n=n, outputs="dx"), drv.call(variant, n=n, outputs="dw")
            assert same_bits(only_dx.z, res.z) and same_bits(only_dw.z, res.z), what
            assert same_bits(only_dx.dx, res.dx) and only_dx.dw is None, what + ("dX alone",)
            assert same_bits(only_dw.dw, res.dw) and only_dw.dx is None, what + ("dW alone",)
        for rows in selections:
            rres = drv.call(variant, rows=rows)
            check(rres, ref, rows, what + ("rows", len(rows)))
            inside = rows < n                                # rows the full call computed as well
            assert same_bits(rres.z[inside], res.z[rows[inside]]), what + ("Z_rows != Z_full[rows]",)
            assert same_bits(rres.dx[inside], res.dx[rows[inside]]), what + ("dX_rows != dX_full[rows]",)
            if partial_outputs:
                only_dx, only_dw = drv.call(variant, rows=rows, outputs="dx"), drv.call(variant, rows=rows, outputs="dw")
                assert same_bits(only_dx.dx, rres.dx) and same_bits(only_dw.dw, rres.dw), what + ("rows: dX / dW alone",)
    return full
