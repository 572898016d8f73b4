"""CPU suite: the two round-3 restatements in oracle/ that pin BITS of the HIP path -- the canonical summation tree
(oracle_spmm_tree_f32) and the counter-based dropout mask of the classifier kernels (oracle/classifier.py).  They are
checked here against independent formulations, so that the GPU suite's bit-exact comparisons rest on something."""
import numpy as np
import scipy.sparse as sp

from oracle import classifier as oc
from oracle import gcn_layer as og


def _rand_hops(n, seed, dens=(0.03, 0.2)):
    rng = np.random.default_rng(seed)
    hops = []
    for k, d in enumerate(dens):
        m = sp.random(n, n, d, format="csr", random_state=seed + k, dtype=np.float32)
        m.data = rng.uniform(-1, 1, m.nnz).astype(np.float32)
        m.sort_indices()
        hops.append(m)
    return hops


def test_tree_restatement_is_a_regrouping_of_the_reference_sum():
    """Same terms as the reference's sequential loop, only grouped differently: on integer-valued operands (every partial
    sum exact in fp32) the tree, the sequential C port and scipy agree EXACTLY -- short rows, rows cut into 64-neighbour
    chunks over four "waves", forward and adjoint; on real-valued operands both are within fp32 round-off of fp64."""
    n, d = 400, 9
    rng = np.random.default_rng(1)
    hops = _rand_hops(n, 3)
    for h in hops:
        h.data = rng.integers(-3, 4, h.nnz).astype(np.float32)
    hops[1] = sp.csr_matrix(sp.vstack([hops[1][:5], sp.csr_matrix(np.ones((1, n), dtype=np.float32)), hops[1][6:]]))   # a 400-nnz row
    x = rng.integers(-4, 5, (n, d)).astype(np.float32)
    w = rng.integers(-2, 3, (n, 2, d)).astype(np.float32)
    want = og.gcn_layer_c(hops, x)
    want_t = og.gcn_layer_grad_c(hops, w, n)
    for thr in (8, 64, 256, 100000):
        assert np.array_equal(og.gcn_layer_tree(hops, x, long_threshold=thr), want), thr
        assert np.array_equal(og.gcn_layer_grad_tree(hops, w, n, long_threshold=thr), want_t), thr
    # real-valued: round-off only
    hops = _rand_hops(n, 7)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    exact = og.gcn_layer_f64acc(hops, x)
    mag = og.gcn_layer_f64acc([abs(h) for h in hops], np.abs(x))
    for thr in (8, 256):
        t = og.gcn_layer_tree(hops, x, long_threshold=thr)
        assert (np.abs(t - exact) <= 2e-6 * np.maximum(mag, 1.0)).all()
    assert not np.array_equal(og.gcn_layer_tree(hops, x, 8), og.gcn_layer_tree(hops, x, 256))   # the threshold is part of the tree


def test_tree_of_one_row_by_hand():
    """P[j mod 4] accumulation and (P0 + P1) + (P2 + P3), spelled out with numpy float32 FMAs for one 7-nonzero row."""
    a = np.array([0.1, -0.7, 0.3, 0.9, -0.2, 0.5, 0.25], dtype=np.float32)
    xcol = np.array([1.5, -2.25, 0.125, 3.0, -1.0, 0.75, 2.5], dtype=np.float32)
    m = sp.csr_matrix((a, np.arange(7), [0, 7]), shape=(1, 7))
    got = og.gcn_layer_tree([m], xcol.reshape(7, 1))[0, 0, 0]

    def fma(p, q, r):   # one rounding: exact in float64 for fp32 inputs of this size, then rounded once
        return np.float32(np.float64(p) * np.float64(q) + np.float64(r))
    P = [np.float32(0)] * 4
    for j in range(7):
        P[j % 4] = fma(a[j], xcol[j], P[j % 4])
    assert got == np.float32(np.float32(P[0] + P[1]) + np.float32(P[2] + P[3]))


def test_sddmm_order_restatement():
    """oracle_sddmm_order_f32 restates the ONE order include/h2gcn_hip.h documents for h2gcn_sddmm_hops_*: fma quad chains from
    g0 * x0, columns >= d as +0, the xor butterfly over 16 quads, block totals added in ascending order to +0."""
    rng = np.random.default_rng(5)
    n_rows, n_cols = 9, 23
    m = sp.random(n_rows, n_cols, 0.4, format="csr", random_state=5, dtype=np.float32)
    m.sort_indices()
    rows = np.repeat(np.arange(n_rows), np.diff(m.indptr))
    # (a) integer-valued operands: every partial sum is exact in fp32 (|sum| <= 516 * 16 < 2^24), so every order gives the integer dot product
    for d in (1, 3, 4, 5, 63, 64, 65, 130, 516):
        g = rng.integers(-4, 5, (n_rows, 2, d)).astype(np.float32)
        x = rng.integers(-4, 5, (n_cols, d)).astype(np.float32)
        got = og.sddmm_order([m, m], g, x)
        for k in range(2):
            want = (g[rows, k, :].astype(np.int64) * x[m.indices].astype(np.int64)).sum(-1)
            assert got[k].dtype == np.float32 and np.array_equal(got[k].astype(np.int64), want), (d, k)
    # (b) by hand, d = 8, x = 1 everywhere, g = [1, 0, 0, 0, 2^-24, 2^-24, 0, 0] (every product exact).
    #   documented order: quad 0 = fma chain over columns 0..3 = 1;  quad 1 = 2^-24 + 2^-24 = 2^-23 (exact);  quads 2..15 = +0;
    #     butterfly distance 1: v[0] = quad 0 + quad 1 = 1 + 2^-23, representable (1 + one ulp of 1), bits 0x3F800001; the
    #     distances 2, 4, 8 add +0, and the element is +0 + B_0 = 1 + 2^-23.
    #   left to right: 1 + 2^-24 is a tie between 1 and 1 + 2^-23 and rounds to the even 1 -- twice; the sum is 1, bits 0x3F800000.
    one = sp.csr_matrix((np.ones(1, np.float32), [0], [0, 1]), shape=(1, 1))
    g = np.array([1, 0, 0, 0, 2.0 ** -24, 2.0 ** -24, 0, 0], np.float32).reshape(1, 1, 8)
    x = np.ones((1, 8), np.float32)
    left = np.float32(0)
    for c in range(8):
        left = np.float32(left + np.float32(g[0, 0, c] * x[0, c]))
    got = og.sddmm_order([one], g, x)[0]
    assert left.view(np.uint32) == 0x3F800000 and got.view(np.uint32)[0] == 0x3F800001
    #   the chain is FUSED: d = 2, g = [-1, 1 + 2^-12], x = [1, 1 + 2^-12]: t = -1, then fma((1 + 2^-12)^2, t) = 2^-11 + 2^-24
    #   exactly, where a rounded product (1 + 2^-11 + 2^-24 -> 1 + 2^-11, a tie to even) would leave 2^-11.
    a = np.float32(1 + 2.0 ** -12)
    got = og.sddmm_order([one], np.array([-1, a], np.float32).reshape(1, 1, 2), np.array([[1, a]], np.float32))[0]
    assert float(got[0]) == 2.0 ** -11 + 2.0 ** -24
    # (c) real-valued: within the bound of ANY order of a d-term fp32 dot product
    u = 2.0 ** -24
    for d in (5, 64, 130, 516):
        g = rng.uniform(-1, 1, (n_rows, 1, d)).astype(np.float32)
        x = rng.uniform(-1, 1, (n_cols, d)).astype(np.float32)
        prod = g[rows, 0, :].astype(np.float64) * x[m.indices].astype(np.float64)
        bound = d * u / (1 - d * u) * np.abs(prod).sum(-1) + d * 2.0 ** -149
        assert (np.abs(og.sddmm_order([m], g, x)[0] - prod.sum(-1)) <= bound).all(), d


def test_mask_generator_statistics_and_structure():
    for keep in (0.5, 0.9, 0.25):
        m = oc.keep_mask(4000, 448, keep, seed=0xDEADBEEF12345, step=3)
        assert abs(m.mean() - keep) < 2e-3
        assert np.abs(m.mean(0) - keep).max() < 0.04 and np.abs(m.mean(1) - keep).max() < 0.12   # every column / row
        assert abs((m[:, :-1] & m[:, 1:]).mean() - keep * keep) < 3e-3                           # neighbours independent
        assert abs((m[:-1] & m[1:]).mean() - keep * keep) < 3e-3
    a = oc.keep_mask(100, 30, 0.5, 11, 5)
    assert np.array_equal(a, oc.keep_mask(100, 30, 0.5, 11, 5))                  # a pure function of (seed, step, index)
    assert not np.array_equal(a, oc.keep_mask(100, 30, 0.5, 11, 6)) and not np.array_equal(a, oc.keep_mask(100, 30, 0.5, 12, 5))
    assert np.array_equal(oc.keep_mask(40, 30, 0.5, 11, 5, row0=60), a[60:])     # rows are addressed globally
    for keep in (0.5, 0.9):                                                      # 8-bit / 16-bit fields
        s5, s6 = oc.keep_mask(3000, 448, keep, 77, 5), oc.keep_mask(3000, 448, keep, 77, 6)
        assert abs((s5 & s6).mean() - keep * keep) < 3e-3                        # consecutive steps independent
        far = oc.keep_mask(3000, 448, keep, 77, 5, row0=2 ** 33)                 # group ids beyond 32 bits
        assert abs(far.mean() - keep) < 2e-3 and abs((far & s5).mean() - keep * keep) < 3e-3
    assert oc.keep_mask(5, 7, 1.0, 1, 1).all()
    # widths that are not multiples of 4: the row's last group is partial, columns beyond it do not exist
    assert oc.keep_mask(50, 7, 0.5, 1, 1).shape == (50, 7)


def test_dropout_dense_gradients_by_finite_differences():
    rng = np.random.default_rng(0)
    n, k, c = 30, 13, 5
    x, w, b = rng.standard_normal((n, k)), rng.standard_normal((k, c)), rng.standard_normal(c)
    g = rng.standard_normal((n, c))
    seed, step, keep = 99, 4, 0.7
    f = lambda xx, ww: float((oc.dropout_dense(xx, ww, b, keep, seed, step) * g).sum())
    dx, dw, db = oc.dropout_dense_grad(x, w, g, keep, seed, step)
    eps = 1e-6
    for (i, j) in ((0, 0), (7, 12), (29, 5)):
        xp = x.copy(); xp[i, j] += eps
        assert abs((f(xp, w) - f(x, w)) / eps - dx[i, j]) < 1e-4
    for (i, j) in ((0, 0), (12, 4), (5, 2)):
        wp = w.copy(); wp[i, j] += eps
        assert abs((f(x, wp) - f(x, w)) / eps - dw[i, j]) < 1e-4
    assert np.allclose(db, g.sum(0))
    m = oc.keep_mask(n, k, keep, seed, step)
    assert np.array_equal(dx == 0, ~m)


def test_keras_adam_restatement_first_step_by_hand_and_cpu_optimizer_follows_it():
    """Keras / TensorFlow Adam (reference `H2GCN.py:62-63, 73`): epsilon joins the UNCORRECTED sqrt(v).  First step by hand:
    m = 0.1 g, v = 0.001 g^2, alpha = lr sqrt(0.001) / 0.1, update = alpha m / (sqrt(v) + eps) = lr g / (|g| + eps / sqrt(0.001))
    -- so a gradient of 1e-6 moves a weight by lr * 1e-6 / (1e-6 + 3.16e-6) = 0.24 lr, where torch's Adam (epsilon on the
    corrected sqrt(v)) would move it by lr * 1e-6 / (1e-6 + 1e-7) = 0.91 lr."""
    import torch
    from oracle import keras_adam as ok
    from h2gcn_amd.optim import KerasAdam

    g = np.array([1.0, -2.0, 1e-6, 0.0], np.float32)
    p, m, v = ok.keras_adam_step(np.zeros(4, np.float32), g, np.zeros(4), np.zeros(4), 1, lr=0.01)
    want = -0.01 * g.astype(np.float64) / (np.abs(g.astype(np.float64)) + 1e-7 / np.sqrt(0.001))
    assert np.allclose(p, want, rtol=2e-4, atol=1e-9) and abs(p[2] / -0.01 - 0.2403) < 2e-3 and p[3] == 0
    assert np.allclose(m, 0.1 * g, rtol=1e-6) and np.allclose(v, 0.001 * g * g, rtol=3e-5)   # fp32(1) - fp32(0.999) = 0.99998713e-3
    # the CPU branch of the optimizer is the same arithmetic, step after step
    rng = np.random.default_rng(0)
    w0 = rng.normal(size=(5, 3)).astype(np.float32)
    w = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = KerasAdam([w], lr=0.01)
    p, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    for t in range(1, 8):
        gt = (rng.normal(size=w0.shape) * (10.0 ** rng.integers(-6, 1))).astype(np.float32)
        w.grad = torch.from_numpy(gt.copy())
        opt.step()
        p, m, v = ok.keras_adam_step(p, gt, m, v, t, lr=0.01)
        assert np.allclose(w.detach().numpy(), p, rtol=2e-6, atol=3e-7), t      # pow / sqrt of torch vs numpy: last-bit differences
    assert "step_dev" in opt.state_dict()["param_groups"][0]


def test_keras_rmsprop_by_hand():
    """TensorFlow's ApplyRMSProp puts epsilon inside the square root: first step ms = 0.1 g^2, update = lr g / sqrt(0.1 g^2 + eps)."""
    import torch
    from h2gcn_amd.optim import KerasRMSprop
    g = np.array([1.0, -0.5, 1e-5, 0.0])
    w = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    w.grad = torch.from_numpy(g.copy())
    KerasRMSprop([w], lr=0.01).step()
    assert np.allclose(w.detach().numpy(), -0.01 * g / np.sqrt(0.1 * g * g + 1e-7), rtol=1e-12)
    assert abs(w[2].item() / -0.01 - 1e-5 / np.sqrt(1e-11 + 1e-7)) < 1e-9        # 0.0316: the epsilon floor, not 1 / sqrt(0.1) = 3.16


def test_threaded_tree_oracle_has_the_bits_of_the_serial_one_and_the_checksum_helpers_count_right():
    """oracle_spmm_tree_f32_mt (rows spread over OpenMP threads, what the full-size GPU checks run) == oracle_spmm_tree_f32 bit
    for bit, forward and adjoint, long segments included; the whole-array helpers agree with numpy."""
    import scipy.sparse as sp
    from oracle import fullsize as fs
    from oracle import gcn_layer as og

    rng = np.random.default_rng(11)
    n, d = 900, 40
    hops = []
    for k, dens in enumerate((0.01, 0.08)):
        m = sp.random(n, n, dens, format="lil", random_state=k, dtype=np.float32)
        m[5, :700] = 1.0                                   # a long segment (>= 256): the 4-"wave" branch of the tree
        m = sp.csr_matrix(m)
        m.data[:] = rng.uniform(-1, 1, len(m.data)).astype(np.float32)
        m.sort_indices()
        hops.append(m)
    x = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    parts = [og._csr_parts(m) for m in hops]
    y0, y1 = og.gcn_layer_tree(hops, x), fs.gcn_layer_tree_mt(parts, x)
    assert np.array_equal(y0, y1)
    assert np.array_equal(og.gcn_layer_c(hops, x), fs.gcn_layer_seq_mt(parts, x))
    dy = rng.uniform(-1, 1, (n, 2, d)).astype(np.float32)
    t_parts = []
    for m in hops:
        t = m.T.tocsr()
        t.sort_indices()
        t_parts.append(og._csr_parts(t))
    assert np.array_equal(og.gcn_layer_grad_tree(hops, dy, n), fs.gcn_layer_grad_tree_mt(t_parts, dy))
    assert fs.bits_checksum(y0) == int(y0.view(np.int32).astype(np.int64).sum())
    assert fs.count_bit_mismatches(y0, y1) == (0, -1)
    y2 = y1.copy()
    y2.reshape(-1)[[77, 5000]] += np.float32(1e-3)
    y2.reshape(-1)[9] = -y2.reshape(-1)[9] if y2.reshape(-1)[9] != 0 else np.float32(-0.0)
    assert fs.count_bit_mismatches(y0, y2) == (3, 9)
    assert abs(fs.max_abs_diff(y0, y2) - float(np.abs(y0.astype(np.float64) - y2).max())) < 1e-12
    y2.reshape(-1)[3] = np.nan
    assert fs.max_abs_diff(y0, y2) == float("inf")


def test_bench_checksum_constants_come_from_the_oracle():
    """bench.py's N1_CHECKSUMS (what `checksum_matches_n1` compares with) is the ORACLE's checksum of Y -- recomputed here on the
    CPU for BASELINE configs[2] (the arxiv shape: a second; the products constant is re-derived the same way by `python -m
    oracle.fullsize products`, ~30 s on 8 cores, and asserted on the GPU box in tests/test_fullsize_parity_gpu.py)."""
    import sys
    from pathlib import Path
    from oracle import fullsize as fs

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    ck, nnz = fs.oracle_checksum("arxiv", block_rows=60_000)       # three row blocks: the sum does not depend on the blocking
    assert ck == bench.N1_CHECKSUMS[("arxiv", 128)]
    assert nnz == [1203951, 1205200]


def test_kept_fraction_at_every_keep_value_and_step_of_the_sweep():
    """Kept fraction of a [300, 130] mask (N = 39 000 elements) within 5 binomial standard deviations of the field threshold
    over the field range, thr / 2^bits -- at thresholds next to both ends of both field widths and at steps whose high word is
    set (measured: at most 2.6 sigma)."""
    import classifier_driver as cd

    n, k = 300, 130
    for keep in cd.KEEPS + (0.5, 0.9):
        thr16 = int(float(np.float32(keep)) * 65536.0)
        p = (thr16 // 256) / 256 if thr16 % 256 == 0 else thr16 / 65536
        sigma = np.sqrt(p * (1 - p) / (n * k))
        for step in cd.STEPS:
            got = oc.keep_mask(n, k, keep, cd.SEED, step).mean()
            assert abs(got - p) <= 5 * sigma, (keep, step, (got - p) / sigma)


_U32 = 0xFFFFFFFF


def _scalar_keep(row, col, k, keep_prob, seed, step):
    """keep(row, col) in Python integers, written from the description in include/h2gcn_hip.h (not from oracle.classifier)."""
    def mix(h):
        h ^= h >> 16
        h = h * 0x7FEB352D & _U32
        h ^= h >> 15
        h = h * 0x846CA68B & _U32
        return h ^ h >> 16

    key0 = mix(seed & _U32 ^ mix((step & _U32) + 0x9E3779B9 & _U32))
    key1 = mix(seed >> 32 & _U32 ^ step >> 32 & _U32 ^ key0 ^ 0x85EBCA6B)
    gid = (row * ((k + 3) // 4) + col // 4) & (2 ** 64 - 1)
    lo, hi = gid & _U32, gid >> 32
    h = lo ^ (hi << 16 & _U32 | hi >> 16) ^ key0
    h ^= h >> 16
    h = h * 0x7FEB352D & _U32
    h ^= key1
    h ^= h >> 15
    h = h * 0x846CA68B & _U32
    w0 = h ^ h >> 16
    t = int(float(np.float32(keep_prob)) * 65536.0)          # T = floor(keep_prob * 65536), keep_prob an fp32
    if t % 256 == 0:
        return (w0 >> 8 * (col % 4) & 0xFF) < t // 256
    w1 = mix(w0 ^ 0x85EBCA6B)
    return (w0 & 0xFFFF, w0 >> 16, w1 & 0xFFFF, w1 >> 16)[col % 4] < t


def test_mask_generator_against_a_scalar_restatement_of_the_header():
    """oracle.classifier.keep_mask (numpy, what the GPU suites hold the device to) == the generator of include/h2gcn_hip.h
    spelled out with Python integers, element by element: both field widths, every key of the sweep's ends, widths with a
    partial last group, and rows whose group ids need more than 32 bits (which no device test can afford to reach)."""
    import classifier_driver as cd

    k = 130                                                   # 33 groups per row, the last one partial
    row0s = (0, 5, 2 ** 32 // 33 - 1, 2 ** 32 // 33 + 7, 2 ** 33 + 12345, (2 ** 48 + 9) // 33, 2 ** 57)
    cols = (0, 1, 2, 3, 4, 63, 64, 127, 128, 129)
    keys = [(cd.SEED, cd.STEP), (0, 0), (2 ** 64 - 1, 2 ** 63 - 1), (0x1234 << 32, (7 << 40) + 3), (0x9ABC, 2 ** 32 + 41)]
    n_checked = n_far = 0
    for keep in (0.5, 0.9, 1 / 256, 65534 / 65536, 0.999, 255 / 256):
        for seed, step in keys:
            for row0 in row0s:
                m = oc.keep_mask(3, k, keep, seed, step, row0=row0)
                for r in range(3):
                    for col in cols:
                        assert bool(m[r, col]) == _scalar_keep(row0 + r, col, k, keep, seed, step), (keep, seed, step, row0 + r, col)
                        n_checked += 1
                        n_far += (row0 + r) * 33 >= 2 ** 32
    assert n_checked >= 5000 and n_far >= 2000
    # the two high words matter in the scalar form as well
    a = [_scalar_keep(r, c, k, 0.5, cd.SEED, 41) for r in range(40) for c in range(k)]
    assert a != [_scalar_keep(r, c, k, 0.5, cd.SEED, 2 ** 32 + 41) for r in range(40) for c in range(k)]
    assert a != [_scalar_keep(r, c, k, 0.5, cd.SEED ^ 1 << 40, 41) for r in range(40) for c in range(k)]


def test_sweep_driver_reference_is_the_oracle():
    """tests/classifier_driver.reference (one mask, every product once, any row subset) == oracle.classifier.dropout_dense /
    dropout_dense_grad: exactly for the full matrix, and for a row subset the oracle on G scattered into a zero matrix."""
    import classifier_driver as cd

    for keep, bias in ((0.5, True), (0.9, False), (1.0, True)):
        inp = cd.make_inputs(57, 13, 5, data_seed=3)
        b = inp.b if bias else None
        ref = cd.reference(inp.x32, inp.w, b, inp.g, keep, cd.SEED, cd.STEP)
        assert np.array_equal(ref.z, oc.dropout_dense(inp.x32, inp.w, b, keep, cd.SEED, cd.STEP))
        dx, dw, _ = oc.dropout_dense_grad(inp.x32, inp.w, inp.g, keep, cd.SEED, cd.STEP)
        assert np.array_equal(ref.dx, dx) and np.array_equal(ref.dw(slice(0, 57))[0], dw)
        assert np.array_equal(ref.mask, oc.keep_mask(57, 13, keep, cd.SEED, cd.STEP))
        rows = cd.selection(57, 19, np.random.default_rng(0))
        g0 = np.zeros_like(inp.g)
        g0[rows] = inp.g[rows]
        dx0, dw0, _ = oc.dropout_dense_grad(inp.x32, inp.w, g0, keep, cd.SEED, cd.STEP)
        assert np.array_equal(ref.dx[rows], dx0[rows]) and np.allclose(ref.dw(rows)[0], dw0, rtol=0, atol=1e-13)
    # the bf16 helpers: round to nearest even, ties included, and the exact widening
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3, 1e-30], np.float32)
    assert list(cd.bf16_bits(v)[:3]) == [0x3F80, 0x3F80, 0x3F82]
    assert np.array_equal(cd.bf16_widen(cd.bf16_bits(v))[:3], np.array([1.0, 1.0, 1.0 + 2.0 ** -6], np.float32))
