"""GPU suite: boundary sweep of the fused dropout + output-Dense kernels (csrc/classifier_kernels.hip.h, all eight entry points)
against the fp64 restatement (oracle/classifier.py), through tests/classifier_driver.py -- NaN around every input, sentinels
around every output, a 0xFF workspace, every call made twice.

At every shape: the three element-type variants (X / dX = fp32 / fp32, bf16 / fp32, bf16 / bf16), the full-matrix call, dX alone
and dW alone, and from 5 rows on the row-selected call on ~n/3 rows (always row 0 and row n - 1) and on the identity selection.
Every result is compared with the restatement element by element (fp32: 2e-6 * max(sum |terms|, 1); a bf16 dX: one more
rounding to 8 bits), the zero pattern of dX is exactly the dropped elements, and the contracts between launches hold bit for
bit (rows of the full call, fp32 call on the upcast X, RNE of the fp32 dX, partial outputs).  See classifier_driver.run_shape.

Shapes: the smallest that reach each edge of the tiling and of the dispatch -- see the parameter lists."""
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import classifier_driver as cd

pytestmark = pytest.mark.gpu

FAMILIES = ["matrix-core kernels", "small-operand kernels where they apply"]


def _set_family(name):
    from h2gcn_amd import _capi
    return _capi.lib().h2gcn_dropout_dense_small_rows(0 if name.startswith("matrix") else 12288)


@pytest.fixture(autouse=True, params=FAMILIES)
def _kernel_family(request):
    """Every test runs with the small-operand kernels switched off (h2gcn_dropout_dense_small_rows(0)) and with the shipped
    rule (<= 12288 rows, <= 16 classes, K <= 512: the plain kernels), which the row-selected calls apply to the rows of X.  (A test
    whose sizes are on the matrix-core kernels under either rule, or that draws the family itself, names ONE value.)"""
    from h2gcn_amd import _capi
    old = _set_family(request.param)
    yield request.param
    _capi.lib().h2gcn_dropout_dense_small_rows(old)


def _shape(n, k, c, keep=0.5, seed=cd.SEED, step=cd.STEP, tag=""):
    """Everything at one shape; returns the full calls' results."""
    inp = cd.make_inputs(n, k, c, data_seed=n * 7 + k * 131 + c)
    rng = np.random.default_rng(n + k + c)
    sels = [cd.selection(n, max(2, n // 3), rng), np.arange(n)] if n >= 5 else []
    cd.RATIOS.update(dict.fromkeys(cd.RATIOS, 0.0))
    full = cd.run_shape(inp, keep, seed, step, selections=sels, tag=tag)
    print("max |err| / bound:", ", ".join(f"{kind} {r:.3f}" for kind, r in cd.RATIOS.items()))
    return full


# K: 1-3 a partial mask group only; 63-65 one W chunk / two; 127-129 and 255-257 dW's row_split 4 -> 2 -> 1; 511-513 the small
# kernels' limit, their second column group per lane, dW's grid.y 1 -> 2; 1024 / 1025 grid.y 2 -> 3; 1792 the documented maximum.
# n = 131: one full row group plus 3 rows
@pytest.mark.parametrize("k", [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025, 1792])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_k_edges(k, keep):
    _shape(131, k, 5, keep)


# C: 16 the last class count of the small kernels (lane 15 owns a class) and of one class tile; 32 / 33, 48 / 49 the tile edges.
# K = 68: two W chunks, the second partial
@pytest.mark.parametrize("c", [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_c_edges(c, keep):
    _shape(131, 68, c, keep)


# rows: the 4-row reduction step of dW, the 16-row tiles, a wave's 32 rows, the 64 rows of a dW workgroup, the 128 of a group
@pytest.mark.parametrize("n", [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_row_edges(n, keep):
    _shape(n, 68, 16, keep)


# dW with row_split 4 (K = 100) and 2 (K = 200) over 16 workgroups of 64 rows, the last one full / ragged
@pytest.mark.parametrize("n,k", [(1000, 100), (1003, 100), (1000, 200), (1003, 200)])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_dw_row_split_over_several_workgroups(n, k, keep):
    _shape(n, k, 7, keep)


# the last row count on the small kernels under the shipped rule and the first on the matrix-core ones
@pytest.mark.parametrize("n", [12288, 12289])
@pytest.mark.parametrize("k,c", [(512, 16), (8, 1)])
def test_small_matrix_switch(n, k, c):
    _shape(n, k, c, 0.5)


# thresholds of both field widths away from the middle: 8-bit fields 1, 64, 192, 255; 16-bit fields 65470, 65534
@pytest.mark.parametrize("n,k,c", [(300, 130, 17), (131, 448, 7)])
@pytest.mark.parametrize("keep", cd.KEEPS)
def test_keep_values(n, k, c, keep):
    _shape(n, k, c, keep)


def _dropped(full):
    return full[("f32", "f32")].dx == 0


@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_keys(keep):
    """Both words of step and of seed reach the mask: every key against the restatement, and a change of the HIGH word alone
    changes the mask the device drew (on the CPU restatement about half the bits differ)."""
    n, k, c = 131, 68, 16
    by_step = {step: _dropped(_shape(n, k, c, keep, step=step)) for step in cd.STEPS}
    by_seed = {seed: _dropped(_shape(n, k, c, keep, seed=seed)) for seed in cd.SEEDS}
    assert not np.array_equal(by_step[41], by_step[2 ** 32 + 41])               # same low word
    assert not np.array_equal(by_seed[0], by_seed[0x1234 << 32])                # same low word
    assert len({m.tobytes() for m in list(by_step.values()) + list(by_seed.values())}) == len(cd.STEPS) + len(cd.SEEDS)


def second_round_rows():
    """The forward and dX kernels are persistent: grid = min(row groups, CUs * resident workgroups per CU), a workgroup walks the
    groups blockIdx.x, blockIdx.x + gridDim.x, ...; a group is 128 rows.  A workgroup is 4 waves and a SIMD holds at most 8, so
    at most 8 workgroups per CU are resident whatever the occupancy query returns: with G = CUs * 8, any n with more than G row
    groups sends some workgroups into a second group.  n = (G + 3) * 128 + 1 has G + 4 groups -- at least four workgroups take a
    second one -- and the last group holds ONE row (262 529 rows on 256 CUs)."""
    g = torch.cuda.get_device_properties(0).multi_processor_count * 8
    return (g + 3) * 128 + 1


# (4, 1): one chunk, one class tile -- the worst case for the barrier between groups; (68, 47): two chunks, three class tiles;
# (130, 64): three chunks (the double buffer comes back to buffer 0 inside a group), four class tiles
@pytest.mark.parametrize("_kernel_family", FAMILIES[:1], indirect=True)
@pytest.mark.parametrize("xtype", ["f32", "bf16"])
@pytest.mark.parametrize("keep", [0.5, 0.9])
@pytest.mark.parametrize("k,c", [(4, 1), (68, 47), (130, 64)])
def test_second_persistent_round(k, c, keep, xtype):
    """A row count at which workgroups of the forward and dX kernels reuse their LDS double buffer for a second row group (see
    second_round_rows), every element against the restatement.  The row-selected call picks its n rows out of n + 1000."""
    n = second_round_rows()
    inp = cd.make_inputs(n + 1000, k, c, data_seed=k * 131 + c)
    rng = np.random.default_rng(k + c)
    drop = rng.choice(np.arange(1, n + 999), size=1000, replace=False)
    rows = np.setdiff1d(np.arange(n + 1000), drop)                 # n rows, row 0 and the last row among them
    assert len(rows) == n and rows[0] == 0 and rows[-1] == n + 999
    variants = [("f32", "f32")] if xtype == "f32" else [("bf16", "bf16")]
    cd.RATIOS.update(dict.fromkeys(cd.RATIOS, 0.0))
    cd.run_shape(inp, keep, cd.SEED, cd.STEP, n=n, selections=[rows], variants=variants, partial_outputs=False, tag="second round")
    print(f"n = {n}; max |err| / bound:", ", ".join(f"{kind} {r:.3f}" for kind, r in cd.RATIOS.items()))


@pytest.mark.parametrize("_kernel_family", ["family drawn per example"], indirect=True)
@settings(max_examples=int(os.environ.get("H2GCN_FUZZ_EXAMPLES", "200")), deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
@given(n=st.integers(1, 700), k=st.integers(1, 1100), c=st.integers(1, 64), keep=st.sampled_from(cd.KEEPS + (0.5, 0.9, 1.0)),
       step=st.integers(0, 2 ** 63 - 1), seed=st.integers(0, 2 ** 64 - 1), variant=st.sampled_from(cd.VARIANTS),
       sel_seed=st.one_of(st.none(), st.integers(0, 2 ** 31 - 1)), sel_frac=st.floats(0.0, 1.0), partial=st.booleans(),
       bias=st.booleans(), offsets=st.tuples(st.integers(0, 3), st.integers(0, 3), st.integers(0, 3)),
       family=st.sampled_from(FAMILIES), data_seed=st.integers(0, 2 ** 31 - 1))
def test_random_shapes_keys_and_layouts(n, k, c, keep, step, seed, variant, sel_seed, sel_frac, partial, bias, offsets, family,
                                        data_seed):
    """Property-based sweep: shape, keep value, both 64-bit key words, element types, full or a drawn row selection, the
    requested outputs, bias or none, the column offsets of the X / Z / dX slots and the kernel family, all drawn; the checks of
    run_shape.  200 examples by default (about two seconds) (H2GCN_FUZZ_EXAMPLES sets another count), the same ones on every run (derandomize)."""
    from h2gcn_amd import _capi
    inp = cd.make_inputs(n, k, c, data_seed)
    sels = []
    if sel_seed is not None:
        rng = np.random.default_rng(sel_seed)
        sels = [np.sort(rng.choice(n, size=max(1, int(round(sel_frac * n))), replace=False)).astype(np.int64)]
    old = _set_family(family)
    try:
        cd.run_shape(inp, keep, seed, step, selections=sels, variants=[variant], bias=bias, partial_outputs=partial, offsets=offsets,
                     tag="drawn")
    finally:
        _capi.lib().h2gcn_dropout_dense_small_rows(old)
