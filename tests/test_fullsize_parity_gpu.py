"""GPU suite: BASELINE configs[2] (arxiv shape) and configs[3] (products shape, the headline) checked EXHAUSTIVELY -- every row of
the operands and every element of Y -- against the CPU oracle, at full size.

* operands: the host rebuilds all rows of both hop matrices and of X (oracle/spmm_oracle.c: C restatement of the synthetic
  generator, pinned against the numpy one in tests/test_synth.py); row pointers, column ids, values and features the device
  generated must be bit-equal;
* forward: the HIP result must equal ``oracle_spmm_tree_f32_mt`` BIT FOR BIT on all N x 2 x d elements (the library's documented
  summation tree), and lie within the north star's 1e-5 of ``oracle_gcn_layer_f32_mt`` -- the reference's own order (sequential fp32
  sum per row in ascending column order: TF's SparseTensorDenseMatMul, reference h2gcn/models/_layers.py:74-81) -- on all of them;
* the order-independent checksum of the ORACLE's Y is what bench.py's N1_CHECKSUMS table holds for the shape (`python -m
  oracle.fullsize` prints it, CPU only): the `checksum_matches_n1` of every bench line is a comparison with the oracle, not with
  an earlier run of the HIP path;
* adjoint: every element of dX of the SUM-mode launch on the device-built transposed operands, bit-equal to the tree oracle on a
  host-built transpose (its checksum is bench.py's N1_ADJOINT_CHECKSUMS entry); the identity <A x, w> == <x, A^T w> ties it to the
  forward that has just been pinned to the reference's order."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
ATOL = 1e-5        # BASELINE.json north_star: "layer outputs within 1e-5 of reference"


def _device_operands(shape):
    from h2gcn_amd import synth

    cfg = synth.SHAPES[shape]
    n, d = cfg["n"], cfg["d"]
    device = torch.device("cuda", 0)
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, device) for k in range(2)]
    x = synth.synth_features(d, synth.SEED_X, 0, n, device)
    return csr, x, n, d


#: the two BASELINE shapes always; H2GCN_FULLSIZE_ALL=1 adds the other benchmark shapes that have oracle checksums (the in-tile short-row
#: walk and the list-driven walks at full size: +70 s; their checksums are asserted in every run by test_spmm_gpu.py
#: ::test_baseline_shapes_properties, the element-wise run is on record in profiles/r06_fullsize_all_shapes.txt)
_SHAPES = ["arxiv", "products"] + (["lowdeg", "h2gcn_like", "products_tail"] if os.environ.get("H2GCN_FULLSIZE_ALL") == "1" else [])


@pytest.mark.parametrize("shape", _SHAPES)
def test_every_row_of_the_baseline_shape_against_the_oracle(shape):
    from h2gcn_amd import HopPlan
    from oracle import fullsize as fs

    sys.path.insert(0, str(ROOT))
    import bench

    csr, x, n, d = _device_operands(shape)
    parts, x_host, n_h, d_h = fs.host_operands(shape)
    assert (n_h, d_h) == (n, d)
    # operands: every row pointer, column id, value and feature the device built == the host's independent rebuild
    for k in range(2):
        for got, want in zip(csr[k], parts[k]):
            assert np.array_equal(got.cpu().numpy(), want), (shape, k)
    assert np.array_equal(x.cpu().numpy(), x_host)

    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n, build_transpose=True)
    y = plan.spmm(x)
    torch.cuda.synchronize()
    y_dev_checksum = int(y.view(torch.int32).to(torch.int64).sum().item())
    y_hip = y.cpu().numpy()

    # (1) bit-exact against the documented summation tree, all elements
    y_tree = fs.gcn_layer_tree_mt(parts, x_host)
    bad, first = fs.count_bit_mismatches(y_hip, y_tree)
    assert bad == 0, f"{shape}: {bad} of {y_hip.size} elements differ from the canonical tree, first at flat index {first}"
    # (2) the oracle's checksum is the constant bench.py compares every line with
    ck = fs.bits_checksum(y_tree)
    print(f"\noracle checksum of Y, {shape} d={d}: {ck}")
    assert ck == y_dev_checksum == bench.N1_CHECKSUMS[(shape, d)]
    del y_tree
    # (3) within 1e-5 of the reference's own summation order, all elements
    y_seq = fs.gcn_layer_seq_mt(parts, x_host)
    err = fs.max_abs_diff(y_hip, y_seq)
    print(f"max |HIP - reference-order oracle| over all {y_hip.size} elements of Y, {shape}: {err:.3e}")
    assert err <= ATOL
    del y_seq, y_hip

    # (4) adjoint, all elements: dX = sum_k A_k^T W[:, k, :] on the device-built transposed operands vs the tree oracle on a
    #     host-built transpose (stable counting sort: ascending row order inside every output row)
    import scipy.sparse as sp
    from h2gcn_amd import synth

    w = synth.synth_features(2 * d, 77, 0, n, x.device).view(n, 2, d)
    dx = plan.spmm_t(w)
    torch.cuda.synchronize()
    dx_hip = dx.cpu().numpy()
    w_host = fs.synth_features_c(2 * d, 77, 0, n).reshape(n, 2, d)
    t_parts = []
    for rp, ci, va in parts:
        t = sp.csr_matrix((va, ci, rp), shape=(n, n)).T.tocsr()
        t.sort_indices()
        t_parts.append((t.indptr.astype(np.int64), t.indices.astype(np.int32), t.data.astype(np.float32)))
    dx_tree = fs.gcn_layer_grad_tree_mt(t_parts, w_host)
    bad, first = fs.count_bit_mismatches(dx_hip, dx_tree)
    assert bad == 0, f"{shape} adjoint: {bad} of {dx_hip.size} elements differ from the canonical tree, first at flat index {first}"
    assert fs.bits_checksum(dx_tree) == bench.N1_ADJOINT_CHECKSUMS[(shape, d)]      # what bench.py's adjoint leg is compared with
    # ... and the identity <A x, w> == <x, A^T w> ties the adjoint to the forward that (3) has pinned to the reference order
    lhs = float((y.double() * w.double()).sum().item())
    rhs = float((x.double() * dx.double()).sum().item())
    assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs), float((y.double().abs() * w.double().abs()).sum().item()) * 1e-3)


def test_plain_bench_run_and_its_dumped_outputs(tmp_path):
    """A plain `bench.py` run (no --full) on the arxiv shape: one line with the K timed steps and the headline keys, none of the
    --full figures; `--dump-outputs` writes Y of the last timed step, for the rows bench.dump_rows names, bit-equal to the
    oracle's documented summation tree."""
    import json
    import subprocess

    from oracle import fullsize as fs

    sys.path.insert(0, str(ROOT))
    import bench

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "H2GCN_SHARE_GPU")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--shape", "arxiv", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert abs(line["value"] - sum(line["config"]["nnz_per_hop"]) / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert not {"adjoint", "secondary"} & set(line) and "checksum_matches_n1" not in line["config"], sorted(line)
    assert line["cpu_baseline"]["value"] is None and "ceilings" not in line["roofline"]
    files = sorted((tmp_path / "out").iterdir())
    assert [f.name for f in files] == ["y.npy"] and files[0].stat().st_size <= 64 << 20
    y = np.load(files[0])
    parts, x_host, n, d = fs.host_operands("arxiv")
    rows = bench.dump_rows(n, d)
    assert y.dtype == np.float32 and y.shape == (len(rows), 2, d) and 0 < len(rows) < n
    bad, first = fs.count_bit_mismatches(y, fs.gcn_layer_tree_mt(parts, x_host)[rows])
    assert bad == 0, f"{bad} of {y.size} dumped elements differ from the canonical tree, first at flat index {first}"
