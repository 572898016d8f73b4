"""GPU suite: the H2GCN model on bf16 embeddings -- the classifier kernels on a bf16 X (csrc/classifier_bf16.hip), the bf16
fused propagation and its backward (layers.fused_propagation(dtype=bfloat16)), the model / CLI switch (--embedding_dtype).

Bit contracts (torch.equal on the raw bits, no tolerance), every expected value derived from the contract:
  * classifier: Z and dW equal the _f32 entry points on X.float(); an fp32 dX too; a bf16 dX is that fp32 dX rounded to nearest even;
  * propagation: the buffer equals the chain built by hand from HopPlan.spmm on separate bf16 tensors (which tests/test_bf16_gpu.py
    pins to the oracle); the backward equals the hand-built chain of spmm_t calls with the documented order of roundings;
  * model: logits and parameter gradients equal the composition SparseDense -> hand-built chain -> classifier _f32 on the upcast buffer.
Accuracy of the embedding against an fp64 host product: the derived bound of the issue, no extra factor."""
import ctypes as C
import json

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_planetoid_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
H2GCN2_NO_DROPOUT = "M64-R-T1-G-V-T2-G-V-C1-C2-D0.0-MO"


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int16 if got.dtype == BF else torch.int32
    return torch.equal(got.detach().contiguous().view(it), want.detach().contiguous().view(it))


# ---- 4. classifier kernels ---------------------------------------------------------------------------------------------------
@pytest.fixture(params=["matrix-core kernels", "small-operand kernels where they apply"])
def kernel_family(request):
    from h2gcn_amd import _capi
    L = _capi.lib()
    old = L.h2gcn_dropout_dense_small_rows(0 if request.param.startswith("matrix") else 12288)
    yield request.param
    L.h2gcn_dropout_dense_small_rows(old)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _classifier_f32(x, w, b, g, keep, seed, st):
    from h2gcn_amd import _capi
    L = _capi.lib()
    n, k = x.shape
    c = w.shape[1]
    ws = torch.empty(int(L.h2gcn_dropout_dense_workspace_bytes(n, k, c)), dtype=torch.uint8, device=DEV)
    z, dx, dw = torch.empty((n, c), device=DEV), torch.empty((n, k), device=DEV), torch.empty((k, c), device=DEV)
    _capi.check(L.h2gcn_dropout_dense_f32(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, seed, _ptr(st), _ptr(z), z.stride(0),
                                          _ptr(ws), ws.numel(), None))
    _capi.check(L.h2gcn_dropout_dense_backward_f32(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g), g.stride(0), keep, seed, _ptr(st),
                                                   _ptr(dx), dx.stride(0), _ptr(dw), _ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    return z, dx, dw


# the shapes of test_classifier_gpu.py::test_forward_and_backward_match_the_restatement with an even K, plus one odd-K case
@pytest.mark.parametrize("n,k,c", [(1, 4, 1), (129, 448, 47), (1000, 700, 10), (513, 896, 64), (300, 130, 17), (4099, 448, 7), (37, 7, 3)])
@pytest.mark.parametrize("keep", [0.5, 1.0, 0.9])
def test_classifier_on_bf16_x_has_the_bits_of_the_f32_call_on_the_upcast_x(kernel_family, n, k, c, keep):
    from h2gcn_amd import _capi
    L = _capi.lib()
    rng = np.random.default_rng(n * 7 + k + c)
    pad = k % 2                                                   # even row strides for an odd K
    xbuf = torch.zeros((n, k + 6 + pad), device=DEV, dtype=BF)    # X is a column slot of a wider buffer
    x = xbuf[:, 2:2 + k]
    x.copy_(torch.from_numpy(rng.uniform(-1, 1, (n, k)).astype(np.float32)))
    w = torch.from_numpy(rng.uniform(-0.3, 0.3, (k, c)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.uniform(-0.5, 0.5, c).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)).to(DEV)
    seed, step = 0x1234_5678_9ABC, 41
    st = torch.tensor([step], dtype=torch.int64, device=DEV)
    z32, dx32, dw32 = _classifier_f32(x.float().contiguous(), w, b, g, keep, seed, st)   # same seed and step: the same mask

    ws = torch.empty(int(L.h2gcn_dropout_dense_workspace_bytes(n, k, c)), dtype=torch.uint8, device=DEV)
    zbuf = torch.full((n, c + 3), 9.0, device=DEV)
    _capi.check(L.h2gcn_dropout_dense_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(b), keep, seed, _ptr(st), _ptr(zbuf), zbuf.stride(0),
                                           _ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    assert bool((zbuf[:, c:] == 9.0).all())
    assert same_bits(zbuf[:, :c], z32)
    for dx_dtype, tdt in ((_capi.DTYPE_F32, torch.float32), (_capi.DTYPE_BF16, BF)):
        dxbuf = torch.full((n, k + 2 + pad), 5.0, device=DEV, dtype=tdt)
        dw = torch.empty((k, c), device=DEV)
        _capi.check(L.h2gcn_dropout_dense_backward_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g), g.stride(0), keep, seed, _ptr(st),
                                                        dx_dtype, _ptr(dxbuf), dxbuf.stride(0), _ptr(dw), _ptr(ws), ws.numel(), None))
        torch.cuda.synchronize()
        assert bool((dxbuf[:, k:] == 5.0).all()), "guard columns of the strided dX were written"
        assert same_bits(dw, dw32), tdt
        assert same_bits(dxbuf[:, :k], dx32 if tdt == torch.float32 else dx32.to(BF)), tdt
    assert bool((xbuf[:, :2] == 0).all()) and bool((xbuf[:, 2 + k:] == 0).all())
    # dW alone (dX NULL) and dX alone (dW NULL)
    dw = torch.empty((k, c), device=DEV)
    _capi.check(L.h2gcn_dropout_dense_backward_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g), g.stride(0), keep, seed, _ptr(st),
                                                    _capi.DTYPE_BF16, None, k + pad, _ptr(dw), _ptr(ws), ws.numel(), None))
    dx = torch.empty((n, k + pad), device=DEV, dtype=BF)
    _capi.check(L.h2gcn_dropout_dense_backward_bf16(_ptr(x), x.stride(0), n, k, _ptr(w), c, _ptr(g), g.stride(0), keep, seed, _ptr(st),
                                                    _capi.DTYPE_BF16, _ptr(dx), dx.stride(0), None, _ptr(ws), ws.numel(), None))
    torch.cuda.synchronize()
    assert same_bits(dw, dw32) and same_bits(dx[:, :k], dx32.to(BF))


def test_dropout_dense_module_on_a_bf16_input(kernel_family):
    """DropoutDense: a bf16 input takes the bf16 entry points (fp32 logits equal to the fp32 layer on the upcast input, bf16 input
    gradient equal to the rounded fp32 one, same kernel / bias gradients); wide layers upcast onto the stock path."""
    from h2gcn_amd.layers import DropoutDense

    torch.manual_seed(3)
    n, k, c = 2000, 448, 7
    layer = DropoutDense(k, c, use_bias=True, drop_prob=0.5).to(DEV).train()
    xb = torch.randn((n, k), device=DEV).to(BF)
    wgt = torch.randn((n, c), device=DEV)
    got = {}
    for name, x in (("bf16", xb.clone().requires_grad_(True)), ("f32", xb.float().requires_grad_(True))):
        layer._step.zero_()
        layer.zero_grad(set_to_none=True)
        z = layer(x)
        assert z.dtype == torch.float32
        (z * wgt).sum().backward()
        got[name] = (z.detach(), x.grad, layer.kernel.grad.clone(), layer.bias.grad.clone())
    assert got["bf16"][1].dtype == BF and got["f32"][1].dtype == torch.float32
    assert same_bits(got["bf16"][0], got["f32"][0])
    assert same_bits(got["bf16"][1], got["f32"][1].to(BF))
    assert same_bits(got["bf16"][2], got["f32"][2]) and same_bits(got["bf16"][3], got["f32"][3])
    z2 = layer(xb)
    assert not torch.equal(z2, got["bf16"][0])                     # next step, next mask
    wide = DropoutDense(16, 100, use_bias=False, drop_prob=0.5).to(DEV).eval()
    assert same_bits(wide(xb[:, :16]), xb[:, :16].float() @ wide.kernel)


# ---- 5. propagation ----------------------------------------------------------------------------------------------------------
def _nonsymmetric_hops(rng, n):
    """two square, non-symmetric hop matrices with signed values: Poisson degrees, 10 % empty rows, a few long rows"""
    hops = []
    for k in range(2):
        deg = np.minimum(rng.poisson(5 * (2 * k + 1), n), n)
        deg[rng.random(n) < 0.1] = 0
        deg[rng.integers(0, n, 3)] = [70, 300, 129]
        rows = np.repeat(np.arange(n), deg)
        cols = np.concatenate([rng.choice(n, kk, replace=False) for kk in deg])
        m = sp.csr_matrix((rng.uniform(-1, 1, len(rows)).astype(np.float32), (rows, cols)), shape=(n, n))
        m.sort_indices()
        hops.append(m)
    return hops


def _plans():
    from h2gcn_amd import HopPlan
    g = load_planetoid_golden("cora")
    yield "cora_sym", HopPlan.from_scipy([g["hop1_sym"], g["hop2_sym"]], torch.device(DEV), build_transpose=True)
    yield "cora_rw", HopPlan.from_scipy([g["hop1_rw"], g["hop2_rw"]], torch.device(DEV), build_transpose=True)
    yield "synthetic", HopPlan.from_scipy(_nonsymmetric_hops(np.random.default_rng(5), 1500), torch.device(DEV), build_transpose=True)


def hand_chain(plan, r0, K):
    """[r_K | r_0 | ... | r_{K-1}] from separate bf16 tensors: r_0 = r0 rounded, r_k = flatten(plan.spmm(r_{k-1})) (bf16 -> bf16)."""
    r = [r0.detach().to(BF)]
    for _ in range(K):
        r.append(plan.spmm(r[-1].contiguous()).flatten(1))
    return torch.cat([r[K]] + r[:K], dim=1), r


def hand_chain_backward(plan, G, widths, K):
    """the rounding order of layers._FusedPropagation: t = spmm_t(g_k) in fp32; t += slot_{k-1} widened; g_{k-1} = bf16(t) for k > 1,
    fp32 for k = 1"""
    H = plan.n_hops
    off = [0] * (K + 1)
    pos = widths[K]
    for k in range(K):
        off[k] = pos
        pos += widths[k]
    g_k = G[:, off[K]:off[K] + widths[K]].contiguous()
    for k in range(K, 0, -1):
        t = plan.spmm_t(g_k.unflatten(1, (H, widths[k - 1])).contiguous(), out_dtype=torch.float32)
        t = t + G[:, off[k - 1]:off[k - 1] + widths[k - 1]].float()
        g_k = t.to(BF) if k > 1 else t
    return g_k


@pytest.mark.parametrize("K", [1, 2, 3])
def test_bf16_propagation_equals_the_hand_built_chain_forward_and_backward(K):
    from h2gcn_amd import layers as L

    for name, plan in _plans():
        torch.manual_seed(K)
        n, d = plan.n_cols, 64
        r0 = torch.relu(torch.randn((n, d), device=DEV)).requires_grad_(True)
        want, r = hand_chain(plan, r0, K)
        widths = [t.shape[1] for t in r]
        buf = L.fused_propagation(plan, r0, K, dtype=BF)
        assert buf.dtype == BF and same_bits(buf, want), name
        with torch.no_grad():
            assert same_bits(L.fused_propagation(plan, r0, K, dtype=BF), want), name
        own = torch.full(want.shape, 3.0, device=DEV, dtype=BF)
        out = L.fused_propagation(plan, r0, K, out=own, dtype=BF)
        assert out.data_ptr() == own.data_ptr() and same_bits(own, want), name
        adopted = L.fused_propagation(plan, r0, K, out=own, reuse=True, dtype=BF)
        assert adopted.data_ptr() == own.data_ptr() and same_bits(adopted, want), name
        with pytest.raises(ValueError, match="bfloat16"):
            L.fused_propagation(plan, r0, K, out=torch.empty(want.shape, device=DEV), dtype=BF)
        # backward, through the freshly computed buffer and through the adopted one
        G = torch.randn(want.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7 + K)).to(BF)
        keep = G.clone()
        d_r0 = hand_chain_backward(plan, G, widths, K)
        assert d_r0.dtype == torch.float32
        for node in (buf, adopted):
            r0.grad = None
            node.backward(G)
            assert r0.grad.dtype == torch.float32 and same_bits(r0.grad, d_r0), name
        assert same_bits(G, keep), "the caller's gradient tensor was modified"


# ---- 6. model ------------------------------------------------------------------------------------------------------------------
def _cora_model(tmp_path, network, dtype):
    from test_entrypoints import _export_fixture
    from h2gcn_amd.datasets._dataset import PlanetoidData
    from h2gcn_amd.models import parse_network_setup
    from h2gcn_amd.models.H2GCN import H2GCN

    _export_fixture(load_planetoid_golden("cora"), tmp_path, "ind.cora")
    data = PlanetoidData("ind.cora", tmp_path, val_size=500)
    data.row_normalize_features()
    data.adj_remove_eye()
    tensors = data.get_tensors(torch.device(DEV), adj_norm_hops=["1", "2"])
    setup = parse_network_setup(network, data.num_labels, _dense_units=64, _dropout_rate=0.5)
    torch.manual_seed(0)
    model = H2GCN(setup, input_dim=tensors["features"].n_cols, n_hops=2, l2_regularize_weight=5e-4, embedding_dtype=dtype).to(DEV)
    return tensors, model


def test_model_in_bf16_mode_equals_the_composition(tmp_path, kernel_family):
    tensors, model = _cora_model(tmp_path, H2GCN2_NO_DROPOUT, BF)
    args = (tensors["adj"], tensors["features"], tensors["adj_hops"])
    plan, embed, classifier = tensors["adj_hops"], model.layer_objs[0], model.layer_objs[-1]
    model.eval()
    tagged = {}
    with torch.no_grad():
        logits = model(*args, tagged_out=tagged)
        want_buf, r = hand_chain(plan, embed(tensors["features"]), 2)
        want_logits = classifier(want_buf.float())
        emb = model(*args, return_before=-1)
    assert logits.dtype == torch.float32 and same_bits(logits, want_logits)
    assert emb.dtype == BF and same_bits(emb, want_buf)                        # embeddings keep the buffer's dtype
    assert tagged["1"].dtype == torch.float32 and tagged["2"].dtype == BF and same_bits(tagged["2"], r[1])   # r_1 is a bf16 view
    assert model._prop_buf is not None and model._prop_buf.dtype == BF and model.reuse_propagation
    # one loss.backward(): every parameter gradient equals the composition's
    model.train()
    for adopt in (True, False):            # the training forward right after an evaluation adopts its buffer; then a recomputing one
        model.zero_grad(set_to_none=True)
        if not adopt:
            model._prop_key = None
        model.loss(model(*args), tensors["y_train"], tensors["train_mask"]).backward()
        got = [p.grad.clone() for p in model.parameters()]
        model.zero_grad(set_to_none=True)
        r0 = embed(tensors["features"])
        xb32 = hand_chain(plan, r0, 2)[0].float().requires_grad_(True)
        model.loss(classifier(xb32), tensors["y_train"], tensors["train_mask"]).backward()   # classifier gradient + both l2 terms
        d_r0 = hand_chain_backward(plan, xb32.grad.to(BF), [64, 128, 256], 2)
        r0.backward(d_r0)
        for p, gq in zip(model.parameters(), got):
            assert same_bits(gq, p.grad)


def test_model_in_bf16_mode_draws_masks_like_the_f32_model(tmp_path):
    tensors, model = _cora_model(tmp_path, "M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO", BF)
    args = (tensors["adj"], tensors["features"], tensors["adj_hops"])
    model.train()
    with torch.no_grad():
        z1, z2 = model(*args), model(*args)
        assert not torch.equal(z1, z2)                       # two training forwards: two masks
        model.layer_objs[-1]._step.zero_()
        assert torch.equal(model(*args), z1)                 # the same (seed, step): the same mask


# ---- 7. accuracy of the embedding against an fp64 host product -------------------------------------------------------------
def _check_bound(plan, r0, K, label):
    """|B_bf16 - B_exact| of slot k <= ((1 + 2^-8 + L 2^-23)^(k+1) - 1) (|A|^k |r0|), element-wise: k + 1 roundings to bf16 (unit
    roundoff 2^-8: r_0 and one per round) and k fp32-accumulated products over rows of at most L terms."""
    from h2gcn_amd import layers as L_

    hops = [sp.csr_matrix((plan.vals[h].cpu().numpy().astype(np.float64), plan.colidx[h].cpu().numpy(), plan.rowptr[h].cpu().numpy()),
                          shape=(plan.n_rows, plan.n_cols)) for h in range(plan.n_hops)]
    longest = max(int(np.diff(h.indptr).max()) for h in hops)
    with torch.no_grad():
        buf = L_.fused_propagation(plan, r0, K, dtype=BF).float().cpu().numpy().astype(np.float64)
    exact, mag = [r0.cpu().numpy().astype(np.float64)], [np.abs(r0.cpu().numpy().astype(np.float64))]
    for _ in range(K):
        exact.append(np.concatenate([h @ exact[-1] for h in hops], axis=1))      # stacked as the layer stacks them
        mag.append(np.concatenate([abs(h) @ mag[-1] for h in hops], axis=1))
    order = [K] + list(range(K))
    pos, worst = 0, 0.0
    for k in order:
        w = exact[k].shape[1]
        err = np.abs(buf[:, pos:pos + w] - exact[k])
        bound = ((1 + 2.0 ** -8 + longest * 2.0 ** -23) ** (k + 1) - 1) * mag[k]
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"{label}: slot r_{k}: worst error / bound = {ratio:.3f} (longest row {longest})")
        assert (err <= bound).all(), (label, k, ratio)
        pos += w
    assert worst > 0.05, worst          # (the bf16 roundings are really there)


def test_embedding_accuracy_bound_on_cora():
    for name, plan in _plans():
        if name == "synthetic":
            continue
        torch.manual_seed(11)
        r0 = torch.relu(torch.randn((plan.n_cols, 64), device=DEV))
        for K in (1, 2, 3):
            _check_bound(plan, r0, K, f"{name} K={K}")


def test_embedding_accuracy_bound_on_the_arxiv_shape():
    from h2gcn_amd import HopPlan, synth

    cfg = synth.SHAPES["arxiv"]
    n = cfg["n"]
    device = torch.device(DEV)
    degs = synth.hop_degrees(cfg)
    csr = [synth.synth_hop_rows(degs[k], n, (synth.SEED_A1, synth.SEED_A2)[k], 0, n, device) for k in range(2)]
    x = synth.synth_features(cfg["d"], synth.SEED_X, 0, n, device)
    plan = HopPlan([c[0] for c in csr], [c[1] for c in csr], [c[2] for c in csr], n)
    r0 = torch.relu(x[:, :32]).contiguous()
    _check_bound(plan, r0, 2, "arxiv K=2")


# ---- 8 - 10. end to end ------------------------------------------------------------------------------------------------------
def _cora_dir(tmp_path):
    from test_entrypoints import _export_fixture
    _export_fixture(load_planetoid_golden("cora"), tmp_path, "ind.cora")
    return str(tmp_path)


def test_entry_point_trains_cora_in_bf16_mode(tmp_path, capsys):
    """the band tests/test_model_gpu.py::test_entry_point_trains_cora asserts for float32 (a sanity band, not a target)"""
    from h2gcn_amd import run_experiments

    args = run_experiments.main(["H2GCN", "planetoid", "--dataset", "ind.cora", "--dataset_path", _cora_dir(tmp_path),
                                 "--epochs", "120", "--random_seed", "123", "--embedding_dtype", "bfloat16"])
    out = capsys.readouterr().out
    assert "Epoch: 0001" in out and "Best performance:" in out
    model = args.objects["model"]
    assert model.embedding_dtype == BF and model._prop_buf.dtype == BF
    best = args.objects["best_val_stats"]
    assert best["val_acc"] >= 0.75 and best["test_accuracy"] >= 0.75
    first_loss = float(out.split("Train Loss:")[1].split()[0])
    assert args.objects["epoch_stats"]["train_loss"] < 0.6 * first_loss
    preds = args.objects["predict_step"](**args.objects["tensors"])
    embs = model(args.objects["tensors"]["adj"], args.objects["tensors"]["features"], args.objects["tensors"]["adj_hops"], return_before=-1)
    assert preds.dtype == torch.float32 and embs.dtype == BF


def test_hipgraph_replay_matches_eager_training_in_bf16_mode(tmp_path, capsys):
    from h2gcn_amd import run_experiments

    common = ["H2GCN", "planetoid", "--dataset", "ind.cora", "--dataset_path", _cora_dir(tmp_path), "--epochs", "25",
              "--random_seed", "7", "--network_setup", H2GCN2_NO_DROPOUT, "--embedding_dtype", "bfloat16"]
    a = run_experiments.main(common)
    stats_graph = dict(a.objects["epoch_stats"])
    assert a.objects["train_step"].__closure__ is not None
    b = run_experiments.main(common + ["--no_hipgraph"])
    stats_eager = dict(b.objects["epoch_stats"])
    for k in ("train_loss", "val_loss", "test_loss", "val_acc", "test_accuracy"):
        assert abs(stats_graph[k] - stats_eager[k]) <= 1e-4, (k, stats_graph[k], stats_eager[k])
    out = capsys.readouterr().out
    assert "capture unavailable" not in out


def test_propagation_reuse_is_invisible_in_bf16_mode(tmp_path, monkeypatch, capsys):
    from h2gcn_amd import run_experiments

    per_epoch = {}
    for reuse in ("1", "0"):
        monkeypatch.setenv("H2GCN_PROPAGATION_REUSE", reuse)
        capsys.readouterr()
        args = run_experiments.main(["H2GCN", "planetoid", "--dataset", "ind.cora", "--dataset_path", _cora_dir(tmp_path), "--epochs", "12",
                                     "--random_seed", "5", "--embedding_dtype", "bfloat16", "--json_stats"])
        assert args.objects["model"].reuse_propagation == (reuse == "1")
        per_epoch[reuse] = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith('{"epoch"')]
        assert len(per_epoch[reuse]) == 12
    assert per_epoch["1"] == per_epoch["0"]


def test_arxiv_shape_runs_through_the_entry_point_in_bf16_mode():
    from h2gcn_amd import run_experiments

    args = run_experiments.main(["H2GCN", "synthetic", "--shape", "arxiv", "--epochs", "6", "--no_feature_normalize", "--classes", "40",
                                 "--random_seed", "3", "--embedding_dtype", "bfloat16"])
    stats = args.objects["epoch_stats"]
    assert args.objects["model"].embedding_dtype == BF
    assert np.isfinite(stats["train_loss"]) and 0.0 <= stats["val_acc"] <= 1.0
