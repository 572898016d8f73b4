"""GPU suite: training on the labelled rows only (H2GCN(train_rows_only=True), --train_rows_only) on the Cora fixtures -- the
row-selected classifier + the adjoint through A_k[rows]^T as one autograd node (layers.fused_propagation_classify_rows).

Tolerances are those of the tests the full path already passes: the dense float64 replica's (1e-5 on the loss, 1e-6 + 1e-4
max|want| on the gradients: test_model_gpu.py::test_gradients_match_dense_float64_replica), the fused-vs-generic one (1e-6 + 1e-5
max|off|: ::test_concat_free_propagation_equals_generic_interpreter) for flag on vs flag off -- the masks are identical by
construction, only the summation order over rows differs -- and the replay-vs-eager 1e-4 on epoch statistics."""
import json

import numpy as np
import pytest
import torch

from conftest import load_planetoid_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H2GCN2 = "M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO"


def _cora_dir(tmp_path):
    from test_entrypoints import _export_fixture
    g = load_planetoid_golden("cora")
    _export_fixture(g, tmp_path, "ind.cora")
    return g


@pytest.fixture(scope="module")
def cora(tmp_path_factory):
    from h2gcn_amd.datasets._dataset import PlanetoidData
    from h2gcn_amd.models import parse_network_setup

    tmp = tmp_path_factory.mktemp("cora")
    g = _cora_dir(tmp)
    data = PlanetoidData("ind.cora", tmp, val_size=500)
    data.row_normalize_features()
    data.adj_remove_eye()
    tensors = data.get_tensors(torch.device(DEV), adj_norm_hops=["1", "2"])
    setup = parse_network_setup(H2GCN2, data.num_labels, _dense_units=64, _dropout_rate=0.5)
    sel = tensors["adj_hops"].select_rows(tensors["train_mask"] != 0)
    return g, tensors, setup, sel


def _model(cora, seed=0, **kw):
    from h2gcn_amd.models.H2GCN import H2GCN
    _, tensors, setup, _ = cora
    torch.manual_seed(seed)
    return H2GCN(setup, input_dim=tensors["features"].n_cols, n_hops=2, l2_regularize_weight=5e-4, **kw).to(DEV)


def _rows_loss(model, cora):
    from h2gcn_amd.models._metrics import masked_softmax_cross_entropy
    _, t, _, sel = cora
    z_c = model(t["adj"], t["features"], t["adj_hops"], rows=sel)
    ones = torch.ones(len(sel), device=DEV)
    return z_c, masked_softmax_cross_entropy(z_c, t["y_train"][sel.rows_long], ones) + model.regularization_loss()


def test_eval_mode_gradients_match_dense_float64_replica(cora):
    g, t, _, sel = cora
    assert len(sel) == int(np.asarray(g["train_mask"]).sum()) == 140
    model = _model(cora, train_rows_only=True).eval()
    z_c, loss = _rows_loss(model, cora)
    assert z_c.shape == (140, t["y_train"].shape[1])
    with torch.no_grad():
        assert torch.equal(z_c, model(t["adj"], t["features"], t["adj_hops"])[sel.rows_long])   # the full logits' rows, bit for bit
    loss.backward()
    A1 = torch.from_numpy(g["hop1_sym"].toarray().astype(np.float64))
    A2 = torch.from_numpy(g["hop2_sym"].toarray().astype(np.float64))
    X = torch.from_numpy(g["feat_rownorm"].toarray().astype(np.float64))
    W0 = model.regularized[0].kernel.detach().cpu().double().requires_grad_(True)
    W1 = model.regularized[1].kernel.detach().cpu().double().requires_grad_(True)
    r0 = torch.relu(X @ W0)
    r1 = torch.cat([A1 @ r0, A2 @ r0], 1)
    r2 = torch.cat([A1 @ r1, A2 @ r1], 1)
    z = torch.cat([r2, r0, r1], 1) @ W1
    y = torch.from_numpy((g["y_all"] * g["train_mask"][:, None]).astype(np.float64))
    m = torch.from_numpy(g["train_mask"].astype(np.float64))
    ref = (-(y * torch.log_softmax(z, 1)).sum(1) * (m / m.sum())).sum() + 5e-4 * ((W0 ** 2).sum() + (W1 ** 2).sum())
    ref.backward()
    print(f"rows path vs float64 replica: loss diff {abs(loss.item() - ref.item()):.3e}")
    assert abs(loss.item() - ref.item()) <= 1e-5
    for got, want in ((model.regularized[0].kernel.grad, W0.grad), (model.regularized[1].kernel.grad, W1.grad)):
        err = (got.cpu().double() - want).abs().max().item()
        print(f"  grad max|err| {err:.3e}  bound {1e-6 + 1e-4 * want.abs().max().item():.3e}")
        assert err <= 1e-6 + 1e-4 * want.abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("adopt", [False, True])
def test_train_mode_flag_on_equals_flag_off(cora, dtype, adopt):
    """Two models with equal seeds, one forward/backward in training mode (dropout 0.5: the same mask, the step counters advance
    alike).  float32: every parameter gradient; bfloat16: the first-layer weights' gradient (both paths round at the same points)
    -- and the classifier's.  `adopt`: the training forward follows an evaluation and adopts its propagation buffer."""
    _, t, _, sel = cora
    args = (t["adj"], t["features"], t["adj_hops"])
    on, off = _model(cora, train_rows_only=True, embedding_dtype=dtype), _model(cora, embedding_dtype=dtype)
    for p, q in zip(on.parameters(), off.parameters()):
        assert torch.equal(p, q)
    for model in (on, off):
        if adopt:
            with torch.no_grad():
                model.eval()(*args)
        model.train()
    z_c, loss_on = _rows_loss(on, cora)
    z_off = off(*args)
    loss_off = off.loss(z_off, t["y_train"], t["train_mask"])
    assert torch.equal(z_c, z_off[sel.rows_long])                                           # same mask, same bits
    assert torch.equal(on.layer_objs[-1]._step, off.layer_objs[-1]._step) and int(on.layer_objs[-1]._step) == 1
    loss_on.backward()
    loss_off.backward()
    print(f"train_loss on {loss_on.item():.7f} off {loss_off.item():.7f}")
    assert abs(loss_on.item() - loss_off.item()) <= 1e-5
    for (name, p), q in zip(on.named_parameters(), off.parameters()):
        err, bound = (p.grad - q.grad).abs().max().item(), 1e-6 + 1e-5 * q.grad.abs().max().item()
        print(f"  {dtype} adopt={adopt} {name}: max|on - off| {err:.3e}  bound {bound:.3e}")
        assert err <= bound, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_mode_on_a_scattered_selection(cora, dtype):
    """Cora's train mask is rows 0 .. 139, a prefix: the same comparison on 200 rows drawn from the whole graph (row 0 and the last
    row among them), where list entry i is not row i and the workgroups of the row-selected dW kernel see other rows than the full
    call's.  Same tolerances."""
    from h2gcn_amd.models._metrics import masked_softmax_cross_entropy
    g, t, _, _ = cora
    n = t["adj_hops"].n_rows
    rng = np.random.default_rng(4)
    rows = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), 198, replace=False)]))
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[torch.from_numpy(rows).to(DEV)] = True
    y = torch.from_numpy(np.asarray(g["y_all"], dtype=np.float32)).to(DEV) * mask[:, None]
    sel = t["adj_hops"].select_rows(mask)
    args = (t["adj"], t["features"], t["adj_hops"])
    on, off = _model(cora, train_rows_only=True, embedding_dtype=dtype).train(), _model(cora, embedding_dtype=dtype).train()
    z_c = on(*args, rows=sel)
    loss_on = masked_softmax_cross_entropy(z_c, y[sel.rows_long], torch.ones(len(sel), device=DEV)) + on.regularization_loss()
    z_off = off(*args)
    loss_off = off.loss(z_off, y, mask)
    assert torch.equal(z_c, z_off[sel.rows_long])
    loss_on.backward()
    loss_off.backward()
    assert abs(loss_on.item() - loss_off.item()) <= 1e-5
    for (name, p), q in zip(on.named_parameters(), off.parameters()):
        err, bound = (p.grad - q.grad).abs().max().item(), 1e-6 + 1e-5 * q.grad.abs().max().item()
        print(f"  scattered rows {dtype} {name}: max|on - off| {err:.3e}  bound {bound:.3e}")
        assert err <= bound, name


KEYS = ("train_loss", "val_loss", "test_loss", "val_acc", "test_accuracy")


def _run(tmp_path, capsys, *extra):
    from h2gcn_amd import run_experiments
    _cora_dir(tmp_path)
    capsys.readouterr()
    a = run_experiments.main(["H2GCN", "planetoid", "--dataset", "ind.cora", "--dataset_path", str(tmp_path), "--random_seed", "7",
                              "--json_stats"] + list(extra))
    out = capsys.readouterr().out
    assert "capture unavailable" not in out
    return a, [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"epoch"')]


def test_entry_point_three_epochs_flag_on_follows_flag_off(tmp_path, capsys):
    a, on = _run(tmp_path, capsys, "--train_rows_only", "--epochs", "3")
    assert a.objects["model"].train_rows_only and len(on) == 3
    _, on_eager = _run(tmp_path, capsys, "--train_rows_only", "--epochs", "3", "--no_hipgraph")
    _, off = _run(tmp_path, capsys, "--epochs", "3")
    for k in KEYS:
        assert abs(on[-1][k] - on_eager[-1][k]) <= 1e-4, (k, on[-1][k], on_eager[-1][k])
        assert abs(on[0][k] - off[0][k]) <= 1e-4, (k, on[0][k], off[0][k])               # epoch 1: flag on vs flag off


def test_entry_point_replayed_steps_follow_eager_ones(tmp_path, capsys):
    """(three epochs are all warm-up -- the steps are captured after it: eight epochs replay the captured training step)"""
    a, on = _run(tmp_path, capsys, "--train_rows_only", "--epochs", "8")
    assert a.objects["train_step"].__closure__ is not None
    _, on_eager = _run(tmp_path, capsys, "--train_rows_only", "--epochs", "8", "--no_hipgraph")
    for k in KEYS:
        assert abs(on[-1][k] - on_eager[-1][k]) <= 1e-4, (k, on[-1][k], on_eager[-1][k])


def test_refusals(cora):
    from h2gcn_amd.models import parse_network_setup
    from h2gcn_amd.models.H2GCN import H2GCN
    _, t, setup, sel = cora
    args = (t["adj"], t["features"])
    model = _model(cora, train_rows_only=True)

    class ShardedLike:                       # what partition.ShardedHops looks like to the model
        n_hops, n_rows, n_cols = 2, 2708, 2708

        def fused_propagation(self, *a, **k):
            raise AssertionError("must not run")
    with pytest.raises(ValueError, match="row-partitioned hops"):
        model(*args, ShardedLike(), rows=sel)
    with pytest.raises(ValueError, match="fuse=True"):
        model(*args, t["adj_hops"], rows=sel, fuse=False)
    with pytest.raises(ValueError, match="--no_fused_classifier"):
        H2GCN(setup, input_dim=10, fused_classifier=False, train_rows_only=True)
    with pytest.raises(ValueError, match="units > 64"):
        H2GCN(parse_network_setup(H2GCN2, 100), input_dim=10, train_rows_only=True)
    with pytest.raises(ValueError, match="train_rows_only=True"):
        _model(cora)(*args, t["adj_hops"], rows=sel)
