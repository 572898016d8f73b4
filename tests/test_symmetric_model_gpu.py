"""GPU suite: the model on symmetric hop plans (get_tensors(symmetric_hops=True), --symmetric_hops) on Cora as the reference
ships it (tests/golden/planetoid/).  The option changes which arrays the backward reads, never a bit it computes: with equal
seeds, five training steps and an evaluation give torch.equal losses, accuracies and parameters with the option on and off."""
import gzip
import json
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H2GCN2 = "M64-R-T1-G-V-T2-G-V-C1-C2-D0.5-MO"
PLANETOID = Path(__file__).resolve().parent / "golden" / "planetoid"


def _cora_files(tmp):
    files = sorted(PLANETOID.glob("ind.cora.*.gz"))
    assert len(files) == 8, files
    for f in files:
        (tmp / f.name[: -len(".gz")]).write_bytes(gzip.decompress(f.read_bytes()))
    return tmp


@pytest.fixture(scope="module")
def cora_dir(tmp_path_factory):
    return _cora_files(tmp_path_factory.mktemp("cora"))


def _dataset(cora_dir):
    from h2gcn_amd.datasets._dataset import PlanetoidData
    data = PlanetoidData("ind.cora", cora_dir, val_size=500)
    data.row_normalize_features()
    data.adj_remove_eye()
    return data


def _five_steps_and_an_evaluation(data, symmetric, norm="sym", **model_kw):
    """The steps of the entry point (models/H2GCN.py::initialize_model), eager; returns every tensor they produced."""
    from h2gcn_amd.models import parse_network_setup
    from h2gcn_amd.models.H2GCN import initialize_model

    torch.manual_seed(5)
    tensors = data.get_tensors(torch.device(DEV), adj_norm_hops=["1", "2"], norm=norm, symmetric_hops=symmetric)
    args = SimpleNamespace(objects=dict(tensors=tensors, post_epoch_callbacks=[], post_train_callbacks=[]), _device=DEV,
                           _no_hipgraph=True, best_val_criteria="val_acc", **model_kw)
    setup = parse_network_setup(H2GCN2, data.num_labels, _dense_units=64, _dropout_rate=0.5)
    initialize_model(args, setup, "adam", 0.01, 5e-4, 0)
    out = []
    for _ in range(5):
        out.append(args.objects["train_step"](**tensors)["train_loss"])
    stats = args.objects["test_step"](**tensors)
    out += [stats[k] for k in ("train_acc", "val_acc", "test_accuracy", "val_loss", "test_loss")]
    out += [p.detach() for p in args.objects["model"].parameters()]
    return tensors["adj_hops"], out


@pytest.mark.parametrize("config", [
    dict(),
    dict(embedding_dtype="bfloat16"),
    dict(train_rows_only=True),
    dict(norm="rw"),
], ids=["fp32", "bf16", "train_rows_only", "adj_norm_rw"])
def test_symmetric_hops_change_no_bit_of_training(cora_dir, config):
    config = dict(config)
    norm = config.pop("norm", "sym")
    data = _dataset(cora_dir)
    plan_on, on = _five_steps_and_an_evaluation(data, True, norm, **config)
    plan_off, off = _five_steps_and_an_evaluation(data, False, norm, **config)
    assert plan_on.transpose_sharing == ["indices+values" if norm == "sym" else "indices"] * 2
    assert plan_off.transpose_sharing == ["none"] * 2
    assert plan_off.device_bytes() - plan_on.device_bytes() >= sum((8 if norm == "sym" else 4) * z + 8 * (plan_on.n_rows + 1)
                                                                   for z in plan_on.nnz)
    assert len(on) == len(off) >= 5 + 5 + 2
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.dtype == b.dtype and torch.equal(a, b), i
    assert torch.isfinite(on[4]) and float(on[4]) < float(on[0])          # (it trains)


def _run(cora_dir, capsys, *extra):
    from h2gcn_amd import run_experiments
    capsys.readouterr()
    a = run_experiments.main(["H2GCN", "planetoid", "--dataset", "ind.cora", "--dataset_path", str(cora_dir), "--random_seed", "7",
                              "--json_stats", "--epochs", "6"] + list(extra))
    out = capsys.readouterr().out
    assert "capture unavailable" not in out
    return a, [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"epoch"')]


def test_entry_point_with_hipgraph_replay(cora_dir, capsys):
    """Six epochs: three eager warm-up epochs, the capture, then replayed steps -- the plan (and its mirror pass) exists before any
    capture.  The per-epoch statistics lines are identical with the option on and off."""
    from h2gcn_amd.models.H2GCN import _GraphedSteps
    assert 6 > _GraphedSteps.WARMUP + 1
    a_on, on = _run(cora_dir, capsys, "--symmetric_hops")
    a_off, off = _run(cora_dir, capsys)
    assert a_on.objects["train_step"].__closure__ is not None                # the graphed steps
    assert a_on.objects["tensors"]["adj_hops"].transpose_sharing == ["indices+values"] * 2
    assert a_off.objects["tensors"]["adj_hops"].transpose_sharing == ["none"] * 2
    assert len(on) == len(off) == 6
    assert on == off
