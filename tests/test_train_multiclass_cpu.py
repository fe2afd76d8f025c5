"""K-class ``train_model`` / ``evaluate_model`` / ``rdp eval`` on the eager CPU path, and the promise that
nothing changes while ``n_classes = 1`` and ``val_metrics = False``."""
import json

import pytest
import torch

from robotic_discovery_platform_amd import mlstore
from robotic_discovery_platform_amd.config import TrainConfig

NEW_HISTORY_KEYS = {"val_metrics", "val_confusion"}


def _cfg(tmp_path, **kw):
    c = TrainConfig(epochs=2, batch_size=4, image_size=32, synthetic_samples=10, model_depth=2,
                    dataset_dir=str(tmp_path / "nodata"), mlruns_dir=str(tmp_path / "mlruns"),
                    model_output_dir=str(tmp_path / "models"), backend="eager", learning_rate=1e-3)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def run3(tmp_path_factory):
    """One K = 3 run with validation metrics, shared by the tests below (left unchanged by them)."""
    from robotic_discovery_platform_amd.train.trainer import train_model
    tmp = tmp_path_factory.mktemp("k3")
    cfg = _cfg(tmp, n_classes=3, val_metrics=True)
    return tmp, cfg, train_model(cfg)


def test_k3_history_and_store(run3):
    tmp, cfg, res = run3
    assert res["registered_version"] == "1" and len(res["history"]) == 2
    n_val = int(10 * cfg.validation_split)
    for h in res["history"]:
        conf = h["val_confusion"]
        assert len(conf) == 3 and all(len(r) == 3 for r in conf)
        assert sum(sum(r) for r in conf) + h["val_metrics"]["ignored"] == n_val * 32 * 32
        assert h["val_metrics"]["ignored"] == 0 and h["val_metrics"]["kept"] == n_val * 32 * 32
        assert 0.0 <= h["val_metrics"]["miou"] <= 1.0 and len(h["val_metrics"]["iou"]) == 3
    st = mlstore.FileStore(str(tmp / "mlruns"))
    m = st.get_metrics(res["run_id"])
    assert [s for _, _, s in m["val_miou"]] == [0, 1] and [s for _, _, s in m["val_pixel_acc"]] == [0, 1]
    assert "val_iou_c1" in m and "val_dice_c1" in m and "val_mdice" in m and "best_val_miou" in m
    best = min(res["history"], key=lambda h: h["val_loss"])
    assert res["best_val_miou"] == best["val_metrics"]["miou"]
    p = st.get_run(res["run_id"]).data["params"]
    assert p["n_classes"] == "3" and p["loss"] == "ce" and "mask_values" in p
    assert cfg.loss == "bce"  # the caller's config is not edited


def test_k3_model_loads_and_evaluates(run3):
    from robotic_discovery_platform_amd.data.dataset import SyntheticSegmentationDataset, preload, split_dataset
    from robotic_discovery_platform_amd.train.evaluate import evaluate_model
    from robotic_discovery_platform_amd.train.metrics import confusion_matrix, confusion_reference
    tmp, cfg, res = run3
    uri = "models:/Actuator-Segmenter/latest"
    model = mlstore.pytorch.load_model(uri, backend="eager", tracking_uri=str(tmp / "mlruns"))
    assert model.n_classes == 3
    ds = SyntheticSegmentationDataset(10, (32, 32), seed=cfg.seed, n_classes=3)
    _, val = split_dataset(ds, cfg.validation_split, cfg.seed)
    out = evaluate_model(uri, image_size=32, batch_size=4, backend="eager", mlruns_dir=str(tmp / "mlruns"),
                         dataset=ds, indices=val.indices)
    x, y = preload(ds, val.indices)
    with torch.no_grad():
        logits = model(x)
    exp = confusion_reference(logits.permute(0, 2, 3, 1).reshape(-1), y.reshape(-1), 3)
    assert out["confusion"] == confusion_matrix(exp, 3) and out["n_classes"] == 3 and out["samples"] == len(val)
    # the registered weights are the best-loss epoch's: its validation confusion is this one
    best = min(res["history"], key=lambda h: h["val_loss"])
    assert out["confusion"] == best["val_confusion"] and out["loss"] == pytest.approx(best["val_loss"], rel=1e-5)
    assert out["miou"] == best["val_metrics"]["miou"]
    with pytest.raises(ValueError):
        evaluate_model(uri, image_size=32, backend="eager", mlruns_dir=str(tmp / "mlruns"),
                       dataset=SyntheticSegmentationDataset(2, (32, 32), n_classes=2))


def test_k3_on_disk_dataset_trains_and_rdp_eval_prints_json(tmp_path, capsys):
    from robotic_discovery_platform_amd.cli import main
    from robotic_discovery_platform_amd.data.dataset import SegmentationDataset
    from robotic_discovery_platform_amd.data.synthetic import write_dataset
    from robotic_discovery_platform_amd.train.trainer import train_model
    root = tmp_path / "ds"
    write_dataset(str(root), 6, n_classes=3)
    ds = SegmentationDataset(str(root / "images"), str(root / "masks"), (32, 32), n_classes=3)
    x, y = ds[0]
    assert y.dtype == torch.uint8 and y.shape == (32, 32) and set(torch.unique(y).tolist()) <= {0, 1, 2}
    res = train_model(_cfg(tmp_path, dataset_dir=str(root), epochs=1, n_classes=3, val_metrics=True))
    assert res["registered_version"] == "1" and "val_confusion" in res["history"][0]
    capsys.readouterr()
    rc = main(["eval", "--model-uri", "models:/Actuator-Segmenter/1", "--dataset-dir", str(root), "--image-size", "32",
               "--batch-size", "4", "--backend", "eager", "--mlruns-dir", str(tmp_path / "mlruns")])
    assert rc == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_classes"] == 3 and out["samples"] == 6 and out["kept"] + out["ignored"] == 6 * 32 * 32
    assert sum(sum(r) for r in out["confusion"]) == out["kept"] and 0.0 <= out["miou"] <= 1.0
    assert set(out) >= {"loss", "pixel_acc", "miou", "mdice", "iou", "dice", "confusion"}


def test_mask_values_reach_the_dataset(tmp_path):
    """Gray values 0 / 80 / 160 on disk are mapped to ids by ``TrainConfig.mask_values``; without it the
    gray values come through as they are (80 and 160 are >= K: ignored by the loss)."""
    import numpy as np
    from robotic_discovery_platform_amd.data.image_io import imread_gray, imwrite
    from robotic_discovery_platform_amd.data.synthetic import write_dataset
    from robotic_discovery_platform_amd.train.trainer import build_dataset
    root = tmp_path / "ds"
    write_dataset(str(root), 2, n_classes=3)
    for f in (root / "masks").iterdir():
        imwrite(str(f), (imread_gray(str(f)) * 80).astype(np.uint8))
    ds = build_dataset(_cfg(tmp_path, dataset_dir=str(root), n_classes=3, mask_values="0,80,160"))
    assert set(torch.unique(ds[0][1]).tolist()) == {0, 1, 2}
    raw = build_dataset(_cfg(tmp_path, dataset_dir=str(root), n_classes=3))
    assert set(torch.unique(raw[0][1]).tolist()) == {0, 80, 160}


def test_binary_run_is_unchanged_by_val_metrics(tmp_path):
    from robotic_discovery_platform_amd.train.trainer import train_model
    off = train_model(_cfg(tmp_path / "off"))
    on = train_model(_cfg(tmp_path / "on", val_metrics=True))
    assert [h["train_loss"] for h in on["history"]] == [h["train_loss"] for h in off["history"]]
    assert [h["val_loss"] for h in on["history"]] == [h["val_loss"] for h in off["history"]]
    assert on["best_val_loss"] == off["best_val_loss"]
    # off: none of the new keys, metric names or params
    assert all(not (NEW_HISTORY_KEYS & set(h)) for h in off["history"]) and "best_val_miou" not in off
    assert set(off["history"][0]) == {"epoch", "train_loss", "val_loss", "epoch_s", "train_s", "train_imgs_per_s"}
    st = mlstore.FileStore(str(tmp_path / "off" / "mlruns"))
    assert set(st.get_metrics(off["run_id"])) == {"train_loss", "val_loss", "epoch_time_s", "train_imgs_per_s",
                                                  "best_val_loss"}
    params = st.get_run(off["run_id"]).data["params"]
    assert "n_classes" not in params and "mask_values" not in params and params["loss"] == "bce"
    # on: a 2 x 2 matrix per epoch over the whole validation set, the foreground's IoU logged as c1
    n_val = int(10 * 0.2)
    for h in on["history"]:
        assert len(h["val_confusion"]) == 2 and sum(sum(r) for r in h["val_confusion"]) == n_val * 32 * 32
        assert len(h["val_metrics"]["iou"]) == 1
    m = mlstore.FileStore(str(tmp_path / "on" / "mlruns")).get_metrics(on["run_id"])
    assert "val_miou" in m and "val_iou_c0" not in m


def test_bad_class_settings_raise(tmp_path):
    from robotic_discovery_platform_amd.train.trainer import train_model
    with pytest.raises(ValueError):
        train_model(_cfg(tmp_path, n_classes=9))
    with pytest.raises(ValueError):
        train_model(_cfg(tmp_path, n_classes=0))
    with pytest.raises(ValueError):
        train_model(_cfg(tmp_path, n_classes=3, loss="bce_dice"))


def test_cli_and_env_carry_the_new_fields(monkeypatch):
    from robotic_discovery_platform_amd import config as C
    from robotic_discovery_platform_amd.cli import _cfg_from, build_parser
    args = build_parser().parse_args(["train", "--n-classes", "3", "--mask-values", "0,80,160", "--val-metrics",
                                      "true"])
    cfg = _cfg_from(C.TrainConfig, args, "train")
    assert cfg.n_classes == 3 and cfg.mask_values == "0,80,160" and cfg.val_metrics is True
    monkeypatch.setenv("RDP_TRAIN_N_CLASSES", "4")
    assert C.apply_env(C.TrainConfig(), "train").n_classes == 4
    d = C.TrainConfig()
    assert d.n_classes == 1 and d.val_metrics is False and d.mask_values == "" and d.mask_threshold == 0.5


def test_k3_retraining_pipeline_promotes(tmp_path):
    from robotic_discovery_platform_amd.workflows.retrain import run_retraining_pipeline
    out = run_retraining_pipeline(_cfg(tmp_path, epochs=1, n_classes=3, val_metrics=True))
    assert out["promoted"] and out["version"] == "1" and "error" not in out
    c = mlstore.MlflowClient(str(tmp_path / "mlruns"))
    assert c.get_model_version_by_alias("Actuator-Segmenter", "staging").version == "1"
    cfg, _ = mlstore.pytorch.load_state("models:/Actuator-Segmenter@staging", str(tmp_path / "mlruns"))
    assert cfg["n_classes"] == 3
