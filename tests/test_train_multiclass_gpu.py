"""Native ``train_model`` for K classes with on-device validation metrics: trains, registers, serves,
and ``evaluate_model`` reports exactly the counts the reference gives on the executor's own logits."""
import pytest
import torch

from robotic_discovery_platform_amd import mlstore
from robotic_discovery_platform_amd.config import TrainConfig

pytestmark = pytest.mark.gpu

SIZE, SAMPLES = 64, 12


def _cfg(tmp_path, **kw):
    c = TrainConfig(epochs=2, batch_size=4, image_size=SIZE, synthetic_samples=SAMPLES, model_depth=2,
                    dataset_dir=str(tmp_path / "nodata"), mlruns_dir=str(tmp_path / "mlruns"),
                    model_output_dir=str(tmp_path / "models"), backend="native", learning_rate=1e-3,
                    val_metrics=True)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _reference_confusion(model, ds, indices, K, batch_size):
    """The counts of ``confusion_reference`` on the eval executor's own ``logits_nchw()`` and targets,
    batch by batch over the device-resident samples, and the mean loss of the batches."""
    from robotic_discovery_platform_amd.data.device_data import build_device_dataset
    from robotic_discovery_platform_amd.train.metrics import confusion_reference, confusion_size
    from robotic_discovery_platform_amd.train.trainer import _batches
    dev = torch.device("cuda")
    x, y = build_device_dataset(ds, indices, dev, (SIZE, SIZE))
    total = torch.zeros(confusion_size(K), dtype=torch.int64)
    losses = []
    for xb, yb in _batches(x, y, torch.arange(len(x)), batch_size, dev, K):
        ex = model.executor(xb.shape[0], SIZE, SIZE, training=False, loss="ce" if K > 1 else "bce")
        ex.set_input(xb, yb)
        ex.forward()
        lg = ex.logits_nchw().permute(0, 2, 3, 1).reshape(-1)
        total += confusion_reference(lg, ex.target, K)
        losses.append(float(ex.loss[0]))
    return total, sum(losses) / len(losses)


def _train_and_check(tmp_path, K, **kw):
    from robotic_discovery_platform_amd.data.dataset import SyntheticSegmentationDataset, split_dataset
    from robotic_discovery_platform_amd.train.evaluate import evaluate_model
    from robotic_discovery_platform_amd.train.metrics import confusion_matrix
    from robotic_discovery_platform_amd.train.trainer import train_model
    cfg = _cfg(tmp_path, n_classes=K, **kw)
    res = train_model(cfg)
    assert res["backend"] == "native" and res["registered_version"] == "1" and len(res["history"]) == 2
    kc = max(K, 2)
    n_val = int(SAMPLES * cfg.validation_split)
    for h in res["history"]:
        assert h["train_loss"] == h["train_loss"] and h["val_loss"] == h["val_loss"]  # finite, not NaN
        assert len(h["val_confusion"]) == kc
        assert sum(sum(r) for r in h["val_confusion"]) == n_val * SIZE * SIZE and h["val_metrics"]["ignored"] == 0
    uri, store = "models:/Actuator-Segmenter/1", str(tmp_path / "mlruns")
    model = mlstore.pytorch.load_model(uri, map_location=torch.device("cuda"), backend="native", tracking_uri=store)
    assert model.n_classes == K
    ds = SyntheticSegmentationDataset(SAMPLES, (SIZE, SIZE), seed=cfg.seed, n_classes=K)
    _, val = split_dataset(ds, cfg.validation_split, cfg.seed)
    for indices, bs in ((val.indices, 4), (list(range(SAMPLES)), 5)):  # 5: a ragged last batch of 2
        out = evaluate_model(uri, image_size=SIZE, batch_size=bs, backend="native", mlruns_dir=store, dataset=ds,
                             indices=indices)
        exp, loss = _reference_confusion(model, ds, indices, K, bs)
        assert out["confusion"] == confusion_matrix(exp, K) and out["ignored"] == int(exp[-1]) == 0
        assert out["loss"] == pytest.approx(loss, rel=1e-6) and out["samples"] == len(indices)
    return res, model


@pytest.mark.parametrize("augment", [False, True])
def test_k3_native_train_register_serve_evaluate(tmp_path, augment):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.serve.engine import FramePipeline
    res, model = _train_and_check(tmp_path, 3, augment=augment)
    st = mlstore.FileStore(str(tmp_path / "mlruns"))
    m = st.get_metrics(res["run_id"])
    assert [s for _, _, s in m["val_miou"]] == [0, 1] and "val_iou_c0" in m and "best_val_miou" in m
    assert st.get_run(res["run_id"]).data["params"]["n_classes"] == "3"
    sc = make_scene(2, n_classes=3)
    r = FramePipeline(model, DEFAULT_K, 0.001, graph=False, mask_class=1).process(sc.color, sc.depth)
    torch.cuda.synchronize()
    assert r.mask.shape == sc.depth.shape and 0.0 <= r.coverage <= 100.0


def test_binary_native_run_scores_a_2x2_matrix(tmp_path):
    res, _ = _train_and_check(tmp_path, 1)
    st = mlstore.FileStore(str(tmp_path / "mlruns"))
    m = st.get_metrics(res["run_id"])
    assert "val_iou_c1" in m and "val_iou_c0" not in m  # the truth holds foreground: its IoU is defined
    assert "n_classes" not in st.get_run(res["run_id"]).data["params"]


def test_device_dataset_keeps_class_ids(tmp_path):
    """The resident masks are the nearest-sampled ids of the file-size masks, byte for byte."""
    from robotic_discovery_platform_amd.data.dataset import SyntheticSegmentationDataset
    from robotic_discovery_platform_amd.data.device_data import build_device_dataset
    from robotic_discovery_platform_amd.data.image_io import resize_nearest
    ds = SyntheticSegmentationDataset(3, (SIZE, SIZE), seed=4, n_classes=5)
    _, y = build_device_dataset(ds, [0, 1, 2], torch.device("cuda"), (SIZE, SIZE))
    for i in range(3):
        exp = resize_nearest(ds.raw_arrays(i)[1], (SIZE, SIZE))
        assert y[i].cpu().numpy().tolist() == exp.tolist()
    assert set(torch.unique(y).tolist()) <= set(range(5)) and int(y.max()) >= 1
