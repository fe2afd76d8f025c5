"""Validation metrics on the host: the confusion-count reference (the oracle of the ``seg_confusion``
kernel), the metrics derived from the counts, and the K-class data they are computed on."""
import hashlib
import logging

import numpy as np
import pytest
import torch

from seg_cases import brute_force, planted_case
from robotic_discovery_platform_amd.train.metrics import (confusion_matrix, confusion_reference, confusion_size,
                                                          metric_items, metrics_from_confusion, threshold_logit)


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_confusion_reference_equals_brute_force(K):
    thr = 0.25 if K == 1 else 0.0
    x, t = planted_case(K, 203, thr=thr)
    got = confusion_reference(x, t, K, thr)
    assert got.dtype == torch.int64 and got.shape == (confusion_size(K),)
    assert torch.equal(got, brute_force(x, t, K, thr))
    assert int(got.sum()) == 203
    if K == 1:
        assert int(got[-1]) == 0 and int((x == thr).sum()) > 0
    else:
        assert int(got[-1]) == int((t >= K).sum()) > 0
    assert confusion_matrix(got, K) == got[:-1].view(max(K, 2), -1).tolist()


def test_confusion_reference_accepts_2d_logits_and_rejects_bad_sizes():
    x, t = planted_case(3, 50)
    assert torch.equal(confusion_reference(x.view(50, 3), t, 3), confusion_reference(x, t, 3))
    with pytest.raises(ValueError):
        confusion_reference(x[:-1], t, 3)
    with pytest.raises(ValueError):
        confusion_reference(x, t, 9)


def test_metrics_hand_computed_three_classes():
    m = [[50, 2, 3], [4, 20, 1], [0, 5, 15]]  # rows: truth, columns: prediction
    counts = torch.tensor(sum(m, []) + [7])
    r = metrics_from_confusion(counts, 3)
    assert r["kept"] == 100 and r["ignored"] == 7
    assert r["pixel_acc"] == pytest.approx(85 / 100)
    iou = [50 / (50 + 4 + 5), 20 / (20 + 7 + 5), 15 / (15 + 4 + 5)]
    dice = [100 / (100 + 4 + 5), 40 / (40 + 7 + 5), 30 / (30 + 4 + 5)]
    assert r["iou"] == pytest.approx(iou) and r["dice"] == pytest.approx(dice)
    assert r["miou"] == pytest.approx(sum(iou) / 3) and r["mdice"] == pytest.approx(sum(dice) / 3)


def test_absent_class_is_none_and_left_out_of_the_mean():
    m = [[10, 0, 2], [0, 0, 0], [3, 0, 5]]  # class 1: in neither truth nor prediction
    r = metrics_from_confusion(torch.tensor(sum(m, []) + [0]), 3)
    assert r["iou"][1] is None and r["dice"][1] is None
    assert r["miou"] == pytest.approx((10 / 15 + 5 / 10) / 2)
    names = [n for n, _ in metric_items(r, 3)]
    assert "val_iou_c0" in names and "val_iou_c2" in names and "val_iou_c1" not in names and "val_dice_c1" not in names


@pytest.mark.parametrize("K", [1, 3])
def test_all_pixels_ignored_gives_zeros(K):
    counts = torch.zeros(confusion_size(K), dtype=torch.int64)
    counts[-1] = 99
    r = metrics_from_confusion(counts, K)
    assert r["pixel_acc"] == 0.0 and r["miou"] == 0.0 and r["mdice"] == 0.0 and r["kept"] == 0 and r["ignored"] == 99
    assert all(v is None for v in r["iou"] + r["dice"])
    assert [n for n, _ in metric_items(r, K)] == ["val_miou", "val_mdice", "val_pixel_acc"]


def test_one_class_foreground_iou():
    tn, fp, fn, tp = 70, 5, 10, 15
    r = metrics_from_confusion(torch.tensor([tn, fp, fn, tp, 0]), 1)
    assert r["iou"] == pytest.approx([tp / (tp + fp + fn)])
    assert r["dice"] == pytest.approx([2 * tp / (2 * tp + fp + fn)])
    assert r["miou"] == pytest.approx((tn / (tn + fp + fn) + tp / (tp + fp + fn)) / 2)
    assert r["pixel_acc"] == pytest.approx(0.85)
    assert [n for n, _ in metric_items(r, 1)] == ["val_miou", "val_mdice", "val_pixel_acc", "val_iou_c1", "val_dice_c1"]


def test_threshold_logit():
    assert threshold_logit(0.5) == 0.0
    assert threshold_logit(0.7) == pytest.approx(np.log(0.7 / 0.3))


# ---- K-class data ----
def test_mask_values_lut(tmp_path, caplog):
    from robotic_discovery_platform_amd.data.dataset import SegmentationDataset, mask_lut
    from robotic_discovery_platform_amd.data.image_io import imwrite
    lut = mask_lut((0, 80, 160), 3)
    assert lut[0] == 0 and lut[80] == 1 and lut[160] == 2 and lut[255] == 255 and lut[81] == 255
    assert int((lut != 255).sum()) == 3
    for bad in ((0, 80), (0, 80, 80), (0, 80, 300)):
        with pytest.raises(ValueError):
            mask_lut(bad, 3)
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    rng = np.random.default_rng(0)
    gray = rng.choice(np.array([0, 80, 160, 37], np.uint8), size=(48, 64))  # 37 is unlisted
    imwrite(str(tmp_path / "images" / "a.png"), rng.integers(0, 255, (48, 64, 3), dtype=np.uint8))
    imwrite(str(tmp_path / "masks" / "a.png"), gray)
    ds = SegmentationDataset(str(tmp_path / "images"), str(tmp_path / "masks"), (64, 48), n_classes=3,
                             mask_values=(0, 80, 160))
    exp = np.select([gray == 0, gray == 80, gray == 160], [0, 1, 2], 255).astype(np.uint8)
    assert np.array_equal(ds.raw_arrays(0)[1], exp)
    x, y = ds[0]
    assert x.shape == (3, 48, 64) and x.dtype == torch.float32
    assert y.dtype == torch.uint8 and y.shape == (48, 64) and np.array_equal(y.numpy(), exp)
    # without mask_values the gray value is the id: values >= K are kept (the loss ignores them), one warning
    raw = SegmentationDataset(str(tmp_path / "images"), str(tmp_path / "masks"), (64, 48), n_classes=3)
    with caplog.at_level(logging.WARNING, logger="rdp.data"):
        assert np.array_equal(raw[0][1].numpy(), gray) and np.array_equal(raw.raw_arrays(0)[1], gray)
    assert len([r for r in caplog.records if r.name == "rdp.data"]) == 1
    with pytest.raises(ValueError):
        SegmentationDataset(str(tmp_path / "images"), str(tmp_path / "masks"), n_classes=1, mask_values=(0, 255))
    with pytest.raises(ValueError):
        SegmentationDataset(str(tmp_path / "images"), str(tmp_path / "masks"), n_classes=9)


def test_ids_survive_nearest_resize():
    from robotic_discovery_platform_amd.data.image_io import resize_nearest
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    ids = make_scene(4, n_classes=5).mask
    assert ids.shape == (480, 640)
    small = resize_nearest(ids, (64, 64))
    ys = np.minimum(np.floor(np.arange(64) * (480 / 64)).astype(int), 479)
    xs = np.minimum(np.floor(np.arange(64) * (640 / 64)).astype(int), 639)
    assert small.dtype == np.uint8 and np.array_equal(small, ids[np.ix_(ys, xs)])  # sampled bytes, never blended
    assert set(np.unique(small).tolist()) <= set(range(5))


@pytest.mark.parametrize("K", [2, 3, 8])
def test_multiclass_scene(K):
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    a, b, ref = make_scene(7, n_classes=K), make_scene(7, n_classes=K), make_scene(7)
    assert np.array_equal(a.color, b.color) and np.array_equal(a.mask, b.mask) and np.array_equal(a.depth, b.depth)
    assert np.array_equal(a.mask > 0, ref.mask > 0)  # same geometry as the binary scene of the seed
    assert np.array_equal(a.depth, ref.depth) and a.curvature == ref.curvature
    assert np.unique(a.mask).tolist() == list(range(K))  # background and every segment 1..K-1
    assert np.array_equal(a.color[a.mask == 0], ref.color[ref.mask == 0])
    if K > 2:
        assert not np.array_equal(a.color, ref.color)  # the segments have hues of their own
    with pytest.raises(ValueError):
        make_scene(7, n_classes=9)


def test_binary_synthetic_data_is_unchanged():
    """Checksums computed on the commit before the K-class scene form existed."""
    from robotic_discovery_platform_amd.data.dataset import SyntheticSegmentationDataset
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    h = hashlib.sha256()
    ds = SyntheticSegmentationDataset(3, (64, 64), 5)
    for i in range(3):
        x, y = ds[i]
        assert y.dtype == torch.float32 and y.shape == (1, 64, 64)
        h.update(x.numpy().tobytes())
        h.update(y.numpy().tobytes())
        c, m = ds.raw_arrays(i)
        h.update(c.tobytes())
        h.update(m.tobytes())
    assert h.hexdigest() == "6f788705a80bbc7aa723000e22555710ecd17a74e7d39f1ed75acc8e639a336c"
    s = make_scene(3)
    h = hashlib.sha256()
    for a in (s.color, s.depth, s.mask):
        h.update(a.tobytes())
    assert h.hexdigest() == "c9edcbff5b9075e8815fb73e1cda7d7c89862150b6ba79655097af80efb6b92c"


def test_multiclass_synthetic_dataset_items():
    from robotic_discovery_platform_amd.data.dataset import SyntheticSegmentationDataset, preload
    ds = SyntheticSegmentationDataset(3, (32, 32), 1, n_classes=4)
    x, y = preload(ds)
    assert x.shape == (3, 3, 32, 32) and y.shape == (3, 32, 32) and y.dtype == torch.uint8
    assert int(y.max()) <= 3 and int(y.max()) >= 1
