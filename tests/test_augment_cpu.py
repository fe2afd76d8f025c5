"""Training augmentation on the CPU: the parameter model (data/augment.py), the plain-torch sampling
reference that is both the CPU training path and the kernel's oracle, and ``train_model`` with
``augment=True`` on the eager backend (determinism, effect, resume)."""
import math
import os

import pytest
import torch

from robotic_discovery_platform_amd.data.augment import (AugmentSpec, affine_params, augment_batch_reference,
                                                         draw_params, epoch_generator)

FULL = AugmentSpec(hflip=0.5, rotate_deg=15.0, scale=0.1, translate=0.05, contrast=0.1, brightness=0.1)


# ---------------------------------------------------------------- parameter model
def test_zero_ranges_give_exact_identity_rows():
    rows = draw_params(AugmentSpec(), 7, 24, 40, epoch_generator(3, 1, 0))
    assert rows.dtype == torch.float32 and rows.shape == (7, 8)
    want = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]).repeat(7, 1)
    assert torch.equal(rows, want)
    assert not torch.signbit(rows).any()  # no -0.0 either


def test_draws_are_a_function_of_seed_epoch_rank():
    a = draw_params(FULL, 16, 32, 48, epoch_generator(5, 2, 1))
    b = draw_params(FULL, 16, 32, 48, epoch_generator(5, 2, 1))
    assert torch.equal(a, b)
    for other in ((5, 3, 1), (5, 2, 0), (6, 2, 1)):
        assert not torch.equal(a, draw_params(FULL, 16, 32, 48, epoch_generator(*other))), other


def test_draws_stay_inside_the_spec():
    H, W = 32, 48
    rows = draw_params(FULL, 1000, H, W, epoch_generator(0, 0, 0)).double()
    gain, bias = rows[:, 6], rows[:, 7]
    assert (gain >= 1 - FULL.contrast - 1e-6).all() and (gain <= 1 + FULL.contrast + 1e-6).all()
    assert (bias.abs() <= FULL.brightness + 1e-6).all()
    # the row is the inverse map: |det| = 1 / s^2 with s in [1 - a, 1 + a]
    det = (rows[:, 0] * rows[:, 4] - rows[:, 1] * rows[:, 3]).abs()
    assert (det >= 1 / (1 + FULL.scale) ** 2 - 1e-5).all() and (det <= 1 / (1 - FULL.scale) ** 2 + 1e-5).all()
    flips = (rows[:, 0] * rows[:, 4] - rows[:, 1] * rows[:, 3]) < 0
    assert 400 < int(flips.sum()) < 600  # p = 0.5: 1000 draws are within 6 sigma of 500
    # every range is actually used
    assert gain.max() - gain.min() > 0.15 and bias.max() - bias.min() > 0.15 and det.max() - det.min() > 0.3
    # the centre moves by the shift only: forward(centre) = centre + t, |t| <= translate * size
    cx, cy = (W - 1) / 2, (H - 1) / 2
    m = rows[:, :6].reshape(-1, 2, 3)
    # solve M p' + m2 = centre for p' (the forward image of the centre)
    rhs = torch.stack([cx - m[:, 0, 2], cy - m[:, 1, 2]], 1).unsqueeze(2)
    fwd = torch.linalg.solve(m[:, :, :2], rhs).squeeze(2)
    assert ((fwd[:, 0] - cx).abs() <= FULL.translate * W + 1e-3).all()
    assert ((fwd[:, 1] - cy).abs() <= FULL.translate * H + 1e-3).all()


def test_draw_leaves_the_global_rng_alone():
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    draw_params(FULL, 64, 16, 16, epoch_generator(1, 2, 3))
    assert torch.equal(before, torch.get_rng_state())


# ---------------------------------------------------------------- reference sampling
def _batch(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 3, h, w), generator=g).float() / 255.0
    y = (torch.rand(n, 1, h, w, generator=g) > 0.5).float()
    return x, y


def _rows(row, n):
    return row.unsqueeze(0).repeat(n, 1)


def test_reference_identity_is_bitwise():
    x, y = _batch(2, 12, 20)
    xo, yo = augment_batch_reference(x, y, _rows(affine_params(12, 20), 2))
    assert xo.dtype == x.dtype and yo.dtype == y.dtype and yo.shape == y.shape
    assert torch.equal(xo, x) and torch.equal(yo, y)


def test_reference_flip_equals_torch_flip():
    x, y = _batch(2, 12, 20)
    xo, yo = augment_batch_reference(x, y, _rows(affine_params(12, 20, flip=True), 2))
    assert torch.equal(xo, torch.flip(x, dims=[3])) and torch.equal(yo, torch.flip(y, dims=[3]))


def test_reference_integer_shift_is_zero_filled():
    x, y = _batch(2, 12, 20)
    xo, yo = augment_batch_reference(x, y, _rows(affine_params(12, 20, tx=3, ty=-2), 2))
    # content moves right by 3 and up by 2; the uncovered border is 0
    for src, out in ((x, xo), (y, yo)):
        want = torch.zeros_like(src)
        want[:, :, :-2, 3:] = src[:, :, 2:, :-3]
        assert torch.equal(out, want)


def test_reference_quarter_turn_equals_rot90():
    x, y = _batch(2, 16, 16)
    xo, yo = augment_batch_reference(x, y, _rows(affine_params(16, 16, rotate_deg=90.0), 2))
    # +90 degrees in pixel coordinates (y down) is a clockwise turn on screen: rot90 with k = -1
    assert torch.equal(xo, torch.rot90(x, -1, dims=(2, 3))) and torch.equal(yo, torch.rot90(y, -1, dims=(2, 3)))


def test_reference_gain_bias_clamp():
    x, y = _batch(1, 8, 8)
    xo, _ = augment_batch_reference(x, y, _rows(affine_params(8, 8, gain=1.5, bias=-0.2), 1))
    want = (x.double() * torch.tensor(1.5, dtype=torch.float32).double()
            + torch.tensor(-0.2, dtype=torch.float32).double()).clamp(0, 1).float()
    assert torch.equal(xo, want) and xo.min() == 0.0 and xo.max() == 1.0


def test_reference_k_class_fill_is_255():
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 12, 20, generator=g)
    ids = torch.randint(0, 3, (2, 12, 20), generator=g).to(torch.uint8)
    rows = _rows(affine_params(12, 20, tx=3, ty=-2), 2)
    _, yo = augment_batch_reference(x, ids, rows, n_classes=3)
    assert yo.dtype == torch.uint8 and yo.shape == ids.shape
    want = torch.full_like(ids, 255)
    want[:, :-2, 3:] = ids[:, 2:, :-3]
    assert torch.equal(yo, want)
    _, y1 = augment_batch_reference(x, ids.float().unsqueeze(1), rows)  # one-class: 0 outside
    assert y1[:, :, -2:, :].eq(0).all() and y1[:, :, :, :3].eq(0).all()


# ---------------------------------------------------------------- train_model, eager backend on the CPU
def _cfg(root, tag, **kw):
    from robotic_discovery_platform_amd.config import TrainConfig
    base = dict(image_size=32, model_depth=2, synthetic_samples=10, batch_size=2, epochs=2, backend="eager",
                learning_rate=1e-3, dataset_dir=os.path.join(root, "nodata"),
                mlruns_dir=os.path.join(root, f"mlruns_{tag}"), model_output_dir=os.path.join(root, f"models_{tag}"))
    base.update(kw)
    return TrainConfig(**base)


def _train(root, tag, resume=None, **kw):
    from robotic_discovery_platform_amd.mlstore import pytorch as mlpt
    from robotic_discovery_platform_amd.train.trainer import train_model
    cfg = _cfg(root, tag, **kw)
    res = train_model(cfg, resume=resume)
    _, sd = mlpt.load_state("models:/Actuator-Segmenter/latest", cfg.mlruns_dir)
    return res["history"], sd


@pytest.fixture(scope="module")
def cpu_only():
    # train_model picks the device itself: keep these runs on the CPU on a GPU machine too
    import unittest.mock as mock
    with mock.patch("torch.cuda.is_available", return_value=False):
        yield


@pytest.fixture(scope="module")
def straight_run(tmp_path_factory, cpu_only):
    root = str(tmp_path_factory.mktemp("aug_straight"))
    return _train(root, "a", augment=True)


def _losses(hist):
    return [(h["train_loss"], h["val_loss"]) for h in hist]


def test_train_model_augmented_is_deterministic(tmp_path, cpu_only, straight_run):
    hist_a, sd_a = straight_run
    hist_b, sd_b = _train(str(tmp_path), "b", augment=True)
    assert _losses(hist_a) == _losses(hist_b)
    assert all(math.isfinite(v) for pair in _losses(hist_a) for v in pair)
    assert sd_a.keys() == sd_b.keys()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k


def test_train_model_augmentation_changes_the_training(tmp_path, cpu_only, straight_run):
    hist_plain, _ = _train(str(tmp_path), "plain", augment=False, epochs=1)
    assert hist_plain[0]["train_loss"] != straight_run[0][0]["train_loss"]


def test_train_model_augmented_resume_matches_straight_run(tmp_path, cpu_only, straight_run):
    root = str(tmp_path)
    _train(root, "r", augment=True, epochs=1)
    hist, sd = _train(root, "r", resume="auto", augment=True, epochs=2)
    assert [h["epoch"] for h in hist] == [1]
    assert _losses(hist) == _losses(straight_run[0][1:])
    for k in straight_run[1]:
        assert torch.equal(sd[k], straight_run[1][k]), k


# ---------------------------------------------------------------- configuration surface
def test_env_and_cli_reach_the_config(monkeypatch):
    from robotic_discovery_platform_amd import cli, config as C
    assert C.TrainConfig().augment is False
    monkeypatch.setenv("RDP_TRAIN_AUGMENT", "1")
    monkeypatch.setenv("RDP_TRAIN_AUG_SCALE", "0.25")
    cfg = C.apply_env(C.TrainConfig(), "train")
    assert cfg.augment is True and cfg.aug_scale == 0.25
    monkeypatch.delenv("RDP_TRAIN_AUGMENT")
    monkeypatch.delenv("RDP_TRAIN_AUG_SCALE")
    args = cli.build_parser().parse_args(["train", "--augment", "1", "--aug-rotate-deg", "5"])
    cfg = cli._cfg_from(C.TrainConfig, args, "train")
    assert cfg.augment is True and cfg.aug_rotate_deg == 5.0 and cfg.aug_hflip == 0.5
    spec = AugmentSpec.from_config(cfg)
    assert spec.rotate_deg == 5.0 and spec.hflip == 0.5 and spec.brightness == 0.1
