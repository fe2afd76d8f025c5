"""The fused batch gather + augmentation kernel (csrc/data_kernels.hip batch_augment) against the
plain-torch oracle (data/augment.py augment_batch_reference), and its way up through the executor,
``NativeTrainer`` and ``train_model``.

Shapes are the smallest that can still go wrong: non-square, not a multiple of the 256-lane block per
sample, more than one block, repeated and out-of-order sample indices."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# (rotation degrees, scale, tx, ty, flip): the general-affine cases, at 40 x 56
AFFINES = [(17.0, 1.13, 1.7, -2.3, False), (-31.0, 0.9, -3.2, 0.6, True), (8.5, 1.0, 0.25, 0.25, True)]
GAIN, BIAS = 1.15, -0.07


def _dev():
    return torch.device("cuda")


def _resident(S, H, W, seed, k_class=False):
    """Random-noise resident set: a one-pixel or swapped-axis error shows as a difference of order 0.3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (S, H, W, 3), generator=g, dtype=torch.uint8)
    if k_class:  # ids 0..2 plus some 255 (ignore)
        y = torch.randint(0, 3, (S, H, W), generator=g, dtype=torch.uint8)
        y[torch.rand(S, H, W, generator=g) < 0.05] = 255
    else:
        y = (torch.randint(0, 2, (S, H, W), generator=g, dtype=torch.uint8) * 255)
    return x.to(_dev()), y.to(_dev())


def _kernel(x_res, y_res, idx, params, k_class=False):
    """x_out [N,H,W,8] bf16 and target [N*H*W] from the kernel, over poisoned buffers (every element of
    both must be written, channels 3-7 included)."""
    from robotic_discovery_platform_amd.data.augment import batch_augment
    N, (H, W) = len(idx), x_res.shape[1:3]
    x_out = torch.full((N, H, W, 8), 7.0, dtype=torch.bfloat16, device=_dev())
    target = torch.full((N * H * W,), 77, dtype=torch.uint8 if k_class else torch.float32, device=_dev())
    batch_augment(x_res, y_res, idx, params.to(_dev()), x_out, target)
    torch.cuda.synchronize()
    return x_out, target


def _float_batch(x_res, y_res, idx):
    from robotic_discovery_platform_amd.data.device_data import batch_to_float
    i = torch.as_tensor(idx, device=_dev())
    return batch_to_float(x_res.index_select(0, i), y_res.index_select(0, i))


def _rows(H, W, cases, gain=1.0, bias=0.0):
    from robotic_discovery_platform_amd.data.augment import affine_params
    return torch.stack([affine_params(H, W, rotate_deg=r, scale=s, tx=tx, ty=ty, flip=f, gain=gain, bias=bias)
                        for r, s, tx, ty, f in cases])


def test_identity_is_bitwise_the_plain_path():
    from robotic_discovery_platform_amd.data.augment import identity_params
    S, H, W, idx = 5, 16, 24, [4, 0, 4]
    x_res, y_res = _resident(S, H, W, seed=0)
    x_out, target = _kernel(x_res, y_res, idx, identity_params(3))
    # what the plain path leaves in the executor's buffers: UNetExecutor.set_input's own operations
    xf, yf = _float_batch(x_res, y_res, idx)
    want_x = torch.full_like(x_out, 7.0)
    want_x.zero_()
    want_x[..., :3].copy_(xf.permute(0, 2, 3, 1))
    want_t = torch.empty_like(target)
    want_t.copy_(yf.reshape(-1))
    assert torch.equal(x_out.view(torch.int16), want_x.view(torch.int16))
    assert torch.equal(target.view(torch.int32), want_t.view(torch.int32))
    assert x_out[..., 3:].eq(0).all() and x_out[..., :3].float().abs().sum() > 0


@pytest.mark.parametrize("name,H,W,case", [("flip", 16, 24, (0.0, 1.0, 0.0, 0.0, True)),
                                           ("shift", 16, 24, (0.0, 1.0, 3.0, -2.0, False)),
                                           ("quarter_turn", 24, 24, (90.0, 1.0, 0.0, 0.0, False))])
def test_exact_coordinate_maps_are_bitwise_the_reference(name, H, W, case):
    from robotic_discovery_platform_amd.data.augment import augment_batch_reference
    idx = [2, 0, 2]
    x_res, y_res = _resident(3, H, W, seed=1)
    params = _rows(H, W, [case] * 3)
    x_out, target = _kernel(x_res, y_res, idx, params)
    xf, yf = _float_batch(x_res, y_res, idx)
    xr, yr = augment_batch_reference(xf, yf, params)
    assert not torch.equal(xr, xf)  # the map does move pixels
    assert torch.equal(x_out[..., :3].view(torch.int16), xr.permute(0, 2, 3, 1).to(torch.bfloat16).view(torch.int16))
    assert x_out[..., 3:].eq(0).all()
    assert torch.equal(target, yr.reshape(-1))
    # and the K-class target of the same map
    xk, yk = _resident(3, H, W, seed=2, k_class=True)
    _, tk = _kernel(xk, yk, idx, params, k_class=True)
    _, ykr = augment_batch_reference(xf, yk[torch.as_tensor(idx, device=_dev())], params, n_classes=3)
    assert torch.equal(tk, ykr.reshape(-1))
    if name == "shift":
        assert tk.view(3, H, W)[:, -2:, :].eq(255).all() and tk.view(3, H, W)[:, :, :3].eq(255).all()


def _bf16_ulp(v):
    """Spacing of bf16 (8 significand bits) at |v|, 0 at v = 0; fp64 tensor."""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-300)))
    return torch.where(v == 0, torch.zeros_like(v), torch.exp2(e - 7))


def _source_coords(params, H, W):
    p = params.to(device=_dev(), dtype=torch.float64).view(-1, 8, 1, 1)
    oy = torch.arange(H, dtype=torch.float64, device=_dev()).view(1, H, 1)
    ox = torch.arange(W, dtype=torch.float64, device=_dev()).view(1, 1, W)
    return p[:, 0] * ox + p[:, 1] * oy + p[:, 2], p[:, 3] * ox + p[:, 4] * oy + p[:, 5]


def _away_from_rounding_boundary(params, H, W, band=1e-3):
    """Pixels whose source coordinates are both at least ``band`` from a nearest-rounding boundary
    (200x the fp32 coordinate error at this size)."""
    sx, sy = _source_coords(params, H, W)
    dist = lambda s: ((s + 0.5) - torch.round(s + 0.5)).abs()  # noqa: E731
    return (dist(sx) >= band) & (dist(sy) >= band)


@pytest.fixture(scope="module")
def affine_case():
    H, W, idx = 40, 56, [3, 1, 3]
    return H, W, idx, _rows(H, W, AFFINES, gain=GAIN, bias=BIAS)


def test_general_affine_image_and_mask(affine_case):
    """|out - v| <= ulp_bf16(v) / 2 + 1e-4 against the fp64 oracle value v: the final rounding plus a
    slack over the fp32 coordinate / blend error (about 2e-5 at this size)."""
    from robotic_discovery_platform_amd.data.augment import augment_batch_reference
    H, W, idx, params = affine_case
    x_res, y_res = _resident(4, H, W, seed=3)
    x_out, target = _kernel(x_res, y_res, idx, params)
    xf, yf = _float_batch(x_res, y_res, idx)
    v, yr = augment_batch_reference(xf.double(), yf, params)  # fp64 in, fp64 out
    out = x_out[..., :3].permute(0, 3, 1, 2).double()
    err = (out - v).abs()
    bound = _bf16_ulp(v) / 2 + 1e-4
    print(f"image: max |out - v| {err.max().item():.3e}, max (err - ulp/2) {(err - _bf16_ulp(v) / 2).max().item():.3e}")
    assert (err <= bound).all(), f"worst excess {(err - bound).max().item():.3e}"
    assert x_out[..., 3:].eq(0).all()
    assert ((v > 0) & (v < 1)).double().mean() > 0.5  # the clamp is not what makes it pass
    keep = _away_from_rounding_boundary(params, H, W)
    excluded = 1.0 - keep.double().mean().item()
    print(f"mask: excluded share {excluded:.4%}")
    assert excluded <= 0.01
    got = target.view(3, H, W)
    assert torch.equal(got[keep], yr.view(3, H, W)[keep])
    assert got.eq(0).logical_or(got.eq(1)).all()


def test_general_affine_k_class_target(affine_case):
    from robotic_discovery_platform_amd.data.augment import augment_batch_reference
    H, W, idx, params = affine_case
    x_res, y_res = _resident(4, H, W, seed=4, k_class=True)
    _, target = _kernel(x_res, y_res, idx, params, k_class=True)
    xf, _ = _float_batch(x_res, y_res, idx)
    ids = y_res[torch.as_tensor(idx, device=_dev())]
    _, yr = augment_batch_reference(xf, ids, params, n_classes=3)
    keep = _away_from_rounding_boundary(params, H, W)
    assert 1.0 - keep.double().mean().item() <= 0.01
    got = target.view(3, H, W)
    assert got.dtype == torch.uint8 and torch.equal(got[keep], yr[keep])
    # the rotated frame leaves corners uncovered: they are ignore labels, not background
    sx, sy = _source_coords(params, H, W)
    outside = (sx < -1) | (sx > W) | (sy < -1) | (sy > H)
    assert outside.any() and got[outside].eq(255).all()


@pytest.mark.parametrize("bad", [5, -1])
def test_host_index_check_raises_before_any_launch(bad):
    from robotic_discovery_platform_amd.data.augment import batch_augment, device_order, identity_params
    with pytest.raises(ValueError):
        device_order([0, bad, 1], 5, _dev())
    x_res, y_res = _resident(5, 16, 24, seed=5)
    x_out = torch.full((3, 16, 24, 8), 7.0, dtype=torch.bfloat16, device=_dev())
    target = torch.full((3 * 16 * 24,), 77.0, device=_dev())
    with pytest.raises(ValueError):
        batch_augment(x_res, y_res, [0, bad, 1], identity_params(3), x_out, target)
    torch.cuda.synchronize()
    assert x_out.eq(7.0).all() and target.eq(77.0).all()  # nothing ran


def _trainer(K, n, size, seed=0):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    torch.manual_seed(seed)
    nat = UNetNative(3, K, depth=2, device=_dev(), init_from=UNetRef(3, K, depth=2))
    kw = {"loss": "ce"} if K > 1 else {}
    return nat, NativeTrainer(nat, n, size, size, lr=1e-3, **kw)


@pytest.mark.parametrize("K", [1, 3])
def test_native_trainer_resident_identity_matches_set_batch(K):
    """Two steps fed by set_batch_resident with identity rows against two steps fed by
    set_batch(batch_to_float(...)): bitwise equal buffers, losses and parameters, default plan mode."""
    from robotic_discovery_platform_amd.data.augment import device_order, identity_params
    S, size = 4, 32
    x_res, y_res = _resident(S, size, size, seed=6, k_class=K > 1)
    batches = [[3, 1], [0, 3]]
    runs = []
    for resident in (False, True):
        nat, tr = _trainer(K, 2, size)
        losses = []
        for idx in batches:
            if resident:
                tr.set_batch_resident(x_res, y_res, device_order(idx, S, _dev()), identity_params(2, _dev()))
            else:
                xf, yf = _float_batch(x_res, y_res, idx)
                tr.set_batch(xf, yf if K == 1 else y_res[torch.as_tensor(idx, device=_dev())])
            inputs = (tr.ex.x_in.clone(), tr.ex.target.clone())
            losses.append(tr.step().clone())
        torch.cuda.synchronize()
        runs.append((inputs, torch.stack(losses), nat.store.flat.clone()))
    (in_a, loss_a, flat_a), (in_b, loss_b, flat_b) = runs
    assert torch.equal(in_a[0].view(torch.int16), in_b[0].view(torch.int16)) and torch.equal(in_a[1], in_b[1])
    assert torch.isfinite(loss_a).all()
    assert torch.equal(loss_a, loss_b)
    assert torch.equal(flat_a, flat_b)


def test_train_model_native_augmented(tmp_path):
    from robotic_discovery_platform_amd.config import TrainConfig
    from robotic_discovery_platform_amd.mlstore import pytorch as mlpt
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.train.trainer import train_model

    def run(tag, **kw):
        root = os.path.join(str(tmp_path), tag)
        # 10 samples, 3 of them validation: 7 training samples in batches of 4 + 3 (the short last batch)
        cfg = TrainConfig(image_size=64, model_depth=2, batch_size=4, synthetic_samples=10, backend="native",
                          validation_split=0.3, learning_rate=1e-3, dataset_dir=os.path.join(root, "nodata"),
                          mlruns_dir=os.path.join(root, "mlruns"), model_output_dir=os.path.join(root, "models"), **kw)
        return train_model(cfg), os.path.join(root, "mlruns")

    res, mlruns = run("aug", epochs=2, augment=True)
    h = res["history"]
    assert res["backend"] == "native" and len(h) == 2
    assert all(math.isfinite(e["train_loss"]) and math.isfinite(e["val_loss"]) for e in h)
    model = mlpt.load_model("models:/Actuator-Segmenter/latest", map_location=_dev(), backend="native",
                            tracking_uri=mlruns)
    assert isinstance(model, UNetNative)
    plain, _ = run("plain", epochs=1, augment=False)
    assert plain["history"][0]["train_loss"] != h[0]["train_loss"]
