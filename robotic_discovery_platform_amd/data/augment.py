"""Training augmentation: the parameter model, its plain-torch oracle and the fused device gather.

A training sample is warped by translate o rotate o scale o flip about the image centre and its
colours by a gain / bias. Per sample that is one row of 8 floats
``(m00, m01, m02, m10, m11, m12, gain, bias)``: the matrix is the INVERSE map, from an output pixel
``(ox, oy)`` to source coordinates in pixel-index units (pixel centres at integers),

    sx = m00 * ox + m01 * oy + m02,    sy = m10 * ox + m11 * oy + m12.

Sampling (``augment_batch_reference`` here and ``batch_augment`` in csrc/data_kernels.hip alike):
  * image: bilinear over the taps ``x0 = floor(sx)``, ``x0 + 1``, ``y0 = floor(sy)``, ``y0 + 1`` with the
    fractional parts as weights, over the [0, 1] values; a tap outside the frame contributes 0;
    ``out = clamp(gain * c + bias, 0, 1)``.
  * mask: nearest, ``jx = floor(sx + 0.5)``, ``jy = floor(sy + 0.5)``; outside the frame 0 for a
    one-class model and label 255 for a K-class model (ignored by the CE loss, so a warped-in border is
    not learned as background).

The draws of an epoch come from a private generator that is a function of (seed, epoch, rank) only:
the global RNG is never touched, and a resumed run re-creates epoch k's draws with nothing new in the
checkpoint.
"""
from __future__ import annotations

import hashlib
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
IGNORE_LABEL = 255


@dataclass
class AugmentSpec:
    """Ranges of the random transform; every range 0 (the default) is the identity."""
    hflip: float = 0.0  # probability of a horizontal flip
    rotate_deg: float = 0.0  # angle ~ U(-r, r) degrees
    scale: float = 0.0  # s ~ U(1 - a, 1 + a)
    translate: float = 0.0  # shift as a fraction of width / height, U(-t, t) per axis
    contrast: float = 0.0  # gain ~ U(1 - c, 1 + c)
    brightness: float = 0.0  # bias ~ U(-b, b), on the [0, 1] value scale

    @classmethod
    def from_config(cls, cfg) -> "AugmentSpec":
        """The ``aug_*`` fields of a ``TrainConfig``."""
        return cls(hflip=cfg.aug_hflip, rotate_deg=cfg.aug_rotate_deg, scale=cfg.aug_scale,
                   translate=cfg.aug_translate, contrast=cfg.aug_contrast, brightness=cfg.aug_brightness)


def _inverse_rows(theta: torch.Tensor, s: torch.Tensor, tx: torch.Tensor, ty: torch.Tensor, flip: torch.Tensor,
                  gain: torch.Tensor, bias: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """fp64 [n] angle (radians), scale, shift (pixels), flip (bool), gain, bias -> fp32 [n, 8] rows.

    Forward map about the centre c: ``p' = R(theta) * s * F * (p - c) + c + t`` with F = diag(-1, 1) for a
    flip; the row holds its inverse ``p = F * R(-theta) / s * (p' - c - t) + c``."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    cos, sin = torch.cos(theta), torch.sin(theta)
    # multiples of a quarter turn are exact maps of the pixel grid: drop the rounding residue of cos / sin
    cos = torch.where(cos.abs() < 1e-15, torch.zeros_like(cos), cos)
    sin = torch.where(sin.abs() < 1e-15, torch.zeros_like(sin), sin)
    f = torch.where(flip, -torch.ones_like(s), torch.ones_like(s))
    m00, m01 = f * cos / s, f * sin / s
    m10, m11 = -sin / s, cos / s
    px, py = cx + tx, cy + ty
    m02 = cx - (m00 * px + m01 * py)
    m12 = cy - (m10 * px + m11 * py)
    rows = torch.stack([m00, m01, m02, m10, m11, m12, gain, bias], dim=1) + 0.0  # (-0.0 -> 0.0)
    return rows.to(torch.float32)


def affine_params(H: int, W: int, rotate_deg: float = 0.0, scale: float = 1.0, tx: float = 0.0, ty: float = 0.0,
                  flip: bool = False, gain: float = 1.0, bias: float = 0.0) -> torch.Tensor:
    """One fp32 [8] row for an explicit transform (``tx`` / ``ty`` in pixels)."""
    d = lambda v: torch.tensor([float(v)], dtype=torch.float64)  # noqa: E731
    return _inverse_rows(d(math.radians(rotate_deg)), d(scale), d(tx), d(ty), torch.tensor([bool(flip)]),
                         d(gain), d(bias), H, W)[0]


def draw_params(spec: AugmentSpec, n: int, H: int, W: int, generator: torch.Generator) -> torch.Tensor:
    """``n`` random transforms of ``spec`` as fp32 [n, 8] rows, drawn from ``generator`` only."""
    u = torch.rand(n, 7, dtype=torch.float64, generator=generator)
    sym = 2.0 * u - 1.0  # U(-1, 1)
    flip = u[:, 0] < spec.hflip
    theta = sym[:, 1] * math.radians(spec.rotate_deg)
    s = 1.0 + sym[:, 2] * spec.scale
    tx = sym[:, 3] * spec.translate * W
    ty = sym[:, 4] * spec.translate * H
    gain = 1.0 + sym[:, 5] * spec.contrast
    bias = sym[:, 6] * spec.brightness
    return _inverse_rows(theta, s, tx, ty, flip, gain, bias, H, W)


def epoch_generator(seed: int, epoch: int, rank: int) -> torch.Generator:
    """A private CPU generator whose stream is a function of (seed, epoch, rank) only."""
    digest = hashlib.sha256(f"rdp-augment:{int(seed)}:{int(epoch)}:{int(rank)}".encode()).digest()
    g = torch.Generator(device="cpu")
    g.manual_seed(int.from_bytes(digest[:8], "little") >> 1)
    return g


def augment_batch_reference(x: torch.Tensor, y: Optional[torch.Tensor], params: torch.Tensor,
                            n_classes: int = 1) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Plain-torch augmentation of a float batch, computed in fp64: the CPU / eager training path and
    the oracle of the ``batch_augment`` kernel.

    ``x``: float [N,C,H,W] in [0, 1]; ``y``: one-class float masks [N,1,H,W] (outside the frame: 0), or
    with ``n_classes`` > 1 class ids [N,H,W] / [N,1,H,W] of any dtype (outside the frame: 255);
    ``params``: [N,8] rows. Returns the same shapes and dtypes."""
    N, C, H, W = x.shape
    dev = x.device
    p = params.to(device=dev, dtype=torch.float64).reshape(N, 8, 1, 1)
    oy = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    ox = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    sx = p[:, 0] * ox + p[:, 1] * oy + p[:, 2]  # [N,H,W]
    sy = p[:, 3] * ox + p[:, 4] * oy + p[:, 5]

    def gather(src, jx, jy, fill):
        """src [N,c,H,W] at integer (jx, jy) [N,H,W]; ``fill`` where the tap is outside the frame."""
        inside = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
        lin = (jy.clamp(0, H - 1) * W + jx.clamp(0, W - 1)).view(N, 1, H * W).expand(N, src.shape[1], H * W)
        v = src.reshape(N, src.shape[1], H * W).gather(2, lin).view(N, src.shape[1], H, W)
        return torch.where(inside.unsqueeze(1), v, torch.full_like(v, fill))

    x0f, y0f = torch.floor(sx), torch.floor(sy)
    ax, ay = (sx - x0f).unsqueeze(1), (sy - y0f).unsqueeze(1)
    x0, y0 = x0f.long(), y0f.long()
    xd = x.to(torch.float64)
    c = ((1.0 - ax) * (1.0 - ay) * gather(xd, x0, y0, 0.0) + ax * (1.0 - ay) * gather(xd, x0 + 1, y0, 0.0)
         + (1.0 - ax) * ay * gather(xd, x0, y0 + 1, 0.0) + ax * ay * gather(xd, x0 + 1, y0 + 1, 0.0))
    out = (p[:, 6:7] * c + p[:, 7:8]).clamp(0.0, 1.0).to(x.dtype)
    if y is None:
        return out, None
    jx, jy = torch.floor(sx + 0.5).long(), torch.floor(sy + 0.5).long()
    y4 = y.reshape(N, 1, H, W)
    ym = gather(y4, jx, jy, IGNORE_LABEL if n_classes > 1 else 0)
    return out, ym.reshape(y.shape)


def device_order(order, n_samples: int, device) -> torch.Tensor:
    """An epoch's sample order as the i32 device tensor ``batch_augment`` indexes with, checked on the
    host BEFORE the upload: an index outside [0, n_samples) raises ``ValueError`` (the kernel itself
    reads nothing for such an index, but a batch of blank samples is never what the caller meant)."""
    o = torch.as_tensor(order).to("cpu")
    if o.dim() != 1 or o.dtype.is_floating_point or o.dtype == torch.bool:
        raise ValueError("sample order must be a 1-D integer sequence")
    if o.numel() and (int(o.min()) < 0 or int(o.max()) >= n_samples):
        raise ValueError(f"sample index outside [0, {n_samples}): min {int(o.min())}, max {int(o.max())}")
    return o.to(torch.int32).to(device)


def identity_params(n: int, device=None) -> torch.Tensor:
    """[n, 8] identity rows: the fused gather without augmentation."""
    return torch.tensor(IDENTITY_ROW, dtype=torch.float32, device=device).repeat(n, 1)


def batch_augment(x_res: torch.Tensor, y_res: torch.Tensor, idx, params: torch.Tensor, x_out: torch.Tensor,
                  target: torch.Tensor) -> None:
    """The fused gather: resident u8 ``x_res`` [S,H,W,3] / ``y_res`` [S,H,W] at ``idx`` [N], warped by
    ``params`` [N,8], into ``x_out`` (bf16 [N,H,W,8]) and ``target`` (fp32 | u8 [N*H*W]) in one launch.

    ``idx`` is an i32 device tensor from :func:`device_order`, or any host sequence (checked and
    uploaded here)."""
    from ..ops import native
    if not (isinstance(idx, torch.Tensor) and idx.device.type == "cuda"):
        idx = device_order(idx, x_res.shape[0], x_res.device)
    if params.device != x_res.device or params.dtype != torch.float32:
        params = params.to(device=x_res.device, dtype=torch.float32)
    native().batch_augment(x_res, y_res, idx, params.contiguous(), x_out, target)
