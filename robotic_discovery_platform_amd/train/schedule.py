"""Learning-rate schedule and gradient-norm clipping: the one definition both backends use.

``t`` is the number of completed optimizer updates (Adam's step counter before the update):

    mult(t) = (t + 1) / W                                   if t < W            (linear warmup)
            = 1                                             else if "constant"
            = r + (1 - r) / 2 * (1 + cos(pi q)),  q = min(1, (t - W) / max(1, T - W))       ("cosine")

    coef    = min(1, c / (norm + 1e-6))     (torch.nn.utils.clip_grad_norm_, L2);  1 when c == 0

with the update ``g_eff = g * coef``, ``lr_eff = lr * mult(t)``. Plain Python fp64: these functions are the
oracle of the native kernels (csrc/optim.hip ``optim_ctl_kernel`` forms the same values on the device and
rounds them once to fp32) and what ``EagerTrainer`` applies.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

SCHEDULES = ("constant", "cosine")
CLIP_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s


def _finite(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_options(clip_grad_norm: float = 0.0, lr_schedule: str = "constant", warmup_steps: int = 0,
                  total_steps: Optional[int] = None, min_lr_ratio: float = 0.0) -> None:
    """Raise ``ValueError`` for an option outside its range (the same rules on both backends)."""
    if lr_schedule not in SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {SCHEDULES}, got {lr_schedule!r}")
    if not _finite(clip_grad_norm) or clip_grad_norm < 0:
        raise ValueError(f"clip_grad_norm must be finite and >= 0 (0 = off), got {clip_grad_norm!r}")
    if not _finite(warmup_steps) or warmup_steps < 0 or int(warmup_steps) != warmup_steps:
        raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}")
    if not _finite(min_lr_ratio) or not 0.0 <= min_lr_ratio <= 1.0:
        raise ValueError(f"min_lr_ratio must lie in [0, 1], got {min_lr_ratio!r}")
    if total_steps is not None and (not _finite(total_steps) or total_steps < 0 or int(total_steps) != total_steps):
        raise ValueError(f"total_steps must be an integer >= 0, got {total_steps!r}")
    if lr_schedule == "cosine" and (total_steps is None or total_steps <= warmup_steps):
        raise ValueError(f'lr_schedule="cosine" needs total_steps > warmup_steps, got total_steps={total_steps!r}, '
                         f"warmup_steps={warmup_steps!r}")


def lr_multiplier(t: int, schedule: str = "constant", W: int = 0, T: Optional[int] = None, r: float = 0.0) -> float:
    """The factor on the base learning rate for the update that follows ``t`` completed ones."""
    check_options(0.0, schedule, W, T, r)
    if t < 0:
        raise ValueError(f"t must be >= 0, got {t!r}")
    if t < W:
        return (t + 1) / W
    if schedule == "constant":
        return 1.0
    q = min(1.0, (t - W) / max(1, T - W))
    return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q))


def clip_coef(norm: float, c: float) -> float:
    """The factor on the gradient for a total L2 norm ``norm`` and a clip threshold ``c`` (0 = off)."""
    if not _finite(c) or c < 0:
        raise ValueError(f"clip_grad_norm must be finite and >= 0 (0 = off), got {c!r}")
    if c == 0:
        return 1.0
    return min(1.0, c / (norm + CLIP_EPS))


@dataclass(frozen=True)
class OptimOptions:
    """The options of one run (constants of the run: they are part of a recorded launch plan's key)."""
    clip_grad_norm: float = 0.0
    lr_schedule: str = "constant"
    warmup_steps: int = 0
    total_steps: Optional[int] = None
    min_lr_ratio: float = 0.0

    def __post_init__(self):
        check_options(self.clip_grad_norm, self.lr_schedule, self.warmup_steps, self.total_steps, self.min_lr_ratio)

    @property
    def enabled(self) -> bool:
        return self.clip_grad_norm > 0 or self.warmup_steps > 0 or self.lr_schedule == "cosine"

    def multiplier(self, t: int) -> float:
        return lr_multiplier(t, self.lr_schedule, int(self.warmup_steps), self.total_steps, float(self.min_lr_ratio))

    def key(self) -> tuple:
        return (float(self.clip_grad_norm), self.lr_schedule, int(self.warmup_steps),
                None if self.total_steps is None else int(self.total_steps), float(self.min_lr_ratio))
