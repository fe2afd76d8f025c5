"""Segmentation validation metrics from a confusion matrix.

The counts come from ``seg_confusion`` (csrc/seg_metrics.hip) on the native backend and from
:func:`confusion_reference` (plain torch / numpy: the CPU / eager path and the kernel's oracle)
everywhere else; :func:`metrics_from_confusion` turns them into per-class IoU / Dice, their means
and the pixel accuracy on the host in fp64 (65 numbers cross once per epoch).

Counts layout, ``KC = max(K, 2)``: int64 ``[KC * KC + 1]``, ``counts[t * KC + p]`` = kept pixels with
truth ``t`` predicted as ``p``; the last slot = ignored pixels.

  * K >= 2: ``logits`` [M, K] pixel-major, ``target`` integer ids [M]. Prediction = arg-max, ties to the
    LOWEST class (``headk_mask``'s rule: a pixel is scored by the class serving would pick). A label
    >= K (255 and K..254) is ignored, as the loss ignores it.
  * K == 1: ``logits`` [M], ``target`` float [M]. Prediction = ``logit > thr`` (strict; ``thr`` is a
    logit), truth = ``target > 0.5``; a 2 x 2 matrix (class 0 = background, 1 = foreground).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch


def confusion_size(K: int) -> int:
    kc = max(int(K), 2)
    return kc * kc + 1


def threshold_logit(p: float) -> float:
    """The logit of a probability threshold (``sigmoid(x) > p  <=>  x > logit(p)``), as serving forms it."""
    p = min(max(float(p), 1e-7), 1 - 1e-7)  # serve/engine.py _logit
    return math.log(p / (1 - p))


def confusion_reference(logits, target, K: int, thr: float = 0.0) -> torch.Tensor:
    """int64 [KC*KC + 1] counts of ``logits`` (K >= 2: [M*K] / [M,K] pixel-major; K == 1: [M]) against
    ``target`` ([M]); see the module docstring for the rules."""
    K = int(K)
    if not 1 <= K <= 8:
        raise ValueError(f"1 <= K <= 8 classes, got {K}")
    kc = max(K, 2)
    x = torch.as_tensor(logits).detach().to("cpu", torch.float32).numpy()
    t = torch.as_tensor(target).detach().to("cpu").numpy().reshape(-1)
    M = t.shape[0]
    if x.size != M * K:
        raise ValueError(f"logits hold {x.size} values, expected {M} * {K}")
    if K == 1:
        pred = (x.reshape(-1) > np.float32(thr)).astype(np.int64)
        truth = (t.astype(np.float32) > np.float32(0.5)).astype(np.int64)
        keep = np.ones(M, bool)
    else:
        pred = np.argmax(x.reshape(M, K), axis=1).astype(np.int64)  # the first maximum: ties to the lowest class
        truth = t.astype(np.int64)
        keep = (truth >= 0) & (truth < K)
    counts = np.zeros(kc * kc + 1, np.int64)
    counts[: kc * kc] = np.bincount(truth[keep] * kc + pred[keep], minlength=kc * kc)
    counts[kc * kc] = M - int(keep.sum())
    return torch.from_numpy(counts)


def confusion_matrix(counts, K: int) -> List[List[int]]:
    """The KC x KC matrix (rows: truth, columns: prediction) as nested lists."""
    kc = max(int(K), 2)
    c = torch.as_tensor(counts).detach().to("cpu", torch.int64).reshape(-1)
    return c[: kc * kc].view(kc, kc).tolist()


def metrics_from_confusion(counts, K: int) -> dict:
    """``pixel_acc``, per-class ``iou`` / ``dice`` (lists; ``None`` for a class absent from truth and
    prediction), ``miou`` / ``mdice`` (means over the classes whose union is > 0; 0.0 if none), ``kept``
    and ``ignored`` pixel counts. K == 1: ``iou`` / ``dice`` are the foreground's one entry, the means
    run over background and foreground."""
    K = int(K)
    kc = max(K, 2)
    c = np.asarray(torch.as_tensor(counts).detach().to("cpu", torch.int64).reshape(-1).numpy(), np.int64)
    if c.shape[0] != kc * kc + 1:
        raise ValueError(f"counts must hold {kc * kc + 1} values for K = {K}, got {c.shape[0]}")
    m = c[: kc * kc].reshape(kc, kc).astype(np.float64)
    tp = np.diag(m)
    fp = m.sum(0) - tp
    fn = m.sum(1) - tp
    kept = float(m.sum())
    iou: List[Optional[float]] = []
    dice: List[Optional[float]] = []
    for k in range(kc):
        union = tp[k] + fp[k] + fn[k]
        iou.append(float(tp[k] / union) if union > 0 else None)
        dice.append(float(2 * tp[k] / (2 * tp[k] + fp[k] + fn[k])) if union > 0 else None)
    present = [v for v in iou if v is not None]
    present_d = [v for v in dice if v is not None]
    out = {"pixel_acc": float(tp.sum() / kept) if kept > 0 else 0.0,
           "miou": float(np.mean(present)) if present else 0.0,
           "mdice": float(np.mean(present_d)) if present_d else 0.0,
           "kept": int(kept), "ignored": int(c[kc * kc])}
    if K == 1:
        iou, dice = iou[1:], dice[1:]
    out["iou"], out["dice"] = iou, dice
    return out


def metric_items(metrics: dict, K: int, prefix: str = "val_"):
    """(name, value) pairs to log for one epoch: the three summary values, then ``iou_c{c}`` /
    ``dice_c{c}`` per class (K == 1: c = 1 only); classes whose value is ``None`` are skipped."""
    items = [(prefix + "miou", metrics["miou"]), (prefix + "mdice", metrics["mdice"]),
             (prefix + "pixel_acc", metrics["pixel_acc"])]
    first = 1 if int(K) == 1 else 0
    for j, (i, d) in enumerate(zip(metrics["iou"], metrics["dice"])):
        if i is not None:
            items.append((f"{prefix}iou_c{first + j}", i))
        if d is not None:
            items.append((f"{prefix}dice_c{first + j}", d))
    return items


class ConfusionAccumulator:
    """One epoch's confusion counts. Native backend: an int64 device buffer that ``seg_confusion`` adds
    to after every validation forward (no host sync in between; zeroed and read once per epoch).
    Eager: the host sum of :func:`confusion_reference`."""

    def __init__(self, K: int, thr: float = 0.0, device=None, native: bool = False):
        self.K, self.thr, self.native = int(K), float(thr), bool(native)
        self.counts = torch.zeros(confusion_size(K), dtype=torch.int64, device=device if native else "cpu")

    def reset(self):
        self.counts.zero_()

    def add_executor(self, ex):
        """The eval executor's ``logits`` / ``target`` right after its ``forward()``."""
        from ..ops import native
        native(build_if_missing=False).seg_confusion(ex.logits, ex.target, self.K, self.counts, self.thr)

    def add(self, logits_nchw: torch.Tensor, target: torch.Tensor):
        """Model output [N,K,H,W] and its target ([N,1,H,W] float masks or integer ids)."""
        lg = logits_nchw.detach().float()
        lg = lg.permute(0, 2, 3, 1).reshape(-1) if self.K > 1 else lg.reshape(-1)
        self.counts += confusion_reference(lg, target.reshape(-1), self.K, self.thr)

    def result(self) -> torch.Tensor:
        return self.counts.to("cpu")
