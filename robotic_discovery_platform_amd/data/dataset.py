"""Segmentation datasets.

``SegmentationDataset`` reproduces ``/root/reference/scripts/train_segmenter.py:66-100``: images and
masks are paired by identical filename; colour is read as BGR, converted to RGB and resized with
INTER_AREA; the mask is read grayscale and resized with INTER_NEAREST; both are scaled by 1/255;
items are (float32 CHW image, float32 1HW mask).

K-class form (``n_classes`` >= 2): the mask PNG's gray value is the class id, or with ``mask_values``
(a list of gray values; the position in the list is the class id) a 256-entry host LUT maps it right
after the read, before any resize (unlisted values become 255 = ignore). Items are then
(float32 CHW image, uint8 [H,W] ids); nearest resizing copies bytes, so ids survive it.

``SyntheticSegmentationDataset`` serves procedurally generated scenes (no files needed), and
``split_dataset`` is a *seeded* random split (the reference's ``random_split`` is unseeded).
"""
from __future__ import annotations

import os
import logging
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset, Subset

from .image_io import bgr2rgb, imread, imread_gray, resize_area, resize_nearest
from .synthetic import make_scene

log = logging.getLogger("rdp.data")

IGNORE_LABEL = 255


def check_n_classes(n_classes: int) -> int:
    if not isinstance(n_classes, int) or isinstance(n_classes, bool) or not 1 <= n_classes <= 8:
        raise ValueError(f"n_classes must be an integer in 1..8, got {n_classes!r}")
    return n_classes


def parse_mask_values(text) -> Optional[Tuple[int, ...]]:
    """``"0,80,160"`` (or a sequence) -> (0, 80, 160); empty -> None."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    vals = tuple(int(v) for v in (text.split(",") if isinstance(text, str) else text))
    return vals or None


def mask_lut(mask_values: Sequence[int], n_classes: int) -> np.ndarray:
    """u8 [256]: gray value -> class id (its position in ``mask_values``), 255 for unlisted values."""
    vals = [int(v) for v in mask_values]
    if len(vals) != n_classes or len(set(vals)) != len(vals) or any(not 0 <= v <= 255 for v in vals):
        raise ValueError(f"mask_values must list {n_classes} distinct gray values in 0..255, got {vals}")
    lut = np.full(256, IGNORE_LABEL, np.uint8)
    for cls, v in enumerate(vals):
        lut[v] = cls
    return lut


class SegmentationDataset(Dataset):
    def __init__(self, image_dir: str, mask_dir: str, size: Tuple[int, int] = (256, 256), cache: bool = False,
                 n_classes: int = 1, mask_values: Optional[Sequence[int]] = None):
        self.image_dir, self.mask_dir, self.size = image_dir, mask_dir, size
        self.n_classes = check_n_classes(n_classes)
        if mask_values is not None and self.n_classes == 1:
            raise ValueError("mask_values needs n_classes >= 2 (a one-class mask is its gray value / 255)")
        self._lut = mask_lut(mask_values, self.n_classes) if mask_values is not None else None
        self._warned = False
        self.ids: List[str] = sorted(f for f in os.listdir(image_dir) if os.path.isfile(os.path.join(mask_dir, f)))
        self._cache = {} if cache else None

    def __len__(self) -> int:
        return len(self.ids)

    def raw_arrays(self, idx: int) -> Tuple[np.ndarray, np.ndarray]:
        """(colour BGR u8 at file size, mask u8 at file size): input of the device-side resizes."""
        name = self.ids[idx]
        return imread(os.path.join(self.image_dir, name), color=True), self._read_mask(name)

    def _read_mask(self, name: str) -> np.ndarray:
        """The mask at file size: gray values (one class), class ids (K classes)."""
        m = imread_gray(os.path.join(self.mask_dir, name))
        if self.n_classes == 1:
            return m
        if self._lut is not None:
            return self._lut[m]
        if not self._warned and bool(((m >= self.n_classes) & (m != IGNORE_LABEL)).any()):
            self._warned = True  # (a benign race under the loader threads: at worst two warnings)
            log.warning("mask %s holds gray values in %d..254: kept, and ignored by the loss like 255 "
                        "(mask_values maps gray values to class ids)", name, self.n_classes)
        return m

    def load_arrays(self, idx: int) -> Tuple[np.ndarray, np.ndarray]:
        name = self.ids[idx]
        img = imread(os.path.join(self.image_dir, name), color=True)
        img = resize_area(bgr2rgb(img), self.size)
        mask = resize_nearest(self._read_mask(name), self.size)
        return img, mask

    def __getitem__(self, idx: int):
        if self._cache is not None and idx in self._cache:
            return self._cache[idx]
        img, mask = self.load_arrays(idx)
        x = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).contiguous()
        if self.n_classes > 1:
            y = torch.from_numpy(np.ascontiguousarray(mask))
        else:
            y = torch.from_numpy(mask.astype(np.float32) / 255.0).unsqueeze(0)
        if self._cache is not None:
            self._cache[idx] = (x, y)
        return x, y


class SyntheticSegmentationDataset(Dataset):
    def __init__(self, n: int, size: Tuple[int, int] = (256, 256), seed: int = 0, n_classes: int = 1):
        self.n, self.size, self.seed = n, size, seed
        self.n_classes = check_n_classes(n_classes)

    def __len__(self) -> int:
        return self.n

    def raw_arrays(self, idx: int) -> Tuple[np.ndarray, np.ndarray]:
        s = make_scene(self.seed + idx, n_classes=self.n_classes)
        return s.color, s.mask

    def __getitem__(self, idx: int):
        s = make_scene(self.seed + idx, n_classes=self.n_classes)
        img = resize_area(bgr2rgb(s.color), self.size)
        mask = resize_nearest(s.mask, self.size)
        x = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).contiguous()
        if self.n_classes > 1:
            return x, torch.from_numpy(np.ascontiguousarray(mask))
        y = torch.from_numpy(mask.astype(np.float32) / 255.0).unsqueeze(0)
        return x, y


def split_dataset(ds: Dataset, val_fraction: float = 0.2, seed: int = 0) -> Tuple[Subset, Subset]:
    """random_split(ds, [n - int(n*f), int(n*f)]) with a fixed generator seed."""
    n = len(ds)
    n_val = int(n * val_fraction)
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n, generator=g).tolist()
    return Subset(ds, perm[: n - n_val]), Subset(ds, perm[n - n_val:])


def preload(ds: Dataset, indices: Optional[List[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Materialise (a subset of) a dataset as two stacked tensors (host)."""
    idx = list(range(len(ds))) if indices is None else indices
    xs, ys = zip(*(ds[i] for i in idx)) if idx else ((), ())
    if not idx:
        return torch.empty(0), torch.empty(0)
    return torch.stack(xs), torch.stack(ys)
