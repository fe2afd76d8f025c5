"""Connected-component filter of the model-resolution serving mask.

A small false-positive blob away from the actuator stretches the geometry's x-bin range and pulls edge
points into the spline fit (the curvature halves while the status stays ``ok``). The filter removes small
8-connected components and, when asked, every component but the largest, before anything downstream
(nearest upsample, coverage, geometry, the response mask) sees the mask.

:func:`filter_components_reference` is the definition (numpy + ``scipy.ndimage.label``);
:func:`filter_components` runs it in place on device masks (``csrc/mask_components.hip``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

KEEP_MODES = ("all", "largest")
MAX_PIXELS = 65536  # the native kernel's limit per mask: the 256 x 256 serving mask


def check_filter(keep, min_area) -> Optional[Tuple[str, int]]:
    """Validate the options: ``(keep, min_area)``, or None for the identity setting (``"all"``, 0)."""
    if keep not in KEEP_MODES:
        raise ValueError(f"mask_components must be one of {KEEP_MODES} (got {keep!r})")
    if isinstance(min_area, bool) or int(min_area) != min_area or int(min_area) < 0:
        raise ValueError(f"mask_min_area must be an integer >= 0 (got {min_area!r})")
    min_area = int(min_area)
    return None if keep == "all" and min_area == 0 else (keep, min_area)


def check_native_size(flt: Optional[Tuple[str, int]], size: int) -> None:
    """An active filter on a native pipeline needs a model mask within the kernel's limit."""
    if flt is not None and size * size > MAX_PIXELS:
        raise ValueError(f"the mask component filter takes masks of at most {MAX_PIXELS} pixels "
                         f"(model_img_size {size} gives {size * size})")


def filter_components_reference(mask: np.ndarray, keep: str = "all", min_area: int = 0):
    """``(filtered mask, stats)`` of a u8 ``[H, W]`` mask.

    Foreground is byte > 0, connectivity is 8, a component's area is its pixel count. Components with
    area < ``min_area`` are removed; with ``keep="largest"`` only the survivor with the largest area stays
    (among equal areas the one whose first pixel in row-major order comes first; none if nothing survives).
    Kept pixels keep their byte value, all others become 0. ``stats`` = int32 [components found, components
    kept, pixels kept, pixels removed]. ``keep="all", min_area=0`` is the identity."""
    from scipy import ndimage
    flt = check_filter(keep, min_area)
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.uint8:
        raise ValueError(f"mask must be a u8 [H, W] array (got {mask.dtype} {mask.shape})")
    labels, found = ndimage.label(mask > 0, structure=np.ones((3, 3), np.int8))
    flat = labels.ravel()
    area = np.bincount(flat, minlength=found + 1)[1:]
    total = int(area.sum())
    if flt is None:
        return mask.copy(), np.array([found, found, total, 0], np.int32)
    # first pixel (row-major index) of every label, independent of the order the labels were given in
    _, first = np.unique(flat, return_index=True)
    first = first[1:] if flat.size and (flat == 0).any() else first
    alive = area >= int(min_area)
    if keep == "largest" and alive.any():
        cand = np.flatnonzero(alive)
        order = np.lexsort((first[cand], -area[cand]))  # largest area, then earliest first pixel
        alive = np.zeros(found, bool)
        alive[cand[order[0]]] = True
    kept = np.concatenate(([False], alive))[labels]
    out = np.where(kept, mask, 0).astype(np.uint8)
    pixels_kept = int(area[alive].sum())
    return out, np.array([found, int(alive.sum()), pixels_kept, total - pixels_kept], np.int32)


def filter_components(mask_dev, keep: str, min_area: int, stats=None):
    """Filter device masks in place: ``mask_dev`` is a contiguous u8 GPU tensor ``[H, W]`` or ``[n, H, W]``
    (each frame on its own); ``stats`` (optional) an int32 GPU tensor of ``n * 4`` elements that receives each
    frame's [found, kept, pixels kept, pixels removed]. Nothing is launched for the identity setting. Returns
    ``mask_dev``."""
    flt = check_filter(keep, min_area)
    if mask_dev.dim() not in (2, 3):
        raise ValueError(f"mask_dev must be [H, W] or [n, H, W] (got {tuple(mask_dev.shape)})")
    if flt is None:
        return mask_dev
    from ..ops import native
    n = 1 if mask_dev.dim() == 2 else int(mask_dev.shape[0])
    H, W = int(mask_dev.shape[-2]), int(mask_dev.shape[-1])
    native().mask_components(mask_dev, n, H, W, int(flt[0] == "largest"), flt[1], stats)
    return mask_dev
