"""``evaluate_model()``: score a registered segmenter on a dataset (``rdp eval``).

Loads the model with ``mlstore.pytorch.load_model`` and takes its class count K from the stored
config, builds the dataset with that K (device-resident on the GPU), runs the eval executor and
``seg_confusion`` per batch (native) or the plain-torch path (eager), and returns the metrics of
train/metrics.py, the mean loss over the batches (``train_model``'s validation loss) and the
confusion matrix. A K-class model predicts by arg-max; a one-class model by ``mask_threshold``,
applied as a logit like serving.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from .. import mlstore
from ..config import TrainConfig
from ..data.dataset import SegmentationDataset, parse_mask_values, preload
from .metrics import ConfusionAccumulator, confusion_matrix, metrics_from_confusion, threshold_logit
from .trainer import _batches, _device, native_eval_batch


def _eager_loss(logits: torch.Tensor, target: torch.Tensor, K: int) -> torch.Tensor:
    logits = logits.float()
    if K > 1:
        labels = target.long()
        return torch.nn.functional.cross_entropy(logits, labels.squeeze(1) if labels.dim() == 4 else labels,
                                                 ignore_index=255)
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, target)


def evaluate_model(model_uri: str, dataset_dir: Optional[str] = None, image_size: int = 256, batch_size: int = 4,
                   mask_values="", mask_threshold: float = 0.5, backend: str = "auto",
                   mlruns_dir: Optional[str] = None, dataset=None, indices: Optional[Sequence[int]] = None) -> dict:
    """``dataset_dir``: ``{images,masks}/<name>`` paired by filename (default: ``TrainConfig.dataset_dir``);
    ``dataset`` (any dataset object of data/dataset.py) replaces it, ``indices`` picks a subset."""
    defaults = TrainConfig()
    mlruns_dir = mlruns_dir or defaults.mlruns_dir
    uri = mlruns_dir if "://" in mlruns_dir else os.path.abspath(mlruns_dir)
    dev = _device()
    if backend == "auto":
        backend = "native" if dev.type == "cuda" else "eager"
    model = mlstore.pytorch.load_model(model_uri, map_location=dev, backend=backend, tracking_uri=uri)
    K = int(getattr(model, "n_classes", 1))
    size = (image_size, image_size)
    if dataset is None:
        root = dataset_dir or defaults.dataset_dir
        img_dir, mask_dir = os.path.join(root, "images"), os.path.join(root, "masks")
        if not (os.path.isdir(img_dir) and os.path.isdir(mask_dir)):
            raise FileNotFoundError(f"dataset not found at {root}")
        dataset = SegmentationDataset(img_dir, mask_dir, size, n_classes=K,
                                      mask_values=parse_mask_values(mask_values) if K > 1 else None)
    elif getattr(dataset, "n_classes", K) != K:
        raise ValueError(f"the model has {K} classes, the dataset {dataset.n_classes}")
    idx = list(range(len(dataset))) if indices is None else list(indices)
    if not idx:
        raise ValueError("evaluate_model: no samples")
    if dev.type == "cuda" and hasattr(dataset, "raw_arrays"):
        from ..data.device_data import build_device_dataset
        x, y = build_device_dataset(dataset, idx, dev, size)
    else:
        x, y = preload(dataset, idx)

    native = backend == "native"
    acc = ConfusionAccumulator(K, threshold_logit(mask_threshold), device=dev, native=native)
    loss_name = "ce" if K > 1 else "bce"
    total, nb = torch.zeros((), device=dev), 0
    with torch.no_grad():
        for xb, yb in _batches(x, y, torch.arange(len(x)), batch_size, dev, K):
            if native:
                total += native_eval_batch(model, xb, yb, loss_name, confusion=acc).float()
            else:
                out = model(xb)
                acc.add(out, yb)
                total += _eager_loss(out, yb, K)
            nb += 1
    counts = acc.result()
    res = {"model_uri": model_uri, "n_classes": K, "backend": backend, "samples": len(idx),
           "loss": float(total.item()) / nb}
    res.update(metrics_from_confusion(counts, K))
    res["confusion"] = confusion_matrix(counts, K)
    return res
