"""``train_model()``: the reference training + registration pipeline on the native engine.

Mirrors ``/root/reference/scripts/train_segmenter.py:103-210`` step by step:
  * MLflow setup: tracking URI = file store ``ml/mlruns``, experiment "Actuator Segmentation" (:112-113)
  * params logged: learning_rate, batch_size, epochs, validation_split, image_size, device, architecture (:119-128)
  * dataset ``ml/datasets/processed/{images,masks}`` paired by filename, 80/20 split (:132-136) -- seeded here;
    synthetic scenes are generated when the directory is missing (no camera/data in this environment)
  * UNet(3,1), Adam(lr 1e-4), BCEWithLogitsLoss (:143-145); optional BCE+Dice (north star)
  * per epoch: train loss (mean over batches), eval-mode val loss, both logged with step=epoch (:151-184)
  * best-val checkpoint ``best_segmentation_model.pth`` (state_dict, :186-189), ``best_val_loss`` metric (:191)
  * best weights logged as artifact "model" and registered as "Actuator-Segmenter" (:195-207)

MI355X-native differences: the step runs on the HIP kernels (hipGraph-captured on one GPU), the
loss is accumulated on device and read once per epoch (the reference syncs with ``.item()`` every
step), DDP over RCCL with rank-0-only store writes, and a full resume checkpoint
(model + Adam state + epoch + best val + RNG) beside the best-only one. Optional augmentation
(``augment``, off by default; the reference has none): per-sample flip / rotate / scale / shift and
contrast / brightness jitter, fused into the batch gather on the native backend (data/augment.py).
K-class training (``n_classes`` 2..8; the reference is binary): UNet(3, K), softmax cross-entropy over
integer class ids (255 = ignore). ``val_metrics``: per-epoch IoU / Dice / pixel accuracy from confusion
counts accumulated on the device (train/metrics.py, csrc/seg_metrics.hip). Both are off by default.
``clip_grad_norm`` / ``lr_schedule`` / ``warmup_steps`` / ``min_lr_ratio`` (off by default; the reference has
neither): gradient-norm clipping and a warmup / cosine learning-rate schedule over the run's steps, on both
backends (train/schedule.py); ``lr`` and ``grad_norm`` of each epoch's last step are then logged.
"""
from __future__ import annotations

import logging
import os
import time
from dataclasses import asdict, replace
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from .. import mlstore
from ..config import TrainConfig
from ..data.dataset import (SegmentationDataset, SyntheticSegmentationDataset, check_n_classes, parse_mask_values,
                            preload, split_dataset)
from ..data.synthetic import write_dataset
from ..models.unet_ref import UNetRef
from ..parallel.ddp import DistributedShardSampler, dist_info
from .losses import check_class_weights, parse_class_weights
from .schedule import OptimOptions

log = logging.getLogger("rdp.train")


def _device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    return torch.device("cpu")


def _pick_backend(cfg: TrainConfig, dev: torch.device) -> str:
    if cfg.backend != "auto":
        return cfg.backend
    return "native" if dev.type == "cuda" else "eager"


def resolve_classes(cfg: TrainConfig) -> TrainConfig:
    """Validate ``n_classes`` (1..8) and settle the loss of a K-class run: "ce" or "ce_dice"; the default
    "bce" is switched to "ce", an explicit "bce_dice" raises as the trainers do. ``class_weights`` ("1,4,4")
    must list ``n_classes`` valid weights; a one-class run takes neither them nor "ce_dice". Returns ``cfg``
    or an edited copy."""
    k = check_n_classes(cfg.n_classes)
    weights = parse_class_weights(cfg.class_weights)
    if k == 1:
        if cfg.loss == "ce_dice" or weights is not None:
            raise ValueError('loss="ce_dice" and class_weights need n_classes > 1 '
                             '(the one-class model takes "bce" / "bce_dice")')
        return cfg
    check_class_weights(weights, k)
    if cfg.loss == "bce":
        log.info('n_classes = %d: the loss is softmax cross-entropy ("ce")', k)
        return replace(cfg, loss="ce")
    if cfg.loss not in ("ce", "ce_dice"):
        raise ValueError(f'a {k}-class model trains with loss="ce" or "ce_dice", got {cfg.loss!r}')
    return cfg


def native_eval_batch(model, x, y, loss: str, dice_weight: float = 1.0, confusion=None,
                      class_weights=None) -> torch.Tensor:
    """Eval-mode forward of one batch on the native executor; returns the device loss. ``confusion`` (a
    ``ConfusionAccumulator``) also takes the batch's counts, from the executor's own logits / target."""
    ex = model.executor(x.shape[0], x.shape[2], x.shape[3], training=False, loss=loss, dice_weight=dice_weight,
                        class_weights=class_weights)
    ex.set_input(x, y)
    ex.forward()
    if confusion is not None:
        confusion.add_executor(ex)
    return ex.loss[0]


class _NativeRunner:
    """Per-batch-shape native executors (+ hipGraphs) over one model / one Adam state."""

    def __init__(self, model, cfg: TrainConfig, options: Optional[OptimOptions] = None):
        from ..models.unet import NativeAdam
        from .engine import NativeTrainer
        self.model, self.cfg = model, cfg
        self.class_weights = parse_class_weights(cfg.class_weights)
        self._trainers = {}
        self._cls = NativeTrainer
        # one Adam (state, step counter, clip / schedule options) for every batch shape: a ragged last
        # batch's trainer follows the same device step counter, hence the same schedule
        self._opt_kw = _optim_kwargs(options)
        self._shared_opt = NativeAdam(model, lr=cfg.learning_rate, **self._opt_kw)

    def _get(self, n, h, w):
        key = (n, h, w)
        if key not in self._trainers:
            tr = self._cls(self.model, n, h, w, lr=self.cfg.learning_rate, loss=self.cfg.loss,
                           dice_weight=self.cfg.dice_weight, graph=self.cfg.graph, bucket_mb=self.cfg.grad_bucket_mb,
                           sync_bn=self.cfg.sync_bn, grad_comm=self.cfg.grad_comm, class_weights=self.class_weights,
                           **self._opt_kw)
            tr.opt = self._shared_opt
            self._trainers[key] = tr
        return self._trainers[key]

    def train_step(self, x, y) -> torch.Tensor:
        tr = self._get(x.shape[0], x.shape[2], x.shape[3])
        tr.set_batch(x, y)
        return tr.step()[0]

    def train_step_resident(self, x_res, y_res, idx, params) -> torch.Tensor:
        """A step on the samples ``idx`` of the device-resident u8 dataset, gathered and augmented by one
        kernel straight into the executor's buffers (``idx`` / ``params``: device views of the epoch's)."""
        tr = self._get(idx.shape[0], x_res.shape[1], x_res.shape[2])
        tr.set_batch_resident(x_res, y_res, idx, params)
        return tr.step()[0]

    def eval_loss(self, x, y, confusion=None) -> torch.Tensor:
        return native_eval_batch(self.model, x, y, self.cfg.loss, self.cfg.dice_weight, confusion,
                                 self.class_weights)

    def optimizer_state(self):
        return self._shared_opt.state_dict()

    def load_optimizer_state(self, sd):
        self._shared_opt.load_state_dict(sd)

    def last_optim(self):
        """(lr, grad_norm or None) of the last step: one host read of the device scalars, per epoch."""
        ctl = self._shared_opt.last_ctl()
        clip = self._shared_opt.options.clip_grad_norm > 0
        return self._shared_opt.lr * ctl["mult"], (ctl["norm"] if clip else None)


def _optim_kwargs(options: Optional[OptimOptions]) -> dict:
    if options is None:
        return {}
    return {"clip_grad_norm": options.clip_grad_norm, "lr_schedule": options.lr_schedule,
            "warmup_steps": options.warmup_steps, "total_steps": options.total_steps,
            "min_lr_ratio": options.min_lr_ratio}


class _EagerRunner:
    def __init__(self, model, cfg: TrainConfig, dev, options: Optional[OptimOptions] = None):
        from .engine import EagerTrainer
        amp = torch.bfloat16 if (dev.type == "cuda" and cfg.dtype == "bf16") else None
        self.tr = EagerTrainer(model, lr=cfg.learning_rate, loss=cfg.loss, dice_weight=cfg.dice_weight,
                               bucket_mb=cfg.grad_bucket_mb, amp=amp,
                               class_weights=parse_class_weights(cfg.class_weights), **_optim_kwargs(options))
        self.model = model

    def train_step(self, x, y):
        self.model.train()
        return self.tr.step(x, y)

    @torch.no_grad()
    def eval_loss(self, x, y, confusion=None):
        self.model.eval()
        out = self.model(x)
        if confusion is not None:
            confusion.add(out, y)
        return self.tr.compute_loss(out, y)

    def optimizer_state(self):
        return self.tr.opt.state_dict()

    def load_optimizer_state(self, sd):
        self.tr.opt.load_state_dict(sd)

    def last_optim(self):
        gn = self.tr.last_grad_norm
        return self.tr.last_lr, (float(gn.item()) if gn is not None else None)


def _batches(x: torch.Tensor, y: torch.Tensor, order, bs: int, dev, n_classes: int = 1):
    """Batches (float NCHW image, float N1HW mask) in ``order``; u8 device-resident data is gathered
    and converted on the device. K classes: the mask is the u8 [N,H,W] class ids, handed on as gathered."""
    if x.dtype == torch.uint8:
        from ..data.device_data import batch_to_float, batch_to_float_ids
        convert = batch_to_float_ids if n_classes > 1 else batch_to_float
        order = order.to(x.device)
        for i in range(0, len(order), bs):
            idx = order[i:i + bs]
            yield convert(x.index_select(0, idx), y.index_select(0, idx))
        return
    for i in range(0, len(order), bs):
        idx = order[i:i + bs]
        yield x[idx].to(dev, non_blocking=True), y[idx].to(dev, non_blocking=True)


def build_dataset(cfg: TrainConfig):
    img_dir = os.path.join(cfg.dataset_dir, "images")
    mask_dir = os.path.join(cfg.dataset_dir, "masks")
    size = (cfg.image_size, cfg.image_size)
    if os.path.isdir(img_dir) and os.path.isdir(mask_dir) and os.listdir(img_dir):
        if cfg.n_classes > 1:
            return SegmentationDataset(img_dir, mask_dir, size, n_classes=cfg.n_classes,
                                       mask_values=parse_mask_values(cfg.mask_values))
        return SegmentationDataset(img_dir, mask_dir, size)
    if not cfg.synthetic_if_missing:
        raise FileNotFoundError(f"dataset not found at {cfg.dataset_dir}")
    log.info("dataset %s missing: using %d synthetic scenes", cfg.dataset_dir, cfg.synthetic_samples)
    if cfg.n_classes > 1:
        return SyntheticSegmentationDataset(cfg.synthetic_samples, size, seed=cfg.seed, n_classes=cfg.n_classes)
    return SyntheticSegmentationDataset(cfg.synthetic_samples, size, seed=cfg.seed)


def train_model(cfg: Optional[TrainConfig] = None, resume: Optional[str] = None) -> dict:
    cfg = cfg or TrainConfig()
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    cfg = resolve_classes(cfg)
    K = cfg.n_classes
    rank, world = dist_info()
    dev = _device()
    backend = _pick_backend(cfg, dev)
    is_main = rank == 0
    torch.manual_seed(cfg.seed)
    np.random.seed(cfg.seed)
    os.makedirs(cfg.model_output_dir, exist_ok=True)

    if is_main:
        mlstore.set_tracking_uri(cfg.mlruns_dir if "://" in cfg.mlruns_dir else os.path.abspath(cfg.mlruns_dir))
        mlstore.set_experiment(cfg.experiment_name)
        run = mlstore.start_run()
        log.info("Starting run %s", run.info.run_name)
        mlstore.log_params({"learning_rate": cfg.learning_rate, "batch_size": cfg.batch_size, "epochs": cfg.epochs,
                            "validation_split": cfg.validation_split, "image_size": cfg.image_size,
                            "device": str(dev), "architecture": "UNet", "backend": backend, "world_size": world,
                            "loss": cfg.loss, "dtype": cfg.dtype, "augment": cfg.augment})
        if cfg.augment:
            mlstore.log_params({k: v for k, v in asdict(cfg).items() if k.startswith("aug_")})
        if K > 1:
            mlstore.log_params({"n_classes": K, "mask_values": cfg.mask_values})
            if cfg.class_weights.strip():
                mlstore.log_params({"class_weights": cfg.class_weights})

    # ---- data ----
    # GPU: the processed dataset is built once on the device (u8 NHWC; INTER_AREA / nearest resizes
    # as kernels) and batches are gathered there -- no per-step host work or H2D copy. CPU: host
    # float tensors (the reference's item format).
    ds = build_dataset(cfg)
    train_set, val_set = split_dataset(ds, cfg.validation_split, cfg.seed)
    size = (cfg.image_size, cfg.image_size)
    device_data = cfg.device_data and dev.type == "cuda" and hasattr(ds, "raw_arrays")
    if device_data:
        from ..data.device_data import build_device_dataset
        xtr, ytr = build_device_dataset(ds, train_set.indices, dev, size)
        xva, yva = build_device_dataset(ds, val_set.indices, dev, size) if len(val_set) else (None, None)
    else:
        xtr, ytr = preload(ds, train_set.indices)
        xva, yva = preload(ds, val_set.indices) if len(val_set) else (None, None)
    log.info("Dataset: %d training, %d validation samples (%s)", len(train_set), len(val_set),
             "device-resident u8" if device_data else "host")
    sampler = DistributedShardSampler(len(train_set), rank, world, shuffle=True, seed=cfg.seed)

    # gradient clipping / learning-rate schedule (off by default: nothing below changes then). The schedule
    # spans the whole run: epochs x this rank's steps per epoch, the same total when the run is resumed.
    steps_per_epoch = (len(sampler) + cfg.batch_size - 1) // cfg.batch_size
    options = OptimOptions(cfg.clip_grad_norm, cfg.lr_schedule, cfg.warmup_steps, cfg.epochs * steps_per_epoch,
                           cfg.min_lr_ratio)
    if not options.enabled:
        options = None
    elif is_main:
        mlstore.log_params({"clip_grad_norm": options.clip_grad_norm, "lr_schedule": options.lr_schedule,
                            "warmup_steps": options.warmup_steps, "min_lr_ratio": options.min_lr_ratio,
                            "total_steps": options.total_steps})

    # ---- model / engine ----
    ref = UNetRef(3, K, bilinear=cfg.bilinear, depth=cfg.model_depth)
    if backend == "native":
        from ..models.unet import UNetNative
        model = UNetNative(3, K, bilinear=cfg.bilinear, depth=cfg.model_depth, device=dev, init_from=ref)
        runner = _NativeRunner(model, cfg, options)
    else:
        model = ref.to(dev)
        if cfg.sync_bn and dev.type == "cuda" and dist_info()[1] > 1:  # torch's SyncBatchNorm is GPU-only
            model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        runner = _EagerRunner(model, cfg, dev, options)

    # validation metrics (off by default: nothing below changes then): the epoch's confusion counts, added
    # up on the device by seg_confusion after each eval forward (native) or by the torch reference (eager)
    confusion, best_miou = None, None
    if cfg.val_metrics:
        from .metrics import (ConfusionAccumulator, confusion_matrix, metric_items, metrics_from_confusion,
                              threshold_logit)
        confusion = ConfusionAccumulator(K, threshold_logit(cfg.mask_threshold), device=dev, native=backend == "native")

    start_epoch, best_val = 0, float("inf")
    ckpt_last = os.path.join(cfg.model_output_dir, "last_checkpoint.pt")
    best_path = os.path.join(cfg.model_output_dir, "best_segmentation_model.pth")
    if resume:
        state = torch.load(resume if resume != "auto" else ckpt_last, map_location="cpu", weights_only=True)
        model.load_state_dict(state["model"])
        runner.load_optimizer_state(state["optimizer"])
        start_epoch, best_val = int(state["epoch"]) + 1, float(state["best_val"])
        best_miou = state.get("best_val_miou")
        torch.set_rng_state(state["rng_cpu"])
        log.info("Resumed from epoch %d (best val %.4f)", start_epoch, best_val)

    # augmentation (off by default: nothing below changes a step then). Native backend on device-resident
    # data: the fused gather kernel; any other path: the plain-torch reference on the float batch.
    aug_spec, fused_aug = None, False
    if cfg.augment:
        from ..data.augment import (AugmentSpec, augment_batch_reference, device_order, draw_params,
                                    epoch_generator)
        aug_spec = AugmentSpec.from_config(cfg)
        fused_aug = backend == "native" and device_data

    history = []
    from ..utils.launch import maybe_crash
    for epoch in range(start_epoch, cfg.epochs):
        maybe_crash(epoch, rank)
        t0 = time.time()
        sampler.set_epoch(epoch)
        order = torch.tensor(list(iter(sampler)), dtype=torch.long)
        tl = torch.zeros((), device=dev)
        nb = 0
        if aug_spec is not None:
            # one transform per sample of this rank's order, from a generator that is a function of
            # (seed, epoch, rank) alone: a resumed run draws the same epoch again
            params = draw_params(aug_spec, len(order), cfg.image_size, cfg.image_size,
                                 epoch_generator(cfg.seed, epoch, rank))
        if aug_spec is not None and fused_aug:
            # order and transforms go up once per epoch; each step hands views of them to the one kernel
            # that gathers, warps and writes the executor's input and target (no per-step H2D copy)
            idx_dev, params_dev = device_order(order, len(xtr), dev), params.to(dev)
            for i in range(0, len(order), cfg.batch_size):
                sl = slice(i, i + cfg.batch_size)
                tl += runner.train_step_resident(xtr, ytr, idx_dev[sl], params_dev[sl]).float()
                nb += 1
        elif aug_spec is not None:
            for xb, yb in _batches(xtr, ytr, order, cfg.batch_size, dev, K):
                xb, yb = augment_batch_reference(xb, yb, params[nb * cfg.batch_size:(nb + 1) * cfg.batch_size],
                                                 n_classes=K)
                tl += runner.train_step(xb, yb).float()
                nb += 1
        else:
            for xb, yb in _batches(xtr, ytr, order, cfg.batch_size, dev, K):
                tl += runner.train_step(xb, yb).float()
                nb += 1
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t_train = time.time() - t0
        if world > 1:
            stats = torch.stack([tl, torch.tensor(float(nb), device=dev)])
            dist.all_reduce(stats)
            tl, nb = stats[0], int(stats[1].item())
        avg_train = float(tl.item()) / max(nb, 1)
        vl, nv = torch.zeros((), device=dev), 0
        if xva is not None and len(xva):
            if confusion is not None:
                confusion.reset()
            for xb, yb in _batches(xva, yva, torch.arange(len(xva)), cfg.batch_size, dev, K):
                vl += (runner.eval_loss(xb, yb, confusion) if confusion is not None
                       else runner.eval_loss(xb, yb)).float()
                nv += 1
        avg_val = float(vl.item()) / max(nv, 1) if nv else avg_train
        vm = None
        if confusion is not None and nv:
            # every rank validates the WHOLE validation set, so the counts are equal on all ranks: no
            # collective is needed, and rank 0 logs its own
            counts = confusion.result()  # the epoch's one read-back of the counts
            vm = metrics_from_confusion(counts, K)
        dt = time.time() - t0
        history.append({"epoch": epoch, "train_loss": avg_train, "val_loss": avg_val, "epoch_s": dt,
                        "train_s": t_train, "train_imgs_per_s": len(order) * world / max(t_train, 1e-9)})
        if vm is not None:
            history[-1].update(val_metrics=vm, val_confusion=confusion_matrix(counts, K))
        if options is not None and nb:
            # the epoch's last step: the rate it used and (clipping on) its pre-clip gradient norm
            lr_last, gnorm_last = runner.last_optim()
            history[-1]["lr"] = lr_last
            if gnorm_last is not None:
                history[-1]["grad_norm"] = gnorm_last
            if is_main:
                mlstore.log_metric("lr", lr_last, step=epoch)
                if gnorm_last is not None:
                    mlstore.log_metric("grad_norm", gnorm_last, step=epoch)
        if is_main:
            mlstore.log_metric("train_loss", avg_train, step=epoch)
            mlstore.log_metric("val_loss", avg_val, step=epoch)
            mlstore.log_metric("epoch_time_s", dt, step=epoch)
            mlstore.log_metric("train_imgs_per_s", len(order) * world / max(t_train, 1e-9), step=epoch)
            log.info("Epoch %d/%d: train %.4f val %.4f (%.1fs)", epoch + 1, cfg.epochs, avg_train, avg_val, dt)
            if vm is not None:
                for name, value in metric_items(vm, K):
                    mlstore.log_metric(name, value, step=epoch)
                log.info("Epoch %d/%d: val mIoU %.4f mDice %.4f pixel acc %.4f", epoch + 1, cfg.epochs, vm["miou"],
                         vm["mdice"], vm["pixel_acc"])
            if avg_val < best_val:
                if vm is not None:
                    best_miou = vm["miou"]  # the value at the best-LOSS epoch: selection stays by val loss
                best_val = avg_val
                torch.save({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}, best_path)
                log.info("New best model at epoch %d: val %.4f", epoch + 1, best_val)
            ckpt = {"model": {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
                    "optimizer": _to_cpu(runner.optimizer_state()), "epoch": epoch, "best_val": best_val,
                    "rng_cpu": torch.get_rng_state()}
            if best_miou is not None:
                ckpt["best_val_miou"] = float(best_miou)
            torch.save(ckpt, ckpt_last)
        if world > 1:
            dist.barrier()

    result = {"history": history, "best_val_loss": best_val, "backend": backend}
    if is_main:
        mlstore.log_metric("best_val_loss", best_val)
        if confusion is not None and best_miou is not None:
            mlstore.log_metric("best_val_miou", float(best_miou))
            result["best_val_miou"] = float(best_miou)
        if os.path.exists(best_path):
            model.load_state_dict(torch.load(best_path, map_location="cpu", weights_only=True))
        info = mlstore.pytorch.log_model(model, name="model", registered_model_name=cfg.registered_model_name)
        log.info("Model '%s' registered with version %s", cfg.registered_model_name, info.registered_model_version)
        result.update(run_id=info.run_id, registered_version=info.registered_model_version)
        if os.path.exists(best_path):
            os.remove(best_path)  # reference removes the temporary checkpoint (:210)
        mlstore.end_run()
    if world > 1:
        dist.barrier()
    return result


def _to_cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj
