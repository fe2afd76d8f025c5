#!/usr/bin/env python
"""Batch preparation of a training step: the fused gather + augmentation kernel against the plain path.

Per batch size at one image size, on one GPU:
  * ``fused``: ``UNetExecutor.set_input_resident`` (one ``batch_augment`` launch) with random transforms
    and with identity rows;
  * ``plain``: what ``train_model`` does without augmentation -- two ``index_select``s of the resident u8
    tensors, ``batch_to_float`` and ``UNetExecutor.set_input`` (seven torch launches);
  * ``train_model`` img/s with ``augment`` off and on (native backend, device-resident data), the median
    of the per-epoch training rates after the warm-up epochs.

Timing: device events around ``--reps`` back-to-back calls after a warm-up, the variants interleaved over
``--rounds`` rounds in one process (same clocks, same neighbours). The event window holds what the GPU
spends per batch when the host stays ahead of it; the host's own cost per call is reported beside it
(host clock around the enqueue, before the synchronise).

Usage: python scripts/augment_bench.py [--size 256] [--batches 4,64] [--out profiles/batch_augment.md]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    """(device us per call, host enqueue us per call) of ``reps`` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps


def prep_bench(bs, size, samples, reps, rounds, dev, only=None):
    from robotic_discovery_platform_amd.data.augment import (AugmentSpec, device_order, draw_params, epoch_generator,
                                                             identity_params)
    from robotic_discovery_platform_amd.data.device_data import batch_to_float
    from robotic_discovery_platform_amd.models.unet import UNetNative
    g = torch.Generator().manual_seed(0)
    x_res = torch.randint(0, 256, (samples, size, size, 3), generator=g, dtype=torch.uint8).to(dev)
    y_res = (torch.randint(0, 2, (samples, size, size), generator=g, dtype=torch.uint8) * 255).to(dev)
    ex = UNetNative(3, 1, device=dev).executor(bs, size, size)
    order = torch.randperm(samples, generator=g)[:bs]
    idx = device_order(order, samples, dev)
    idx_long = order.to(dev)
    spec = AugmentSpec(hflip=0.5, rotate_deg=15.0, scale=0.1, translate=0.05, contrast=0.1, brightness=0.1)
    p_aug = draw_params(spec, bs, size, size, epoch_generator(0, 0, 0)).to(dev)
    p_id = identity_params(bs, dev)

    def plain():
        xb, yb = batch_to_float(x_res.index_select(0, idx_long), y_res.index_select(0, idx_long))
        ex.set_input(xb, yb)

    variants = {"plain": plain,
                "fused_identity": lambda: ex.set_input_resident(x_res, y_res, idx, p_id),
                "fused_augment": lambda: ex.set_input_resident(x_res, y_res, idx, p_aug)}
    variants = {k: v for k, v in variants.items() if only is None or k in only}
    out = {k: {"device_us": [], "host_us": []} for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            d, h = timed(fn, reps, warmup=10)
            out[name]["device_us"].append(d)
            out[name]["host_us"].append(h)
    # the bytes the fused pass must move: x_in + target written, the u8 sources read once
    px = bs * size * size
    out["bytes_min"] = px * (16 + 4 + 3 + 1)
    return out


def train_bench(bs, size, data_dir, epochs, rounds, warm_epochs):
    from robotic_discovery_platform_amd.config import TrainConfig
    from robotic_discovery_platform_amd.train.trainer import train_model
    res = {"off": [], "on": []}
    for r in range(rounds):
        for mode in ("off", "on"):
            with tempfile.TemporaryDirectory() as tmp:
                cfg = TrainConfig(batch_size=bs, image_size=size, epochs=epochs, backend="native", dataset_dir=data_dir,
                                  validation_split=0.04, augment=mode == "on", mlruns_dir=os.path.join(tmp, "mlruns"),
                                  model_output_dir=os.path.join(tmp, "models"))
                hist = train_model(cfg)["history"]
            res[mode].append(statistics.median(h["train_imgs_per_s"] for h in hist[warm_epochs:]))
    return res


def fmt_list(v, nd=1):
    return " / ".join(f"{x:.{nd}f}" for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", default="4,64")
    ap.add_argument("--samples", type=int, default=200, help="resident samples (and training scenes)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--variants", default=None, help="comma list of plain,fused_identity,fused_augment (a kernel "
                    "trace of one variant: rocprofv3 --kernel-trace --stats -- python scripts/augment_bench.py ...)")
    ap.add_argument("--out", default=None, help="write the markdown table here (default: stdout only)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py measures on a GPU; none is visible")
    import logging
    logging.disable(logging.INFO)
    dev = torch.device("cuda", 0)
    batches = [int(b) for b in a.batches.split(",")]
    only = a.variants.split(",") if a.variants else None
    result = {"size": a.size, "device": torch.cuda.get_device_name(0), "prep": {}, "train": {}}
    for bs in batches:
        result["prep"][bs] = prep_bench(bs, a.size, a.samples, a.reps, a.rounds, dev, only)
        print(json.dumps({"bs": bs, "prep": result["prep"][bs]}), flush=True)
    if not a.skip_train:
        from robotic_discovery_platform_amd.data.synthetic import write_dataset
        with tempfile.TemporaryDirectory() as data:
            write_dataset(data, a.samples, seed=0)
            for bs in batches:
                steps = max(1, int(a.samples * 0.96) // bs)
                epochs = max(6, 2 + 120 // steps)  # >= ~120 timed steps after the two warm-up epochs
                result["train"][bs] = train_bench(bs, a.size, data, epochs, a.train_rounds, warm_epochs=2)
                print(json.dumps({"bs": bs, "train": result["train"][bs]}), flush=True)
    lines = [f"Image size {a.size} x {a.size}, {a.samples} resident samples, {result['device']}; device events around "
             f"{a.reps} back-to-back calls, {a.rounds} interleaved rounds (values per round).", "",
             "| batch | variant | device us / batch | host us / batch | GB/s of the minimum bytes |", "|---|---|---|---|---|"]
    for bs in batches:
        p = result["prep"][bs]
        for name in (n for n in ("plain", "fused_identity", "fused_augment") if n in p):
            best = min(p[name]["device_us"])
            lines.append(f"| {bs} | {name} | {fmt_list(p[name]['device_us'])} | {fmt_list(p[name]['host_us'])} | "
                         f"{p['bytes_min'] / best / 1e3:.0f} |")
    if result["train"]:
        lines += ["", "`train_model` (native backend, device-resident data), median per-epoch training img/s after two "
                  "warm-up epochs, runs interleaved off / on:", "", "| batch | augment off | augment on |", "|---|---|---|"]
        for bs in batches:
            t = result["train"][bs]
            lines.append(f"| {bs} | {fmt_list(t['off'], 0)} | {fmt_list(t['on'], 0)} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
