#!/usr/bin/env python
"""The validation-metric pass: ``seg_confusion`` against torch on the device and against its byte floor.

At one image size and batch (default 256^2, batch 64: M = 4.19 M pixels), for K = 1, 3 and 8, on two
label maps -- ``background`` (99 % of the pixels are class 0 predicted as class 0: what a segmentation
map looks like, 1-2 distinct bins per wave) and ``random`` (uniform labels and random logits: many bins
per wave) -- the confusion counts are formed by

  * ``kernel``: ``seg_confusion`` (csrc/seg_metrics.hip);
  * ``torch``: the same counts from torch ops on the device (``argmax`` / compare, bin index,
    ``bincount``), checked equal to the kernel's before timing.

``floor`` is the pass's bytes, M * (4 K + 1) (K = 1: 8 M, its target is fp32), at the copy rate
``scripts/write_bw.py`` records (``--copy-tbs``, default 5.2 TB/s).

Then ``train_model`` (native backend, device-resident synthetic data) with ``val_metrics`` off and on,
alternating, for K = 1 and 3: the median epoch time after the warm-up epochs.

Timing: device events, the paths interleaved over ``--rounds`` rounds in one process. The kernel is
timed as ``--reps`` launches captured into one graph and replayed (its device time: eager back-to-back
calls of a 10-30 us kernel time the host's enqueue instead); torch's ``bincount`` synchronises, so the
torch path is ``--reps`` eager back-to-back calls.

Usage: python scripts/seg_metrics_bench.py [--size 256] [--batch 64] [--out profiles/seg_metrics.md]
"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def timed_graph(fn, reps, replays=5):
    """us per call of ``reps`` launches captured into one graph and replayed: device time without the
    host's per-call enqueue cost (a linear chain on one stream)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    return timed(g.replay, replays, warmup=2) / reps


def make_map(kind, K, M, dev):
    g = torch.Generator().manual_seed(17 * K + len(kind))
    kc = max(K, 2)
    if kind == "random":
        x = torch.randn(M, K, generator=g)
        t = torch.randint(0, kc, (M,), generator=g)
    else:
        t = (torch.rand(M, generator=g) < 0.005).long() * torch.randint(1, kc, (M,), generator=g)
        x = torch.full((M, K), -2.0)
        if K > 1:
            x[:, 0] = 2.0
        flip = torch.rand(M, generator=g) < 0.005
        x[flip, K - 1] = 3.0
    target = t.float() if K == 1 else t.to(torch.uint8)
    return x.reshape(-1).contiguous().to(dev), target.to(dev)


def torch_counts(x, t, K):
    kc = max(K, 2)
    if K == 1:
        idx = (t > 0.5).long() * 2 + (x > 0.0).long()
    else:
        tl = t.long()
        idx = torch.where(tl < K, tl * K + x.view(-1, K).argmax(1), torch.full_like(tl, kc * kc))
    return torch.bincount(idx, minlength=kc * kc + 1)


def kernel_bench(args, dev, lines):
    from robotic_discovery_platform_amd.ops import native
    from robotic_discovery_platform_amd.train.metrics import confusion_size
    C = native()
    M = args.batch * args.size * args.size
    lines += [f"## Counts of one batch: {args.batch} x {args.size}^2 (M = {M:,} pixels)", "",
              "| K | map | path | us (median) | us (min..max) | GB/s of the floor bytes | x floor |",
              "|---|---|---|---|---|---|---|"]
    for K in (1, 3, 8):
        nbytes = M * (8 if K == 1 else 4 * K + 1)
        floor_us = nbytes / (args.copy_tbs * 1e12) * 1e6
        for kind in ("background", "random"):
            x, t = make_map(kind, K, M, dev)
            counts = torch.zeros(confusion_size(K), dtype=torch.int64, device=dev)
            paths = [("kernel", lambda: C.seg_confusion(x, t, K, counts)), ("torch", lambda: torch_counts(x, t, K))]
            want = torch_counts(x, t, K)
            for name, fn in paths[:-1]:  # equal counts before any timing
                counts.zero_()
                fn()
                assert torch.equal(counts, want), (K, kind, name)
            ts = {name: [] for name, _ in paths}
            for _ in range(args.rounds):
                for name, fn in paths:
                    ts[name].append(timed(fn, args.reps) if name == "torch" else timed_graph(fn, args.reps))
            for name, _ in paths:
                med = statistics.median(ts[name])
                lines.append(f"| {K} | {kind} | {name} | {med:.1f} | {min(ts[name]):.1f}..{max(ts[name]):.1f} | "
                             f"{nbytes / med / 1e3:.0f} | {med / floor_us:.2f} |")
            lines.append(f"| {K} | {kind} | floor ({nbytes / 1e6:.1f} MB at {args.copy_tbs} TB/s) | {floor_us:.1f} "
                         "| | | 1.00 |")
            print("\n".join(lines[-len(paths) - 1:]), flush=True)
    lines.append("")


def train_bench(args, dev, lines):
    from robotic_discovery_platform_amd.config import TrainConfig
    from robotic_discovery_platform_amd.train.trainer import train_model
    lines += [f"## train_model epoch time, val_metrics off / on ({args.train_samples} synthetic scenes at "
              f"{args.size}^2, batch {args.train_batch}, validation split 0.2, native, device-resident)", "",
              "| K | val_metrics | epoch s (median of the epochs after the first two) | per-epoch values |",
              "|---|---|---|---|"]
    for K in (1, 3):
        for on in (False, True, False, True):
            with tempfile.TemporaryDirectory() as tmp:
                cfg = TrainConfig(epochs=args.train_epochs, batch_size=args.train_batch, image_size=args.size,
                                  synthetic_samples=args.train_samples, dataset_dir=os.path.join(tmp, "none"),
                                  mlruns_dir=os.path.join(tmp, "mlruns"), model_output_dir=os.path.join(tmp, "models"),
                                  backend="native", n_classes=K, val_metrics=on)
                hist = train_model(cfg)["history"]
            es = [h["epoch_s"] for h in hist[2:]]
            lines.append(f"| {K} | {'on' if on else 'off'} | {statistics.median(es):.4f} | "
                         f"{' '.join(f'{e:.4f}' for e in es)} |")
            print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, default=5.2, help="copy rate of scripts/write_bw.py, TB/s")
    ap.add_argument("--train-samples", type=int, default=160)
    ap.add_argument("--train-batch", type=int, default=16)
    ap.add_argument("--train-epochs", type=int, default=7)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_metrics_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    lines = ["# seg_confusion: measured", "",
             f"{torch.cuda.get_device_name(0)}; `python scripts/seg_metrics_bench.py`; "
             f"device events, {args.reps} calls per window, {args.rounds} interleaved rounds.", ""]
    kernel_bench(args, dev, lines)
    if not args.skip_train:
        train_bench(args, dev, lines)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
