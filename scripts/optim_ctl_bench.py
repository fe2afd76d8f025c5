#!/usr/bin/env python
"""Cost of gradient clipping and the learning-rate schedule inside the native training step.

On one GPU, in one process, variants interleaved over ``--rounds`` rounds (same clocks, same neighbours):
  * ``grad_sqnorm`` alone at the flagship model's ``store.numel`` (depth-4 bilinear U-Net), fp32 and bf16
    gradients: device time per launch and GB/s of the bytes it must read (4 n / 2 n), against the copy rate
    scripts/write_bw.py recorded (5.2 TB/s). ``cold`` rotates over enough gradient buffers to exceed the
    256 MiB Infinity Cache, so every launch reads from HBM; ``warm`` re-reads one buffer (what the step sees
    when the weight gradients were just written and still sit in the cache);
  * ``optim_ctl`` alone (one block) with the norm pass's full 2048 partials;
  * the training step (256 x 256, plan mode as ``bench.py`` runs it) at each batch size with the options
    off, a schedule only (warmup + cosine: ``optim_ctl`` + ``adam_ctl``) and clipping + schedule (+ the norm pass).

Timing: device events around back-to-back calls after a warm-up; the step's window also ends in a
synchronise, so it holds the GPU's time per step when the host stays ahead and the host's when it does not.

Usage: python scripts/optim_ctl_bench.py [--batches 4,64] [--steps 200] [--rounds 3] [--out profiles/optim_ctl.md]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_RATE_TBS = 5.2  # scripts/write_bw.py (README): the device copy rate the byte floors are taken at
L3_BYTES = 256 << 20


def timed(fn, reps, warmup):
    """(device us per call, host enqueue us per call) of ``reps`` back-to-back calls. Where the two agree
    the window is host-bound: it shows what the host spends to issue the launch, an upper bound on the kernel."""
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


def kernel_bench(C, n, reps, rounds, dev):
    blocks = C.grad_sqnorm_blocks(n)
    partial = torch.zeros(blocks, dtype=torch.float64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    ctl = torch.zeros(4, device=dev)
    variants, nbytes = {}, {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        es = torch.empty((), dtype=dt).element_size()
        copies = 2 * L3_BYTES // (n * es) + 1
        bufs = [torch.randn(n, device=dev).to(dt) for _ in range(copies)]
        state = {"i": 0}

        def cold(bufs=bufs, state=state):
            state["i"] = (state["i"] + 1) % len(bufs)
            C.grad_sqnorm(bufs[state["i"]], partial)

        variants[f"grad_sqnorm {name} cold"] = cold
        variants[f"grad_sqnorm {name} warm"] = lambda g=bufs[0]: C.grad_sqnorm(g, partial)
        nbytes[f"grad_sqnorm {name} cold"] = nbytes[f"grad_sqnorm {name} warm"] = n * es
    variants["optim_ctl"] = lambda: C.optim_ctl(partial, blocks, 1.0, 1.0, 1, 100, 10000, 0.01, step, ctl)
    out, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            d, h = timed(fn, reps, warmup=20)
            out[k].append(d)
            host[k].append(h)
    return {"n": n, "blocks": blocks, "us": out, "host_us": host, "bytes": nbytes}


def step_bench(bs, size, steps, rounds, dev):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    opts = {"off": {},
            "schedule": dict(lr_schedule="cosine", warmup_steps=100, total_steps=1_000_000, min_lr_ratio=0.01),
            "clip+schedule": dict(clip_grad_norm=1.0, lr_schedule="cosine", warmup_steps=100, total_steps=1_000_000,
                                  min_lr_ratio=0.01)}
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.rand(bs, 3, size, size, generator=g).to(dev)
    y = (torch.rand(bs, 1, size, size, generator=g) > 0.5).float().to(dev)
    trainers = {}
    for name, kw in opts.items():
        torch.manual_seed(0)
        model = UNetNative(3, 1, device=dev, init_from=UNetRef(3, 1))
        tr = NativeTrainer(model, bs, size, size, **kw)
        tr.set_batch(x, y)
        trainers[name] = tr
    out = {k: [] for k in trainers}
    for _ in range(rounds):
        for name, tr in trainers.items():
            out[name].append(timed(tr.step, steps, warmup=10)[0] / 1e3)  # ms per step
    info = {name: tr.opt.last_ctl() for name, tr in trainers.items()}
    return {"ms": out, "ctl": info, "plan": {k: tr.plan_id is not None for k, tr in trainers.items()}}


def fmt(v, nd):
    return " / ".join(f"{x:.{nd}f}" for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", default="4,64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true", help="only the stand-alone launches")
    ap.add_argument("--out", default=None, help="write the markdown tables here (default: stdout only)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_ctl_bench.py measures on a GPU; none is visible")
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.ops import native
    C = native()
    dev = torch.device("cuda", 0)
    n = UNetNative(3, 1, device=dev).store.numel
    result = {"device": torch.cuda.get_device_name(0), "size": a.size, "kernels": kernel_bench(C, n, a.reps, a.rounds, dev),
              "steps": {}}
    print(json.dumps(result["kernels"]), flush=True)
    for bs in [] if a.skip_steps else [int(b) for b in a.batches.split(",")]:
        steps = a.steps if bs <= 16 else max(20, a.steps // 4)
        result["steps"][bs] = step_bench(bs, a.size, steps, a.rounds, dev)
        print(json.dumps({"bs": bs, **result["steps"][bs]}), flush=True)
    k = result["kernels"]
    lines = [f"{result['device']}; store.numel = {k['n']:,} ({k['blocks']} blocks of 256 threads); device events around "
             f"{a.reps} back-to-back launches, {a.rounds} interleaved rounds (values per round).", "",
             f"| launch | event window, us | host enqueue, us | bytes read | best GB/s | floor at {COPY_RATE_TBS} TB/s (us) |",
             "|---|---|---|---|---|---|"]
    for name, us in k["us"].items():
        b, h = k["bytes"].get(name), fmt(k["host_us"][name], 2)
        if b is None:
            lines.append(f"| {name} | {fmt(us, 2)} | {h} | - | - | - |")
        else:
            lines.append(f"| {name} | {fmt(us, 2)} | {h} | {b:,} | {b / min(us) / 1e3:.0f} | "
                         f"{b / COPY_RATE_TBS / 1e6:.2f} |")
    if result["steps"]:
        lines += ["", f"Training step, {a.size} x {a.size}, plan mode, ms per step (values per round, variants interleaved):", "",
                  "| batch | off | schedule | clip + schedule |", "|---|---|---|---|"]
    for bs, s in result["steps"].items():
        lines.append(f"| {bs} | {fmt(s['ms']['off'], 3)} | {fmt(s['ms']['schedule'], 3)} | "
                     f"{fmt(s['ms']['clip+schedule'], 3)} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
