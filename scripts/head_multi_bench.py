#!/usr/bin/env python
"""The K-class head's extended mode (class-weighted CE + soft Dice) against its plain mode.

At one image size and batch (default 256^2, batch 64: M = 4.19 M pixels), for K = 3 and 8:

  * ``headk_fwd`` / ``headk_bwd`` (kernel + its finalize) in plain mode and in extended mode
    (``dice_w`` = 1 with class weights 0.5 + 0.75 k), the two interleaved over ``--rounds`` rounds in one
    process; device events around ``--reps`` back-to-back calls, us per call;
  * the ``NativeTrainer`` step (launch plan, random data) with ``loss="ce"`` and with ``loss="ce_dice"`` +
    class weights, the two alternating, ms per step.

There is no threshold on the extended times: the table records them and their ratio to the plain
kernels of the same run.

Usage: python scripts/head_multi_bench.py [--size 256] [--batch 64] [--out FILE]
"""
import argparse
import os
import statistics
import sys

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


def kernel_bench(args, dev, lines):
    from robotic_discovery_platform_amd.ops import native
    C = native()
    N, S = args.batch, args.size
    M = N * S * S
    lines += [f"## Kernels, plain against extended: {N} x {S}^2 (M = {M:,} pixels)", "",
              "| K | call | plain us (median, min..max) | extended us (median, min..max) | extended / plain |",
              "|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(3)
    for K in (3, 8):
        a = torch.randn(N, S, S, 64, generator=g).to(torch.bfloat16).to(dev)
        w = (torch.randn(K * 64, generator=g) * 0.1).to(dev)
        b = (torch.randn(K, generator=g) * 0.1).to(dev)
        lab = torch.randint(0, K, (M,), generator=g)
        lab[torch.rand(M, generator=g) < 0.1] = 255
        lab = lab.to(torch.uint8).to(dev)
        cw = torch.tensor([0.5 + 0.75 * k for k in range(K)], device=dev)
        logits = torch.zeros(M * K, device=dev)
        part = torch.zeros(C.headk_partial_blocks(M) * K * 65, device=dev)
        sums, loss = torch.zeros(2 + 3 * K, device=dev), torch.zeros(2, device=dev)
        da = torch.zeros_like(a)
        gw, gb = torch.zeros(K * 64, device=dev), torch.zeros(K, device=dev)
        ext = dict(class_weights=cw, dice_w=1.0)
        # the backward reads the sums of the forward of its own mode: each forward runs just before it
        calls = {
            ("forward + loss", "plain"): lambda: C.headk_fwd(a, w, b, lab, logits, part, sums, loss),
            ("forward + loss", "ext"): lambda: C.headk_fwd(a, w, b, lab, logits, part, sums, loss, **ext),
            ("backward (da, dW, db)", "plain"): lambda: C.headk_bwd(a, w, logits, lab, sums, da, part, gw, gb, 1.0),
            ("backward (da, dW, db)", "ext"): lambda: C.headk_bwd(a, w, logits, lab, sums, da, part, gw, gb, 1.0,
                                                                  **ext),
        }
        ts = {k: [] for k in calls}
        for _ in range(args.rounds):
            for mode in ("plain", "ext"):
                calls[("forward + loss", mode)]()
                for call in ("forward + loss", "backward (da, dW, db)"):
                    ts[(call, mode)].append(timed(calls[(call, mode)], args.reps))
        for call in ("forward + loss", "backward (da, dW, db)"):
            p, e = ts[(call, "plain")], ts[(call, "ext")]
            mp, me = statistics.median(p), statistics.median(e)
            lines.append(f"| {K} | {call} | {mp:.1f}, {min(p):.1f}..{max(p):.1f} | {me:.1f}, {min(e):.1f}..{max(e):.1f} "
                         f"| {me / mp:.3f} |")
            print(lines[-1], flush=True)
    lines.append("")


def step_bench(args, dev, lines):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    N, S = args.batch, args.size
    lines += [f"## Training step, batch {N} at {S}^2, bilinear decoder", "",
              f"`NativeTrainer` (launch plan), random data, 5 warm-up steps, then {args.step_rounds} rounds of "
              f"{args.steps} timed steps per loss, the losses alternating; ms per step.", "",
              "| model | " + " | ".join(f"round {i + 1}" for i in range(args.step_rounds)) + " |",
              "|---|" + "---|" * args.step_rounds]
    for K in (3, 8):
        torch.manual_seed(0)
        ref = UNetRef(3, K)
        x = torch.rand(N, 3, S, S, device=dev)
        t = torch.randint(0, K, (N, S, S), device=dev)
        cw = tuple(0.5 + 0.75 * k for k in range(K))
        trainers = {}
        for name, kw in (('`loss="ce"`', dict(loss="ce")),
                         ('`loss="ce_dice"`, class weights', dict(loss="ce_dice", dice_weight=1.0, class_weights=cw))):
            tr = NativeTrainer(UNetNative(3, K, device=dev, init_from=ref), N, S, S, graph=False, **kw)
            tr.set_batch(x, t)
            for _ in range(5):
                tr.step()
            trainers[name] = tr
        ts = {name: [] for name in trainers}
        for _ in range(args.step_rounds):
            for name, tr in trainers.items():
                ts[name].append(timed(tr.step, args.steps, warmup=1) / 1e3)
        for name in trainers:
            lines.append(f"| `UNetNative(3, {K})`, {name} | " + " | ".join(f"{v:.3f}" for v in ts[name]) + " |")
            print(lines[-1], flush=True)
        del trainers
        torch.cuda.empty_cache()
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_multi_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    lines = ["# K-class head, extended mode: measured", "",
             f"{torch.cuda.get_device_name(0)}; `python scripts/head_multi_bench.py`; device events, "
             f"{args.reps} calls per window, {args.rounds} interleaved rounds.", ""]
    kernel_bench(args, dev, lines)
    if not args.skip_step:
        step_bench(args, dev, lines)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
