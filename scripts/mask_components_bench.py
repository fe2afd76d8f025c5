#!/usr/bin/env python
"""Cost of the mask component filter (csrc/mask_components.hip): profiles/mask_components.md.

  kernel   the launch alone at 256 x 256, n = 1 and 4 frames, on four inputs: a scene's band plus three speckle
           blobs (the realistic case), density-0.41 noise, the serpentine, the 16,384-singleton grid. The kernel
           works in place, so every iteration restores the input first (outside the timed events).
  engine   the frame: FramePipeline GPU p50 and lock-step p50 (serve/bench_serve.py measure_engine, the harness
           behind serve_engine_*), filter off / last in the network graph / first in the geometry graph,
           alternating for --rounds rounds on one box.

Usage: python scripts/mask_components_bench.py [--iters 300] [--frames 1000] [--rounds 3] [--skip-engine]
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _inputs():
    from robotic_discovery_platform_amd.data.image_io import resize_nearest
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    S = 256
    rng = np.random.default_rng(0)
    scene = np.ascontiguousarray(resize_nearest((make_scene(2).mask > 0).astype(np.uint8), (S, S)))
    ys, xs = np.nonzero(scene)
    y0 = 2 if ys.mean() >= S / 2 else S - 24  # speckle in the half away from the actuator
    for k, side in enumerate((15, 6, 3)):
        scene[y0:y0 + side, 8 + 60 * k:8 + 60 * k + side] = 1
    noise = (rng.random((S, S)) < 0.41).astype(np.uint8)
    serp = np.zeros((S, S), np.uint8)
    serp[0::2, :] = 1
    serp[1::4, S - 1] = 1
    serp[3::4, 0] = 1
    single = np.zeros((S, S), np.uint8)
    single[::2, ::2] = 1
    return {"scene+speckle": scene, "noise0.41": noise, "serpentine": serp, "singletons": single}


def _pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def bench_kernel(iters: int):
    from robotic_discovery_platform_amd.ops import native
    C = native()
    dev = torch.device("cuda")
    for name, m in _inputs().items():
        for n in (1, 4):
            src = torch.from_numpy(np.stack([m] * n)).to(dev)
            buf = torch.empty_like(src)
            st = torch.zeros(n, 4, dtype=torch.int32, device=dev)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for it in range(-20, iters):  # 20 warm-up launches
                buf.copy_(src)
                if it >= 0:
                    ev[it][0].record()
                C.mask_components(buf, n, 256, 256, 1, 0, st)
                if it >= 0:
                    ev[it][1].record()
            torch.cuda.synchronize()
            us = [a.elapsed_time(b) * 1e3 for a, b in ev]
            print(json.dumps({"kernel": name, "n": n, "iters": iters, "us_min": round(min(us), 2),
                              "us_p10": round(_pct(us, 10), 2), "us_p50": round(_pct(us, 50), 2),
                              "us_p90": round(_pct(us, 90), 2), "stats": st[0].tolist()}), flush=True)


def bench_engine(frames: int, warmup: int, rounds: int, train_steps: int):
    from robotic_discovery_platform_amd.serve.bench_serve import measure_engine, prepare_model
    dev = torch.device("cuda")
    model, scenes = prepare_model(dev, train_steps=train_steps)
    configs = [("off", {}, "net"), ("largest@net", dict(mask_components="largest"), "net"),
               ("largest@geo", dict(mask_components="largest"), "geo")]
    for r in range(rounds):
        for name, args, at in configs:
            os.environ["RDP_SERVE_MASK_FILTER_AT"] = at
            out = measure_engine(model, scenes, frames=frames, warmup=warmup, pipelined=False, **args)
            print(json.dumps({"engine": name, "round": r, "gpu_p50_ms": out["engine_gpu_p50_ms"],
                              "gpu_p99_ms": out["engine_gpu_p99_ms"], "lockstep_p50_ms": out["engine_p50_ms"],
                              "lockstep_p99_ms": out["engine_p99_ms"], "fps": out["engine_fps"],
                              "ok_frac": out["engine_ok_frac"], "frames": out["engine_frames"]}), flush=True)
    os.environ.pop("RDP_SERVE_MASK_FILTER_AT", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernel:
        bench_kernel(a.iters)
    if not a.skip_engine:
        bench_engine(a.frames, a.warmup, a.rounds, a.train_steps)


if __name__ == "__main__":
    main()
