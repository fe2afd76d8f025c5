"""Serving a stock client's frames: the colour frame as ``cv2.imencode('.jpg')`` writes it -- one baseline
scan, q95, 4:2:0, no restart markers -- and the depth frame as a one-stream 16-bit PNG
(the reference's services/vision_analysis/client.py). Measures where such a JPEG's entropy decode should
run: on the host (csrc/jpeg.cpp, one serial loop) or on the GPU in the frame graph (csrc/jpeg_entropy.hip).

  1. host times: the scan front end (rdp_jpeg_scan: headers + de-stuffing, all the host does on the GPU
     path) against the host entropy decode (rdp_jpeg_decode);
  2. the entropy stage alone on the GPU: its five launches captured as a graph, event-timed over replays,
     per subsequence size S, with subsequences and rounds;
  3. the engine: lock-step p50 / p99 (submit_encoded + collect_encoded of one pipeline) and pipelined FPS
     (a double-buffered session), jpeg_entropy = host vs gpu interleaved, ``--rounds`` rounds in one process.

Two frames: the synthetic scene and the same scene with +-40 noise (a scan ~3x as long).
Usage: python scripts/refclient_bench.py [--frames 300] [--rounds 3] [--out results.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robotic_discovery_platform_amd.data.image_io import encode_jpeg, encode_png  # noqa: E402
from robotic_discovery_platform_amd.data.jpeg import decode_coefs, scan_jpeg  # noqa: E402
from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene  # noqa: E402
from robotic_discovery_platform_amd.ops import native  # noqa: E402


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def frames_of(seed=3):
    sc = make_scene(seed)
    rng = np.random.default_rng(seed)
    noisy = np.clip(sc.color.astype(np.int32) + rng.integers(-40, 40, sc.color.shape), 0, 255).astype(np.uint8)
    depth = encode_png(sc.depth)
    return {"scene": (encode_jpeg(sc.color, 95, restart_rows=0), depth),
            "noisy": (encode_jpeg(noisy, 95, restart_rows=0), depth)}


def host_times(C, data, n=200):
    scan, dec = [], []
    for _ in range(n):
        t = time.perf_counter()
        C.jpeg_scan(data, False, 0)
        scan.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        C.jpeg_decode(data, True, False)
        dec.append((time.perf_counter() - t) * 1e3)
    return {"scan_host_p50_ms": round(pct(scan, 50), 4), "decode_host_p50_ms": round(pct(dec, 50), 4)}


def entropy_stage(C, data, S, cap, replays=100):
    """GPU time of the entropy stage alone (graph replays, events), its subsequences and rounds."""
    dev = torch.device("cuda")
    js = scan_jpeg(data)
    want = decode_coefs(data, parallel=False)
    scan = torch.zeros(cap, dtype=torch.uint8, device=dev)
    scan[:js.scan.numel()] = js.scan.to(dev)
    nbits = torch.tensor([js.nbits], dtype=torch.int32, device=dev)
    tables, geo = js.tables.to(dev), js.meta[:32].to(dev)
    coefs = torch.empty(js.blocks * 64, dtype=torch.int16, device=dev)
    work = torch.zeros(C.jpeg_entropy_work_words(cap, S), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        n, rounds = C.jpeg_entropy_gpu(scan, nbits, tables, geo, coefs, work, status, S)
    st.synchronize()
    assert int(status.item()) == 0 and torch.equal(coefs.cpu(), want.coefs), "GPU entropy decode differs"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        C.jpeg_entropy_gpu(scan, nbits, tables, geo, coefs, work, status, S)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    with torch.cuda.stream(st):
        for _ in range(replays + 10):
            e0.record(st)
            g.replay()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    ms = ms[10:]
    return {"S": S, "subsequences": n, "rounds": rounds, "bits": js.nbits,
            "gpu_p50_us": round(pct(ms, 50) * 1e3, 1), "gpu_p99_us": round(pct(ms, 99) * 1e3, 1)}


def lockstep(p, policy, color, depth, frames, warmup=30):
    p.set_jpeg_entropy(policy)
    lat, gpu = [], []
    for i in range(warmup + frames):
        t = time.perf_counter()
        code = p.submit_encoded(color, depth)
        assert code == 0, code
        r = p.collect_encoded()
        if i >= warmup:
            lat.append((time.perf_counter() - t) * 1e3)
            gpu.append(r.gpu_ms if hasattr(r, "gpu_ms") else r.timings["gpu_ms"])
    return {"p50_ms": round(pct(lat, 50), 4), "p99_ms": round(pct(lat, 99), 4), "gpu_p50_ms": round(pct(gpu, 50), 4)}


def pipelined(pool, color, depth, frames, warmup=30):
    s = pool.session()
    for i in range(warmup):
        s.submit_encoded(color, depth, tag=i)
    s.drain()
    t = time.perf_counter()
    for i in range(frames):
        _, code = s.submit_encoded(color, depth, tag=i)
        assert code == 0, code
    s.drain()
    dt = time.perf_counter() - t
    s.close()
    return round(frames / dt, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--train-steps", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from robotic_discovery_platform_amd.serve.bench_serve import prepare_model
    from robotic_discovery_platform_amd.serve.engine import EnginePool, FramePipeline
    C = native()
    dev = torch.device("cuda")
    model, _ = prepare_model(dev, train_steps=a.train_steps)  # a model that segments: the fit stays on the device
    fr = frames_of()
    res = {"frames": {k: {"jpeg_bytes": len(c), "png_bytes": len(d)} for k, (c, d) in fr.items()}}
    for k, (c, _) in fr.items():
        res["frames"][k].update(host_times(C, c))
    cap = ((480 * 640 * 3 // 2 + 1023) // 1024) * 1024  # the pipeline's scan capacity
    res["entropy_stage"] = {k: [entropy_stage(C, c, int(S), cap) for S in a.sizes.split(",")]
                            for k, (c, _) in fr.items()}
    print(json.dumps({"frames": res["frames"], "entropy_stage": res["entropy_stage"]}), flush=True)
    # the subsequence size the engine runs: RDP_SERVE_JPEG_SUBSEQ_BITS if set, else the built-in default
    p = FramePipeline(model, DEFAULT_K, 0.001, graph=True, rgb=True, jpeg=True)
    pools = {pol: EnginePool(model, DEFAULT_K, 0.001, n=2, graph=True, rgb=True, jpeg=True, batch=0, jpeg_entropy=pol)
             for pol in ("host", "gpu")}
    res["engine_S"] = p.subseq_bits or "default"
    res["rounds"] = []
    for r in range(a.rounds):
        row = {}
        for k, (c, d) in fr.items():
            for pol in (("host", "gpu") if r % 2 == 0 else ("gpu", "host")):
                row[f"{k}_{pol}"] = dict(lockstep(p, pol, c, d, a.frames), pipelined_fps=pipelined(pools[pol], c, d, a.frames))
        res["rounds"].append(row)
        print(json.dumps({"round": r, **row}), flush=True)
    wins = {k: all(row[f"{k}_gpu"]["p50_ms"] < row[f"{k}_host"]["p50_ms"] for row in res["rounds"]) for k in fr}
    res["gpu_wins_p50_every_round"] = wins
    print(json.dumps({"gpu_wins_p50_every_round": wins}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
