"""bench.py's ``--gpus N`` contract without a launcher (CPU, gloo): a plain ``python bench.py --gpus 2``
must start two ranks itself and report ``n_gpus == 2`` / ``dp2``; a launcher whose WORLD_SIZE
disagrees with ``--gpus`` must fail loudly instead of measuring a different job. The eager
implementation is used so the test needs no GPU; the GPU variant of the same check is in
``tests/test_bench_dist_gpu.py``. Reference step per rank: ``scripts/train_segmenter.py:156-165``."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["RDP_NO_BUILD"] = "1"
    # a CPU / gloo run on every machine: with a GPU visible the two ranks would want a device each
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return env


def test_plain_bench_gpus2_launches_two_ranks():
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--impl", "eager", "--steps", "2", "--warmup", "1",
           "--batch", "1", "--size", "32"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 2
    assert d["steps"] == 2 and d["warmup"] == 1
    assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) / d["value"] < 0.02


def test_dump_outputs_written_and_repeatable(tmp_path):
    """``--dump-outputs DIR``: the last timed step's loss / logits / parameters / gradients as float32
    ``.npy`` files, under 64 MB in all, identical from run to run (seeded inputs and weights); a plain
    run reports none of the ``--full`` measurements."""
    import numpy as np
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    procs = [subprocess.Popen([sys.executable, "bench.py", "--gpus", "1", "--impl", "eager", "--steps", "2",
                               "--warmup", "1", "--batch", "1", "--size", "32", "--dump-outputs", d],
                              cwd=ROOT, env=_env(),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for d in dirs]
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    d = json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("{")][0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert not any(k.startswith(("ref_batch", "transposed", "train_model", "serve")) for k in d)
    assert sorted(os.listdir(dirs[0])) == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0])) <= 64e6
    for f in os.listdir(dirs[0]):
        a, b = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), f
    assert np.load(os.path.join(dirs[0], "logits.npy")).shape == (1, 1, 32, 32)
    assert np.abs(np.load(os.path.join(dirs[0], "grads.npy"))).sum() > 0


def test_secondary_measurements_need_full():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--impl", "eager", "--serve", "1"], cwd=ROOT,
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()


def test_world_size_mismatch_fails():
    env = _env()
    env.update(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--impl", "eager"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=3" in r.stderr and not r.stdout.strip()
