"""bench.py's multi-rank contract, end to end: torch.distributed.run launches 2 ranks (sharing the one
GPU of the test box over gloo; the driver's real N-GPU runs use RCCL), rank 0 prints ONE JSON line
whose value aggregates both ranks. Also exercises --sync-bn through the launcher."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("sync_bn", [0, 1])
def test_bench_two_ranks_json_contract(sync_bn):
    env = dict(os.environ, RDP_DIST_BACKEND="gloo", RDP_NO_BUILD="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
           "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--sync-bn", str(sync_bn)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    assert d["config"]["sync_bn"] is bool(sync_bn)
    assert d["value"] > 0 and abs(d["value"] - 4 * 1000.0 / d["ms_per_step"]) / d["value"] < 0.02
    # the collective self-check and per-rank spread (parallel/selfcheck.py)
    assert d["dist_backend"] == "gloo" and d["world_size"] == 2 and d["comm_probe"].startswith("ok")
    assert d["allreduce_busbw_gbps"] > 0 and d["rank_ms_per_step_min"] <= d["rank_ms_per_step_max"]


def test_plain_bench_gpus2_self_launches():
    """The driver's form ``python bench.py --gpus N`` (no launcher): bench.py starts the N ranks
    itself, from a parent that never touches the GPU (native implementation, gloo sharing one GPU)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RDP_DIST_BACKEND="gloo", RDP_NO_BUILD="1")
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2",
           "--size", "64"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    assert d["config"]["impl"] == "native"


def test_plain_native_run_is_lean_and_dumps_outputs(tmp_path):
    """``python bench.py --gpus 1 --steps K --warmup W``: the headline step only (none of the ``--full``
    measurements in the line), K timed steps, and with ``--dump-outputs`` the native step's loss, logits,
    updated parameters and gradients as float32 arrays."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RDP_NO_BUILD="1")
    out = str(tmp_path / "dump")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
           "--size", "64", "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["steps"] == 3 and d["config"]["impl"] == "native" and d["dtype"] == "bf16"
    assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) / d["value"] < 0.02
    assert not any(k.startswith(("ref_batch", "transposed", "train_model", "serve")) for k in d)
    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(arrays) == ["grads", "logits", "loss", "params"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert arrays["logits"].shape == (2, 1, 64, 64) and arrays["logits"].std() > 0
    assert arrays["params"].shape == arrays["grads"].shape and np.abs(arrays["grads"]).sum() > 0
    assert 0 < arrays["loss"][0] < 10
    # BCE of the dumped logits against the seeded targets of the step is the dumped loss
    import torch
    g = torch.Generator(device="cpu").manual_seed(1234)
    torch.rand(2, 3, 64, 64, generator=g)
    y = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(arrays["logits"]), y)
    # (fp32 sum of 8,192 terms of ~0.7: worst case 8192 x 2^-24 x 0.7 = 3.4e-4 on the mean)
    assert abs(float(bce) - float(arrays["loss"][0])) < 5e-4


@pytest.mark.parametrize("fail", [0, 1])
def test_bench_ddp_force_world1_native_selfcheck(fail):
    """World 1 under nccl with the DDP path forced: the self-check runs the native ncclAllReduce probe
    (RCCL reports 1 rank) -- and with RDP_COMM_PROBE_FAIL=1 the run falls back to torch.distributed
    issue, says why in the JSON, still prints its line and exits 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RDP_NO_BUILD="1", RDP_COMM_PROBE_FAIL=str(fail))
    cmd = [sys.executable, "bench.py", "--ddp-force", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
           "--size", "64", "--extras", "0", "--serve", "0"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["dist_backend"] == "nccl" and d["rccl_ranks"] == 1 and d["world_size"] == 1
    if fail:
        assert d["ddp_comm"].startswith("torch (native probe failed: ") and d["config"]["ddp_stream"] is None
    else:
        assert d["ddp_comm"] == "native" and d["comm_probe"] == "ok" and d["config"]["ddp_stream"] == "side"
