"""The native DDP step of a K-class model (``loss="ce"``) under a 1-rank ``nccl`` group with the DDP
machinery forced on: it must equal the plain step bit for bit (method of test_ddp_rccl_gpu.py; the
case runs in a spawned child so the process group never leaks into other tests)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

STEPS = 5  # a launch plan is recorded at the third step and replayed from the fourth
K = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(n=4, hw=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, hw, hw, generator=g)
    t = torch.randint(0, K, (n, hw, hw), generator=g)
    t[torch.rand(n, hw, hw, generator=g) < 0.1] = 255
    return x, t


def _model(dev):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(7)
    return UNetNative(3, K, device=dev, init_from=UNetRef(3, K))


def _worker(rank, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", RDP_DDP_COMM="native")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from robotic_discovery_platform_amd.train.engine import NativeTrainer
        nat = _model(dev)
        tr = NativeTrainer(nat, 4, 64, 64, lr=1e-3, loss="ce", graph=False, bucket_mb=4.0, ddp_force=True, plan=True)
        assert tr.ddp and tr.bucketer is not None and tr.use_plan
        x, t = _data()
        tr.set_batch(x.to(dev), t.to(dev))
        grads = []
        for _ in range(STEPS):
            tr.step()
            grads.append(nat.store.grad.clone())
        torch.cuda.synchronize()
        assert tr.plan_id is not None
        torch.save({"flat": nat.store.flat.cpu(), "grads": [g.cpu() for g in grads]}, out)
    finally:
        dist.destroy_process_group()


def test_multiclass_ddp_step_matches_plain_step(tmp_path):
    from robotic_discovery_platform_amd.models.unet import NativeAdam
    out = str(tmp_path / "ddp_ce.pt")
    mp.spawn(_worker, args=(_free_port(), out), nprocs=1, join=True)
    got = torch.load(out, weights_only=True)
    dev = torch.device("cuda", 0)
    nat = _model(dev)
    ex = nat.executor(4, 64, 64, training=True, loss="ce")
    opt = NativeAdam(nat, lr=1e-3)
    x, t = _data()
    ex.set_input(x.to(dev), t.to(dev))
    for i in range(STEPS):
        ex.forward()
        ex.backward()
        assert torch.equal(got["grads"][i], nat.store.grad.cpu()), f"step {i}: grads differ"
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(got["flat"], nat.store.flat.cpu())
