"""Multi-class plumbing that runs without a GPU: the CPU serving pipeline's class-selected mask, the
eager trainer's softmax cross-entropy loss and the ServeConfig field."""
import numpy as np
import torch
import torch.nn.functional as F


def _model3(bias):
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(0)
    m = UNetRef(3, 3, depth=2).eval()
    with torch.no_grad():
        m.outc.conv.bias.copy_(torch.tensor(bias))
    return m


def test_cpu_pipeline_serves_the_selected_class():
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K
    from robotic_discovery_platform_amd.serve.engine import CpuFramePipeline
    m = _model3([0.0, 0.0, 50.0])  # class 2 wins every pixel
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    depth = np.full((48, 64), 500, np.uint16)
    r2 = CpuFramePipeline(m, DEFAULT_K, 0.001, H=48, W=64, size=32, mask_class=2).process(bgr, depth)
    assert r2.mask.shape == (48, 64) and np.all(r2.mask == 1) and r2.coverage == 100.0
    r1 = CpuFramePipeline(m, DEFAULT_K, 0.001, H=48, W=64, size=32, mask_class=1).process(bgr, depth)
    assert np.all(r1.mask == 0) and r1.coverage == 0.0


def test_cpu_pipeline_rejects_a_class_the_model_lacks():
    import pytest
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K
    from robotic_discovery_platform_amd.serve.engine import CpuFramePipeline
    with pytest.raises(ValueError):
        CpuFramePipeline(_model3([0.0, 0.0, 0.0]), DEFAULT_K, 0.001, H=48, W=64, size=32, mask_class=3)


def test_eager_trainer_cross_entropy_step():
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import EagerTrainer
    torch.manual_seed(1)
    a = UNetRef(3, 3, depth=2)
    b = UNetRef(3, 3, depth=2)
    b.load_state_dict(a.state_dict())
    x = torch.rand(2, 3, 32, 32)
    t = torch.randint(0, 3, (2, 1, 32, 32))
    t[0, 0, :4] = 255  # ignored
    loss = EagerTrainer(a, lr=1e-3, loss="ce").step(x, t)
    opt = torch.optim.Adam(b.parameters(), lr=1e-3)
    ref = F.cross_entropy(b(x), t.long().squeeze(1), ignore_index=255)
    ref.backward()
    opt.step()
    assert abs(loss.item() - ref.item()) < 1e-6
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.allclose(p, q, rtol=0, atol=1e-6), n
    # [N,H,W] labels are the same loss
    assert torch.equal(EagerTrainer(b, loss="ce").compute_loss(b(x), t[:, 0]),
                       EagerTrainer(b, loss="ce").compute_loss(b(x), t))


def test_serve_config_mask_class(monkeypatch):
    from robotic_discovery_platform_amd.config import ServeConfig, apply_env
    assert ServeConfig().mask_class == 1
    monkeypatch.setenv("RDP_SERVE_MASK_CLASS", "2")
    cfg = apply_env(ServeConfig(), "serve")
    assert cfg.mask_class == 2 and isinstance(cfg.mask_class, int)
