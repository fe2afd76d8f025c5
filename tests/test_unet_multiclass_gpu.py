"""K-class native U-Net (softmax cross-entropy head, csrc/head_multi.hip) vs the plain-torch reference,
with the method and margins of test_unet_native_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.float().reshape(-1), b.float().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-20)).item()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _labels(N, H, W, K, gen=None, ignore=0.1):
    t = torch.randint(0, K, (N, H, W), generator=gen)
    t[torch.rand(N, H, W, generator=gen) < ignore] = 255
    return t


@pytest.mark.parametrize("depth,size", [(2, 64), (4, 96)])
def test_multiclass_forward_backward_matches_reference(depth, size):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(0)
    dev = torch.device("cuda")
    N, K = 2, 3
    ref = UNetRef(3, K, True, 64, depth).to(dev)
    nat = UNetNative(3, K, True, 64, depth, device=dev, init_from=ref)
    x = torch.rand(N, 3, size, size, device=dev)
    t = _labels(N, size, size, K).to(dev)
    xq = x.to(torch.bfloat16).float()  # the reference sees the same bf16-rounded input
    ex = nat.executor(N, size, size, training=True, loss="ce")
    ex.set_input(x, t)
    ex.forward()
    ref.train()
    out = ref(xq)
    loss = F.cross_entropy(out, t, ignore_index=255)
    loss.backward()
    assert ex.logits.numel() == N * size * size * K and ex.logits_nchw().shape == out.shape
    assert _rel(ex.logits_nchw(), out.detach()) < 0.08
    assert abs(ex.loss[0].item() - loss.item()) < 2e-2
    assert ex.loss[1].item() == ex.loss[0].item()
    ex.backward()
    st = nat.store
    # yardstick: torch's own bf16 autocast run of the same step vs the fp32 reference
    ref16 = UNetRef(3, K, True, 64, depth).to(dev)
    ref16.load_state_dict(ref.state_dict())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o16 = ref16(xq)
    F.cross_entropy(o16.float(), t, ignore_index=255).backward()
    p16 = dict(ref16.named_parameters())
    report = []
    for name, p in ref.named_parameters():
        g = st.view(name, st.grad)
        report.append((name, round(_cos(g, p.grad), 4), round(_cos(p16[name].grad, p.grad), 4)))
    print("\n".join(map(str, report)))
    names = [r[0] for r in report]
    assert "outc.conv.weight" in names and "outc.conv.bias" in names
    mean_c = sum(r[1] for r in report) / len(report)
    mean_c16 = sum(r[2] for r in report) / len(report)
    assert mean_c > mean_c16 - 0.02, (mean_c, mean_c16)
    for name, c, c16 in report:
        assert c > min(0.97, c16 - 0.1), (name, c, c16)


def test_multiclass_state_dict_roundtrip():
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    ref = UNetRef(3, 3)
    nat = UNetNative(3, 3, device=torch.device("cuda"), init_from=ref)
    sd = nat.state_dict()
    assert list(sd.keys()) == list(ref.state_dict().keys())
    for k, v in ref.state_dict().items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    assert sd["outc.conv.weight"].shape == (3, 64, 1, 1)


def test_multiclass_training_reduces_loss_and_graph_replay_matches():
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    torch.manual_seed(0)
    dev = torch.device("cuda")
    ref = UNetRef(3, 3)
    x = torch.rand(4, 3, 64, 64, device=dev)
    yy, xx = torch.meshgrid(torch.arange(64, device=dev), torch.arange(64, device=dev), indexing="ij")
    r2 = (yy - 32) ** 2 + (xx - 32) ** 2
    lab = torch.zeros(64, 64, dtype=torch.int64, device=dev)  # 0: background
    lab[r2 < 150] = 1  # disc
    lab[(r2 >= 300) & (r2 < 600)] = 2  # ring
    t = lab.expand(4, 64, 64).contiguous()
    x[:, 0] += (t == 1) * 0.5
    x[:, 1] += (t == 2) * 0.5
    losses = {}
    for graph in (False, True):
        nat = UNetNative(3, 3, device=dev, init_from=ref)
        tr = NativeTrainer(nat, 4, 64, 64, lr=1e-3, loss="ce", graph=graph)
        tr.set_batch(x, t)
        ls = [tr.step()[0].item() for _ in range(12)]
        losses[graph] = ls
        assert ls[-1] < ls[0] * 0.8, ls
    assert max(abs(a - b) for a, b in zip(losses[False], losses[True])) < 1e-3
    # eval-mode loss of the trained model through the trainer (K-class eval executor)
    assert torch.isfinite(tr.eval_loss()[0]).item()


@pytest.mark.parametrize("bilinear", [True, False])
def test_multiclass_plan_replay_bitwise_equals_eager(bilinear):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    torch.manual_seed(3)
    dev = torch.device("cuda")
    ref = UNetRef(3, 3, bilinear=bilinear)
    g = torch.Generator(device="cpu").manual_seed(5)
    batches = [(torch.rand(2, 3, 64, 96, generator=g), _labels(2, 64, 96, 3, g)) for _ in range(7)]
    runs = {}
    for mode in ("eager", "plan"):
        plan = mode != "eager"
        nat = UNetNative(3, 3, bilinear=bilinear, device=dev, init_from=ref)
        tr = NativeTrainer(nat, 2, 64, 96, lr=1e-3, loss="ce", plan=plan)
        assert tr.use_plan == plan
        ls = []
        for x, y in batches:
            tr.set_batch(x.to(dev), y.to(dev))
            ls.append(tr.step().clone())
        torch.cuda.synchronize()
        if plan:
            assert tr.plan_id is not None
        st = nat.store
        runs[mode] = (torch.stack(ls), st.flat.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(),
                      nat.derived.clone(), [b.clone() for _, b in nat.named_buffers()])
    a, b = runs["eager"], runs["plan"]
    for u, v in zip(a[:5], b[:5]):
        assert torch.equal(u, v)
    for u, v in zip(a[5], b[5]):
        assert torch.equal(u, v)


def test_one_class_step_is_unchanged_and_repeatable():
    """The K = 1 constructor and step after the K-class change: two runs from the same state agree bitwise."""
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    torch.manual_seed(2)
    dev = torch.device("cuda")
    ref = UNetRef(3, 1)
    x = torch.rand(2, 3, 64, 64, device=dev)
    t = (torch.rand(2, 1, 64, 64, device=dev) > 0.5).float()
    runs = []
    for _ in range(2):
        nat = UNetNative(3, 1, device=dev, init_from=ref)
        tr = NativeTrainer(nat, 2, 64, 64, lr=1e-3)
        assert tr.ex.fuse_head and tr.ex.logits.numel() == 2 * 64 * 64
        tr.set_batch(x, t)
        loss = tr.step().clone()
        torch.cuda.synchronize()
        runs.append((loss, nat.store.flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_multiclass_errors():
    from robotic_discovery_platform_amd.models.unet import UNetNative
    dev = torch.device("cuda")
    with pytest.raises(NotImplementedError):
        UNetNative(3, 9, device=dev)
    nat3 = UNetNative(3, 3, depth=2, device=dev)
    with pytest.raises(ValueError):
        nat3.executor(1, 32, 32, training=True, loss="bce")
    nat1 = UNetNative(3, 1, depth=2, device=dev)
    with pytest.raises(ValueError):
        nat1.executor(1, 32, 32, training=True, loss="ce")
