"""K-class native U-Net trained with ``"ce_dice"`` and class weights: against the plain-torch reference
(``UNetRef`` + ``train/losses.py::ce_dice_reference``), in eager / plan / graph modes, and through
``train_model``. Method and margins of test_unet_multiclass_gpu.py."""
import pytest
import torch

from robotic_discovery_platform_amd import mlstore
from robotic_discovery_platform_amd.config import TrainConfig
from robotic_discovery_platform_amd.train.losses import ce_dice_reference

pytestmark = pytest.mark.gpu

WEIGHTS = (1.0, 4.0, 2.5)
LAM = 1.5


def _cos(a, b):
    a, b = a.float().reshape(-1), b.float().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-20)).item()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def _labels(N, H, W, K, gen=None, ignore=0.1):
    t = torch.randint(0, K, (N, H, W), generator=gen)
    t[torch.rand(N, H, W, generator=gen) < ignore] = 255
    return t


def test_ce_dice_forward_backward_matches_reference():
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(0)
    dev = torch.device("cuda")
    N, K, depth, size = 2, 3, 2, 64
    ref = UNetRef(3, K, True, 64, depth).to(dev)
    nat = UNetNative(3, K, True, 64, depth, device=dev, init_from=ref)
    x = torch.rand(N, 3, size, size, device=dev)
    t = _labels(N, size, size, K).to(dev)
    xq = x.to(torch.bfloat16).float()  # the reference sees the same bf16-rounded input
    ex = nat.executor(N, size, size, training=True, loss="ce_dice", dice_weight=LAM, class_weights=WEIGHTS)
    assert ex.loss_sums.numel() == 2 + 3 * K
    ex.set_input(x, t)
    ex.forward()
    ref.train()
    out = ref(xq)
    loss, ce = ce_dice_reference(out, t, WEIGHTS, LAM)
    loss.backward()
    assert _rel(ex.logits_nchw(), out.detach()) < 0.08
    assert abs(ex.loss[0].item() - loss.item()) < 2e-2
    assert abs(ex.loss[1].item() - ce.item()) < 2e-2
    assert ex.loss[0].item() > ex.loss[1].item()  # the Dice term is there
    ex.backward()
    st = nat.store
    # yardstick: torch's own bf16 autocast run of the same step vs the fp32 reference
    ref16 = UNetRef(3, K, True, 64, depth).to(dev)
    ref16.load_state_dict(ref.state_dict())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o16 = ref16(xq)
    ce_dice_reference(o16.float(), t, WEIGHTS, LAM)[0].backward()
    p16 = dict(ref16.named_parameters())
    report = []
    for name, p in ref.named_parameters():
        g = st.view(name, st.grad)
        report.append((name, round(_cos(g, p.grad), 4), round(_cos(p16[name].grad, p.grad), 4)))
    print("\n".join(map(str, report)))
    mean_c = sum(r[1] for r in report) / len(report)
    mean_c16 = sum(r[2] for r in report) / len(report)
    assert mean_c > mean_c16 - 0.02, (mean_c, mean_c16)
    for name, c, c16 in report:
        assert c > min(0.97, c16 - 0.1), (name, c, c16)


def _run_steps(mode, ref, batches, dev):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    nat = UNetNative(3, 3, depth=2, device=dev, init_from=ref)
    tr = NativeTrainer(nat, 2, 64, 96, lr=1e-3, loss="ce_dice", dice_weight=LAM, class_weights=WEIGHTS,
                       plan=mode == "plan", graph=mode == "graph")
    assert tr.use_plan == (mode == "plan")
    ls = []
    for x, y in batches:
        tr.set_batch(x.to(dev), y.to(dev))
        ls.append(tr.step().clone())
    torch.cuda.synchronize()
    st = nat.store
    return (torch.stack(ls), st.flat.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(), nat.derived.clone(),
            [b.clone() for _, b in nat.named_buffers()])


def test_ce_dice_plan_and_graph_replay_bitwise_equal_eager():
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(3)
    dev = torch.device("cuda")
    ref = UNetRef(3, 3, depth=2)
    g = torch.Generator(device="cpu").manual_seed(5)
    batches = [(torch.rand(2, 3, 64, 96, generator=g), _labels(2, 64, 96, 3, g)) for _ in range(7)]
    runs = {mode: _run_steps(mode, ref, batches, dev) for mode in ("eager", "plan", "graph")}
    a = runs["eager"]
    assert (a[0][:, 0] > a[0][:, 1]).all()  # loss[0] = CE + Dice term, loss[1] = CE
    for mode in ("plan", "graph"):
        b = runs[mode]
        for u, v in zip(a[:5], b[:5]):
            assert torch.equal(u, v), mode
        for u, v in zip(a[5], b[5]):
            assert torch.equal(u, v), mode


def test_ce_dice_training_reduces_loss_and_eval_loss_uses_it():
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
    nat = UNetNative(3, 3, device=dev, init_from=ref)
    tr = NativeTrainer(nat, 4, 64, 64, lr=1e-3, loss="ce_dice", dice_weight=1.0, class_weights=(1, 4, 4), graph=False)
    tr.set_batch(x, t)
    ls = [tr.step()[0].item() for _ in range(12)]
    assert ls[-1] < ls[0] * 0.8, ls
    ev = tr.eval_loss().clone()
    assert torch.isfinite(ev).all().item()
    evx = nat.executor(4, 64, 64, training=False, loss="ce_dice", dice_weight=1.0, class_weights=(1, 4, 4))
    assert evx.loss_kind == "ce_dice" and evx.dice_w == 1.0 and evx.class_weights == (1.0, 4.0, 4.0)
    assert evx.loss.data_ptr() == tr.eval_loss().data_ptr()  # the trainer's eval executor is this one
    # and its value is the reference loss of its own logits
    L, ce = ce_dice_reference(evx.logits_nchw().double(), t, (1, 4, 4), 1.0)
    assert abs(ev[0].item() - L.item()) < 1e-4 and abs(ev[1].item() - ce.item()) < 1e-4
    assert ev[0].item() > ev[1].item()


def test_ce_dice_errors():
    from robotic_discovery_platform_amd.models.unet import UNetNative
    dev = torch.device("cuda")
    nat3 = UNetNative(3, 3, depth=2, device=dev)
    with pytest.raises(ValueError):  # as before
        nat3.executor(1, 32, 32, training=True, loss="bce_dice")
    nat1 = UNetNative(3, 1, depth=2, device=dev)
    with pytest.raises(ValueError):
        nat1.executor(1, 32, 32, training=True, loss="ce_dice")
    with pytest.raises(ValueError):
        nat1.executor(1, 32, 32, training=True, loss="bce", class_weights=(1.0,))
    for bad in ((1.0, 2.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (0.0, 0.0, 0.0), (1.0, float("inf"), 1.0)):
        with pytest.raises(ValueError):
            nat3.executor(1, 32, 32, training=True, loss="ce_dice", class_weights=bad)
        with pytest.raises(ValueError):
            nat3.executor(1, 32, 32, training=True, loss="ce", class_weights=bad)
    # the weights are part of the executor cache key
    e1 = nat3.executor(1, 32, 32, training=True, loss="ce", class_weights=(1, 2, 3))
    e2 = nat3.executor(1, 32, 32, training=True, loss="ce", class_weights=(1, 2, 4))
    e3 = nat3.executor(1, 32, 32, training=True, loss="ce")
    assert e1 is not e2 and e1 is not e3 and e3.class_w is None
    assert e1 is nat3.executor(1, 32, 32, training=True, loss="ce", class_weights=[1.0, 2.0, 3.0])
    assert e1.class_w.dtype == torch.float32 and e1.class_w.is_cuda and e1.class_w.tolist() == [1.0, 2.0, 3.0]


def test_ce_dice_native_train_register_serve(tmp_path):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.serve.engine import FramePipeline
    from robotic_discovery_platform_amd.train.trainer import train_model
    cfg = TrainConfig(epochs=2, batch_size=4, image_size=32, synthetic_samples=12, model_depth=2,
                      dataset_dir=str(tmp_path / "nodata"), mlruns_dir=str(tmp_path / "mlruns"),
                      model_output_dir=str(tmp_path / "models"), backend="native", learning_rate=1e-3,
                      n_classes=3, loss="ce_dice", class_weights="1,4,4")
    res = train_model(cfg)
    assert res["backend"] == "native" and res["registered_version"] == "1" and len(res["history"]) == 2
    for h in res["history"]:
        assert h["train_loss"] == h["train_loss"] and h["val_loss"] == h["val_loss"]  # finite, not NaN
    store = str(tmp_path / "mlruns")
    p = mlstore.FileStore(store).get_run(res["run_id"]).data["params"]
    assert p["loss"] == "ce_dice" and p["class_weights"] == "1,4,4" and p["n_classes"] == "3"
    model = mlstore.pytorch.load_model("models:/Actuator-Segmenter/1", map_location=torch.device("cuda"),
                                       backend="native", tracking_uri=store)
    assert model.n_classes == 3
    sc = make_scene(2, n_classes=3)
    r = FramePipeline(model, DEFAULT_K, 0.001, graph=False, mask_class=1).process(sc.color, sc.depth)
    torch.cuda.synchronize()
    assert r.mask.shape == sc.depth.shape and 0.0 <= r.coverage <= 100.0
