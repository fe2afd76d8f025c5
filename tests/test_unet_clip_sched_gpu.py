"""Gradient clipping and the warmup / cosine schedule inside the native training step (depth-2 U-Net,
batch 2, 64 x 64): off = today's step bit for bit; on = one recorded plan for the whole run, the same
bits in eager, plan and hipGraph modes, with the overlapped and the single-launch Adam and under DDP,
and the losses of the eager reference trainer with the same options."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from robotic_discovery_platform_amd import mlstore
from robotic_discovery_platform_amd.config import TrainConfig
from robotic_discovery_platform_amd.train.schedule import lr_multiplier

pytestmark = pytest.mark.gpu

N, HW, DEPTH = 2, 64, 2
W_, T_ = 2, 8
WEIGHTS = (1.0, 4.0, 4.0)


def _within_one_ulp(got: float, want64: float) -> bool:
    w = np.float32(want64)
    return np.float32(got) in (w, np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf)))


def _batches(K=1, steps=8, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for _ in range(steps):
        x = torch.rand(N, 3, HW, HW, generator=g)
        if K == 1:
            y = (torch.rand(N, 1, HW, HW, generator=g) > 0.5).float()
        else:
            y = torch.randint(0, K, (N, HW, HW), generator=g)
        out.append((x, y))
    return out


def _ref_state(K=1, seed=3):
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in UNetRef(3, K, depth=DEPTH).state_dict().items()}


def _native(sd, K=1):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    ref = UNetRef(3, K, depth=DEPTH)
    ref.load_state_dict(sd)
    return UNetNative(3, K, depth=DEPTH, device=torch.device("cuda"), init_from=ref)


def _state(nat):
    st = nat.store
    torch.cuda.synchronize()
    return (st.flat.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(), st.shadow.clone(), nat.derived.clone(),
            int(st.step.item()))


def _assert_same(a, b, what=""):
    assert a[5] == b[5], what
    for u, v in zip(a[:5], b[:5]):
        assert torch.equal(u, v), what


@pytest.fixture(scope="module")
def first_norm():
    """The L2 norm of the first step's gradient (a reference step without the options): the clip
    thresholds below are half of it, so clipping is active from the first step."""
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    nat = _native(_ref_state())
    tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=False)
    x, y = _batches()[0]
    tr.set_batch(x.cuda(), y.cuda())
    tr.step()
    torch.cuda.synchronize()
    norm = float(nat.store.grad.double().norm())
    assert norm > 0 and np.isfinite(norm)
    return norm


def _options(first_norm):
    return dict(clip_grad_norm=0.5 * first_norm, lr_schedule="cosine", warmup_steps=W_, total_steps=T_)


def test_options_off_is_todays_step():
    from robotic_discovery_platform_amd.ops import native
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    C = native()
    sd, batches = _ref_state(), _batches(steps=4)
    runs = []
    for kw in ({}, dict(clip_grad_norm=0.0, lr_schedule="constant", warmup_steps=0, total_steps=100, min_lr_ratio=0.3)):
        nat = _native(sd)
        tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=True, **kw)
        assert tr.opt.last_ctl() is None and tr.opt._ctl is None and len(tr.opt.hyper_key()) == 4
        for x, y in batches:
            tr.set_batch(x.cuda(), y.cuda())
            tr.step()
        runs.append((C.plan_kinds(tr.plan_id), _state(nat)))
    assert runs[0][0] == runs[1][0]
    _assert_same(runs[0][1], runs[1][1])


@pytest.fixture(scope="module")
def runs_on(first_norm):
    """8 steps with clipping + warmup + cosine in the three execution modes (shared, left unchanged)."""
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    sd, batches = _ref_state(), _batches()
    out = {}
    for mode in ("eager", "plan", "graph"):
        nat = _native(sd)
        tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=mode == "plan", graph=mode == "graph", **_options(first_norm))
        assert tr.use_plan == (mode == "plan") and tr.use_graph == (mode == "graph")
        losses, ctls, plan_ids = [], [], []
        for x, y in batches:
            tr.set_batch(x.cuda(), y.cuda())
            losses.append(tr.step().clone())
            ctls.append(tr.opt.last_ctl())
            plan_ids.append(tr.plan_id)
        out[mode] = dict(state=_state(nat), losses=torch.stack(losses).cpu(), ctls=ctls, plan_ids=plan_ids,
                         graph=tr.graph)
    return out


def test_options_on_modes_agree_bitwise(runs_on):
    for mode in ("plan", "graph"):
        _assert_same(runs_on["eager"]["state"], runs_on[mode]["state"], mode)
        assert torch.equal(runs_on["eager"]["losses"], runs_on[mode]["losses"]), mode
        assert [c["coef"] for c in runs_on[mode]["ctls"]] == [c["coef"] for c in runs_on["eager"]["ctls"]]
    assert runs_on["eager"]["state"][5] == 8 and runs_on["graph"]["graph"] is not None


def test_one_plan_for_the_whole_schedule(runs_on):
    ids = runs_on["plan"]["plan_ids"]
    assert ids[2] is not None and all(i == ids[2] for i in ids[2:])  # recorded at step 3, replayed to step 8


def test_last_ctl_follows_the_step_counter(runs_on, first_norm):
    for mode, run in runs_on.items():
        for k, c in enumerate(run["ctls"], start=1):
            assert c["t"] == k - 1, (mode, k)
            assert _within_one_ulp(c["mult"], lr_multiplier(k - 1, "cosine", W_, T_, 0.0)), (mode, k, c)
            assert 0.0 < c["coef"] <= 1.0 and c["norm"] > 0
        first = run["ctls"][0]
        assert first["coef"] < 1.0  # clipping is active: the threshold is half the first norm
        assert first["norm"] == pytest.approx(first_norm, rel=1e-5)
        assert run["ctls"][-1]["mult"] < run["ctls"][2]["mult"] == 1.0


def test_losses_match_the_eager_reference_trainer(runs_on, first_norm):
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import EagerTrainer
    ref = UNetRef(3, 1, depth=DEPTH)
    ref.load_state_dict(_ref_state())
    ref = ref.cuda().train()
    tr = EagerTrainer(ref, lr=1e-3, **_options(first_norm))
    want = []
    for k, (x, y) in enumerate(_batches()):
        want.append(float(tr.step(x.cuda().to(torch.bfloat16).float(), y.cuda())))  # the same bf16-rounded input
        assert tr.last_lr == 1e-3 * lr_multiplier(k, "cosine", W_, T_, 0.0)
    got = runs_on["eager"]["losses"][:, 0].tolist()
    print(list(zip(got, want)))
    # the native-vs-reference loss tolerance of tests/test_unet_native_gpu.py
    assert max(abs(a - b) for a, b in zip(got, want)) < 2e-2, list(zip(got, want))


@pytest.mark.parametrize("plan", [False, True])
def test_overlapped_adam_matches_single_launch(first_norm, plan):
    from robotic_discovery_platform_amd.models.unet import NativeAdam
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    sd, batches = _ref_state(), _batches(steps=5)
    states = []
    for overlap in (True, False):
        NativeAdam.OVERLAP = overlap
        try:
            nat = _native(sd)
            tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=plan, **_options(first_norm))
            assert nat._adam_split > 0 and tr._wprep_side() is not None
            losses = []
            for x, y in batches:
                tr.set_batch(x.cuda(), y.cuda())
                losses.append(tr.step().clone())
            states.append((_state(nat), torch.stack(losses), tr.opt.last_ctl()))
        finally:
            NativeAdam.OVERLAP = True
    _assert_same(states[0][0], states[1][0])
    assert states[0][0][5] == 5 and torch.equal(states[0][1], states[1][1]) and states[0][2] == states[1][2]


def test_k3_ce_dice_plan_equals_eager(first_norm):
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    sd, batches = _ref_state(K=3), _batches(K=3, steps=6)
    opts = dict(clip_grad_norm=0.25 * first_norm, lr_schedule="cosine", warmup_steps=W_, total_steps=6,
                min_lr_ratio=0.1)
    runs = []
    for plan in (False, True):
        nat = _native(sd, K=3)
        tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, loss="ce_dice", dice_weight=0.5, class_weights=WEIGHTS, plan=plan,
                           **opts)
        losses = []
        for x, y in batches:
            tr.set_batch(x.cuda(), y.cuda())
            losses.append(tr.step().clone())
        runs.append((_state(nat), torch.stack(losses), tr.opt.last_ctl()))
        assert (tr.plan_id is not None) == plan
    _assert_same(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert runs[0][2]["t"] == 5 and _within_one_ulp(runs[0][2]["mult"], lr_multiplier(5, "cosine", W_, 6, 0.1))


def test_restored_state_continues_the_schedule(first_norm):
    """Model + Adam state saved after 3 steps and loaded into a fresh trainer: the 4th and 5th steps are
    bitwise those of the uninterrupted trainer (the schedule follows the restored device step counter;
    ``state_dict()`` keeps its keys)."""
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    sd, batches, opts = _ref_state(), _batches(steps=5), _options(first_norm)
    nat = _native(sd)
    tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=True, **opts)
    for x, y in batches[:3]:
        tr.set_batch(x.cuda(), y.cuda())
        tr.step()
    saved = ({k: v.clone() for k, v in nat.state_dict().items()}, tr.opt.state_dict())
    assert set(saved[1]) == {"step", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay"}
    nat2 = _native(sd)
    tr2 = NativeTrainer(nat2, N, HW, HW, lr=1e-3, plan=True, **opts)
    nat2.load_state_dict(saved[0])
    tr2.opt.load_state_dict(saved[1])
    for x, y in batches[3:]:
        for t in (tr, tr2):
            t.set_batch(x.cuda(), y.cuda())
            t.step()
    _assert_same(_state(nat), _state(nat2))
    assert tr.opt.last_ctl() == tr2.opt.last_ctl() and tr2.opt.last_ctl()["t"] == 4


# ---- DDP forced at world 1 under nccl ---------------------------------------------------------------

DDP_STEPS = 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, port, comm, opts, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", RDP_DDP_COMM="native")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from robotic_discovery_platform_amd.train.engine import NativeTrainer
        nat = _native(_ref_state())
        tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, graph=False, bucket_mb=0.25, ddp_force=True, grad_comm=comm,
                           plan=True, **opts)
        assert tr.ddp and tr.bucketer is not None and len(tr.bucketer.buckets) >= 2 and tr.use_plan
        assert tr.bucketer.native_comm is not None and (tr.bucketer.comm is not None) == (comm == "bf16")
        for x, y in _batches(steps=DDP_STEPS):
            tr.set_batch(x.to(dev), y.to(dev))
            tr.step()
        torch.cuda.synchronize()
        assert tr.plan_id is not None
        st = nat.store
        torch.save({"flat": st.flat.cpu(), "exp_avg_sq": st.exp_avg_sq.cpu(), "ctl": tr.opt.last_ctl()}, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_ddp_world1_equals_plain_trainer(tmp_path, first_norm, comm):
    """fp32 buckets: bitwise the non-DDP trainer. bf16 buckets (the norm and Adam read the reduced bf16
    buffer): bitwise the plain step on gradients rounded to bf16, as tests/test_ddp_rccl_gpu.py compares."""
    from robotic_discovery_platform_amd.models.unet import NativeAdam
    from robotic_discovery_platform_amd.train.engine import NativeTrainer
    opts = _options(first_norm)
    out = str(tmp_path / f"ddp_{comm}.pt")
    mp.spawn(_ddp_worker, args=(_free_port(), comm, opts, out), nprocs=1, join=True)
    got = torch.load(out, weights_only=True)
    nat = _native(_ref_state())
    if comm == "fp32":
        tr = NativeTrainer(nat, N, HW, HW, lr=1e-3, plan=True, **opts)
        assert not tr.ddp
        for x, y in _batches(steps=DDP_STEPS):
            tr.set_batch(x.cuda(), y.cuda())
            tr.step()
        opt = tr.opt
    else:
        ex = nat.executor(N, HW, HW, training=True)
        opt = NativeAdam(nat, lr=1e-3, **opts)
        for x, y in _batches(steps=DDP_STEPS):
            ex.set_input(x.cuda(), y.cuda())
            ex.forward()
            ex.backward()
            nat.store.grad.copy_(nat.store.grad.to(torch.bfloat16).float())
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(got["flat"], nat.store.flat.cpu()) and torch.equal(got["exp_avg_sq"], nat.store.exp_avg_sq.cpu())
    assert got["ctl"] == opt.last_ctl() and got["ctl"]["t"] == DDP_STEPS - 1 and got["ctl"]["coef"] < 1.0


# ---- train_model ------------------------------------------------------------------------------------

def test_native_train_model_logs_lr_and_grad_norm(tmp_path):
    from robotic_discovery_platform_amd.train.trainer import train_model
    cfg = TrainConfig(epochs=2, batch_size=4, image_size=64, synthetic_samples=12, model_depth=2,
                      dataset_dir=str(tmp_path / "nodata"), mlruns_dir=str(tmp_path / "mlruns"),
                      model_output_dir=str(tmp_path / "models"), backend="native", learning_rate=1e-3,
                      clip_grad_norm=0.5, lr_schedule="cosine", warmup_steps=2, min_lr_ratio=0.01)
    res = train_model(cfg)
    assert res["backend"] == "native" and len(res["history"]) == 2
    steps_per_epoch = 3  # 10 training samples, batch 4: the last batch is ragged (a second trainer, one counter)
    total = cfg.epochs * steps_per_epoch
    st = mlstore.FileStore(str(tmp_path / "mlruns"))
    m = st.get_metrics(res["run_id"])
    assert [s for _, _, s in m["lr"]] == [0, 1] and [s for _, _, s in m["grad_norm"]] == [0, 1]
    p = st.get_run(res["run_id"]).data["params"]
    assert p["lr_schedule"] == "cosine" and p["total_steps"] == str(total) and p["warmup_steps"] == "2"
    for e, h in enumerate(res["history"]):
        assert h["train_loss"] == h["train_loss"] and h["grad_norm"] > 0 and np.isfinite(h["grad_norm"])
        want = lr_multiplier((e + 1) * steps_per_epoch - 1, "cosine", 2, total, 0.01)
        assert _within_one_ulp(h["lr"] / cfg.learning_rate, want), (e, h["lr"], want)
    # the run's final rate: lr x the multiplier of the last update, the multiplier to one fp32 ulp
    assert _within_one_ulp(res["history"][-1]["lr"] / cfg.learning_rate, lr_multiplier(total - 1, "cosine", 2, total, 0.01))
    assert [v for _, v, _ in m["lr"]] == [h["lr"] for h in res["history"]]
