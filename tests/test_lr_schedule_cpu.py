"""The learning-rate schedule / gradient-clipping definition (train/schedule.py) against hand values and
torch's own LambdaLR / clip_grad_norm_, and the eager ``train_model`` path that uses it: logging, the
promise that a default run logs nothing new, and resume (the schedule follows the optimizer's step)."""
import math

import pytest
import torch

from robotic_discovery_platform_amd import mlstore
from robotic_discovery_platform_amd.config import TrainConfig
from robotic_discovery_platform_amd.train.schedule import OptimOptions, clip_coef, lr_multiplier

NEW_PARAMS = {"clip_grad_norm", "lr_schedule", "warmup_steps", "min_lr_ratio", "total_steps"}
NEW_METRICS = {"lr", "grad_norm"}


def test_warmup_hand_values():
    assert [lr_multiplier(t, "constant", 4) for t in range(4)] == [0.25, 0.5, 0.75, 1.0]
    assert [lr_multiplier(t, "constant", 4) for t in (4, 5, 1000)] == [1.0, 1.0, 1.0]
    assert lr_multiplier(0) == 1.0 and lr_multiplier(7, "constant", 0, None, 0.5) == 1.0


def test_cosine_hand_values():
    W, T, r = 2, 10, 0.1
    f = lambda t: lr_multiplier(t, "cosine", W, T, r)  # noqa: E731
    assert f(0) == 0.5 and f(1) == 1.0  # warmup
    assert f(2) == 1.0  # q = 0, exactly
    for t in (10, 11, 15, 10_000):
        assert f(t) == r  # q = 1, exactly
    assert f(6) == pytest.approx(0.55, abs=1e-15)  # the midpoint: r + (1 - r) / 2
    after = [f(t) for t in range(W, T + 4)]
    assert all(a >= b for a, b in zip(after, after[1:]))
    assert all(r <= v <= 1.0 for v in after)


def test_matches_torch_lambda_lr():
    W, T, r, lr = 2, 10, 0.1, 1e-3
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([p], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda t: lr_multiplier(t, "cosine", W, T, r))
    for t in range(12):
        assert opt.param_groups[0]["lr"] == lr * lr_multiplier(t, "cosine", W, T, r), t
        p.grad = torch.ones(3)
        opt.step()
        sched.step()


def test_clip_coef_matches_clip_grad_norm():
    g = torch.Generator().manual_seed(0)
    shapes = [(5, 3), (7,), (2, 2, 4)]
    grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    norm = math.sqrt(sum(float((x * x).sum()) for x in grads))
    for c in (0.5 * norm, 0.1, 2.0 * norm):
        params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
        for p, x in zip(params, grads):
            p.grad = x.clone()
        total = torch.nn.utils.clip_grad_norm_(params, c)
        assert float(total) == pytest.approx(norm, rel=1e-14)
        k = clip_coef(norm, c)
        assert (k == 1.0) == (c >= norm + 1e-6)
        for p, x in zip(params, grads):
            assert torch.allclose(p.grad, x * k, rtol=1e-14, atol=0)
    assert clip_coef(123.0, 0.0) == 1.0 and clip_coef(0.0, 1.0) == 1.0
    assert clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)


@pytest.mark.parametrize("kw", [
    {"lr_schedule": "cosine"},  # no total_steps
    {"lr_schedule": "cosine", "warmup_steps": 5, "total_steps": 5},
    {"lr_schedule": "linear"},
    {"clip_grad_norm": -1.0}, {"clip_grad_norm": float("inf")}, {"clip_grad_norm": float("nan")},
    {"warmup_steps": -1}, {"min_lr_ratio": -0.1}, {"min_lr_ratio": 1.5}, {"min_lr_ratio": float("nan")},
])
def test_bad_options_raise(kw):
    from robotic_discovery_platform_amd.models.unet_ref import UNetRef
    from robotic_discovery_platform_amd.train.engine import EagerTrainer
    with pytest.raises(ValueError):
        OptimOptions(**kw)
    with pytest.raises(ValueError):
        EagerTrainer(UNetRef(3, 1, depth=2), **kw)


def test_functions_reject_bad_arguments():
    for args in [(0, "cosine"), (0, "cosine", 5, 5), (0, "linear"), (0, "constant", -1), (-1,),
                 (0, "cosine", 0, 4, 1.5), (0, "cosine", 0, 4, float("nan"))]:
        with pytest.raises(ValueError):
            lr_multiplier(*args)
    for c in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            clip_coef(1.0, c)


def test_enabled_iff_an_option_is_on():
    assert not OptimOptions().enabled and not OptimOptions(min_lr_ratio=0.5, total_steps=10).enabled
    assert OptimOptions(clip_grad_norm=1.0).enabled and OptimOptions(warmup_steps=1).enabled
    assert OptimOptions(lr_schedule="cosine", total_steps=3).enabled


def _cfg(tmp_path, **kw):
    c = TrainConfig(epochs=2, batch_size=4, image_size=32, synthetic_samples=10, model_depth=2,
                    dataset_dir=str(tmp_path / "nodata"), mlruns_dir=str(tmp_path / "mlruns"),
                    model_output_dir=str(tmp_path / "models"), backend="eager", learning_rate=1e-3)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_eager_train_model_logs_lr_and_params(tmp_path):
    from robotic_discovery_platform_amd.train.trainer import train_model
    cfg = _cfg(tmp_path, clip_grad_norm=0.5, lr_schedule="cosine", warmup_steps=2)
    res = train_model(cfg)
    steps_per_epoch = 2  # 8 training samples, batch 4
    total = cfg.epochs * steps_per_epoch
    st = mlstore.FileStore(str(tmp_path / "mlruns"))
    p = st.get_run(res["run_id"]).data["params"]
    assert NEW_PARAMS <= set(p)
    assert p["lr_schedule"] == "cosine" and p["warmup_steps"] == "2" and p["total_steps"] == str(total)
    assert float(p["clip_grad_norm"]) == 0.5
    m = st.get_metrics(res["run_id"])
    assert [s for _, _, s in m["lr"]] == [0, 1] and [s for _, _, s in m["grad_norm"]] == [0, 1]
    for e, h in enumerate(res["history"]):
        t_last = (e + 1) * steps_per_epoch - 1
        assert h["lr"] == cfg.learning_rate * lr_multiplier(t_last, "cosine", 2, total, 0.0)
        assert math.isfinite(h["grad_norm"]) and h["grad_norm"] > 0
    assert [v for _, v, _ in m["lr"]] == [h["lr"] for h in res["history"]]


def test_default_run_logs_none_of_the_new_keys(tmp_path):
    from robotic_discovery_platform_amd.train.trainer import train_model
    res = train_model(_cfg(tmp_path))
    st = mlstore.FileStore(str(tmp_path / "mlruns"))
    assert not NEW_PARAMS & set(st.get_run(res["run_id"]).data["params"])
    assert not NEW_METRICS & set(st.get_metrics(res["run_id"]))
    assert all(not NEW_METRICS & set(h) for h in res["history"])


def test_resume_continues_the_schedule(tmp_path, monkeypatch):
    """A run stopped after its first epoch and resumed from the checkpoint ends with exactly the weights
    and learning rates of the uninterrupted run: the schedule follows the optimizer's restored step."""
    from robotic_discovery_platform_amd.mlstore import pytorch as mlpt
    from robotic_discovery_platform_amd.train.trainer import train_model
    from robotic_discovery_platform_amd.utils import launch
    kw = dict(epochs=3, clip_grad_norm=0.5, lr_schedule="cosine", warmup_steps=2, min_lr_ratio=0.1)
    clean = train_model(_cfg(tmp_path / "clean", **kw))

    class Stop(Exception):
        pass

    def stop_at_epoch_1(epoch, rank=None):
        if epoch == 1:
            raise Stop()
    monkeypatch.setattr(launch, "maybe_crash", stop_at_epoch_1)
    with pytest.raises(Stop):
        train_model(_cfg(tmp_path / "job", **kw))
    mlstore.end_run()
    monkeypatch.undo()
    resumed = train_model(_cfg(tmp_path / "job", **kw), resume="auto")
    assert [h["epoch"] for h in resumed["history"]] == [1, 2]
    for a, b in zip(clean["history"][1:], resumed["history"]):
        assert a["lr"] == b["lr"] and a["train_loss"] == b["train_loss"] and a["val_loss"] == b["val_loss"]
    uri = "models:/Actuator-Segmenter/latest"
    _, sa = mlpt.load_state(uri, str(tmp_path / "clean" / "mlruns"))
    _, sb = mlpt.load_state(uri, str(tmp_path / "job" / "mlruns"))
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
