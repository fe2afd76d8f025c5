"""The optimizer's device scalars (csrc/optim.hip): the gradient's sum of squares (exact on integer
gradients), the one-block control kernel against the fp64 oracle of train/schedule.py, and ``adam_ctl``
against ``adam`` (bitwise with neutral scalars) and against torch's Adam + clip_grad_norm_ + LambdaLR."""
import math

import numpy as np
import pytest
import torch

import lattice as L
from robotic_discovery_platform_amd.train.schedule import clip_coef, lr_multiplier

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def _within_one_ulp(got: float, want64: float) -> bool:
    """``got`` (an fp32 value) is the fp32 rounding of ``want64`` or one of its two fp32 neighbours."""
    w = np.float32(want64)
    return np.float32(got) in (w, np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf)))


# ---- the norm pass ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def int_grads():
    """Integer gradients in -3..3 per size (fp32 and their exact bf16 form) with the CPU integer sum of squares."""
    out = {}
    for n in (4, 4 * 257, 1 << 20):
        g = L.int_vector(n, torch.Generator().manual_seed(100 + n), 3)
        want = int((g.long() ** 2).sum())
        assert want <= 9 * (1 << 20) < (1 << 24)
        out[n] = (g.to(DEV), g.to(torch.bfloat16).to(DEV), want)
    return out


@pytest.mark.parametrize("n,max_blocks", [(4, 0), (4 * 257, 0), (1 << 20, 0), (1 << 20, 2)])
@pytest.mark.parametrize("bf16", [False, True])
def test_grad_sqnorm_exact(C, int_grads, n, max_blocks, bf16):
    g32, g16, want = int_grads[n]
    g = g16 if bf16 else g32
    assert torch.equal(g.float(), g32)  # -3..3 are exact in bf16
    auto = C.grad_sqnorm_blocks(n)
    blocks = min(auto, max_blocks) if max_blocks else auto
    assert blocks >= 1 and (n != 4 * 257 or blocks == 2) and (n != 1 << 20 or max_blocks or blocks > 2)
    partial = torch.full((blocks + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    assert C.grad_sqnorm(g, partial, max_blocks) == blocks
    first = partial.clone()
    # every partial is an integer below 2^24: any summation order is exact
    assert float(first[:blocks].sum().item()) == float(want)
    assert torch.equal(first[blocks:], torch.full((8,), SENTINEL, dtype=torch.float64, device=DEV))
    partial.fill_(SENTINEL)
    assert C.grad_sqnorm(g, partial, max_blocks) == blocks
    assert torch.equal(partial, first)  # no atomics: the same grid gives the same bits


# ---- the control block -----------------------------------------------------------------------------

W_, T_, R_ = 3, 11, 0.1
STEPS = [0, W_ - 1, W_, W_ + (T_ - W_) // 2, T_ - 1, T_, T_ + 5]
PARTIALS = [1.5, 2.25, 1000.0, 0.125]  # fp64 partial sums of squares


def _ctl(C, t, nblocks=0, gscale=1.0, clip=0.0, sched="constant", W=0, T=0, r=0.0):
    partial = torch.tensor(PARTIALS, dtype=torch.float64, device=DEV)
    step = torch.tensor([t], dtype=torch.int32, device=DEV)
    ctl = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
    C.optim_ctl(partial, nblocks, gscale, clip, 1 if sched == "cosine" else 0, W, T, r, step, ctl)
    assert int(step.item()) == t  # reads the counter, never advances it
    return ctl.tolist()


@pytest.mark.parametrize("sched", ["constant", "cosine"])
@pytest.mark.parametrize("r", [R_, 0.0])
def test_optim_ctl_multiplier(C, sched, r):
    for t in STEPS:
        c = _ctl(C, t, sched=sched, W=W_, T=T_ if sched == "cosine" else 0, r=r)
        want = lr_multiplier(t, sched, W_, T_ if sched == "cosine" else None, r)
        assert _within_one_ulp(c[1], want), (t, c[1], want)
        q_end = sched == "constant" or t == W_ or t >= T_
        if t < W_ or q_end:  # warmup and q in {0, 1}: no cosine rounding in the way
            assert np.float32(c[1]) == np.float32(want), (t, c[1], want)
        assert c[0] == 1.0 and c[2] == 0.0 and c[3] == float(t)  # no norm was computed


@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_optim_ctl_clip(C, gscale):
    norm64 = math.sqrt(sum(PARTIALS)) * gscale
    n = len(PARTIALS)
    for clip in (0.5 * norm64, 0.01, norm64):  # clipping active (at c == norm the 1e-6 still clips)
        c = _ctl(C, 5, n, gscale, clip)
        want = clip_coef(norm64, clip)
        assert want < 1.0 and _within_one_ulp(c[0], want), (clip, c[0], want)
        assert _within_one_ulp(c[2], norm64) and c[1] == 1.0 and c[3] == 5.0
    for clip in (norm64 + 1e-6, 2.0 * norm64, 1e9, 0.0):  # at or above the norm (+ eps), and off
        c = _ctl(C, 5, n, gscale, clip)
        assert clip_coef(norm64, clip) == 1.0 and c[0] == 1.0, (clip, c[0])
        assert _within_one_ulp(c[2], norm64)
    # a prefix of the partials only
    c = _ctl(C, 0, 2, 1.0, 1.0)
    assert _within_one_ulp(c[2], math.sqrt(3.75)) and _within_one_ulp(c[0], clip_coef(math.sqrt(3.75), 1.0))


def test_optim_ctl_many_partials_fixed_order(C):
    """2048 partials (the largest grid): the sum is exact for integers and bitwise the same twice."""
    g = torch.Generator().manual_seed(3)
    vals = torch.randint(0, 1 << 12, (2048,), generator=g).double()
    partial = vals.to(DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = torch.zeros(4, device=DEV)
    b = torch.zeros(4, device=DEV)
    C.optim_ctl(partial, 2048, 1.0, 1.0, 0, 0, 0, 0.0, step, a)
    C.optim_ctl(partial, 2048, 1.0, 1.0, 0, 0, 0, 0.0, step, b)
    assert torch.equal(a, b)
    norm64 = math.sqrt(float(vals.sum()))
    assert _within_one_ulp(a[2].item(), norm64) and _within_one_ulp(a[0].item(), clip_coef(norm64, 1.0))


# ---- Adam with the control block -------------------------------------------------------------------

def _adam_state(n, seed):
    torch.manual_seed(seed)
    p = torch.randn(n, device=DEV)
    return [p, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV),
            torch.zeros(n, dtype=torch.bfloat16, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("max_blocks", [0, 3])
def test_adam_ctl_neutral_is_bitwise_adam(C, bf16, max_blocks):
    n = 4 * 1031  # 5 blocks, the last one partly filled; 3 blocks take two passes
    a, b = _adam_state(n, 9), _adam_state(n, 9)
    ctl = torch.tensor([1.0, 1.0, 123.0, 7.0], device=DEV)
    for k in range(5):
        g = torch.randn(n, device=DEV)
        if bf16:
            g = g.to(torch.bfloat16)
        C.adam(a[0], g, a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5, a[4], True, max_blocks)
        C.adam_ctl(b[0], g, b[1], b[2], b[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5, b[4], ctl, True, max_blocks)
    assert a[4].item() == b[4].item() == 5
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("max_blocks", [0, 1])
def test_adam_ctl_clip_cosine_matches_torch(C, max_blocks):
    """``max_blocks=1``: one block walks the 1024 float4s in four passes of the grid-stride loop."""
    n, lr, W, T, r = 4096, 1e-3, 2, 8, 0.1
    torch.manual_seed(9)
    p0 = torch.randn(n, device=DEV)
    scales = [1.0, 0.2, 1.5, 0.3, 2.0, 0.25, 1.0, 0.1]
    grads = [torch.randn(n, device=DEV) * s for s in scales]
    clip = 0.6 * math.sqrt(n)  # randn: norm ~ scale * sqrt(n)
    norms = [float(g.double().norm()) for g in grads]
    assert sum(nm > clip for nm in norms) >= 3 and sum(nm + 1e-6 <= clip for nm in norms) >= 1
    p = p0.clone()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctl = torch.zeros(4, device=DEV)
    partial = torch.zeros(C.grad_sqnorm_blocks(n), dtype=torch.float64, device=DEV)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda t: lr_multiplier(t, "cosine", W, T, r))
    for k, g in enumerate(grads):
        nb = C.grad_sqnorm(g, partial)
        C.optim_ctl(partial, nb, 1.0, clip, 1, W, T, r, step, ctl)
        C.adam_ctl(p, g, m, v, sh, lr, 0.9, 0.999, 1e-8, 0.0, 1.0, step, ctl, True, max_blocks)
        got = ctl.tolist()
        assert _within_one_ulp(got[0], clip_coef(norms[k], clip)) and _within_one_ulp(got[2], norms[k])
        assert _within_one_ulp(got[1], lr_multiplier(k, "cosine", W, T, r)) and got[3] == float(k)
        ref.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref], clip)
        opt.step()
        sched.step()
    assert step.item() == 8
    assert torch.allclose(p, ref.detach(), atol=1e-6, rtol=1e-5)
    assert torch.equal(sh, p.to(torch.bfloat16))


@pytest.mark.parametrize("kernel", ["adam", "adam_ctl"])
@pytest.mark.parametrize("bf16", [False, True])
def test_grid_stride_passes_match_torch(C, kernel, bf16):
    """Several passes of the update's grid-stride loop (2 blocks over 1031 float4s, the last pass partly
    filled) against torch.optim.Adam, 5 steps: the tolerance of the existing ``test_adam_matches_torch``."""
    n = 4 * 1031
    torch.manual_seed(11)
    p0 = torch.randn(n, device=DEV)
    p = p0.clone()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctl = torch.tensor([1.0, 1.0, 0.0, 0.0], device=DEV)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    for _ in range(5):
        g = torch.randn(n, device=DEV)
        if bf16:
            g = g.to(torch.bfloat16)
        if kernel == "adam":
            C.adam(p, g, m, v, sh, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, step, True, 2)
        else:
            C.adam_ctl(p, g, m, v, sh, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, step, ctl, True, 2)
        ref.grad = g.float()
        opt.step()
    assert step.item() == 5
    assert torch.allclose(p, ref.detach(), atol=1e-6, rtol=1e-5)
    assert torch.equal(sh, p.to(torch.bfloat16))


def test_argument_checks(C):
    f32 = lambda n: torch.zeros(n, device=DEV)  # noqa: E731
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)  # noqa: E731
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    big = f32(1 << 20)
    with pytest.raises(RuntimeError):
        C.grad_sqnorm_blocks(6)
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(f32(6), f64(8))  # n % 4
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(big, f64(C.grad_sqnorm_blocks(1 << 20) - 1))  # short partial buffer
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(big, f32(4096))  # partial dtype
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(f64(8), f64(8))  # gradient dtype
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(big[::2], f64(4096))  # not contiguous
    with pytest.raises(RuntimeError):
        C.grad_sqnorm(torch.zeros(8), f64(8))  # host gradient
    C.grad_sqnorm(big, f64(2), 2)  # a capped grid needs only its own blocks
    with pytest.raises(RuntimeError):
        C.optim_ctl(f64(4), 5, 1.0, 1.0, 0, 0, 0, 0.0, step, f32(4))  # nblocks past the buffer
    with pytest.raises(RuntimeError):
        C.optim_ctl(f64(4), 4, 1.0, 1.0, 0, 0, 0, 0.0, step, f32(3))  # short ctl
    with pytest.raises(RuntimeError):
        C.optim_ctl(f32(4), 4, 1.0, 1.0, 0, 0, 0, 0.0, step, f32(4))  # partial dtype
    with pytest.raises(RuntimeError):
        C.optim_ctl(f64(4), 4, 1.0, 1.0, 0, 0, 0, 0.0, step.long(), f32(4))  # step dtype
    with pytest.raises(RuntimeError):
        C.optim_ctl(f64(4), 4, 1.0, 1.0, 1, 4, 4, 0.0, step, f32(4))  # cosine needs total > warmup
    with pytest.raises(RuntimeError):
        C.optim_ctl(f64(4), 4, 1.0, -1.0, 0, 0, 0, 0.0, step, f32(4))  # negative clip
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, step)
    with pytest.raises(RuntimeError):
        C.adam_ctl(f32(6), f32(6), f32(6), f32(6), None, *args, f32(4))  # n % 4
    with pytest.raises(RuntimeError):
        C.adam_ctl(f32(8), f32(8), f32(8), f32(4), None, *args, f32(4))  # short state buffer
    with pytest.raises(RuntimeError):
        C.adam_ctl(f32(8), f32(8), f32(8), f32(8), None, *args, f32(2))  # short ctl
    with pytest.raises(RuntimeError):
        C.adam_ctl(f32(8), f32(8), f32(8), f32(8), None, *args, f64(4))  # ctl dtype
    torch.cuda.synchronize()
