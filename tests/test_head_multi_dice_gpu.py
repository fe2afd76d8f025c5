"""The K-class head's extended mode (csrc/head_multi.hip: class-weighted CE + soft Dice) vs
``ce_dice_reference`` in fp64.

Operands as in test_head_multi_gpu.py: ``a`` rounded to bf16 first; the reference is ``F.conv2d`` of it in
fp64 followed by ``train/losses.py::ce_dice_reference``. The bounds are those of
``test_headk_fwd_bwd_matches_torch``.
"""
import pytest
import torch
import torch.nn.functional as F

from robotic_discovery_platform_amd.train.losses import ce_dice_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def relerr(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _operands(K, N, H, W, seed=8, ignore=0.1, odd_labels=True):
    """test_head_multi_gpu.py::_operands: labels hold 255 and (odd_labels) five 200s"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(N, H, W, 64, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(K, 64, generator=g) * 0.1).cuda()
    b = (torch.randn(K, generator=g) * 0.1).cuda()
    lab = torch.randint(0, K, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < ignore] = 255
    if odd_labels:  # ids in K..254 are never an index: ignored like 255
        flat = lab.view(-1)
        flat[torch.randperm(flat.numel(), generator=g)[:5]] = 200
    return a, w, b, lab.to(torch.uint8).cuda()


def _weights(K):
    return torch.tensor([0.5 + 0.75 * k for k in range(K)], device="cuda")


def _run(C, a, w, b, lab, cw=None, lam=0.0, gscale=1.0, plain=False):
    K, M = b.numel(), lab.numel()
    logits = torch.zeros(M * K, device="cuda")
    part = torch.zeros(C.headk_partial_blocks(M) * K * 65, device="cuda")
    sums, loss = torch.zeros(2 + 3 * K, device="cuda"), torch.zeros(2, device="cuda")
    da = torch.full_like(a, 7.0)  # every pixel must be written, the ignored ones with zeros
    gw, gb = torch.full((K * 64,), 7.0, device="cuda"), torch.full((K,), 7.0, device="cuda")
    if plain:
        C.headk_fwd(a, w.reshape(-1), b, lab.reshape(-1), logits, part, sums, loss)
        C.headk_bwd(a, w.reshape(-1), logits, lab.reshape(-1), sums, da, part, gw, gb, gscale)
    else:
        C.headk_fwd(a, w.reshape(-1), b, lab.reshape(-1), logits, part, sums, loss, class_weights=cw, dice_w=lam)
        C.headk_bwd(a, w.reshape(-1), logits, lab.reshape(-1), sums, da, part, gw, gb, gscale, class_weights=cw,
                    dice_w=lam)
    return logits, loss, sums, da, gw, gb


def _reference(a, w, b, lab, cw, lam):
    """fp64: (L, CE, d a [N,64,H,W], dW [K,64], db [K])"""
    K = b.numel()
    ar = nchw(a).double().requires_grad_(True)
    wr = w.double().view(K, 64, 1, 1).requires_grad_(True)
    br = b.double().requires_grad_(True)
    L, ce = ce_dice_reference(F.conv2d(ar, wr, br), lab, None if cw is None else cw.double(), lam)
    L.backward()
    return L.item(), ce.item(), ar.grad, wr.grad.view(K, 64), br.grad


def _check(C, K, N, H, W, lam, weighted):
    a, w, b, lab = _operands(K, N, H, W)
    cw = _weights(K) if weighted else None
    logits, loss, sums, da, gw, gb = _run(C, a, w, b, lab, cw, lam)
    L, ce, ga, gwr, gbr = _reference(a, w, b, lab, cw, lam)
    errs = (relerr(nchw(da), ga), relerr(gw.view(K, 64), gwr), relerr(gb, gbr))
    print(f"K={K} M={N * H * W} lam={lam} weighted={weighted}: dL={abs(loss[0].item() - L):.2e} "
          f"dCE={abs(loss[1].item() - ce):.2e} relerr(da, dW, db)={errs}")
    assert abs(loss[0].item() - L) < 1e-4
    assert abs(loss[1].item() - ce) < 1e-4
    assert errs[0] < 1e-2  # da is stored as bf16
    assert errs[1] < 1e-4 and errs[2] < 1e-4
    ignored = (lab >= K)[:, None].expand(-1, 64, -1, -1)
    assert torch.count_nonzero(nchw(da).float()[ignored]) == 0
    return lab, sums


CASES = [(K, shape, lam, weighted) for K in (2, 3, 5, 8) for shape in ((2, 24, 20), (1, 5, 7))
         for lam in (0.0, 1.0, 2.5) for weighted in (False, True) if lam > 0 or weighted]


@pytest.mark.parametrize("K,shape,lam,weighted", CASES)
def test_headk_ext_matches_reference(C, K, shape, lam, weighted):
    """M = 960: the pixel-group stride does not divide it; M = 35: less than one block, ragged tail."""
    _check(C, K, *shape, lam, weighted)


@pytest.mark.parametrize("K", [2, 3, 5, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_headk_ext_sums(C, K, weighted):
    a, w, b, lab = _operands(K, 2, 24, 20)
    _, _, sums, _, _, _ = _run(C, a, w, b, lab, _weights(K) if weighted else None, 1.0)
    kept_lab = lab[lab < K].long()
    kept = kept_lab.numel()
    counts = torch.bincount(kept_lab, minlength=K).float()
    I, P, T = sums[2:2 + K], sums[2 + K:2 + 2 * K], sums[2 + 2 * K:2 + 3 * K]
    assert torch.equal(T, counts)  # integers below 2^24: exact
    if not weighted:
        assert sums[1].item() == kept
    assert abs(P.sum().item() - kept) <= 1e-5 * kept
    assert (I >= 0).all() and (I <= torch.minimum(P, T) * (1 + 1e-6)).all()


@pytest.mark.parametrize("K", [3, 8])
def test_headk_unit_weights_equal_plain_bitwise(C, K):
    a, w, b, lab = _operands(K, 2, 24, 20)
    plain = _run(C, a, w, b, lab, plain=True)
    ext = _run(C, a, w, b, lab, torch.ones(K, device="cuda"), 0.0)
    for i in (1, 3, 4, 5):  # loss, da, gw, gb
        assert torch.equal(plain[i], ext[i]), i


@pytest.mark.parametrize("K,zero", [(3, 1), (5, 0), (8, 7)])
def test_headk_zero_weight_class_equals_ignored_bitwise(C, K, zero):
    a, w, b, lab = _operands(K, 2, 24, 20)
    cw = _weights(K)
    cw[zero] = 0.0
    r1 = _run(C, a, w, b, lab, cw, 0.0)
    lab2 = lab.clone()
    lab2[lab == zero] = 255
    r2 = _run(C, a, w, b, lab2, cw, 0.0)
    for i in (1, 3, 4, 5):
        assert torch.equal(r1[i], r2[i]), i


def test_headk_ext_all_ignored(C):
    """No kept pixel: Dice = 1 - eps / eps = 0, so the loss is 0 and every gradient is 0."""
    a, w, b, lab = _operands(3, 1, 5, 7)
    lab.fill_(255)
    _, loss, sums, da, gw, gb = _run(C, a, w, b, lab, _weights(3), 1.5)
    assert loss[0].item() == 0.0 and loss[1].item() == 0.0 and sums[1].item() == 0.0
    assert torch.count_nonzero(da) == 0 and torch.count_nonzero(gw) == 0 and torch.count_nonzero(gb) == 0


def test_headk_ext_deterministic(C):
    a, w, b, lab = _operands(8, 2, 24, 20)
    r1, r2 = _run(C, a, w, b, lab, _weights(8), 1.0), _run(C, a, w, b, lab, _weights(8), 1.0)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)


def test_headk_ext_loss_scale(C):
    """test_head_multi_gpu.py::test_headk_loss_scale in extended mode, with its bounds: gscale = 3 scales
    the fp32 dW / db within rtol 1e-6, and da (bf16, rounded after the scale) within 1.01 * 2^-7."""
    a, w, b, lab = _operands(3, 2, 24, 20, odd_labels=False)
    _, _, _, da1, gw1, gb1 = _run(C, a, w, b, lab, _weights(3), 1.0, 1.0)
    _, _, _, da3, gw3, gb3 = _run(C, a, w, b, lab, _weights(3), 1.0, 3.0)
    assert torch.allclose(gw3, 3 * gw1, rtol=1e-6, atol=0) and torch.allclose(gb3, 3 * gb1, rtol=1e-6, atol=0)
    assert torch.allclose(da3.float(), 3 * da1.float(), rtol=1.01 * 2 ** -7, atol=0)


def test_headk_ext_second_grid_stride_pass(C):
    """M = 266,240 > 2048 blocks * 32 groups * 4 pixels in flight: a second pass, with a ragged tail."""
    lab, sums = _check(C, 5, 1, 520, 512, 1.0, True)
    assert torch.equal(sums[2 + 10:2 + 15], torch.bincount(lab[lab < 5].long(), minlength=5).float())


def test_headk_ext_argument_checks(C):
    K, M = 3, 35
    a, w, b, lab = _operands(K, 1, 5, 7)
    logits = torch.zeros(M * K, device="cuda")
    part = torch.zeros(C.headk_partial_blocks(M) * K * 65, device="cuda")
    loss = torch.zeros(2, device="cuda")
    args = (a, w.reshape(-1), b, lab.reshape(-1), logits, part)
    big, small = torch.zeros(2 + 3 * K, device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(RuntimeError):
        C.headk_fwd(*args, big, loss, class_weights=torch.ones(K - 1, device="cuda"))
    with pytest.raises(RuntimeError):
        C.headk_fwd(*args, big, loss, class_weights=torch.ones(K, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        C.headk_fwd(*args, small, loss, dice_w=1.0)
    da = torch.full_like(a, 7.0)
    gw, gb = torch.full((K * 64,), 7.0, device="cuda"), torch.full((K,), 7.0, device="cuda")
    bargs = (a, w.reshape(-1), logits, lab.reshape(-1))
    with pytest.raises(RuntimeError):
        C.headk_bwd(*bargs, big, da, part, gw, gb, 1.0, class_weights=torch.ones(K - 1, device="cuda"))
    with pytest.raises(RuntimeError):
        C.headk_bwd(*bargs, small, da, part, gw, gb, 1.0, dice_w=1.0)
    torch.cuda.synchronize()
    assert torch.count_nonzero(logits) == 0 and torch.count_nonzero(loss) == 0  # nothing ran
    assert (da == 7).all() and (gw == 7).all() and (gb == 7).all()
