"""The row-ring conv's fused K-class serving head (csrc/conv_ring.hip HK variant, ``conv_headk_mask``): the last
conv (64 -> 64, BN fold + ReLU) + 1x1 head + arg-max class == cls in one launch, BIT FOR BIT the mask of
``conv_fwd`` (eval coefficients, ReLU) followed by ``headk_mask`` -- both run the head code of
csrc/head_multi_dev.h on the same bf16 activations."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7
GUARD = 256  # bytes past N*H*W that must keep the sentinel


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def bf(x):
    return x.to(torch.bfloat16)


def ohwi(w):  # [Cout,Cin,kh,kw] -> [Cout, kh*kw*Cin]
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _conv_inputs(C, N, H, W, seed=10):
    """Random bf16 input and weights and eval BN coefficients, as test_conv_head_mask_fused builds them."""
    torch.manual_seed(seed)
    dev = "cuda"
    x = bf(torch.randn(N, H, W, 64, device=dev))
    w = bf(torch.randn(64, 64, 3, 3, device=dev) / math.sqrt(9 * 64))
    wk = ohwi(w).contiguous()
    g, b = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev) * 0.5
    rm, rv = torch.randn(64, device=dev) * 0.1, torch.rand(64, device=dev) + 0.5
    coef = torch.zeros(4 * 64, device=dev)
    C.bn_eval_coef(g, b, rm, rv, 1e-5, coef)
    return x, wk, coef


def _head(K, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed + K)
    hw = torch.randn(K, 64, device="cuda", generator=gen) * 0.3
    hb = torch.randn(K, device="cuda", generator=gen) * 0.1  # non-zero bias
    return hw, hb


def _mask_buf(M):
    return torch.full((M + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def _pair(C, x, wk, coef, hw, hb, cls, a=None):
    """conv_fwd (eval, ReLU) + headk_mask; ``a``: the stored activation, computed once per shape"""
    N, H, W, _ = x.shape
    if a is None:
        a = torch.empty(N, H, W, 64, dtype=torch.bfloat16, device="cuda")
        C.conv_fwd(x, None, wk, 9, 0, a, None, None, C.CONV_AUTO, coef, 1)
    ref = torch.full((N * H * W,), SENTINEL, dtype=torch.uint8, device="cuda")
    C.headk_mask(a, hw.reshape(-1), hb, cls, ref)
    return ref, a


# (1, 2, 64): one block, one step, only the final-barrier finish; (2, 6, 128): two column segments, image
# top and bottom inside a block's neighbourhood; (1, 256, 256): 512 row pairs, 2 steps per block, both
# parities of the LDS tile; (1, 256, 512): 4 steps per block, the ks >= 2 wait counts; (1, 260, 256): 520
# pairs at 3 per block, the last block runs a single step
SHAPES = [(1, 2, 64), (2, 6, 128), (1, 256, 256), (1, 256, 512), (1, 260, 256)]


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_fused_mask_is_bitwise_the_pair(C, N, H, W):
    x, wk, coef = _conv_inputs(C, N, H, W)
    M = N * H * W
    a = None
    for K in (2, 3, 5, 8):
        hw, hb = _head(K)
        for cls in range(K):
            ref, a = _pair(C, x, wk, coef, hw, hb, cls, a)
            got = _mask_buf(M)
            assert C.conv_headk_mask(x, wk, coef, hw.reshape(-1), hb, cls, got)
            torch.cuda.synchronize()
            assert (got[M:] == SENTINEL).all(), (K, cls)
            assert (got[:M] <= 1).all(), (K, cls)
            ndiff = int((got[:M] != ref).sum())
            assert torch.equal(got[:M], ref), (K, cls, ndiff)


def test_planted_exact_ties_go_to_the_lowest_class(C):
    N, H, W = 1, 64, 128
    x, wk, coef = _conv_inputs(C, N, H, W, seed=12)
    M = N * H * W
    hw, hb = _head(4)
    hw[2] = hw[1]
    hb[2] = hb[1]  # logits 1 and 2 are bitwise equal on every pixel
    got2 = _mask_buf(M)
    assert C.conv_headk_mask(x, wk, coef, hw.reshape(-1), hb, 2, got2)
    assert int(got2[:M].sum()) == 0 and (got2[M:] == SENTINEL).all()
    ref1, _ = _pair(C, x, wk, coef, hw, hb, 1)
    got1 = _mask_buf(M)
    assert C.conv_headk_mask(x, wk, coef, hw.reshape(-1), hb, 1, got1)
    assert torch.equal(got1[:M], ref1)
    assert int(ref1.sum()) > 0  # class 1 does win pixels: the tie rule was exercised


def test_not_applicable_and_bad_arguments(C):
    _, wk, coef = _conv_inputs(C, 1, 2, 64)
    hw, hb = _head(3)
    dev = "cuda"
    got = _mask_buf(64 * 64)
    # W % 64 != 0, odd H, strided input view: nothing launched, the caller falls back
    xs = bf(torch.randn(1, 16, 24, 64, device=dev))
    assert not C.conv_headk_mask(xs, wk, coef, hw.reshape(-1), hb, 1, got)
    xo = bf(torch.randn(1, 3, 64, 64, device=dev))
    assert not C.conv_headk_mask(xo, wk, coef, hw.reshape(-1), hb, 1, got)
    xv = bf(torch.randn(1, 4, 64, 128, device=dev))[..., :64]
    assert not xv.is_contiguous()
    assert not C.conv_headk_mask(xv, wk, coef, hw.reshape(-1), hb, 1, got)
    torch.cuda.synchronize()
    assert (got == SENTINEL).all()
    x = bf(torch.randn(1, 2, 64, 64, device=dev))
    for K in (1, 9):  # head shapes outside 2..8
        with pytest.raises(RuntimeError):
            C.conv_headk_mask(x, wk, coef, torch.zeros(K * 64, device=dev), torch.zeros(K, device=dev), 0, got)
    for cls in (-1, 3):
        with pytest.raises(RuntimeError):
            C.conv_headk_mask(x, wk, coef, hw.reshape(-1), hb, cls, got)
    torch.cuda.synchronize()
    assert (got == SENTINEL).all()


def _scene_input(size):
    """A synthetic scene at the executor's size (an image with structure: a random one gives one class everywhere)"""
    from robotic_discovery_platform_amd.data.image_io import bgr2rgb, resize_area
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    img = resize_area(bgr2rgb(make_scene(2).color), (size, size)).astype("float32") / 255.0
    return torch.from_numpy(img).permute(2, 0, 1)[None].contiguous().cuda()


def _executor_mask(nat, size, cls, monkeypatch, fused_env):
    if fused_env is None:
        monkeypatch.delenv("RDP_SERVE_FUSED_HEADK", raising=False)
    else:
        monkeypatch.setenv("RDP_SERVE_FUSED_HEADK", fused_env)
    ex = nat.executor(1, size, size, training=False, loss="ce" if nat.n_classes > 1 else "bce")
    ex.set_input(_scene_input(size))
    st = nat.store
    mask = torch.full((size * size,), SENTINEL, dtype=torch.uint8, device="cuda")
    if nat.n_classes > 1:
        mh = (st.flat_slice("outc.conv.weight"), st.view("outc.conv.bias"), cls, mask)
    else:
        mh = (st.view("outc.conv.weight").reshape(-1), st.view("outc.conv.bias"), 0.0, mask)
    ex.forward(head=False, mask_head=mh)
    torch.cuda.synchronize()
    return mask, ex.mask_head_fused


@pytest.mark.parametrize("size", [64, 256])
def test_executor_takes_the_fused_head(monkeypatch, size):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    torch.manual_seed(0)
    nat = UNetNative(3, 3, device=torch.device("cuda")).eval()
    with torch.no_grad():
        nat.store.view("outc.conv.bias").fill_(0.0)  # as tests/test_serve_multiclass_gpu.py: every class gets pixels
    total = torch.zeros(size * size, dtype=torch.int32, device="cuda")
    for cls in range(3):
        fused, was_fused = _executor_mask(nat, size, cls, monkeypatch, None)
        assert was_fused is True
        plain, was_fused0 = _executor_mask(nat, size, cls, monkeypatch, "0")
        assert was_fused0 is False
        assert (fused <= 1).all()
        assert torch.equal(fused, plain), int((fused != plain).sum())
        print(f"size {size} class {cls}: {int(plain.sum())} pixels")
        total += plain
    assert (total == 1).all()  # exactly one class wins each pixel
    if size == 256:
        assert 0 < int(plain.sum()) < plain.numel()


def test_executor_falls_back_where_the_ring_does_not_apply(monkeypatch):
    """A last conv the ring kernel does not take keeps the separate launch and gives the same mask. (UNetNative
    builds base_width = 64 only, so the case is a 48 x 48 executor: W % 64 != 0.)"""
    from robotic_discovery_platform_amd.models.unet import UNetNative
    with pytest.raises(NotImplementedError):
        UNetNative(3, 3, device=torch.device("cuda"), base_width=32)
    torch.manual_seed(0)
    nat = UNetNative(3, 3, device=torch.device("cuda")).eval()
    a, fa = _executor_mask(nat, 48, 1, monkeypatch, None)
    b, fb = _executor_mask(nat, 48, 1, monkeypatch, "0")
    assert fa is False and fb is False
    assert torch.equal(a, b) and (a <= 1).all()
    # and it is headk_mask's mask of the stored activation
    ex = nat.executor(1, 48, 48, training=False, loss="ce")
    ex.set_input(_scene_input(48))
    ex.forward(head=False)
    from robotic_discovery_platform_amd.ops import native
    exp = torch.empty(48 * 48, dtype=torch.uint8, device="cuda")
    native().headk_mask(ex.final, nat.store.flat_slice("outc.conv.weight"), nat.store.view("outc.conv.bias"), 1, exp)
    assert torch.equal(a, exp)


def test_one_class_path_and_flag_unchanged(monkeypatch):
    from robotic_discovery_platform_amd.models.unet import UNetNative
    torch.manual_seed(0)
    nat = UNetNative(3, 1, device=torch.device("cuda")).eval()
    a, fa = _executor_mask(nat, 64, 0, monkeypatch, None)
    b, fb = _executor_mask(nat, 64, 0, monkeypatch, "0")  # the K-class switch does not touch the one-class head
    assert fa is True and fb is True
    assert torch.equal(a, b) and (a <= 1).all()
