"""``seg_confusion`` (csrc/seg_metrics.hip) bitwise against ``confusion_reference``: integer counts, so
every comparison is ``torch.equal`` on int64."""
import pytest
import torch

from seg_cases import planted_case

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def run(C, x, t, K, thr=0.0, max_blocks=0, counts=None):
    from robotic_discovery_platform_amd.train.metrics import confusion_size
    if counts is None:
        counts = torch.zeros(confusion_size(K), dtype=torch.int64, device=DEV)
    C.seg_confusion(x.to(DEV), t.to(DEV), K, counts, thr, max_blocks)
    return counts


def ref(x, t, K, thr=0.0):
    from robotic_discovery_platform_amd.train.metrics import confusion_reference
    return confusion_reference(x, t, K, thr)


# M = 35: less than one wave, ragged; 960: 15 groups of 64 (four waves of one block, the last one
# ragged); 1500 with the grid capped at 2: the cap above the natural grid. The last two make the
# grid-stride loop run more than once, with a ragged last pass: a block takes ``seg_confusion_block_pixels``
# (4096) pixels per pass, so 9000 on one block is three passes (the last of 808 pixels: waves with full
# groups, one ragged group, waves with nothing) and 20000 on two blocks is three passes with only
# block 0 in the last one.
@pytest.mark.parametrize("M,max_blocks", [(35, 0), (960, 0), (1500, 2), (9000, 1), (20000, 2)])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_counts_equal_reference(C, K, M, max_blocks):
    if M >= 9000:
        px = C.seg_confusion_block_pixels()
        assert M > 2 * max_blocks * px and M % (max_blocks * px) % 64 != 0  # three passes, a ragged last group
    thr = 0.25 if K == 1 else 0.0  # K == 1: planted logits sit exactly at the (non-zero) threshold
    x, t = planted_case(K, M, seed=M, thr=thr)
    got = run(C, x, t, K, thr, max_blocks).cpu()
    exp = ref(x, t, K, thr)
    assert torch.equal(got, exp)
    assert int(got.sum()) == M


def test_real_launch_geometry_over_one_pass(C):
    """No cap: more pixels than one pass of the full grid (256 blocks), so every block strides."""
    K = 3
    M = C.seg_confusion_blocks(1 << 30) * C.seg_confusion_block_pixels() + 12345
    assert C.seg_confusion_blocks(M) * C.seg_confusion_block_pixels() < M
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(-4, 5, (M * K,), generator=g).float() / 4)
    t = torch.randint(0, 4, (M,), generator=g).to(torch.uint8)  # label 3 >= K: ignored
    got = run(C, x, t, K).cpu()
    assert torch.equal(got, ref(x, t, K)) and int(got.sum()) == M


def test_mostly_one_bin_map(C):
    """99 % background predicted as background: nearly every wave retires in one round of the ballot loop."""
    K, M = 3, 8192
    g = torch.Generator().manual_seed(3)
    x = torch.zeros(M, K)
    x[:, 0] = 1.0
    t = torch.zeros(M, dtype=torch.uint8)
    odd = torch.rand(M, generator=g) < 0.01
    t[odd] = torch.randint(1, 3, (int(odd.sum()),), generator=g, dtype=torch.int64).to(torch.uint8)
    x[torch.rand(M, generator=g) < 0.01, 2] = 2.0
    got = run(C, x.reshape(-1), t, K).cpu()
    assert torch.equal(got, ref(x.reshape(-1), t, K))
    assert int(got[0]) > 0.97 * M


def test_every_lane_a_bin_of_its_own(C):
    """K = 8: lane i of each wave has truth i // 8 and prediction i % 8 -- 64 bins, 64 rounds per wave."""
    K, M = 8, 320
    i = torch.arange(M) % 64
    t = (i // 8).to(torch.uint8)
    x = torch.zeros(M, K)
    x[torch.arange(M), i % 8] = 1.0
    got = run(C, x.reshape(-1), t, K).cpu()
    assert torch.equal(got, ref(x.reshape(-1), t, K))
    assert got[:-1].tolist() == [5] * 64 and int(got[-1]) == 0


@pytest.mark.parametrize("K", [1, 3])
def test_accumulates_and_stays_inside_its_slots(C, K):
    from robotic_discovery_platform_amd.train.metrics import confusion_size
    nb = confusion_size(K)
    x, t = planted_case(K, 777, seed=9)
    buf = torch.full((nb + 16,), -12345, dtype=torch.int64, device=DEV)
    counts = buf[8:8 + nb]
    counts.zero_()
    run(C, x, t, K, counts=counts)
    once = counts.cpu().clone()
    run(C, x, t, K, counts=counts)
    assert torch.equal(once, ref(x, t, K))
    assert torch.equal(counts.cpu(), 2 * once)
    assert bool((buf[:8] == -12345).all()) and bool((buf[8 + nb:] == -12345).all())


def test_bad_arguments_raise(C):
    x, t = planted_case(3, 64)
    x, t = x.to(DEV), t.to(DEV)
    good = torch.zeros(10, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        C.seg_confusion(x, t, 3, torch.zeros(10, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        C.seg_confusion(x, t, 3, torch.zeros(9, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        C.seg_confusion(x[:-3], t, 3, good)
    with pytest.raises(RuntimeError):
        C.seg_confusion(x, t.float(), 3, good)  # K >= 2 takes u8 labels
    with pytest.raises(RuntimeError):
        C.seg_confusion(x[:64], t, 1, torch.zeros(5, dtype=torch.int64, device=DEV))  # K == 1 takes a float target
    with pytest.raises(RuntimeError):
        C.seg_confusion(x.double(), t, 3, good)
    with pytest.raises(RuntimeError):
        C.seg_confusion(x, t, 9, good)
    with pytest.raises(RuntimeError):
        C.seg_confusion(x, t.cpu(), 3, good)
    torch.cuda.synchronize()
    assert int(good.sum()) == 0  # nothing was launched


def test_column_sums_agree_with_serving(C):
    """K = 3: the predicted-class totals of one frame's confusion matrix are the pixel counts of
    ``headk_mask`` for each class, on the same activations and weights."""
    from robotic_discovery_platform_amd.models.unet import UNetNative
    torch.manual_seed(0)
    nat = UNetNative(3, 3, depth=2, device=torch.device(DEV)).eval()
    with torch.no_grad():
        nat.store.view("outc.conv.bias").fill_(0.0)
    H = W = 64
    ex = nat.executor(1, H, W, training=False, loss="ce")
    g = torch.Generator().manual_seed(1)
    ex.set_input(torch.rand(1, 3, H, W, generator=g).to(DEV), torch.randint(0, 3, (1, H, W), generator=g).to(DEV))
    ex.forward()
    counts = torch.zeros(10, dtype=torch.int64, device=DEV)
    C.seg_confusion(ex.logits, ex.target, 3, counts)
    cols = counts[:9].view(3, 3).sum(0).cpu()
    st = nat.store
    mask = torch.empty(H * W, dtype=torch.uint8, device=DEV)
    served = []
    for cls in range(3):
        C.headk_mask(ex.final, st.flat_slice("outc.conv.weight"), st.view("outc.conv.bias"), cls, mask)
        served.append(int(mask.sum()))
    assert cols.tolist() == served and sum(served) == H * W and int(counts[9]) == 0
