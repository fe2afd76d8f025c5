"""The lattice helper (tests/lattice.py) on the CPU: every case of tests/test_conv_exact_gpu.py builds its
inputs and fp64 reference here and must meet the preconditions under which bitwise equality is a sound
demand -- so a broken case shows without a GPU. The references of the longest-K cases are formed for
their first output channels only (same inputs, same per-channel conditions)."""
import pytest
import torch

import lattice as L

COUT_LIMIT = 64  # cases above WORK_LIMIT multiply-adds reference this many output channels here
WORK_LIMIT = 1 << 29


def _limit(work):
    return COUT_LIMIT if work > WORK_LIMIT else None


def test_generators_are_seeded_and_in_range():
    a = L.ternary((64, 33), 0.3, L.generator(5))
    b = L.ternary((64, 33), 0.3, L.generator(5))
    assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    assert set(a.float().unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.2 < (a != 0).float().mean().item() < 0.4
    c = L.small_ints((4096,), L.generator(6))
    assert set(c.float().unique().tolist()) == {float(v) for v in range(-3, 4)}
    assert torch.equal(c, L.small_ints((4096,), L.generator(6)))
    s = L.pow2_signed(64, L.generator(7))
    assert (s > 0).any() and (s < 0).any()
    m, e = torch.frexp(s.abs())
    assert torch.equal(m, torch.full_like(m, 0.5))  # exact powers of two


def test_expected_bf16_rounds_ties_to_even():
    ref = torch.tensor([255.0, 256.0, 257.0, 259.0, 261.0, -257.0, -259.0, 511.0, 513.0, 514.0, 515.0], dtype=torch.float64)
    exp = torch.tensor([255.0, 256.0, 256.0, 260.0, 260.0, -256.0, -260.0, 512.0, 512.0, 512.0, 516.0])
    assert torch.equal(L.expected_bf16(ref).float(), exp)
    assert L.true_ties(ref) == 6  # 257, 259, 261, -257, -259, 511


def test_preconditions_reject_broken_cases():
    ok = torch.tensor([[1.0, -256.0], [3.0, 0.0]], dtype=torch.float64)
    L.assert_exact_class(ok)
    with pytest.raises(AssertionError):
        L.assert_exact_class(torch.tensor([[257.0]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        L.assert_exact_class(torch.tensor([[0.5]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        L.assert_exact_class(torch.full((70000, 1), 16.0, dtype=torch.float64))  # sum y^2 = 2^24 + ...
    with pytest.raises(AssertionError):
        L.assert_rounding_class(ok)  # no ties
    with pytest.raises(AssertionError):
        L.assert_f32_sums(torch.full((1 << 20, 1), 16.5, dtype=torch.float64), "t")
    L.assert_f32_sums(torch.full((1 << 10, 1), 16.5, dtype=torch.float64), "t")


def test_embed_and_guard_check():
    t = L.ternary((2, 3, 5, 16), 0.5, L.generator(1))
    flat, view = L.embed(t, t.shape, 8, 24, "cpu")
    assert view.stride() == (3 * 5 * 48, 5 * 48, 48, 1) and view.data_ptr() % 16 == 0
    assert torch.equal(view, t) and L.outside_view_intact(flat, view)
    view.fill_(2.0)
    assert L.outside_view_intact(flat, view)
    for idx in (0, L.GUARD - 1, L.GUARD + 7, L.GUARD + 8 + 16, flat.numel() - 1):  # guards and both pads
        bad = flat.clone()
        bad[idx] = 0.0
        assert not L.outside_view_intact(bad, bad[L.GUARD:-L.GUARD].view(2, 3, 5, 48)[..., 8:24])
    f32, v32 = L.embed(None, (1, 1, 1, 24), 0, 8, "cpu", dtype=torch.float32, fill=-7.0)
    assert L.outside_view_intact(f32, v32, fill=-7.0)


@pytest.mark.parametrize("c", L.FWD_CASES + L.EVAL_CASES, ids=lambda c: c.name)
def test_conv_case_preconditions(c):
    x, w, ref = L.conv_data(c, _limit(c.M * c.K * c.Cout))
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and ref.dtype == torch.float64
    assert x.abs().max().item() <= (1 if c.cls == "exact" else c.amax)
    L.check_conv_case(c, ref)
    if c.split:
        assert 0 < c.split < c.Cout
    if c.pool:
        assert c.evalmode and c.H % 2 == 0 and c.W % 2 == 0
    if c.evalmode:  # what the GPU test will demand is representable: fp32 exactly, then one RNE
        e = L.eval_ref(c, ref)
        assert torch.equal(e.float().double(), e)


@pytest.mark.parametrize("c", L.DGRAD_CASES, ids=lambda c: c.name)
def test_dgrad_case_preconditions(c):
    Cdx = c.Cs + c.Cu
    dy, w, dx = L.dgrad_data(c.N, c.H, c.W, c.Cdy, Cdx, c.seed, _limit(c.N * c.H * c.W * 9 * c.Cdy * Cdx))
    L.assert_exact_class(dx)
    assert L.dgrad_weight(w).shape == (Cdx, 9 * c.Cdy)


@pytest.mark.parametrize("b", L.BNRED_CASES, ids=lambda b: b.name)
def test_bnred_case_preconditions(b):
    dy, w, dx, y, coef, sums, terms = L.bnred_data(b, _limit(b.N * b.H * b.W * 9 * b.Cdy * b.Cdx))
    L.check_bnred_case(b, dx, terms)
    mean, inv, scale, shift = coef.view(4, b.Cdx)
    assert torch.equal(mean, mean.round()) and torch.equal(shift, shift.round())
    for v in (inv, scale.abs()):
        assert torch.equal(torch.frexp(v)[0], torch.full_like(v, 0.5))
    assert torch.equal(sums.float().double(), sums)  # the demanded sums are fp32 values


@pytest.mark.parametrize("c", L.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_case_preconditions(c):
    x, dy, dw = L.wgrad_data(c)
    L.check_wgrad_ref(dw, c.N * c.H * c.W)
    assert dw.numel() == c.Cout * 9 * (3 if c.packed else c.C1 + c.C2)


@pytest.mark.parametrize("c", L.FIRSTBN_CASES, ids=lambda c: c.name)
def test_firstbn_case_preconditions(c):
    x, da, y, coef, coef2, dz, dw = L.firstbn_data(c)
    assert (c.N * c.H * c.W) % 64 == 0  # the fused kernel's shape condition
    L.check_firstbn_case(dz, dw)
    assert torch.equal(dw.float().double(), dw)


@pytest.mark.parametrize("c", L.UPT_FWD_CASES + L.UPT_SMALL_CASES, ids=lambda c: c.name)
def test_upT_fwd_case_preconditions(c):
    d = L.upT_data(c, "fwd")
    L.assert_exact_class(d["u"])
    inside = torch.zeros(c.H2, c.W2, dtype=torch.bool)
    inside[c.oy:c.oy + 2 * c.h, c.ox:c.ox + 2 * c.w] = True
    assert (d["u"][:, ~inside] == 0).all()


@pytest.mark.parametrize("c", L.UPT_SMALL_CASES, ids=lambda c: c.name)
def test_upT_bwd_case_preconditions(c):
    d = L.upT_data(c, "bwd")
    L.assert_exact_class(d["dx"])
    M = c.N * c.h * c.w
    assert d["dW"].abs().max().item() <= M and d["db"].abs().max().item() <= 4 * M
    assert torch.equal(d["dW"], d["dW"].round())
    # the window layout is the transposed conv as one GEMM: u = x @ Wfwd^T + bias
    wf, wd = L.upT_weights(d["W"])
    yT = d["x"].double().reshape(M, c.Cin) @ wf.double().t() + d["bias"].double().repeat(4)
    assert torch.equal(yT.reshape(c.N, c.h, c.w, 4 * c.C), L.upT_window(c, d["u"]))
    assert torch.equal(L.upT_window(c, d["du"].double()).reshape(M, -1) @ wd.double().t(), d["dx"].reshape(M, c.Cin))


@pytest.mark.parametrize("c", L.UPT_DGRAD_CASES, ids=lambda c: c.name)
def test_upT_dgrad_case_preconditions(c):
    L.assert_exact_class(L.upT_data(c, "dx", COUT_LIMIT)["dx"])


# -- the fp64 references against int64 einsums (independent of conv2d / autograd) ------------------

def _unfold_int(x):  # [N,H,W,C] int64 -> [N,H,W,9,C], zero 'same' padding
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.int64)
    xp[:, 1:-1, 1:-1] = x
    return torch.stack([xp[:, r:r + H, s:s + W] for r in range(3) for s in range(3)], 3)


@pytest.mark.parametrize("c", [L.FWD_CASES[0], L.FWD_CASES[1], L.FWD_CASES[6]], ids=lambda c: c.name)
def test_conv_reference_vs_int64(c):
    x, w, ref = L.conv_data(c)
    cols = _unfold_int(x.long())
    wi = w.long().permute(0, 2, 3, 1).reshape(c.Cout, 9, -1)
    y = torch.einsum("nhwtc,otc->nhwo", cols, wi)
    assert torch.equal(ref, y.double())
    assert torch.equal(L.ohwi(w).long(), wi.reshape(c.Cout, -1))


def test_first_layer_reference_vs_int64():
    c = L.FWD_CASES[[k.name for k in L.FWD_CASES].index("first")]
    x, w, ref = L.conv_data(c)
    y = torch.einsum("nhwtc,otc->nhwo", _unfold_int(x.long()), w.long().permute(0, 2, 3, 1).reshape(64, 9, 3))
    assert torch.equal(ref, y.double())
    x8, wp = L.pack_first(x, w)
    assert x8.shape[-1] == 8 and wp.shape == (64, 128) and (x8[..., 3:] == 0).all()


def test_dgrad_and_wgrad_references_vs_int64():
    c = L.DGRAD_CASES[0]
    Cdx = c.Cs + c.Cu
    dy, w, dx = L.dgrad_data(c.N, c.H, c.W, c.Cdy, Cdx, c.seed)
    # dX = conv(dY, flip(W)^T): the kernel's weight layout [Cdx][tap][Cdy]
    wt = L.dgrad_weight(w).long().reshape(Cdx, 9, c.Cdy)
    assert torch.equal(dx, torch.einsum("nhwtc,otc->nhwo", _unfold_int(dy.long()), wt).double())
    g = L.WGRAD_CASES[0]
    x, dyw, dw = L.wgrad_data(g)
    ref = torch.einsum("nhwtc,nhwo->otc", _unfold_int(x.long()), dyw.long())
    assert torch.equal(dw, ref.reshape(-1).double())


def test_case_names_are_unique():
    for table in (L.FWD_CASES + L.EVAL_CASES, L.DGRAD_CASES, L.BNRED_CASES, L.WGRAD_CASES, L.FIRSTBN_CASES,
                  L.UPT_FWD_CASES + L.UPT_DGRAD_CASES + L.UPT_SMALL_CASES):
        names = [c.name for c in table]
        assert len(names) == len(set(names))
