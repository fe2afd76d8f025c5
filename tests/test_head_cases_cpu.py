"""The loss-head cases of tests/head_cases.py on the CPU: every case of tests/test_head_exact_gpu.py is checked
here against the preconditions under which its demands are sound -- exact logits, the u slots and grid-stride
passes its M reaches, the share of elements near a bf16 rounding tie, logits that leave the gradient checks
something to see -- from the reference and the transcribed launcher formulas alone, without the native
extension."""
import math

import pytest
import torch

import head_cases as H
import lattice as L

CHUNK = 1 << 16  # pixels per slice of the [M, 64] checks


def _ids(c):
    return c.name


# -- the launchers' grid arithmetic -------------------------------------------------------------------

def test_grid_formulas():
    assert [H.blocks_for(M) for M in (1, 32, 33, 35, 960, 65536, 65537, 1 << 22)] == [1, 1, 2, 2, 30, 2048, 2048, 2048]
    assert H.stride(960) == 960 and H.stride(2016) == 2016 and H.stride(1 << 20) == 65536
    # up to 65,536 pixels the stride covers M: only slot u = 0 ever holds a pixel
    for M in (35, 960, 2016, 65535, 65536):
        assert H.slot_fill(M) == [M, 0, 0, 0] and H.passes(M) == 1 and H.mask_trips(M) == 1
    assert H.slot_fill(65537) == [65536, 1, 0, 0]
    assert H.slot_fill(262144) == [65536] * 4 and H.passes(262144) == 1 and H.passes(262145) == 2
    assert H.slot_fill(262145, 1) == [1, 0, 0, 0]
    # the benchmark's flagship step, batch 64 of 256^2: 16 passes
    assert H.passes(64 * 256 * 256) == 16 and H.mask_trips(64 * 256 * 256) == 64
    # head_bn_bwd_apply: ceil(M / 128) blocks, so all four slots are in use from M > 96 on
    assert [H.apply_blocks(M) for M in (35, 128, 129, 1229, H.M_U1)] == [1, 1, 2, 10, 513]
    assert H.apply_slot_fill(35) == [32, 3, 0, 0] and H.apply_slot_fill(1229) == [320, 320, 320, 269]
    assert H.apply_slot_fill(H.M_U1) == [16416, 16416, 16416, 16325]
    assert H.chain(960) == 13 and H.chain(H.M_PASS2) == 17 and H.chain_final(H.M_PASS2) == 17 + 8 + 10


@pytest.mark.parametrize("name", list(H.M_CASES), ids=str)
def test_regime_sizes(name):
    H.check_regime(name, H.M_CASES[name])


def test_cases_cover_the_issue_grid():
    for table in (H.BIN_CASES, H.K_CASES):
        assert {c.M for c in table} == set(H.M_CASES.values())
        assert {c.pitch for c in table} == {64, 128, 192} and all(c.off % 8 == 0 and c.pads[1] >= 0 for c in table)
        assert len({c.name for c in table}) == len(table)
    assert {c.targets for c in H.BIN_CASES} == {"binary", "soft", "zero"}
    assert any(c.targets == "zero" and H.passes(c.M) > 1 for c in H.BIN_CASES)
    assert any(c.labels == "ignored" and H.passes(c.M) > 1 for c in H.K_CASES)
    for K in (2, 3, 5, 8):  # both paddings of pow2_classes; each K below and above the one-slot regime
        ms = {c.M for c in H.K_CASES if c.K == K}
        assert min(ms) <= H.M_U0 and max(ms) > 65536
    ms = [c.M for c in H.APPLY_CASES]
    assert H.M_TINY in ms and any(M % 128 % 2 == 1 and M < 4096 for M in ms) and max(ms) >= H.LARGE_M
    for M in ms[1:]:
        assert all(f > 0 for f in H.apply_slot_fill(M)) and H.apply_slot_fill(M)[3] % H.GROUPS
    assert set(H.DICE_WS) == {0.0, 1.0, 2.5}
    assert {(w, d) for _, w, d in H.K_MODES} == {(False, 0.0), (True, 0.0), (False, 1.0), (True, 2.5)}


def test_intrinsic_allowance_is_far_below_half_a_bf16_ulp():
    worst = max(v for _, v in H.EXPF_MEASURED)
    assert 2 * worst * H.U32 < 2.0 ** -9 / 64 and H.LOG1P_REL < 2.0 ** -9 / 64 and H.LOGF_ABS < 2.0 ** -9 / 64
    assert [e for e, _ in H.EXPF_MEASURED] == sorted(e for e, _ in H.EXPF_MEASURED)
    x = torch.tensor([0.0, -1.0, -1.5, -40.0, -79.0], dtype=torch.float64)
    assert torch.equal(H.expf_rel(x), 2 * H.U32 * torch.tensor([1.58, 1.58, 2.56, 55.71, 62.99], dtype=torch.float64))


# -- operands ------------------------------------------------------------------------------------------

def _is_pow2(v):
    return torch.equal(torch.frexp(v.abs())[0], torch.full_like(v, 0.5))


def _check_logits_exact(a64, w, b, x, values=H.W_VALUES, q=32):
    """Every partial sum of a logit is a multiple of 1 / q below 2^24 / q: exact in fp32 in any order."""
    a, w = a64.reshape(-1, H.HEAD_C), w.double().reshape(-1, H.HEAD_C)
    assert L.bf16_exact(a64) and torch.equal(a * 4, (a * 4).round()) and a.min().item() >= 0
    assert set(w.unique().tolist()) <= set(values) and torch.equal(b.double() * 8, (b.double() * 8).round())
    worst = (a.abs() @ w.abs().t()).max().item() + b.abs().max().item()
    assert worst * q < L.F32_EXACT
    assert torch.equal(x * q, (x * q).round()) and L.f32_exact(x)


def _check_coef(coef):
    mean, inv, sc, sh = coef.view(4, H.HEAD_C)
    assert torch.equal(mean, mean.round()) and torch.equal(sh, sh.round()) and _is_pow2(inv) and _is_pow2(sc)
    assert (sc > 0).any() and (sc < 0).any()


@pytest.mark.parametrize("c", H.BIN_CASES + H.APPLY_CASES, ids=_ids)
def test_binary_case_preconditions(c):
    d = H.bin_data(c)
    y, coef, w, b, t = d["y"], d["coef"], d["w"], d["b"], d["t"]
    _check_coef(coef)
    assert torch.equal(y.double(), y.double().round()) and y.abs().max().item() <= H.HOT_AMP
    # the BN + ReLU activation, the ReLU mask and xhat are exact: proven on every (value, channel) pair
    v = torch.arange(-H.HOT_AMP, H.HOT_AMP + 1).to(L.BF16).view(-1, 1).expand(-1, H.HEAD_C)
    tab = H.bn_apply64(v, coef)
    assert L.bf16_exact(tab) and torch.equal(tab * 4, (tab * 4).round()) and (tab == 0).any() and (tab > 0).any()
    xh = H.xhat(v, coef)
    assert torch.equal(xh * 4, (xh * 4).round()) and xh.abs().max().item() <= 2 * (H.HOT_AMP + 2)
    assert torch.equal(d["a"].double(), d["a64"]) and torch.equal(d["a64"], H.bn_apply64(y, coef))
    x = H.logits64(d["a64"], w, b)
    _check_logits_exact(d["a64"], w, b, x)
    assert (w[1:] != w[:-1]).all()                       # a neighbour's weight is always a different weight
    assert set(w.tolist()) == set(H.W_VALUES)
    # targets: dyadic, their sum exact in fp32
    want = {"binary": {0.0, 1.0}, "soft": {0.0, 0.25, 1.0}, "zero": {0.0}}[c.targets]
    assert set(t.unique().tolist()) == want and t.sum().item() * 4 < L.F32_EXACT
    # the logits leave most pixels unsaturated and saturate a deliberate minority, some out to |x| ~ 40
    ax = x.abs()
    assert (ax < 8).double().mean().item() >= 0.9
    assert (ax > 16).double().mean().item() >= 0.01
    assert 24 <= ax.max().item() <= 48
    if c.M >= H.M_U0:
        assert ax.max().item() >= 32 and (x > 16).any() and (x < -16).any()


def _g_tie_share(r, d):
    """Share of the elements of dlogit * w within slop of a bf16 rounding tie, in slices of CHUNK pixels."""
    n = 0
    for p in range(0, r["M"], CHUNK):
        ref, slop = H.outer_bounds(r["dx"][p:p + CHUNK], r["dx_slop"][p:p + CHUNK], d["w"])
        n += H.tie_share(ref, slop) * ref.numel()
    return n / (r["M"] * H.HEAD_C)


@pytest.mark.parametrize("dice_w", H.DICE_WS)
@pytest.mark.parametrize("c", H.BIN_CASES + H.APPLY_CASES, ids=_ids)
def test_binary_tie_share_and_slop(c, dice_w):
    """At most 1 % of the elements of bf16(dlogit * w) may lie within slop of a rounding tie (where the BN-fused
    checks accept either neighbour), and the slop stays below a tenth of half a bf16 ulp at the pixels with
    |x| < 4, at least 60 % of them -- so the per-element bound is the bf16 rounding, not the allowance."""
    d = H.bin_data(c)
    x = H.logits64(d["a64"], d["w"], d["b"])
    for gscale in (1.0, 0.5, 0.25):
        r = H.bin_ref(x, d["t"], dice_w, gscale=gscale)
        assert _g_tie_share(r, d) <= 0.01
    mid = x.abs() < 4   # beyond, sigmoid(x) - 1 cancels and only the absolute bound can hold
    assert mid.double().mean().item() >= 0.6
    rel = r["dx_slop"][mid] / (r["dx"][mid].abs() * 2.0 ** -9)
    assert rel.max().item() < 0.1 if c.targets != "soft" else rel.median().item() < 0.01
    assert math.isfinite(r["loss"][0].item())


@pytest.mark.parametrize("c", H.APPLY_CASES, ids=_ids)
def test_apply_case_coefficients(c):
    """coef2 is dyadic, dy = A g + B y + K is exact in fp32 given g, and B y + K does not swamp g: the gradient
    moves dy's bf16 value at a stated share of the elements."""
    d = H.bin_data(c)
    coef2 = H.bwd_coef2(c.M, L.generator(33000 + c.seed))
    A, B, K = coef2.view(3, H.HEAD_C).double()
    q = 2.0 ** -(math.ceil(math.log2(c.M)) + 4)
    assert _is_pow2(A) and (A > 0).any() and (A < 0).any()
    assert torch.equal(B / q, (B / q).round()) and torch.equal(K / q, (K / q).round()) and (B != 0).any() and (K != 0).any()
    x = H.logits64(d["a64"], d["w"], d["b"])
    r = H.bin_ref(x, d["t"], 0.0, gscale=0.5)
    f = H.bn_fused_ref(r, d["y"], d["coef"], d["w"])
    rest = B * d["y"].double().view(-1, H.HEAD_C) + K
    assert L.f32_exact(rest)
    moved = ((A * f["g_lo"] + rest).float().to(L.BF16) != rest.float().to(L.BF16)).double().mean().item()
    assert moved > 0.15 and 0.2 < f["kept_share"] < 0.8 and f["amb_share"] <= 0.01


# -- K-class --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", H.K_CASES, ids=_ids)
def test_k_case_preconditions(c):
    d = H.k_data(c)
    K, w, b, lab, cw = c.K, d["w"], d["b"], d["lab"].long(), d["cw"]
    x = H.logits64(d["a64"], w, b)
    assert x.shape == (c.M, K)
    _check_logits_exact(d["a64"], w, b, x, values=H.KW_VALUES, q=64)
    assert (w[:, 1:] != w[:, :-1]).any(0).all()          # neighbouring channels differ in some class row
    # no two classes share a weight at any channel: sum_k dlogit_k w[k][c] never cancels for lack of a difference
    assert all(w[:, ch].unique().numel() == K for ch in range(H.HEAD_C))
    # exact ties at the top: two-way, three-way (K >= 3), not only all-equal, not only involving class 0
    tt, am = H.top_ties(x), H.argmax_lowest(x)
    assert (tt == 2).sum().item() >= 2 and (tt == 1).double().mean().item() > 0.5
    if K >= 3:
        assert (tt == 3).sum().item() >= 1 and ((tt >= 2) & (am > 0)).sum().item() >= 1
    if K > 3:
        assert ((tt >= 2) & (tt < K)).sum().item() >= 2
    assert torch.equal(am[tt == 1], x.argmax(1)[tt == 1])
    if c.M >= H.M_U0:
        assert set(am.unique().tolist()) == set(range(K))    # every class wins somewhere
    # labels: every class, 255, ids in K..254
    if c.labels == "ignored":
        assert (lab == 255).all()
    else:
        assert set(range(K)) <= set(lab.unique().tolist()) and (lab == 255).any() and ((lab >= K) & (lab < 255)).any()
        assert 0.7 < (lab < K).double().mean().item() < 0.95
    # dyadic class weights with one zero: the weight sum is exact in fp32
    assert set(cw.tolist()) <= {0.0, 0.5, 1.0, 2.0} and cw[K - 1].item() == 0.0 and (cw[:K - 1] > 0).all()
    assert 2.0 * c.M * 2 < L.F32_EXACT and c.M < L.F32_EXACT
    # softmax: most pixels unsaturated, a minority saturated, the __expf arguments inside the probed range
    spread = x.max(1).values - x.min(1).values
    assert (spread < 8).double().mean().item() >= 0.6 and (spread > 16).double().mean().item() >= 0.005
    assert 20 <= spread.max().item() <= 80
    # a few pixels stay saturated ON their label (softmax - onehot cancels there: the absolute bound alone holds)
    if c.labels != "ignored" and c.M >= H.M_U1:
        s_t = torch.softmax(x, 1).gather(1, lab.clamp(max=K - 1)[:, None])[:, 0]
        assert ((lab < K) & (s_t > 0.99)).sum().item() >= 1


def _k_shares(r, d, kept):
    """(tie share, tight share) of da, in slices of CHUNK pixels: the share of all elements within slop of a bf16
    rounding tie, and the share of the kept pixels' elements whose slop is below 1/16 of half an ulp."""
    ties = tight = 0
    for p in range(0, r["M"], CHUNK):
        px = slice(p, p + CHUNK)
        ref, slop = H.k_da_bounds(r, d["w"], "cpu", px)
        ties += H.tie_share(ref, slop) * ref.numel()
        tight += int(((ref != 0) & (slop <= 0.5 * L.ulp_bf16(ref) / 16))[kept[px]].sum())
        assert not ref[~kept[px]].any() and not slop[~kept[px]].any()   # ignored / zero-weight: exactly zero
    return ties / (r["M"] * H.HEAD_C), tight / max(int(kept.sum()) * H.HEAD_C, 1)


@pytest.mark.parametrize("mode", H.K_MODES, ids=lambda m: m[0])
@pytest.mark.parametrize("c", H.K_CASES, ids=_ids)
def test_k_tie_share_and_slop(c, mode):
    """At most 1 % of the elements of da may lie within slop of a bf16 rounding tie (where the per-element check
    accepts either neighbour), for every case and mode; and at 60 % or more of the kept pixels' elements the slop is
    below 1/16 of half an ulp, so the bound there is the bf16 rounding, not the allowance."""
    _, weights, dice_w = mode
    d = H.k_data(c)
    x = H.logits64(d["a64"], d["w"], d["b"])
    r = H.k_ref(x, d["lab"], d["cw"] if weights else None, dice_w)
    kept = r["kept"]
    if weights and dice_w == 0.0:
        kept = kept & (d["lab"].long() != c.K - 1)
    ties, tight = _k_shares(r, d, kept)
    assert ties <= 0.01
    if c.labels == "ignored":
        assert not kept.any() and not r["dl"].any() and not r["dl_slop"].any() and not r["loss"].any()
        return
    assert tight >= 0.6
    assert math.isfinite(r["loss"][0].item()) and r["loss_bounds"].max().item() < 1e-4
