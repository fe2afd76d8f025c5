"""Exact and per-element tests of the loss heads (GPU only): csrc/head_loss.hip (head_fwd in its three
instantiations, head_bwd plain and BN-fused, head_bn_bwd_apply, head_grad_finalize, head_mask) and
csrc/head_multi.hip (headk_fwd / headk_bwd / headk_mask, plain and extended).

Exact class. On the lattice operands of tests/head_cases.py every logit is one fixed fp32 value, so logits,
masks, target sums and label counts are compared bit for bit with the fp64 reference; outputs are prefilled
with a sentinel, views sit between guard bands, partial-row buffers must be written for exactly
blocks_for(M) rows, inputs must come back unchanged, and a loss scale of 2^-k must scale every gradient
exactly.

Per-element class. Every element of da / dy must satisfy |got - ref| <= 1/2 ulp_bf16(ref) + slop against the
fp64 reference, slop being an absolute bound derived in head_cases.py from the kernels' fp32 operations and
the measured accuracy of __expf / log1pf / logf (scripts/expf_probe.hip) -- never from what a head kernel
returns. Reductions are folded in fp64 and held to n U32 sum|term| + sum slop. Each test prints its margin
(profiles/head_exact.md). The BN-fused forms are checked against the fp64 composite, not against the
separate kernels.

The sizes are the smallest M at which each path of the shared grid arithmetic exists (one ragged block, u = 0
only, u = 1 ragged, all four slots, a second grid-stride pass); tests/test_head_cases_cpu.py proves that
and every other precondition without a GPU.
"""
import pytest
import torch

import head_cases as H
import lattice as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = H.DICE_EPS


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def _ids(c):
    return c.name


class Act:
    """A [1, 1, M, 64] device activation: dense, or a 64-channel slice of a wider buffer between guard bands.
    t = None: an output, prefilled with the sentinel."""

    def __init__(self, t, M, c):
        shape = (1, 1, M, H.HEAD_C)
        self.views = c.views
        if c.views:
            self.flat, self.t = L.embed(t, shape, c.pads[0], c.pads[1], DEV)
        elif t is None:
            self.flat = self.t = torch.full(shape, L.SENTINEL, dtype=L.BF16, device=DEV)
        else:
            self.flat = self.t = t.to(DEV).contiguous()
        self.before = self.flat.clone()

    def unchanged(self):
        return torch.equal(self.flat.view(torch.int16), self.before.view(torch.int16))

    def outside_intact(self):
        return (not self.views) or L.outside_view_intact(self.flat, self.t)


class F32:
    """n fp32 values between guard bands, everything prefilled with the sentinel."""

    def __init__(self, n):
        self.flat = torch.full((2 * L.GUARD + n,), L.SENTINEL, device=DEV)
        self.t = self.flat[L.GUARD:L.GUARD + n]

    def only_wrote(self, n):
        """The first n values were all written (no sentinel left) and nothing else was."""
        probe = self.flat.clone()
        probe[L.GUARD:L.GUARD + n] = L.SENTINEL
        return bool((self.t[:n] != L.SENTINEL).all()) and torch.equal(probe, torch.full_like(probe, L.SENTINEL))


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (fp64); a missed zero bound gives inf."""
    ref, bound = ref.to(got.device), bound.to(got.device)
    if ref.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item()


def _dev(t):
    return t.to(DEV)


# ---------------------------------------------------------------------------------------------
# binary head
# ---------------------------------------------------------------------------------------------

class BinRun:
    """The operands of one binary case on the device, and its exact logits."""

    def __init__(self, c):
        d = H.bin_data(c)
        self.c, self.M, self.d = c, c.M, d
        self.nb = H.blocks_for(c.M)
        self.a, self.y = Act(d["a"], c.M, c), Act(d["y"], c.M, c)
        self.w, self.b, self.t, self.coef = _dev(d["w"]), _dev(d["b"]), _dev(d["t"]), _dev(d["coef"])
        self.small = [self.w, self.b, self.t, self.coef]
        self.small_before = [t.clone() for t in self.small]
        self.x = H.logits64(d["a64"], d["w"], d["b"])
        self.a64 = self.a.t.double()

    def inputs_unchanged(self):
        return self.a.unchanged() and self.y.unchanged() and all(torch.equal(u, v) for u, v in zip(self.small, self.small_before))

    def fwd(self, C, form, dice_w, gscale=1.0):
        """form: "plain" (head_fwd<false,false> on a), "bn" (<true,false> on y), "grad" (<true,true>)."""
        o = {"logits": F32(self.M), "part": F32(self.nb * 65 + 64), "sums": F32(8), "loss": F32(4)}
        if form == "plain":
            C.head_fwd(self.a.t, self.w, self.b, self.t, o["logits"].t, o["part"].t, o["sums"].t, o["loss"].t, dice_w, EPS)
        elif form == "bn":
            C.head_fwd(self.y.t, self.w, self.b, self.t, o["logits"].t, o["part"].t, o["sums"].t, o["loss"].t, dice_w, EPS,
                       self.coef)
        else:
            o["gpart"], o["bnpart"] = F32(self.nb * 65 + 64), F32(self.nb * 128 + 64)
            C.head_fwd(self.y.t, self.w, self.b, self.t, o["logits"].t, o["part"].t, o["sums"].t, o["loss"].t, dice_w, EPS,
                       self.coef, o["gpart"].t, o["bnpart"].t, gscale)
        torch.cuda.synchronize()
        return o


def _check_fwd(run, o, r, what):
    """Logits bitwise, the 4-float partial rows (exactly nb of them) within the reduction bounds, sum t exact,
    sums[] and the loss pair within theirs; the scalars behind sums[0..3] / loss[0..1] untouched."""
    M, nb = run.M, run.nb
    assert torch.equal(o["logits"].t, _dev(r["x"].float())) and o["logits"].only_wrote(M)
    assert o["part"].only_wrote(nb * 4)
    rows = o["part"].t[:nb * 4].view(nb, 4).double().sum(0).cpu()
    assert rows[3].item() == r["sums"][3].item()
    m_rows = _ratio(rows[:3], r["sums"][:3], r["sum_bounds"][:3])
    assert o["sums"].only_wrote(4) and o["loss"].only_wrote(2)
    sums = o["sums"].t[:4].cpu()
    assert sums[3].item() == r["sums"][3].item()
    m_sums = _ratio(sums[:3], r["sums"][:3], r["sum_bounds"][:3])
    m_loss = _ratio(o["loss"].t[:2].cpu(), r["loss"], r["loss_bounds"])
    print(f"{run.c.name} {what}: rows {m_rows:.4f} sums {m_sums:.4f} loss {m_loss:.4f} of the bound")
    assert m_rows <= 1 and m_sums <= 1 and m_loss <= 1


@pytest.mark.parametrize("c", H.BIN_CASES, ids=_ids)
def test_head_fwd_exact(C, c):
    """head_fwd<false,false>, <true,false> and <true,true>: logits bitwise the fp64 reference (hence each
    other), loss terms within the derived reduction bounds, sum t exact; the GRAD form's head-gradient rows and
    BN-backward rows against the fp64 composite, and head_grad_finalize on them."""
    run = BinRun(c)
    GS = 0.5
    r1, r0 = H.bin_ref(run.x, run.d["t"], 1.0), H.bin_ref(run.x, run.d["t"], 0.0, gscale=GS)
    o_plain, o_bn, o_grad = run.fwd(C, "plain", 1.0), run.fwd(C, "bn", 1.0), run.fwd(C, "grad", 0.0, GS)
    _check_fwd(run, o_plain, r1, "plain")
    _check_fwd(run, o_bn, r1, "bn")
    _check_fwd(run, o_grad, r0, "grad")
    assert torch.equal(o_plain["logits"].t, o_bn["logits"].t) and torch.equal(o_bn["logits"].t, o_grad["logits"].t)
    assert torch.equal(o_plain["part"].flat, o_bn["part"].flat) and torch.equal(o_plain["loss"].flat, o_bn["loss"].flat)
    nb = run.nb
    # the GRAD form's rows
    assert o_grad["gpart"].only_wrote(nb * 65) and o_grad["bnpart"].only_wrote(nb * 128)
    gw, bw, gb, bb = H.head_grad_ref(r0, run.a64, final=False)
    rows = o_grad["gpart"].t[:nb * 65].view(nb, 65).double().sum(0)
    m_gw, m_gb = _ratio(rows[:64], gw, bw), _ratio(rows[64], gb, bb)
    f = H.bn_fused_ref(r0, run.y.t, run.coef, run.w)
    bn = o_grad["bnpart"].t[:nb * 128].view(nb, 2, 64).double().sum(0)
    m_bn = _ratio(bn, f["sums"], f["bounds"])
    gwf, gbf = F32(64), F32(1)
    C.head_grad_finalize(o_grad["gpart"].t, c.M, gwf.t, gbf.t)
    torch.cuda.synchronize()
    gw, bw, gb, bb = H.head_grad_ref(r0, run.a64, final=True)
    m_fin = max(_ratio(gwf.t, gw, bw), _ratio(gbf.t[0], gb, bb))
    print(f"{c.name} grad rows: gw {m_gw:.4f} gb {m_gb:.4f} bn rows {m_bn:.4f} finalized {m_fin:.4f} of the bound; "
          f"tie-ambiguous g {f['amb_share']:.5f}")
    assert m_gw <= 1 and m_gb <= 1 and m_bn <= 1 and m_fin <= 1
    assert gwf.only_wrote(64) and gbf.only_wrote(1)
    assert run.inputs_unchanged()
    if c.M >= H.LARGE_M:  # bitwise repeatable
        for form, o, args in (("plain", o_plain, (1.0,)), ("grad", o_grad, (0.0, GS))):
            again = run.fwd(C, form, *args)
            assert all(torch.equal(again[k].flat, o[k].flat) for k in o)


@pytest.mark.parametrize("dice_w", H.DICE_WS)
@pytest.mark.parametrize("c", H.BIN_CASES, ids=_ids)
def test_head_bwd_per_element(C, c, dice_w):
    """head_bwd<false>: every element of da within 1/2 ulp_bf16 + slop of the fp64 reference, dW / db rows and
    finalized values within the reduction bounds, exactly nb partial rows, a 2^-3 loss scale exact;
    head_bwd<true> (BN-fused): its BN-backward rows and head gradients against the fp64 composite."""
    run = BinRun(c)
    nb, M = run.nb, c.M
    r = H.bin_ref(run.x, run.d["t"], dice_w)
    fw = run.fwd(C, "plain", dice_w)
    logits, sums = fw["logits"].t, fw["sums"].t[:4]
    keep = [logits.clone(), sums.clone()]

    def bwd(gscale):
        o = {"da": Act(None, M, c), "part": F32(nb * 65 + 64), "gw": F32(64), "gb": F32(1)}
        T = C.head_bwd(run.a.t, run.w, logits, run.t, sums, o["da"].t, o["part"].t, o["gw"].t, o["gb"].t, dice_w, EPS, gscale)
        torch.cuda.synchronize()
        assert T == nb
        return o

    o = bwd(1.0)
    ref, slop = H.outer_bounds(_dev(r["dx"]), _dev(r["dx_slop"]), run.w)
    m_da = H.within(o["da"].t.view(M, 64), ref, slop)
    off = (o["da"].t.view(M, 64) != ref.float().to(L.BF16)).sum().item()
    assert o["da"].outside_intact()
    assert o["part"].only_wrote(nb * 65) and o["gw"].only_wrote(64) and o["gb"].only_wrote(1)
    gw, bw, gb, bb = H.head_grad_ref(r, run.a64, final=False)
    rows = o["part"].t[:nb * 65].view(nb, 65).double().sum(0)
    m_rows = max(_ratio(rows[:64], gw, bw), _ratio(rows[64], gb, bb))
    gw, bw, gb, bb = H.head_grad_ref(r, run.a64, final=True)
    m_fin = max(_ratio(o["gw"].t, gw, bw), _ratio(o["gb"].t[0], gb, bb))
    print(f"{c.name} dice_w={dice_w}: da {m_da:.4f} (largest slop {slop.max().item():.3e}, {off} / {M * 64} off "
          f"RNE_bf16(ref)) rows {m_rows:.4f} gw/gb {m_fin:.4f} of the bound")
    assert m_da <= 1 and m_rows <= 1 and m_fin <= 1
    if c.targets == "zero" and dice_w == 0.0:
        assert (o["da"].t.float() * run.w.sign() >= 0).all()  # sigmoid - 0 > 0: da carries w's sign everywhere
    # loss scale 2^-3 (DDP's 1 / world): exact in binary, so every gradient is bitwise 1/8 of the unscaled one
    s = bwd(0.125)
    assert torch.equal(s["da"].t.float(), o["da"].t.float() * 0.125)
    assert torch.equal(s["gw"].t, o["gw"].t * 0.125) and torch.equal(s["gb"].t, o["gb"].t * 0.125)
    assert torch.equal(s["part"].t[:nb * 65], o["part"].t[:nb * 65] * 0.125)
    # BN-fused: no da; the BN-backward rows of g = bf16(dlogit * w) * relu'(y) and the same head gradients
    GS = 0.25
    rg = H.bin_ref(run.x, run.d["t"], dice_w, gscale=GS)
    q = {"part": F32(nb * 65 + 64), "gw": F32(64), "gb": F32(1), "bnpart": F32(nb * 128 + 64)}
    T = C.head_bwd(run.y.t, run.w, logits, run.t, sums, None, q["part"].t, q["gw"].t, q["gb"].t, dice_w, EPS, GS, run.coef,
                   q["bnpart"].t)
    torch.cuda.synchronize()
    assert T == nb and q["part"].only_wrote(nb * 65) and q["bnpart"].only_wrote(nb * 128)
    f = H.bn_fused_ref(rg, run.y.t, run.coef, run.w)
    bn = q["bnpart"].t[:nb * 128].view(nb, 2, 64).double().sum(0)
    m_bn = _ratio(bn, f["sums"], f["bounds"])
    gw, bw, gb, bb = H.head_grad_ref(rg, run.a64, final=True)
    m_fg = max(_ratio(q["gw"].t, gw, bw), _ratio(q["gb"].t[0], gb, bb))
    print(f"{c.name} dice_w={dice_w} BN-fused: bn rows {m_bn:.4f} gw/gb {m_fg:.4f} of the bound; "
          f"tie-ambiguous g {f['amb_share']:.5f}")
    assert m_bn <= 1 and m_fg <= 1
    assert run.inputs_unchanged() and torch.equal(logits, keep[0]) and torch.equal(sums, keep[1])
    if M >= H.LARGE_M:
        again = bwd(1.0)
        assert all(torch.equal(again[k].flat, o[k].flat) for k in o)


@pytest.mark.parametrize("dice_w", (0.0, 2.5))
@pytest.mark.parametrize("c", H.APPLY_CASES, ids=_ids)
def test_head_bn_bwd_apply_per_element(C, c, dice_w):
    """dy = A g + B y + K with g = bf16(dlogit * w) * relu'(y) recomputed from the logits, per element against
    the fp64 composite. Where dlogit * w lies within its slop of a bf16 rounding tie either neighbour of g is
    accepted. dy rounds twice in fp32 (the two fmas): slop = 2 U32 (|A g| + |B y + K|)."""
    run = BinRun(c)
    M, GS = c.M, 0.5
    r = H.bin_ref(run.x, run.d["t"], dice_w, gscale=GS)
    fw = run.fwd(C, "bn", dice_w)
    coef2 = H.bwd_coef2(M, L.generator(33000 + c.seed))
    c2 = _dev(coef2)
    dy = Act(None, M, c)
    C.head_bn_bwd_apply(run.y.t, run.w, fw["logits"].t, run.t, fw["sums"].t[:4], run.coef, c2, dy.t, dice_w, EPS, GS)
    torch.cuda.synchronize()
    f = H.bn_fused_ref(r, run.y.t, run.coef, run.w)
    A, B, K = (c2[k * 64:(k + 1) * 64].double() for k in range(3))
    yd = run.y.t.double().view(M, 64)
    rest = B * yd + K
    got = dy.t.view(M, 64)
    # g lies between its two candidates (equal at all but the tie-ambiguous elements; where the sigmoid saturates
    # and dlogit cancels to ~0 the slop spans several bf16 values and any of them is legal), and dy is monotone in g
    refs = [A * g + rest for g in (f["g_lo"], f["g_hi"])]
    lo, hi = torch.minimum(*refs), torch.maximum(*refs)
    big = torch.maximum(lo.abs(), hi.abs())
    bound = 0.5 * L.ulp_bf16(big) + 2 * H.U32 * (torch.maximum((A * f["g_lo"]).abs(), (A * f["g_hi"]).abs()) + rest.abs())
    err = torch.maximum(lo - got.double(), got.double() - hi).clamp_min(0)
    m = (err / bound.clamp_min(1e-300)).max().item()
    moved = ((A * f["g_lo"] + rest).float().to(L.BF16) != rest.float().to(L.BF16)).double().mean().item()
    print(f"{c.name} dice_w={dice_w}: dy {m:.4f} of the bound; tie-ambiguous g {f['amb_share']:.5f}; "
          f"g moves dy's bf16 value at {moved:.3f} of the elements")
    assert m <= 1
    assert moved > 0.15  # B y + K does not swamp g: the check sees the recomputed gradient
    assert dy.outside_intact() and run.inputs_unchanged()
    if M >= H.LARGE_M:
        dy2 = Act(None, M, c)
        C.head_bn_bwd_apply(run.y.t, run.w, fw["logits"].t, run.t, fw["sums"].t[:4], run.coef, c2, dy2.t, dice_w, EPS, GS)
        assert torch.equal(dy2.flat, dy.flat)


def _mask_out(M):
    flat = torch.full((2 * L.GUARD + M,), 9, dtype=torch.uint8, device=DEV)
    return flat, flat[L.GUARD:L.GUARD + M]


def _mask_intact(flat, M):
    return bool((flat[:L.GUARD] == 9).all()) and bool((flat[L.GUARD + M:] == 9).all())


@pytest.mark.parametrize("c", [c for c in H.BIN_CASES if c.targets != "zero"], ids=_ids)
def test_head_mask_exact(C, c):
    """mask = (logit > thr), exactly: the threshold sits ON a logit value many pixels hold (they must give 0) and
    one fp32 step below (they give 1) and above it."""
    run = BinRun(c)
    M = c.M
    x32 = run.x.float()
    vals, counts = x32.unique(return_counts=True)
    thr0 = vals[counts.argmax()]
    on = int(counts.max())   # pixels that sit on the threshold
    assert on >= (2 if M >= H.M_U0 else 1) and (x32 > thr0).any() and (x32 < thr0).any()
    inf = torch.tensor(float("inf"))
    flips = []
    for thr in (torch.nextafter(thr0, -inf), thr0, torch.nextafter(thr0, inf)):
        flat, mask = _mask_out(M)
        C.head_mask(run.a.t, run.w, run.b, float(thr.item()), mask)
        torch.cuda.synchronize()
        exp = (run.x > thr.double()).to(torch.uint8)
        assert torch.equal(mask.cpu(), exp) and _mask_intact(flat, M)
        flips.append(int(mask.sum()))
    # the on-threshold pixels, and only they, flip between the first two thresholds; nothing between the last two
    assert flips[0] - flips[1] == on and flips[1] == flips[2]
    assert run.inputs_unchanged()


# ---------------------------------------------------------------------------------------------
# K-class head
# ---------------------------------------------------------------------------------------------

class KRun:
    def __init__(self, c):
        d = H.k_data(c)
        self.c, self.M, self.K, self.d = c, c.M, c.K, d
        self.nb = H.blocks_for(c.M)
        self.a = Act(d["a"], c.M, c)
        self.w, self.b, self.lab, self.cw = _dev(d["w"].reshape(-1)), _dev(d["b"]), _dev(d["lab"]), _dev(d["cw"])
        self.small = [self.w, self.b, self.lab, self.cw]
        self.small_before = [t.clone() for t in self.small]
        self.x = H.logits64(d["a64"], d["w"], d["b"])
        self.a64 = self.a.t.double()

    def inputs_unchanged(self):
        return self.a.unchanged() and all(torch.equal(u, v) for u, v in zip(self.small, self.small_before))

    def fwd(self, C, weights, dice_w):
        K, ext = self.K, weights or dice_w != 0
        self.prow = 2 + 3 * K if ext else 2
        o = {"logits": F32(self.M * K), "part": F32(self.nb * K * 65 + 64), "sums": F32(2 + 3 * K + 4), "loss": F32(4)}
        C.headk_fwd(self.a.t, self.w, self.b, self.lab, o["logits"].t, o["part"].t, o["sums"].t, o["loss"].t,
                    self.cw if weights else None, dice_w, EPS)
        torch.cuda.synchronize()
        return o


@pytest.mark.parametrize("mode", [H.K_MODES[0], H.K_MODES[3]], ids=lambda m: m[0])
@pytest.mark.parametrize("c", H.K_CASES, ids=_ids)
def test_headk_fwd_exact(C, c, mode):
    """headk_fwd, plain and extended, K = 2 / 3 / 5 / 8 (both paddings of pow2_classes): logits bitwise the fp64
    reference, the kept count, the weight sum and the T_k counts exact, sum ce / I_k / P_k and the loss pair within
    the derived bounds, exactly nb partial rows."""
    _, weights, dice_w = mode
    run = KRun(c)
    M, K, nb = c.M, c.K, run.nb
    r = H.k_ref(run.x, run.d["lab"], run.d["cw"] if weights else None, dice_w)
    o = run.fwd(C, weights, dice_w)
    n = run.prow
    assert torch.equal(o["logits"].t, _dev(r["x"].float().reshape(-1))) and o["logits"].only_wrote(M * K)
    assert o["part"].only_wrote(nb * n) and o["sums"].only_wrote(n) and o["loss"].only_wrote(2)
    rows = o["part"].t[:nb * n].view(nb, n).double().sum(0).cpu()
    sums = o["sums"].t[:n].cpu()
    exact = r["sum_bounds"] == 0   # the weight sum / kept count and the T_k counts
    assert torch.equal(rows[exact], r["sums"][exact]) and torch.equal(sums[exact].double(), r["sums"][exact])
    m_rows = _ratio(rows[~exact], r["sums"][~exact], r["sum_bounds"][~exact])
    m_sums = _ratio(sums[~exact], r["sums"][~exact], r["sum_bounds"][~exact])
    m_loss = _ratio(o["loss"].t[:2].cpu(), r["loss"], r["loss_bounds"])
    print(f"{c.name} {mode[0]}: rows {m_rows:.4f} sums {m_sums:.4f} loss {m_loss:.4f} of the bound")
    assert m_rows <= 1 and m_sums <= 1 and m_loss <= 1
    if c.labels == "ignored":
        assert o["loss"].t[0].item() == 0.0 and sums[1].item() == 0.0
    assert run.inputs_unchanged()
    if M >= H.LARGE_M:
        again = run.fwd(C, weights, dice_w)
        assert all(torch.equal(again[k].flat, o[k].flat) for k in o)


@pytest.mark.parametrize("mode", H.K_MODES, ids=lambda m: m[0])
@pytest.mark.parametrize("c", H.K_CASES, ids=_ids)
def test_headk_bwd_per_element(C, c, mode):
    """headk_bwd: every element of da within 1/2 ulp_bf16 + slop, zero bits at the ignored pixels (labels 255 and
    K..254) and, with class weights and no Dice term, at the zero-weight class; dW / db within the reduction
    bounds; exactly nb partial rows; a 2^-3 loss scale exact."""
    _, weights, dice_w = mode
    run = KRun(c)
    M, K, nb = c.M, c.K, run.nb
    r = H.k_ref(run.x, run.d["lab"], run.d["cw"] if weights else None, dice_w)
    fw = run.fwd(C, weights, dice_w)
    logits, sums = fw["logits"].t, fw["sums"].t[:run.prow]
    keep = [logits.clone(), sums.clone()]
    row = K * 65

    def bwd(gscale):
        o = {"da": Act(None, M, c), "part": F32(nb * row + 64), "gw": F32(K * 64), "gb": F32(K)}
        C.headk_bwd(run.a.t, run.w, logits, run.lab, sums, o["da"].t, o["part"].t, o["gw"].t, o["gb"].t, gscale,
                    run.cw if weights else None, dice_w, EPS)
        torch.cuda.synchronize()
        return o

    o = bwd(1.0)
    da = o["da"].t.view(M, 64)
    ref, slop = H.k_da_bounds(r, run.d["w"], DEV)
    m_da = H.within(da, ref, slop)
    assert o["da"].outside_intact()
    assert o["part"].only_wrote(nb * row) and o["gw"].only_wrote(K * 64) and o["gb"].only_wrote(K)
    gw, bw, gb, bb = H.k_grad_ref(r, run.a64, final=True)
    m_gw, m_gb = _ratio(o["gw"].t.view(K, 64), gw, bw), _ratio(o["gb"].t, gb, bb)
    gw, bw, gb, bb = H.k_grad_ref(r, run.a64, final=False)
    rows = o["part"].t[:nb * row].view(nb, row).double().sum(0)
    m_rows = max(_ratio(rows[:K * 64].view(K, 64), gw, bw), _ratio(rows[K * 64:], gb, bb))
    print(f"{c.name} {mode[0]}: da {m_da:.4f} (largest slop {slop.max().item():.3e}) rows {m_rows:.4f} gw {m_gw:.4f} "
          f"gb {m_gb:.4f} of the bound")
    assert m_da <= 1 and m_rows <= 1 and m_gw <= 1 and m_gb <= 1
    dead = ~r["kept"]
    if weights and dice_w == 0.0:
        dead = dead | (run.d["lab"].long() == K - 1)   # the zero-weight class
    assert dead.any() and not bool(da.view(torch.int16)[_dev(dead)].any())
    if c.labels == "ignored":
        assert not bool(o["gw"].t.any()) and not bool(o["gb"].t.any())
    s = bwd(0.125)
    assert torch.equal(s["da"].t.float(), o["da"].t.float() * 0.125)
    assert torch.equal(s["gw"].t, o["gw"].t * 0.125) and torch.equal(s["gb"].t, o["gb"].t * 0.125)
    assert run.inputs_unchanged() and torch.equal(logits, keep[0]) and torch.equal(sums, keep[1])
    if M >= H.LARGE_M:
        again = bwd(1.0)
        assert all(torch.equal(again[k].flat, o[k].flat) for k in o)


@pytest.mark.parametrize("c", [c for c in H.K_CASES if c.labels != "ignored"], ids=_ids)
def test_headk_mask_exact(C, c):
    """mask = (arg-max class == cls) for every class, exactly; the data holds exact two- and three-way ties at
    the top (not only all-equal), which must resolve to the lowest class."""
    run = KRun(c)
    M, K = c.M, c.K
    ref = H.argmax_lowest(run.x)
    total = torch.zeros(M, dtype=torch.int32)
    for cls in range(K):
        flat, mask = _mask_out(M)
        C.headk_mask(run.a.t, run.w, run.b, cls, mask)
        torch.cuda.synchronize()
        assert torch.equal(mask.cpu(), (ref == cls).to(torch.uint8)), f"class {cls}"
        assert _mask_intact(flat, M)
        total += mask.cpu().int()
    assert (total == 1).all() and run.inputs_unchanged()
