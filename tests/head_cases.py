"""Cases, lattice operands, fp64 references and error bounds of the loss-head tests (csrc/head_loss.hip,
csrc/head_multi.hip): tests/test_head_exact_gpu.py runs them on the GPU, tests/test_head_cases_cpu.py
proves their preconditions without one.

Operands. The activation holds small dyadic numbers (the exact BN + ReLU of small integers), the head
weights are 0, +-1/8 or +-1/4 (binary) or multiples of 1/16 up to 1/4 (K-class) and the bias a multiple of 1/8, so
every partial sum of a logit is a small multiple of 2^-6: exact in fp32 in any order. The logits are therefore ONE fixed fp32 value each, and the
ReLU mask, xhat, the targets' sums and the label counts are exact too. Only the sigmoid / softmax / log
terms are inexact, and those get a per-element bound derived from the kernels' fp32 operations (below).

Sizes. All the head kernels share blocks_for(M) = min(ceil(M / 32), 2048) blocks of 32 pixel groups with
HPX = 4 pixels in flight per 8-lane group at p0 + u * stride, stride = 32 * blocks. `slot_fill` / `passes`
transcribe that arithmetic; M_CASES holds the smallest M at which each path exists.

Pure torch: the native extension is never imported here. The per-pixel references are formed on the CPU
in fp64; the [M, 64] outer products and comparisons run on whatever device the operands are on.
"""
import functools
import math
from dataclasses import dataclass

import torch

import lattice as L

BF16 = L.BF16
HEAD_C = 64
HPX = 4
GROUPS = 32          # pixel groups (of 8 lanes) per block of 256 threads
GRID_CAP = 2048
APPLY_PX = 128       # head_bn_bwd_apply: pixels per block (32 groups x 4 slots), grid = ceil(M / 128)
APPLY_GRID_CAP = 1 << 20

U32 = 2.0 ** -24     # unit roundoff of fp32
# Worst relative error of the device intrinsics, measured alone against fp64 by scripts/expf_probe.hip on an
# MI355X (profiles/head_exact.md), in units of U32. No AMD accuracy table ships with the toolchain. __expf's
# error grows with |x| (its product x * log2(e) rounds), so it is kept per range of |x|: (upper edge, worst).
# The allowance is twice the measured value.
EXPF_MEASURED = ((1.0, 1.58), (2.0, 2.56), (4.0, 4.54), (8.0, 8.07), (16.0, 15.41), (32.0, 30.06), (48.0, 55.71), (80.0, 62.99))
LOG1P_MEASURED = 1.98          # log1pf(e), e in (0, 1]: relative
LOGF_MEASURED = 5.17           # logf over [1, 8]: absolute
LOG1P_REL = 2 * LOG1P_MEASURED * U32
LOGF_ABS = 2 * LOGF_MEASURED * U32
DIVU = 5 * U32                 # an fp32 division: allowed 2.5 ulp (measured: 1 / (1 + e), the addition included, 1.5 U32)


def expf_rel(arg: torch.Tensor) -> torch.Tensor:
    """Allowed relative error of __expf(arg), arg in [-80, 0]: twice the worst measured in |arg|'s range."""
    edges = torch.tensor([e for e, _ in EXPF_MEASURED[:-1]], dtype=torch.float64, device=arg.device)
    worst = torch.tensor([v for _, v in EXPF_MEASURED], dtype=torch.float64, device=arg.device).cummax(0).values
    assert arg.abs().max().item() <= EXPF_MEASURED[-1][0]
    return 2 * U32 * worst[torch.bucketize(arg.abs(), edges)]


# ---------------------------------------------------------------------------------------------
# the launchers' grid arithmetic
# ---------------------------------------------------------------------------------------------

def blocks_for(M: int) -> int:
    return max(1, min(L.cdiv(M, GROUPS), GRID_CAP))


def stride(M: int) -> int:
    return GROUPS * blocks_for(M)


def passes(M: int) -> int:
    """Trips of the `p0 += stride * HPX` loop that hold a pixel."""
    return L.cdiv(M, stride(M) * HPX)


def slot_fill(M: int, p: int = 0):
    """Pixels in each of the HPX slots u = 0..3 of pass p."""
    s = stride(M)
    base = p * s * HPX
    return [max(0, min(s, M - base - u * s)) for u in range(HPX)]


def mask_trips(M: int) -> int:
    """Trips of head_mask / headk_mask's plain grid-stride loop (`p += stride`)."""
    return L.cdiv(M, stride(M))


def apply_blocks(M: int) -> int:
    return max(1, min(L.cdiv(M, APPLY_PX), APPLY_GRID_CAP))


def apply_slot_fill(M: int):
    s = GROUPS * apply_blocks(M)
    return [max(0, min(s, M - u * s)) for u in range(HPX)]


def chain(M: int) -> int:
    """The longest fp32 addition chain behind one value of a per-block partial row: a lane adds up to HPX
    terms per pass, then at most 6 shuffle steps and the 3 additions over the block's 4 waves."""
    return HPX * passes(M) + 6 + 3


def chain_final(M: int) -> int:
    """... and behind a finalized fp32 gradient: 256 threads walk the rows, 6 shuffle steps, 3 wave adds, and
    one more rounding for the loss scale / the store."""
    return chain(M) + L.cdiv(blocks_for(M), 256) + 6 + 3 + 1


M_TINY = 35
M_U0 = 960
M_U1 = GRID_CAP * GROUPS + 37
M_U3 = 3 * GRID_CAP * GROUPS + 5
M_PASS2 = HPX * GRID_CAP * GROUPS + GRID_CAP * GROUPS + 77
M_CASES = {"tiny": M_TINY, "u0-only": M_U0, "u1-ragged": M_U1, "u3-ragged": M_U3,
           "pass2-ragged": M_PASS2}


def check_regime(name: str, M: int) -> None:
    """The M of a case reaches the path its name claims."""
    f0 = slot_fill(M, 0)
    s = stride(M)
    if name == "tiny":  # a full block and a second one with 3 of its 32 pixel groups at work
        assert blocks_for(M) == 2 and 0 < M - GROUPS < 8 and f0 == [M, 0, 0, 0] and passes(M) == 1
    elif name == "u0-only":
        assert 1 < blocks_for(M) < GRID_CAP and f0 == [M, 0, 0, 0] and passes(M) == 1
    elif name == "u1-ragged":
        assert blocks_for(M) == GRID_CAP and f0[0] == s and 0 < f0[1] < s and f0[1] % GROUPS and f0[2] == 0
        assert f0[1] > GROUPS and passes(M) == 1
    elif name == "u3-ragged":
        assert f0[:3] == [s, s, s] and 0 < f0[3] < GROUPS and passes(M) == 1
    elif name == "pass2-ragged":
        f1 = slot_fill(M, 1)
        assert f0 == [s] * 4 and passes(M) == 2 and f1[0] == s and 0 < f1[1] < s and f1[1] % GROUPS and f1[2] == 0
        assert mask_trips(M) == 6
    else:
        raise AssertionError(name)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Bin:
    """One binary-head case: M pixels of 64 channels as [1, 1, M, 64]."""
    name: str
    M: int
    targets: str = "binary"    # "binary" {0, 1} | "soft" {0, 1/4, 1} | "zero" (all background)
    pitch: int = 64            # > 64: the activation and da / dy are channel slices of a wider buffer
    off: int = 0
    seed: int = 0

    @property
    def views(self) -> bool:
        return self.pitch > HEAD_C

    @property
    def pads(self):
        return self.off, self.pitch - HEAD_C - self.off


BIN_CASES = [
    Bin("tiny-views", M_TINY, pitch=128, off=8),
    Bin("u0-only", M_U0),
    Bin("u1-ragged-views", M_U1, pitch=192, off=64),
    Bin("u1-ragged-soft", M_U1, targets="soft", seed=1),
    Bin("u3-ragged", M_U3),
    Bin("pass2-ragged", M_PASS2),
    Bin("pass2-ragged-all-background", M_PASS2, targets="zero"),
]
APPLY_CASES = [
    Bin("apply-tiny-views", M_TINY, pitch=128, off=8),
    Bin("apply-odd-tail", 128 * 9 + 77, seed=3),
    Bin("apply-u1-ragged-soft-views", M_U1, targets="soft", pitch=192, off=64, seed=1),
]
LARGE_M = M_U1   # cases at or above: run twice, bitwise equal


@dataclass(frozen=True)
class HeadK:
    name: str
    K: int
    M: int
    pitch: int = 64
    off: int = 0
    labels: str = "mixed"      # "mixed": classes, 10 % 255, a few in K..254 | "ignored": all 255
    seed: int = 0

    @property
    def views(self) -> bool:
        return self.pitch > HEAD_C

    @property
    def pads(self):
        return self.off, self.pitch - HEAD_C - self.off


K_CASES = [
    HeadK("k2-tiny", 2, M_TINY),
    HeadK("k2-u3-ragged", 2, M_U3),
    HeadK("k3-u0-only", 3, M_U0),
    HeadK("k3-pass2-ragged", 3, M_PASS2),
    HeadK("k5-tiny-views", 5, M_TINY, pitch=128, off=8),
    HeadK("k5-u1-ragged", 5, M_U1),
    HeadK("k8-u0-only-views", 8, M_U0, pitch=192, off=64),
    HeadK("k8-u1-ragged", 8, M_U1, seed=1),
    HeadK("k8-pass2-ragged", 8, M_PASS2),
    HeadK("k3-pass2-all-ignored", 3, M_PASS2, labels="ignored"),
]
# (name, class weights on, dice_w): the plain kernels and the three extended forms
K_MODES = [("plain", False, 0.0), ("weights", True, 0.0), ("dice1", False, 1.0), ("weights-dice2.5", True, 2.5)]
DICE_WS = (0.0, 1.0, 2.5)
DICE_EPS = 1.0


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------

W_VALUES = (-0.25, -0.125, 0.0, 0.125, 0.25)
HOT_AMP = 9


def head_weights(rows: int, gen: torch.Generator) -> torch.Tensor:
    """[rows, 64] fp32 in {0, +-1/8, +-1/4}; neighbouring channels of a row always differ, so a kernel that
    uses a neighbour's weight changes every such element."""
    vals = torch.tensor(W_VALUES)
    idx = torch.randint(0, 5, (rows, HEAD_C), generator=gen)
    for c in range(1, HEAD_C):
        same = idx[:, c] == idx[:, c - 1]
        idx[same, c] = (idx[same, c] + 1 + torch.randint(0, 4, (int(same.sum()),), generator=gen)) % 5
    return vals[idx].float()


def bn_apply64(y: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """fp64 relu(y * scale + shift) of a 64-channel tensor, on y's device."""
    return L.apply_ref(y, coef, 1)


def relu_mask(y: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    sc, sh = (coef[k * HEAD_C:(k + 1) * HEAD_C].double().to(y.device) for k in (2, 3))
    return (y.double() * sc + sh) > 0


def xhat(y: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    mean, inv = (coef[k * HEAD_C:(k + 1) * HEAD_C].double().to(y.device) for k in (0, 1))
    return (y.double() - mean) * inv


def _activation(M: int, w_dir: torch.Tensor, coef: torch.Tensor, gen: torch.Generator, hot: float = 0.025, amp_max: int = HOT_AMP):
    """y [1, 1, M, 64] bf16 of integers -3..3. A `hot` share of the pixels is driven along +-w_dir (a [64] weight
    row) through the BN's sign, at amplitude 1..HOT_AMP: those saturate the sigmoid / softmax, some out to
    |x| ~ 40. (|y| <= 9 under |scale| <= 2 and |shift| <= 1 keeps a <= 19 in units of 1/4: 7 bits, exact in bf16.)"""
    y = torch.randint(-3, 4, (M, HEAD_C), generator=gen)
    sc = coef[2 * HEAD_C:3 * HEAD_C]
    is_hot = torch.rand(M, generator=gen) < hot
    is_hot[1] = is_hot[M // 2] = True      # the smallest cases saturate too: one pixel each way, the first at full
    n = int(is_hot.sum())
    if n:
        amp = torch.randint(1, amp_max + 1, (n, 1), generator=gen)
        side = torch.randint(0, 2, (n, 1), generator=gen) * 2 - 1
        amp[0], amp[-1], side[0], side[-1] = amp_max, amp_max - 2, 1, -1
        want = torch.where(w_dir[None, :] * side > 0, 1, -1)           # channels to switch on (+) / off (-)
        y[is_hot] = (want * amp * torch.sign(sc)[None, :].long()).long()
    return y.to(BF16).view(1, 1, M, HEAD_C)


def bn_coef(gen: torch.Generator) -> torch.Tensor:
    """[mean | invstd | scale | shift]: integer mean, invstd = 2^k, scale = +-2^k (k = -2..1), integer shift."""
    return L.bn_lattice_coef(HEAD_C, gen)


@functools.lru_cache(maxsize=3)
def _bin_data(M: int, targets: str, seed: int):
    g = L.generator(31000 + seed)
    coef = bn_coef(g)
    w = head_weights(1, g)[0]
    b = torch.tensor([0.125 * int(torch.randint(-4, 5, (1,), generator=g))])
    y = _activation(M, w, coef, g)
    a64 = bn_apply64(y, coef)
    # centre the logits: the post-ReLU activation is non-negative, so w . E[a] is not zero
    x0 = (a64.view(M, HEAD_C) @ w.double())
    b = b - torch.round(x0.median() * 8) / 8
    b = b.float()
    if targets == "binary":
        t = torch.randint(0, 2, (M,), generator=g).float()
    elif targets == "soft":
        t = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (M,), generator=g)]
    else:
        t = torch.zeros(M)
    t[1] = 0.0   # the forced saturated pixel (x >> 0): with t = 1 its gradient would cancel to ~0, all slop
    return {"y": y, "coef": coef, "a": a64.to(BF16), "a64": a64, "w": w, "b": b, "t": t}


def bin_data(c: Bin):
    """y (pre-BN, integers), coef, a = relu(bn(y)) (exact in bf16), w [64], b [1], t [M] fp32."""
    return _bin_data(c.M, c.targets, c.seed)


def bwd_coef2(M: int, gen: torch.Generator) -> torch.Tensor:
    """coef2 = [A | B | K] of head_bn_bwd_apply: A = +-2^k (k = -1..1); B and K are integers -2..2 times the
    quantum 2^-(ceil(log2 M) + 4), the size of g = dlogit * w there, so no term of dy = A g + B y + K swamps g."""
    q = 2.0 ** -(math.ceil(math.log2(M)) + 4)
    return torch.cat([L.pow2_signed(HEAD_C, gen, -1, 1), L.int_vector(HEAD_C, gen, 2) * q,
                      L.int_vector(HEAD_C, gen, 2) * q])


KW_VALUES = tuple(k / 16 for k in range(-4, 5))
K_HOT = 0.012


def k_weights(K: int, gen: torch.Generator):
    """w [K, 64] of multiples of 1/16 in -1/4..1/4 whose K values at every channel are all different, and b [K] of
    multiples of 1/8. da[c] = sum_k dlogit_k w[k][c] with sum_k dlogit_k = 0: where two class rows carried the same
    weight at a channel, da would cancel towards 0 at every pixel those two classes share, leaving only slop.
    Channels 0 and 1 carry the tie probes of headk_mask, through the biases (0, 1/8, 1/4, ...) rather than equal
    weights: a pixel 2 e_0 gives classes 0, 1, 2 the logit 1/2 (K = 2: classes 0, 1) and the rest at most 1/8; a
    pixel 2 e_1 gives classes 1 and 2 the logit 5/8, class 0 -1/2 and the rest at most 1/4."""
    vals = torch.tensor(KW_VALUES if K > 5 else W_VALUES)   # up to 5 classes: gaps of 1/8 at least (less cancellation)
    cols = []
    while len(cols) < HEAD_C:   # neighbouring channels differ in some class row
        col = vals[torch.randperm(vals.numel(), generator=gen)[:K]]
        if not cols or not torch.equal(col, cols[-1]):
            cols.append(col)
    w = torch.stack(cols, 1)
    w[:, 2] = w[:, 2].roll(1)   # (channels 0 and 1 are set below: channel 2 then differs from both wherever it did not)
    b = 0.125 * torch.randint(-1, 2, (K,), generator=gen).float()
    b[:3] = torch.tensor([0.0, 0.125, 0.25])[:min(K, 3)]
    w[:3, 0] = torch.tensor([0.25, 0.1875, 0.125])[:min(K, 3)]
    w[:3, 1] = torch.tensor([-0.25, 0.25, 0.1875])[:min(K, 3)]
    if K > 3:
        w[3:, 0] = torch.tensor([0.0, -0.0625, -0.125, -0.1875, -0.25])[torch.randperm(5, generator=gen)[:K - 3]]
        w[3:, 1] = torch.tensor([0.0, -0.0625, -0.125, -0.1875, 0.0625])[torch.randperm(5, generator=gen)[:K - 3]]
    return w.float(), b


@functools.lru_cache(maxsize=3)
def _k_data(K: int, M: int, labels: str, seed: int):
    g = L.generator(32000 + 17 * K + seed)
    coef = bn_coef(g)                      # only to shape the activation as the binary cases do
    w, b = k_weights(K, g)
    a = bn_apply64(_activation(M, w[K - 1] - w[0], coef, g, hot=K_HOT, amp_max=HOT_AMP if K > 5 else 6), coef).view(M, HEAD_C)
    probes = torch.arange(3, M, 7)[:48]
    a[probes] = 0
    a[probes, probes % 2] = 2.0
    lab = torch.randint(0, K, (M,), generator=g)
    lab[torch.rand(M, generator=g) < 0.1] = 255
    odd = torch.randperm(M, generator=g)[:max(2, M // 97)]
    lab[odd] = torch.randint(K, 255, (odd.numel(),), generator=g)
    # Where the softmax saturates on the labelled class, softmax - onehot cancels to ~0 and all 64 elements of da at
    # that pixel are slop only; all but every sixteenth of those pixels get another class as their label instead
    x = logits64(a, w, b)
    top = x.argmax(1)
    sat = (x.max(1).values - x.topk(2, 1).values[:, 1] > 5) & (lab == top)
    if M >= M_U0:                    # (one such pixel would be 3 % of the smallest cases)
        sat &= sat.cumsum(0) % 16 != 1   # the 1st, 17th, ... stay as they are
    lab[sat] = (top[sat] + 1) % K
    if labels == "ignored":
        lab[:] = 255
    cw = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=g)]
    cw[K - 1] = 0.0                        # one zero-weight class
    return {"a": a.to(BF16).view(1, 1, M, HEAD_C), "a64": a.view(1, 1, M, HEAD_C), "w": w, "b": b,
            "lab": lab.to(torch.uint8), "cw": cw, "probes": probes}


def k_data(c: HeadK):
    """a (exact in bf16), w [K, 64], b [K], labels u8 [M], dyadic class weights cw [K] (the last one 0)."""
    return _k_data(c.K, c.M, c.labels, c.seed)


# ---------------------------------------------------------------------------------------------
# binary head: fp64 reference and error bounds
# ---------------------------------------------------------------------------------------------

def logits64(a64: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[M] (w [64]) or [M, K] (w [K, 64]) in fp64."""
    x = a64.reshape(-1, HEAD_C) @ w.double().reshape(-1, HEAD_C).t() + b.double()
    return x[:, 0] if w.dim() == 1 else x


def sig_rel(x: torch.Tensor) -> torch.Tensor:
    """Relative error of the fp32 sigmoid [1 | e] / (1 + e), e = __expf(-|x|): the intrinsic (the error of e
    moves the quotient by less than its own relative size), one addition, one division."""
    return expf_rel(x) + U32 + DIVU


def bin_ref(x: torch.Tensor, t: torch.Tensor, dice_w: float, eps: float = DICE_EPS, gscale: float = 1.0):
    """Per-pixel fp64 reference of head_fwd / head_bwd from the exact logits x [M] and targets t [M]."""
    M = x.numel()
    t = t.double()
    e = torch.exp(-x.abs())
    sg = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(e)
    sums = torch.stack([bce.sum(), (sg * t).sum(), sg.sum(), t.sum()])
    I, den = sums[1], sums[2] + sums[3] + eps
    dice = 1 - (2 * I + eps) / den
    loss = torch.stack([sums[0] / M + dice_w * dice, sums[0] / M])
    dx = (sg - t) / M
    ddp = -(2 * t * den - (2 * I + eps)) / (den * den)
    if dice_w:
        dx = dx + dice_w * ddp * sg * (1 - sg)
    r = {"x": x, "t": t, "e": e, "sg": sg, "bce": bce, "sums": sums, "loss": loss, "dx": dx * gscale, "ddp": ddp,
         "den": den, "I": I, "M": M, "dice_w": dice_w, "gscale": gscale, "sr": sig_rel(x)}
    r["sum_bounds"], r["loss_bounds"] = bin_loss_bounds(r)
    r["dx_slop"] = bin_dx_slop(r)
    return r


def bin_loss_bounds(r):
    """(bounds of sums[0..3] [4], bounds of loss [2]). A lane adds one term per pass, then 6 shuffle steps and 3
    wave additions; the rows are folded in fp64 (and sums[] rounded to fp32 once: one more).
    bce term: max(x, 0) - x t + log1pf(e): e off by expf_rel e (d log1p / de <= 1), log1pf by LOG1P_REL, two
    additions of magnitudes <= |x| + log 2 (x t is exact: t dyadic). sg t and sg: sig_rel sg. t: exact.
    The loss is formed in fp64 from the folded rows and rounded once."""
    x, e, sg, t, M = r["x"], r["e"], r["sg"], r["t"], r["M"]
    n = (passes(M) + 6 + 3 + 1) * U32
    term = expf_rel(x) * e + LOG1P_REL * torch.log1p(e) + 2 * U32 * (x.abs() + 1)
    mag = torch.clamp(x, min=0) + (x * t).abs() + torch.log1p(e)
    bs = torch.stack([term.sum() + n * mag.sum(), (r["sr"] * sg * t).sum() + n * (sg * t).sum(),
                      (r["sr"] * sg).sum() + n * sg.sum(), torch.zeros((), dtype=torch.float64)])
    den = r["den"]
    ddice = 2 * bs[1] / den + (2 * r["I"] + DICE_EPS) / (den * den) * bs[2]
    bl = torch.stack([bs[0] / M + r["dice_w"] * ddice + U32 * r["loss"][0].abs(), bs[0] / M + U32 * r["loss"][1].abs()])
    return bs, bl


def bin_dx_slop(r) -> torch.Tensor:
    """|fp32 dlogit - dx| per pixel, from head_dlogit's operations (the GRAD forward's (sgm - t) * gs is the
    dice_w = 0 form with one operation fewer):
      sg           : sig_rel sg
      sg - t       : + U32 |sg - t|
      * invM       : invM = 1.f / (float)M is one division, the product one rounding
      ddp          : num = 2 t den - (2 I + eps) with I and P as read back from fp32 sums (off by their sum_bounds);
                     U = P + T and den = U + eps round (3 U32 den with T's own rounding); |num| and 2 I + eps are
                     <= 3 den and round once each; den * den: twice den's relative error + U32; the division
      sg (1 - sg)  : sig_rel q + sg (sig_rel sg + U32 (1 - sg)) + U32 q, q = sg (1 - sg)
      dice_w * ddp * q : two more roundings; the sum of the two parts and * gscale: two more."""
    sg, t, M, den, ddp, dw, sr = r["sg"], r["t"], r["M"], r["den"], r["ddp"], r["dice_w"], r["sr"]
    d1 = (sr * sg + U32 * (sg - t).abs()) / M + (sg - t).abs() / M * (DIVU + U32)
    tot = ((sg - t) / M).abs()
    if dw:
        dI = r["sum_bounds"][1]
        dden = r["sum_bounds"][2] + 3 * U32 * den
        dnum = 2 * t * dden + 2 * dI + 6 * U32 * den
        dddp = dnum / (den * den) + ddp.abs() * (2 * dden / den + U32 + DIVU)
        q = sg * (1 - sg)
        dq = sr * q + sg * (sr * sg + U32 * (1 - sg)) + U32 * q
        d1 = d1 + dw * (dddp * q + ddp.abs() * dq + 2 * U32 * ddp.abs() * q)
        tot = tot + dw * ddp.abs() * q
    return (d1 + 2 * U32 * tot) * r["gscale"]


def outer_bounds(dx: torch.Tensor, slop: torch.Tensor, w: torch.Tensor):
    """(ref, slop) [M, 64] of da = dlogit * w[c]: the weights are powers of two (or 0), the product is exact."""
    w = w.double().to(dx.device)
    return dx[:, None] * w[None, :], slop[:, None] * w.abs()[None, :]


def within(got: torch.Tensor, ref: torch.Tensor, slop: torch.Tensor) -> float:
    """max over the elements of |got - ref| / (1/2 ulp_bf16(ref) + slop); inf where a zero bound is missed."""
    bound = 0.5 * L.ulp_bf16(ref) + slop
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return math.inf if not bool(ok.all()) and ratio.max().item() <= 1 else ratio.max().item()


def round_pair(ref: torch.Tensor, slop: torch.Tensor):
    """The bf16 values a quantity within `slop` of ref can round to: (lowest, highest), both fp64."""
    return (ref - slop).float().to(BF16).double(), (ref + slop).float().to(BF16).double()


def tie_share(ref: torch.Tensor, slop: torch.Tensor) -> float:
    lo, hi = round_pair(ref, slop)
    return (lo != hi).double().mean().item()


def bn_fused_ref(r, y: torch.Tensor, coef: torch.Tensor, w: torch.Tensor):
    """The composite behind the BN-fused forms, on y's device: g = bf16(dlogit * w) * relu'(y), the BN-backward
    sums {sum g, sum g * xhat} with their bounds. g is taken at RNE of the reference; where dlogit * w lies within
    its slop of a bf16 rounding tie either neighbour is legal, and the bounds of the sums grow by that element's
    ulp. g * xhat is exact in fp32 (8 bits times a small dyadic), so only the additions round."""
    dev = y.device
    ref, slop = outer_bounds(r["dx"].to(dev), r["dx_slop"].to(dev), w)
    mask = relu_mask(y, coef).view(-1, HEAD_C)
    xh = xhat(y, coef).view(-1, HEAD_C)
    lo, hi = round_pair(ref, slop)
    g = ref.float().to(BF16).double() * mask
    amb = (hi - lo).abs() * mask
    n = chain(r["M"]) * U32
    sums = torch.stack([g.sum(0), (g * xh).sum(0)])
    bounds = torch.stack([n * g.abs().sum(0) + amb.sum(0), n * (g * xh).abs().sum(0) + (amb * xh.abs()).sum(0)])
    return {"g_lo": lo * mask, "g_hi": hi * mask, "sums": sums, "bounds": bounds,
            "amb_share": (amb != 0).double().mean().item(), "kept_share": mask.double().mean().item()}


def head_grad_ref(r, a64: torch.Tensor, final: bool):
    """gw [64] = sum dlogit * a, gb = sum dlogit with bounds: every term is one fma of a value off by dx_slop,
    summed over chain (block rows, folded in fp64) or chain_final (the finalized gradient) additions."""
    dev = a64.device
    dx, sl = r["dx"].to(dev), r["dx_slop"].to(dev)
    a = a64.view(-1, HEAD_C)
    n = (chain_final(r["M"]) if final else chain(r["M"])) * U32
    return dx @ a, sl @ a.abs() + n * (dx.abs() @ a.abs()), dx.sum(), sl.sum() + n * dx.abs().sum()


# ---------------------------------------------------------------------------------------------
# K-class head: fp64 reference and error bounds
# ---------------------------------------------------------------------------------------------

def argmax_lowest(x: torch.Tensor) -> torch.Tensor:
    """The lowest index among the maxima of each row, without relying on argmax's tie rule."""
    eq = x == x.max(1, keepdim=True).values
    idx = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(eq, idx, torch.full_like(idx, x.shape[1])).min(1).values


def top_ties(x: torch.Tensor) -> torch.Tensor:
    """How many classes attain each row's maximum."""
    return (x == x.max(1, keepdim=True).values).sum(1)


def k_ref(x: torch.Tensor, lab: torch.Tensor, cw, dice_w: float, eps: float = DICE_EPS, gscale: float = 1.0):
    """fp64 reference of headk_fwd / headk_bwd from the exact logits x [M, K]. cw = None with dice_w = 0 is the
    plain mode. Returns the sums row with its bounds, the loss pair, dlogit [M, K] (times gscale) and its
    per-element slop.

    Softmax value s_k = e_k / se in fp32: __expf on every term (se's relative error is the e-weighted mean of
    theirs), K - 1 additions of non-negative terms, one division (or a reciprocal and a product): `es` (below).
    I_k / P_k as the backward reads them: es s per term, `chain` additions and the rounding of sums[] to fp32."""
    M, K = x.shape
    ext = cw is not None or dice_w != 0
    lab = lab.long()
    kept = lab < K
    kf = kept[:, None].double()
    li = torch.where(kept, lab, torch.zeros_like(lab))
    oh = torch.zeros(M, K, dtype=torch.float64)
    oh[kept, li[kept]] = 1.0
    mx = x.max(1, keepdim=True).values
    ex = torch.exp(x - mx)
    se = ex.sum(1, keepdim=True)
    s = ex / se
    er_e = expf_rel(x - mx)
    se_rel = (ex * er_e).sum(1, keepdim=True) / se + (K - 1) * U32
    # the same e_j feed the numerator and se, so their errors partly cancel in the quotient: with E_j = expf_rel,
    # d s_k / s_k = E_k - sum_j s_j E_j = (1 - s_k) E_k - sum_{j != k} s_j E_j. Near s_k = 1, where s_k - 1 cancels,
    # the intrinsic's error therefore shrinks with 1 - s_k; only the roundings of the sum and the division stay
    sE = s * er_e
    es = (1 - s) * er_e + (sE.sum(1, keepdim=True) - sE) + (K - 1) * U32 + DIVU + U32
    ce = (mx + torch.log(se))[:, 0] - x.gather(1, li[:, None])[:, 0]
    cwv = torch.ones(K, dtype=torch.float64) if cw is None else cw.double()
    wt = torch.where(kept, cwv[li], torch.zeros(M, dtype=torch.float64))
    sk = s * kf
    Ik, Pk, Tk = (sk * oh).sum(0), sk.sum(0), oh.sum(0)
    Wsum = wt.sum()
    sce = (wt * ce).sum()
    n = (chain(M) + 1) * U32
    zero = torch.zeros((), dtype=torch.float64)
    # ce = mx + logf(se) - x[label]: se's relative error moves the log by as much absolutely, logf's own error
    # is absolute on [1, 8], two additions of magnitudes <= 2 max|x| + log K; the class weight is dyadic
    t_ce = (se_rel[:, 0] + LOGF_ABS + 2 * U32 * (2 * x.abs().max(1).values + math.log(K))) * wt
    b_ce = t_ce.sum() + n * (wt * ce.abs()).sum()
    dI, dP = (es * sk * oh).sum(0) + n * Ik, (es * sk).sum(0) + n * Pk
    if not ext:
        cnt = max(float(kept.sum()), 1.0)
        sums, sum_bounds = torch.stack([sce, Wsum]), torch.stack([b_ce, zero])
        loss = torch.stack([sce / cnt, sce / cnt])
        loss_bounds = (b_ce / cnt + U32 * loss[0].abs()).expand(2)
        dl = (s - oh) * kf / cnt
        # (s - oh) * invc: the softmax value, one subtraction (or fma), invc = 1 / count (a division), a product
        ddl = ((es * s + U32 * (s - oh).abs()) + (s - oh).abs() * (DIVU + U32)) * kf / cnt
    else:
        sums = torch.cat([torch.stack([sce, Wsum]), Ik, Pk, Tk])
        sum_bounds = torch.cat([torch.stack([b_ce, zero]), dI, dP, torch.zeros(K, dtype=torch.float64)])
        CE = sce / Wsum if Wsum > 0 else zero
        D = Pk + Tk + eps
        dice = 1 - ((2 * Ik + eps) / D).sum() / K
        loss = torch.stack([CE + dice_w * dice, CE])
        b_CE = b_ce / Wsum if Wsum > 0 else zero
        b_dice = ((2 * dI) / D + (2 * Ik + eps) / (D * D) * dP).sum() / K
        loss_bounds = torch.stack([b_CE + dice_w * b_dice + U32 * loss[0].abs(), b_CE + U32 * loss[1].abs()])
        invW = 1 / Wsum if Wsum > 0 else 0.0
        A = -2 * dice_w / (K * D)
        B = dice_w * (2 * Ik + eps) / (K * D * D)
        # constants, once per thread: D = P + T + eps (two additions), rk = dice_w / (K D) (a product, a
        # division), A = -2 rk, B = rk (2 I + eps) / D (an fma, a product, a division)
        eD = dP / D + 2 * U32
        er = eD + U32 + DIVU
        eB = er + (2 * dI + U32 * (2 * Ik + eps)) / (2 * Ik + eps) + U32 + DIVU + eD
        G = B[None, :] + oh * A[None, :]
        dG = B.abs()[None, :] * eB[None, :] + oh * (A.abs() * er)[None, :] + U32 * G.abs()
        dot = (G * s).sum(1, keepdim=True)
        # s_k (G_k - dot), dot = sum_j G_j s_j. The kernel forms each G_j once per pixel and uses that one value in
        # dot and in G_k - dot, so an error dG_j in it (from the constants or the addition) moves G_k - dot by
        # (1 - s_k) dG_k - sum_{j != k} s_j dG_j: near s_k = 1, where G_k - dot cancels, it shrinks with 1 - s_k.
        # dot's own errors: the softmax values (es) and K fmas.
        sdG = s * dG
        corr = (1 - s) * dG + (sdG.sum(1, keepdim=True) - sdG)
        ddot = (G.abs() * s * (es + U32)).sum(1, keepdim=True) + K * U32 * (G * s).abs().sum(1, keepdim=True)
        second = s * (G - dot)
        dsecond = s * (corr + ddot + U32 * (G - dot).abs()) + (G - dot).abs() * s * (es + 2 * U32)
        # the CE part: fma(e, inv, -onehot) * wt, wt = cw[t] * (1 / W): W is exact (dyadic weights)
        wl = (wt * invW)[:, None]
        first = (s - oh) * wl
        dfirst = wl * ((es * s + U32 * (s - oh).abs()) + (s - oh).abs() * (DIVU + 2 * U32))
        dl = (first + second) * kf
        ddl = (dfirst + dsecond + U32 * dl.abs()) * kf
    return {"x": x, "kept": kept, "s": s, "sums": sums, "sum_bounds": sum_bounds, "loss": loss,
            "loss_bounds": loss_bounds, "dl": dl * gscale, "dl_slop": ddl * gscale, "K": K, "M": M, "ext": ext,
            "counts": Tk}


def k_da_bounds(r, w: torch.Tensor, dev, px: slice = slice(None)):
    """(ref, slop) [M, 64] (or of the pixels px) of da = sum_k dlogit_k w[k][c]: K fmas, each rounding the running
    sum once (the product inside an fma does not round), and the product with gscale."""
    dl, sl = r["dl"][px].to(dev), r["dl_slop"][px].to(dev)
    wd = w.double().to(dev)
    return dl @ wd, sl @ wd.abs() + (r["K"] + 1) * U32 * (dl.abs() @ wd.abs())


def k_grad_ref(r, a64: torch.Tensor, final: bool):
    """gw [K, 64], gb [K] and their bounds: fma terms summed over chain (the block rows, folded in fp64) or
    chain_final (the finalized gradients) additions."""
    dev = a64.device
    dl, sl = r["dl"].to(dev), r["dl_slop"].to(dev)
    a = a64.view(-1, HEAD_C)
    n = (chain_final(r["M"]) if final else chain(r["M"])) * U32
    return dl.t() @ a, sl.t() @ a.abs() + n * (dl.abs().t() @ a.abs()), dl.sum(0), sl.sum(0) + n * dl.abs().sum(0)
