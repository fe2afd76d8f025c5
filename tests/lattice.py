"""Integer-lattice inputs, fp64 references and the case tables of the exact conv tests.

Every MFMA kernel here multiplies bf16 operands and accumulates in fp32. For integer-valued operands
whose partial sums stay below 2^24 every summation order gives the same exact integer, so a kernel's
bf16 output is one fixed value: that integer rounded to nearest even. The GPU tests
(tests/test_conv_exact_gpu.py) therefore demand bitwise equality with a CPU fp64 reference; this module
builds the inputs and references and states the preconditions under which that demand is sound.
tests/test_lattice_cpu.py checks, without a GPU, that every case of the tables meets them.

The second half of the module does the same for the memory-bound passes between the convs (BN finalize /
apply / backward, max pool, bilinear upsample): tests/test_pass_exact_gpu.py, tests/test_pass_lattice_cpu.py.

Pure torch on the CPU: the native extension is never imported here.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
SENTINEL = 30080.0   # exact in bf16, far outside every expected output
F32_EXACT = float(1 << 24)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------

def generator(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ternary(shape, density: float, gen: torch.Generator) -> torch.Tensor:
    """bf16 tensor with values in {-1, 0, 1}; P(non-zero) = density."""
    shape = tuple(shape)
    nz = torch.rand(shape, generator=gen) < density
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (nz * sign).to(BF16)


def small_ints(shape, gen: torch.Generator, amax: int = 3) -> torch.Tensor:
    """bf16 tensor of uniform integers in -amax..amax (the rounding class' wider form)."""
    return torch.randint(-amax, amax + 1, tuple(shape), generator=gen).to(BF16)


def densities(K: int, target: float = 100.0) -> Tuple[float, float]:
    """(p, q) with p * q ~ target / K: the output's variance is ~target (sigma ~ 10) whatever K is."""
    p = min(1.0, math.sqrt(target / K))
    return p, p


def pow2_signed(n: int, gen: torch.Generator, kmin: int = -2, kmax: int = 1) -> torch.Tensor:
    """fp32 vector of +-2^k, k in kmin..kmax, both signs present."""
    k = torch.randint(kmin, kmax + 1, (n,), generator=gen)
    s = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    s[0], s[1] = 1, -1
    return (s * torch.pow(2.0, k.double())).float()


def int_vector(n: int, gen: torch.Generator, amax: int) -> torch.Tensor:
    return torch.randint(-amax, amax + 1, (n,), generator=gen).float()


# ---------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------

def ohwi(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, kh, kw] -> [Cout, kh * kw * Cin], the forward kernels' weight layout."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [Cin, 9 * Cout]: dX = conv(dY, flip(W)^T) through the forward kernels."""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()


def pack_first(x3: torch.Tensor, w: torch.Tensor):
    """The packed first layer: x [N,H,W,3] -> 8 stored channels, w [64,3,3,3] -> [64][16 taps][8] = [64][128]."""
    x8 = torch.zeros(*x3.shape[:3], 8, dtype=BF16)
    x8[..., :3] = x3
    wp = torch.zeros(w.shape[0], 16, 8, dtype=BF16)
    wp[:, :9, :3] = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, 3)
    return x8, wp.view(w.shape[0], 128)


# ---------------------------------------------------------------------------------------------
# fp64 references (CPU only: integer sums below 2^53 are exact in every order)
# ---------------------------------------------------------------------------------------------

def conv_ref(x_nhwc: torch.Tensor, w_oihw: torch.Tensor) -> torch.Tensor:
    """fp64 'same' conv of an NHWC tensor, NHWC result."""
    pad = w_oihw.shape[-1] // 2
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_oihw.double(), padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_grads_ref(x_nhwc: torch.Tensor, w_oihw: torch.Tensor, dy_nhwc: torch.Tensor, want_x: bool, want_w: bool):
    """fp64 autograd gradients of the 'same' conv: (dx NHWC or None, dw [Cout, Cin, kh, kw] or None)."""
    x = x_nhwc.double().permute(0, 3, 1, 2).requires_grad_(want_x)
    w = w_oihw.double().clone().requires_grad_(want_w)
    y = F.conv2d(x, w, padding=w.shape[-1] // 2)
    y.backward(dy_nhwc.double().permute(0, 3, 1, 2))
    dx = x.grad.permute(0, 2, 3, 1).contiguous() if want_x else None
    return dx, (w.grad if want_w else None)


def expected_bf16(ref64: torch.Tensor) -> torch.Tensor:
    """The one bf16 value a correct kernel can write: exact in fp32 below 2^24, then RNE to bf16."""
    return ref64.to(torch.float32).to(BF16)


# ---------------------------------------------------------------------------------------------
# preconditions: asserted on the reference alone. A case that violates one is a broken case.
# ---------------------------------------------------------------------------------------------

def assert_exact_class(ref64: torch.Tensor) -> None:
    """max|y| <= 256 (integers: no bf16 rounding) and per-channel sum(y^2) < 2^24 over the whole tensor,
    which bounds every partial sum of y or y^2 any tiling can form. Channels are the last dim."""
    assert torch.equal(ref64, ref64.round()), "reference is not integer-valued"
    amax = ref64.abs().max().item()
    assert amax <= 256, f"exact class: max|y| = {amax} > 256"
    assert amax > 0, "degenerate case: the reference is all zero"
    ssq = (ref64 * ref64).reshape(-1, ref64.shape[-1]).sum(0).max().item()
    assert ssq < F32_EXACT, f"exact class: per-channel sum y^2 = {ssq} >= 2^24"


def true_ties(ref64: torch.Tensor) -> int:
    """Odd integers in (256, 512): spacing of bf16 there is 2, so each is a true round-to-even tie."""
    a = ref64.abs()
    return int(((a > 256) & (a < 512) & (a % 2 == 1)).sum().item())


def assert_rounding_class(ref64: torch.Tensor, min_ties: int = 16) -> None:
    assert torch.equal(ref64, ref64.round()), "reference is not integer-valued"
    amax = ref64.abs().max().item()
    assert amax < F32_EXACT, f"rounding class: max|y| = {amax} >= 2^24"
    n = true_ties(ref64)
    assert n >= min_ties, f"rounding class: only {n} true bf16 ties in the reference (need {min_ties})"


def assert_f32_sums(terms64: torch.Tensor, what: str) -> None:
    """Per-channel sum|t| / quantum < 2^24, quantum = the largest power of two dividing every term: then
    every partial sum of the terms is a multiple of the quantum with < 24 significant bits, exact in fp32."""
    nz = terms64[terms64 != 0].abs()
    assert nz.numel() > 0, f"{what}: all terms are zero"
    q = 1.0
    while not torch.equal(nz / q, (nz / q).round()):
        q /= 2.0
        assert q >= 2.0 ** -16, f"{what}: terms are not dyadic"
    tot = terms64.abs().reshape(-1, terms64.shape[-1]).sum(0).max().item() / q
    assert tot < F32_EXACT, f"{what}: per-channel sum|t| / {q} = {tot} >= 2^24"


# ---------------------------------------------------------------------------------------------
# guard-banded, pitch-sliced buffers
# ---------------------------------------------------------------------------------------------

GUARD = 512  # elements on each side (a multiple of 8: the view stays 16-byte aligned)


def embed(t: Optional[torch.Tensor], shape, pad_lo: int, pad_hi: int, device, dtype=BF16, fill=SENTINEL):
    """A [N,H,W,C] view (pixel pitch pad_lo + C + pad_hi, channel offset pad_lo) inside a flat buffer
    with GUARD sentinel elements before and after. pad_lo and the pitch must be multiples of 8.
    Returns (flat, view); the view holds t (or the sentinel if t is None)."""
    N, H, W, C = shape
    pitch = pad_lo + C + pad_hi
    assert pad_lo % 8 == 0 and pitch % 8 == 0
    flat = torch.full((2 * GUARD + N * H * W * pitch,), fill, dtype=dtype, device=device)
    view = flat[GUARD:GUARD + N * H * W * pitch].view(N, H, W, pitch)[..., pad_lo:pad_lo + C]
    if t is not None:
        view.copy_(t)
    return flat, view


def outside_view_intact(flat: torch.Tensor, view: torch.Tensor, fill=SENTINEL) -> bool:
    """True if every element of flat that is not part of view still holds the sentinel, bit for bit."""
    probe = flat.clone()
    off = view.storage_offset() - flat.storage_offset()
    probe.as_strided(view.shape, view.stride(), off).fill_(fill)
    bits = torch.int16 if flat.dtype == BF16 else torch.int32
    return torch.equal(probe.view(bits), torch.full_like(flat, fill).view(bits))


# ---------------------------------------------------------------------------------------------
# forward / eval / dgrad cases
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Conv:
    """One conv_fwd launch: cat(x1, x2) [N,H,W,C1+C2] -> Cout, on the kernel `pref` names: an RdpConvKernel
    enumerator of csrc/conv_plan.h without its prefix (the extension exports its value as _C.CONV_<name>)."""
    name: str
    N: int
    H: int
    W: int
    C1: int
    C2: int
    Cout: int
    pref: str
    taps: int = 9
    packed: bool = False     # first layer: 3 real channels stored as 8, C1 = 8
    cls: str = "exact"       # "exact" | "round"
    stats: bool = True       # exact class only
    split: int = 0           # > 0: two destinations y1 [.., split] | y2 [.., Cout - split]
    views: bool = False      # pitch-sliced inputs / outputs inside guard bands
    ws: bool = False         # split-K workspace of conv_ws_elems (must be > 0), NaN-filled
    evalmode: bool = False   # affine = +-2^k scales, integer shifts, ReLU
    pool: bool = False       # eval: fused 2x2 max pool output
    wfrag: int = 0           # eval through the fragment-major weight copy: expected rowband_frag_mode
    amax: int = 3            # rounding class: operand range -amax..amax
    seed: int = 0

    @property
    def K(self) -> int:
        return 27 if self.packed else self.taps * (self.C1 + self.C2)

    @property
    def M(self) -> int:
        return self.N * self.H * self.W


def _c(name, shape, pref, **kw):
    return Conv(name, *shape, pref, **kw)


S_TINY = (3, 7, 5, 64, 0, 64)          # M = 105: one ragged tile, odd H / W, N > 1
S_DUAL = (2, 9, 13, 64, 64, 128)       # M = 234: ragged, odd, two sources
S_PP = (3, 37, 29, 128, 0, 256)        # M = 3219: 13 tiles of 256, ragged last
S_PPD = (1, 24, 40, 128, 128, 256)     # ping-pong, two sources
S_SK7 = (5, 37, 29, 256, 0, 512)       # M = 5365: split-K ping-pong 256 x 128, ragged
S_SK8 = (4, 32, 32, 512, 0, 512)       # split-K ping-pong 256 x 256
S_FIRST = (1, 7, 9, 8, 0, 64)
S_FIRST2 = (2, 20, 12, 8, 0, 64)

FWD_CASES = [
    # implicit GEMM, 4- and 8-wave tiles, auto
    _c("auto-256x64", S_TINY, "AUTO"),
    _c("auto-128x128", S_DUAL, "AUTO"),
    _c("tile128-split-views", S_DUAL, "IGEMM4_128", split=64, views=True),
    _c("tile256", S_TINY, "IGEMM4_256"),
    _c("wave8-128", S_DUAL, "IGEMM8_128"),
    _c("wave8-256-views", S_TINY, "IGEMM8_256", views=True),
    _c("tile128-round", S_DUAL, "IGEMM4_128", cls="round", stats=False),
    # ping-pong
    _c("pp256", S_PP, "PP256"),
    _c("pp128-split-views", S_PPD, "PP128", split=128, views=True),
    _c("pp256-round", S_PP, "PP256", cls="round", stats=False),
    # split-K ping-pong (NaN-filled workspace)
    _c("ppsk128", S_SK7, "PPSK128", ws=True),
    _c("ppsk256-split", S_SK8, "PPSK256", ws=True, split=256),
    _c("ppsk128-views", (4, 32, 32, 256, 0, 512), "PPSK128", ws=True, views=True),
    _c("ppsk128-round", S_SK7, "PPSK128", ws=True, cls="round", stats=False),
    # auto split-K of the implicit GEMM (small M, long K)
    _c("splitk-auto", (2, 7, 9, 128, 0, 64), "AUTO", ws=True),
    _c("splitk-auto-dual-split", (1, 8, 8, 256, 256, 256), "AUTO", ws=True, split=128),
    _c("splitk-auto-round", (1, 8, 8, 256, 256, 256), "AUTO", ws=True, cls="round", stats=False),
    # halo tiles 16 x 16, 64 x 4, 32 x 8
    _c("halo16", (3, 16, 16, 64, 0, 128), "HALO"),
    _c("halo64-dual-views", (1, 8, 128, 64, 64, 128), "HALO", views=True),
    _c("halo32", (2, 16, 32, 128, 0, 64), "HALO"),
    _c("halo16-round", (3, 16, 16, 64, 0, 128), "HALO", cls="round", stats=False),
    # row ring, 64 -> 64 and 64 -> 128 (two destinations)
    _c("ring-3seg", (3, 2, 192, 64, 0, 64), "RING"),
    _c("ring-views", (2, 6, 64, 64, 0, 64), "RING", views=True),
    _c("ring-cout128-split", (2, 2, 64, 64, 0, 128), "RING", split=64),
    _c("ring-round", (2, 6, 64, 64, 0, 64), "RING", cls="round", stats=False),
    # two-source ring, 128 -> 64 (RING2) and 128 -> 128 as halves (RING2X2)
    _c("ring2-concat", (3, 2, 192, 64, 64, 64), "RING2"),
    _c("ring2-one128-views", (2, 6, 64, 128, 0, 64), "RING2", views=True),
    _c("ring2x2-concat", (1, 6, 64, 64, 64, 128), "RING2X2"),
    _c("ring2x2-one128-views", (2, 8, 128, 128, 0, 128), "RING2X2", views=True),
    _c("ring2-round", (2, 6, 64, 128, 0, 64), "RING2", cls="round", stats=False),
    # first layer, packed (K = 27: the rounding case needs operands in -7..7 to reach 256)
    _c("first", S_FIRST, "FIRST", packed=True),
    _c("first-views", S_FIRST2, "FIRST", packed=True, views=True),
    _c("first-round", S_FIRST2, "FIRST", packed=True, cls="round", stats=False, amax=7),
    # taps = 1 (the transposed decoder's GEMMs)
    _c("taps1-auto", (1, 4, 5, 256, 0, 512), "AUTO", taps=1),
    _c("taps1-pp128", (3, 20, 52, 256, 0, 512), "PP128", taps=1, stats=False),
]

EVAL_CASES = [
    _c("eval-tile128", S_DUAL, "IGEMM4_128", evalmode=True, stats=False),
    _c("eval-splitk-auto-pool", (1, 8, 8, 256, 256, 256), "AUTO", ws=True, evalmode=True, pool=True, stats=False),
    _c("eval-ppsk256-pool", S_SK8, "PPSK256", ws=True, evalmode=True, pool=True, stats=False),
    _c("eval-halo64-views", (1, 8, 128, 64, 64, 128), "HALO", evalmode=True, views=True, stats=False),
    _c("eval-ring-pool", (2, 6, 64, 64, 0, 64), "RING", evalmode=True, pool=True, stats=False),
    _c("eval-ring2", (2, 6, 64, 128, 0, 64), "RING2", evalmode=True, stats=False),
    _c("eval-ring2x2", (1, 6, 64, 64, 64, 128), "RING2X2", evalmode=True, stats=False),
    _c("eval-first", S_FIRST, "FIRST", packed=True, evalmode=True, stats=False),
    # row band (eval only), forced and through the fragment-major weights
    _c("rowband-dual", (3, 16, 32, 64, 64, 96), "ROWBAND", evalmode=True, stats=False),
    _c("rowband-pool-views", (2, 16, 16, 256, 256, 128), "ROWBAND", evalmode=True, pool=True, views=True, stats=False),
    _c("rowband-round", (3, 16, 32, 64, 64, 96), "ROWBAND", evalmode=True, cls="round", stats=False),
    _c("wfrag-mode1", (1, 16, 16, 64, 0, 64), "AUTO", evalmode=True, wfrag=1, stats=False),
    _c("wfrag-mode2-pool", (1, 16, 16, 256, 0, 128), "AUTO", evalmode=True, wfrag=2, pool=True, stats=False),
]


@functools.lru_cache(maxsize=6)
def _conv_data(N, H, W, C1, C2, Cout, taps, packed, cls, amax, seed, cout_limit):
    g = generator(1000 + seed)
    co = Cout if cout_limit is None else min(Cout, cout_limit)
    k = 3 if taps == 9 else 1
    cin = 3 if packed else C1 + C2
    K = k * k * cin
    if cls == "exact":
        p, q = densities(K)
        x = ternary((N, H, W, cin), p, g)
        w = ternary((Cout, cin, k, k), q, g)
    else:
        x = small_ints((N, H, W, cin), g, amax)
        w = small_ints((Cout, cin, k, k), g, amax)
    ref = conv_ref(x, w[:co])
    return x, w, ref


def conv_data(c: Conv, cout_limit: Optional[int] = None):
    """(x [N,H,W,Cin] bf16, w [Cout,Cin,k,k] bf16, ref [N,H,W,Cout'] fp64). cout_limit (CPU test only)
    references the first channels alone; the inputs are the same."""
    return _conv_data(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.taps, c.packed, c.cls, c.amax, c.seed, cout_limit)


def eval_coef(c: Conv):
    """(scale, shift) fp32: +-2^k and integers, so relu(scale * y + shift) is exact in fp32 whether the
    kernel fuses the multiply-add or not. The rounding-class row-band case keeps the identity."""
    g = generator(2000 + c.seed)
    if c.cls == "round":
        return torch.ones(c.Cout), torch.zeros(c.Cout)
    return pow2_signed(c.Cout, g), int_vector(c.Cout, g, 8)


def eval_ref(c: Conv, ref64: torch.Tensor) -> torch.Tensor:
    sc, sh = eval_coef(c)
    n = ref64.shape[-1]
    return torch.relu(ref64 * sc[:n].double() + sh[:n].double())


def check_conv_case(c: Conv, ref64: torch.Tensor) -> None:
    """The case's preconditions, on the reference alone."""
    if c.cls == "exact":
        assert_exact_class(ref64)
    else:
        assert not c.stats
        assert_rounding_class(ref64)
    if c.evalmode:
        e = eval_ref(c, ref64)
        assert e.abs().max().item() * 4 < F32_EXACT          # multiples of 1/4: exact in fp32
        assert (e == 0).any() and (e > 0).any()              # ReLU cuts and passes
        sc, _ = eval_coef(c)
        if c.cls == "exact":
            assert (sc > 0).any() and (sc < 0).any()         # ... on both sides


@dataclass(frozen=True)
class Dgrad:
    """dX [N,H,W,Cs+Cu] of a 3x3 conv (Cs+Cu -> Cdy) from dY, through conv_fwd on the flipped transposed
    weight, written to the concat's two destinations."""
    name: str
    N: int
    H: int
    W: int
    Cdy: int
    Cs: int
    Cu: int
    pref: str
    ws: bool = False
    views: bool = False
    seed: int = 0


DGRAD_CASES = [
    Dgrad("dgrad-auto", 2, 12, 10, 64, 64, 64, "AUTO"),
    Dgrad("dgrad-halo-views", 2, 8, 64, 128, 64, 64, "HALO", views=True),
    Dgrad("dgrad-ring", 2, 2, 64, 64, 64, 64, "RING"),
    Dgrad("dgrad-pp128", 1, 24, 40, 256, 128, 128, "PP128"),
    Dgrad("dgrad-ppsk128", 4, 32, 32, 256, 256, 256, "PPSK128", ws=True),
    Dgrad("dgrad-splitk-auto-views", 1, 8, 8, 512, 128, 128, "AUTO", ws=True, views=True),
]


@functools.lru_cache(maxsize=4)
def _dgrad_data(N, H, W, Cdy, Cdx, seed, cdx_limit):
    g = generator(3000 + seed)
    p, q = densities(9 * Cdy)
    dy = ternary((N, H, W, Cdy), p, g)
    w = ternary((Cdy, Cdx, 3, 3), q, g)  # the forward conv's weight: Cdx inputs -> Cdy outputs
    cx = Cdx if cdx_limit is None else min(Cdx, cdx_limit)
    x0 = torch.zeros(N, H, W, cx, dtype=BF16)
    dx, _ = conv_grads_ref(x0, w[:, :cx], dy, True, False)
    return dy, w, dx


def dgrad_data(N, H, W, Cdy, Cdx, seed=0, cdx_limit=None):
    """(dy bf16, forward weight w [Cdy, Cdx, 3, 3] bf16, dx [N,H,W,Cdx'] fp64 by autograd)."""
    return _dgrad_data(N, H, W, Cdy, Cdx, seed, cdx_limit)


@dataclass(frozen=True)
class BnRed:
    """A dgrad with the owner BN layer's backward reduction fused: rows of sum(g), sum(g * xhat)."""
    name: str
    N: int
    H: int
    W: int
    Cdy: int
    Cdx: int
    splitk: bool   # what the plan must answer: a split-K conv whose reduce writes the rows (else the BNRED ring)
    seed: int = 0


BNRED_CASES = [
    BnRed("bnred-ring", 2, 6, 64, 64, 64, False),
    BnRed("bnred-ring-3seg", 3, 2, 192, 64, 64, False),
    BnRed("bnred-splitk", 2, 8, 8, 128, 64, True),
    BnRed("bnred-splitk-512", 4, 16, 16, 512, 512, True),
]


def bnred_data(b: BnRed, cdx_limit=None):
    """dy, w, dx64 as dgrad_data, plus y (ternary pre-BN output of the owner layer), coef = [mean | invstd |
    scale | shift] (integer mean, power-of-two invstd and scale, integer shift) and the fp64 sums
    [2][Cdx'] of g = dx * [scale * y + shift > 0] and g * (y - mean) * invstd."""
    dy, w, dx = dgrad_data(b.N, b.H, b.W, b.Cdy, b.Cdx, 50 + b.seed, cdx_limit)
    g = generator(4000 + b.seed)
    y = ternary((b.N, b.H, b.W, b.Cdx), 0.7, g)
    mean = int_vector(b.Cdx, g, 2)
    inv = torch.pow(2.0, torch.randint(-2, 2, (b.Cdx,), generator=g).double()).float()
    scale = pow2_signed(b.Cdx, g)
    shift = torch.randint(-1, 2, (b.Cdx,), generator=g).float()
    n = dx.shape[-1]
    yd = y[..., :n].double()
    gg = dx * ((yd * scale[:n].double() + shift[:n].double()) > 0)
    t2 = gg * (yd - mean[:n].double()) * inv[:n].double()
    sums = torch.stack([gg.reshape(-1, n).sum(0), t2.reshape(-1, n).sum(0)])
    return dy, w, dx, y, torch.cat([mean, inv, scale, shift]), sums, (gg, t2)


def check_bnred_case(b: BnRed, dx, terms) -> None:
    assert_exact_class(dx)
    assert_f32_sums(terms[0], "sum g")
    assert_f32_sums(terms[1], "sum g * xhat")
    assert (terms[0] != dx).any() and (terms[0] != 0).any()  # the ReLU mask cuts some and keeps some


# ---------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Wgrad:
    name: str
    N: int
    H: int
    W: int
    C1: int
    C2: int
    Cout: int
    splits: int
    variant: int
    packed: bool = False
    accumulate: bool = False
    views: bool = False
    seed: int = 0


def _w(name, shape, splits, variant, **kw):
    return Wgrad(name, *shape, splits, variant, **kw)


WGRAD_CASES = [
    # generic layout (odd sizes, dual source), splits 1 / mid / two-level (> 8)
    _w("generic-dual-v0", (2, 9, 13, 64, 64, 128), 2, 0),
    _w("generic-dual-v4-views", (2, 9, 13, 64, 64, 128), 2, 4, views=True),
    _w("generic-1split", (1, 8, 8, 256, 0, 512), 1, 0),
    _w("generic-150-v0", (4, 20, 20, 64, 0, 64), 150, 0),
    _w("generic-150-v4-acc", (4, 20, 20, 64, 0, 64), 150, 4, accumulate=True),
    _w("generic-512-v4", (2, 64, 64, 64, 0, 64), 512, 4),
    # W % 64 == 0: row ring (auto, 64 couts), halo kernel (forced, or 128 couts)
    _w("w64-ring-v0", (2, 5, 64, 64, 0, 64), 3, 0),
    _w("w64-halo-v5-acc", (2, 5, 64, 64, 0, 64), 3, 5, accumulate=True),
    _w("w64-generic-v4", (2, 5, 64, 64, 0, 64), 3, 4),
    _w("w128-dual-v0-views", (1, 6, 128, 64, 64, 128), 4, 0, views=True),
    _w("w64-ring-512", (2, 64, 64, 64, 0, 64), 512, 0),
    _w("w192-v5", (1, 4, 192, 64, 128, 256), 2, 5),
    # W | 64: multi-row segments
    _w("w32-v0", (2, 6, 32, 64, 0, 64), 3, 0),
    _w("w32-v5-views", (2, 6, 32, 64, 0, 64), 3, 5, views=True),
    _w("w16-dual-v5", (1, 8, 16, 128, 128, 128), 2, 5),
    _w("w8-v5", (3, 8, 8, 64, 0, 128), 5, 5),
    _w("w8-v0", (3, 8, 8, 64, 0, 128), 5, 0),
    # packed first layer
    _w("packed-5", (2, 18, 14, 8, 0, 64), 5, 0, packed=True),
    _w("packed-300-acc-views", (2, 64, 64, 8, 0, 64), 300, 0, packed=True, accumulate=True, views=True),
]


@functools.lru_cache(maxsize=4)
def _wgrad_data(N, H, W, cin, Cout, seed):
    g = generator(5000 + seed)
    x = ternary((N, H, W, cin), 0.5, g)
    dy = ternary((N, H, W, Cout), 0.5, g)
    w0 = torch.zeros(Cout, cin, 3, 3, dtype=BF16)
    _, dw = conv_grads_ref(x, w0, dy, False, True)
    return x, dy, dw.permute(0, 2, 3, 1).reshape(-1).contiguous()


def wgrad_data(c: Wgrad):
    """(x [N,H,W,Cin] bf16 (3 real channels when packed), dy bf16, dw fp64 flat [Cout][9][Cin])."""
    return _wgrad_data(c.N, c.H, c.W, 3 if c.packed else c.C1 + c.C2, c.Cout, c.seed)


def wgrad_init(n: int, seed: int) -> torch.Tensor:
    """The non-zero integer `out` that accumulate = 1 adds onto."""
    return torch.randint(-50, 51, (n,), generator=generator(6000 + seed)).float()


def check_wgrad_ref(dw64: torch.Tensor, M: int) -> None:
    """Ternary operands: every partial sum of a weight-gradient element is an integer of magnitude <= M."""
    assert torch.equal(dw64, dw64.round())
    assert M + 50 < F32_EXACT and dw64.abs().max().item() <= M
    assert (dw64 != 0).float().mean().item() > 0.5


@dataclass(frozen=True)
class FirstBn:
    name: str
    N: int
    H: int
    W: int
    splits: int
    accumulate: bool = False
    views: bool = False
    seed: int = 0


FIRSTBN_CASES = [
    FirstBn("firstbn-5", 2, 16, 12, 5),
    FirstBn("firstbn-1-views", 3, 8, 8, 1, views=True),
    FirstBn("firstbn-300-acc", 2, 64, 64, 300, accumulate=True),
]


def firstbn_data(c: FirstBn):
    """x (3 real channels), da, y ternary; coef = [mean | invstd | scale | shift] (the kernel reads scale and
    shift for the ReLU mask), coef2 = [A | B | Cc] with A = +-2^k, B and Cc small integers. Returns the
    fp64 dz = A * da * [scale * y + shift > 0] + B * y + Cc and the fp64 weight gradient of that dz."""
    g = generator(7000 + c.seed)
    shape = (c.N, c.H, c.W)
    x = ternary(shape + (3,), 0.8, g)
    da = ternary(shape + (64,), 0.7, g)
    y = ternary(shape + (64,), 0.7, g)
    scale = pow2_signed(64, g)
    shift = torch.randint(-1, 2, (64,), generator=g).float()
    A = pow2_signed(64, g, -1, 2)
    B = int_vector(64, g, 2)
    Cc = int_vector(64, g, 2)
    yd = y.double()
    dz = A.double() * (da.double() * ((yd * scale.double() + shift.double()) > 0)) + B.double() * yd + Cc.double()
    _, dw = conv_grads_ref(x, torch.zeros(64, 3, 3, 3), dz, False, True)
    coef = torch.cat([torch.zeros(64), torch.ones(64), scale, shift])
    coef2 = torch.cat([A, B, Cc])
    return x, da, y, coef, coef2, dz, dw.permute(0, 2, 3, 1).reshape(-1).contiguous()


def check_firstbn_case(dz64: torch.Tensor, dw64: torch.Tensor) -> None:
    """|dz| <= 256 in units of 1/2 with <= 8 significant bits: dz is exact in bf16; the weight-gradient
    sums are multiples of 1/2 far below 2^24."""
    assert dz64.abs().max().item() <= 9 and torch.equal(dz64 * 2, (dz64 * 2).round())
    assert torch.equal(dz64, dz64.to(BF16).double())
    assert_f32_sums(dz64, "dz")
    assert (dw64 != 0).any()


# ---------------------------------------------------------------------------------------------
# transposed decoder: ConvTranspose2d(k = 2, s = 2)
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class UpT:
    name: str
    N: int
    h: int
    w: int
    Cin: int
    C: int       # output channels of the transposed conv
    H2: int
    W2: int
    oy: int
    ox: int
    seed: int = 0


# conv_upT_fwd / conv_upT_dgrad decline below 256 ping-pong tiles, so these are the smallest shapes they run
UPT_FWD_CASES = [
    UpT("upT-fwd-pp128-odd-pad", 1, 61, 67, 128, 512, 125, 136, 1, 1),   # M = 4087: 16 x 16 tiles, ragged
    UpT("upT-fwd-pp256", 2, 128, 128, 64, 128, 256, 256, 0, 0),
]
UPT_DGRAD_CASES = [
    UpT("upT-dgrad-pp128-odd-pad", 1, 149, 147, 384, 64, 301, 297, 2, 1),  # M = 21903: 86 x 3 tiles, ragged
    UpT("upT-dgrad-pp256", 8, 64, 64, 512, 64, 128, 128, 0, 0),
]
UPT_SMALL_CASES = [   # the generic weight gradient, the taps = 1 GEMMs and the bias column sums
    UpT("upT-small", 2, 8, 8, 128, 64, 16, 16, 0, 0),
    UpT("upT-small-odd-pad", 1, 4, 5, 256, 128, 9, 11, 1, 0),
    UpT("upT-small-odd-pad2", 2, 5, 7, 128, 64, 13, 17, 1, 2),
]


@functools.lru_cache(maxsize=2)
def _upT_data(N, h, w, Cin, C, H2, W2, oy, ox, seed, want, cin_limit):
    g = generator(8000 + seed)
    p, q = densities(Cin)
    x = ternary((N, h, w, Cin), p, g)
    Wt = ternary((Cin, C, 2, 2), q, g)
    bias = int_vector(C, g, 4)
    if cin_limit is not None:  # dx of the first input channels alone (u is then not the case's)
        x, Wt = x[..., :cin_limit].contiguous(), Wt[:cin_limit].contiguous()
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(want != "fwd")
    Wr = Wt.double().requires_grad_(want == "bwd")
    br = bias.double().requires_grad_(want == "bwd")
    y = F.conv_transpose2d(xr, Wr, br, stride=2)
    u = F.pad(y, [ox, W2 - 2 * w - ox, oy, H2 - 2 * h - oy])
    out = {"x": x, "W": Wt, "bias": bias, "u": u.detach().permute(0, 2, 3, 1).contiguous()}
    if want != "fwd":
        pd, _ = densities(4 * C)
        du = ternary((N, H2, W2, C), pd, g)
        u.backward(du.double().permute(0, 3, 1, 2))
        out.update(du=du, dx=xr.grad.permute(0, 2, 3, 1).contiguous())
        if want == "bwd":
            out.update(dW=Wr.grad, db=br.grad)
    return out


def upT_data(c: UpT, want: str = "fwd", cin_limit: Optional[int] = None):
    """x [N,h,w,Cin], W [Cin,C,2,2], integer bias; u = pad(conv_transpose2d(x, W, bias)) [N,H2,W2,C] fp64
    (zero outside the window at (oy, ox)); with want = "dx" also du (ternary, whole padded map) and the
    fp64 autograd dx [N,h,w,Cin]; with "bwd" dW [Cin,C,2,2] and db [C] too."""
    return _upT_data(c.N, c.h, c.w, c.Cin, c.C, c.H2, c.W2, c.oy, c.ox, c.seed, want, cin_limit)


def upT_weights(Wt: torch.Tensor):
    """(forward [4C][Cin], dgrad [Cin][4C]) GEMM weights, columns ordered (dh, dw, c)."""
    wd = Wt.permute(0, 2, 3, 1).reshape(Wt.shape[0], -1).contiguous()
    return wd.t().contiguous(), wd


def upT_window(c: UpT, t: torch.Tensor) -> torch.Tensor:
    """[N,H2,W2,C] -> the sub-pixel GEMM layout [N,h,w,(dh,dw,c)] of the 2h x 2w window at (oy, ox)."""
    win = t[:, c.oy:c.oy + 2 * c.h, c.ox:c.ox + 2 * c.w]
    return win.reshape(c.N, c.h, 2, c.w, 2, c.C).permute(0, 1, 3, 2, 4, 5).reshape(c.N, c.h, c.w, 4 * c.C).contiguous()


# =============================================================================================
# The memory-bound passes between the convs: BN finalize / apply / backward, max pool, bilinear
# upsample (tests/test_pass_exact_gpu.py; preconditions in tests/test_pass_lattice_cpu.py)
# =============================================================================================
#
# The elementwise passes evaluate fma(y, scale, shift) (and the backward's A * g + B * y + Cc) in fp32
# and round once to bf16. With small-integer y, scale = +-2^k and integer shift every such value is a
# small dyadic number: exact in fp32 whether or not the compiler fuses the multiply-add, and exactly
# representable in bf16, so the stored value is fixed bit for bit. Because these passes are elementwise,
# a case's preconditions depend only on the set of input values and its coefficients: the *_table
# functions evaluate the reference for every possible input value of every channel.

APX = 4                      # pixels in flight per thread in the BN apply kernels
PX_GRID_CAP = 2048           # their grid cap
FIN_DIRECT_ROWS = 2048       # rows the finalize kernels fold themselves; above, colsum_kernel (needs a workspace)
POOL_GRID_CAP = 4096         # maxpool2_fwd / bwd: blocks of 256 items, grid-stride beyond
APPLY_POOL_GRID_CAP = 16384  # bn_relu_apply_pool
UP_MIN_ITEMS = 4096          # the upsample launchers halve the band height below this many work items


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def px_grid(M: int, C: int):
    """(grid, chunk, rows per block) of the pixel-walking BN apply launchers (grid_px / px_chunk)."""
    rpb = 256 // (C // 8)
    step = rpb * APX
    grid = max(1, min(cdiv(M, step), PX_GRID_CAP))
    chunk = cdiv(cdiv(M, grid), step) * step
    return grid, chunk, rpb


def up_band_rows(N: int, rows: int, cols: int, C: int, start: int) -> int:
    """Band height of the upsample launchers: `start` (8 forward over output rows / columns, 4 backward
    over input-gradient rows / columns), halved while fewer than 4096 work items would be in flight."""
    nchunk = cdiv(cols * (C // 8), 256)
    R = start
    while R > 1 and N * cdiv(rows, R) * nchunk < UP_MIN_ITEMS:
        R //= 2
    return R


def bf16_exact(ref64: torch.Tensor) -> bool:
    return torch.equal(ref64, ref64.to(BF16).double())


def f32_exact(ref64: torch.Tensor) -> bool:
    return torch.equal(ref64, ref64.float().double())


def _odd_signed(n: int, gen: torch.Generator, lo: int, hi: int) -> torch.Tensor:
    """fp32 vector of odd integers with lo <= |v| <= hi, both signs present."""
    v = torch.randint(lo // 2, (hi - 1) // 2 + 1, (n,), generator=gen) * 2 + 1
    s = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    s[0], s[1] = 1, -1
    return (s * v).float()


# ---------------------------------------------------------------------------------------------
# bn_relu_apply / bn_relu_bwd_apply
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Px:
    """One launch of a pixel-walking BN pass over M = N * H * W pixels of C channels."""
    name: str
    N: int
    H: int
    W: int
    C: int
    relu: int = 1
    cls: str = "exact"     # "exact" | "round"
    views: bool = False
    capped: bool = False   # M > 2048 * (2048 / C) * 4: the grid reaches its cap
    seed: int = 0

    @property
    def M(self) -> int:
        return self.N * self.H * self.W


PX_CASES = [
    Px("c64-one-block-views", 1, 7, 5, 64, views=True),
    Px("c8-ragged", 2, 37, 29, 8),
    Px("c512-ragged-norelu-views", 2, 37, 29, 512, relu=0, views=True),
    Px("c2048-ragged", 1, 9, 11, 2048),
    Px("c64-round", 2, 37, 29, 64, relu=0, cls="round"),
    Px("c2048-round-views", 1, 9, 11, 2048, cls="round", views=True),
    Px("c8-capped", 2, 1025, 1031, 8, capped=True),
    Px("c64-capped", 3, 301, 293, 64, relu=0, capped=True),
    Px("c512-capped", 1, 181, 183, 512, capped=True),
    Px("c2048-capped-views", 1, 91, 93, 2048, capped=True, views=True),
]


def check_px_shape(c: Px) -> None:
    """The last working block's chunk is ragged: its last step of rpb * APX pixels is partial, and (where a
    block holds more than one pixel row) so is the last row group; capped cases reach 2048 blocks."""
    grid, chunk, rpb = px_grid(c.M, c.C)
    tail = c.M % chunk
    assert tail % (rpb * APX) != 0 and (rpb == 1 or tail % rpb != 0), f"{c.name}: the last chunk is not ragged"
    if c.capped:
        assert c.M > PX_GRID_CAP * (2048 // c.C) * APX and grid == PX_GRID_CAP
        assert chunk > rpb * APX  # more than one step per block
    else:
        assert grid < PX_GRID_CAP


def apply_coef(c: Px) -> torch.Tensor:
    """[mean | invstd | scale | shift]. exact: +-2^k (k = -2..1), integer shift. round: +-2^k (k = 1..5) and
    odd shifts of magnitude 361..409, so y in -3..3 gives odd integers within 265..505: every one a tie."""
    g = generator(11000 + c.seed + c.C)
    if c.cls == "exact":
        scale, shift = pow2_signed(c.C, g), int_vector(c.C, g, 8)
    else:
        scale, shift = pow2_signed(c.C, g, 1, 5), _odd_signed(c.C, g, 361, 409)
    return torch.cat([torch.zeros(c.C), torch.ones(c.C), scale, shift])


def apply_ref(y: torch.Tensor, coef: torch.Tensor, relu: int) -> torch.Tensor:
    """fp64 relu(y * scale + shift), on the device y lives on."""
    C = y.shape[-1]
    z = y.double() * coef[2 * C:3 * C].double().to(y.device) + coef[3 * C:4 * C].double().to(y.device)
    return torch.relu(z) if relu else z


def apply_data(c: Px):
    y = small_ints((c.N, c.H, c.W, c.C), generator(12000 + c.seed + c.C), 3)
    coef = apply_coef(c)
    return y, coef, apply_ref(y, coef, c.relu)


def apply_table(c: Px) -> torch.Tensor:
    """The reference for every input value -3..3 of every channel: [7, C] fp64."""
    v = torch.arange(-3, 4).to(BF16).view(7, 1).expand(7, c.C)
    return apply_ref(v, apply_coef(c), c.relu)


def check_apply_table(c: Px, tab: torch.Tensor) -> None:
    if c.cls == "exact":
        assert bf16_exact(tab) and (tab.abs() * 4 < 256).all() and torch.equal(tab * 4, (tab * 4).round())
        if c.relu:
            assert (tab == 0).any() and (tab > 0).any()
        else:
            assert (tab < 0).any() and (tab > 0).any()
    else:
        pre = apply_ref(torch.arange(-3, 4).to(BF16).view(7, 1).expand(7, c.C), apply_coef(c), 0)
        assert true_ties(pre) == pre.numel(), "round class: every pre-ReLU value must be a true tie"
        assert_rounding_class(tab)


def bwd_apply_coefs(c: Px):
    """coef as the kernel reads it for the ReLU mask (scale = +-2^k, shift -1..1) and coef2 = [A | B | Cc].
    exact: A = +-2^k (k = -1..2), B and Cc in -2..2 (firstbn_data's form). round: A = +-2^k (k = 1..4), B even,
    Cc odd of magnitude 331..439: dy is an odd integer within 281..489."""
    g = generator(13000 + c.seed + c.C)
    scale = pow2_signed(c.C, g)
    shift = torch.randint(-1, 2, (c.C,), generator=g).float()
    if c.cls == "exact":
        A, B, Cc = pow2_signed(c.C, g, -1, 2), int_vector(c.C, g, 2), int_vector(c.C, g, 2)
    else:
        A = pow2_signed(c.C, g, 1, 4)
        B = (torch.randint(-1, 2, (c.C,), generator=g) * 2).float()
        Cc = _odd_signed(c.C, g, 331, 439)
    return torch.cat([torch.zeros(c.C), torch.ones(c.C), scale, shift]), torch.cat([A, B, Cc])


def bwd_apply_ref(da, y, coef, coef2, relu: int) -> torch.Tensor:
    """fp64 dy = A * g + B * y + Cc, g = da * [scale * y + shift > 0] (g = da without ReLU)."""
    C = y.shape[-1]
    k = [coef[2 * C:3 * C], coef[3 * C:4 * C], coef2[:C], coef2[C:2 * C], coef2[2 * C:3 * C]]
    sc, sh, A, B, Cc = (t.double().to(y.device) for t in k)
    yd, g = y.double(), da.double()
    if relu:
        g = g * ((yd * sc + sh) > 0)
    return A * g + B * yd + Cc


def bwd_apply_data(c: Px):
    g = generator(14000 + c.seed + c.C)
    shape = (c.N, c.H, c.W, c.C)
    da, y = small_ints(shape, g, 3), ternary(shape, 0.7, g)
    coef, coef2 = bwd_apply_coefs(c)
    return da, y, coef, coef2, bwd_apply_ref(da, y, coef, coef2, c.relu)


def bwd_apply_table(c: Px) -> torch.Tensor:
    """[7 (da = -3..3), 3 (y = -1..1), C] fp64."""
    da = torch.arange(-3, 4).to(BF16).view(7, 1, 1).expand(7, 3, c.C)
    y = torch.arange(-1, 2).to(BF16).view(1, 3, 1).expand(7, 3, c.C)
    coef, coef2 = bwd_apply_coefs(c)
    return bwd_apply_ref(da, y, coef, coef2, c.relu)


def check_bwd_apply_table(c: Px, tab: torch.Tensor) -> None:
    if c.cls == "exact":
        assert bf16_exact(tab) and (tab.abs() * 2 < 256).all() and torch.equal(tab * 2, (tab * 2).round())
        if c.relu:  # the mask cuts some and keeps some
            assert (tab[6] != tab[0]).any() and (tab[6] == tab[0]).any()
    else:
        assert true_ties(tab) == tab.numel()
        assert_rounding_class(tab)


# ---------------------------------------------------------------------------------------------
# the BN backward reductions: bn_relu_bwd_reduce, maxpool2_bwd_bn_reduce, upsample2_bwd + reduce
# ---------------------------------------------------------------------------------------------

def bn_lattice_coef(C: int, gen: torch.Generator, shift_amax: int = 1) -> torch.Tensor:
    """[mean | invstd | scale | shift] as bnred_data builds it: integer mean, invstd = 2^k, scale = +-2^k,
    integer shift -- every term of sum(g) and sum(g * xhat) is then dyadic."""
    mean = int_vector(C, gen, 2)
    inv = torch.pow(2.0, torch.randint(-2, 2, (C,), generator=gen).double()).float()
    return torch.cat([mean, inv, pow2_signed(C, gen), int_vector(C, gen, shift_amax)])


def reduce_terms(g64: torch.Tensor, y: torch.Tensor, coef: torch.Tensor, relu: int = 1):
    """(g * mask, g * mask * (y - mean) * invstd) in fp64 and their per-channel sums [2][C]."""
    C = y.shape[-1]
    mean, inv, sc, sh = (coef[k * C:(k + 1) * C].double().to(y.device) for k in range(4))
    yd = y.double()
    gg = g64 * ((yd * sc + sh) > 0) if relu else g64
    t2 = gg * (yd - mean) * inv
    return (gg, t2), torch.stack([gg.reshape(-1, C).sum(0), t2.reshape(-1, C).sum(0)])


@dataclass(frozen=True)
class Red:
    name: str
    N: int
    H: int
    W: int
    C: int
    relu: int = 1
    views: bool = False
    cap: int = 1024     # partial rows offered to the kernel
    seed: int = 0


RED_CASES = [
    Red("red-c64-odd", 2, 37, 29, 64),
    Red("red-c8", 3, 33, 47, 8),
    Red("red-c512-views", 2, 9, 13, 512, views=True),
    Red("red-c2048", 1, 9, 11, 2048),
    Red("red-c96-not-pow2", 2, 9, 13, 96),
    Red("red-c64-cap3-wraps", 2, 37, 29, 64, cap=3),
    Red("red-c128-norelu-views", 1, 21, 17, 128, relu=0, views=True),
]


def red_data(c: Red):
    g = generator(15000 + c.seed + c.C)
    shape = (c.N, c.H, c.W, c.C)
    da, y = small_ints(shape, g, 3), ternary(shape, 0.7, g)
    coef = bn_lattice_coef(c.C, g)
    terms, sums = reduce_terms(da.double(), y, coef, c.relu)
    return da, y, coef, terms, sums


def check_red_terms(terms, sums, masked: bool = True) -> None:
    assert_f32_sums(terms[0], "sum g")
    assert_f32_sums(terms[1], "sum g * xhat")
    assert f32_exact(sums) and (sums[0] != 0).any() and (sums[1] != 0).any()
    if masked:
        assert (terms[0] == 0).any() and (terms[0] != 0).any()


# ---------------------------------------------------------------------------------------------
# max pool and its BN fusions
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Pool:
    name: str
    N: int
    H: int
    W: int
    C: int
    dskip: bool = True
    views: bool = False
    cap: int = 1024      # fused backward: partial rows offered
    big: bool = False    # a path-forcing size: its reference is evaluated by torch fp64 on the device
    seed: int = 0


POOL_CASES = [
    Pool("pool-c64-even", 2, 16, 16, 64),
    Pool("pool-c8-odd-both-views", 1, 9, 7, 8, views=True),
    Pool("pool-c512-odd-h-noskip-views", 2, 9, 8, 512, dskip=False, views=True),
    Pool("pool-c64-odd-w-noskip", 2, 8, 9, 64, dskip=False),
    Pool("pool-c8-grid-wraps", 4, 1027, 1027, 8, big=True),
]

POOLFUSE_CASES = [
    Pool("fuse-c64-even", 2, 16, 16, 64),
    Pool("fuse-c8-odd-both-views", 1, 9, 13, 8, views=True),
    Pool("fuse-c512-odd-w-noskip-views", 3, 8, 7, 512, dskip=False, views=True),
    Pool("fuse-c64-odd-h-cap2-wraps", 4, 33, 24, 64, cap=2),
    Pool("fuse-c128-odd-both", 1, 33, 31, 128),
]
APPLY_POOL_BIG = Pool("fuse-c512-grid-capped", 2, 363, 363, 512, big=True)


def pool_items(c: Pool):
    """(forward, backward) work items of maxpool2_fwd / maxpool2_bwd: one per (window, 8-channel group)."""
    cg = c.C // 8
    return c.N * (c.H // 2) * (c.W // 2) * cg, c.N * cdiv(c.H, 2) * cdiv(c.W, 2) * cg


def apply_pool_blocks(c: Pool) -> int:
    """Blocks bn_relu_apply_pool would need for one window row each (before the 16384 cap)."""
    return cdiv(c.N * cdiv(c.H, 2) * cdiv(c.W, 2), 256 // (c.C // 8))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pool_ref(a64: torch.Tensor, dp: Optional[torch.Tensor], dskip: Optional[torch.Tensor]):
    """fp64 F.max_pool2d(2) of an NHWC tensor and, with dp, its autograd input gradient (+ dskip): torch
    routes each window's gradient to its first maximum in row-major order."""
    x = _nchw(a64).contiguous().requires_grad_(dp is not None)
    p = F.max_pool2d(x, 2)
    if dp is None:
        return _nhwc(p), None
    p.backward(_nchw(dp.double()).contiguous())
    dx = _nhwc(x.grad)
    if dskip is not None:
        dx = dx + dskip.double()
    return _nhwc(p.detach()), dx


def tie_fraction(a64: torch.Tensor) -> float:
    """Fraction of 2x2 windows whose maximum is attained more than once."""
    H, W = a64.shape[1] // 2 * 2, a64.shape[2] // 2 * 2
    w = torch.stack([a64[:, i:H:2, j:W:2] for i in (0, 1) for j in (0, 1)])
    return ((w == w.max(0).values).sum(0) > 1).double().mean().item()


def pool_data(c: Pool, device="cpu"):
    """Ternary x (most windows tie), small-integer dp / dskip. big cases draw on `device`."""
    if c.big:
        g = torch.Generator(device=device)
        g.manual_seed(16000 + c.seed)
        def draw(shape, amax):
            return torch.randint(-amax, amax + 1, shape, generator=g, device=device).to(BF16)
    else:
        g = generator(16000 + c.seed + c.C)
        def draw(shape, amax):
            return torch.randint(-amax, amax + 1, shape, generator=g).to(BF16)
    x = draw((c.N, c.H, c.W, c.C), 1)
    dp = draw((c.N, c.H // 2, c.W // 2, c.C), 3)
    ds = draw((c.N, c.H, c.W, c.C), 3) if c.dskip else None
    return x, dp, ds


def poolfuse_coef(c: Pool) -> torch.Tensor:
    return bn_lattice_coef(c.C, generator(17000 + c.seed + c.C), shift_amax=2)


def poolfuse_data(c: Pool, device="cpu"):
    """y in -3..3 under +-2^k scales and integer shifts: a = relu(bn(y)) is exact in bf16 and its many zeros
    tie. Returns y, dp, dskip, coef and the fp64 a."""
    if c.big:
        g = torch.Generator(device=device)
        g.manual_seed(17000 + c.seed)
        y = torch.randint(-3, 4, (c.N, c.H, c.W, c.C), generator=g, device=device).to(BF16)
        dp = ds = None
    else:
        g = generator(18000 + c.seed + c.C)
        y = small_ints((c.N, c.H, c.W, c.C), g, 3)
        dp = small_ints((c.N, c.H // 2, c.W // 2, c.C), g, 3)
        ds = small_ints((c.N, c.H, c.W, c.C), g, 3) if c.dskip else None
    coef = poolfuse_coef(c)
    return y, dp, ds, coef, apply_ref(y, coef, 1)


def poolfuse_table(c: Pool) -> torch.Tensor:
    v = torch.arange(-3, 4).to(BF16).view(7, 1).expand(7, c.C)
    return apply_ref(v, poolfuse_coef(c), 1)


# ---------------------------------------------------------------------------------------------
# bn_finalize / bn_bwd_finalize on synthetic partial rows
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Fin:
    name: str
    T: int
    C: int
    ws: bool = False   # pass the colsum workspace (used when T > 2048)
    seed: int = 0


FIN_COUNT = 1 << 14
FIN_CASES = [Fin(f"T{T}-C{C}", T, C) for T in (1, 16, 17, 63, 64, 65, 2048) for C in (64, 96, 512)] + \
            [Fin(f"T{T}-C{C}-{'colsum' if ws else 'direct'}", T, C, ws)
             for T in (2049, 5000) for C in (64, 96, 512) for ws in (True, False)]


def split_rows(total: torch.Tensor, T: int, gen: torch.Generator, amp: int = 3) -> torch.Tensor:
    """Integer rows [T][K] that sum to total [K] exactly: an even split plus zero-sum integer noise."""
    total = total.long()
    base = total // T
    rem = total - base * T
    rows = base[None, :] + (torch.arange(T)[:, None] < rem[None, :]).long()
    n = torch.randint(-amp, amp + 1, (T, total.numel()), generator=gen)
    return rows + n - n.roll(1, 0)


def _dyadic(n: int, gen: torch.Generator, amax: int, denom: int, nonzero: bool = False) -> torch.Tensor:
    v = torch.randint(-amax, amax + 1, (n,), generator=gen)
    if nonzero:
        v[v == 0] = amax
    return (v.double() / denom).float()


def fin_data(c: Fin):
    """Synthetic (sum, sum of squares) rows of a layer whose channel has integer mean mu and sigma = 2^j over
    count = 2^14 pixels; eps = 0, momentum = 1/2, dyadic gamma / beta / running stats. Every output is then
    one fixed fp32 value (running_var, through count / (count - 1), within one ulp). Returns the inputs and
    the expected outputs in fp64."""
    g = generator(19000 + c.seed + 7 * c.T + c.C)
    mu = torch.randint(-3, 4, (c.C,), generator=g).double()
    j = torch.randint(0, 3, (c.C,), generator=g).double()
    var = torch.pow(4.0, j)
    S, Q = FIN_COUNT * mu, FIN_COUNT * (var + mu * mu)
    rows = torch.cat([split_rows(S, c.T, g), split_rows(Q, c.T, g)], 1).float()   # [T][2C]
    gamma, beta = _dyadic(c.C, g, 6, 2, nonzero=True), _dyadic(c.C, g, 8, 4)
    rmean, rvar = _dyadic(c.C, g, 8, 4), (torch.randint(1, 9, (c.C,), generator=g).double() / 4).float()
    inv = torch.pow(2.0, -j)
    sc = gamma.double() * inv
    exp = {"mean": mu, "invstd": inv, "scale": sc, "shift": beta.double() - mu * sc,
           "rmean": 0.5 * rmean.double() + 0.5 * mu,
           "rvar": 0.5 * rvar.double() + 0.5 * (var * FIN_COUNT / (FIN_COUNT - 1))}
    return rows, gamma, beta, rmean, rvar, exp


def bwd_fin_data(c: Fin):
    """Integer partial rows of (sum g, sum g * xhat), dyadic gamma / invstd, integer mean. dbeta and dgamma
    are the integer totals; coef2 = [A | B | Cc] is formed in fp64 from dyadic factors with fewer than 24
    significant bits, so its fp32 value is fixed too."""
    g = generator(20000 + c.seed + 7 * c.T + c.C)
    S = torch.randint(-4000, 4001, (c.C,), generator=g).double()
    Q = torch.randint(-4000, 4001, (c.C,), generator=g).double()
    rows = torch.cat([split_rows(S, c.T, g), split_rows(Q, c.T, g)], 1).float()
    gamma = _dyadic(c.C, g, 6, 2, nonzero=True)
    mean = int_vector(c.C, g, 3)
    inv = torch.pow(2.0, -torch.randint(0, 3, (c.C,), generator=g).double()).float()
    coef = torch.cat([mean, inv, gamma * inv, torch.zeros(c.C)])
    A = gamma.double() * inv.double()
    mg, mgx = S / FIN_COUNT, Q / FIN_COUNT
    exp = {"dbeta": S, "dgamma": Q,
           "coef2": torch.cat([A, -A * inv.double() * mgx, -A * mg + A * inv.double() * mgx * mean.double()])}
    return rows, gamma, coef, exp


def check_fin_rows(c: Fin, rows: torch.Tensor) -> None:
    """Integer rows whose every partial sum is exact in fp32 (the colsum pre-reduction adds them in fp32)."""
    assert rows.shape == (c.T, 2 * c.C) and rows.dtype == torch.float32
    assert_f32_sums(rows.double(), "partial rows")
    assert torch.equal(rows, rows.round())


# ---------------------------------------------------------------------------------------------
# bilinear x2 upsample (align_corners) + centred pad: per-element class
# ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Up:
    """x [N,hin,win,C] -> out [N,Hout,Wout,C] with the 2x map at (oy, ox); R: the band height the launcher
    must pick for this shape (forward: over Hout / Wout from 8; backward: over hin / win from 4)."""
    name: str
    N: int
    hin: int
    win: int
    C: int
    Hout: int
    Wout: int
    oy: int
    ox: int
    R: int
    views: bool = False
    coef: bool = False    # forward: also the fused producer BN + ReLU form
    bnred: bool = False   # backward: also the fused BN reduction form (UP_BNRED_CASES: its sums are exact)
    seed: int = 0


UP_FWD_CASES = [
    Up("fwd-R1-one-pixel", 2, 1, 1, 64, 3, 5, 1, 1, 1, views=True, coef=True),
    Up("fwd-R1-hin1", 1, 1, 6, 128, 2, 13, 0, 1, 1),
    Up("fwd-R1-win1", 3, 5, 1, 512, 11, 3, 1, 1, 1, coef=True),
    Up("fwd-R1-odd-pad-views", 2, 5, 7, 64, 11, 15, 1, 1, 1, views=True, coef=True),
    Up("fwd-R1-two-chunks", 1, 9, 19, 128, 20, 39, 1, 1, 1),
    Up("fwd-R2-c512", 8, 30, 30, 512, 63, 63, 3, 1, 2, coef=True),
    Up("fwd-R2-c64", 14, 61, 64, 64, 125, 130, 1, 1, 2),
    Up("fwd-R4-c512", 16, 30, 30, 512, 63, 63, 1, 3, 4),
    Up("fwd-R4-c128", 16, 61, 64, 128, 125, 130, 3, 1, 4, coef=True),
    Up("fwd-R8-c512", 32, 30, 30, 512, 63, 63, 1, 1, 8),
    Up("fwd-R8-c64", 52, 61, 64, 64, 125, 130, 1, 1, 8, coef=True),
    Up("fwd-R4-c128-views", 16, 61, 64, 128, 125, 130, 1, 1, 4, views=True),
]

UP_BWD_CASES = [
    Up("bwd-R1-one-pixel", 2, 1, 1, 64, 3, 5, 1, 1, 1, views=True, bnred=True),
    Up("bwd-R1-hin1", 1, 1, 6, 128, 2, 13, 0, 1, 1, bnred=True),
    Up("bwd-R1-win1", 3, 5, 1, 512, 11, 3, 1, 1, 1),
    Up("bwd-R1-odd-pad-views", 2, 5, 7, 64, 11, 15, 1, 1, 1, views=True, bnred=True),
    Up("bwd-R1-two-chunks", 1, 9, 37, 64, 20, 75, 1, 1, 1),
    Up("bwd-R2-c512", 32, 31, 30, 512, 63, 61, 1, 1, 2),
    Up("bwd-R2-c64", 45, 61, 65, 64, 125, 133, 3, 1, 2),
    Up("bwd-R4-c512", 64, 30, 30, 512, 63, 63, 1, 3, 4),
    Up("bwd-R4-c128", 52, 61, 65, 128, 125, 133, 1, 1, 4),
    Up("bwd-R2-c128-views", 27, 61, 65, 128, 123, 131, 1, 1, 2, views=True),
]

# The fused BN reduction is exact only while M = N * hin * win is small (below): the banded heights are
# reached at C = 2048, where a chunk of 256 lanes is one pixel.
UP_BNRED_CASES = [
    Up("bnred-R1-c512", 2, 9, 7, 512, 19, 15, 1, 1, 1, bnred=True),
    Up("bnred-R2-c2048", 1, 91, 91, 2048, 183, 183, 1, 1, 2, bnred=True),
    Up("bnred-R4-c2048", 2, 91, 91, 2048, 183, 183, 1, 1, 4, bnred=True),
]


def check_up_shape(c: Up, fwd: bool) -> None:
    assert 2 * c.hin + c.oy <= c.Hout and 2 * c.win + c.ox <= c.Wout
    assert (c.oy, c.ox) != (0, 0)
    rows, cols, start = (c.Hout, c.Wout, 8) if fwd else (c.hin, c.win, 4)
    assert up_band_rows(c.N, rows, cols, c.C, start) == c.R, f"{c.name}: the launcher would not pick R = {c.R}"
    if c.R > 1:
        assert rows % c.R != 0, f"{c.name}: the last band is not ragged"
        if c.C < 2048:  # at C = 2048 a chunk is exactly one pixel
            assert (cols * (c.C // 8)) % 256 != 0, f"{c.name}: the last 256-lane chunk is not ragged"


def up_bnred_coef(C: int, seed: int = 0) -> torch.Tensor:
    """mean -1..1, invstd 1 or 2, scale +-2^k, shift -1..1: with dout in 4..6 the gradient dx lies in two
    binades, so the terms of the reduction share a coarse quantum (asserted on the dx read back)."""
    g = generator(21000 + seed + C)
    mean = int_vector(C, g, 1)
    inv = torch.pow(2.0, torch.randint(0, 2, (C,), generator=g).double()).float()
    return torch.cat([mean, inv, pow2_signed(C, g), int_vector(C, g, 1)])


def up_ref(x64: torch.Tensor, c: Up) -> torch.Tensor:
    """fp64 F.interpolate(scale 2, bilinear, align_corners) + the pad that puts it at (oy, ox); NHWC."""
    up = F.interpolate(_nchw(x64), scale_factor=2, mode="bilinear", align_corners=True)
    return F.pad(up, [c.ox, c.Wout - 2 * c.win - c.ox, c.oy, c.Hout - 2 * c.hin - c.oy]).permute(0, 2, 3, 1)


def ulp_bf16(ref64: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |ref| (8 significant bits); 0 at 0."""
    _, e = torch.frexp(ref64)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), torch.ldexp(torch.ones_like(ref64), e - 8))


def up_bwd_ref(dout64: torch.Tensor, c: Up) -> torch.Tensor:
    """fp64 autograd gradient of up_ref with respect to its input, NHWC [N,hin,win,C']."""
    x = torch.zeros(c.N, c.hin, c.win, dout64.shape[-1], dtype=torch.float64, device=dout64.device).requires_grad_(True)
    up_ref(x, c).backward(dout64)
    return x.grad


UP_TILE = 128  # the fused-reduction cases draw this many channels and repeat them: the kernel treats channels alike


def up_bnred_inputs(c: Up):
    """dout in 4..6 over the whole padded map (dx then lies within [8, 32)), ternary y, up_bnred_coef."""
    g = generator(22000 + c.seed + c.C)
    cb = min(c.C, UP_TILE)
    dout = torch.randint(4, 7, (c.N, c.Hout, c.Wout, cb), generator=g).to(BF16)
    y = ternary((c.N, c.hin, c.win, cb), 0.7, g)
    rep = c.C // cb
    return dout.repeat(1, 1, 1, rep), y.repeat(1, 1, 1, rep), up_bnred_coef(c.C, c.seed)


def up_bnred_ref_dx(c: Up, dout: torch.Tensor) -> torch.Tensor:
    """fp64 autograd dx of a fused-reduction case (computed on the drawn channels, then repeated)."""
    cb = min(c.C, UP_TILE)
    return up_bwd_ref(dout[..., :cb].double(), c).repeat(1, 1, 1, c.C // cb)
