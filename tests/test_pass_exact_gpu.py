"""Exact and per-element tests of the memory-bound passes between the convs (GPU only): bn_finalize,
bn_relu_apply, bn_relu_bwd_reduce, bn_bwd_finalize, bn_relu_bwd_apply, maxpool2_fwd / bwd, bn_relu_apply_pool,
maxpool2_bwd_bn_reduce and upsample2_fwd / bwd.

Exact class. On the lattice inputs of tests/lattice.py (small integers, +-2^k scales, integer shifts) every
value these passes form is a small dyadic number, exact in fp32 in any evaluation order and representable
in bf16, so each output is compared bit for bit with an fp64 reference and each reduction, folded in fp64,
with the exact sums. There is no tolerance in that class. The reference is formed on the CPU; the few
path-forcing sizes marked `big` (> 30M elements) are referenced by torch in fp64 on the device instead, which
is independent code. Outputs are prefilled with a sentinel, views sit between guard bands.

Per-element class. The bilinear upsample's weights are not dyadic, and realistic BN coefficients are not
either; there every element must satisfy |got - ref| <= 1/2 ulp_bf16(ref) + slop against an fp64
reference, with `slop` derived next to each test from the fp32 operations the kernel needs -- never from
what the kernel returns. Each such test prints its margin (profiles/pass_exact.md).

tests/test_pass_lattice_cpu.py asserts every case's preconditions, and the band height every upsample case
is meant to reach, without a GPU.
"""
import pytest
import torch
import torch.nn.functional as F

import lattice as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
U32 = 2.0 ** -24   # unit roundoff of fp32: one rounding moves a value v by at most U32 * |v|


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native()


def _ids(c):
    return c.name


class Buf:
    """A device activation: dense, or a channel slice of a wider buffer between sentinel guard bands."""

    def __init__(self, t, shape, views, pads=(8, 24)):
        self.views = views
        if views:
            self.flat, self.t = L.embed(t, shape, pads[0], pads[1], DEV)
            self.before = self.flat.clone()
        elif t is None:
            self.t = torch.full(tuple(shape), L.SENTINEL, dtype=L.BF16, device=DEV)
        else:
            self.t = t.to(DEV).contiguous()
            self.before = self.t.clone()

    def assert_unchanged(self):  # an input: the whole buffer, guards and padding included
        cur = self.flat if self.views else self.t
        assert torch.equal(cur.view(torch.int16), self.before.view(torch.int16))

    def assert_outside_intact(self):  # an output: everything but the view
        if self.views:
            assert L.outside_view_intact(self.flat, self.t)


def _inp(t, views, pads=(16, 8)):
    return None if t is None else Buf(t, t.shape, views, pads)


def _out(shape, views, pads=(8, 24)):
    return Buf(None, shape, views, pads)


def _check_inputs(*bufs):
    for b in bufs:
        if b is not None:
            b.assert_unchanged()


def _same(got, exp64):
    """got (bf16, device) holds exactly the bf16 rounding of the fp64 reference."""
    return torch.equal(got, L.expected_bf16(exp64).to(got.device))


class F32Out:
    """n fp32 outputs between guard bands, all prefilled with the sentinel."""

    def __init__(self, n):
        self.flat = torch.full((2 * L.GUARD + n,), L.SENTINEL, device=DEV)
        self.t = self.flat[L.GUARD:L.GUARD + n]

    def assert_rest_intact(self, written):
        """Everything but the first `written` elements still holds the sentinel."""
        probe = self.flat.clone()
        probe[L.GUARD:L.GUARD + written] = L.SENTINEL
        assert torch.equal(probe, torch.full_like(probe, L.SENTINEL))


def _check_partial(part, T, cap, Ch, sums):
    """1 <= T <= cap rows were written, they fold (fp64) to exactly `sums`, nothing else was touched."""
    assert 1 <= T <= cap
    got = part.t[:T * 2 * Ch].view(T, 2, Ch).double().sum(0)
    sums = sums.to(got.device)
    assert (got[0] == sums[0]).all()
    assert (got[1] == sums[1]).all()
    part.assert_rest_intact(T * 2 * Ch)


# ---------------------------------------------------------------------------------------------
# 1. exact class: BN apply passes
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.PX_CASES, ids=_ids)
def test_bn_relu_apply_exact(C, c):
    """out = [relu](fma(y, scale, shift)), bitwise: ragged last chunks, the 2048-block cap, C = 8 .. 2048,
    pitched views; the rounding cases are all true bf16 ties (odd integers in (256, 512))."""
    L.check_px_shape(c)
    L.check_apply_table(c, L.apply_table(c))
    y, coef, ref = L.apply_data(c)
    by, out = _inp(y, c.views), _out(y.shape, c.views)
    C.bn_relu_apply(by.t, out.t, coef.to(DEV), c.relu)
    torch.cuda.synchronize()
    assert _same(out.t, ref)
    _check_inputs(by)
    out.assert_outside_intact()


@pytest.mark.parametrize("c", L.PX_CASES, ids=_ids)
def test_bn_relu_bwd_apply_exact(C, c):
    """dy = A * g + B * y + Cc, g = da * [scale * y + shift > 0], bitwise; same shape rules."""
    L.check_px_shape(c)
    L.check_bwd_apply_table(c, L.bwd_apply_table(c))
    da, y, coef, coef2, ref = L.bwd_apply_data(c)
    bda, by, out = _inp(da, c.views), _inp(y, c.views, (24, 8)), _out(y.shape, c.views)
    C.bn_relu_bwd_apply(bda.t, by.t, coef.to(DEV), coef2.to(DEV), out.t, c.relu)
    torch.cuda.synchronize()
    assert _same(out.t, ref)
    _check_inputs(bda, by)
    out.assert_outside_intact()


@pytest.mark.parametrize("c", L.RED_CASES, ids=_ids)
def test_bn_relu_bwd_reduce_exact(C, c):
    """The partial rows fold to exactly sum(g) and sum(g * xhat); 1 <= T <= the rows offered; rows beyond T
    and the guard bands keep the sentinel."""
    da, y, coef, terms, sums = L.red_data(c)
    L.check_red_terms(terms, sums, masked=bool(c.relu))
    bda, by = _inp(da, c.views), _inp(y, c.views, (24, 8))
    part = F32Out(c.cap * 2 * c.C)
    T = C.bn_relu_bwd_reduce(bda.t, by.t, coef.to(DEV), c.relu, part.t)
    torch.cuda.synchronize()
    _check_partial(part, T, c.cap, c.C, sums)
    _check_inputs(bda, by)


# ---------------------------------------------------------------------------------------------
# exact class: the finalize kernels on synthetic partial rows
# ---------------------------------------------------------------------------------------------

def _ulps_apart(a, b):
    """Distance in fp32 ulps between two positive fp32 tensors."""
    return (a.view(torch.int32) - b.view(torch.int32)).abs().max().item()


@pytest.mark.parametrize("c", L.FIN_CASES, ids=_ids)
def test_bn_finalize_exact(C, c):
    """mean, invstd, scale, shift and running_mean are fixed fp32 values (integer mean, sigma = 2^j, eps = 0,
    momentum = 1/2): bitwise. running_var within one fp32 ulp of the fp64 value. T = 1 .. 2048 fold directly
    (4x-unrolled body and tail of fin_rows); 2049 and 5000 through colsum_kernel with a workspace, directly
    without. C = 96 leaves the last block of 64 channels half empty."""
    rows, gamma, beta, rmean, rvar, exp = L.fin_data(c)
    L.check_fin_rows(c, rows)
    coef = F32Out(4 * c.C)
    rm, rv = rmean.to(DEV), rvar.to(DEV)
    nbt = torch.tensor([5], dtype=torch.int64, device=DEV)
    ws = torch.full((64 * 2 * c.C,), NAN, device=DEV) if c.ws else None
    stats = rows.to(DEV).reshape(-1)
    C.bn_finalize(stats, c.T, L.FIN_COUNT, gamma.to(DEV), beta.to(DEV), rm, rv, nbt, 0.5, 0.0, coef.t, ws)
    torch.cuda.synchronize()
    want = torch.cat([exp["mean"], exp["invstd"], exp["scale"], exp["shift"]]).float()
    assert torch.equal(coef.t.cpu(), want)
    coef.assert_rest_intact(4 * c.C)
    assert torch.equal(rm.cpu(), exp["rmean"].float())
    assert _ulps_apart(rv.cpu(), exp["rvar"].float()) <= 1
    assert nbt.item() == 6
    assert torch.equal(stats.cpu(), rows.reshape(-1))


@pytest.mark.parametrize("c", L.FIN_CASES, ids=_ids)
def test_bn_bwd_finalize_exact(C, c):
    """dbeta / dgamma are the integer totals of the partial rows; coef2 = [A | B | Cc], formed by the kernel
    in fp64 and rounded once, equals the fp64 reference rounded to fp32 bit for bit."""
    rows, gamma, coef, exp = L.bwd_fin_data(c)
    L.check_fin_rows(c, rows)
    dg, db, coef2 = F32Out(c.C), F32Out(c.C), F32Out(3 * c.C)
    ws = torch.full((64 * 2 * c.C,), NAN, device=DEV) if c.ws else None
    C.bn_bwd_finalize(rows.to(DEV).reshape(-1), c.T, L.FIN_COUNT, gamma.to(DEV), coef.to(DEV), dg.t, db.t, coef2.t, ws)
    torch.cuda.synchronize()
    assert torch.equal(db.t.cpu(), exp["dbeta"].float())
    assert torch.equal(dg.t.cpu(), exp["dgamma"].float())
    assert torch.equal(coef2.t.cpu(), exp["coef2"].float())
    for o, n in ((dg, c.C), (db, c.C), (coef2, 3 * c.C)):
        o.assert_rest_intact(n)


# ---------------------------------------------------------------------------------------------
# exact class: max pool and its BN fusions
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.POOL_CASES, ids=_ids)
def test_maxpool2_fwd_bwd_exact(C, c):
    """maxpool2_fwd bitwise F.max_pool2d (fp64); maxpool2_bwd bitwise its autograd (+ dskip): ternary inputs,
    so most windows tie and the first maximum in row-major order must win; an uncovered last row / column
    receives dskip alone (zero without it). The big case wraps the 4096-block grid-stride loops."""
    dev = DEV if c.big else "cpu"
    x, dp, ds = L.pool_data(c, dev)
    fwd_items, bwd_items = L.pool_items(c)
    assert (bwd_items > L.POOL_GRID_CAP * 256) == c.big and (fwd_items > L.POOL_GRID_CAP * 256) == c.big
    assert L.tie_fraction(x.double()) > 0.5
    p_ref, dx_ref = L.pool_ref(x.double(), dp, ds)
    bx = _inp(x, c.views)
    p = _out((c.N, c.H // 2, c.W // 2, c.C), c.views, (16, 16))
    C.maxpool2_fwd(bx.t, p.t)
    torch.cuda.synchronize()
    assert _same(p.t, p_ref)
    p.assert_outside_intact()
    bdp, bds = _inp(dp, c.views, (8, 8)), _inp(ds, c.views, (24, 8))
    dx = _out(x.shape, c.views)
    C.maxpool2_bwd(bdp.t, bx.t, bds.t if bds else None, dx.t)
    torch.cuda.synchronize()
    assert _same(dx.t, dx_ref)
    if c.H % 2:
        assert torch.equal(dx.t[:, -1], bds.t[:, -1] if bds else torch.zeros_like(dx.t[:, -1]))
    if c.W % 2:
        assert torch.equal(dx.t[:, :, -1], bds.t[:, :, -1] if bds else torch.zeros_like(dx.t[:, :, -1]))
    _check_inputs(bx, bdp, bds)
    dx.assert_outside_intact()


@pytest.mark.parametrize("c", L.POOLFUSE_CASES + [L.APPLY_POOL_BIG], ids=_ids)
def test_bn_relu_apply_pool_exact(C, c):
    """a = relu(bn(y)) and its 2x2 max pool, both bitwise the fp64 reference (not merely the unfused
    kernels); the pool-only form (a = None) writes the same pool. The big case exceeds the 16384-block cap."""
    assert L.bf16_exact(L.poolfuse_table(c))
    assert (L.apply_pool_blocks(c) > L.APPLY_POOL_GRID_CAP) == c.big
    y, _, _, coef, a_ref = L.poolfuse_data(c, DEV if c.big else "cpu")
    p_ref, _ = L.pool_ref(a_ref, None, None)
    by = _inp(y, c.views)
    pshape = (c.N, c.H // 2, c.W // 2, c.C)
    a, p = _out(y.shape, c.views), _out(pshape, c.views, (16, 16))
    C.bn_relu_apply_pool(by.t, a.t, p.t, coef.to(DEV))
    torch.cuda.synchronize()
    assert _same(a.t, a_ref)
    assert _same(p.t, p_ref)
    p2 = _out(pshape, c.views, (24, 8))
    C.bn_relu_apply_pool(by.t, None, p2.t, coef.to(DEV))
    torch.cuda.synchronize()
    assert _same(p2.t, p_ref)
    _check_inputs(by)
    for o in (a, p, p2):
        o.assert_outside_intact()


@pytest.mark.parametrize("c", L.POOLFUSE_CASES, ids=_ids)
def test_maxpool2_bwd_bn_reduce_exact(C, c):
    """dx = maxpool_bwd(dp) (+ dskip) with the argmax recomputed from relu(bn(y)) -- post-ReLU zeros tie
    constantly, the first maximum in row-major order wins -- bitwise the fp64 autograd; the partial rows fold
    to exactly sum(g) and sum(g * xhat) of that dx."""
    y, dp, ds, coef, a_ref = L.poolfuse_data(c)
    assert L.tie_fraction(a_ref) > 0.2
    _, dx_ref = L.pool_ref(a_ref, dp, ds)
    terms, sums = L.reduce_terms(dx_ref, y, coef)
    L.check_red_terms(terms, sums)
    by, bdp, bds = _inp(y, c.views), _inp(dp, c.views, (8, 8)), _inp(ds, c.views, (24, 8))
    ba = _inp(L.expected_bf16(a_ref), c.views)
    dx = _out(y.shape, c.views)
    part = F32Out(c.cap * 2 * c.C)
    T = C.maxpool2_bwd_bn_reduce(bdp.t, ba.t, bds.t if bds else None, dx.t, by.t, coef.to(DEV), part.t)
    torch.cuda.synchronize()
    assert _same(dx.t, dx_ref)
    _check_partial(part, T, c.cap, c.C, sums)
    _check_inputs(by, bdp, bds, ba)
    dx.assert_outside_intact()


# ---------------------------------------------------------------------------------------------
# 2. per-element class
# ---------------------------------------------------------------------------------------------

def _per_element(name, got, ref64, slop, bound_text):
    """Assert |got - ref| <= 1/2 ulp_bf16(ref) + slop on every element, after printing the margin."""
    ref64, slop = ref64.to(got.device), slop.to(got.device)
    bound = 0.5 * L.ulp_bf16(ref64) + slop
    err = (got.double() - ref64).abs()
    ok = err <= bound
    zero = torch.zeros_like(err)  # bound = 0 (ref = 0, no slop): any error at all is infinitely far out
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, zero + float("inf"), zero))
    frac = frac.max().item()
    # how much of the slop is used: the part of the error beyond 1/2 ulp, as a fraction of the slop
    over = err - 0.5 * L.ulp_bf16(ref64)
    used = torch.where(slop > 0, over / slop.clamp_min(1e-300), zero).clamp_min(0).max().item()
    differ = (got != ref64.float().to(L.BF16)).sum().item()
    print(f"[pass_exact] {name}: bound = 1/2 ulp_bf16(ref) + {bound_text}; max slop {slop.max().item():.3e}; "
          f"max err / bound = {frac:.4f}; max slop used = {used:.4f}; "
          f"{differ} of {got.numel()} elements differ from RNE_bf16(ref)")
    assert ok.all(), f"{name}: {(~ok).sum().item()} elements exceed the bound (worst err / bound = {frac:.3f})"


def _randn_bf16(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g, device=DEV) * scale + shift).to(L.BF16)


def _real_coef(Ch, seed):
    """[mean | invstd | scale | shift] of a plausible trained layer (not dyadic)."""
    g = L.generator(seed)
    mean, inv = torch.randn(Ch, generator=g) * 0.3, torch.rand(Ch, generator=g) + 0.5
    gamma, beta = torch.randn(Ch, generator=g), torch.randn(Ch, generator=g) * 0.2
    sc = gamma * inv
    return torch.cat([mean, inv, sc, beta - mean * sc]).to(DEV)


def _act_ref(y, coef):
    """fp64 reference of the stored activation bf16(fp32 relu(fma(y, scale, shift))), as a double tensor,
    and the fp64 pre-rounding value. y * scale is exact in fp64 and the sum rounds at 2^-53, so rounding the
    fp64 result to fp32 gives the fma's fp32 value."""
    Ch = y.shape[-1]
    z = torch.relu(y.double() * coef[2 * Ch:3 * Ch].double() + coef[3 * Ch:4 * Ch].double())
    return z.float().to(L.BF16).double(), z


def _tap_span(x64, dim):
    """Largest |difference| of neighbouring taps along dim, per (image, channel): [N,1,1,C]."""
    if x64.shape[dim] < 2:
        return torch.zeros(x64.shape[0], 1, 1, x64.shape[3], dtype=torch.float64, device=x64.device)
    return x64.diff(dim=dim).abs().amax((1, 2), keepdim=True)


def _up_fwd_slop(x64, c):
    """The kernel forms src = (float)(in - 1) / (float)(2 in - 1) * u in fp32: against the fp64 index that is
    off by at most in * 2^-22 (two roundings of a value below in, plus the rounding of 1 - l), and the
    interpolant is piecewise linear and continuous in src, so the output moves by at most that times the
    difference of the neighbouring taps -- bounded per (image, channel) by the largest such difference,
    vertical and horizontal. The blend itself is 8 fp32 operations on sum |w * tap|."""
    S = L.up_ref(x64.abs(), c)
    return 2.0 ** -22 * (c.hin * _tap_span(x64, 1) + c.win * _tap_span(x64, 2)) + 8 * U32 * S


def _check_up_fwd(name, out, ref, slop, c):
    _per_element(name, out.t, ref, slop, "2^-22 (hin Dv + win Dh) + 8 * 2^-24 sum|w tap|")
    inside = torch.zeros(c.Hout, c.Wout, dtype=torch.bool, device=DEV)
    inside[c.oy:c.oy + 2 * c.hin, c.ox:c.ox + 2 * c.win] = True
    assert (out.t[:, ~inside].view(torch.int16) == 0).all(), "the pad region must be bitwise +0"
    out.assert_outside_intact()


@pytest.mark.parametrize("c", L.UP_FWD_CASES, ids=_ids)
def test_upsample2_fwd_per_element(C, c):
    """upsample2_fwd against fp64 F.interpolate(align_corners=True) + centred pad (on the device), every band
    height R = 1, 2, 4, 8 with ragged last bands and chunks at odd pad offsets, hin = 1 and win = 1. With
    `coef` also the fused producer BN + ReLU form, against the fp64 interpolation of the bf16-rounded
    activation, and equal to apply-then-upsample bit for bit."""
    L.check_up_shape(c, fwd=True)
    x = _randn_bf16((c.N, c.hin, c.win, c.C), 100 + c.seed)
    bx = _inp(x, c.views)
    oshape = (c.N, c.Hout, c.Wout, c.C)
    out = _out(oshape, c.views)
    C.upsample2_fwd(bx.t, out.t, c.oy, c.ox)
    torch.cuda.synchronize()
    x64 = x.double()
    _check_up_fwd(c.name, out, L.up_ref(x64, c), _up_fwd_slop(x64, c), c)
    _check_inputs(bx)
    if not c.coef:
        return
    del x64
    y = _randn_bf16((c.N, c.hin, c.win, c.C), 200 + c.seed, 2.0, 0.3)
    coef = _real_coef(c.C, 300 + c.seed)
    by = _inp(y, c.views)
    fused = _out(oshape, c.views)
    C.upsample2_fwd(by.t, fused.t, c.oy, c.ox, coef)
    torch.cuda.synchronize()
    a64, _ = _act_ref(y, coef)
    _check_up_fwd(c.name + "+bn", fused, L.up_ref(a64, c), _up_fwd_slop(a64, c), c)
    a = torch.empty_like(y)
    C.bn_relu_apply(y, a, coef, 1)
    unfused = torch.empty(oshape, dtype=L.BF16, device=DEV)
    C.upsample2_fwd(a, unfused, c.oy, c.ox)
    torch.cuda.synchronize()
    assert torch.equal(fused.t, unfused)
    _check_inputs(by)


def _up_bwd_slop(d64, c):
    """dx = sum over a 4 x 4 window of wy * wx * dout. Each fp32 weight is off by at most in * 2^-22 (see the
    forward; a weight that moves to the neighbouring input row keeps that bound, the hat function being
    continuous), the other weight is at most 1, so the weights contribute 2^-22 (hin + win) * (the window's
    sum |dout|); the 16 multiply-adds and 8 weight products are 24 fp32 operations on sum |wy wx dout|."""
    S = L.up_bwd_ref(d64.abs(), c)
    win = d64[:, c.oy:c.oy + 2 * c.hin, c.ox:c.ox + 2 * c.win].abs().permute(0, 3, 1, 2)
    W4 = 16 * F.avg_pool2d(F.pad(win, (1, 1, 1, 1)), 4, 2).permute(0, 2, 3, 1)
    return 2.0 ** -22 * (c.hin + c.win) * W4 + 24 * U32 * S


BWD_BOUND = "2^-22 (hin + win) sum_4x4|dout| + 24 * 2^-24 sum|wy wx dout|"


@pytest.mark.parametrize("c", L.UP_BWD_CASES, ids=_ids)
def test_upsample2_bwd_per_element(C, c):
    """upsample2_bwd against the fp64 autograd of interpolate + pad: band heights R = 1, 2, 4 with ragged
    last bands (hin % R != 0) and chunks, odd pad offsets, hin = 1 and win = 1. With `bnred` the fused
    BN-reduction form must write the same dx."""
    L.check_up_shape(c, fwd=False)
    dout = _randn_bf16((c.N, c.Hout, c.Wout, c.C), 400 + c.seed)
    bd = _inp(dout, c.views)
    dx = _out((c.N, c.hin, c.win, c.C), c.views)
    assert C.upsample2_bwd(bd.t, dx.t, c.oy, c.ox) == 0
    torch.cuda.synchronize()
    d64 = dout.double()
    _per_element(c.name, dx.t, L.up_bwd_ref(d64, c), _up_bwd_slop(d64, c), BWD_BOUND)
    _check_inputs(bd)
    dx.assert_outside_intact()
    if c.bnred:
        y = _randn_bf16((c.N, c.hin, c.win, c.C), 500 + c.seed, 2.0, 0.3)
        dx2 = _out((c.N, c.hin, c.win, c.C), c.views)
        part = F32Out(64 * 2 * c.C)
        T = C.upsample2_bwd(bd.t, dx2.t, c.oy, c.ox, y, _real_coef(c.C, 600 + c.seed), part.t)
        torch.cuda.synchronize()
        assert 1 <= T <= 64 and torch.equal(dx2.t, dx.t)
        part.assert_rest_intact(T * 2 * c.C)
        dx2.assert_outside_intact()


@pytest.mark.parametrize("c", L.UP_BNRED_CASES, ids=_ids)
def test_upsample2_bwd_bn_reduce_exact(C, c):
    """upsample2_bwd with the fused BN reduction: dx by the per-element criterion, and the partial rows fold
    to exactly sum(g) and sum(g * xhat) of the dx the kernel wrote (read back; dx itself is not dyadic). With
    dout in 4..6 that dx lies in [8, 32), two binades of bf16, and the terms meet assert_f32_sums -- asserted
    here on the dx read back. R = 2 and 4 at C = 2048, where the band heights need the fewest pixels."""
    L.check_up_shape(c, fwd=False)
    dout, y, coef = L.up_bnred_inputs(c)
    dout, y = dout.to(DEV), y.to(DEV)
    cap = 300
    dx = _out((c.N, c.hin, c.win, c.C), False)
    part = F32Out(cap * 2 * c.C)
    T = C.upsample2_bwd(dout, dx.t, c.oy, c.ox, y, coef.to(DEV), part.t)
    torch.cuda.synchronize()
    d64 = dout.double()
    _per_element(c.name, dx.t, L.up_bnred_ref_dx(c, dout), _up_bwd_slop(d64, c), BWD_BOUND)
    del d64
    got = dx.t.double()
    assert got.min().item() >= 8 and got.max().item() < 32
    terms, sums = L.reduce_terms(got, y, coef)
    L.check_red_terms(terms, sums)
    _check_partial(part, T, cap, c.C, sums)


# -- BN apply, backward apply and the pool fusions on realistic values ---------------------------------

REAL_SHAPES = [(2, 37, 29, 64), (1, 9, 11, 512)]


def _finalized(C, y, seed):
    """coef of a training BN over y, out of bn_finalize itself (so nothing about it is dyadic)."""
    Ch = y.shape[-1]
    g = L.generator(seed)
    gamma = (torch.rand(Ch, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(Ch, generator=g) * 0.1).to(DEV)
    yf = y.float().reshape(-1, Ch)
    stats = torch.cat([yf.sum(0), (yf * yf).sum(0)]).contiguous()
    coef = torch.zeros(4 * Ch, device=DEV)
    C.bn_finalize(stats, 1, yf.shape[0], gamma, beta, None, None, None, 0.1, 1e-5, coef, None)
    return gamma, coef


@pytest.mark.parametrize("N,H,W,Ch", REAL_SHAPES)
def test_bn_apply_and_pool_realistic(C, N, H, W, Ch):
    """bn_relu_apply and bn_relu_apply_pool on Gaussian bf16 y with coefficients out of bn_finalize. One fma:
    slop = 2^-24 (|y * scale| + |shift|). The pool is the exact 2x2 maximum of the stored activation."""
    y = _randn_bf16((N, H, W, Ch), 700 + Ch, 2.0, 0.5)
    _, coef = _finalized(C, y, 701)
    sc, sh = coef[2 * Ch:3 * Ch].double(), coef[3 * Ch:].double()
    ref = torch.relu(y.double() * sc + sh)
    slop = U32 * ((y.double() * sc).abs() + sh.abs())
    a = torch.full_like(y, L.SENTINEL)
    C.bn_relu_apply(y, a, coef, 1)
    a2 = torch.full_like(y, L.SENTINEL)
    p = torch.full((N, H // 2, W // 2, Ch), L.SENTINEL, dtype=L.BF16, device=DEV)
    C.bn_relu_apply_pool(y, a2, p, coef)
    torch.cuda.synchronize()
    _per_element(f"bn_relu_apply {N}x{H}x{W}x{Ch}", a, ref, slop, "2^-24 (|y scale| + |shift|)")
    _per_element(f"bn_relu_apply_pool {N}x{H}x{W}x{Ch}", a2, ref, slop, "2^-24 (|y scale| + |shift|)")
    assert (a > 0).any() and (a == 0).any()
    assert _same(p, L.pool_ref(a2.double(), None, None)[0])


@pytest.mark.parametrize("N,H,W,Ch", REAL_SHAPES)
def test_bn_bwd_realistic(C, N, H, W, Ch):
    """bn_relu_bwd_reduce -> bn_bwd_finalize -> bn_relu_bwd_apply and maxpool2_bwd_bn_reduce on Gaussian
    values. dy = fma(A, g, fma(B, y, Cc)): two roundings, slop = 2^-23 (|A g| + |B y| + |Cc|), coef2 taken as
    the kernel chain produced it. The fused pool backward adds two bf16 values in fp32: slop = 2^-24 (|dskip|
    + |dp|). The fp32 partial sums (at most M terms per chain, three operations per term) are within
    (M + 3) 2^-24 sum|t| of the fp64 sums."""
    M = N * H * W
    y = _randn_bf16((N, H, W, Ch), 800 + Ch, 2.0, 0.5)
    da = _randn_bf16((N, H, W, Ch), 801 + Ch)
    gamma, coef = _finalized(C, y, 802)
    part = torch.full((1024 * 2 * Ch,), L.SENTINEL, device=DEV)
    T = C.bn_relu_bwd_reduce(da, y, coef, 1, part)
    dg, db, coef2 = (torch.zeros(k * Ch, device=DEV) for k in (1, 1, 3))
    C.bn_bwd_finalize(part, T, M, gamma, coef, dg, db, coef2, None)
    dy = torch.full_like(y, L.SENTINEL)
    C.bn_relu_bwd_apply(da, y, coef, coef2, dy, 1)
    torch.cuda.synchronize()

    def sums_ok(name, part, T, g64):
        terms, sums = L.reduce_terms(g64, y, coef)
        got = part[:T * 2 * Ch].view(T, 2, Ch).double().sum(0)
        for k in (0, 1):
            bound = (M + 3) * U32 * terms[k].abs().reshape(-1, Ch).sum(0)
            frac = ((got[k] - sums[k]).abs() / bound).max().item()
            print(f"[pass_exact] {name} sums[{k}] {N}x{H}x{W}x{Ch}: bound = (M + 3) 2^-24 sum|t|; "
                  f"max err / bound = {frac:.4f}")
            assert frac <= 1
        return sums

    sums_ok("bn_relu_bwd_reduce", part, T, da.double())
    A, B, Cc = (coef2[k * Ch:(k + 1) * Ch].double() for k in range(3))
    yd = y.double()
    g = da.double() * ((yd * coef[2 * Ch:3 * Ch].double() + coef[3 * Ch:].double()) > 0)
    _per_element(f"bn_relu_bwd_apply {N}x{H}x{W}x{Ch}", dy, A * g + B * yd + Cc,
                 2 * U32 * ((A * g).abs() + (B * yd).abs() + Cc.abs()), "2^-23 (|A g| + |B y| + |Cc|)")
    # fused pool backward + reduce
    a64, _ = _act_ref(y, coef)
    dp = _randn_bf16((N, H // 2, W // 2, Ch), 803 + Ch)
    ds = _randn_bf16((N, H, W, Ch), 804 + Ch)
    _, routed = L.pool_ref(a64, dp, None)
    dx = torch.full_like(y, L.SENTINEL)
    part2 = torch.full((1024 * 2 * Ch,), L.SENTINEL, device=DEV)
    T2 = C.maxpool2_bwd_bn_reduce(dp, a64.to(L.BF16), ds, dx, y, coef, part2)
    torch.cuda.synchronize()
    _per_element(f"maxpool2_bwd_bn_reduce {N}x{H}x{W}x{Ch}", dx, routed + ds.double(),
                 U32 * (routed.abs() + ds.double().abs()), "2^-24 (|dskip| + |dp|)")
    sums_ok("maxpool2_bwd_bn_reduce", part2, T2, dx.double())
