"""The pass-kernel cases of tests/lattice.py on the CPU: every case of tests/test_pass_exact_gpu.py is checked
here against the preconditions under which its demand (bitwise equality, exact fp32 sums, a given band
height) is sound -- from the reference and the launchers' formulas alone, without the native extension.

The elementwise passes' preconditions depend only on the input value set and the coefficients, so they are
proven on the table of every (input value, channel) pair; the small cases are also checked on their data."""
import pytest
import torch

import lattice as L

DATA_LIMIT = 1 << 22  # elements: larger cases are covered by their value tables alone here


def _ids(c):
    return c.name


# -- helpers ---------------------------------------------------------------------------------------

def test_launcher_formulas():
    # grid_px / px_chunk: C = 64 -> 32 pixel rows per block, 128 pixels per step
    assert L.px_grid(35, 64) == (1, 128, 32)
    assert L.px_grid(2146, 64) == (17, 128, 32)
    assert L.px_grid(264579, 64) == (2048, 256, 32)
    assert L.px_grid(8463, 2048) == (2048, 8, 1)
    # the benchmark's bs 64, 16^2 -> 32^2 x 512 upsample takes R = 4; 128^2 -> 256^2 x 64 takes 8
    assert L.up_band_rows(64, 32, 32, 512, 8) == 4
    assert L.up_band_rows(64, 256, 256, 64, 8) == 8
    assert L.up_band_rows(1, 256, 256, 64, 8) == 1
    assert L.up_band_rows(64, 128, 128, 64, 4) == 4


def test_split_rows_sum_exactly():
    g = L.generator(3)
    total = torch.tensor([0, 1, -1, 16384 * 3, -16384 * 25, 4999, -5001])
    for T in (1, 2, 17, 5000):
        rows = L.split_rows(total, T, g)
        assert rows.shape == (T, 7) and torch.equal(rows.sum(0), total)
    assert L.split_rows(total, 64, g).unique().numel() > 8  # not a constant split


def test_ulp_bf16():
    v = torch.tensor([0.0, 1.0, -1.5, 1.9999, 2.0, 255.0, 256.0, 3e-5], dtype=torch.float64)
    u = L.ulp_bf16(v)
    assert u.tolist()[:7] == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0]
    # against bf16 itself: the gap from the bf16 value at or below |x| to the next one up
    for x, s in zip(v[1:].abs().tolist(), u[1:].tolist()):
        bits = torch.tensor(x, dtype=torch.float32).view(torch.int32) >> 16  # truncate to bf16
        lo, hi = (((bits + k) << 16).view(torch.float32).item() for k in (0, 1))
        assert lo <= x < hi and hi - lo == s


# -- bn_relu_apply / bn_relu_bwd_apply ---------------------------------------------------------------

@pytest.mark.parametrize("c", L.PX_CASES, ids=_ids)
def test_px_case_shapes(c):
    assert c.C in (8, 64, 512, 2048)
    L.check_px_shape(c)


def test_px_cases_cover_the_issue_grid():
    for C in (8, 64, 512, 2048):
        assert any(c.C == C and c.capped for c in L.PX_CASES) and any(c.C == C and not c.capped for c in L.PX_CASES)
    assert any(c.views and c.capped for c in L.PX_CASES) and any(c.views and not c.capped for c in L.PX_CASES)
    assert {c.relu for c in L.PX_CASES if c.cls == "exact"} == {0, 1}
    assert any(c.cls == "round" for c in L.PX_CASES)


@pytest.mark.parametrize("c", L.PX_CASES, ids=_ids)
def test_apply_case_preconditions(c):
    tab = L.apply_table(c)
    L.check_apply_table(c, tab)
    coef = L.apply_coef(c)
    sc, sh = coef[2 * c.C:3 * c.C], coef[3 * c.C:]
    assert torch.equal(torch.frexp(sc.abs())[0], torch.full_like(sc, 0.5)) and torch.equal(sh, sh.round())
    assert (sc > 0).any() and (sc < 0).any()
    if c.M * c.C <= DATA_LIMIT:
        y, _, ref = L.apply_data(c)
        assert y.abs().max().item() <= 3 and set(ref.unique().tolist()) <= set(tab.unique().tolist())
        if c.cls == "round":
            L.assert_rounding_class(ref)
        else:
            assert L.bf16_exact(ref)


@pytest.mark.parametrize("c", L.PX_CASES, ids=_ids)
def test_bwd_apply_case_preconditions(c):
    tab = L.bwd_apply_table(c)
    L.check_bwd_apply_table(c, tab)
    coef, coef2 = L.bwd_apply_coefs(c)
    A = coef2[:c.C]
    assert torch.equal(torch.frexp(A.abs())[0], torch.full_like(A, 0.5)) and (A > 0).any() and (A < 0).any()
    assert torch.equal(coef2[c.C:], coef2[c.C:].round())
    if c.M * c.C <= DATA_LIMIT:
        da, y, _, _, ref = L.bwd_apply_data(c)
        assert da.abs().max().item() <= 3 and y.abs().max().item() <= 1
        assert set(ref.unique().tolist()) <= set(tab.unique().tolist())
        if c.cls == "round":
            L.assert_rounding_class(ref)
        else:
            assert L.bf16_exact(ref)


# -- reductions -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.RED_CASES, ids=_ids)
def test_red_case_preconditions(c):
    da, y, coef, terms, sums = L.red_data(c)
    L.check_red_terms(terms, sums, masked=bool(c.relu))
    assert c.C % 8 == 0 and c.C <= 2048 and c.cap >= 1
    natural = L.cdiv(c.N * c.H * c.W, (256 // (c.C // 8)) * 8)
    if "wraps" in c.name:
        assert natural > c.cap  # the grid-stride loop wraps
    else:
        assert natural < c.cap  # rows beyond T exist and must stay untouched


@pytest.mark.parametrize("c", L.POOLFUSE_CASES, ids=_ids)
def test_poolfuse_case_preconditions(c):
    y, dp, ds, coef, a = L.poolfuse_data(c)
    tab = L.poolfuse_table(c)
    assert L.bf16_exact(tab) and L.bf16_exact(a) and (tab == 0).any() and (tab > 0).any()
    assert L.tie_fraction(a) > 0.2  # post-ReLU zeros tie constantly
    _, dx = L.pool_ref(a, dp, ds)
    assert L.bf16_exact(dx) and dx.abs().max().item() <= 6
    terms, sums = L.reduce_terms(dx, y, coef)
    L.check_red_terms(terms, sums)
    if c.H % 2:
        assert torch.equal(dx[:, -1], ds[:, -1].double() if c.dskip else torch.zeros_like(dx[:, -1]))
    if c.W % 2:
        assert torch.equal(dx[:, :, -1], ds[:, :, -1].double() if c.dskip else torch.zeros_like(dx[:, :, -1]))
    natural = L.cdiv(c.N * L.cdiv(c.H, 2) * L.cdiv(c.W, 2), 4 * (256 // (c.C // 8)))
    assert (natural > c.cap) == ("wraps" in c.name)
    assert L.apply_pool_blocks(c) < L.APPLY_POOL_GRID_CAP


def test_apply_pool_big_case_reaches_the_cap():
    c = L.APPLY_POOL_BIG
    assert c.big and L.apply_pool_blocks(c) > L.APPLY_POOL_GRID_CAP
    tab = L.poolfuse_table(c)
    assert L.bf16_exact(tab) and (tab == 0).any() and (tab > 0).any()
    assert c.H % 2 == 1 and c.W % 2 == 1


@pytest.mark.parametrize("c", L.POOL_CASES, ids=_ids)
def test_pool_case_preconditions(c):
    fwd, bwd = L.pool_items(c)
    if c.big:
        assert fwd > L.POOL_GRID_CAP * 256 and bwd > L.POOL_GRID_CAP * 256  # both grid-stride loops wrap
        return
    assert bwd <= L.POOL_GRID_CAP * 256
    x, dp, ds = L.pool_data(c)
    assert set(x.float().unique().tolist()) == {-1.0, 0.0, 1.0}
    assert L.tie_fraction(x.double()) > 0.5  # ternary inputs: most windows tie
    p, dx = L.pool_ref(x.double(), dp, ds)
    assert L.bf16_exact(p) and L.bf16_exact(dx) and (dx != 0).any()
    assert (ds is None) == (not c.dskip)


def test_pool_cases_cover_the_issue_grid():
    small = [c for c in L.POOL_CASES if not c.big]
    assert {c.C for c in small} == {8, 64, 512}
    assert {(c.H % 2, c.W % 2) for c in small} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    assert {c.dskip for c in small} == {True, False} and any(c.views for c in small)
    fuse = L.POOLFUSE_CASES
    assert {(c.H % 2, c.W % 2) for c in fuse} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    assert {c.dskip for c in fuse} == {True, False} and any(c.views for c in fuse)


# -- finalize ---------------------------------------------------------------------------------------

def test_fin_cases_cover_the_issue_grid():
    direct = {(c.T, c.C) for c in L.FIN_CASES if c.T <= L.FIN_DIRECT_ROWS}
    assert direct == {(T, C) for T in (1, 16, 17, 63, 64, 65, 2048) for C in (64, 96, 512)}
    big = {(c.T, c.C, c.ws) for c in L.FIN_CASES if c.T > L.FIN_DIRECT_ROWS}
    assert big == {(T, C, ws) for T in (2049, 5000) for C in (64, 96, 512) for ws in (True, False)}
    assert len({c.name for c in L.FIN_CASES}) == len(L.FIN_CASES)


@pytest.mark.parametrize("c", L.FIN_CASES, ids=_ids)
def test_fin_case_preconditions(c):
    rows, gamma, beta, rmean, rvar, exp = L.fin_data(c)
    L.check_fin_rows(c, rows)
    cnt = float(L.FIN_COUNT)
    s, q = rows.double().sum(0).view(2, c.C)
    assert torch.equal(s / cnt, exp["mean"]) and torch.equal(q / cnt - exp["mean"] ** 2, exp["invstd"] ** -2)
    for k in ("mean", "invstd", "scale", "shift", "rmean"):  # fixed fp32 values
        assert L.f32_exact(exp[k]), k
    assert not L.f32_exact(exp["rvar"])  # count / (count - 1) rounds: compared within one ulp
    assert (exp["invstd"] != 1).any() and (exp["mean"] != 0).any()


@pytest.mark.parametrize("c", L.FIN_CASES, ids=_ids)
def test_bwd_fin_case_preconditions(c):
    rows, gamma, coef, exp = L.bwd_fin_data(c)
    L.check_fin_rows(c, rows)
    s, q = rows.double().sum(0).view(2, c.C)
    assert torch.equal(s, exp["dbeta"]) and torch.equal(q, exp["dgamma"])
    assert L.f32_exact(exp["dbeta"]) and L.f32_exact(exp["dgamma"]) and L.f32_exact(exp["coef2"])
    assert (exp["coef2"][c.C:] != 0).float().mean() > 0.9  # B and Cc are not trivially zero


# -- upsample ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.UP_FWD_CASES, ids=_ids)
def test_up_fwd_case_band_height(c):
    L.check_up_shape(c, fwd=True)


@pytest.mark.parametrize("c", L.UP_BWD_CASES + L.UP_BNRED_CASES, ids=_ids)
def test_up_bwd_case_band_height(c):
    L.check_up_shape(c, fwd=False)


def test_up_cases_cover_the_issue_grid():
    for table, heights in ((L.UP_FWD_CASES, (2, 4, 8)), (L.UP_BWD_CASES, (2, 4))):
        assert any(c.R == 1 and c.hin == 1 for c in table) and any(c.R == 1 and c.win == 1 for c in table)
        for R in heights:
            cs = {c.C for c in table if c.R == R}
            assert len(cs & {64, 128, 512}) >= 2, f"R = {R}: channel counts {cs}"
        assert any(c.views and c.R > 1 for c in table) and any(c.views and c.R == 1 for c in table)
    assert {c.R for c in L.UP_FWD_CASES if c.coef} == {1, 2, 4, 8}
    assert {c.R for c in L.UP_BNRED_CASES} == {1, 2, 4}


@pytest.mark.parametrize("c", L.UP_BNRED_CASES, ids=_ids)
def test_up_bnred_case_preconditions(c):
    """The GPU test asserts these on the dx it reads back; here on the bf16-rounded fp64 autograd dx, which
    differs from it by an ulp at most on a few elements."""
    dout, y, coef = L.up_bnred_inputs(c)
    dx = L.up_bnred_ref_dx(c, dout).to(L.BF16).double()
    assert dx.min().item() >= 8 and dx.max().item() < 32
    terms, sums = L.reduce_terms(dx, y, coef)
    L.check_red_terms(terms, sums)


def test_up_reference_matches_the_index_arithmetic():
    """up_ref against the definition: src = dst * (in - 1) / (out - 1), blend of the two neighbours."""
    c = L.UP_FWD_CASES[3]
    x = torch.randn(c.N, c.hin, c.win, 8, generator=L.generator(1), dtype=torch.float64)
    ref = L.up_ref(x, c)
    assert ref.shape == (c.N, c.Hout, c.Wout, 8)
    inside = torch.zeros(c.Hout, c.Wout, dtype=torch.bool)
    inside[c.oy:c.oy + 2 * c.hin, c.ox:c.ox + 2 * c.win] = True
    assert (ref[:, ~inside] == 0).all()
    for (uy, ux) in ((0, 0), (3, 5), (2 * c.hin - 1, 2 * c.win - 1), (4, 13)):
        sy, sx = uy * (c.hin - 1) / (2 * c.hin - 1), ux * (c.win - 1) / (2 * c.win - 1)
        y0, x0 = int(sy), int(sx)
        y1, x1 = min(y0 + 1, c.hin - 1), min(x0 + 1, c.win - 1)
        ly, lx = sy - y0, sx - x0
        v = (1 - ly) * ((1 - lx) * x[:, y0, x0] + lx * x[:, y0, x1]) + ly * ((1 - lx) * x[:, y1, x0] + lx * x[:, y1, x1])
        assert torch.allclose(ref[:, uy + c.oy, ux + c.ox], v, rtol=0, atol=1e-12)


def test_pass_case_names_are_unique():
    for table in (L.PX_CASES, L.RED_CASES, L.POOL_CASES, L.POOLFUSE_CASES + [L.APPLY_POOL_BIG], L.FIN_CASES,
                  L.UP_FWD_CASES, L.UP_BWD_CASES + L.UP_BNRED_CASES):
        names = [c.name for c in table]
        assert len(names) == len(set(names))
