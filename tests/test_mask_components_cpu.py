"""The mask component filter's definition (geometry/components.py), its configuration and the CPU serving path."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn as nn

from mask_component_cases import DENSITIES, checkerboard, random_mask, structures

from robotic_discovery_platform_amd.config import ServeConfig, add_dataclass_args, apply_env, from_args
from robotic_discovery_platform_amd.data.image_io import resize_nearest
from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
from robotic_discovery_platform_amd.geometry.components import filter_components_reference
from robotic_discovery_platform_amd.geometry.curvature import compute_curvature_profile
from robotic_discovery_platform_amd.serve.engine import CpuFramePipeline, EnginePool


def flood_fill_filter(mask, keep, min_area):
    """The definition again, by brute force: a stack flood fill in raster order, no scipy."""
    H, W = mask.shape
    label = np.zeros((H, W), np.int64)
    comps = []  # pixel lists, in the order of their first pixel
    for y0 in range(H):
        for x0 in range(W):
            if mask[y0, x0] == 0 or label[y0, x0]:
                continue
            label[y0, x0] = len(comps) + 1
            stack, px = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                px.append((y, x))
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if mask[yy, xx] and not label[yy, xx]:
                            label[yy, xx] = len(comps) + 1
                            stack.append((yy, xx))
            comps.append(px)
    alive = [c for c in comps if len(c) >= min_area]
    if keep == "largest" and alive:
        best = max(len(c) for c in alive)
        alive = [next(c for c in alive if len(c) == best)]  # comps are in first-pixel order
    out = np.zeros_like(mask)
    for c in alive:
        for y, x in c:
            out[y, x] = mask[y, x]
    kept = sum(len(c) for c in alive)
    return out, np.array([len(comps), len(alive), kept, int((mask > 0).sum()) - kept], np.int32)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (37, 53), (64, 96)])
@pytest.mark.parametrize("density", DENSITIES)
def test_reference_matches_flood_fill(H, W, density):
    m = random_mask(H, W, density, value=255 if density > 0.35 else 1)
    biggest = int(flood_fill_filter(m, "largest", 0)[1][2])
    for keep in ("all", "largest"):
        for min_area in (0, 1, 2, 9, biggest, biggest + 1):
            got, st = filter_components_reference(m, keep, min_area)
            want, wst = flood_fill_filter(m, keep, min_area)
            assert np.array_equal(got, want) and got.dtype == np.uint8, (keep, min_area)
            assert np.array_equal(st, wst) and st.dtype == np.int32, (keep, min_area, st, wst)


def test_structure_component_counts():
    for name, m, ncomp in structures():
        assert int(filter_components_reference(m)[1][0]) == ncomp, name


def test_hand_cases():
    f = filter_components_reference
    # two equal-area blobs: the one whose first pixel comes first stays -- here the RIGHT one (row 0), although
    # the left one starts in an earlier column
    m = np.zeros((8, 12), np.uint8)
    m[1:3, 1:3] = 1
    m[0:2, 8:10] = 1
    out, st = f(m, "largest", 0)
    assert out[0:2, 8:10].all() and out.sum() == 4 and st.tolist() == [2, 1, 4, 4]
    # a component whose first pixel is not in its first 2 x 2 cell still wins the tie by that pixel
    m = np.zeros((6, 12), np.uint8)
    m[1, 0] = m[2, 1] = m[1, 2] = m[0, 3] = 1   # first pixel (0, 3)
    m[0, 6] = m[0, 7] = m[0, 8] = m[0, 9] = 1   # first pixel (0, 6)
    assert f(m, "largest", 0)[0][0, 3] == 1 and f(m, "largest", 0)[0][0, 6] == 0
    # a diagonal line is one component: 8-, not 4-connectivity
    d = np.eye(9, dtype=np.uint8)
    out, st = f(d, "largest", 0)
    assert np.array_equal(out, d) and st.tolist() == [1, 1, 9, 0]
    assert f(checkerboard(8, 8))[1][0] == 1
    # min_area equal to an area keeps it, area + 1 removes it
    m = np.zeros((8, 8), np.uint8)
    m[0:3, 0:3] = 1
    m[6, 6] = 1
    assert f(m, "all", 9)[1].tolist() == [2, 1, 9, 1] and f(m, "all", 10)[1].tolist() == [2, 0, 0, 10]
    assert f(m, "largest", 10)[0].sum() == 0 and f(m, "all", 1)[1].tolist() == [2, 2, 10, 0]
    # empty and full
    z = np.zeros((5, 7), np.uint8)
    assert f(z, "largest", 0)[0].sum() == 0 and f(z, "largest", 0)[1].tolist() == [0, 0, 0, 0]
    o = np.ones((5, 7), np.uint8)
    assert np.array_equal(f(o, "largest", 35)[0], o) and f(o, "largest", 36)[1].tolist() == [1, 0, 0, 35]
    # byte values are kept
    for v in (1, 255):
        mv = random_mask(16, 16, 0.3, seed=1, value=v)
        assert set(np.unique(f(mv, "largest", 0)[0])) == {0, v}
    # the identity setting returns the input (a copy of it), with the counts
    r = random_mask(16, 16, 0.3, seed=2, value=200)
    out, st = f(r)
    assert np.array_equal(out, r) and st[0] == st[1] and st[2] == (r > 0).sum() and st[3] == 0
    for bad in (dict(keep="biggest"), dict(min_area=-1), dict(keep=None), dict(min_area=1.5)):
        with pytest.raises(ValueError):
            f(r, **bad)
    with pytest.raises(ValueError):
        f(r.astype(np.int32), "largest", 0)


@pytest.mark.parametrize("seed", [0, 2, 5])
def test_planted_blob_is_removed_and_the_curvature_restored(seed):
    sc = make_scene(seed)
    one = np.ones((3, 3), np.int8)
    from scipy import ndimage
    assert ndimage.label(sc.mask > 0, structure=one)[1] == 1
    clean = resize_nearest((sc.mask > 0).astype(np.uint8), (256, 256))
    assert filter_components_reference(clean)[1][0] == 1
    dirty = clean.copy()
    ys, xs = np.nonzero(clean)
    y0 = 2 if ys.mean() >= 128 else 248  # the corner away from the actuator
    x0 = 2 if xs.mean() >= 128 else 248
    dirty[y0:y0 + 6, x0:x0 + 6] = 1
    assert filter_components_reference(dirty)[1][0] == 2

    def curv(m256):
        return compute_curvature_profile(resize_nearest(m256, (640, 480)), sc.depth, DEFAULT_K, 0.001, device="cpu")

    c0, c1 = curv(clean), curv(dirty)
    assert c0.status == "ok"
    assert (c1.status, c1.mean_curvature, c1.max_curvature) != (c0.status, c0.mean_curvature, c0.max_curvature)
    for keep, min_area in (("largest", 0), ("all", 64)):
        fixed, st = filter_components_reference(dirty, keep, min_area)
        assert np.array_equal(fixed, clean) and st.tolist() == [2, 1, int(clean.sum()), 36]
        c2 = curv(fixed)
        assert (c2.status, c2.mean_curvature, c2.max_curvature, c2.n_points) == (
            c0.status, c0.mean_curvature, c0.max_curvature, c0.n_points)


def test_serve_config(monkeypatch):
    cfg = ServeConfig()
    assert cfg.mask_components == "all" and cfg.mask_min_area == 0
    monkeypatch.setenv("RDP_SERVE_MASK_COMPONENTS", "largest")
    monkeypatch.setenv("RDP_SERVE_MASK_MIN_AREA", "32")
    cfg = apply_env(ServeConfig(), "serve")
    assert cfg.mask_components == "largest" and cfg.mask_min_area == 32 and isinstance(cfg.mask_min_area, int)
    p = argparse.ArgumentParser()
    add_dataclass_args(p, ServeConfig())
    cfg = from_args(ServeConfig, p.parse_args(["--mask-components", "largest", "--mask-min-area", "32"]))
    assert cfg.mask_components == "largest" and cfg.mask_min_area == 32
    cfg = from_args(ServeConfig, p.parse_args([]))
    assert cfg.mask_components == "all" and cfg.mask_min_area == 0


def test_cli_serve_options(monkeypatch):
    from robotic_discovery_platform_amd import cli
    args = cli.build_parser().parse_args(["serve", "--mask-components", "largest", "--mask-min-area", "32"])
    cfg = cli._cfg_from(ServeConfig, args, "serve")
    assert cfg.mask_components == "largest" and cfg.mask_min_area == 32
    monkeypatch.setenv("RDP_SERVE_MASK_MIN_AREA", "48")  # the environment sets the default, the flag wins
    cfg = cli._cfg_from(ServeConfig, cli.build_parser().parse_args(["serve", "--mask-components", "largest"]), "serve")
    assert cfg.mask_components == "largest" and cfg.mask_min_area == 48


class FixedSegmenter(nn.Module):
    """+-8 logits from a fixed model-resolution mask."""

    def __init__(self, m):
        super().__init__()
        self.register_buffer("m", torch.from_numpy(m.astype(np.float32)))
        self.p = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return (self.m * 16 - 8)[None, None].expand(x.shape[0], 1, -1, -1)


def test_bad_values_raise_when_the_pipeline_is_built():
    seg = FixedSegmenter(np.zeros((256, 256), np.uint8))
    for bad in (dict(mask_components="biggest"), dict(mask_min_area=-1), dict(mask_components="")):
        with pytest.raises(ValueError):
            CpuFramePipeline(seg, DEFAULT_K, 0.001, **bad)
        with pytest.raises(ValueError):
            EnginePool(seg, DEFAULT_K, 0.001, n=1, **bad)


def test_default_pipeline_has_no_filter():
    seg = FixedSegmenter(np.zeros((256, 256), np.uint8))
    assert CpuFramePipeline(seg, DEFAULT_K, 0.001).mask_filter is None
    assert CpuFramePipeline(seg, DEFAULT_K, 0.001, mask_components="all", mask_min_area=0).mask_filter is None
    pool = EnginePool(seg, DEFAULT_K, 0.001, n=1)
    assert pool.mask_filter is None and pool._get(0, 480, 640).queue[0].mask_filter is None


@pytest.mark.parametrize("keep,min_area", [("largest", 0), ("all", 64), ("largest", 5000)])
def test_cpu_pipeline_serves_the_filtered_mask(keep, min_area):
    sc = make_scene(2)
    m256 = resize_nearest((sc.mask > 0).astype(np.uint8), (256, 256))
    m256[248:254, 2:8] = 1
    m256[2:8, 248:254] = 1
    m256[2:5, 2:5] = 1
    seg = FixedSegmenter(m256)
    plain = CpuFramePipeline(seg, DEFAULT_K, 0.001)
    r0 = plain.process(sc.color, sc.depth)
    assert np.array_equal(plain.m_model, m256) and filter_components_reference(plain.m_model)[1][0] >= 3
    pipe = CpuFramePipeline(seg, DEFAULT_K, 0.001, mask_components=keep, mask_min_area=min_area)
    assert pipe.mask_filter == (keep, min_area)
    r = pipe.process(sc.color, sc.depth)
    want256, wst = filter_components_reference(plain.m_model, keep, min_area)
    full = resize_nearest(want256, (640, 480))
    assert np.array_equal(r.mask, full) and np.array_equal(pipe.stats, wst)
    assert r.coverage == pytest.approx(100.0 * np.count_nonzero(full) / full.size)
    exp = compute_curvature_profile(full, sc.depth, DEFAULT_K, 0.001, device="cpu")
    assert (r.curvature.status, r.curvature.mean_curvature, r.curvature.max_curvature) == (
        exp.status, exp.mean_curvature, exp.max_curvature)
    if min_area < 5000:
        assert not np.array_equal(r.mask, r0.mask)
    else:
        assert r.mask.sum() == 0  # nothing survives: an empty mask, as the definition says
    # the pool hands the options to the pipelines it builds
    pool = EnginePool(seg, DEFAULT_K, 0.001, n=1, mask_components=keep, mask_min_area=min_area)
    assert pool.mask_filter == (keep, min_area) and pool.args["mask_components"] == keep
    assert np.array_equal(pool.process(sc.color, sc.depth).mask, full)
