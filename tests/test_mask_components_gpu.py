"""The on-device mask component filter (csrc/mask_components.hip) against its definition
(geometry/components.py filter_components_reference), bit for bit, and through the serving pipelines."""
import numpy as np
import pytest
import torch

from mask_component_cases import DENSITIES, random_mask, structures

from robotic_discovery_platform_amd.geometry.components import filter_components, filter_components_reference

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 64), (64, 1), (3, 5), (37, 53), (64, 96), (255, 257), (256, 256)]


@pytest.fixture(scope="module")
def C():
    from robotic_discovery_platform_amd.ops import native
    return native(build_if_missing=False)


def _dev():
    return torch.device("cuda")


def _run(C, masks, keep, min_area):
    """The kernel on a batch of equal-size masks: (filtered [n, H, W] on the host, stats [n, 4])."""
    n, (H, W) = len(masks), masks[0].shape
    d = torch.from_numpy(np.stack(masks)).to(_dev())
    st = torch.full((n, 4), -7, dtype=torch.int32, device=_dev())
    C.mask_components(d, n, H, W, int(keep == "largest"), min_area, st)
    return d.cpu(), st.cpu()


def _check(C, masks, keep, min_area):
    got, st = _run(C, masks, keep, min_area)
    for j, m in enumerate(masks):
        want, wst = filter_components_reference(m, keep, min_area)
        assert torch.equal(got[j], torch.from_numpy(want)), (keep, min_area, j)
        assert torch.equal(st[j], torch.from_numpy(wst)), (keep, min_area, j, st[j], wst)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("density", DENSITIES)
def test_random_masks(C, H, W, density):
    m = random_mask(H, W, density)
    above = int(filter_components_reference(m, "largest", 0)[1][2]) + 1  # above the largest area
    for keep in ("all", "largest"):
        for min_area in (0, 1, 2, 9, above):
            _check(C, [m], keep, min_area)


@pytest.mark.parametrize("case", structures(), ids=lambda c: c[0])
def test_structures(C, case):
    name, m, ncomp = case
    assert int(filter_components_reference(m)[1][0]) == ncomp
    for keep, min_area in (("largest", 0), ("all", 2), ("largest", 7), ("all", 0)):
        _check(C, [m], keep, min_area)
    if name == "singletons":
        got, st = _run(C, [m], "largest", 0)
        assert int(got.sum()) == 1 and int(got[0, 0, 0]) == 1 and st[0].tolist() == [16384, 1, 1, 16383]
    if name == "double_spiral":  # equal areas: the arm whose first pixel comes first stays
        got, _ = _run(C, [m], "largest", 0)
        first = int(np.flatnonzero(m.ravel())[0])
        assert int(got.reshape(-1)[first]) == 1 and int(got.sum()) * 2 == int(m.sum())


def test_byte_values_are_kept(C):
    for value in (1, 255, 37):
        m = random_mask(64, 96, 0.3, seed=3, value=value)
        _check(C, [m], "largest", 0)
        _check(C, [m], "all", 3)
        got, _ = _run(C, [m], "largest", 0)
        assert set(np.unique(got.numpy())) == {0, value}


def test_empty_and_full(C):
    for H, W in ((256, 256), (37, 53), (1, 1)):
        _check(C, [np.zeros((H, W), np.uint8)], "largest", 0)
        _check(C, [np.ones((H, W), np.uint8)], "largest", 0)
        _check(C, [np.ones((H, W), np.uint8)], "all", H * W)
        _check(C, [np.ones((H, W), np.uint8)], "all", H * W + 1)


def test_batch_frames_are_independent(C):
    masks = [random_mask(256, 256, d, seed=5) for d in (0.05, 0.3, 0.41, 0.9)]
    _check(C, masks, "largest", 0)
    _check(C, masks, "all", 9)
    a, sa = _run(C, masks, "largest", 4)
    swapped = [masks[2], masks[1], masks[0], masks[3]]
    b, sb = _run(C, swapped, "largest", 4)
    assert torch.equal(a[0], b[2]) and torch.equal(a[2], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(sa[0], sb[2]) and torch.equal(sa[2], sb[0])
    # odd frame size: every second frame starts at an odd address
    _check(C, [random_mask(37, 53, d, seed=6) for d in (0.3, 0.41, 0.9, 0.05)], "largest", 0)


def test_same_buffers_three_masks_and_graph_replay(C):
    """No state survives a launch: the same buffers on new masks, eagerly and as a replayed graph."""
    masks = [random_mask(256, 256, 0.41, seed=11), structures()[0][1], random_mask(256, 256, 0.05, seed=12),
             np.ones((256, 256), np.uint8)]
    dev = _dev()
    buf = torch.zeros(256, 256, dtype=torch.uint8, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    for m in masks:
        buf.copy_(torch.from_numpy(m))
        C.mask_components(buf, 1, 256, 256, 1, 5, st)
        want, wst = filter_components_reference(m, "largest", 5)
        assert torch.equal(buf.cpu(), torch.from_numpy(want)) and torch.equal(st.cpu(), torch.from_numpy(wst))
    s = torch.cuda.Stream()
    src = torch.zeros(256, 256, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(s):
        buf.copy_(src)
        C.mask_components(buf, 1, 256, 256, 1, 5, st)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        buf.copy_(src)
        C.mask_components(buf, 1, 256, 256, 1, 5, st)
    for m in masks:
        src.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, wst = filter_components_reference(m, "largest", 5)
        assert torch.equal(buf.cpu(), torch.from_numpy(want)) and torch.equal(st.cpu(), torch.from_numpy(wst))


@pytest.mark.parametrize("H,W,n", [(37, 53, 3), (256, 256, 2), (255, 257, 1)])
def test_guard_bytes(C, H, W, n):
    dev = _dev()
    pad = 4099  # odd: the masks start at an odd address
    big = torch.full((pad + n * H * W + pad,), 0xAB, dtype=torch.uint8, device=dev)
    masks = [random_mask(H, W, 0.41, seed=20 + j) for j in range(n)]
    view = big[pad:pad + n * H * W]
    view.copy_(torch.from_numpy(np.stack(masks)).reshape(-1))
    stbig = torch.full((8 + 4 * n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    C.mask_components(view, n, H, W, 1, 2, stbig[8:8 + 4 * n])
    out = big.cpu()
    assert (out[:pad] == 0xAB).all() and (out[pad + n * H * W:] == 0xAB).all()
    sto = stbig.cpu()
    assert (sto[:8] == 0x5A5A5A5A).all() and (sto[8 + 4 * n:] == 0x5A5A5A5A).all()
    for j, m in enumerate(masks):
        want, wst = filter_components_reference(m, "largest", 2)
        assert torch.equal(out[pad + j * H * W:pad + (j + 1) * H * W].view(H, W), torch.from_numpy(want))
        assert torch.equal(sto[8 + 4 * j:12 + 4 * j], torch.from_numpy(wst))


def test_two_runs_are_bitwise_equal(C):
    masks = [random_mask(256, 256, 0.41, seed=31), random_mask(256, 256, 0.3, seed=32)]
    a, sa = _run(C, masks, "largest", 3)
    b, sb = _run(C, masks, "largest", 3)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_refusals_leave_the_mask_untouched(C):
    dev = _dev()
    sent = torch.full((65537,), 1, dtype=torch.uint8, device=dev)
    st = torch.zeros(16, dtype=torch.int32, device=dev)

    def refused(*args):
        with pytest.raises(ValueError):
            C.mask_components(*args)
        torch.cuda.synchronize()
        assert bool((sent == 1).all())

    refused(sent, 1, 1, 65537, 1, 0, st)                       # H * W = 65,537
    refused(sent, 1, 65537, 1, 1, 0, st)
    refused(sent, 0, 16, 16, 1, 0, st)                         # n = 0
    refused(sent, 1, 0, 16, 1, 0, st)
    refused(sent, 1, 16, 16, 1, -1, st)                        # negative min_area
    refused(sent, 1, 256, 257, 1, 0, st)                       # 65,792 pixels
    refused(sent[:256], 2, 16, 16, 1, 0, st)                   # mask too short for n frames
    refused(sent[:1024].view(32, 32)[:, :16], 1, 32, 16, 1, 0, st)   # non-contiguous
    refused(sent[:256], 1, 16, 16, 1, 0, st[:3])               # stats too short
    refused(sent[:256], 1, 16, 16, 1, 0, st[:8].float())       # stats not int32
    refused(sent[:256], 1, 16, 16, 1, 0, st[:8].cpu())         # stats on the wrong device
    f32 = torch.ones(256, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):                            # a non-u8 tensor
        C.mask_components(f32, 1, 16, 16, 1, 0, st)
    cpu = torch.ones(256, dtype=torch.uint8)
    with pytest.raises(ValueError):                            # a tensor on the wrong device
        C.mask_components(cpu, 1, 16, 16, 1, 0, None)
    torch.cuda.synchronize()
    assert bool((f32 == 1).all()) and bool((cpu == 1).all())
    # the wrapper refuses bad options itself, and launches nothing for the identity setting
    with pytest.raises(ValueError):
        filter_components(sent[:256].view(16, 16), "biggest", 0)
    with pytest.raises(ValueError):
        filter_components(sent[:256].view(16, 16), "all", -1)


def test_wrapper(C, monkeypatch):
    m = random_mask(64, 96, 0.41, seed=40)
    d = torch.from_numpy(m).to(_dev())
    st = torch.zeros(4, dtype=torch.int32, device=_dev())
    assert filter_components(d, "largest", 3, st) is d
    want, wst = filter_components_reference(m, "largest", 3)
    assert torch.equal(d.cpu(), torch.from_numpy(want)) and torch.equal(st.cpu(), torch.from_numpy(wst))
    d3 = torch.from_numpy(np.stack([m, m[::-1].copy()])).to(_dev())
    filter_components(d3, "all", 4)
    assert torch.equal(d3[1].cpu(), torch.from_numpy(filter_components_reference(m[::-1].copy(), "all", 4)[0]))

    def boom(*a, **k):
        raise AssertionError("the identity setting must not launch")

    monkeypatch.setattr(C, "mask_components", boom)
    d2 = torch.from_numpy(m).to(_dev())
    assert filter_components(d2, "all", 0) is d2 and torch.equal(d2.cpu(), torch.from_numpy(m))


# ---------------------------------------------------------------------------------------------- serving pipelines
@pytest.fixture(scope="module")
def models():
    """The random-init one-class model of test_serve_gpu.py (zero head bias) and a K = 3 model. The seeds are the
    first whose masks have many components and a fit that succeeds (one-class: ~750 components, the largest ~780
    pixels; K = 3, class 1: ~20 components, the largest ~510 pixels); seed 0 gives a one-pixel mask."""
    from robotic_discovery_platform_amd.models.unet import UNetNative
    out = {}
    for k, seed in ((1, 2), (3, 3)):
        torch.manual_seed(seed)
        nat = UNetNative(3, k, device=_dev()).eval()
        with torch.no_grad():
            nat.store.view("outc.conv.bias").fill_(0.0)
        out[k] = nat
    return out


def _pipeline_case(models, k):
    return models[k], (dict(mask_class=1) if k > 1 else {})


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("k", [1, 3], ids=["one_class", "three_class"])
@pytest.mark.parametrize("keep,min_area", [("largest", 0), ("all", 12)])
def test_frame_pipeline_serves_the_filtered_mask(models, k, graph, keep, min_area):
    from robotic_discovery_platform_amd.data.image_io import resize_nearest
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.geometry import reference as gref
    from robotic_discovery_platform_amd.serve.engine import FramePipeline
    nat, extra = _pipeline_case(models, k)
    off = FramePipeline(nat, DEFAULT_K, 0.001, graph=graph, **extra)
    on = FramePipeline(nat, DEFAULT_K, 0.001, graph=graph, mask_components=keep, mask_min_area=min_area, **extra)
    assert off.mask_filter is None and not hasattr(off, "stats") and on.mask_filter == (keep, min_area)
    for seed in (2, 5):  # the second frame goes through the same graph and buffers
        sc = make_scene(seed)
        off.process(sc.color, sc.depth)
        raw = off.m256.view(256, 256).cpu().numpy().copy()  # the unfiltered model-resolution mask
        assert int(filter_components_reference(raw)[1][0]) >= 2
        want256, wst = filter_components_reference(raw, keep, min_area)
        assert not np.array_equal(want256, raw)
        r = on.process(sc.color, sc.depth)
        assert torch.equal(on.m256.view(256, 256).cpu(), torch.from_numpy(want256))
        assert torch.equal(on.stats.cpu(), torch.from_numpy(wst))
        full = resize_nearest(want256, (640, 480))
        assert (full == r.mask).mean() > 0.999
        assert r.coverage == pytest.approx(100.0 * r.mask.sum() / r.mask.size)
        assert r.coverage == pytest.approx(100.0 * np.count_nonzero(full) / full.size, abs=0.1)
        x = gref.compute_curvature_profile(full, sc.depth, DEFAULT_K, 0.001)
        assert r.curvature.status == x.status
        assert r.curvature.mean_curvature == pytest.approx(x.mean_curvature, rel=1e-7, abs=1e-12)
        assert r.curvature.max_curvature == pytest.approx(x.max_curvature, rel=1e-7, abs=1e-12)


def test_filter_at_the_start_of_the_geometry_graph(models, monkeypatch):
    """RDP_SERVE_MASK_FILTER_AT=geo (the measured alternative placement) serves the same frame."""
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.serve.engine import FramePipeline
    sc = make_scene(2)
    a = FramePipeline(models[1], DEFAULT_K, 0.001, graph=True, mask_components="largest")
    monkeypatch.setenv("RDP_SERVE_MASK_FILTER_AT", "geo")
    b = FramePipeline(models[1], DEFAULT_K, 0.001, graph=True, mask_components="largest")
    ra, rb = a.process(sc.color, sc.depth), b.process(sc.color, sc.depth)
    assert not a.filter_at_geo and b.filter_at_geo
    assert torch.equal(a.m256, b.m256) and np.array_equal(ra.mask, rb.mask) and torch.equal(a.stats, b.stats)
    assert ra.curvature.mean_curvature == rb.curvature.mean_curvature


def test_bad_options_and_oversize_models_raise_at_build(models):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K
    from robotic_discovery_platform_amd.serve.engine import SRC_BGR, BatchEngine, EnginePool, FramePipeline
    for bad in (dict(mask_components="biggest"), dict(mask_min_area=-1), dict(mask_components="largest", size=272)):
        with pytest.raises(ValueError):
            FramePipeline(models[1], DEFAULT_K, 0.001, graph=False, **bad)
        with pytest.raises(ValueError):
            BatchEngine(models[1], DEFAULT_K, 0.001, src=SRC_BGR, positions=2, frames=1, **bad)
        with pytest.raises(ValueError):
            EnginePool(models[1], DEFAULT_K, 0.001, n=1, graph=False, batch=0, **bad)


def _batch_frames(be, scenes):
    pos = [be._acquire() for _ in scenes]  # hold the launcher until every frame is staged: ONE batch
    tickets = [be.submit(sc.color, sc.depth, pos=p) for sc, p in zip(scenes, pos)]
    return [be.collect(t) for t in tickets]


def test_batch_engine_filters_each_position(models):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.serve.engine import SRC_BGR, BatchEngine, FramePipeline
    nat = models[1]
    scenes = [make_scene(s) for s in (2, 5, 0, 3)]
    S2 = 256 * 256
    kw = dict(src=SRC_BGR, positions=4, frames=1, window_us=200000.0)
    off = BatchEngine(nat, DEFAULT_K, 0.001, **kw)
    on = BatchEngine(nat, DEFAULT_K, 0.001, mask_components="largest", mask_min_area=3, **kw)
    try:
        assert off.mask_filter is None and not hasattr(off, "stats") and on.mask_filter == ("largest", 3)
        _batch_frames(off, scenes)
        raw = off.m256[4].view(4, 256, 256).cpu().numpy().copy()
        got = _batch_frames(on, scenes)
        assert on.batch_sizes[4] >= 1
        m = on.m256[4].view(4, 256, 256).cpu()
        st = on.stats[4].cpu()
    finally:
        off.close()
        on.close()
    for j, sc in enumerate(scenes):
        assert int(filter_components_reference(raw[j])[1][0]) >= 2
        want, wst = filter_components_reference(raw[j], "largest", 3)
        assert torch.equal(m[j], torch.from_numpy(want)) and torch.equal(st[j], torch.from_numpy(wst))
    # the per-stream pipelines with the same options serve the same frames. The network's kernels are chosen per
    # batch size, so a batch-4 mask differs from the batch-1 mask in a few |logit| ~ 0 pixels before any filter:
    # the agreement asked is that of tests/test_serve_batch_gpu.py::test_batch_matches_single_frame_pipeline
    single = FramePipeline(nat, DEFAULT_K, 0.001, graph=True, mask_components="largest", mask_min_area=3)
    for j, sc in enumerate(scenes):
        r = single.process(sc.color, sc.depth)
        frac = float((r.mask == got[j].mask).mean())
        print(f"position {j}: batch / per-stream mask agreement {frac:.6f}, "
              f"differing model pixels {int((single.m256.view(256, 256).cpu() != m[j]).sum())}")
        assert frac > 0.999, frac
        assert r.curvature.status == got[j].curvature.status
        assert abs(r.coverage - got[j].coverage) < 0.1


def test_engine_pool_carries_the_options(models):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.serve.engine import EnginePool
    pool = EnginePool(models[1], DEFAULT_K, 0.001, n=1, graph=True, batch=2, mask_components="all", mask_min_area=20)
    try:
        assert pool.mask_filter == ("all", 20) and pool.args["mask_min_area"] == 20
        pipes = list(pool._get(0, 480, 640).queue)
        assert pipes and all(p.mask_filter == ("all", 20) for p in pipes)
        assert pool.batchers and all(b.mask_filter == ("all", 20) for b in pool.batchers)
        assert pool._new(0, 120, 160).mask_filter == ("all", 20)  # a pipeline built later, for another frame size
        sc = make_scene(2)
        r = pool.process(sc.color, sc.depth)
        p = pipes[0]
        want = filter_components_reference(p.m256.view(256, 256).cpu().numpy(), "all", 20)
        assert np.array_equal(want[0], p.m256.view(256, 256).cpu().numpy())  # nothing below 20 pixels is left
        assert int(p.stats[0]) > int(p.stats[1]) >= 1 and r.mask.shape == sc.depth.shape
    finally:
        for b in pool.batchers:
            b.close()


def test_default_pipeline_never_calls_the_filter(models, monkeypatch):
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K, make_scene
    from robotic_discovery_platform_amd.ops import native
    from robotic_discovery_platform_amd.serve.engine import FramePipeline

    def boom(*a, **k):
        raise AssertionError("the default pipeline must not launch the component filter")

    monkeypatch.setattr(native(), "mask_components", boom)
    sc = make_scene(2)
    for graph in (True, False):
        p = FramePipeline(models[1], DEFAULT_K, 0.001, graph=graph)
        assert p.mask_filter is None and not hasattr(p, "stats")
        r = p.process(sc.color, sc.depth)
        assert r.mask.any()
