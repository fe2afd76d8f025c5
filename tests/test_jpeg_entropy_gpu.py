"""The GPU entropy decoder of marker-less baseline scans (csrc/jpeg_entropy.hip): coefficient planes bit for
bit those of the serial host decoder, the same statistics as its CPU emulation, the same verdict on
corrupt scans, and -- wired into the frame graph -- the same mask, result vector and response bytes as the
host entropy decode."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from robotic_discovery_platform_amd.data.jpeg import decode_coefs, entropy_decode, scan_jpeg
from robotic_discovery_platform_amd.ops import native

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(native(build_if_missing=False) is None, reason="native extension not built")]

SUBSEQ = [64, 128, 0]


def _frame(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 3) % 256], -1)
    return np.clip(base + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)


def _jpeg(rgb, **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb, "L" if rgb.ndim == 2 else "RGB").save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _scan_region(data):
    i = data.index(b"\xff\xda")
    ln = (data[i + 2] << 8) | data[i + 3]
    return i + 2 + ln, len(data) - 2


def _gpu_decode(js, subseq_bits, capacity=None, stale=0xA5):
    """(coefs on the host | None when corrupt, (subsequences, rounds)). The output is pre-filled with
    garbage (the kernels must zero it); ``capacity``: a scan buffer of that many bytes whose tail after
    the frame's bits holds stale bytes."""
    C = native()
    dev = torch.device("cuda")
    n = js.blocks * 64
    nbytes = js.scan.numel()
    cap = nbytes if capacity is None else capacity
    scan = torch.full((cap,), stale, dtype=torch.uint8, device=dev)
    used = (js.nbits + 7) // 8
    scan[:used] = js.scan[:used].to(dev)
    coefs = torch.full((n,), 0x5A5A, dtype=torch.int16, device=dev)
    work = torch.empty(C.jpeg_entropy_work_words(cap, subseq_bits), dtype=torch.int32, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    st = C.jpeg_entropy_gpu(scan, js.nbits, js.tables.to(dev), js.meta[:32].to(dev), coefs, work, status, subseq_bits)
    torch.cuda.synchronize()
    s = int(status.item())
    assert s in (0, 1)
    return (coefs.cpu() if s == 0 else None), tuple(st)


def _check(data, subseq_bits, capacity=None):
    want = decode_coefs(data, parallel=False)
    js = scan_jpeg(data)
    assert want is not None and js is not None
    emu = []
    assert entropy_decode(js, subseq_bits=subseq_bits, stats=emu) is not None
    got, st = _gpu_decode(js, subseq_bits, capacity)
    assert got is not None
    assert torch.equal(got, want.coefs)
    assert st == tuple(emu)


@pytest.mark.parametrize("subseq_bits", SUBSEQ)
@pytest.mark.parametrize("subsampling", [0, 1, 2])
@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (48, 80), (1, 9)])
def test_gpu_equals_host_decode(hw, subsampling, subseq_bits):
    _check(_jpeg(_frame(*hw, seed=hw[0] + subsampling), quality=90, subsampling=subsampling), subseq_bits)


@pytest.mark.parametrize("subseq_bits", SUBSEQ)
def test_grayscale(subseq_bits):
    _check(_jpeg(_frame(37, 53, 5)[..., 0].copy(), quality=90), subseq_bits)


@pytest.mark.parametrize("subseq_bits", SUBSEQ)
@pytest.mark.parametrize("quality,subsampling", [(30, 2), (100, 2), (100, 0)])
def test_quality_range(quality, subsampling, subseq_bits):
    # 48x80 q100 4:4:4 at 64 bits: ~1,450 subsequences, two workgroups and a stitched boundary
    _check(_jpeg(_frame(48, 80, quality), quality=quality, subsampling=subsampling), subseq_bits)


@pytest.mark.parametrize("subseq_bits", SUBSEQ)
def test_optimized_tables(subseq_bits):
    _check(_jpeg(_frame(48, 80, 7), quality=90, subsampling=2, optimize=True), subseq_bits)


def test_entropy_decode_on_the_gpu_matches():
    data = _jpeg(_frame(48, 80, 3), quality=90, subsampling=2)
    want = decode_coefs(data, parallel=False)
    got = entropy_decode(scan_jpeg(data), device="cuda")
    assert got.coefs.is_cuda and torch.equal(got.coefs.cpu(), want.coefs) and torch.equal(got.meta.cpu(), want.meta)


@pytest.mark.parametrize("subseq_bits", [64, 0])
def test_capacity_sized_buffer_with_stale_tail(subseq_bits):
    """The grids come from the buffer's capacity (here several workgroups of idle lanes at 64 bits) and the
    bytes after the frame's bits are another frame's leftovers."""
    _check(_jpeg(_frame(37, 53, 6), quality=90, subsampling=2), subseq_bits, capacity=24 * 1024)


def test_truncated_scan():
    data = _jpeg(_frame(37, 53, 3), quality=90, subsampling=2)
    b, e = _scan_region(data)
    cut = data[: b + (e - b) * 2 // 3]
    want = decode_coefs(cut, parallel=False)
    got, _ = _gpu_decode(scan_jpeg(cut), 64)
    assert (want is None) == (got is None)
    if want is not None:
        assert torch.equal(got, want.coefs)


def test_corrupt_verdict_equals_host_and_emulation():
    """Verdict equality on eight byte-flip mutants; each goes through the emulation (the same per-lane
    code, whose memory safety the sanitizer build covers) before it is launched."""
    data = _jpeg(_frame(37, 53, 4), quality=90, subsampling=2)
    b, e = _scan_region(data)
    rng = np.random.default_rng(11)
    for _ in range(8):
        m = bytearray(data)
        for i in rng.integers(b, e, 3):
            m[int(i)] = int(rng.integers(0, 256))
        m = bytes(m)
        want = decode_coefs(m, parallel=False)
        js = scan_jpeg(m)
        emu = []
        ref = entropy_decode(js, subseq_bits=64, stats=emu)
        assert (ref is None) == (want is None)
        got, st = _gpu_decode(js, 64)
        assert (got is None) == (want is None) and st == tuple(emu)
        if want is not None:
            assert torch.equal(got, want.coefs)


def test_entropy_plus_pixel_stage_equals_pil():
    C = native()
    data = _jpeg(_frame(48, 80, 2), quality=90, subsampling=2)
    jc = entropy_decode(scan_jpeg(data), device="cuda")
    H, W = 48, 80
    coefs = torch.zeros(C.jpeg_max_coefs(H, W), dtype=torch.int16, device="cuda")
    coefs[:jc.coefs.numel()] = jc.coefs
    planes = torch.empty(C.jpeg_plane_bytes(H, W), dtype=torch.uint8, device="cuda")
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")
    C.jpeg_to_rgb(coefs, jc.meta[:32].contiguous(), jc.meta[32:].contiguous(), planes, rgb)
    np.testing.assert_array_equal(rgb.cpu().numpy(), _pil(data))


# ------------------------------------------------------------------ the frame graph and the encoded-request path
@pytest.fixture(scope="module")
def pipeline():
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K
    from robotic_discovery_platform_amd.models.unet import UNetNative
    from robotic_discovery_platform_amd.serve.engine import SRC_SCAN, FramePipeline
    torch.manual_seed(0)
    nat = UNetNative(3, 1, device=torch.device("cuda")).eval()
    with torch.no_grad():
        nat.store.view("outc.conv.bias").fill_(0.0)
    p = FramePipeline(nat, DEFAULT_K, 0.001, graph=True, rgb=True, jpeg=True)
    assert SRC_SCAN in p.graphs  # captured at build, not on the first request
    return p


def _scene_request(seed):
    """(colour JPEG as a stock client sends it: q95 4:2:0, no restart markers; one-stream 16-bit depth PNG; depth)"""
    from robotic_discovery_platform_amd.data.image_io import encode_jpeg, encode_png
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    sc = make_scene(seed)
    return encode_jpeg(sc.color, 95, restart_rows=0), encode_png(sc.depth), sc.depth


def _encoded(p, policy, color, depth):
    """(response fields that do not carry a time, mask, result vector) of one frame through submit_encoded"""
    from robotic_discovery_platform_amd.serve.engine import WireResult
    p.set_jpeg_entropy(policy)
    assert p.submit_encoded(color, depth) == 0
    r = p.collect_encoded()
    assert isinstance(r, WireResult)
    return (r.mean_curvature, r.max_curvature, r.coverage), p.h_mask.numpy().copy(), p.h_res.numpy().copy()


def test_frame_graph_scan_source_equals_host_entropy(pipeline):
    """Two different marker-less frames through the one captured graph, as a JpegScan and through
    submit_encoded under jpeg_entropy=gpu: mask and result vector bitwise those of jpeg_entropy=host."""
    p = pipeline
    for seed in (2, 5):
        color, depth_png, depth = _scene_request(seed)
        assert scan_jpeg(color) is not None and b"\xff\xd0" not in color[:700]
        fh, mh, rh = _encoded(p, "host", color, depth_png)
        assert p.runner.scan_status() == 0
        fg, mg, rg = _encoded(p, "gpu", color, depth_png)
        assert np.array_equal(mg, mh) and np.array_equal(rg, rh) and fg == fh
        p.submit(scan_jpeg(color, pin=True), depth)
        rs = p.collect()
        assert np.array_equal(rs.mask, mh) and np.array_equal(p.h_res.numpy(), rh)
        p.submit(decode_coefs(color, pin=True), depth)  # the host-decoded coefficients, same pipeline
        rc = p.collect()
        assert np.array_equal(rc.mask, mh) and rc.coverage == rs.coverage
    p.set_jpeg_entropy("host")


def test_restart_marker_stream_keeps_the_host_path(pipeline):
    from robotic_discovery_platform_amd.data.image_io import encode_jpeg
    from robotic_discovery_platform_amd.data.synthetic import make_scene
    p = pipeline
    color, depth_png, depth = _scene_request(3)
    marked = encode_jpeg(make_scene(3).color, 95, restart_rows=1)
    fh, mh, rh = _encoded(p, "host", marked, depth_png)
    fg, mg, rg = _encoded(p, "auto", marked, depth_png)
    assert p.runner.scan_status() == 0 and np.array_equal(mg, mh) and np.array_equal(rg, rh) and fg == fh
    p.set_jpeg_entropy("host")


def _corrupt(color):
    """A scan the entropy decoders call corrupt (the headers stay intact)"""
    b, e = _scan_region(color)
    rng = np.random.default_rng(5)
    for _ in range(64):
        m = bytearray(color)
        for i in rng.integers(b + (e - b) // 4, e, 6):
            m[int(i)] = int(rng.integers(0, 256))
        m = bytes(m)
        js = scan_jpeg(m)
        if js is not None and decode_coefs(m, parallel=False) is None:
            assert entropy_decode(js) is None  # the emulation's verdict before anything is launched
            return m
    raise AssertionError("no corrupt mutant found")


def test_corrupt_scan_gets_the_host_paths_response(pipeline):
    """Under jpeg_entropy=host a corrupt scan is refused at submit (code 3) and the caller decodes the frame
    itself; under gpu the corruption shows at collect and the session does the same: one response."""
    import queue
    from robotic_discovery_platform_amd.serve.engine import CorruptScan, EngineSession
    p = pipeline
    color, depth_png, depth = _scene_request(2)
    bad = _corrupt(color)
    p.set_jpeg_entropy("host")
    assert p.submit_encoded(bad, depth_png) == 3

    class _Pool:  # what EngineSession needs of a pool: one pipeline of the configured size
        home_size = (p.H, p.W)

        def __init__(self):
            self.q = queue.Queue()
            self.q.put(p)

        def _batcher(self, *a):
            return None

        def _get(self, *a):
            return self.q

    out = {}
    for policy in ("host", "gpu"):
        p.set_jpeg_entropy(policy)
        sess = EngineSession(_Pool(), 0)
        done, code = sess.submit_encoded(bad, depth_png, tag=0)
        assert done == [] and code == (3 if policy == "host" else 0)
        if code:  # today's handling of code 3: decode here, submit as an array
            c, d = sess.decoder(bad, depth_png)
            done = sess.submit(c, d, tag=0, rgb=True)
        (tag, r), = done + sess.drain()
        assert tag == 0 and not isinstance(r, Exception), r
        out[policy] = r
    h, g = out["host"], out["gpu"]
    assert np.array_equal(h.mask, g.mask) and h.coverage == g.coverage
    assert h.curvature.status == g.curvature.status and h.curvature.mean_curvature == g.curvature.mean_curvature
    # and the pipeline's own API raises at collect
    p.submit(scan_jpeg(bad, pin=True), depth)
    with pytest.raises(CorruptScan):
        p.collect()
    p.set_jpeg_entropy("host")
    p.submit(decode_coefs(color, pin=True), depth)  # the pipeline goes on
    assert p.collect().mask.shape == (p.H, p.W)


def test_eager_pipeline_takes_a_scan(pipeline):
    """The program outside a graph (no native runner): uploads by torch copies, status read at collect."""
    from robotic_discovery_platform_amd.data.synthetic import DEFAULT_K
    from robotic_discovery_platform_amd.serve.engine import CorruptScan, FramePipeline
    pe = FramePipeline(pipeline.model, DEFAULT_K, 0.001, graph=False)
    color, _, depth = _scene_request(5)
    pe.submit(scan_jpeg(color, pin=True), depth)
    a = pe.collect()
    pe.submit(decode_coefs(color, pin=True), depth)
    b = pe.collect()
    assert np.array_equal(a.mask, b.mask) and a.coverage == b.coverage
    pe.submit(scan_jpeg(_corrupt(color), pin=True), depth)
    with pytest.raises(CorruptScan):
        pe.collect()
